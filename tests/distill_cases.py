"""The inputs of test_distill_cpu.py and test_distill_gpu.py, and their float64 references (computed once).

Student and teacher logits are 3 * randn, seeded.  Every input carries these planted rows, in image 0, anchor 0, at the
cells (flattened row-major index) below:
  cell 0  S == T: the student's 5 + C logits are the teacher's (every difference exactly 0);
  cell 1  student sigmoid logits s0 = 30, s1 = -30, s4 = 30 (1 - sig(s) is 0 in float32, sig(-s) is 9.4e-14);
  cell 2  teacher sigmoid logits t0 = -30, t1 = 30 and a teacher objectness logit of 88 (exp(-88) is below the smallest
          normal float32, q = 1);
  cell 3  teacher class logits 60, -60, 0, 60, ... and teacher objectness 2: pt underflows to 0 for the -60 classes (at
          tau = 1: exp(-120)), whose log pt must stay finite;
  cell 4  student class logits spread evenly over [-30, 30] (30 alone for C = 1), teacher objectness 2;
  cell 5  all 2 * (5 + C) logits zero.
Every input but "b4" carries one more:
  cell 6  a student objectness logit of 88: exp(88) = 1.65e38 is just inside float32 and sig(-88) = 6e-39 below its
          smallest normal number.  "b4" is the input of the batch-independence test, which asserts that 1 / B scales a
          gradient exactly; a subnormal times a power of two is not exact, so that input leaves it out (it keeps the
          teacher-side 88 of cell 2).
"""
import functools

import torch

from distill_ref import distill_ref

# The tolerance of the per-element comparison on the device, in units of eps32 * scale (distill_ref.py).  The float32 torch
# restatement on the CPU is within YARDSTICK units of the float64 reference over every element of every input, scale set
# and temperature below (gradient; loss LOSS_YARDSTICK; printed by test_distill_cpu.py).  K = 4 x the larger, for the
# device's expf / logf and contraction against the CPU's libm, rounded up to a power of two.
YARDSTICK = 10.73            # measured: a1c80; the other inputs 2.63 - 10.37
LOSS_YARDSTICK = 0.44        # measured: 19x19
K = 64.0                     # 4 x 10.73 = 42.9
SCALES = {"s1_1_1": (1.0, 1.0, 1.0), "s1_2_05": (1.0, 2.0, 0.5)}         # (obj, box, cls)
TAUS = (1.0, 2.0, 4.0)

# name: (B, A, C, H, W, seed)
CASES = {
    "13x13": (1, 5, 20, 13, 13, 1),             # the workload's grid
    "b4": (4, 5, 20, 7, 10, 2),                 # image independence
    "a8c1": (2, 8, 1, 17, 16, 3),               # 8 anchors, 1 class; 272 cells: 16 threads on the second walk
    "a1c80": (1, 1, 80, 5, 3, 4),               # 1 anchor, 80 classes, fewer cells than a wave
    "19x19": (1, 5, 20, 19, 19, 5),             # 361 cells: H * W no multiple of 64, two walks per thread
}
SATURATED = ((1, (0, 1, 4)), (6, (4,)))       # (cell, student channels with a saturated sigmoid), see above


@functools.lru_cache(maxsize=None)
def make(name):
    """(student, teacher) [B, A*(5+C), H, W] float32 CPU tensors; do not modify them."""
    B, A, C, H, W, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    S = torch.randn(B, A * (5 + C), H, W, generator=g) * 3.0
    T = torch.randn(B, A * (5 + C), H, W, generator=g) * 3.0
    s = S.view(B, A, 5 + C, H * W)[0, 0]                      # [5 + C, cells] views of image 0, anchor 0
    t = T.view(B, A, 5 + C, H * W)[0, 0]
    s[:, 0] = t[:, 0]
    s[0, 1], s[1, 1], s[4, 1] = 30.0, -30.0, 30.0
    t[0, 2], t[1, 2], t[4, 2] = -30.0, 30.0, 88.0
    t[5:, 3] = torch.tensor([60.0, -60.0, 0.0]).repeat(C // 3 + 1)[:C]
    t[4, 3] = 2.0
    s[5:, 4] = torch.linspace(-30.0, 30.0, C) if C > 1 else torch.tensor([30.0])
    t[4, 4] = 2.0
    s[:, 5] = 0.0
    t[:, 5] = 0.0
    if name != "b4":
        s[4, 6] = 88.0
    return S, T


@functools.lru_cache(maxsize=None)
def reference(name, scales_name, tau):
    B, A, C, H, W, _ = CASES[name]
    S, T = make(name)
    return distill_ref(S.numpy(), T.numpy(), A, C, SCALES[scales_name], tau)


ALL = [(n, s, tau) for n in CASES for s in SCALES for tau in TAUS]
IDS = ["%s-%s-tau%g" % p for p in ALL]
