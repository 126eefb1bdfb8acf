"""The inputs of test_region_loss_cpu.py and test_region_loss_gpu.py, and their float64 references (computed once).

Every input mixes a full list of 50 boxes with no terminator (image 0), a six-box list with rows after its terminator
(image 1) and, where the batch allows, an image without boxes (image 2).  Image 0 ends with the edge rows, so that no later
box overwrites them:
  row 40  a copy of row 5's box with another class (the later one wins the cell),
  row 41  x == 1.0 and row 42 y == 1.0 (cell index clamped, tx / ty from the unclamped integer),
  row 43  w == 0 (no anchor IoU above 0: the last anchor),
  row 44  label C, row 45 label -1 (no class term), row 46 a non-integer label (truncates).
Image 1 starts with a box of 1.2 x the first anchor, and the logits at its cell predict exactly that box (an nCorrect hit);
the logits of the cell right of it predict nearly the same box (a silenced no-object cell).  A few width / height logits
of unassigned cells are 5.0 and 6.0: exp(exp(o)) is inf in float32, all IoUs of that prediction are NaN or 0.
Random width / height logits are capped at 4.0, away from that overflow (4.4855) and from assigned cells, where an
infinite box makes the reference's loss NaN.
"""
import functools
import math

import numpy as np
import torch

from region_loss_ref import region_loss_ref

BENCH_ANCHORS = [1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071]
MORE_ANCHORS = [0.7, 0.9, 2.1, 6.3, 7.5, 2.2]              # the extension for 8 anchors
THRESH = 0.6
# The tolerance of the per-element comparison on the device, in units of eps32 * scale (region_loss_ref.py).  The torch
# restatement on the CPU, float32 like the kernel, is within 7.38 units of the float64 reference over every element of
# every input below (gradient; loss 1.00; printed by test_region_loss_cpu.py).  K = 4 x that, for the device's expf / logf
# and contraction against the CPU's libm, rounded up to a power of two.
YARDSTICK = 7.38
K = 32.0
SCALES = {"s3_05_5_2": (3.0, 0.5, 5.0, 2.0), "workload": (1.0, 1.0, 5.0, 1.0)}     # (coord, noobject, object, class)

# name: (B, A, C, H, W, sigma of the logits, seed)
CASES = {
    "13x13": (3, 5, 20, 13, 13, 1.5, 1),            # the workload's grid
    "19x19": (3, 5, 20, 19, 19, 1.0, 8),            # 361 cells: two trips of the strided loop
    "17x16a8c1": (2, 8, 1, 17, 16, 1.5, 3),         # 272 cells: 16 threads on the second trip; the anchor maximum; one class
    "16x16": (2, 5, 20, 16, 16, 1.0, 4),            # exactly 256 cells
    "7x10": (2, 3, 4, 7, 10, 1.5, 1),               # H below W
    "10x7": (2, 3, 4, 10, 7, 1.0, 2),               # H above W
    "5x3a1c80": (2, 1, 80, 5, 3, 1.5, 3),           # fewer cells than a wave, one anchor, 80 classes
    "b4": (4, 5, 20, 13, 13, 1.0, 4),               # the batch-independence input: 50 boxes, six, none, six
}


def anchors_for(A):
    return (BENCH_ANCHORS + MORE_ANCHORS)[:2 * A]


def _few_rows(g, C, H, W, aw0, ah0):
    rows = torch.zeros(10, 5)
    rows[0] = torch.tensor([float(1 % C), 0.9 / W, 2.5 / H, 1.2 * aw0 / W, 1.2 * ah0 / H])      # cell (row 2, column 0)
    r = torch.rand(9, 5, generator=g)
    for t in range(1, 10):
        edge_row = 0.0 if t % 2 else float(H - 1)               # the other boxes keep to the first and last grid rows
        rows[t] = torch.tensor([float(int(r[t - 1, 0] * C)), 0.02 + 0.96 * float(r[t - 1, 1]),
                                (edge_row + 0.05 + 0.9 * float(r[t - 1, 2])) / H,
                                0.05 + 0.5 * float(r[t - 1, 3]), 0.05 + 0.5 * float(r[t - 1, 4])])
    rows[6, 1] = 0.0                                            # the terminator: only x is 0; rows 7..9 must be ignored
    return rows.view(-1)


@functools.lru_cache(maxsize=None)
def make(name):
    """(out [B, A*(5+C), H, W], target [B, 250]) as float32 CPU tensors; do not modify them."""
    B, A, C, H, W, sigma, seed = CASES[name]
    anchors = anchors_for(A)
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(B, A * (5 + C), H, W, generator=g) * sigma
    o = out.view(B, A, 5 + C, H, W)
    o[:, :, 2:4].clamp_(max=4.0)
    target = torch.zeros(B, 250)
    # image 0: 50 boxes
    r = torch.rand(50, 5, generator=g)
    rows = torch.stack(((r[:, 0] * C).floor(), 0.01 + 0.98 * r[:, 1], 0.01 + 0.98 * r[:, 2], 0.02 + 0.6 * r[:, 3],
                        0.02 + 0.6 * r[:, 4]), 1)
    rows[40] = rows[5]
    rows[40, 0] = (rows[5, 0] + 1) % C
    rows[41, 1], rows[42, 2] = 1.0, 1.0
    rows[43, 3] = 0.0
    rows[44, 0], rows[45, 0] = float(C), -1.0
    rows[46, 0] = min(2, C - 1) + 0.7
    target[0] = rows.view(-1)
    for b in (1, 3):
        if b < B:
            target[b, :50] = _few_rows(g, C, H, W, anchors[0], anchors[1])
            # the prediction at image b's first box, anchor 0, cell (2, 0), and one cell to its right
            lw = math.log(math.log(1.2))
            o[b, 0, 0:5, 2, 0] = torch.tensor([math.log(0.9 / 0.1), 0.0, lw, lw, 0.3])
            if W > 1:
                o[b, 0, 0:5, 2, 1] = torch.tensor([-6.0, 0.0, lw, lw, 0.3])
    # float32-infinite predicted boxes on unassigned cells of the images with boxes
    assigned = region_loss_ref(out.numpy(), target.numpy(), anchors, A, C, SCALES["workload"], THRESH).info["assigned"]
    for b in range(B):
        if target[b, 1] == 0:
            continue
        free = [(n, j, i) for n in range(A) for j in range(H) for i in range(W)
                if not assigned[b, n, j, i] and not (b in (1, 3) and n == 0 and j == 2 and i < 2)]
        for k, (n, j, i) in enumerate(free[::max(1, len(free) // 4)][:4]):
            if k % 2 == 0:
                o[b, n, 2, j, i] = 5.0
            if k % 3 != 0:
                o[b, n, 3, j, i] = 6.0
    return out, target


@functools.lru_cache(maxsize=None)
def reference(name, scales_name, in_range_labels=False):
    """region_loss_ref of make(name).  in_range_labels: with the two out-of-range labels of image 0 replaced by class 0
    (what the torch restatement can be run on: its cross_entropy raises for a label outside [0, C), as the reference's)."""
    B, A, C, H, W, _, _ = CASES[name]
    out, target = make(name)
    if in_range_labels:
        target = labels_in_range(target, C)
    return region_loss_ref(out.numpy(), target.numpy(), anchors_for(A), A, C, SCALES[scales_name], THRESH)


def labels_in_range(target, C):
    t = target.clone().view(target.shape[0], 50, 5)
    t[:, :, 0] = torch.where((t[:, :, 0] < 0) | (t[:, :, 0] >= C), torch.zeros_like(t[:, :, 0]), t[:, :, 0])
    return t.view(target.shape[0], 250)


ALL = [(n, s) for n in CASES for s in SCALES]
IDS = ["%s-%s" % p for p in ALL]
