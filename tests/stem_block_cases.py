"""The inputs and constants of test_stem_block_cpu.py and test_stem_block_gpu.py (csrc/conv_stem_block.hip).

Every input is made of float32 CPU tensors; the reference (stem_block_ref.py) works from `x16` / `w16`, the fp16-rounded
image and the fp16-rounded masked weights in float64 -- what the kernels multiply.  Do not modify what make() returns.
"""
import collections
import functools

import torch

import stem_block_ref as R

SLOPE = 0.1
EPS = 1e-5
TAU = 1e-4                  # pooled pixels whose z_win, or whose gap to the runner-up, is inside (0, TAU) get G = 0
MAX_EXCLUDED = 1e-3         # ... and at most this share of a case's pooled pixels may be
GRAD_SCALE = 8.0

# Tolerances of the per-element / per-channel comparisons on the device, in units of EPS32 * scale (stem_block_ref.py).
# YARDSTICK_*: the float32 restatement on the CPU against the float64 reference, the largest figure over every case below
# (test_stem_block_cpu.py measures and prints them, and fails should one outgrow its K).  K = 4 x the yardstick, rounded up
# to a power of two; the factor 4 is for the MFMA's internal order and contraction.
YARDSTICK_FWD, K_FWD = 2.14, 16.0         # z = sc y + sh: F.conv2d and one fma in float32
YARDSTICK_STATS, K_STATS = 4.42, 32.0    # mean and var from S and C accumulated in float32 chains of 128 steps of 32 pixels
YARDSTICK_BWD, K_BWD = 0.148, 1.0         # dW, dgamma, dbeta from T and sum g_z accumulated the same way
# Split operands (x_hi w_hi + x_lo w_hi + x_hi w_lo) against the reference on the UNROUNDED fp32 image and weights: the
# block's documented claims, hi + lo within 2e-6 and the hi plane alone within the fp16 rounding (4e-4), per element:
# 2e-6 / EPS32 = 16.8 -> 16 units (the three dropped or rounded 2^-22 terms are 1.5 of them), hi alone as every fp16 output.
K_SPLIT = 16.0
LO_TERM = 2.0 ** -22        # planes >= 2: hi + lo against the unrounded m, in place of the fp16 half-ulp

SHAPES = [(1, 2, 32), (3, 6, 64), (5, 20, 96)]      # one unit, all border | a 32-column block and a unit-row pair | a ragged tail
MULTIPASS = (5470, 6, 64)                           # 32820 units, 65640 Gram steps: every kernel makes >= 2 passes
STATS_SHAPE = (4, 32, 64)
TIES_SHAPE = (2, 20, 64)

Case = collections.namedtuple("Case", "B H W x w mask gamma beta rm0 rv0 G x16 w16")


def q16(t):
    return t.half().float()


def _finish(B, H, W, x, w, mask, gen, gamma=None, beta=None):
    n = w.shape[0]
    gamma = torch.rand(n, generator=gen) + 0.5 if gamma is None else gamma
    beta = torch.randn(n, generator=gen) * 0.2 if beta is None else beta
    rm0, rv0 = torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) + 0.5
    G = q16(torch.randn(B, n, H // 2, W // 2, generator=gen))
    weff = w * mask if mask is not None else w
    return Case(B, H, W, x, w, mask, gamma, beta, rm0, rv0, G, q16(x).double(), q16(weff).double())


@functools.lru_cache(maxsize=None)
def make(B, H, W, masked=False, cout=32):
    """Uniform-random image, randn * 0.3 filters; masked: 40 % of the taps pruned and filter 5 pruned entirely."""
    gen = torch.Generator().manual_seed(1000 * B + 10 * H + W + (1 if masked else 0) + cout)
    x = torch.rand(B, 3, H, W, generator=gen)
    w = torch.randn(cout, 3, 3, 3, generator=gen) * 0.3
    mask = None
    if masked:
        mask = (torch.rand(cout, 3, 3, 3, generator=gen) > 0.4).float()
        mask[5] = 0.0
    return _finish(B, H, W, x, w, mask, gen)


BLOB, EDGE, PRUNED, TINY, HUGE = 0, 1, 2, 3, 4      # the conditioning filters of make_stats


@functools.lru_cache(maxsize=None)
def make_stats(image):
    """Statistics conditioning.  Filters: 0 a blob (all taps positive), 1 an edge (taps sum to zero after the fp16
    rounding), 2 fully pruned, 3 at weight scale 1e-3 (var < eps), 4 at scale 30, the rest randn * 0.3.  Images:
    "a" uniform random; "b" 8-bit levels, mean 0.5, std 0.1; "c" 8-bit levels, 0.9 +- 0.02."""
    B, H, W = STATS_SHAPE
    gen = torch.Generator().manual_seed(77)
    w = torch.randn(32, 3, 3, 3, generator=gen) * 0.3
    w[BLOB] = torch.rand(3, 3, 3, generator=gen) * 0.3 + 0.05
    col = torch.tensor([-1.0, 0.0, 1.0]) * torch.tensor([0.25, 0.5, 0.25]).view(3, 1)     # a Sobel filter: exact in fp16
    w[EDGE] = col.expand(3, 3, 3) * torch.tensor([0.5, 1.0, 0.25]).view(3, 1, 1)
    w[TINY] *= 1e-3 / 0.3
    w[HUGE] *= 30.0 / 0.3
    mask = torch.ones(32, 3, 3, 3)
    mask[PRUNED] = 0.0
    gen = torch.Generator().manual_seed({"a": 1, "b": 2, "c": 3}[image])
    if image == "a":
        x = torch.rand(B, 3, H, W, generator=gen)
    else:
        mu, sd = (0.5, 0.1) if image == "b" else (0.9, 0.02)
        x = ((mu + sd * torch.randn(B, 3, H, W, generator=gen)).clamp(0, 1) * 255.0).round() / 255.0
    return _finish(B, H, W, x, w, mask, gen)


@functools.lru_cache(maxsize=None)
def make_ties(kind):
    """Pool ties with exact arithmetic: image values are multiples of 1/16 in [0, 1] and weights multiples of 1/8 in
    [-1/2, 1/2], so every y is exact in float32 and float64 in any summation order.  No mask.
    "rows": only the centre-row taps are non-zero and image rows 2j, 2j + 1 are equal (neighbouring pairs differ): the two
            rows of every window tie while their v differ, so the ty = 0 and ty = 2 entries of dW depend on the choice;
    "cols": the transposed construction;
    "bands": constant colour bands, 6 pixels wide, on all four borders around random content, dense filters."""
    B, H, W = TIES_SHAPE
    gen = torch.Generator().manual_seed({"rows": 11, "cols": 12, "bands": 13}[kind])
    lv = lambda *shape: torch.randint(0, 17, shape, generator=gen).float() / 16.0
    w = torch.randint(-4, 5, (32, 3, 3, 3), generator=gen).float() / 8.0
    if kind == "rows":
        x = lv(B, 3, H // 2, W).repeat_interleave(2, dim=2)
        w[:, :, 0, :] = 0.0
        w[:, :, 2, :] = 0.0
    elif kind == "cols":
        x = lv(B, 3, H, W // 2).repeat_interleave(2, dim=3)
        w[:, :, :, 0] = 0.0
        w[:, :, :, 2] = 0.0
    else:
        x = lv(B, 3, H, W)
        colour = lv(B, 3, 1, 1).expand(B, 3, H, W)
        inner = torch.zeros(1, 1, H, W, dtype=torch.bool)
        inner[:, :, 6:H - 6, 6:W - 6] = True
        x = torch.where(inner, x, colour).contiguous()
    return _finish(B, H, W, x, w, None, gen)


@functools.lru_cache(maxsize=None)
def make_multipass():
    """Every image of MULTIPASS has content of its own (one stream of uniform random numbers) and a brightness of its own
    in [0.25, 1]: a pass that reads other images than its own then moves the batch statistics beyond their bound (with
    equally bright images only the per-element forward and backward comparisons notice)."""
    B, H, W = MULTIPASS
    gen = torch.Generator().manual_seed(5470)
    x = torch.rand(B, 3, H, W, generator=gen) * (0.25 + 0.75 * torch.rand(B, 1, 1, 1, generator=gen))
    w = torch.randn(32, 3, 3, 3, generator=gen) * 0.3
    return _finish(B, H, W, x, w, None, gen)


@functools.lru_cache(maxsize=None)
def pre(case_fn, *args):
    c = case_fn(*args)
    return R.pre(c.x16, c.w16)


@functools.lru_cache(maxsize=None)
def stats(case_fn, *args):
    c = case_fn(*args)
    return R.stats(c.x16, c.w16, EPS)


def split_operands(c):
    """The float64 reference operands of the split-operand block: the UNROUNDED fp32 image and masked weights."""
    weff = c.w * c.mask if c.mask is not None else c.w
    return c.x.double(), weff.double()
