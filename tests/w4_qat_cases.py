"""The cases of tests/test_q8_w4_qat_kernels_gpu.py: launches of mcamd_conv_fwd_q8_w4_raw (csrc/conv_q8_w4.hip),
their operands and exact references.  The shapes are q8_cases._RAW_ROWS -- r-stats, r-nostats, r-walk, r-one-tile on every
instance of w4_cases.INSTANCES -- and the 180-chunk long-K row on the (0, 128) and (1, 256) instances; test_q8_w4_qat_cpu.py
proves without a GPU that they reach every instance and that every case of the exact test meets q8_cases.exactness on the
reference's own operands, the statistics condition included.  Test-side only."""
import zlib

import torch
import torch.nn.functional as F

import q8_cases as QC
import q8_ref as R
import w4_cases as WC
import w4_ref as W

ROWS = ("r-stats", "r-nostats", "r-walk", "r-one-tile")
CASES = [c for c in QC.RAW_CASES if c.name.split("-", 1)[1] in ROWS + ("long-k",)]
CASES += [QC.case("r256m-long-k", "raw", 2, 13, 13, 3, 1280, 256, ("raw", 1, 256), mfma=1, draw="s4", wdraw="s4u", fmt="f32")]
DETERMINISM_CASES = ("r128-r-stats", "r256m-r-stats")
DRAW_SETS = (("W4_DRAW", WC.W4_DRAW), ("W4_DRAW_F16", WC.W4_DRAW_F16))


def instance_of(c):
    return c.expect[1:]


def _operands(c, draw):
    o = QC.operands(c)
    if c.wdraw.startswith("s"):                              # the long-K rows keep their sparse draw (condition 1)
        return o
    gen = torch.Generator().manual_seed(zlib.crc32(("w4-qat-" + c.name).encode()))
    w = QC._draw(gen, draw, tuple(o.w.shape)) * torch.pow(2.0, -o.p.float()).view(-1, 1, 1, 1)
    return o._replace(w=w)


def operands(c, gaussian=False):
    return QC.operands(c, gaussian=True) if gaussian else operands_and_reference(c)[0]


def reference(c, o):
    """q8_cases.reference's raw form on w4_ref's bytes and exponents: y = 2^-(e4 + 1) S in float64 and its per-channel sum and
    sum of squares over every 128-pixel slab row."""
    codes, g, e4, values, w8 = W.quantise(o.w, o.mask)
    assert torch.equal(R.deq(w8).double(), values), "every w4 value is an e4m3 number"
    Sum = F.conv2d(R.deq(o.a8).double(), values, None, 1, (c.k - 1) // 2)
    raw = Sum * torch.pow(2.0, -(e4.double() + 1.0)).view(1, -1, 1, 1)
    flat = raw.permute(0, 2, 3, 1).reshape(c.M, c.cout)
    rows = -(-c.M // 128)
    padded = torch.zeros(rows * 128, c.cout, dtype=torch.float64)
    padded[:c.M] = flat
    padded = padded.view(rows, 128, c.cout)
    return QC.Reference(None, None, raw, None, raw, padded.sum(1), (padded * padded).sum(1), w8, w8, e4)


_CACHE = {}


def operands_and_reference(c):
    """Once per process and case; shared by the tests and never modified.  (operands, reference, name of the weight draw): the
    weights come from w4_cases.W4_DRAW -- 5 and 7 are off the grid, so rounding happens -- unless the REFERENCE of that draw
    misses a condition of q8_cases.exactness (decided on the CPU from the reference's operands alone, never from kernel output);
    then from the sparser W4_DRAW_F16."""
    if c.name not in _CACHE:
        for name, draw in DRAW_SETS:
            o = _operands(c, draw)
            ref = reference(c, o)
            if c.wdraw.startswith("s"):
                name = c.wdraw
            if QC.exactness(c, o, ref) == [] or name == DRAW_SETS[-1][0]:
                break
        _CACHE[c.name] = (o, ref, name)
    return _CACHE[c.name]
