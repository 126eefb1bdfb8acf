"""The cases of tests/test_q8_w4_kernels_gpu.py: launches of mcamd_conv_fwd_q8_w4 (csrc/conv_q8_w4.hip), their operands
and references.  The shapes are rows of q8_cases._INFERENCE_ROWS -- the smallest that cross each boundary -- on every instance
the w4 choice can launch, in both MFMA forms; test_q8_w4_cpu.py proves without a GPU that they reach every instance and that
every case's reference meets the conditions of exactness.  Test-side only."""
import zlib

import torch

from modelcompression_amd import ops
import q8_cases as QC
import q8_ref as R
import w4_ref as W

# (f8mfma, bmw): the instances of the w4 choice -- mcamd_q8_choice's for the fp8 block
INSTANCES = ((0, 128), (0, 64), (1, 256), (1, 128), (1, 64))
ROWS = ("plain", "pool", "pool+y2-f8+f16", "reorg", "one-tile", "walk", "long-k")
CASES = [c for c in QC.DENSE_CASES if c.name.split("-", 1)[1] in ROWS]
DETERMINISM_CASES = ("d128-plain", "d256m-pool+y2-f8+f16")
# Weight draws of the exact test: 5 and 7 are not on the e2m1 grid next to a filter maximum of 7 (s / 2^g = d / 2: 2.5 -> 2, 3.5
# -> 4), so rounding happens; uneven, so errors do not cancel.  A case with an fp16 destination takes the sparser draw: its
# values v = 2 c_f sum(d d') + shift_f (c_f <= 2, shifts in steps of 1 / 4) must be fp16 numbers (condition 2), |sum d d'| < 128,
# and over the 576 terms of a 3x3 case with activations from "d1" this draw's sum has a standard deviation of ~21.  The long-K
# cases keep their sparse draw (condition 1).
W4_DRAW = (-7, -5, -3, -1, 0, 0, 0, 0, 0, 0, 1, 2, 5, 7)
W4_DRAW_F16 = (-7, -5, -1, 1, 2, 5, 7) + (0,) * 27


def info_of(c):
    return ops.conv_fwd_q8_w4_info(QC.geom_of(c))


def operands(c, gaussian=False):
    """q8_cases.operands with, for the integer draws, the weights drawn from W4_DRAW / W4_DRAW_F16 (times the same 2^-p_f)."""
    o = QC.operands(c, gaussian=gaussian)
    if gaussian or c.wdraw.startswith("s"):
        return o
    gen = torch.Generator().manual_seed(zlib.crc32(("w4-" + c.name).encode()))
    w = QC._draw(gen, W4_DRAW_F16 if "f16" in c.fmt else W4_DRAW, tuple(o.w.shape)) * torch.pow(2.0, -o.p.float()).view(-1, 1, 1, 1)
    return o._replace(w=w)


def reference(c, o):
    """q8_cases.reference on w4_ref's bytes and exponents: float64 convolution of the codes' values, q8_ref's epilogue and
    stores.  (w8 = w8_eff = the bytes the 4-bit codes stand for, e = e4.)"""
    codes, g, e4, values, w8 = W.quantise(o.w, o.mask)
    assert torch.equal(R.deq(w8).double(), values), "every w4 value is an e4m3 number"
    v = R.block(o.a8, w8, e4, o.scale, o.shift, c.slope, dtype=torch.float64)
    v64 = QC._v64(c, o, w8, e4, c.slope)
    assert torch.equal(v.double(), v64), "the epilogue value is an fp32 number"

    def store(fmt, dst):
        return R.store_bytes(v, dst) if fmt == "f8" else R.store_fp16(v, dst)

    dst = "pool" if c.dst == "pool+y2" else c.dst
    y = store(c.fmt_y, dst)
    y2 = store(c.fmt_y2, "plain") if c.dst == "pool+y2" else None
    return QC.Reference(v64, 2.0 * v64, y, y2, None, None, None, w8, w8, e4), (codes, g)


_CACHE = {}


def operands_and_reference(c):
    """Once per process and case; shared by the tests and never modified."""
    if c.name not in _CACHE:
        o = operands(c)
        ref, cg = reference(c, o)
        _CACHE[c.name] = (o, ref, cg)
    return _CACHE[c.name]


def adversarial(gen, cout=72, cin=128, k=3):
    """Gaussian filters with: filter 0 one 100x outlier; filter 1 one group at 2^-20 of the rest; filter 2 one all-zero group;
    filter 3 all zero; filter 4 a group whose maximum sits exactly on 6 * 2^g after scaling (a power-of-two ratio)."""
    w = torch.randn(cout, cin, k, k, generator=gen) * 0.05
    w[0, 5, k // 2, k // 2] = 100.0 * float(w[0].abs().max())
    w[1, 32:64, 0, 0] *= 2.0 ** -20
    w[2, 0:32, k - 1, k - 1] = 0.0
    w[3] = 0.0
    w[4, 64:96, 0, 0] = w[4, 64:96, 0, 0].clamp(-0.01, 0.01)
    w[4, 70, 0, 0] = 0.75 * 2.0 ** -4                        # 6 * 2^g for some g once scaled by a power of two
    return w
