"""The split-K forward pair (csrc/conv_splitk.hip, mcamd_conv_fwd_splitk) per element.
(These are the Gaussian checks on real shapes; test_splitk_instances_gpu.py holds every instance to an exact reference.)

Reference: float64 conv2d on the fp16-rounded operands, r = leaky(scale * conv + shift) (raw form: r = conv).

T1  slices = 1 is bit-equal to mcamd_conv_fwd on the same operands wherever mcamd_conv_tile_info reports igemm_kernel
    (kernel 0): same instruction, same K order, same epilogue formula.  This pins addressing, pooled enumeration, channel
    offsets and the stores; the split cases then add only the reduction.
T2  slices > 1, per element: |got - r| <= ulp16(r) / 2 + c 2^-24 A, A = |scale| sum |x||w| + |shift| in float64, ulp16 = the
    fp16 spacing at r (2^-24 below the normal range).  A CPU emulation of both summation orders (exact 16-term blocks, fp32
    accumulation, K up to 9 216) gives at most 0.24 for the figure (|got - r| - ulp16 / 2) / (2^-24 A), which would make c = 1
    a fourfold margin.  The maximum of that figure is printed for the split result and for mcamd_conv_fwd on the same inputs;
    on the hardware today's kernel itself reads above 0.5 (MEASURED below: the MFMA's accumulation is not the emulation's
    exact 16-term block), so c is twice ITS measured maximum: c = 2 x 0.749 = 1.498.
T3  against the slices = 1 result at most 1 % of the elements differ at all (the emulation flips 0.5 to 1.9 per thousand
    of the fp16 roundings), and every element passes T2.
T4  two launches with the same slice count are bit-equal.
T5  sentinel method of test_conv_epi_store_gpu.py: every element outside the slice keeps the sentinel (workspace aside) and
    the slice is bit-equal to a launch into a zeroed buffer.

Case c asks for forced slice counts 1, 4 and 7 in all four destination forms; its REORG form is the 1x1 layer, whose K axis
is 3 chunks of 32, and the entry point refuses more slices than chunks, so that form runs 1, 2 and 3 (one chunk each).

MEASURED (MI355X; the figure's maximum per case, mcamd_conv_fwd | split): a 0.143 | 0.125, b 0.026 | 0.006, c 0.110 | 0.123,
c1 (REORG) 0.020 | 0.057, d 0.192 | 0.186, e 0.192 | 0.184, f 0.371 | 0.069, conv19 0.578 | 0.199 (5 slices), conv13 0.749 | 0.296
(2 slices).  Over all cases: mcamd_conv_fwd 0.749, split 0.296 -- the shorter chains of a slice round less.  T3: at most
0.29 % of the elements differ from the one-slice result."""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops, _lib as L  # noqa: E402
from util import to_padded, q16  # noqa: E402
import oracle.darknet_ref as ref  # noqa: E402

OFF, OFF2 = 8, 32
SLOPE = 0.1
SENT = 7.0
C_BOUND = 2 * 0.749      # twice the measured maximum of mcamd_conv_fwd itself (docstring)
CASES = {
    "a": dict(B=1, H=13, W=13, k=3, cin=128, cout=64),
    "b": dict(B=1, H=13, W=13, k=1, cin=192, cout=64),
    "c": dict(B=2, H=6, W=10, k=3, cin=96, cout=72),
    "c1": dict(B=2, H=6, W=10, k=1, cin=96, cout=72),       # case c's REORG form
    "d": dict(B=1, H=12, W=12, k=3, cin=40, cout=264),
    "e": dict(B=1, H=13, W=13, k=3, cin=128, cout=64, x_choff=64),
    "f": dict(B=1, H=13, W=13, k=3, cin=64, cout=40),
    "conv19": dict(B=1, H=13, W=13, k=3, cin=1024, cout=1024),
    "conv13": dict(B=1, H=26, W=26, k=3, cin=256, cout=512),
}
# (case, form, forced slice counts; 0 = the policy)
RUNS = [("a", "plain", (1, 2, 5, 0)), ("b", "plain", (1, 3)),
        ("c", "plain", (1, 4, 7)), ("c", "pool", (1, 4, 7)), ("c", "pool+y2", (1, 4, 7)), ("c1", "reorg", (1, 2, 3)),
        ("d", "pool+y2", (1, 3)), ("e", "plain", (1, 2)), ("f", "raw", (1, 3)),
        ("conv19", "plain", (1, 0)), ("conv13", "pool+y2", (1, 0))]
SPLIT = [(n, f, s) for (n, f, ss) in RUNS for s in ss if s != 1]
IDS = ["%s-%s-%d" % t for t in SPLIT]


def whole(buf):
    return torch.empty(0, dtype=buf.dtype, device=buf.device).set_(buf.untyped_storage())


@functools.lru_cache(maxsize=None)
def operands(dev, name):
    """Input, packed weights, coefficients and the float64 reference (r and A for the fused and the raw form) of a case."""
    c = types.SimpleNamespace(**CASES[name])
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + c.cin + c.cout)
    xoff = CASES[name].get("x_choff", 0)
    xfull = torch.randn(c.B, c.cin + xoff, c.H, c.W, generator=gen)
    w = torch.randn(c.cout, c.cin, c.k, c.k, generator=gen) * (2.0 / (c.cin * c.k * c.k)) ** 0.5
    scale, shift = torch.rand(c.cout, generator=gen) + 0.5, torch.randn(c.cout, generator=gen) * 0.2
    ld = ops.round_up(c.cin + xoff, 32)
    xbuf, _ = to_padded(xfull.to(dev), ld=ld)
    g = ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, ld, xoff)
    wp = ops.pack_weights(g, w.to(dev).contiguous(), None, True, False)[0]
    xq, wq = q16(xfull[:, xoff:]).double(), q16(w).double()
    conv = F.conv2d(xq, wq, padding=c.k // 2)
    aconv = F.conv2d(xq.abs(), wq.abs(), padding=c.k // 2)
    sc, sh = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    z = conv * sc + sh
    return types.SimpleNamespace(c=c, g=g, x=xbuf, wp=wp, scale=scale.to(dev), shift=shift.to(dev),
                                 r=torch.where(z > 0, z, z * SLOPE), A=aconv * sc.abs() + sh.abs(), r_raw=conv, A_raw=aconv)


def launch(dev, name, form, slices, entry="splitk", fill=0.0):
    """One launch; returns [(buffer, kind, (b, h, w), ld, choff, channels)] for y and, when present, y2."""
    op = operands(dev, name)
    c, g = op.c, op.g
    if form == "raw":
        ld = ops.round_up(OFF + c.cout + 8, 32)
        y = torch.full((c.B * c.H * c.W * ld,), fill, dtype=torch.float16, device=dev)
        if entry == "splitk":
            ops.conv_fwd_raw_splitk(g, op.x, op.wp, y, ld, OFF, slices=slices)
        else:
            ops.conv_fwd_raw(g, op.x, op.wp, y, ld, OFF)
        torch.cuda.synchronize()
        return [(y, "raw", (c.B, c.H, c.W), ld, OFF, c.cout)]
    mode = {"plain": L.DST_PLAIN, "pool": L.DST_POOL, "pool+y2": L.DST_POOL, "reorg": L.DST_REORG}[form]
    ho, wo = (c.H, c.W) if form == "plain" else (c.H // 2, c.W // 2)
    cdst = 4 * c.cout if form == "reorg" else c.cout
    ld, ld2 = ops.round_up(OFF + cdst + 8, 32), ops.round_up(OFF2 + c.cout + 8, 32)

    def alloc(hh, ww, ld_):
        buf = ops.alloc_padded(c.B, hh, ww, ld_, dev)
        if fill:
            whole(buf).fill_(fill)
        return buf

    y = alloc(ho, wo, ld)
    y2 = alloc(c.H, c.W, ld2) if form == "pool+y2" else None
    kw = dict(dst_mode=mode, y2=y2, y2_ld=ld2 if y2 is not None else 0, y2_choff=OFF2 if y2 is not None else 0)
    if entry == "splitk":
        ops.conv_fwd_splitk(g, op.x, op.wp, y, ld, OFF, op.scale, op.shift, SLOPE, slices=slices, **kw)
    else:
        ops.conv_fwd_padded(g, op.x, op.wp, y, ld, OFF, op.scale, op.shift, SLOPE, **kw)
    torch.cuda.synchronize()
    out = [(y, "pad", (c.B, ho, wo), ld, OFF, cdst)]
    if y2 is not None:
        out.append((y2, "pad", (c.B, c.H, c.W), ld2, OFF2, c.cout))
    return out


def slice_of(dst):
    """fp16 NCHW (cpu) of a destination's slice."""
    buf, kind, (b, h, w), ld, choff, ch = dst
    if kind == "raw":
        v = buf.view(b, h, w, ld)[..., choff:choff + ch]
    else:
        v = ops.padded_view(buf, b, h, w, ld)[:, 1:-1, 1:-1, choff:choff + ch]
    return v.permute(0, 3, 1, 2).contiguous().cpu()


@functools.lru_cache(maxsize=None)
def result(dev, name, form, slices, entry="splitk"):
    return [slice_of(d) for d in launch(dev, name, form, slices, entry)]


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def ulp16(r):
    e = torch.frexp(r.abs())[1].double()        # |r| = m 2^e, m in [0.5, 1): spacing 2^(e - 11)
    return torch.clamp(torch.exp2(e - 11), min=2.0 ** -24)


def figure(got, r, A):
    """(|got - r| - ulp16(r) / 2) / (2^-24 A) per element: T2 asks for <= c."""
    return ((got.double() - r).abs() - ulp16(r) / 2) / (2.0 ** -24 * A)


def full_res(dev, name, form, outs):
    """The full-resolution per-element tensor a result holds, with its reference: y itself (plain, raw), y2 (pool + y2), the
    inverse of the oracle's reorg permutation (reorg); None for pool alone (checked against pool + y2)."""
    op = operands(dev, name)
    if form == "raw":
        return outs[0], op.r_raw, op.A_raw
    if form == "plain":
        return outs[0], op.r, op.A
    if form == "pool+y2":
        return outs[1], op.r, op.A
    if form == "reorg":
        return outs[0], ref.reorg(op.r), ref.reorg(op.A)
    return None


def check_pool_relations(dev, name, form, slices, outs):
    if form == "pool+y2":
        assert same_bits(outs[0], F.max_pool2d(outs[1].float(), 2, 2).half()), "pooled output != max_pool2d of the stored y2"
    if form == "pool":
        assert same_bits(outs[0], result(dev, name, "pool+y2", slices)[0]), "pool without y2 differs from pool with y2"


@pytest.mark.parametrize("name, form", [(n, f) for (n, f, _) in RUNS], ids=["%s-%s" % (n, f) for (n, f, _) in RUNS])
def test_t1_one_slice_equals_conv_fwd(dev, name, form):
    got, base = result(dev, name, form, 1), result(dev, name, form, 1, "fwd")
    kernel = ops.tile_info(operands(dev, name).g)[3]
    fr = full_res(dev, name, form, got)
    if fr is not None:
        fb = full_res(dev, name, form, base)
        print("T2 figure, one slice: %.3f  mcamd_conv_fwd (kernel %d): %.3f" % (float(figure(*fr).max()), kernel, float(figure(*fb).max())))
        assert float(figure(*fr).max()) <= C_BOUND
    check_pool_relations(dev, name, form, 1, got)
    if kernel == 0:
        for a, b in zip(got, base):
            assert same_bits(a, b), "slices = 1 differs from mcamd_conv_fwd"


@pytest.mark.parametrize("name, form, slices", SPLIT, ids=IDS)
def test_t2_t3_split_per_element(dev, name, form, slices):
    op = operands(dev, name)
    info = ops.conv_fwd_splitk_info(op.g, L.EPI_RAW_F16 if form == "raw" else L.EPI_PAD_F16,
                                    {"pool": 1, "pool+y2": 1, "reorg": 2}.get(form, 0), slices)
    if slices == 0:
        assert info.slices >= 2, (name, info.slices)      # the policy splits these shapes
    got, one = result(dev, name, form, slices), result(dev, name, form, 1)
    fr = full_res(dev, name, form, got)
    if fr is not None:
        fig = figure(*fr)
        fb = full_res(dev, name, form, result(dev, name, form, 1, "fwd"))
        print("T2 figure, %d slices: %.3f  mcamd_conv_fwd: %.3f" % (info.slices, float(fig.max()), float(figure(*fb).max())))
        assert float(fig.max()) <= C_BOUND, "T2: %d elements over the bound" % int((fig > C_BOUND).sum())
    check_pool_relations(dev, name, form, slices, got)
    for a, b in zip(got, one):                                            # T3
        differ = float((a.view(torch.int16) != b.view(torch.int16)).double().mean())
        print("T3: %.4f %% of the elements differ from the one-slice result" % (100 * differ))
        assert differ <= 0.01


@pytest.mark.parametrize("name, form, slices", [("a", "plain", 5), ("c", "pool+y2", 7), ("f", "raw", 3), ("conv19", "plain", 0)])
def test_t4_deterministic(dev, name, form, slices):
    first = result(dev, name, form, slices)
    again = [slice_of(d) for d in launch(dev, name, form, slices)]
    assert all(same_bits(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("name, form", [("c", "plain"), ("c", "pool"), ("c", "pool+y2"), ("c1", "reorg"), ("f", "raw")])
def test_t5_writes_its_slice_only(dev, name, form):
    slices = 3
    dirty = launch(dev, name, form, slices, fill=SENT)
    for dst, clean in zip(dirty, result(dev, name, form, slices)):
        buf, kind, (b, h, w), ld, choff, ch = dst
        got = slice_of(dst)
        all_ = whole(buf).clone()
        if kind == "raw":
            all_.view(b, h, w, ld)[..., choff:choff + ch] = SENT
        else:
            n = b * (h + 2) * (w + 2) * ld
            all_[buf.storage_offset():buf.storage_offset() + n].view(b, h + 2, w + 2, ld)[:, 1:-1, 1:-1, choff:choff + ch] = SENT
        assert bool((all_ == SENT).all()), "an element outside the slice was written"
        assert bool((clean != 0).any()), "the launch wrote nothing"
        assert same_bits(got, clean), "slice differs from the zero-initialised launch"
