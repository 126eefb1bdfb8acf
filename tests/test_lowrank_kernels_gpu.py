"""The fused low-rank forward (csrc/conv_lowrank.hip, mcamd_conv_fwd_lowrank) per element.

Reference, in float64, following the contract of include/mcamd.h: H = conv(x, U) rounded through torch.float16 (saturated),
Y = conv1x1(H, V), out = fp16(leaky(Y * scale + shift)) with power-of-two scales and SLOPE.  The exact cases draw small
integers with max|x| max|U| Ktot < 2^24 and max|H| max|V| r < 2^24, so every partial sum in any order is exact and the
comparison is torch.equal; every byte outside the output slice must keep its NaN sentinel.

Gaussian operands at a real shape: both the fused launch and the unfused pair of the dense kernels (conv_fwd_raw to r
channels, conv_fwd_padded of the 1 x 1 block) differ from the reference only by the order of their fp32 sums and the tie
flips of the fp16 roundings that follow from it; the fused launch may have twice the pair's rel-L2 error.
MEASURED (MI355X): pair 4.654e-05, fused 4.654e-05 (the reference is itself rounded to fp16: only elements whose rounding flipped count)."""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops, _lib as L  # noqa: E402
from conv_cases import _draw, DRAWS, SLOPE, reorg  # noqa: E402
from lowrank_cases import reference  # noqa: E402
from util import fill_padded, padded_split, whole, rel_l2  # noqa: E402

DST = {"plain": L.DST_PLAIN, "pool": L.DST_POOL, "pool+y2": L.DST_POOL, "reorg": L.DST_REORG}
# name: B H W k cin cout r dst (x_ld, x_choff, y_ld, y_choff) draws (x, U, V) absolute
CASES = {
    "k3-r32-n8": (1, 13, 13, 3, 32, 8, 32, "plain", None, ("d1", "d2", "d2"), False),
    "k1-r96-n72": (1, 13, 13, 1, 96, 72, 96, "plain", None, ("d2", "d2", "d2"), False),
    "k3-r256-n264": (1, 13, 13, 3, 96, 264, 256, "plain", None, ("d1", "d2", "d1"), False),
    "k3-r96-pool": (2, 6, 6, 3, 32, 72, 96, "pool", None, ("d2", "d2", "d2"), False),
    "k1-r256-pool+y2": (2, 6, 6, 1, 96, 264, 256, "pool+y2", None, ("d2", "d2", "d1"), False),
    "k3-r32-reorg": (2, 6, 6, 3, 96, 8, 32, "reorg", None, ("d1", "d2", "d2"), False),
    "k3-r96-slices": (1, 13, 13, 3, 32, 72, 96, "plain", (96, 32, 128, 16), ("d2", "d2", "d2"), False),
    # all-positive draws: H is 864 x 1.6 x 1.6 = 2 300 on average, beyond fp16's exact integers -- its rounding shows
    "k3-r32-bigH": (1, 13, 13, 3, 96, 72, 32, "plain", None, ("d3", "d3", "d1"), True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    B, H, W, k, cin, cout, r, dst, sl, draws, absolute = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    x, u, v = (_draw(gen, DRAWS[d], s) for d, s in zip(draws, ((B, cin, H, W), (r, cin, k, k), (cout, r))))
    if absolute:
        x, u = x.abs(), u.abs()
    scale = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (cout,), generator=gen)]
    shift = torch.randint(-8, 9, (cout,), generator=gen).float() * 0.25
    x_ld, x_choff, y_ld, y_choff = sl or (ops.round_up(cin, 32), 0, ops.round_up((4 if dst == "reorg" else 1) * cout, 8), 0)
    return types.SimpleNamespace(name=name, B=B, H=H, W=W, k=k, cin=cin, cout=cout, r=r, dst=dst, x=x, u=u, v=v, scale=scale,
                                 shift=shift, x_ld=x_ld, x_choff=x_choff, y_ld=y_ld, y_choff=y_choff)


def launch(dev, c, u=None, v=None, overflow=True):
    """One fused launch into NaN-filled destinations; returns the [(slice, everything else)] of y and, when present, y2, and the
    overflow flag (cleared before the launch; overflow=False: the launch gets none, and None is returned).  The full-resolution
    copy lies in y's slice unless the case names one of its own (y2_ld, y2_choff); scale / shift may be None."""
    u, v = (c.u if u is None else u), (c.v if v is None else v)
    r = u.shape[0]
    g = ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, c.x_ld, c.x_choff)
    xbuf = fill_padded(dev, c, c.x.half(), c.x_ld, c.x_choff, ops.round_up(c.cin, 32), 0)
    up, vp = ops.pack_lowrank(g, u.to(dev).contiguous(), v.to(dev).contiguous())
    ho, wo = (c.H, c.W) if c.dst == "plain" else (c.H // 2, c.W // 2)
    nch = 4 * c.cout if c.dst == "reorg" else c.cout
    y = ops.alloc_padded(c.B, ho, wo, c.y_ld, dev)
    whole(y).fill_(float("nan"))
    y2, y2_ld, y2_choff = None, 0, 0
    if c.dst == "pool+y2":
        y2_ld, y2_choff = getattr(c, "y2_ld", 0) or c.y_ld, (c.y2_choff if getattr(c, "y2_ld", 0) else c.y_choff)
        y2 = ops.alloc_padded(c.B, c.H, c.W, y2_ld, dev)
        whole(y2).fill_(float("nan"))
    flag = torch.zeros(1, dtype=torch.int32, device=dev) if overflow else None
    scale, shift = (None if t is None else t.to(dev) for t in (c.scale, c.shift))
    ops.conv_fwd_lowrank(g, r, xbuf, up, vp, y, c.y_ld, c.y_choff, scale, shift, SLOPE, dst_mode=DST[c.dst],
                         y2=y2, y2_ld=y2_ld, y2_choff=y2_choff, overflow=flag)
    torch.cuda.synchronize()
    out = [padded_split(y, c.B, ho, wo, c.y_ld, c.y_choff, nch)]
    if y2 is not None:
        out.append(padded_split(y2, c.B, c.H, c.W, y2_ld, y2_choff, c.cout))
    return out, (int(flag.item()) if overflow else None)


@pytest.mark.parametrize("name", list(CASES))
def test_exact(dev, name):
    c = case(name)
    ref, h, clamped = reference(c)
    assert float(h.abs().max()) * float(c.v.abs().max()) * c.r < 2 ** 24 and float(c.x.abs().max() * c.u.abs().max()) * c.cin * c.k * c.k < 2 ** 24
    if name.endswith("bigH"):        # the rounding of the intermediate must be visible: most of H is beyond 2 048
        assert float((h.abs() > 2048).double().mean()) > 0.5 and not torch.equal(h.half().double(), h)
    outs, flag = launch(dev, c)
    want = {"plain": lambda: [ref], "pool": lambda: [F.max_pool2d(ref.float(), 2, 2).half()], "reorg": lambda: [reorg(ref)],
            "pool+y2": lambda: [F.max_pool2d(ref.float(), 2, 2).half(), ref]}[c.dst]()
    for (got, rest), w in zip(outs, want):
        assert torch.isnan(rest).all(), "an element outside the slice was written"
        assert torch.equal(got, w), "%d of %d elements differ" % (int((got != w).sum()), w.numel())
    assert flag == int(clamped)


def test_rank_padding(dev):
    """r = 96 runs the 128-column instance: it must equal the r = 128 launch whose extra U rows and V columns are zero."""
    c = case("k3-r96-slices")
    u = torch.cat([c.u, torch.zeros(32, c.cin, c.k, c.k)])
    v = torch.cat([c.v, torch.zeros(c.cout, 32)], 1)
    assert ops.conv_fwd_lowrank_info(ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, c.x_ld, c.x_choff), 96).rank_padded == 128
    assert torch.equal(launch(dev, c)[0][0][0], launch(dev, c, u, v)[0][0][0])


@pytest.mark.parametrize("k, r", [(3, 40), (3, 288), (5, 64)])
def test_refusals(dev, k, r):
    g = ops.geom(1, 13, 13, k, 32, 64, 32)
    assert not ops.conv_fwd_lowrank_ok(g, r)
    t = torch.zeros(64, dtype=torch.float16, device=dev)
    with pytest.raises(L.McamdError):
        ops.conv_fwd_lowrank(g, r, t, t, t, t, 64)


def test_gaussian_real_shape(dev):
    """4 x 13 x 13, Cin 512 -> r 256 -> Cout 1024, 3 x 3: the fused launch against the unfused pair of the dense kernels."""
    B, H, W, k, cin, cout, r = 4, 13, 13, 3, 512, 1024, 256
    gen = torch.Generator().manual_seed(5)
    c = types.SimpleNamespace(B=B, H=H, W=W, k=k, cin=cin, cout=cout, r=r, dst="plain", x_ld=cin, x_choff=0, y_ld=cout, y_choff=0,
                              x=torch.randn(B, cin, H, W, generator=gen).half().float(),
                              u=(torch.randn(r, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5).half().float(),
                              v=(torch.randn(cout, r, generator=gen) * (2.0 / r) ** 0.5).half().float(),
                              scale=torch.rand(cout, generator=gen) + 0.5, shift=torch.randn(cout, generator=gen) * 0.2)
    ref = reference(c)[0].double()
    fused = launch(dev, c)[0][0][0]
    g = ops.geom(B, H, W, k, cin, cout, cin)
    gu, gv = ops.geom(B, H, W, k, cin, r, cin), ops.geom(B, H, W, 1, r, cout, r)
    xbuf = fill_padded(dev, c, c.x.half(), cin, 0, cin, 0)
    up, vp = ops.pack_lowrank(g, c.u.to(dev), c.v.to(dev))
    assert torch.equal(up, ops.pack_weights(gu, c.u.to(dev), None, True, False)[0])
    assert torch.equal(vp, ops.pack_weights(gv, c.v.to(dev).view(cout, r, 1, 1).contiguous(), None, True, False)[0])
    hraw = torch.zeros(B * H * W * r, dtype=torch.float16, device=dev)
    ops.conv_fwd_raw(gu, xbuf, up, hraw, r)
    hpad = ops.alloc_padded(B, H, W, r, dev)
    ops.padded_view(hpad, B, H, W, r)[:, 1:-1, 1:-1] = hraw.view(B, H, W, r)
    y = ops.alloc_padded(B, H, W, cout, dev)
    ops.conv_fwd_padded(gv, hpad, vp, y, cout, 0, c.scale.to(dev), c.shift.to(dev), SLOPE)
    torch.cuda.synchronize()
    pair = padded_split(y, B, H, W, cout, 0, cout)[0]
    e_pair, e_fused = rel_l2(pair, ref), rel_l2(fused, ref)
    print("rel-L2 against the float64 reference: pair %.3e, fused %.3e" % (e_pair, e_fused))
    assert e_fused <= 2 * e_pair
