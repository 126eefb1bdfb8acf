"""2:4 packer + sparse forward (mcamd_pack_sparse24 / mcamd_conv_fwd_sparse24, csrc/conv_sparse.hip) at every distinct
conv2-conv22 shape of YOLOv2-VOC at 416x416 (B=1 and B=64) and on ragged geometries: against float64 of the fp16-rounded
masked operands with the same epilogue, and against the dense conv_fwd_padded on the same masked weights."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops, _lib as L  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2, to_padded, padded_to_nchw, halo_is_zero, q16  # noqa: E402

TOL = 1e-3

# (H, cin, cout, k, dst, y2): the distinct conv2-conv22 blocks of yolov2-voc at 416x416 (conv16-18, conv20 repeat shapes)
YOLO = [(208, 32, 64, 3, "pool", False), (104, 64, 128, 3, "plain", False), (104, 128, 64, 1, "plain", False),
        (104, 64, 128, 3, "pool", False), (52, 128, 256, 3, "plain", False), (52, 256, 128, 1, "plain", False),
        (52, 128, 256, 3, "pool", False), (26, 256, 512, 3, "plain", False), (26, 512, 256, 1, "plain", False),
        (26, 256, 512, 3, "pool", True), (13, 512, 1024, 3, "plain", False), (13, 1024, 512, 1, "plain", False),
        (13, 1024, 1024, 3, "plain", False), (26, 512, 64, 1, "reorg", False), (13, 1280, 1024, 3, "plain", False)]
# (B, H, W, cin, cout, k, dst, y2, pad, choff): Cout not a tile multiple, Cin = 1280, channel offsets, both pad forms,
# POOL / REORG with and without y2, 32-channel blocks (cin 96), 256-channel tiles with a ragged last tile
RAGGED = [(2, 13, 13, 1280, 1024, 3, "plain", False, 1, 0), (2, 9, 11, 96, 200, 3, "plain", False, 0, 32),
          (3, 10, 14, 64, 72, 3, "pool", False, 1, 0), (2, 12, 12, 256, 136, 1, "reorg", False, 0, 64),
          (2, 26, 26, 256, 512, 3, "pool", True, 1, 32), (1, 13, 13, 40, 48, 1, "plain", False, 0, 8),
          (2, 20, 20, 96, 64, 3, "pool", True, 0, 0), (2, 26, 26, 512, 64, 1, "reorg", False, 1, 0),
          (2, 11, 13, 128, 264, 3, "plain", False, 0, 16), (3, 14, 10, 192, 392, 1, "pool", True, 1, 8)]


def mask24(cout, cin, k, gen):
    """Random 2:4 mask along the input channels whose groups hold 0, 1 or 2 kept entries."""
    g = cin // 4
    nkeep = torch.randint(0, 3, (cout, g, k, k), generator=gen)
    order = torch.rand(cout, g, k, k, 4, generator=gen).argsort(-1)
    keep = order < nkeep.unsqueeze(-1)                           # the first nkeep positions of a random permutation
    return keep.float().permute(0, 1, 4, 2, 3).reshape(cout, cin, k, k).contiguous()


def run_case(dev, B, H, W, cin, cout, k, dst, dual, pad, choff, seed, ref_images=None):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=gen)
    w = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    mask = mask24(cout, cin, k, gen)
    scale, shift = torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.2
    ld = ops.round_up(choff + ops.round_up(cin, 32), 32)
    xb, _ = to_padded(x.to(dev), ld=ld, choff=choff, pad=pad)
    g = ops.geom(B, H, W, k, cin, cout, ld, choff, 0, pad)
    assert ops.conv_fwd_sparse24_ok(g)
    wd, md = w.to(dev).contiguous(), mask.to(dev).contiguous()
    wsp, idx = ops.pack_sparse24(g, wd, md)
    wp, _ = ops.pack_weights(g, wd, md, True, False)
    mode = {"plain": L.DST_PLAIN, "pool": L.DST_POOL, "reorg": L.DST_REORG}[dst]
    Ho, Wo = (H, W) if dst == "plain" else (H // 2, W // 2)
    cdst = 4 * cout if dst == "reorg" else cout
    off = 8
    dld = ops.round_up(off + cdst + 8, 32)
    y2ld = ops.round_up(cout + 40, 32)
    outs = {}
    for name in ("sparse", "dense"):
        y = ops.alloc_padded(B, Ho, Wo, dld, dev)
        y2 = ops.alloc_padded(B, H, W, y2ld, dev) if dual else None
        kw = dict(dst_mode=mode, y2=y2, y2_ld=y2ld if dual else 0, y2_choff=32 if dual else 0)
        if name == "sparse":
            ops.conv_fwd_sparse24(g, xb, wsp, idx, y, dld, off, scale.to(dev), shift.to(dev), 0.1, **kw)
        else:
            ops.conv_fwd_padded(g, xb, wp, y, dld, off, scale.to(dev), shift.to(dev), 0.1, **kw)
        outs[name] = (y, y2)
    y, y2 = outs["sparse"]
    got = padded_to_nchw(y, B, Ho, Wo, dld, cdst, off)
    dense = padded_to_nchw(outs["dense"][0], B, Ho, Wo, dld, cdst, off)
    assert rel_l2(got, dense) < TOL, "sparse vs dense conv_fwd_padded"
    assert halo_is_zero(y, B, Ho, Wo, dld)
    v = ops.padded_view(y, B, Ho, Wo, dld)
    assert float(v[..., :off].abs().sum()) == 0 and float(v[..., off + cdst:].abs().sum()) == 0, "out-of-slice channels"
    imgs = list(range(B)) if ref_images is None else ref_images
    xs = q16(x[imgs]).double()
    act = F.leaky_relu(F.conv2d(xs, q16(w * mask).double(), None, 1, (k - 1) // 2) * scale.double().view(1, -1, 1, 1)
                       + shift.double().view(1, -1, 1, 1), 0.1)
    ref = act if dst == "plain" else (F.max_pool2d(act, 2, 2) if dst == "pool" else O.reorg(act, 2))
    assert rel_l2(got[imgs], ref) < TOL, "sparse vs float64"
    if dual:
        got2 = padded_to_nchw(y2, B, H, W, y2ld, cout, 32)
        assert rel_l2(got2[imgs], act) < TOL
        assert halo_is_zero(y2, B, H, W, y2ld)
        v2 = ops.padded_view(y2, B, H, W, y2ld)
        assert float(v2[..., :32].abs().sum()) == 0 and float(v2[..., 32 + cout:].abs().sum()) == 0
        assert torch.equal(got, F.max_pool2d(got2, 2, 2))


@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("case", YOLO, ids=["%d-%d-%d-k%d-%s%s" % (c[0], c[1], c[2], c[3], c[4], "-y2" if c[5] else "")
                                            for c in YOLO])
def test_sparse24_yolov2_shapes(dev, B, case):
    H, cin, cout, k, dst, dual = case
    # B=64: the float64 reference on the first and the last image (the highest addresses), the dense kernel on all
    run_case(dev, B, H, H, cin, cout, k, dst, dual, 0, 0, seed=H + cin + cout, ref_images=None if B == 1 else [0, B - 1])


@pytest.mark.parametrize("case", RAGGED)
def test_sparse24_ragged(dev, case):
    run_case(dev, *case, seed=sum(case[:6]))


def test_pack_sparse24_layout(dev):
    """The packing itself: kept values in k order, 2-bit offsets, distinct zero-valued slots for groups with < 2 kept."""
    cout, cin, k = 8, 64, 1
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(cout, cin, k, k, generator=gen)
    mask = mask24(cout, cin, k, gen)
    g = ops.geom(1, 4, 4, k, cin, cout, 64)
    vals, idx = ops.pack_sparse24(g, w.to(dev).contiguous(), mask.to(dev).contiguous())
    npad, ktot = 256, 64
    vals = vals.view(npad, ktot // 2).cpu()
    idx = idx.view(ktot // 32, npad, 2).cpu().to(torch.int32) & 0xFFFF
    wm = (w * mask).half().view(cout, cin)
    for n in range(cout):
        for grp in range(cin // 4):
            q, h, gg = grp // 8, (grp // 4) % 2, grp % 4
            word = int(idx[q, n, h])
            p0, p1 = (word >> (4 * gg)) & 3, (word >> (4 * gg + 2)) & 3
            assert p0 < p1
            kept = {4 * grp + p0: vals[n, 2 * grp], 4 * grp + p1: vals[n, 2 * grp + 1]}
            for e in range(4):
                c = 4 * grp + e
                assert float(kept.get(c, 0.0)) == float(wm[n, c]), (n, c)
    assert bool((vals[cout:] == 0).all())
