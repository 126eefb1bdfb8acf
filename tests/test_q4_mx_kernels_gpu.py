"""mcamd_cast_a4_mx and the three kernel instances mcamd_conv_fwd_q4_mx can launch (csrc/conv_q4_mx.hip): MXFP4
activations x MXFP4 weights on the block-scaled MFMA.

  1. the cast pass equals a4_ref byte for byte, every destination byte written and none beyond;
  2. one non-zero activation channel per pixel pins B's nibble order, its lane -> k map and the scale byte per (pixel, half);
  3. on integer draws the cast represents losslessly the output equals the float64 reference code for code, on every instance;
  4. on Gaussian operands it stays as close to float64 as mcamd_conv_fwd_q8_w4_mx on the bytes the activation codes stand for
     (test_q8_w4_mx_kernels_gpu's bound against that baseline), and two launches are bit-equal.

The helpers are test_q8_instances_gpu's and test_q8_w4_mx_kernels_gpu's."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
import a4_ref as A  # noqa: E402
import q8_cases as QC  # noqa: E402
import q8_ref as R  # noqa: E402
import w4_cases as WC  # noqa: E402
import w4_ref as W  # noqa: E402
import test_q8_instances_gpu as T  # noqa: E402  (helpers only)
import test_q8_w4_kernels_gpu as K  # noqa: E402  (helpers only: _same)
import test_q8_w4_mx_kernels_gpu as MX  # noqa: E402  (helpers only: _pack, _launch, _distance)
from util import NAN8, NAN, padded_split, is_sentinel  # noqa: E402

pytestmark = pytest.mark.gpu


def _case(name, B, H, W, k, cin, cout, **kw):
    bmw = 256 if cout >= 256 else 128 if cout >= 128 else 64
    return QC.case("q4-" + name, "dense", B, H, W, k, cin, cout, ("dense", 1, bmw), mfma=1, **kw)


# (the issue's shapes: nine chunks with image-boundary halos, fewer chunks than the ring is deep, eight chunks; every tile, N off
# the tile; a pool, an e4m3 and a y2 destination; an operand slice inside a wider buffer)
CASES = [_case("3x3-5x5", 2, 5, 5, 3, 64, 72, fmt="f8", draw="d1"),
         _case("3x3-13x13", 2, 13, 13, 3, 64, 264, fmt="f8", draw="d1", y_choff=8, y_ld=288),
         _case("1x1-cin128-pool", 2, 12, 14, 1, 128, 128, dst="pool", fmt="f16", draw="d2"),
         _case("1x1-cin512", 2, 13, 13, 1, 512, 64, fmt="f8", draw="d1"),
         _case("3x3-pool+y2", 2, 12, 14, 3, 64, 256, dst="pool+y2", fmt="f8", ld=128, choff=32, y2_choff=16, y2_ld=288, draw="d1")]


def _operands(c, gaussian=False):
    """w4_cases.operands with, on the integer draws, every odd group of 32 activation channels doubled: the shifts differ
    between the groups of a chunk on both sides, and the cast still represents every value."""
    o = WC.operands(c, gaussian=gaussian)
    if gaussian:
        return o
    x = R.deq(o.a8)
    x[:, (torch.arange(c.cin) // 32) % 2 == 1] *= 2.0
    return o._replace(a8=R.q(x), scale=o.scale)


def _rows(c, a8):
    """[B][cin][H][W] codes -> the padded buffer's rows [B (H + 2) (W + 2)][cin], zero halo"""
    return torch.nn.functional.pad(a8, (1, 1, 1, 1)).permute(0, 2, 3, 1).reshape(-1, c.cin)


def _launch(dev, c, o, packed):
    """One cast + one launch into sentinel-filled outputs, as MX._launch returns them."""
    g = QC.geom_of(c)
    xc, xs = ops.cast_a4_mx(T._input(dev, c, o), c.B * (c.H + 2) * (c.W + 2), c.ld or c.cin, c.choff, c.cin)
    Ho, Wo = (c.H, c.W) if c.dst == "plain" else (c.H // 2, c.W // 2)
    y_ld = c.y_ld or ops.round_up(c.cdst, 32)
    y = T._alloc(dev, c.B, Ho, Wo, y_ld, c.fmt_y)
    y2, (y2_ld, y2_choff) = None, (0, 0)
    if c.dst == "pool+y2":
        y2_ld, y2_choff = c.y2_slice
        y2 = T._alloc(dev, c.B, c.H, c.W, y2_ld, c.fmt_y2)
    ops.conv_fwd_q4_mx(g, xc, xs, *packed, y, y_ld, c.y_choff, scale=T._dev(o.scale, dev), shift=T._dev(o.shift, dev), slope=c.slope,
                       dst_mode=QC.DSTS[c.dst], y2=y2, y2_ld=y2_ld, y2_choff=y2_choff, y_f8=c.fmt_y == "f8", y2_f8=c.fmt_y2 == "f8")
    torch.cuda.synchronize()
    out = {"y": padded_split(y, c.B, Ho, Wo, y_ld, c.y_choff, c.cdst, NAN8 if c.fmt_y == "f8" else NAN)}
    if y2 is not None:
        out["y2"] = padded_split(y2, c.B, c.H, c.W, y2_ld, y2_choff, c.cout, NAN8 if c.fmt_y2 == "f8" else NAN)
    return out


def _info(c):
    r = ops.conv_fwd_q4_mx_info(QC.geom_of(c))
    assert (r.f8mfma, r.bmw, r.stages) == c.expect[1:] + (4,), (c.name, r)
    return r


# ------------------------------------------------------------------------------------------------ 1. the cast pass
@pytest.mark.parametrize("cin, ld, choff", [(64, 64, 0), (192, 192, 0), (192, 256, 64)])
def test_cast_equals_the_restatement(dev, cin, ld, choff):
    gen = torch.Generator().manual_seed(cin + choff)
    finite = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8)
    a8 = finite[torch.randint(0, 254, (2, cin, 5, 5), generator=gen)]
    a8[1, 32:64, 2, 3] = 0                                   # an all-zero group inside the image
    c = _case("cast", 2, 5, 5, 1, cin, 64)
    rows = _rows(c, a8)
    buf = torch.full((rows.shape[0], ld), 0x7F, dtype=torch.uint8)   # (NaN bytes around the slice: never read)
    buf[:, choff:choff + cin] = rows
    nc, ns = ops.a4_mx_elems(rows.shape[0], cin)
    oc, osc = (torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=dev) for n in (nc, ns))
    ops.cast_a4_mx(buf.to(dev), rows.shape[0], ld, choff, cin, oc, osc)
    codes, scales, _ = A.cast(rows)
    want_c, want_s = A.packed(codes, scales)
    assert torch.equal(oc[:nc].cpu().view(want_c.shape), want_c), "codes"
    assert torch.equal(osc[:ns].cpu().view(want_s.shape), want_s), "scale words"
    assert bool((oc[nc:] == 0xAB).all()) and bool((osc[ns:] == 0xAB).all()), "nothing beyond the destinations is written"


# ------------------------------------------------------------------------------------------------ 2. one-hot
@pytest.mark.parametrize("k, cin", [(1, 128), (3, 64)])
def test_q4_onehot(dev, k, cin):
    """Pixel p of a 12 x 12 image holds 2^(group - 1) in channel p % cin alone (scale bytes 124 + group, distinct within a chunk);
    the weights are signed integers of the grid, different from channel to channel and tap to tap."""
    c = _case("onehot-k%d" % k, 1, 12, 12, k, cin, 64, fmt="f16", slope=1.0)
    _info(c)
    gen = torch.Generator().manual_seed(k)
    ch = torch.arange(144) % cin
    x = torch.zeros(144, cin)
    x[torch.arange(144), ch] = torch.pow(2.0, (ch // 32).float() - 1.0)
    a8 = R.q(x.view(1, 12, 12, cin).permute(0, 3, 1, 2).contiguous())
    w = QC._draw(gen, (-6, -4, -3, -2, -1, 1, 2, 3, 4, 6), (64, cin, k, k))
    o = QC.Operands(a8, None, w, None, None, torch.ones(64), torch.zeros(64), None, [])
    ref, _ = WC.reference(c, o)
    assert torch.equal(R.deq(ref.w8).double() * torch.pow(2.0, -ref.e.double()).view(-1, 1, 1, 1), w.double()), "integer weight codes"
    got, rest = _launch(dev, c, o, MX._pack(dev, c, o))["y"]
    bad = (got.double() != ref.y.double()).nonzero()
    assert bad.numel() == 0, "%d outputs name the wrong (filter, k); first (image, filter, y, x) %s" % (bad.shape[0], bad[0].tolist())
    T._assert_untouched(c, "y", rest)


# ------------------------------------------------------------------------------------------------ 3. exact against float64
@pytest.mark.parametrize("c", CASES, ids=str)
def test_q4_instance_exact(dev, c):
    r = _info(c)
    o = _operands(c)
    rows = _rows(c, o.a8)
    assert torch.equal(A.cast(rows)[2], rows), "the cast represents the draws losslessly"
    assert len(set(A.cast(rows)[1][c.W + 3].tolist())) > 1, "the shifts differ between the groups of a pixel"
    ref, _ = WC.reference(c, o)
    assert QC.exactness(c, o, ref) == [], c.name             # on the reference's operands, never from kernel output
    out = _launch(dev, c, o, MX._pack(dev, c, o))
    for name, want in (("y", ref.y), ("y2", ref.y2)):
        if want is not None:
            T._assert_equal(c, r, name, out[name][0], want)
            T._assert_untouched(c, name, out[name][1])


# ------------------------------------------------------------------------------------------------ 4. Gaussian operands
@pytest.mark.parametrize("c", CASES, ids=str)
def test_q4_gaussian_against_float64_and_the_fp8_activation_kernel(dev, c):
    o = _operands(c, gaussian=True)
    back = A.cast(_rows(c, o.a8))[2].view(c.B, c.H + 2, c.W + 2, c.cin)[:, 1:-1, 1:-1].permute(0, 3, 1, 2).contiguous()
    o = o._replace(a8=back)                                  # the bytes the activation codes stand for: the cast is lossless on them
    _, _, e4, _, w8 = W.quantise(o.w, o.mask)
    v = R.block(o.a8, w8, e4, o.scale, o.shift, c.slope, dtype=torch.float64)
    store = lambda fmt, dst: R.store_bytes(v, dst) if fmt == "f8" else R.store_fp16(v, dst)
    want = {"y": store(c.fmt_y, "pool" if c.dst == "pool+y2" else c.dst)}
    if c.dst == "pool+y2":
        want["y2"] = store(c.fmt_y2, "plain")
    packed = MX._pack(dev, c, o)
    new, again = _launch(dev, c, o, packed), _launch(dev, c, o, packed)
    base, _ = MX._launch(dev, c, o, packed)
    for what in want:
        (n_new, d_new), (n_base, d_base) = MX._distance(new[what][0], want[what]), MX._distance(base[what][0], want[what])
        print("%s %s: of %d elements the fp4 x fp4 kernel differs from float64 in %d (largest %.3g), mcamd_conv_fwd_q8_w4_mx on the "
              "same values in %d (largest %.3g)" % (c.name, what, want[what].numel(), n_new, d_new, n_base, d_base))
        assert not bool(is_sentinel(new[what][0]).any()) and K._same(new[what][0], again[what][0]), "two launches are bit-equal"
        assert n_new <= 2 * n_base + 2, (c.name, what)
        if want[what].dtype == torch.uint8:
            assert R.byte_mismatch(new[what][0], want[what])[1], "%s %s: a byte is more than one code from the reference" % (c.name, what)
        else:
            assert d_new <= 2.0 * d_base, (c.name, what)
