"""mcamd_pack_q8_w4_mx, mcamd_unpack_q8_w4_mx and the three kernel instances mcamd_conv_fwd_q8_w4_mx can launch
(csrc/conv_q8_w4_mx.hip): the 4-bit codes as the fp4 operand of the block-scaled MFMA.

  1. the packer's codes, scale bytes and exponents, read through the layout include/mcamd.h states, are w4_ref's; the expander's
     bytes equal mcamd_unpack_q8_w4's of mcamd_pack_q8_w4, pad rows included;
  2. one-hot filters pin the nibble order, the lane -> k map of both operands and the scale byte;
  3. on integer draws (with 5 and 7, shifts that differ between groups) the output equals the float64 reference code for code;
  4. on Gaussian operands it stays as close to the float64 reference as mcamd_conv_fwd_q8_w4 under MCAMD_Q8_MFMA=1 does (the
     bound is the issue's: no byte more than one code off, at most twice the baseline's count of differing elements + 2, at
     most twice its largest fp16 relative error);
  5. two launches are bit-equal.

The cases are w4_cases' on the fp8-MFMA instances; the helpers are test_q8_instances_gpu's and test_q8_w4_kernels_gpu's."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
import q8_cases as QC  # noqa: E402
import q8_ref as R  # noqa: E402
import w4_cases as WC  # noqa: E402
import w4_ref as W  # noqa: E402
import test_q8_instances_gpu as T  # noqa: E402  (helpers only)
import test_q8_w4_kernels_gpu as K  # noqa: E402  (helpers only: _pack_sets, _pack, _launch, _same)
from util import NAN8, NAN, padded_split, is_sentinel  # noqa: E402

pytestmark = pytest.mark.gpu

MX_CASES = [c for c in WC.CASES if c.expect[1] == 1]


def _info(c):
    r = ops.conv_fwd_q8_w4_mx_info(QC.geom_of(c))
    assert (r.f8mfma, r.bmw) == c.expect[1:], (c.name, r)
    return r


def _pack(dev, c, o):
    return ops.pack_q8_w4_mx(QC.geom_of(c), T._dev(o.w, dev), T._dev(o.mask, dev))


def _launch(dev, c, o, packed, xb=None):
    """K._launch for mcamd_conv_fwd_q8_w4_mx: one launch into sentinel-filled outputs."""
    g = QC.geom_of(c)
    xb = T._input(dev, c, o) if xb is None else xb
    Ho, Wo = (c.H, c.W) if c.dst == "plain" else (c.H // 2, c.W // 2)
    y_ld = c.y_ld or ops.round_up(c.cdst, 32)
    y = T._alloc(dev, c.B, Ho, Wo, y_ld, c.fmt_y)
    y2, y2_ld, y2_choff = None, 0, 0
    if c.dst == "pool+y2":
        y2_ld, y2_choff = c.y2_slice
        y2 = T._alloc(dev, c.B, c.H, c.W, y2_ld, c.fmt_y2)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.conv_fwd_q8_w4_mx(g, xb, *packed, y, y_ld, c.y_choff, scale=T._dev(o.scale, dev), shift=T._dev(o.shift, dev), slope=c.slope,
                          dst_mode=QC.DSTS[c.dst], y2=y2, y2_ld=y2_ld, y2_choff=y2_choff, y_f8=c.fmt_y == "f8", y2_f8=c.fmt_y2 == "f8",
                          overflow=flag)
    torch.cuda.synchronize()
    out = {"y": padded_split(y, c.B, Ho, Wo, y_ld, c.y_choff, c.cdst, NAN8 if c.fmt_y == "f8" else NAN)}
    if y2 is not None:
        out["y2"] = padded_split(y2, c.B, c.H, c.W, y2_ld, y2_choff, c.cout, NAN8 if c.fmt_y2 == "f8" else NAN)
    return out, int(flag.item())


# ------------------------------------------------------------------------------------------------ 1. packer and expander
@pytest.mark.parametrize("name, w, mask", K._pack_sets(), ids=lambda v: v if isinstance(v, str) else "")
def test_mx_packer_and_expander(dev, name, w, mask):
    cout, cin, k, _ = w.shape
    g = ops.geom(1, 8, 8, k, cin, cout, cin)
    codes_r, g_r, e4_r, values, bytes_r = W.quantise(w, mask)
    npad, ktot = ops.round_up(cout, 256), cin * k * k
    wd, md = w.to(dev).contiguous(), mask.to(dev).contiguous() if mask is not None else None
    # (destinations pre-filled: every row up to Npad must be written)
    oc = torch.full((npad * ktot // 2,), 0xAB, dtype=torch.uint8, device=dev)
    og = torch.full((npad * ktot // 32,), 0xAB, dtype=torch.uint8, device=dev)
    oe = torch.full((npad,), -77, dtype=torch.int32, device=dev)
    codes, scales, wexp = ops.pack_q8_w4_mx(g, wd, md, oc, og, oe)
    wq = ops.unpack_q8_w4_mx(g, codes, scales, torch.full((npad * ktot,), 0xAB, dtype=torch.uint8, device=dev))
    old = ops.pack_q8_w4(g, wd, md)
    assert torch.equal(wq, ops.unpack_q8_w4(g, old[0], old[1])), "expanded bytes = mcamd_unpack_q8_w4's of mcamd_pack_q8_w4"
    codes, scales, wexp = codes.cpu().view(npad, ktot // 2), scales.cpu().view(ktot // 64, npad, 2), wexp.cpu()
    assert torch.equal(wexp[:cout], e4_r), "exponents"
    assert torch.equal(scales[:, :cout], W.shift_rows(g_r) + 122), "scale bytes = 127 + g"
    # the header's layout: byte i of a row holds position 2 i of mcamd_pack_q8's order in its low nibble, 2 i + 1 in its high one
    got = torch.stack((codes[:cout] & 0x0F, codes[:cout] >> 4), 2).reshape(cout, ktot)
    bad = got != W.dense_rows(codes_r)
    assert not bool(bad.any()), "%d of %d codes differ; first (filter, k) %s" % (int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
    assert not bool(codes[cout:].any()) and bool((scales[:, cout:] == 127).all()) and not bool(wexp[cout:].any()), "pad rows"


# ------------------------------------------------------------------------------------------------ 2. one-hot
@pytest.mark.parametrize("h", K.ONEHOT, ids=QC.onehot_id)
def test_mx_onehot(dev, h):
    """K.test_w4_onehot on the fp4 operand: every filter selects exactly its own (channel, tap) with the right sign and value
    (the weight 1 = 4 * 2^5 * 2^-7: code 6, scale byte 132, every other group zero codes with scale byte 122)."""
    c = QC.onehot_case(h, 1)
    r = _info(c)
    a8, w, which = QC.onehot_operands(h)
    o = QC.Operands(a8, None, w, None, None, None, None, None, [])
    want = F.conv2d(R.deq(a8).double(), w.double(), None, 1, (c.k - 1) // 2) / 2.0
    out, flag = _launch(dev, c, o, _pack(dev, c, o))
    got, rest = out["y"]
    bad = [(f, which[f], [float(got[i, f, 1, 1]) for i in (0, 1)], [float(want[i, f, 1, 1]) for i in (0, 1)]) for f in range(c.cout)
           if not all(float(got[i, f, 1, 1]) == float(want[i, f, 1, 1]) for i in (0, 1))]
    assert not bad, "%s: %d of %d filters select the wrong k; first (filter, (channel, tap, sign), got, want): %s" % (
        c.name, len(bad), c.cout, bad[:8])
    T._assert_equal(c, r, "y", got, want.float())
    T._assert_untouched(c, "y", rest)
    assert flag == 0


# ------------------------------------------------------------------------------------------------ 3. exact against float64
@pytest.mark.parametrize("c", MX_CASES, ids=str)
def test_mx_instance_exact(dev, c):
    r = _info(c)
    o, ref, _ = WC.operands_and_reference(c)
    assert QC.exactness(c, o, ref) == [], c.name            # on the reference's operands, never from kernel output
    packed = _pack(dev, c, o)
    assert torch.equal(packed[2][:c.cout].cpu(), ref.e), "exponents"
    out, flag = _launch(dev, c, o, packed)
    for name, want in (("y", ref.y), ("y2", ref.y2)):
        if want is not None:
            T._assert_equal(c, r, name, out[name][0], want)
            T._assert_untouched(c, name, out[name][1])
    assert flag == 0


# ------------------------------------------------------------------------------------------------ 4. Gaussian operands
def _distance(got, want):
    """(elements that differ, the largest distance: in codes for bytes, relative for fp16 values) from the reference's store"""
    if got.dtype == torch.uint8:
        return int((got != want).sum()), float((R.ordinal(got) - R.ordinal(want)).abs().max())
    g, w = got.double(), want.half().double()
    return int((g != w).sum()), float(((g - w).abs() / w.abs().clamp_min(2.0 ** -14)).max())


@pytest.mark.parametrize("c", MX_CASES, ids=str)
def test_mx_gaussian_against_float64_and_the_decode_kernel(dev, c, setenv):
    QC.apply_env(c, setenv)                                  # MCAMD_Q8_MFMA=1: the baseline's form (the new kernel does not read it)
    _info(c)
    o = WC.operands(c, gaussian=True)
    _, _, e4, _, w8 = W.quantise(o.w, o.mask)
    v = R.block(o.a8, w8, e4, o.scale, o.shift, c.slope, dtype=torch.float64)
    store = lambda fmt, dst: R.store_bytes(v, dst) if fmt == "f8" else R.store_fp16(v, dst)
    want = {"y": store(c.fmt_y, "pool" if c.dst == "pool+y2" else c.dst)}
    if c.dst == "pool+y2":
        want["y2"] = store(c.fmt_y2, "plain")
    xb = T._input(dev, c, o)
    new, _ = _launch(dev, c, o, _pack(dev, c, o), xb=xb)
    base, _ = K._launch(dev, c, o, K._pack(dev, c, o), xb=xb)
    for what in want:
        (n_new, d_new), (n_base, d_base) = _distance(new[what][0], want[what]), _distance(base[what][0], want[what])
        print("%s %s: of %d elements the fp4 kernel differs from float64 in %d (largest %.3g), the decode kernel in %d (largest %.3g); "
              "the two kernels bit-equal: %s" % (c.name, what, want[what].numel(), n_new, d_new, n_base, d_base,
                                                 K._same(new[what][0], base[what][0])))
        assert not bool(is_sentinel(new[what][0]).any()) and K._same(new[what][1], base[what][1]), what
        assert n_new <= 2 * n_base + 2, (c.name, what)
        if want[what].dtype == torch.uint8:
            assert R.byte_mismatch(new[what][0], want[what])[1], "%s %s: a byte is more than one code from the reference" % (c.name, what)
        else:
            assert d_new <= 2.0 * d_base, (c.name, what)


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_mx_is_deterministic(dev):
    c = next(c for c in MX_CASES if c.name in WC.DETERMINISM_CASES)
    o = WC.operands(c, gaussian=True)
    p1, p2 = _pack(dev, c, o), _pack(dev, c, o)
    assert all(torch.equal(x, y) for x, y in zip(p1, p2)), "the packer is deterministic"
    a, _ = _launch(dev, c, o, p1)
    b, _ = _launch(dev, c, o, p1)
    for what in a:
        assert not bool(is_sentinel(a[what][0]).any()) and K._same(a[what][0], b[what][0]), what
