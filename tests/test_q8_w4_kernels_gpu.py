"""mcamd_pack_q8_w4, mcamd_unpack_q8_w4 and every kernel instance mcamd_conv_fwd_q8_w4 can launch (csrc/conv_q8_w4.hip), in
both MFMA forms (MCAMD_Q8_MFMA 0 / 1).  There is no tolerance in this file:

  1. the packer's codes, shifts and exponents, read through the layout include/mcamd.h states, are w4_ref's; the expander's
     bytes are w4_ref's bytes in mcamd_pack_q8's layout, pad rows included;
  2. one-hot filters pin the nibble order and the lane -> k map;
  3. on Gaussian operands the kernel equals mcamd_conv_fwd_q8 on the expanded bytes with the same exponents, bit for bit --
     the operands and the MFMA sequence per accumulator are identical by construction;
  4. on integer draws (with 5 and 7, which the grid cannot hold) it equals the float64 reference on w4_ref's bytes, code for
     code (the conditions of exactness are asserted on the reference's operands, here and in test_q8_w4_cpu.py);
  5. two launches are bit-equal.

Sentinels as in test_q8_instances_gpu.py, whose launch helpers this file shares."""
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
import test_q8_instances_gpu as T  # noqa: E402  (helpers only: _input, _alloc, _launch, _assert_equal, _assert_untouched)
from util import NAN8, NAN, padded_split, is_sentinel  # noqa: E402

pytestmark = pytest.mark.gpu


def _check_info(c, setenv):
    QC.apply_env(c, setenv)
    r = WC.info_of(c)
    assert (r.f8mfma, r.bmw) == c.expect[1:], (c.name, r)
    return r


def _pack(dev, c, o):
    return ops.pack_q8_w4(QC.geom_of(c), T._dev(o.w, dev), T._dev(o.mask, dev))


def _launch(dev, c, o, packed, xb=None):
    """T._launch for mcamd_conv_fwd_q8_w4: one launch into sentinel-filled outputs."""
    g = QC.geom_of(c)
    xb = T._input(dev, c, o) if xb is None else xb
    codes, gshift, wexp = packed
    Ho, Wo = (c.H, c.W) if c.dst == "plain" else (c.H // 2, c.W // 2)
    y_ld = c.y_ld or ops.round_up(c.cdst, 32)
    y = T._alloc(dev, c.B, Ho, Wo, y_ld, c.fmt_y)
    y2, y2_ld, y2_choff = None, 0, 0
    if c.dst == "pool+y2":
        y2_ld, y2_choff = c.y2_slice
        y2 = T._alloc(dev, c.B, c.H, c.W, y2_ld, c.fmt_y2)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.conv_fwd_q8_w4(g, xb, codes, gshift, wexp, y, y_ld, c.y_choff, scale=T._dev(o.scale, dev), shift=T._dev(o.shift, dev),
                       slope=c.slope, dst_mode=QC.DSTS[c.dst], y2=y2, y2_ld=y2_ld, y2_choff=y2_choff, y_f8=c.fmt_y == "f8",
                       y2_f8=c.fmt_y2 == "f8", overflow=flag)
    torch.cuda.synchronize()
    out = {"y": padded_split(y, c.B, Ho, Wo, y_ld, c.y_choff, c.cdst, NAN8 if c.fmt_y == "f8" else NAN)}
    if y2 is not None:
        out["y2"] = padded_split(y2, c.B, c.H, c.W, y2_ld, y2_choff, c.cout, NAN8 if c.fmt_y2 == "f8" else NAN)
    return out, int(flag.item())


def _same(a, b):
    """bit equality of two fp16 / uint8 tensors (NaN sentinels included)"""
    return torch.equal(T._bits(a), T._bits(b))


# ------------------------------------------------------------------------------------------------ 1. packer and expander
def _pack_sets():
    gen = torch.Generator().manual_seed(4)
    w1 = torch.randn(72, 64, 3, 3, generator=gen) * 0.04
    w2 = torch.randn(136, 128, 1, 1, generator=gen) * 0.1
    w3 = WC.adversarial(gen)
    w4 = torch.randn(72, 128, 3, 3, generator=gen) * 0.03
    m4 = (torch.rand(w4.shape, generator=gen) > 0.5).float()
    m4[7] = 0.0
    m4[9, 32:64] = 0.0
    return [("gauss-72x64x3", w1, None), ("gauss-136x128x1", w2, None), ("adversarial", w3, None), ("masked", w4, m4)]


@pytest.mark.parametrize("name, w, mask", _pack_sets(), ids=lambda v: v if isinstance(v, str) else "")
def test_packer_and_expander_equal_the_reference(dev, name, w, mask):
    cout, cin, k, _ = w.shape
    g = ops.geom(1, 8, 8, k, cin, cout, cin)
    codes_r, g_r, e4_r, values, bytes_r = W.quantise(w, mask)
    npad, ktot = ops.round_up(cout, 256), cin * k * k
    assert ops.q8_w4_elems(g) == (npad * ktot // 2, npad * ktot // 32, npad)
    # (destinations pre-filled: every row up to Npad must be written)
    oc = torch.full((npad * ktot // 2,), 0xAB, dtype=torch.uint8, device=dev)
    og = torch.full((npad * ktot // 32,), 0xAB, dtype=torch.uint8, device=dev)
    oe = torch.full((npad,), -77, dtype=torch.int32, device=dev)
    codes, gshift, wexp = ops.pack_q8_w4(g, w.to(dev).contiguous(), mask.to(dev).contiguous() if mask is not None else None, oc, og, oe)
    wq = torch.full((npad * ktot,), 0xAB, dtype=torch.uint8, device=dev)
    ops.unpack_q8_w4(g, codes, gshift, wq)
    torch.cuda.synchronize()
    codes, gshift, wexp, wq = codes.cpu().view(npad, ktot // 2), gshift.cpu().view(ktot // 64, npad, 2), wexp.cpu(), wq.cpu().view(npad, ktot)
    assert torch.equal(wexp[:cout], e4_r), "exponents"
    bad = gshift[:, :cout] != W.shift_rows(g_r)
    assert not bool(bad.any()), "%d shift bytes differ; first (chunk, filter, group) %s" % (int(bad.sum()), bad.nonzero()[0].tolist())
    got = W.codes_of_rows(codes[:cout], cin, k)
    bad = got != W.dense_rows(codes_r)
    assert not bool(bad.any()), "%d of %d codes differ; first (filter, k) %s" % (int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
    assert torch.equal(codes[:cout], W.code_rows(codes_r)), "code rows, byte for byte"
    assert not bool(codes[cout:].any()) and not bool(gshift[:, cout:].any()) and not bool(wexp[cout:].any()), "pad rows"
    assert torch.equal(wq[:cout], W.dense_rows(bytes_r)), "expanded bytes = the reference's, in pack_q8's layout"
    assert not bool(wq[cout:].any()), "expanded pad rows are zero bytes"
    # ... and pack_q8 of the dequantised weights gives exactly twice these values with exponent e4 + 1 (the model test's argument)
    wd = W.dequantised(values, e4_r)
    w8, e8 = ops.pack_q8(g, wd.to(dev).contiguous())
    live = values.flatten(1).abs().amax(1) > 0
    assert torch.equal(e8[:cout].cpu()[live], e4_r[live] + 1)
    assert torch.equal(R.deq(w8.cpu().view(npad, ktot)[:cout]).double(), 2.0 * W.dense_rows(values) * live.view(-1, 1))


# ------------------------------------------------------------------------------------------------ 2. one-hot
ONEHOT = [h for h in QC.ONEHOT_CASES if h.fam == "dense"]


@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("h", ONEHOT, ids=QC.onehot_id)
def test_w4_onehot(dev, h, mfma, setenv):
    """q8_cases.onehot_operands: every filter keeps ONE weight +-1 at its own (channel, tap) -- the value 1 = 128 * 2^-7: e4 = 7,
    its group's shift 5, grid entry 4 (index 6), every other group all zero with shift -5 -- and between them the filters
    select every k of the packed order; the centre pixel names channel (image 0) and tap (image 1).  Pins the nibble order,
    the group of every k and the lane -> k map in both forms."""
    c = QC.onehot_case(h, mfma)
    r = _check_info(c, setenv)
    a8, w, which = QC.onehot_operands(h)
    o = QC.Operands(a8, None, w, None, None, None, None, None, [])
    codes, g, e4, values, b = W.quantise(w)
    assert bool((e4 == 7).all()) and set(codes.flatten().tolist()) == {0, 6, 14} and set(R.deq(b).flatten().tolist()) == {0.0, 128.0, -128.0}
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


# ------------------------------------------------------------------------------------------------ 3. same bytes, same result
@pytest.mark.parametrize("c", WC.CASES, ids=str)
def test_w4_equals_the_fp8_kernel_on_the_expanded_bytes(dev, c, setenv):
    _check_info(c, setenv)
    o = WC.operands(c, gaussian=True)
    g = QC.geom_of(c)
    packed = _pack(dev, c, o)
    wq = ops.unpack_q8_w4(g, packed[0], packed[1])
    xb = T._input(dev, c, o)
    a, fa = _launch(dev, c, o, packed, xb=xb)
    b, fb = T._launch(dev, c, o, (wq, None, packed[2]), xb=xb)
    assert set(a) == set(b) and fa == fb
    for what in a:
        assert not bool(is_sentinel(a[what][0]).any()), what
        assert bool((a[what][0].float() != 0).any()), what
        assert _same(a[what][0], b[what][0]), "%s: %s differs from mcamd_conv_fwd_q8 on the same bytes in %d elements" % (
            c.name, what, int((T._bits(a[what][0]) != T._bits(b[what][0])).sum()))
        assert _same(a[what][1], b[what][1]), "%s: outside the slice" % what


# ------------------------------------------------------------------------------------------------ 4. exact against float64
@pytest.mark.parametrize("c", WC.CASES, ids=str)
def test_w4_instance_exact(dev, c, setenv):
    r = _check_info(c, setenv)
    o, ref, (codes_r, g_r) = WC.operands_and_reference(c)
    assert QC.exactness(c, o, ref) == [], c.name            # on the reference's operands, never from kernel output
    packed = _pack(dev, c, o)
    assert torch.equal(packed[2][:c.cout].cpu(), ref.e), "exponents"
    out, flag = _launch(dev, c, o, packed)
    for name, want in (("y", ref.y), ("y2", ref.y2)):
        if want is None:
            continue
        got, rest = out[name]
        T._assert_equal(c, r, name, got, want)
        T._assert_untouched(c, name, rest)
    assert flag == 0


# ------------------------------------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("name", WC.DETERMINISM_CASES)
def test_w4_is_deterministic(dev, name, setenv):
    c = next(c for c in WC.CASES if c.name == name)
    _check_info(c, setenv)
    o = WC.operands(c, gaussian=True)
    p1, p2 = _pack(dev, c, o), _pack(dev, c, o)
    assert all(torch.equal(x, y) for x, y in zip(p1, p2)), "the packer is deterministic"
    a, _ = _launch(dev, c, o, p1)
    b, _ = _launch(dev, c, o, p1)
    for what in a:
        assert not bool(is_sentinel(a[what][0]).any())
        assert _same(a[what][0], b[what][0]), what
