"""The split-K fp4-operand forward pair (csrc/conv_q8_w4_mx.hip's partial kernel + csrc/conv_q8_splitk.hip's finish kernel,
mcamd_conv_fwd_q8_w4_mx_splitk) per element, on w4_mx_splitk_cases' launches.

  1. exact: on integer draws (shifts that differ between groups; every partial sum in every order is an fp32 number, proved per
     case by test_q8_w4_mx_splitk_cpu.py) every destination EQUALS the float64 reference for every slice count -- code for code,
     fp16 bit for bit; outputs and workspace start as sentinels and everything outside the slice must still hold one;
  2. one slice is the unsplit kernel: on Gaussian operands S = 1 equals mcamd_conv_fwd_q8_w4_mx on the same packed operands, bit
     for bit (the per-element instruction sequence is the same whatever the tile);
  3. Gaussian operands, S >= 2, against float64 beside the unsplit kernel (parent code) on the same operands: no byte more than
     one e4m3 code from the reference, at most twice the baseline's count of differing elements + 2, at most twice its largest
     fp16 relative error -- test_q8_w4_mx_kernels_gpu.py's rule;
  4. two launches of one (case, S) are bit-equal.

The helpers are test_q8_splitk_kernels_gpu's and test_q8_w4_mx_kernels_gpu's."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
import q8_cases as QC  # noqa: E402
import q8_ref as R  # noqa: E402
import w4_ref as W  # noqa: E402
import w4_mx_splitk_cases as XC  # noqa: E402
import test_q8_splitk_kernels_gpu as SK  # noqa: E402  (helpers only: _dev, _input, _alloc, _assert_equal, _assert_untouched, _same)
import test_q8_w4_mx_kernels_gpu as MX  # noqa: E402  (helpers only: _pack, _launch, _distance)
from util import NAN, NAN8, padded_split, is_sentinel  # noqa: E402

pytestmark = pytest.mark.gpu


def _launch(dev, c, o, packed, slices, xb=None, ws=None):
    """One launch of mcamd_conv_fwd_q8_w4_mx_splitk into sentinel-filled outputs: ({name: (got NCHW, everything outside the
    slice)}, overflow flag)."""
    g = QC.geom_of(c)
    xb = SK._input(dev, c, o) if xb is None else xb
    Ho, Wo = (c.H, c.W) if c.dst == "plain" else (c.H // 2, c.W // 2)
    y_ld = c.y_ld or ops.round_up(c.cdst, 32)
    y = SK._alloc(dev, c.B, Ho, Wo, y_ld, c.fmt_y)
    y2, y2_ld, y2_choff = None, 0, 0
    if c.dst == "pool+y2":
        y2_ld, y2_choff = c.y2_slice
        y2 = SK._alloc(dev, c.B, c.H, c.W, y2_ld, c.fmt_y2)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.conv_fwd_q8_w4_mx_splitk(g, xb, *packed, y, y_ld, c.y_choff, scale=SK._dev(o.scale, dev), shift=SK._dev(o.shift, dev),
                                 slope=c.slope, dst_mode=QC.DSTS[c.dst], y2=y2, y2_ld=y2_ld, y2_choff=y2_choff, y_f8=c.fmt_y == "f8",
                                 y2_f8=c.fmt_y2 == "f8", overflow=flag, slices=slices, workspace=ws)
    torch.cuda.synchronize()
    out = {"y": padded_split(y, c.B, Ho, Wo, y_ld, c.y_choff, c.cdst, NAN8 if c.fmt_y == "f8" else NAN)}
    if y2 is not None:
        out["y2"] = padded_split(y2, c.B, c.H, c.W, y2_ld, y2_choff, c.cout, NAN8 if c.fmt_y2 == "f8" else NAN)
    return out, int(flag.item())


def _resolved(c, S):
    return ops.conv_fwd_q8_w4_mx_splitk_info(QC.geom_of(c), QC.DSTS["pool" if c.dst == "pool+y2" else c.dst], S)


# ------------------------------------------------------------------------------------------------ 1. exact against float64
@pytest.mark.parametrize("p", XC.LAUNCHES, ids=XC.launch_id)
def test_exact(dev, p):
    sc, slices = p
    c = sc.c
    info = _resolved(c, slices)
    S = info.slices
    assert 1 <= S <= sc.chunks and (slices == XC.POLICY or S == slices)
    o, ref = XC.operands_and_reference(c)
    packed = MX._pack(dev, c, o)
    assert torch.equal(packed[2][:c.cout].cpu(), ref.e), "exponents"
    # (a workspace of its own, pre-filled with NaN: a slab element the partial kernel did not write would poison the sum)
    ws = torch.full((info.workspace_bytes // 4,), NAN, dtype=torch.float32, device=dev)
    out, flag = _launch(dev, c, o, packed, slices, ws=ws)
    for name, want in (("y", ref.y), ("y2", ref.y2)):
        if want is not None:
            SK._assert_equal(c, S, name, out[name][0], want)
            SK._assert_untouched(c, name, out[name][1])
    if not (o.planted and c.fmt_y == "f16"):
        assert flag == 0, "no fp16 value was clamped (bytes saturate silently): the overflow flag must stay 0"
        return
    # row (h): the flag is set and +-65504 stored at the planted elements; with nothing planted it stays 0
    assert flag == 1, "a value was clamped to +-65504: the overflow flag must be set"
    for (b, ch, h, x, sign) in o.planted:
        assert float(out["y"][0][b, ch, h, x]) == sign * 65504.0
    o2, ref2 = XC.operands_and_reference(c, plant=False)
    out2, flag2 = _launch(dev, c, o2, packed, slices)
    SK._assert_equal(c, S, "y (nothing planted)", out2["y"][0], ref2.y)
    assert flag2 == 0, "nothing was clamped: the overflow flag must stay 0"


# ------------------------------------------------------------------------------------------------ 2. one slice
@pytest.mark.parametrize("sc", XC.CASES, ids=XC.case_id)
def test_one_slice_is_the_unsplit_kernel(dev, sc):
    c = sc.c
    o = QC.operands(c, gaussian=True)
    packed, xb = MX._pack(dev, c, o), SK._input(dev, c, o)
    a, fa = _launch(dev, c, o, packed, 1, xb=xb)
    b, fb = MX._launch(dev, c, o, packed, xb=xb)
    for what in a:
        assert not bool(is_sentinel(a[what][0]).any()), what
        same = SK._bits(a[what][0]) == SK._bits(b[what][0])
        assert bool(same.all()), "%s %s: %d of %d elements differ from mcamd_conv_fwd_q8_w4_mx's" % (
            c.name, what, int((~same).sum()), same.numel())
        SK._assert_untouched(c, what, a[what][1])
    assert fa == fb


# ------------------------------------------------------------------------------------------------ 3. Gaussian operands, S >= 2
_GAUSS = {}      # case name -> (operands, {destination: the float64 reference's store}): once, shared, never modified


def _gaussian(c):
    if c.name not in _GAUSS:
        o = QC.operands(c, gaussian=True)
        _, _, e4, _, w8 = W.quantise(o.w, o.mask)
        v = R.block(o.a8, w8, e4, o.scale, o.shift, c.slope, dtype=torch.float64)
        store = lambda fmt, dst: R.store_bytes(v, dst) if fmt == "f8" else R.store_fp16(v, dst)
        want = {"y": store(c.fmt_y, "pool" if c.dst == "pool+y2" else c.dst)}
        if c.dst == "pool+y2":
            want["y2"] = store(c.fmt_y2, "plain")
        _GAUSS[c.name] = (o, want)
    return _GAUSS[c.name]


@pytest.mark.parametrize("p", [p for p in XC.LAUNCHES if p[1] != 1], ids=XC.launch_id)
def test_gaussian_against_float64_beside_the_unsplit_kernel(dev, p):
    sc, slices = p
    c = sc.c
    S = _resolved(c, slices).slices
    assert S >= 2, (c.name, S)
    o, want = _gaussian(c)
    packed, xb = MX._pack(dev, c, o), SK._input(dev, c, o)
    base, _ = MX._launch(dev, c, o, packed, xb=xb)           # the baseline first: parent code on the same operands
    new, _ = _launch(dev, c, o, packed, slices, xb=xb)
    for what in want:
        (n_new, d_new), (n_base, d_base) = MX._distance(new[what][0], want[what]), MX._distance(base[what][0], want[what])
        msg = "%s %s, %d slices: of %d elements the split pair differs from float64 in %d (largest %.3g), the unsplit kernel in %d " \
              "(largest %.3g)" % (c.name, what, S, want[what].numel(), n_new, d_new, n_base, d_base)
        print(msg)
        assert not bool(is_sentinel(new[what][0]).any()), msg
        SK._assert_untouched(c, what, new[what][1])
        assert n_new <= 2 * n_base + 2, msg
        if want[what].dtype == torch.uint8:
            assert R.byte_mismatch(new[what][0], want[what])[1], "a byte is more than one code from the reference: " + msg
        else:
            assert d_new <= 2.0 * d_base, msg


# ------------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("p", [p for p in XC.LAUNCHES if p[1] != 1], ids=XC.launch_id)
def test_deterministic(dev, p):
    sc, slices = p
    c = sc.c
    o = _gaussian(c)[0]
    packed, xb = MX._pack(dev, c, o), SK._input(dev, c, o)
    a, _ = _launch(dev, c, o, packed, slices, xb=xb)
    b, _ = _launch(dev, c, o, packed, slices, xb=xb)
    assert all(not bool(is_sentinel(a[what][0]).any()) for what in a) and SK._same(a, b), (c.name, slices)
