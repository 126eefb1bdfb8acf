"""The fp8 split-K forward pair (csrc/conv_q8_splitk.hip, mcamd_conv_fwd_q8_splitk) per element, in both MFMA forms
(MCAMD_Q8_MFMA 0 / 1), with the method of test_q8_instances_gpu.py.

T1  exact: on q8_cases' operands (small integers times powers of two: the fp32 sum is exact in ANY order, proved per case by
    test_q8_splitk_cpu.py) every destination must EQUAL q8_cases.operands_and_reference for every slice count listed -- code
    for code (0x00 and 0x80 differ), fp16 bit for bit; outputs start as sentinels (NaN / the 0x7F code) and everything outside
    the interior of the slice must still hold its sentinel.  No tolerance.
T2  S = 1 is the unsplit kernel: on Gaussian operands slices = 1 equals ops.conv_fwd_q8 on the same buffers, bit for bit.
T3  real shapes (conv19, conv13 at B = 1) at the policy's slice count, sums that DO depend on the order, against q8_ref.block
    in float64: differing bytes are adjacent codes, their share within q8_ref.MISMATCH_CAP / FP8_MFMA_CAP (the project's caps,
    argued from the formats' widths), fp16 destinations below 1e-3 rel-L2; the unsplit kernel's share is printed beside it.
T4  two launches with the same slice count are bit-equal (Gaussian operands).
T5  one-hot filters with one chunk per slice and with two slices: which chunk lands in which slice and which k each lane
    selects, with no sum in the way."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
import q8_cases as QC  # noqa: E402
import q8_splitk_cases as SKC  # noqa: E402
import q8_ref as R  # noqa: E402
from util import NAN, NAN8, whole, padded_split, is_sentinel, fill_padded_q8, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(t, dev):
    return t.to(dev).contiguous() if t is not None else None


def _pack(dev, c, o):
    return ops.pack_q8(QC.geom_of(c), _dev(o.w, dev), _dev(o.mask, dev))


def _input(dev, c, o):
    return fill_padded_q8(dev, c, o.a8, c.ld or c.k_tap, c.choff, c.k_tap, c.pad, o.fill)


def _alloc(dev, B, H, W, ld, fmt):
    if fmt == "f8":
        buf = ops.alloc_padded_q8(B, H, W, ld, dev)
        buf.fill_(NAN8)
    else:
        buf = ops.alloc_padded(B, H, W, ld, dev)
        whole(buf).fill_(NAN)
    return buf


def _launch(dev, c, o, packed, slices, xb=None, ws=None):
    """One launch into sentinel-filled outputs; slices None: the unsplit ops.conv_fwd_q8.  Returns ({name: (got NCHW,
    everything outside the slice)}, overflow flag)."""
    g = QC.geom_of(c)
    xb = _input(dev, c, o) if xb is None else xb
    wq, wexp = packed
    Ho, Wo = (c.H, c.W) if c.dst == "plain" else (c.H // 2, c.W // 2)
    y_ld = c.y_ld or ops.round_up(c.cdst, 32)
    y = _alloc(dev, c.B, Ho, Wo, y_ld, c.fmt_y)
    y2, y2_ld, y2_choff = None, 0, 0
    if c.dst == "pool+y2":
        y2_ld, y2_choff = c.y2_slice
        y2 = _alloc(dev, c.B, c.H, c.W, y2_ld, c.fmt_y2)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = dict(scale=_dev(o.scale, dev), shift=_dev(o.shift, dev), slope=c.slope, dst_mode=QC.DSTS[c.dst], y2=y2, y2_ld=y2_ld,
              y2_choff=y2_choff, y_f8=c.fmt_y == "f8", y2_f8=c.fmt_y2 == "f8", overflow=flag)
    if slices is None:
        ops.conv_fwd_q8(g, xb, wq, wexp, y, y_ld, c.y_choff, **kw)
    else:
        ops.conv_fwd_q8_splitk(g, xb, wq, wexp, y, y_ld, c.y_choff, slices=slices, workspace=ws, **kw)
    torch.cuda.synchronize()
    out = {"y": padded_split(y, c.B, Ho, Wo, y_ld, c.y_choff, c.cdst, NAN8 if c.fmt_y == "f8" else NAN)}
    if y2 is not None:
        out["y2"] = padded_split(y2, c.B, c.H, c.W, y2_ld, y2_choff, c.cout, NAN8 if c.fmt_y2 == "f8" else NAN)
    return out, int(flag.item())


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.float16 else t


def _assert_equal(c, S, what, got, want):
    """got: uint8 codes or fp16 [B][n][h][w]; want: uint8 codes, or the fp16 values as fp32.  Codes must be the reference's
    codes, fp16 values its bits (a sentinel, an unwritten or polluted element, compares unequal)."""
    if want.dtype != torch.uint8:
        want = want.half()
    assert got.dtype == want.dtype and got.shape == want.shape, (c.name, what, got.dtype, got.shape, want.dtype, want.shape)
    if torch.equal(_bits(got), _bits(want)):
        return
    bad = _bits(got) != _bits(want)
    idx = bad.nonzero()
    first = tuple(idx[0].tolist())
    show = (lambda v: "0x%02X" % int(v)) if got.dtype == torch.uint8 else (lambda v: repr(float(v)))
    raise AssertionError("%s, %d slices, MCAMD_Q8_MFMA=%d: %d of %d elements of %s differ from the exact result; first (image, "
                         "channel, y, x) %s, got %s want %s; %d sentinels among them; 64-channel tiles touched %s"
                         % (c.name, S, c.mfma, int(bad.sum()), bad.numel(), what, list(first), show(got[first]), show(want[first]),
                            int((is_sentinel(got) & bad).sum()), sorted(set((idx[:, 1] % c.cout // 64).tolist()))[:16]))


def _assert_untouched(c, what, rest):
    keep = is_sentinel(rest)
    assert bool(keep.all()), "%s: %d elements of %s outside the slice were written" % (c.name, int((~keep).sum()), what)


def _same(a, b):
    """two results of _launch, bit for bit: the interior and everything around it"""
    return all(torch.equal(_bits(a[k][0]), _bits(b[k][0])) and torch.equal(is_sentinel(a[k][1]), is_sentinel(b[k][1])) for k in a)


# ------------------------------------------------------------------------------------------------------------------ T1
@pytest.mark.parametrize("p", SKC.LAUNCHES, ids=SKC.launch_id)
def test_t1_exact(dev, p, setenv):
    sc, slices = p
    c = sc.c
    QC.apply_env(c, setenv)
    S = SKC.resolved(sc, slices)
    assert 1 <= S <= sc.chunks and (slices == SKC.POLICY or S == slices)
    o, ref = QC.operands_and_reference(c)
    packed = _pack(dev, c, o)
    assert torch.equal(packed[1][:c.cout].cpu(), ref.e), "exponents"
    # the workspace is set aside (its own allocation, sized by the query) and pre-filled with NaN: a slab element the partial
    # kernel did not write would poison the sum
    nbytes = ops.conv_fwd_q8_splitk_info(QC.geom_of(c), QC.DSTS[c.dst], slices).workspace_bytes
    ws = torch.full((nbytes // 4,), NAN, dtype=torch.float32, device=dev)
    out, flag = _launch(dev, c, o, packed, slices, ws=ws)
    for name, want in (("y", ref.y), ("y2", ref.y2)):
        if want is None:
            continue
        got, rest = out[name]
        _assert_equal(c, S, name, got, want)
        _assert_untouched(c, name, rest)
    has_f16 = c.fmt_y == "f16" or (c.dst == "pool+y2" and c.fmt_y2 == "f16")
    if not (o.planted and has_f16):
        assert flag == 0, "no fp16 value was clamped (bytes saturate silently): the overflow flag must stay 0"
        return
    # case (h): the flag is set and +-65504 stored at the planted elements; with nothing planted it stays 0
    assert flag == 1, "a value was clamped to +-65504: the overflow flag must be set"
    got = out["y"][0]
    for (b, ch, h, x, sign) in o.planted:
        assert float(got[b, ch, h, x]) == sign * 65504.0
    o2, ref2 = QC.operands_and_reference(c, plant=False)
    out2, flag2 = _launch(dev, c, o2, packed, slices)
    _assert_equal(c, S, "y (nothing planted)", out2["y"][0], ref2.y)
    assert flag2 == 0, "nothing was clamped: the overflow flag must stay 0"


# ------------------------------------------------------------------------------------------------------------------ T2
def _t2_variants():
    """Every case in its own destination form and, where the image allows (even H and W), in every other one too: (case, id)"""
    out = []
    for sc in SKC.SPLITK_CASES:
        c = sc.c
        out.append((c, c.name))
        if c.H % 2 or c.W % 2:
            continue
        for dst in QC.DSTS:
            if dst != c.dst:
                fmt = "f8+f16" if dst == "pool+y2" else c.fmt_y
                out.append((c._replace(dst=dst, fmt=fmt, y_ld=0, y_choff=0, y2_ld=0, y2_choff=0), "%s-as-%s" % (c.name, dst)))
    return out


_T2 = _t2_variants()


@pytest.mark.parametrize("c", [v[0] for v in _T2], ids=[v[1] for v in _T2])
def test_t2_one_slice_is_the_unsplit_kernel(dev, c, setenv):
    QC.apply_env(c, setenv)
    r = QC.info_of(c)
    assert QC.instance_of(c, r) == c.expect, (c.name, r)            # the unsplit launch it is compared with
    o = QC.operands(c, gaussian=True)
    packed = _pack(dev, c, o)
    xb = _input(dev, c, o)
    a, fa = _launch(dev, c, o, packed, 1, xb=xb)
    b, fb = _launch(dev, c, o, packed, None, xb=xb)
    for what in a:
        assert not bool(is_sentinel(a[what][0]).any()), what
        same = _bits(a[what][0]) == _bits(b[what][0])
        assert bool(same.all()), "%s %s: %d of %d elements differ from mcamd_conv_fwd_q8's (MCAMD_Q8_MFMA=%d)" % (
            c.name, what, int((~same).sum()), same.numel(), c.mfma)
        _assert_untouched(c, what, a[what][1])
    assert fa == fb


# ------------------------------------------------------------------------------------------------------------------ T3
REAL = {"conv19": dict(B=1, H=13, W=13, k=3, cin=1024, cout=1024, dst="plain", fmt="f8"),
        "conv13": dict(B=1, H=26, W=26, k=3, cin=256, cout=512, dst="pool+y2", fmt="f8+f16")}
_REAL_REF = {}       # name -> (operands, float64 reference value): computed once, shared by both MFMA forms, never modified


@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("name", sorted(REAL))
def test_t3_real_shapes_against_float64(dev, name, mfma, setenv):
    s = REAL[name]
    bmw = 256 if mfma else 128
    c = QC.case("sk-%s%s" % (name, ".m" if mfma else ""), "dense", s["B"], s["H"], s["W"], s["k"], s["cin"], s["cout"],
                ("dense", mfma, bmw), mfma=mfma, dst=s["dst"], fmt=s["fmt"], slope=R.SLOPE)
    QC.apply_env(c, setenv)
    info = ops.conv_fwd_q8_splitk_info(QC.geom_of(c), QC.DSTS[c.dst])
    assert info.slices >= 2, (name, info.slices)
    if name not in _REAL_REF:          # (the operands are seeded by the name in front of the dot: both MFMA forms share them)
        o = QC.operands(c, gaussian=True)
        w8, e = R.quantise_weights(o.w, None)
        _REAL_REF[name] = (o, R.block(o.a8, w8, e, o.scale, o.shift, c.slope))
    o, v = _REAL_REF[name]
    packed = _pack(dev, c, o)
    xb = _input(dev, c, o)
    split, _ = _launch(dev, c, o, packed, 0, xb=xb)
    unsplit, _ = _launch(dev, c, o, packed, None, xb=xb)
    cap = R.FP8_MFMA_CAP if mfma else R.MISMATCH_CAP
    dst = "pool" if c.dst == "pool+y2" else c.dst
    for what, fmt, d in (("y", c.fmt_y, dst), ("y2", c.fmt_y2, "plain")):
        if what not in split:
            continue
        got, rest = split[what]
        _assert_untouched(c, what, rest)
        if fmt == "f8":
            want = R.store_bytes(v, d)
            share, adjacent = R.byte_mismatch(got, want)
            share_u, adjacent_u = R.byte_mismatch(unsplit[what][0], want)
            print("%s %s MCAMD_Q8_MFMA=%d, %d slices: share of differing bytes split %.3g, unsplit %.3g (cap %.3g)"
                  % (name, what, mfma, info.slices, share, share_u, cap))
            assert adjacent, "%s %s: a differing byte is not the adjacent e4m3 code" % (name, what)
            assert share <= cap, "%s %s: share of differing bytes %.3g above %.3g" % (name, what, share, cap)
        else:
            want = R.store_fp16(v, d)
            err, err_u = rel_l2(got.float(), want), rel_l2(unsplit[what][0].float(), want)
            print("%s %s MCAMD_Q8_MFMA=%d, %d slices: fp16 rel-L2 split %.3g, unsplit %.3g" % (name, what, mfma, info.slices, err, err_u))
            assert err < 1e-3, "%s %s: fp16 rel-L2 %.3g" % (name, what, err)


# ------------------------------------------------------------------------------------------------------------------ T4
@pytest.mark.parametrize("sc", [sc for sc in SKC.SPLITK_CASES if sc.c.name.split(".")[0] in ("sk-a", "sk-c", "sk-g")], ids=SKC.case_id)
def test_t4_deterministic(dev, sc, setenv):
    c = sc.c
    QC.apply_env(c, setenv)
    o = QC.operands(c, gaussian=True)
    packed = _pack(dev, c, o)
    for slices in sorted(set(sc.slices) - {1}):
        a, _ = _launch(dev, c, o, packed, slices)
        b, _ = _launch(dev, c, o, packed, slices)
        for what in a:
            assert not bool(is_sentinel(a[what][0]).any())
        assert _same(a, b), (c.name, slices)


# ------------------------------------------------------------------------------------------------------------------ T5
@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("h", [h for h in QC.ONEHOT_CASES if h.fam == "dense"], ids=QC.onehot_id)
def test_t5_onehot(dev, h, mfma, setenv):
    """Every filter keeps ONE weight, +-1 at its own (channel, tap); image 0 names the channel, image 1 the tap: the centre
    pixel must be +-(the selected code's value) / 2 for every filter, with every slice one chunk and with two slices."""
    c = QC.onehot_case(h, mfma)
    QC.apply_env(c, setenv)
    a8, w, which = QC.onehot_operands(h)
    o = QC.Operands(a8, None, w, None, None, None, None, None, [])
    want = F.conv2d(R.deq(a8).double(), w.double(), None, 1, (c.k - 1) // 2) / 2.0
    chunks = ops.conv_fwd_q8_splitk_info(QC.geom_of(c)).chunks
    assert chunks == c.ktot // 64
    packed = _pack(dev, c, o)
    for S in sorted({chunks, min(2, chunks)}):
        out, flag = _launch(dev, c, o, packed, S)
        got, rest = out["y"]
        bad = [(f, which[f], [float(got[i, f, 1, 1]) for i in (0, 1)], [float(want[i, f, 1, 1]) for i in (0, 1)]) for f in range(c.cout)
               if not all(float(got[i, f, 1, 1]) == float(want[i, f, 1, 1]) for i in (0, 1))]
        assert not bad, "%s, %d slices: %d of %d filters select the wrong k; first (filter, (channel, tap, sign), got, want): %s" % (
            c.name, S, len(bad), c.cout, bad[:8])
        _assert_equal(c, S, "y", got, want.float())
        _assert_untouched(c, "y", rest)
        assert flag == 0
