"""Every fp8 forward kernel instance mcamd_conv_fwd_q8 (inference and raw fp32 epilogue), mcamd_conv_fwd_q8_slim and
mcamd_conv_fwd_q8_sparse24 can launch (csrc/conv_q8.hip, csrc/conv_q8_sparse.hip, the byte half of conv_epi.h), in both MFMA
forms (MCAMD_Q8_MFMA 0 / 1), against an EXACT reference, with the method of test_conv_instances_gpu.py and
test_sparse_instances_gpu.py.

The operands are small integers times powers of two: their e4m3 codes are exact, every product is a multiple of one power
of two per filter and every partial sum in every order an fp32 number; the epilogue (power-of-two scales, shifts in steps of
1/4, slope 1/8 or 1) is exact; a byte destination adds one rounding of an exactly known value, which float64 and torch's
float8_e4m3fn cast reproduce code for code (tests/q8_cases.py, proved per case without a GPU by test_q8_cases_cpu.py).  The
result must EQUAL the reference, code for code (0x00 and 0x80 are different codes) and fp16 bit for fp16 bit.  There is no
tolerance in this file.

Bytes outside the operand slice hold the NaN code, the halo 0x00, the channels a slim launch reads beyond cin non-zero
finite codes.  fp16 and fp32 outputs start as NaN everywhere, halo and guard bands included, byte outputs as the NaN code
0x7F, which q() never stores; everything outside the interior pixels of the slice must still hold its sentinel."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
import q8_cases as QC  # noqa: E402
import q8_ref as R  # noqa: E402
import q8_sparse_ref as SP  # noqa: E402
from util import NAN, NAN8, whole, padded_split, is_sentinel, has_nan_code, fill_padded_q8  # noqa: E402

pytestmark = pytest.mark.gpu

KERNEL_NAMES = {"dense": "conv_q8_kernel", "raw": "conv_q8_kernel<RAW>", "border": "conv_q8_border_kernel", "sparse": "conv_q8_sparse_kernel"}


def _check_info(c, setenv):
    """The query must still name the instance and the boundary conditions the case was written for."""
    QC.apply_env(c, setenv)
    r = QC.info_of(c)
    assert QC.instance_of(c, r) == c.expect, (c.name, r)
    assert set(c.tags) - set(QC.VALUE_TAGS) <= QC.boundary_tags(c, r), (c.name, r, QC.boundary_tags(c, r))
    return r


def _dev(t, dev):
    return t.to(dev).contiguous() if t is not None else None


def _pack(dev, c, o, fam=None):
    """Pack on the device with the family's packer: (weights, [index words,] exponents)."""
    g = QC.geom_of(c)
    fam = fam or c.fam
    if fam == "sparse":
        wq, idx, wexp = ops.pack_q8_sparse24(g, _dev(o.w, dev), _dev(o.mask, dev))
        return wq, idx, wexp
    if fam == "slim":
        wq, wexp = ops.pack_q8_slim(g, _dev(o.w, dev), _dev(o.mask, dev))
    else:
        wq, wexp = ops.pack_q8(g, _dev(o.w, dev), _dev(o.mask, dev))
    return wq, None, wexp


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


def _launch(dev, c, o, packed, dst=None, fam=None, xb=None):
    """One launch into sentinel-filled outputs.  Returns ({name: (got NCHW, everything outside the slice)}, overflow flag)."""
    dst, fam = dst or c.dst, fam or c.fam
    g = QC.geom_of(c)
    xb = _input(dev, c, o) if xb is None else xb
    wq, idx, wexp = packed
    if fam == "raw":
        y_ld = c.y_ld or c.cout
        y = torch.full((c.M, y_ld), NAN, device=dev)
        slab = torch.full((ops.conv_fwd_q8_stats_rows(g), 2, ops.round_up(c.cout, 256)), NAN, device=dev) if c.stats else None
        ops.conv_fwd_q8_raw(g, xb, wq, wexp, y, y_ld, c.y_choff, stats=slab)
        torch.cuda.synchronize()
        return {"y": y.cpu(), "slab": slab.cpu() if slab is not None else None}, None
    Ho, Wo = (c.H, c.W) if dst == "plain" else (c.H // 2, c.W // 2)
    y_ld = c.y_ld or ops.round_up(c.cdst, 32)
    y = _alloc(dev, c.B, Ho, Wo, y_ld, c.fmt_y)
    y2, y2_ld, y2_choff = None, 0, 0
    if dst == "pool+y2":
        y2_ld, y2_choff = c.y2_slice
        y2 = _alloc(dev, c.B, c.H, c.W, y2_ld, c.fmt_y2)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = dict(scale=_dev(o.scale, dev), shift=_dev(o.shift, dev), slope=c.slope, dst_mode=QC.DSTS[dst], y2=y2, y2_ld=y2_ld,
              y2_choff=y2_choff, y_f8=c.fmt_y == "f8", y2_f8=c.fmt_y2 == "f8", overflow=flag)
    if fam == "sparse":
        ops.conv_fwd_q8_sparse24(g, xb, wq, idx, wexp, y, y_ld, c.y_choff, **kw)
    elif fam == "slim":
        ops.conv_fwd_q8_slim(g, xb, wq, wexp, y, y_ld, c.y_choff, border=_dev(o.border, dev), **kw)
    else:
        ops.conv_fwd_q8(g, xb, wq, wexp, y, y_ld, c.y_choff, **kw)
    torch.cuda.synchronize()
    out = {"y": padded_split(y, c.B, Ho, Wo, y_ld, c.y_choff, c.cdst, NAN8 if c.fmt_y == "f8" else NAN)}
    if y2 is not None:
        out["y2"] = padded_split(y2, c.B, c.H, c.W, y2_ld, y2_choff, c.cout, NAN8 if c.fmt_y2 == "f8" else NAN)
    return out, int(flag.item())


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.float16 else t


def _assert_equal(c, r, what, got, want):
    """got: uint8 codes or fp16 [B][n][h][w]; want: uint8 codes, or the fp16 values as fp32.  Codes must be the reference's
    codes, fp16 values its bits (a sentinel, an unwritten or polluted element, compares unequal)."""
    if want.dtype != torch.uint8:
        want = want.half()
    assert got.dtype == want.dtype and got.shape == want.shape, (c.name, what, got.dtype, got.shape, want.dtype, want.shape)
    if torch.equal(_bits(got), _bits(want)):
        return
    bad = _bits(got) != _bits(want)
    idx = bad.nonzero()
    nt = sorted(set((idx[:, 1] % c.cout // r.bmw).tolist()))
    first = tuple(idx[0].tolist())
    show = (lambda v: "0x%02X" % int(v)) if got.dtype == torch.uint8 else (lambda v: repr(float(v)))
    raise AssertionError("%s (%s<%d, %d, .., F8MFMA = %d>): %d of %d elements of %s differ from the exact result; first (image, channel, "
                         "y, x) %s, got %s want %s; %d sentinels among them; channel tiles touched %s"
                         % (c.name, KERNEL_NAMES[c.kernel], r.bmw, r.bnp, r.f8mfma, int(bad.sum()), bad.numel(), what, list(first),
                            show(got[first]), show(want[first]), int((is_sentinel(got) & bad).sum()), nt[:16]))


def _assert_untouched(c, what, rest):
    keep = is_sentinel(rest)
    assert bool(keep.all()), "%s: %d elements of %s outside the slice were written" % (c.name, int((~keep).sum()), what)


def _check_raw(c, r, o, ref, out):
    y, slab = out["y"], out["slab"]
    y_ld = y.shape[1]
    got = y[:, c.y_choff:c.y_choff + c.cout]
    want = ref.raw.permute(0, 2, 3, 1).reshape(c.M, c.cout).float()
    if not torch.equal(got, want):
        bad = ~(got == want)
        idx = bad.nonzero()
        raise AssertionError("%s (%s<%d, %d, .., F8MFMA = %d>): %d of %d raw values differ; first (pixel, channel) %s got %r want %r; "
                             "channel tiles touched %s" % (c.name, KERNEL_NAMES[c.kernel], r.bmw, r.bnp, r.f8mfma, int(bad.sum()), bad.numel(),
                                                           idx[0].tolist(), float(got[bad][0]), float(want[bad][0]),
                                                           sorted(set((idx[:, 1] // r.bmw).tolist()))[:16]))
    rest = y.clone()
    rest[:, c.y_choff:c.y_choff + c.cout] = NAN
    _assert_untouched(c, "y", rest)
    assert y_ld == (c.y_ld or c.cout)
    if not c.stats:
        assert slab is None
        return
    assert slab.shape[0] == r.mtiles
    nwritten = ops.round_up(c.cout, r.bmw)
    assert torch.equal(slab[:, 0, :c.cout], ref.s1.float()), "%s: sums" % c.name
    assert torch.equal(slab[:, 1, :c.cout], ref.s2.float()), "%s: sums of squares" % c.name
    assert bool((slab[:, :, c.cout:nwritten] == 0).all()), "%s: the channels up to round_up(N, bmw) read zero" % c.name
    assert bool(torch.isnan(slab[:, :, nwritten:]).all()), "%s: slab columns beyond the last filter tile were written" % c.name


@pytest.mark.parametrize("c", QC.Q8_CASES, ids=str)
def test_q8_instance_exact(dev, c, setenv):
    r = _check_info(c, setenv)
    o, ref = QC.operands_and_reference(c)
    assert QC.exactness(c, o, ref) == [], c.name           # the conditions of exactness, on this case's own reference
    assert set(c.tags) & set(QC.VALUE_TAGS) <= QC.value_tags(c, o, ref), c.name
    packed = _pack(dev, c, o)
    assert torch.equal(packed[2][:c.cout].cpu(), ref.e), "exponents"

    out, flag = _launch(dev, c, o, packed)
    if c.fam == "raw":
        _check_raw(c, r, o, ref, out)
        return
    for name, want in (("y", ref.y), ("y2", ref.y2)):
        if want is None:
            continue
        got, rest = out[name]
        _assert_equal(c, r, name, got, want)
        _assert_untouched(c, name, rest)
    if c.dst == "pool+y2" and c.fmt_y == c.fmt_y2:
        y, y2 = out["y"][0], out["y2"][0]
        pooled = R.pool_bytes(y2) if c.fmt_y == "f8" else F.max_pool2d(y2.float(), 2, 2).half()
        assert torch.equal(_bits(y), _bits(pooled)), "y is not the pooled y2, bit for bit"
    if c.dst == "pool":
        # the same launch with the full-resolution copy: the pooled output does not depend on it
        out2, _ = _launch(dev, c, o, packed, dst="pool+y2")
        assert torch.equal(_bits(out["y"][0]), _bits(out2["y"][0])), "pool and pool+y2 differ in y"
        _assert_untouched(c, "y (with y2)", out2["y"][1])
        _assert_untouched(c, "y2", out2["y2"][1])
    has_f16 = c.fmt_y == "f16" or (c.dst == "pool+y2" and c.fmt_y2 == "f16")
    if not (o.planted and has_f16):
        assert flag == 0, "no fp16 value was clamped (bytes saturate silently): the overflow flag must stay 0"
        return
    assert flag == 1, "a value was clamped to +-65504: the overflow flag must be set"
    got = out["y"][0]
    for (b, ch, h, x, sign) in o.planted:
        assert float(got[b, ch, h, x]) == sign * 65504.0
    o2, ref2 = QC.operands_and_reference(c, plant=False)
    assert QC.exactness(c, o2, ref2) == []
    out2, flag2 = _launch(dev, c, o2, packed)
    _assert_equal(c, r, "y (nothing planted)", out2["y"][0], ref2.y)
    assert flag2 == 0, "nothing was clamped: the overflow flag must stay 0"


BYTE_CASES = [c for c in QC.Q8_CASES if c.fam != "raw" and "f8" in c.fmt]


@pytest.mark.parametrize("c", BYTE_CASES, ids=str)
def test_no_nan_code(dev, c, setenv):
    """Every byte output of every case, on the case's own operands and on Gaussian operands under scales that drive a good
    part of the values beyond +-448: no NaN code (0x7F / 0xFF) inside the slice, and the sentinel -- that same code --
    everywhere outside it."""
    _check_info(c, setenv)
    o, _ = QC.operands_and_reference(c)
    og = QC.operands(c, gaussian=True)
    og = og._replace(scale=og.scale * 400.0)
    for which, ops_ in (("exact", o), ("gaussian", og)):
        out, flag = _launch(dev, c, ops_, _pack(dev, c, ops_))
        for name, (got, rest) in out.items():
            if got.dtype != torch.uint8:
                continue
            assert not has_nan_code(got), "%s (%s operands): %s holds a NaN code" % (c.name, which, name)
            _assert_untouched(c, name, rest)
            if which == "gaussian":
                assert bool((got == 0x7E).any()) and bool((got == 0xFE).any() or c.slope != 1.0), "the scales saturate"


SLIM_AS_DENSE = [c for c in QC.Q8_CASES if c.fam == "slim" and not c.table and c.cin % 64 == 0]


@pytest.mark.parametrize("c", SLIM_AS_DENSE, ids=str)
def test_q8_slim_without_table_equals_dense(dev, c, setenv):
    """cin % 64 == 0 and no table: mcamd_pack_q8_slim / mcamd_conv_fwd_q8_slim equal mcamd_pack_q8 / mcamd_conv_fwd_q8 on the
    same buffers, bit for bit."""
    _check_info(c, setenv)
    o, _ = QC.operands_and_reference(c)
    ps, pd = _pack(dev, c, o), _pack(dev, c, o, fam="dense")
    assert torch.equal(ps[0], pd[0]) and torch.equal(ps[2], pd[2])
    xb = _input(dev, c, o)
    a, _ = _launch(dev, c, o, ps, xb=xb)
    b, _ = _launch(dev, c, o, pd, fam="dense", xb=xb)
    assert torch.equal(a["y"][0], b["y"][0]) and torch.equal(a["y"][1], b["y"][1])
    assert bool((a["y"][0] != 0).any())


@pytest.mark.parametrize("c", [c for c in QC.Q8_CASES if c.fam == "sparse"], ids=str)
def test_q8_sparse_packer_decode(dev, c):
    """The device's 2:4 packing, decoded on the host from the layout include/mcamd.h states: the codes the reference
    multiplies, ascending offsets (pad rows included), zero pad rows, and the offsets of the kept rule."""
    o, ref = QC.operands_and_reference(c)
    for ops_, w8_eff, w8 in ((o, ref.w8_eff, ref.w8), (QC.operands(c, gaussian=True), None, None)):
        if w8 is None:
            w8, w8_eff, _ = QC.quantise(c, ops_)
        wq, idx, wexp = _pack(dev, c, ops_)
        npad, ktot = ops.round_up(c.cout, 256), c.ktot
        assert (wq.numel(), idx.numel(), wexp.numel()) == (npad * ktot // 2, npad * ktot // 32, npad)
        kept, words = wq.view(npad, ktot // 2).cpu(), idx.view(ktot // 64, npad, 2).cpu()
        dense = SP.decompress(kept, words)
        bad = R.deq(dense[:c.cout]) != R.deq(SP.dense_rows(w8_eff))
        assert not bool(bad.any()), "%s: %d of %d packed codes differ; first (filter, k) %s" % (
            c.name, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
        assert bool((kept[c.cout:] == 0).all()) and bool((wexp[c.cout:] == 0).all()), "pad rows"
        off = ((words.to(torch.int64) & 0xFFFFFFFF).unsqueeze(-1) >> (2 * torch.arange(16))) & 3
        assert bool((off[..., 0::2] < off[..., 1::2]).all()), "offsets ascending"
        wm = ops_.w if ops_.mask is None else ops_.w * ops_.mask
        want_kept, want_words = SP.compress(w8, SP.keep_positions(wm))
        assert torch.equal(words[:, :c.cout].to(torch.int64) & 0xFFFFFFFF, want_words)
        assert torch.equal(R.deq(kept[:c.cout]), R.deq(want_kept))


@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("h", QC.ONEHOT_CASES, ids=QC.onehot_id)
def test_q8_onehot(dev, h, mfma, setenv):
    """Every filter keeps ONE weight, +-1 at its own (channel, tap), and between them the filters select every k of the
    packed order.  Image 0 names the channel, image 1 the tap: the centre pixel must be +-(the selected code's value) / 2:
    which k each operand lane (and, for 2:4, each index bit-field) selects, with no sum in the way -- in both MFMA forms."""
    c = QC.onehot_case(h, mfma)
    r = _check_info(c, setenv)
    a8, w, which = QC.onehot_operands(h)
    o = QC.Operands(a8, None, w, None, None, None, None, None, [])
    want = F.conv2d(R.deq(a8).double(), w.double(), None, 1, (c.k - 1) // 2) / 2.0
    out, flag = _launch(dev, c, o, _pack(dev, c, o))
    got, rest = out["y"]
    bad = [(f, which[f], [float(got[i, f, 1, 1]) for i in (0, 1)], [float(want[i, f, 1, 1]) for i in (0, 1)]) for f in range(c.cout)
           if not all(float(got[i, f, 1, 1]) == float(want[i, f, 1, 1]) for i in (0, 1))]
    assert not bad, "%s: %d of %d filters select the wrong k; first (filter, (channel, tap, sign), got, want): %s" % (
        c.name, len(bad), c.cout, bad[:8])
    _assert_equal(c, r, "y", got, want.float())
    _assert_untouched(c, "y", rest)
    assert flag == 0


@pytest.mark.parametrize("name", QC.DETERMINISM_CASES)
def test_q8_is_deterministic(dev, name, setenv):
    """Gaussian operands (sums that DO depend on the order) and two launches into fresh buffers: bit-equal."""
    c = next(c for c in QC.Q8_CASES if c.name == name)
    _check_info(c, setenv)
    o = QC.operands(c, gaussian=True)
    packed = _pack(dev, c, o)
    a, _ = _launch(dev, c, o, packed)
    b, _ = _launch(dev, c, o, packed)
    if c.fam == "raw":
        sl = slice(c.y_choff, c.y_choff + c.cout)
        assert not bool(torch.isnan(a["y"][:, sl]).any()) and torch.equal(a["y"][:, sl], b["y"][:, sl])
        if c.stats:
            assert not bool(torch.isnan(a["slab"][:, :, :c.cout]).any()) and torch.equal(a["slab"][:, :, :c.cout], b["slab"][:, :, :c.cout])
        return
    for what in a:
        assert not bool(is_sentinel(a[what][0]).any())
        assert torch.equal(_bits(a[what][0]), _bits(b[what][0])), what
