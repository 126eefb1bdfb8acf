"""Every sparse24_kernel instance mcamd_conv_fwd_sparse24 can launch (csrc/conv_sparse.hip, the v_smfmac forward behind
sparse = "2:4"), against an EXACT reference, with the method of test_conv_instances_gpu.py.

The operands hold small integers; the sparse MFMA is exact on them (tools/smfmac_probe.hip), and while max|x| * max|w| *
(taps * padded channels) < 2^24 every partial sum in every order is an integer that fp32 holds.  The epilogue (scales 1/4
.. 2, shifts in steps of 1/4, slope 1/8) is exact as long as the result is an fp16 number.  The reference is float64
F.conv2d of x with the weights the packer keeps, the epilogue, then max_pool2d / reorg, and the result must EQUAL it: a
wrong index bit-field, an operand piece read by the wrong lane, a tap of the packed K order one block off, a dropped K
chunk or a wrong row of a tile that spans two images is off by at least one unit.  There is no tolerance in this file.

tests/sparse_cases.py holds the cases; test_sparse_cases_cpu.py proves without a GPU that they reach every instance with
every destination form and every boundary condition, and that every reference meets the conditions of exactness.
Channels outside the operand slice hold NaN, the slice beyond the real channels and the halo hold zero; every output
starts as NaN everywhere, halo and guard bands included, and must stay so outside the interior pixels of its slice
(conv_epi.h: store_pad_tile writes nothing else).

The packer is decoded on the host for every case; one-hot filters pin which k each index bit-field and each operand lane
selects, independent of any sum."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
import sparse_cases as SC  # noqa: E402
from util import NAN, whole, fill_padded, padded_split  # noqa: E402

pytestmark = pytest.mark.gpu


def _check_info(c, setenv):
    """The query must still name the instance and the boundary conditions the case was written for."""
    SC.apply_env(c, setenv)
    r = SC.info_of(c)
    assert (r.bmw, r.bnp, r.bk) == c.expect, (c.name, r)
    assert set(c.tags) <= SC.boundary_tags(c, r), (c.name, r, SC.boundary_tags(c, r))
    return r


def _pack(dev, c, w, mask):
    return ops.pack_sparse24(SC.geom_of(c), w.to(dev).contiguous(), mask.to(dev).contiguous() if mask is not None else None)


def _launch(dev, c, act, packed, scale, shift, slope=SC.SLOPE, dst=None, want_flag=False):
    """One launch into NaN-filled outputs.  Returns {name: (got NCHW, everything outside the slice)} and the overflow flag."""
    dst = dst or c.dst
    xb = fill_padded(dev, c, act, c.ld or c.k_tap, c.choff, c.k_tap, c.pad)
    Ho, Wo = (c.H, c.W) if dst == "plain" else (c.H // 2, c.W // 2)
    y_ld = c.y_ld or c.cdst
    y = ops.alloc_padded(c.B, Ho, Wo, y_ld, dev)
    whole(y).fill_(NAN)
    y2, y2_ld, y2_choff = None, 0, 0
    if dst == "pool+y2":
        y2_ld, y2_choff = c.y2_slice
        y2 = ops.alloc_padded(c.B, c.H, c.W, y2_ld, dev)
        whole(y2).fill_(NAN)
    flag = torch.zeros(1, dtype=torch.int32, device=dev) if want_flag else None
    ops.conv_fwd_sparse24(SC.geom_of(c), xb, packed[0], packed[1], y, y_ld, c.y_choff, scale.to(dev) if scale is not None else None,
                          shift.to(dev) if shift is not None else None, slope, dst_mode=SC.DSTS[dst], y2=y2, y2_ld=y2_ld,
                          y2_choff=y2_choff, overflow=flag)
    torch.cuda.synchronize()
    out = {"y": padded_split(y, c.B, Ho, Wo, y_ld, c.y_choff, c.cdst)}
    if y2 is not None:
        out["y2"] = padded_split(y2, c.B, c.H, c.W, y2_ld, y2_choff, c.cout)
    return out, (int(flag.item()) if want_flag else None)


def _assert_equal(c, r, what, got, want):
    """got fp16, want float64 [B][n][h][w]: the fp16 values must be the reference's (NaN, an unwritten or polluted element,
    compares unequal)."""
    assert got.dtype == torch.float16 and got.shape == want.shape, (c.name, what, got.dtype, got.shape, want.shape)
    if torch.equal(got, want.half()) and bool((got.double() == want).all()):
        return
    g = got.double()
    bad = ~(g == want)
    idx = bad.nonzero()
    diff = (g - want)[bad]
    diff = diff[~torch.isnan(diff)]
    nt = sorted(set((idx[:, 1] % c.cout // r.bmw).tolist()))
    raise AssertionError("%s (sparse24_kernel<%d, %d, .., %d>): %d of %d elements of %s differ from the exact result; first (image, "
                         "channel, y, x) %s, got %r want %r; difference min %r max %r (%d NaN); channel tiles touched %s"
                         % (c.name, r.bmw, r.bnp, r.bk, int(bad.sum()), g.numel(), what, idx[0].tolist(), float(g[bad][0]), float(want[bad][0]),
                            float(diff.min()) if diff.numel() else NAN, float(diff.max()) if diff.numel() else NAN,
                            int(bad.sum()) - diff.numel(), nt[:16]))


def _assert_untouched(c, what, rest):
    assert bool(torch.isnan(rest).all()), "%s: %d elements of %s outside the slice were written" % (c.name, int((~torch.isnan(rest)).sum()), what)


@pytest.mark.parametrize("c", SC.SPARSE_CASES, ids=str)
def test_sparse_instance_exact(dev, c, setenv):
    r = _check_info(c, setenv)
    o, ref = SC.operands_and_reference(c)
    assert SC.exactness(c, o, ref) == [], c.name           # the conditions of exactness, on this case's own reference
    packed = _pack(dev, c, o.w, o.mask)

    out, flag = _launch(dev, c, o.act, packed, o.scale, o.shift, want_flag=True)

    for name, want in (("y", ref.y), ("y2", ref.y2)):
        if want is None:
            continue
        got, rest = out[name]
        _assert_equal(c, r, name, got, want)
        _assert_untouched(c, name, rest)
    if c.dst == "pool+y2":
        assert torch.equal(out["y"][0], F.max_pool2d(out["y2"][0].float(), 2, 2).half()), "y is not max_pool2d(y2), bit for bit"
    if c.dst == "pool":
        # the same launch with the full-resolution copy: the pooled output does not depend on it
        out2, _ = _launch(dev, c, o.act, packed, o.scale, o.shift, dst="pool+y2")
        assert torch.equal(out["y"][0].view(torch.int16), out2["y"][0].view(torch.int16)), "pool and pool+y2 differ in y"
        _assert_untouched(c, "y (with y2)", out2["y"][1])
        _assert_untouched(c, "y2", out2["y2"][1])
    if not c.overflow:
        assert flag == 0, "nothing was clamped: the overflow flag must stay 0"
        return
    assert flag == 1, "a value was clamped to +-65504: the overflow flag must be set"
    got = out["y"][0]
    for (b, ch, h, x, sign) in o.planted:
        assert float(got[b, ch, h, x]) == sign * 65504.0
    o2, ref2 = SC.operands_and_reference(c, plant=False)
    assert SC.exactness(c, o2, ref2) == []
    out2, flag2 = _launch(dev, c, o2.act, packed, o2.scale, o2.shift, want_flag=True)
    _assert_equal(c, r, "y (nothing planted)", out2["y"][0], ref2.y)
    assert flag2 == 0, "nothing was clamped: the overflow flag must stay 0"


@pytest.mark.parametrize("h", SC.ONEHOT_CASES, ids=SC.onehot_id)
def test_sparse_index_onehot(dev, h, setenv):
    """Every filter keeps ONE weight, +-1 at its own (channel, tap), and between them the filters select every k of the
    packed order that holds a real channel; every activation value is distinct.  The output must be +-(that value): which
    k each index bit-field, each compressed weight piece and each activation piece of a lane selects, with no sum in the way."""
    c = SC.onehot_case(h)
    r = _check_info(c, setenv)
    x, w, which = SC.onehot_operands(h)
    want = F.conv2d(x.double(), w.double(), None, 1, (c.k - 1) // 2)
    out, _ = _launch(dev, c, x, _pack(dev, c, w, None), None, None, slope=1.0)
    got, rest = out["y"]
    mid = c.H // 2
    bad = [(f, which[f], float(got[0, f, mid, mid]), float(want[0, f, mid, mid])) for f in range(c.cout)
           if not float(got[0, f, mid, mid]) == float(want[0, f, mid, mid])]
    assert not bad, "%s: %d of %d filters select the wrong k; first (filter, (channel, tap, sign), got, want): %s" % (
        c.name, len(bad), c.cout, bad[:8])
    _assert_equal(c, r, "y", got, want)
    _assert_untouched(c, "y", rest)


def _check_packing(c, w, mask, vals, idx):
    """Decode the device's packing on the host: the kept values are (w * mask).half() under the packer's rule, bit for bit
    (a kept value is non-zero, so equal fp16 values have equal bits); offsets ascending; filler slots zero; pad rows zero;
    index words in [ktot / 32][npad][2] order (decode_packed reads them so)."""
    npad = ops.round_up(c.cout, 256)
    assert vals.numel() == npad * c.ktot // 2 and idx.numel() == npad * c.ktot // 16
    vals, p0, p1, dense = SC.decode_packed(c, vals, idx)
    assert bool((p0 < p1).all()), "%s: %d groups without ascending offsets" % (c.name, int((p0 >= p1).sum()))
    assert bool((vals[c.cout:] == 0).all()), "pad rows"
    weff = SC.effective(SC.Operands(None, w, mask, None, None, None, None))
    want = SC.packed_k_order(weff, c).half()
    bad = ~(dense[:c.cout] == want)
    assert not bool(bad.any()), "%s: %d of %d packed weights differ; first (filter, k) %s" % (
        c.name, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
    # a slot that holds no kept weight holds zero: every non-zero slot is accounted for by a non-zero of `want`
    assert int((vals[:c.cout] != 0).sum()) == int((want != 0).sum())
    p = SC.pack_ref(c, w, mask)
    kept = p.dense.view(c.cout, c.ktot // 4, 4) != 0
    two = kept.sum(-1) >= 2
    # where a group has two kept weights or more, the offsets are theirs (the first two in channel order)
    assert torch.equal(p0[:c.cout][two], p.p0[two]) and torch.equal(p1[:c.cout][two], p.p1[two])


@pytest.mark.parametrize("c", SC.SPARSE_CASES, ids=str)
def test_sparse_packer_decode(dev, c):
    o, _ = SC.operands_and_reference(c)
    _check_packing(c, o.w, o.mask, *_pack(dev, c, o.w, o.mask))
    og = SC.operands(c, gaussian=True)
    _check_packing(c, og.w, og.mask, *_pack(dev, c, og.w, og.mask))


@pytest.mark.parametrize("name", SC.DETERMINISM_CASES)
def test_sparse_is_deterministic(dev, name, setenv):
    """Gaussian operands (sums that DO depend on the order) and two launches into fresh buffers: bit-equal."""
    c = next(c for c in SC.SPARSE_CASES if c.name == name)
    _check_info(c, setenv)
    o = SC.operands(c, gaussian=True)
    packed = _pack(dev, c, o.w, o.mask)
    a, _ = _launch(dev, c, o.act, packed, o.scale, o.shift)
    b, _ = _launch(dev, c, o.act, packed, o.scale, o.shift)
    for what in a:
        assert not bool(torch.isnan(a[what][0]).any())
        assert torch.equal(a[what][0].contiguous().view(torch.int16), b[what][0].contiguous().view(torch.int16)), what
