"""Both splitk_partial_kernel instances and both splitk_finish_kernel forms mcamd_conv_fwd_splitk can launch
(csrc/conv_splitk.hip, the low-batch forward behind Darknet.splitk), against an EXACT reference, with the method of
test_conv_instances_gpu.py and test_sparse_instances_gpu.py.

The operands hold small integers; while max|x| * max|w| * (taps * padded channels) is below 2^24 every slab value and every
sum of slabs in slice order is an integer that fp32 holds, so the float64 reference of the UNSPLIT convolution applies
whatever the slice count.  The epilogue (scales 1/4 .. 2, shifts in steps of 1/4, slope 1/8) is exact as long as the result
is an fp16 number.  The result must EQUAL the reference as fp16 bit patterns: a slab the finish loop skips, a slice that
loses or doubles a K chunk, a tap of the packed K order one block off or a wrong row of a tile that spans two images is off
by at least one unit (test_splitk_cases_cpu.py proves that every slice and every boundary chunk is visible in every tile).
There is no tolerance in this file.

tests/splitk_cases.py holds the cases; test_splitk_cases_cpu.py proves without a GPU that they reach both partial instances
with every destination form, the raw form and every boundary condition.  Channels outside the operand slice hold NaN, the
slice beyond the real channels and the halo hold zero; every output starts as NaN everywhere, halo and guard bands included,
and must stay so outside the interior of its slice.  The workspace starts as NaN too -- a slab element the partial kernel
did not write poisons the sum -- and lies between two NaN guard bands that must stay untouched."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
import splitk_cases as SK  # noqa: E402
from util import NAN, whole, fill_padded, padded_split, is_sentinel  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096          # fp32 / fp16 elements in front of and behind the workspace and the raw output


def _check_info(c, setenv):
    """The query must still name the instance and the boundary conditions the case was written for."""
    SK.apply_env(setenv)
    r = SK.info_of(c)
    assert (r.bk, r.stages) == c.expect, (c.name, r.bk, r.stages)
    assert set(c.tags) <= SK.boundary_tags(c, r), (c.name, SK.boundary_tags(c, r))
    return r


def _pack(dev, c, w):
    return ops.pack_weights(SK.geom_of(c), w.to(dev).contiguous(), None, True, False)[0]


def _dev(t, dev):
    return t.to(dev) if t is not None else None


def _launch(dev, c, r, act, wp, scale, shift, slope=SK.SLOPE, form=None):
    """One launch into NaN-filled outputs through a NaN-filled, NaN-guarded workspace sized by the query.  Returns {name:
    (got NCHW, everything outside the slice)} and the overflow flag."""
    form = form or c.form
    g = SK.geom_of(c)
    xb = fill_padded(dev, c, act, c.ld or c.k_tap, c.choff, c.k_tap, 0)
    n = r.workspace_bytes // 4
    ws_all = torch.full((GUARD + n + GUARD,), NAN, dtype=torch.float32, device=dev)
    ws = ws_all[GUARD:GUARD + n]
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = {}
    if form == "raw":
        y_ld = c.y_ld or c.cout
        y_all = torch.full((GUARD + c.M * y_ld + GUARD,), NAN, dtype=torch.float16, device=dev)
        ops.conv_fwd_raw_splitk(g, xb, wp, y_all[GUARD:GUARD + c.M * y_ld], y_ld, c.y_choff, slices=c.slices, workspace=ws, overflow=flag)
        torch.cuda.synchronize()
        all_ = y_all.clone()
        v = all_[GUARD:GUARD + c.M * y_ld].view(c.B, c.H, c.W, y_ld)
        got = v[..., c.y_choff:c.y_choff + c.cout].permute(0, 3, 1, 2).clone().cpu()
        v[..., c.y_choff:c.y_choff + c.cout] = NAN
        out["y"] = (got, all_.cpu())
    else:
        Ho, Wo = (c.H, c.W) if form == "plain" else (c.H // 2, c.W // 2)
        y_ld = c.y_ld or c.cdst
        y = ops.alloc_padded(c.B, Ho, Wo, y_ld, dev)
        whole(y).fill_(NAN)
        y2, y2_ld, y2_choff = None, 0, 0
        if form == "pool+y2":
            y2_ld, y2_choff = c.y2_slice
            y2 = ops.alloc_padded(c.B, c.H, c.W, y2_ld, dev)
            whole(y2).fill_(NAN)
        ops.conv_fwd_splitk(g, xb, wp, y, y_ld, c.y_choff, _dev(scale, dev), _dev(shift, dev), slope, dst_mode=SK.DSTS[form],
                            y2=y2, y2_ld=y2_ld, y2_choff=y2_choff, slices=c.slices, workspace=ws, overflow=flag)
        torch.cuda.synchronize()
        out["y"] = padded_split(y, c.B, Ho, Wo, y_ld, c.y_choff, c.cdst)
        if y2 is not None:
            out["y2"] = padded_split(y2, c.B, c.H, c.W, y2_ld, y2_choff, c.cout)
    guards = torch.cat([ws_all[:GUARD], ws_all[GUARD + n:]])
    assert bool(torch.isnan(guards).all()), "%s: %d elements of the guard bands around the %d-byte workspace were written" % (
        c.name, int((~torch.isnan(guards)).sum()), r.workspace_bytes)
    return out, int(flag.item())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_equal(c, r, what, got, want):
    """got fp16, want float64 [B][n][h][w]: the fp16 bit patterns must be the reference's (NaN, an unwritten or polluted
    element, compares unequal)."""
    assert got.dtype == torch.float16 and got.shape == want.shape, (c.name, what, got.dtype, got.shape, want.shape)
    assert bool((want.half().double() == want).all()), "the reference holds values that are no fp16 numbers"
    bad = _bits(got) != _bits(want.half())
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    first = tuple(idx[0].tolist())
    raise AssertionError("%s (splitk_partial_kernel<%d, %d>, %d slices of %d chunks, splitk_finish_kernel<%s>): %d of %d elements "
                         "of %s differ from the exact result; first (image, channel, y, x) %s, got %r want %r; %d sentinels among "
                         "them; channel tiles touched %s"
                         % (c.name, r.bk, r.stages, r.slices, r.chunks, "RAW" if c.form == "raw" else "PAD", int(bad.sum()), bad.numel(),
                            what, list(first), float(got[first]), float(want[first]), int((is_sentinel(got) & bad).sum()),
                            sorted(set((idx[:, 1] % c.cout // r.bn).tolist()))[:16]))


def _assert_untouched(c, what, rest):
    keep = is_sentinel(rest)
    assert bool(keep.all()), "%s: %d elements of %s outside the slice were written" % (c.name, int((~keep).sum()), what)


@pytest.mark.parametrize("c", SK.SPLITK_CASES, ids=str)
def test_splitk_instance_exact(dev, c, setenv):
    r = _check_info(c, setenv)
    o, ref = SK.operands_and_reference(c)
    assert SK.exactness(c, o, ref) == [], c.name            # the conditions of exactness, on this case's own reference
    wp = _pack(dev, c, o.w)

    out, flag = _launch(dev, c, r, o.act, wp, o.scale, o.shift)

    for name, want in (("y", ref.y), ("y2", ref.y2)):
        if want is None:
            continue
        got, rest = out[name]
        _assert_equal(c, r, name, got, want)
        _assert_untouched(c, name, rest)
    if c.form == "pool+y2":
        assert torch.equal(_bits(out["y"][0]), _bits(F.max_pool2d(out["y2"][0].float(), 2, 2).half())), "y is not max_pool2d(y2), bit for bit"
    if c.form == "pool":
        # the same launch with the full-resolution copy: the pooled output does not depend on it
        out2, _ = _launch(dev, c, r, o.act, wp, o.scale, o.shift, form="pool+y2")
        assert torch.equal(_bits(out["y"][0]), _bits(out2["y"][0])), "pool and pool+y2 differ in y"
        _assert_untouched(c, "y (with y2)", out2["y"][1])
        _assert_untouched(c, "y2", out2["y2"][1])
    if not c.overflow:
        assert flag == 0, "nothing was clamped: the overflow flag must stay 0"
        return
    assert flag == 1, "a value was clamped to +-65504: the overflow flag must be set"
    got = out["y"][0]
    for (b, ch, h, x, sign) in o.planted:
        assert float(got[b, ch, h, x]) == sign * 65504.0
    o2, ref2 = SK.operands_and_reference(c, plant=False)
    assert SK.exactness(c, o2, ref2) == []
    out2, flag2 = _launch(dev, c, r, o2.act, wp, o2.scale, o2.shift)
    _assert_equal(c, r, "y (nothing planted)", out2["y"][0], ref2.y)
    assert flag2 == 0, "nothing was clamped: the overflow flag must stay 0"


@pytest.mark.parametrize("h", SK.ONEHOT_CASES, ids=SK.onehot_id)
def test_splitk_onehot(dev, h, setenv):
    """Every filter keeps ONE weight, +-1 at its own (channel, tap), and between them the filters select every k of the
    packed order that holds a real channel; every activation value is distinct.  With every slice one chunk and with two
    slices the output must be +-(that value): which chunk lands in which slice and which k each operand lane selects,
    with no sum in the way."""
    x, w, which = SK.onehot_operands(h)
    for S in SK.onehot_slices(h):
        c = SK.onehot_case(h, S)
        r = _check_info(c, setenv)
        assert r.slices == S
        want = F.conv2d(x.double(), w.double(), None, 1, (c.k - 1) // 2)
        out, flag = _launch(dev, c, r, x, _pack(dev, c, w), None, None, slope=1.0)
        got, rest = out["y"]
        mid = c.H // 2
        bad = [(f, which[f], float(got[0, f, mid, mid]), float(want[0, f, mid, mid])) for f in range(c.cout)
               if not float(got[0, f, mid, mid]) == float(want[0, f, mid, mid])]
        assert not bad, "%s: %d of %d filters select the wrong k; first (filter, (channel, tap, sign), got, want): %s" % (
            c.name, len(bad), c.cout, bad[:8])
        _assert_equal(c, r, "y", got, want)
        _assert_untouched(c, "y", rest)
        assert flag == 0


@pytest.mark.parametrize("name", SK.DETERMINISM_CASES)
def test_splitk_is_deterministic(dev, name, setenv):
    """Gaussian operands (sums that DO depend on the order) and two launches into fresh buffers through fresh NaN-filled
    workspaces: bit-equal, and no sentinel left inside the slice."""
    c = next(c for c in SK.SPLITK_CASES if c.name == name)
    r = _check_info(c, setenv)
    assert r.slices > 1
    o = SK.operands(c, gaussian=True)
    wp = _pack(dev, c, o.w)
    a, _ = _launch(dev, c, r, o.act, wp, o.scale, o.shift)
    b, _ = _launch(dev, c, r, o.act, wp, o.scale, o.shift)
    for what in a:
        assert not bool(is_sentinel(a[what][0]).any()), what
        assert torch.equal(_bits(a[what][0]), _bits(b[what][0])), what
        _assert_untouched(c, what, a[what][1])
