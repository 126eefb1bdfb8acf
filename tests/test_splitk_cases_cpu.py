"""Coverage of tests/test_splitk_instances_gpu.py, proved without a GPU: what mcamd_conv_fwd_splitk can launch (asked from the
launch's own plan through mcamd_conv_fwd_splitk_info), that the cases of tests/splitk_cases.py reach both partial instances
with every destination form, the raw form and every named boundary condition, that EQUAL is the right comparison for every
case whatever the slice count, and that a lost or doubled slab or K chunk cannot go unseen."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops, _lib as L  # noqa: E402
import splitk_cases as SK  # noqa: E402
from util import fill_padded  # noqa: E402

ROWS = [next(c for c in SK.SPLITK_CASES if c.base == b) for b in dict.fromkeys(c.base for c in SK.SPLITK_CASES)]


def test_splitk_instances_are_the_expected_set(setenv):
    """splitk_partial_kernel<64, 3> and <32, 4>, and no other, over both epilogue modes, all destination forms, every filter
    and channel count from 8 to 1344 in steps of 8, both kernel sizes, images from one pixel to the training batch and
    forced slice counts 0 .. 16; the policy's answer always lies in [1, min(16, chunks)]."""
    assert SK.reachable(setenv) == set(SK.INSTANCES)


def test_splitk_info_names_the_launch(setenv):
    SK.apply_env(setenv)
    r = ops.conv_fwd_splitk_info(ops.geom(1, 13, 13, 3, 128, 264, 128), L.EPI_PAD_F16, 0, 5)
    assert (r.slices, r.bm, r.bn, r.bk, r.chunks, r.tiles) == (5, 64, 64, 64, 18, 15)
    assert (r.stages, r.mtiles, r.ntiles, r.finish_rows, r.finish_cols) == (3, 3, 5, 16, 64)
    assert r.workspace_bytes == 5 * 192 * 320 * 4
    r = ops.conv_fwd_splitk_info(ops.geom(2, 9, 7, 3, 72, 40, 96), L.EPI_RAW_F16, 0, 3)
    assert (r.bk, r.stages, r.chunks, r.mtiles, r.ntiles) == (32, 4, 27, 2, 1)
    # the fp8 pair answers through the same record: 64-byte chunks on a 3-stage ring, the same finish tile
    q = ops.conv_fwd_q8_splitk_info(ops.geom(1, 13, 13, 3, 128, 264, 128), 0, 5)
    assert (q.bk, q.stages, q.mtiles, q.ntiles, q.finish_rows, q.finish_cols) == (64, 3, 3, 5, 16, 64)


def test_splitk_cases_reach_every_instance_and_boundary(setenv):
    SK.apply_env(setenv)
    cs = SK.SPLITK_CASES
    assert len({c.name for c in cs}) == len(cs)
    tags_of = {i: set() for i in SK.INSTANCES}
    for c in cs:
        r = SK.info_of(c)
        assert (r.bk, r.stages) == c.expect, (c.name, r.bk, r.stages)
        assert c.slices == SK.POLICY or r.slices == c.slices
        assert 1 <= r.slices <= r.chunks
        t = SK.boundary_tags(c, r)
        assert set(c.tags) <= t, (c.name, set(c.tags) - t)
        tags_of[c.expect] |= t
    missing = {SK.K64: set(SK.BOUNDARIES_BOTH) - tags_of[SK.K64],
               SK.K32: set(SK.BOUNDARIES_BOTH + SK.BOUNDARIES_K32) - tags_of[SK.K32]}
    assert missing == {SK.K64: set(), SK.K32: set()}, missing
    for inst in SK.INSTANCES:
        mine = [c for c in cs if c.expect == inst]
        assert {c.form for c in mine} == set(SK.FORMS), (inst, {c.form for c in mine})
        assert {c.k for c in mine} == {1, 3}, inst
    assert {c.cin for c in cs if c.k_tap > c.cin} == set(SK.PADDED_CINS)
    # one chunk per slice on the 4-stage ring; the 32-channel K order with more than one block, 3x3
    assert any(c.expect == SK.K32 and SK.info_of(c).slices == SK.info_of(c).chunks for c in cs)
    assert any(c.kb == 32 and c.k == 3 and c.k_tap > 32 for c in cs)
    # the long K axis at the ceiling and at the policy's count
    long_k = [c for c in cs if c.base == SK.LONG_K]
    assert all((c.B, c.H, c.W, c.k, c.cin, c.draw, c.wdraw) == (1, 13, 13, 3, 1280, "s4", "s4u") for c in long_k)
    assert {c.slices for c in long_k} == {16, SK.POLICY} and all(SK.info_of(c).chunks == 180 for c in long_k)
    assert all(2 <= SK.info_of(c).slices <= 16 for c in long_k)
    assert all(c.base == SK.LONG_K or (c.M <= 700 and c.cin <= 256) for c in cs)
    # one overflow case per finish form, one of them with pad rows and pad columns in its last tiles
    sat = [c for c in cs if c.overflow]
    assert sorted(c.form == "raw" for c in sat) == [False, True]
    assert all(SK.info_of(c).slices > 1 for c in sat)
    assert any(c.M % 64 and c.cout % 64 for c in sat)
    got = {(next(c for c in cs if c.name == n).expect, next(c for c in cs if c.name == n).form == "raw") for n in SK.DETERMINISM_CASES}
    assert got == {(i, raw) for i in SK.INSTANCES for raw in (False, True)}
    assert all(SK.info_of(next(c for c in cs if c.name == n)).slices > 1 for n in SK.DETERMINISM_CASES)


@pytest.mark.parametrize("c", ROWS, ids=lambda c: c.base)
def test_splitk_case_is_exact(c):
    """The conditions under which the kernel output must EQUAL the unsplit reference (conv_cases.exactness: accumulator
    bound below 2^24 -- so every slab value and every sum in slice order is an exact fp32 integer --, every reference value an
    fp16 number), and a sentinel arrangement that leaves the reference finite: the convolution of the NaN-surrounded operand
    buffer's slice (zero halo, zero channels beyond cin) IS the reference's accumulator, and so is the restated GEMM."""
    for plant in ((True, False) if c.overflow else (True,)):
        o, ref = SK.operands_and_reference(c, plant)
        assert SK.exactness(c, o, ref) == [], c.name
        assert bool(torch.isfinite(ref.y).all()) and (ref.y2 is None or bool(torch.isfinite(ref.y2).all()))
        assert (ref.y2 is not None) == (c.form == "pool+y2")
        assert len(o.planted) == (2 if c.overflow and plant else 0)
        if c.form == "raw":
            assert o.scale is None and o.shift is None
    o, ref = SK.operands_and_reference(c)
    ld = c.ld or c.k_tap
    buf = fill_padded(torch.device("cpu"), c, o.act, ld, c.choff, c.k_tap, 0)
    view = ops.padded_view(buf, c.B, c.H, c.W, ld, 0)
    sl = view[..., c.choff:c.choff + c.k_tap]
    assert bool(torch.isfinite(sl).all())
    assert bool(torch.isnan(view[..., :c.choff]).all()) and bool(torch.isnan(view[..., c.choff + c.k_tap:]).all())
    wp = torch.zeros(c.cout, c.k_tap, c.k, c.k)
    wp[:, :c.cin] = o.w
    xs = sl.permute(0, 3, 1, 2).float()
    if c.k == 1:
        xs = xs[:, :, 1:-1, 1:-1]
    acc = F.conv2d(xs, wp)                                   # fp32: exact under the accumulator bound
    assert torch.equal(acc.double(), ref.acc)
    X, Wp = SK.gemm_operands(c, o.act, o.w)
    rows = ref.acc.permute(0, 2, 3, 1).reshape(c.M, c.cout)[SK.row_pixels(c)]
    assert torch.equal((X @ Wp.t()).double(), rows)
    assert sorted(SK.row_pixels(c).tolist()) == list(range(c.M))


@pytest.mark.parametrize("c", ROWS, ids=lambda c: c.base)
def test_every_slice_and_boundary_chunk_is_visible(c, setenv):
    """For every launch of the row with S > 1, every slice and every (M tile, N tile): the partial sum of that slice, and the
    contribution of its first and of its last K chunk alone, are non-zero in at least one element of the tile whose value is
    not clamped.  A finish loop that skips a slab, a slice that loses a chunk at either end or walks one chunk into its
    neighbour's range, then changes an element of the exact result by at least one unit."""
    SK.apply_env(setenv)
    o, _ = SK.operands_and_reference(c)
    r0 = SK.info_of(c, 1)
    cum = SK.chunk_sums(c, o, r0.bk)
    free = ~SK.clamped_mask(c, o)
    chunk_seen = SK.tile_any(((cum[1:] - cum[:-1]) != 0) & free, r0.bm, r0.bn)              # [chunks][mtiles][ntiles]
    for cs in (x for x in SK.SPLITK_CASES if x.base == c.base):
        r = SK.info_of(cs)
        if r.slices == 1:
            continue
        for s, (q0, q1) in enumerate(SK.slice_ranges(r.chunks, r.slices)):
            assert q1 > q0
            part = SK.tile_any(((cum[q1] - cum[q0]) != 0) & free, r.bm, r.bn)
            assert tuple(part.shape) == (r.mtiles, r.ntiles)
            assert bool(part.all()), "%s: slice %d adds nothing to tiles %s" % (cs.name, s, (~part).nonzero().tolist())
            for q in (q0, q1 - 1):
                assert bool(chunk_seen[q].all()), "%s: chunk %d adds nothing to tiles %s" % (cs.name, q, (~chunk_seen[q]).nonzero().tolist())


@pytest.mark.parametrize("h", SK.ONEHOT_CASES, ids=SK.onehot_id)
def test_onehot_filters_cover_every_k(h, setenv):
    """One filter per real (channel, tap): every k of the packed order that a real channel occupies is selected by exactly
    one filter, the values are fp16 integers, the reference output is +-(the value that filter selects), and the launches
    run with one chunk per slice and with two slices on the instance the case names."""
    SK.apply_env(setenv)
    slices = SK.onehot_slices(h)
    for S in slices:
        c = SK.onehot_case(h, S)
        r = SK.info_of(c)
        assert (r.bk, r.stages) == h.expect and r.slices == S
    assert slices[-1] == r.chunks and slices[0] == 2
    x, w, which = SK.onehot_operands(h)
    assert bool((x.half().float() == x).all()) and float(x.max()) < 2048
    assert x.flatten().unique().numel() == x.numel()
    dense = SK.packed_k_order(w, c)
    hits = (dense != 0).sum(0).view(c.k_tap // c.kb, c.ntaps, c.kb)
    for cb in range(c.k_tap // c.kb):
        for ch in range(c.kb):
            assert hits[cb, :, ch].tolist() == [1 if cb * c.kb + ch < c.cin else 0] * c.ntaps
    assert bool(((dense != 0).sum(1) == 1).all())
    y = F.conv2d(x.double(), w.double(), None, 1, (c.k - 1) // 2)
    mid = c.H // 2
    for f, (chan, tap, sign) in enumerate(which):
        if c.H == 3:
            assert float(y[0, f, mid, mid]) == sign * (9 * chan + tap + 1)
        elif c.k == 1 or tap == 4:
            assert float(y[0, f, 0, 0]) == sign * (chan + 1)
        else:
            assert float(y[0, f, 0, 0]) == 0.0


def test_onehot_cases_cover_both_k_orders():
    hs = SK.ONEHOT_CASES
    assert {h.expect for h in hs} == set(SK.INSTANCES)
    assert {(h.expect, h.k) for h in hs} == {(i, k) for i in SK.INSTANCES for k in (1, 3)}
    # chunks of 32 with more than one channel block, 3x3, with the tap identified; a padded channel count on either instance
    assert any(h.expect == SK.K32 and h.k == 3 and h.cin > 32 and h.image == "3x3" for h in hs)
    assert {h.expect for h in hs if h.cin % 32} == set(SK.INSTANCES)
    assert all(h.image == "1x1" or h.k == 3 for h in hs)
