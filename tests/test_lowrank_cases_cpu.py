"""Coverage of tests/test_lowrank_instances_gpu.py, proved without a GPU: what mcamd_conv_fwd_lowrank can launch (asked from
the launch's own choice through mcamd_conv_fwd_lowrank_info), that the cases of tests/lowrank_cases.py reach all four
lowrank_kernel<R> instances with a padded and an unpadded rank, both kernel sizes, both K orders, every destination form and
every named boundary condition, that EQUAL is the right comparison for every case, and that a lost, doubled or misplaced K
chunk of either GEMM cannot go unseen."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
import lowrank_cases as LR  # noqa: E402
import splitk_cases as SK  # noqa: E402
from util import fill_padded  # noqa: E402

CASES = LR.LOWRANK_CASES


def test_lowrank_instances_are_the_expected_set():
    """lowrank_kernel<64> / <128> / <192> / <256> and no other, over ranks 32 .. 256, both kernel sizes, every input-channel
    count from 8 to 1024 and every filter count from 8 to 1344 in steps of 8."""
    assert LR.reachable() == set(LR.INSTANCES)


def test_lowrank_cases_reach_every_instance_and_boundary():
    assert len({c.name for c in CASES}) == len(CASES)
    seen = set()
    for c in CASES:
        info = LR.info_of(c)
        assert LR.expect_of(info) == c.expect, (c.name, LR.expect_of(info))
        assert (info.bm, info.bn, info.bk) == (LR.BM, LR.BN, LR.BK)
        t = LR.boundary_tags(c, info)
        assert set(c.tags) <= t, (c.name, set(c.tags) - t)
        seen |= t
        assert c.M <= 700 and c.cin <= 128 and c.cout <= 392, c.name
    assert set(LR.BOUNDARIES) - seen == set()
    assert {c.r for c in CASES} == set(LR.RANKS)
    for inst in LR.INSTANCES:
        mine = [c for c in CASES if c.instance == inst]
        assert {c.dst for c in mine} == set(LR.FORMS), inst
        assert {c.k for c in mine} == {1, 3} and {c.kb for c in mine} == {32, 64}, inst
        assert {c.r for c in mine} == {inst, inst - 32}, inst
        assert any(c.kb == 64 and c.k == 3 for c in mine) and any(c.kb == 32 and c.k == 3 for c in mine), inst
    assert {(c.cin, c.k_tap, c.kb, c.k) for c in CASES if c.k_tap > c.cin} == {(40, 64, 64, 3), (72, 96, 32, 3)}
    # four N tiles with one chunk each; the padded second round; a pooled tile across images beyond the first round
    assert any(c.r == 32 and c.cout == 392 and LR.info_of(c).ntiles == 4 for c in CASES)
    assert any((c.B, c.H, c.W) == (4, 13, 13) and c.expect[1:] == (11, 2, 16) for c in CASES)
    assert any(c.pooled and c.expect[1] == 9 and (c.H * c.W) % 64 for c in CASES)
    # the three planted cases, each with its twin
    planted = [c for c in CASES if c.plant and not c.twin]
    assert sorted(c.plant for c in planted) == ["both", "h", "y"]
    assert all(c.name + ".twin" in LR.BY_NAME for c in planted) and sum(c.twin for c in CASES) == 3
    # test_no_history: large values at rank 256 first, then ranks 32 and 160; test_deterministic: one case per instance
    a, b, c3 = (LR.BY_NAME[n] for n in LR.NO_HISTORY)
    assert (a.r, a.absolute, b.r, c3.r) == (256, True, 32, 160)
    assert float(LR.reference_of(a.name)[1].abs().mean()) > 2048
    assert sorted(LR.BY_NAME[n].instance for n in LR.DETERMINISM_CASES) == list(LR.INSTANCES)


@pytest.mark.parametrize("c", CASES, ids=str)
def test_lowrank_case_is_exact(c):
    """The conditions under which the kernel output must EQUAL the reference (the module text of lowrank_cases.py), on the
    reference's own operands, and a sentinel arrangement that leaves the reference finite: the convolution of the
    NaN-surrounded operand buffer's slice (zero halo, zero channels beyond cin) IS the reference's H."""
    o = LR.operands(c.name)
    want, h, clamped, ref = LR.reference_of(c.name)
    hs = LR.sat_half(h)
    assert float(o.x.abs().max()) * float(o.u.abs().max()) * c.ktot < 2 ** 24
    assert float(hs.abs().max()) * float(o.v.abs().max()) * c.r < 2 ** 24
    # every partial sum of phase 2 in every order: below 2^24 units of the smallest term (1, or 2^-6 in the case that has it)
    unit = float(o.v[o.v != 0].abs().min())
    assert unit in (1.0, 2.0 ** -6) and bool((hs == hs.round()).all()) and bool((o.v / unit == (o.v / unit).round()).all())
    bound = F.conv2d(hs.abs(), o.v.double().abs().view(c.cout, c.r, 1, 1))
    assert float(bound.max()) / unit < 2 ** 24
    # the epilogue in fp32: Y, Y * scale and Y * scale + shift are fp32 numbers (fused or not), so is the slope's product
    y = F.conv2d(hs, o.v.double().view(c.cout, c.r, 1, 1))
    ys = y if o.scale is None else y * o.scale.double().view(1, -1, 1, 1)
    z = ys + o.shift.double().view(1, -1, 1, 1)
    for t in (y, ys, z, z * LR.SLOPE):
        assert torch.equal(t.float().double(), t)
    assert all(bool(torch.isfinite(w).all()) for w in want) and len(want) == (2 if c.dst == "pool+y2" else 1)
    assert clamped == bool(c.plant and not c.twin)
    # what each planted case clamps
    h_over, y_over = bool((h.abs() > LR.F16_MAX).any()), bool((torch.where(z > 0, z, z * LR.SLOPE).abs() > LR.F16_MAX).any())
    assert (h_over, y_over) == {None: (False, False), "h": (True, False), "y": (False, True), "both": (True, True)}[None if c.twin else c.plant]
    if c.plant == "h" and not c.twin:          # the clamp of H, not only the flag, shows in a stored element
        assert not torch.equal(LR.reference(o, clamp_h=False)[0], ref)
    if c.plant == "both" and not c.twin:       # ... at a pixel of the tail tile
        assert (LR.PLANT_PIXEL[0] * c.W + LR.PLANT_PIXEL[1]) // LR.BM == c.expect[1] - 1 and float(h[0, LR.PLANT_ROW][LR.PLANT_PIXEL]) == 65536.0
    if c.absolute:                             # the rounding of the intermediate shows
        assert not torch.equal(h.half().double(), h)
    # the operand buffer the launch reads
    buf = fill_padded(torch.device("cpu"), c, o.x.half(), c.x_ld, c.x_choff, c.k_tap, 0)
    view = ops.padded_view(buf, c.B, c.H, c.W, c.x_ld, 0)
    sl = view[..., c.x_choff:c.x_choff + c.k_tap]
    assert bool(torch.isfinite(sl).all()) and bool((sl[..., c.cin:] == 0).all())
    assert bool(torch.isnan(view[..., :c.x_choff]).all()) and bool(torch.isnan(view[..., c.x_choff + c.k_tap:]).all())
    up = torch.zeros(c.r, c.k_tap, c.k, c.k)
    up[:, :c.cin] = o.u
    xs = sl.permute(0, 3, 1, 2).float()
    if c.k == 1:
        xs = xs[:, :, 1:-1, 1:-1]
    assert torch.equal(F.conv2d(xs, up).double(), h)         # fp32: exact under the first bound
    assert sorted(SK.row_pixels(c).tolist()) == list(range(c.M))


@pytest.mark.parametrize("c", CASES, ids=str)
def test_every_chunk_is_visible(c):
    """For every pixel tile: the contribution of every single K chunk of phase 1 (32 packed K values) to H is non-zero
    somewhere in the tile; for every (pixel tile, N tile): that of every single chunk of phase 2 (32 rank columns) to Y is
    non-zero at an element that is not clamped.  A chunk that is lost, doubled or swapped for another then changes an
    element of the exact result by at least one unit.  The chunks restate both GEMMs: their sums are H and Y."""
    o = LR.operands(c.name)
    _, h, _, _ = LR.reference_of(c.name)
    p1 = LR.phase1_chunks(c, o)
    assert tuple(p1.shape) == (c.ktot // LR.BK, c.M, c.r) and torch.equal(p1.sum(0), LR.in_row_order(c, h))
    seen1 = SK.tile_any(p1 != 0, LR.BM, c.r)
    assert tuple(seen1.shape) == (c.ktot // LR.BK, c.expect[1], 1)
    assert bool(seen1.all()), "%s: phase-1 chunks add nothing to tiles %s" % (c.name, (~seen1).nonzero().tolist())
    p2 = LR.phase2_chunks(c, o, h)
    y = F.conv2d(LR.sat_half(h), o.v.double().view(c.cout, c.r, 1, 1))
    assert torch.equal(p2.sum(0), LR.in_row_order(c, y))
    z = (y if o.scale is None else y * o.scale.double().view(1, -1, 1, 1)) + o.shift.double().view(1, -1, 1, 1)
    free = LR.in_row_order(c, torch.where(z > 0, z, z * LR.SLOPE).abs() <= LR.F16_MAX)
    seen2 = SK.tile_any((p2 != 0) & free, LR.BM, LR.BN)
    assert tuple(seen2.shape) == (c.r // LR.BK,) + c.expect[1:3]
    assert bool(seen2.all()), "%s: phase-2 chunks add nothing to tiles %s" % (c.name, (~seen2).nonzero().tolist())


@pytest.mark.parametrize("h", LR.ONEHOT_CASES, ids=LR.onehot_id)
def test_onehot_filters_cover_every_k(h):
    """One filter per real (channel, tap): every k of the packed order that a real channel occupies is selected by exactly
    one filter, the values are distinct fp16 integers below 2048, every batch is a legal launch with V the identity, and
    the reference output of a filter is the value at its own (channel, tap)."""
    x, u, which, batches = LR.onehot_operands(h)
    assert bool((x.half().float() == x).all()) and float(x.max()) < 2048 and x.flatten().unique().numel() == x.numel()
    c = batches[0].case
    dense = SK.packed_k_order(u, c)
    hits = (dense != 0).sum(0).view(c.k_tap // c.kb, c.ntaps, c.kb)
    for cb in range(c.k_tap // c.kb):
        for ch in range(c.kb):
            assert hits[cb, :, ch].tolist() == [1 if cb * c.kb + ch < h.cin else 0] * c.ntaps
    assert bool(((dense != 0).sum(1) == 1).all()) and len(which) == h.k * h.k * h.cin
    assert sum(min(256, len(which) - b.f0) for b in batches) == len(which)
    for b in batches:
        assert b.r % 32 == 0 and 32 <= b.r <= 256 and ops.conv_fwd_lowrank_ok(LR.geom_of(b.case), b.r)
        assert torch.equal(b.v, torch.eye(b.r)) and b.cout == b.r and b.scale is None and b.shift is None
        y = LR.reference(b)[0]
        for f in range(min(256, len(which) - b.f0)):
            chan, tap = which[b.f0 + f]
            dy, dx = (tap // h.k, tap % h.k) if h.k == 3 else (1, 1)
            assert float(y[0, f, 1, 1]) == 9 * chan + 3 * dy + dx + 1


def test_onehot_cases_cover_both_k_orders():
    got = {(h.k, h.cin, 64 if ops.round_up(h.cin, 32) % 64 == 0 else 32) for h in LR.ONEHOT_CASES}
    assert got == {(k, cin, kb) for k in (1, 3) for cin, kb in ((64, 64), (128, 64), (96, 32), (40, 64))}
    # between them the batches run every instance: ranks 64 / 128 / 96 / 256 (k = 1, the batch of 40 filled to 64) and more
    ranks = {b.r for h in LR.ONEHOT_CASES for b in LR.onehot_operands(h)[3]}
    assert {ops.round_up(r, 64) for r in ranks} >= {64, 128, 256}
