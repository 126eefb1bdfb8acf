"""Coverage of tests/test_bsparse_instances_gpu.py, proved without a GPU: what mcamd_conv_fwd_bsparse can launch (asked from
the launch's own choice through mcamd_conv_fwd_bsparse_info), that the cases of tests/bsparse_cases.py reach all of it with
every destination form, both `pad` forms, every named boundary condition, every list length around the ring's depth and
every mask kind, that EQUAL is the right comparison for every case, and that a list entry the kernel skips, repeats or
reads one place off cannot go unseen."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops, _lib as L  # noqa: E402
import bsparse_cases as BC  # noqa: E402
import bsparse_ref as R  # noqa: E402
from util import fill_padded  # noqa: E402


def test_bsparse_instances_are_the_expected_set(setenv):
    """The four bsparse_kernel instances, and no other, over both settings of MCAMD_BSPARSE_BM, every accepted channel count
    and every filter count up to 1344, both kernel sizes, both `pad` forms and images from one pixel to the training batch."""
    assert BC.reachable(setenv) == set(BC.INSTANCES)


def test_bsparse_info_follows_the_switch(setenv):
    g = ops.geom(2, 13, 13, 3, 64, 200, 64)
    setenv(BC.BM_ENV, "128")
    assert tuple(ops.conv_fwd_bsparse_info(g)) == (128, 64, 64, 3, 3, 4, 32)
    setenv(BC.BM_ENV, "64")
    assert tuple(ops.conv_fwd_bsparse_info(g)) == (64, 64, 64, 3, 6, 4, 32)
    assert tuple(ops.conv_fwd_bsparse_info(ops.geom(2, 13, 13, 3, 96, 200, 96, pad=1))) == (64, 64, 32, 4, 6, 4, 32)
    with pytest.raises(L.McamdError):
        ops.conv_fwd_bsparse_info(ops.geom(2, 13, 13, 3, 40, 200, 64))        # cin % 32 != 0: no block form
    assert len(L.SIGNATURES["mcamd_conv_fwd_bsparse_info"][1]) == 2


def test_bsparse_cases_reach_every_instance_and_boundary(setenv):
    cs = BC.BSPARSE_CASES
    assert len({c.name for c in cs}) == len(cs)
    tags_of = {i: set() for i in BC.INSTANCES}
    lengths = {i: set() for i in BC.INSTANCES}
    for c in cs:
        BC.apply_env(c, setenv)
        assert ops.conv_fwd_bsparse_ok(BC.geom_of(c)), c.name
        r = BC.info_of(c)
        assert (r.bm, r.bk, r.stages) == c.expect, (c.name, r)
        t = BC.boundary_tags(c, r)
        assert set(c.tags) <= t, (c.name, r, set(c.tags) - t)
        tags_of[c.expect] |= t
        o, _ = BC.operands_and_reference(c)
        _, count, _ = BC.lists_ref(c, o)
        # a length counts for the ring's edge cases where the tile has more chunks than that (the last entry: every chunk)
        lengths[c.expect] |= {int(n) for n in count if n < c.nchunks} | ({-1} if (count == c.nchunks).any() else set())
    for inst in BC.INSTANCES:
        bm, bk, stages = inst
        want = set(BC.BOUNDARIES_ALL + (BC.BOUNDARIES_K32 if bk == 32 else ()))
        assert want <= tags_of[inst], (inst, want - tags_of[inst])
        mine = [c for c in cs if c.expect == inst]
        assert {c.dst for c in mine} == set(BC.DSTS), (inst, {c.dst for c in mine})
        assert {c.mask for c in mine} == set(BC.MASK_KINDS), inst
        need = (BC.ring_lengths(stages, -1))
        assert need <= lengths[inst], (inst, need - lengths[inst])
        sat = [c for c in mine if c.overflow]
        assert sat and any(c.M % bm for c in sat), inst
    long_list = [c for c in cs if c.base == BC.LONG_LIST]
    assert len(long_list) == 1
    c = long_list[0]
    assert (c.B, c.H, c.W, c.k, c.cin, c.cout, c.draw, c.wdraw) == (1, 13, 13, 3, 1280, 72, "s4", "s4u") and c.nchunks == 180
    assert all(c.base == BC.LONG_LIST or (c.M <= 700 and c.cin <= 256) for c in cs)
    assert {next(c for c in cs if c.name == n).expect for n in BC.DETERMINISM_CASES} == set(BC.INSTANCES)
    for inst in BC.INSTANCES:
        c = BC.foreign_case(inst)
        BC.apply_env(c, setenv)
        r = BC.info_of(c)
        assert (r.bm, r.bk, r.stages) == inst and r.ntiles == 1 and c.nchunks > r.stages
        o, ref = BC.operands_and_reference(c)
        assert BC.exactness(c, o, ref) == [] and BC.lists_ref(c, o)[1].tolist() == [c.nchunks]


@pytest.mark.parametrize("c", BC.BSPARSE_CASES, ids=str)
def test_bsparse_case_is_exact(c):
    """The conditions under which the kernel output must EQUAL the reference (conv_cases.exactness), the lists the mask was
    built for -- from bsparse_ref.chunk_lists on bsparse_ref.pack_fwd, the restatement the GPU test holds mcamd_bsparse_lists
    to --, and a sentinel arrangement that leaves the reference finite."""
    for plant in ((True, False) if c.overflow else (True,)):
        o, ref = BC.operands_and_reference(c, plant)
        assert BC.exactness(c, o, ref) == [], c.name
        assert bool(torch.isfinite(ref.y).all()) and (ref.y2 is None or bool(torch.isfinite(ref.y2).all()))
        assert (ref.y2 is not None) == (c.dst == "pool+y2")
        assert len(o.planted) == (2 if c.overflow and plant else 0)
    o, ref = BC.operands_and_reference(c)
    packed, count, lst = BC.lists_ref(c, o)
    nch = c.nchunks
    assert count.shape == (c.ntiles,) and lst.shape == (c.ntiles, nch)
    for t in range(c.ntiles):
        assert (np.diff(lst[t, :count[t]]) > 0).all() and (lst[t, count[t]:] == 0).all()
    bits = packed.view(np.uint16)
    if c.mask == "block":
        for t, n in enumerate(c.counts):
            if n is not BC.RANDOM:
                assert count[t] == (nch if n == BC.ALL else n), (c.name, t, count[t], n)
    elif c.mask == "unstructured":
        assert (count == nch).all()
        assert float((o.mask == 0).float().mean()) > 0.5          # most weights are gone, and still every list is full
    elif c.mask == "single":
        seen_cols, seen_rows = set(), set()
        for t in range(c.ntiles):
            for q in range(nch):
                blk = packed[t * R.FILTERS:(t + 1) * R.FILTERS, q * c.kb:(q + 1) * c.kb]
                j = t * nch + q
                if j % 5 == 4:
                    assert not blk.any() and q not in lst[t, :count[t]]
                    continue
                assert int((blk != 0).sum()) == 1 and q in lst[t, :count[t]]
                row, col = (int(v[0]) for v in np.nonzero(blk))
                assert (row, col) == BC.single_position(c, j)
                seen_cols.add(col // 8)
                seen_rows.add(row)
        assert seen_cols == set(range(c.kb // 8)) and {0, R.FILTERS - 1} <= seen_rows and len(seen_rows) > 2
    else:
        # "negzero": in every tile a block of -0.0 only (bit pattern 0x8000 in all 64 x kb places), and it is not listed
        for t in range(c.ntiles):
            q = t % nch
            blk = bits[t * R.FILTERS:min((t + 1) * R.FILTERS, c.cout), q * c.kb:(q + 1) * c.kb]
            assert (blk == 0x8000).all() and q not in lst[t, :count[t]], (c.name, t)
        assert (count > 0).all()
    # the sentinels
    ld = c.ld or c.cin
    buf = fill_padded(torch.device("cpu"), c, o.act, ld, c.choff, c.cin, c.pad)
    view = ops.padded_view(buf, c.B, c.H, c.W, ld, c.pad)
    sl = view[..., c.choff:c.choff + c.cin]
    assert bool(torch.isfinite(sl).all())
    assert bool(torch.isnan(view[..., :c.choff]).all()) and bool(torch.isnan(view[..., c.choff + c.cin:]).all())
    xs = sl.permute(0, 3, 1, 2).float()
    if c.k == 1:
        xs = xs[:, :, 1:-1, 1:-1]
    acc = F.conv2d(xs, o.w * o.mask)                         # fp32: exact under the accumulator bound
    assert torch.equal(acc.double(), ref.acc)


@pytest.mark.parametrize("c", BC.BSPARSE_CASES, ids=str)
def test_every_listed_chunk_is_visible(c):
    """For every (M tile, N tile) and every chunk the tile lists, that chunk's contribution is non-zero in at least one
    element of the tile whose value is not clamped: a kernel that stops one entry early, reads entry i twice or reads entry
    i + 1 in place of entry i changes an element of the exact result by at least one unit.  A chunk that is not listed
    contributes nothing anywhere in the tile (so full lists give the same result)."""
    o, ref = BC.operands_and_reference(c)
    _, count, lst = BC.lists_ref(c, o)
    P = BC.chunk_contributions(c, o)
    rows = ref.acc.permute(0, 2, 3, 1).reshape(c.M, c.cout)[BC.row_pixels(c)]
    assert torch.equal(P.sum(0), rows)
    seen = BC.tile_any((P != 0) & ~BC.clamped_mask(c, o), c.bm, R.FILTERS)      # [nchunks][mtiles][ntiles]
    touched = BC.tile_any(P != 0, c.bm, R.FILTERS)
    for t in range(c.ntiles):
        listed = set(lst[t, :count[t]].tolist())
        for q in range(c.nchunks):
            if q in listed:
                assert bool(seen[q, :, t].all()), "%s: chunk %d adds nothing to M tiles %s of N tile %d" % (
                    c.name, q, (~seen[q, :, t]).nonzero().flatten().tolist(), t)
            else:
                assert not bool(touched[q, :, t].any())


def test_a_shifted_list_read_is_visible():
    """On every instance some tile's list is shorter than the chunk count and does not start with chunk 0: reading entry
    i + 1 in place of entry i then drops its first chunk -- seen, by the test above -- and reads the filler behind the count,
    chunk 0, which that tile does not list and which therefore adds nothing back."""
    for inst in BC.INSTANCES:
        found = False
        for c in (c for c in BC.BSPARSE_CASES if c.expect == inst):
            o, _ = BC.operands_and_reference(c)
            _, count, lst = BC.lists_ref(c, o)
            found |= any(0 < count[t] < c.nchunks and lst[t, 0] != 0 for t in range(c.ntiles))
        assert found, inst
