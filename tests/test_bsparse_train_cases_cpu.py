"""Coverage of tests/test_bsparse_train_instances_gpu.py, proved without a GPU: what mcamd_conv_fwd_bsparse_raw and
mcamd_conv_dgrad_bsparse can launch (asked from the launch's own choice through mcamd_conv_bsparse_train_info), that the
cases of tests/bsparse_train_cases.py reach all four raw-epilogue instances forward with statistics, forward without and
dgrad, with both kernel sizes, both `pad` forms, offset slices, ragged tiles, every list length around the ring's depth and
every mask kind, that EQUAL is the right comparison for every case, and that the dgrad lists are bsparse_ref.chunk_lists
on a numpy restatement of the dgrad packing."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops, _lib as L  # noqa: E402
import bsparse_train_cases as TC  # noqa: E402
import bsparse_ref as R  # noqa: E402


def test_train_queries_follow_the_switch_and_the_rules(setenv):
    g = ops.geom(2, 13, 13, 3, 64, 200, 64)
    setenv(TC.BM_ENV, "128")
    assert tuple(ops.conv_bsparse_train_info(g)) == tuple(ops.conv_fwd_bsparse_info(g)) == (128, 64, 64, 3, 3, 4, 32)
    # dgrad: N = cin = 64 (one tile), K chunks of 32 over cout_p = 224
    assert tuple(ops.conv_bsparse_train_info(g, dgrad=True)) == (128, 64, 32, 4, 3, 1, 8)
    assert ops.bsparse_elems_dgrad(g) == (1, 9 * 224 // 32)
    assert ops.bsparse_raw_stats_rows(g) == 3 and ops.bsparse_raw_stats_rows(g, dgrad=True) == 3
    setenv(TC.BM_ENV, "64")
    assert tuple(ops.conv_bsparse_train_info(g, dgrad=True)) == (64, 64, 32, 4, 6, 1, 8)
    assert ops.bsparse_raw_stats_rows(g) == 6
    # eligibility: the forward's rule forward; dgrad: cin % 8 == 0; stem, x_wrap, x_f8 refused in both directions
    g40 = ops.geom(2, 13, 13, 3, 40, 200, 64)
    assert not ops.conv_bsparse_train_ok(g40) and ops.conv_bsparse_train_ok(g40, dgrad=True)
    assert not ops.conv_bsparse_train_ok(ops.geom(2, 13, 13, 3, 36, 200, 64), dgrad=True)
    assert ops.bsparse_raw_stats_rows(g40) == 0
    with pytest.raises(L.McamdError):
        ops.conv_bsparse_train_info(g40)
    for field, value in (("stem", 1), ("x_wrap", 128), ("x_f8", 64)):
        h = ops.geom(2, 13, 13, 3, 64, 200, 64)
        setattr(h, field, value)
        assert not ops.conv_bsparse_train_ok(h) and not ops.conv_bsparse_train_ok(h, dgrad=True), field
    assert len(L.SIGNATURES["mcamd_conv_bsparse_train_info"][1]) == 3


def test_train_cases_reach_every_instance_in_every_form(setenv):
    cs = TC.TRAIN_CASES
    assert len({c.name for c in cs}) == len(cs)
    reached = {f: set() for f in TC.FORMS}
    cover = {(d, i): {"kpad": set(), "len": set(), "mask": set(), "choff": set(), "ragged": set(), "sat": set()}
             for d in ("fwd", "dgrad") for i in TC.INSTANCES}
    for c in cs:
        TC.apply_env(c, setenv)
        assert ops.conv_bsparse_train_ok(TC.geom_of(c), c.dgrad), c.name
        r = TC.info_of(c)
        assert (r.bm, r.bk, r.stages) == c.expect and r.bn == R.FILTERS, (c.name, r)
        assert r.mtiles == -(-c.M // r.bm) and r.ntiles == c.ntiles == -(-c.n // 64) and r.bk == c.kb
        assert ops.bsparse_raw_stats_rows(TC.geom_of(c), c.dgrad) == r.mtiles
        reached[c.form].add(c.expect)
        cv = cover["dgrad" if c.dgrad else "fwd", c.expect]
        cv["kpad"].add((c.k, c.pad))
        cv["mask"].add(c.mask)
        if c.y_choff > 0 and c.y_ld > c.y_choff + c.n:
            cv["choff"].add("y")
        if c.choff > 0 and c.ld > c.choff + c.kpad:
            cv["choff"].add("in")
        if c.M % r.bm:
            cv["ragged"].add("M")
        if c.n % 64:
            cv["ragged"].add("N")
        if c.overflow:
            cv["sat"].add(c.M % r.bm != 0)
        o, _ = TC.operands_and_reference(c)
        _, count, _ = TC.lists_ref(c, o)
        cv["len"] |= {int(n) for n in count if n < c.nchunks} | ({-1} if (count == c.nchunks).any() else set())
        assert c.B == 2 and (c.H, c.W) in ((13, 13), (8, 8)) and c.cin in (32, 64, 96, 128) and c.cout in (40, 64, 72, 136), c.name
    for f in TC.FORMS:
        assert reached[f] == set(TC.INSTANCES), (f, reached[f])
    for (d, inst), cv in cover.items():
        assert cv["kpad"] == {(1, 0), (1, 1), (3, 0), (3, 1)}, (d, inst, cv["kpad"])
        assert cv["mask"] == set(TC.MASK_KINDS), (d, inst)
        assert cv["choff"] == {"y", "in"} and cv["ragged"] == {"M", "N"}, (d, inst, cv)
        assert TC.ring_lengths(inst[2], -1) <= cv["len"], (d, inst, TC.ring_lengths(inst[2], -1) - cv["len"])
        assert True in cv["sat"], (d, inst)
    for f in TC.FORMS:
        for inst in TC.INSTANCES:
            c = TC.foreign_case(f, inst)
            TC.apply_env(c, setenv)
            r = TC.info_of(c)
            assert (r.bm, r.bk, r.stages) == inst and r.ntiles == 1 and c.nchunks > r.stages
            o, ref = TC.operands_and_reference(c)
            assert TC.exactness(c, o, ref) == [] and TC.lists_ref(c, o)[1].tolist() == [c.nchunks]


@pytest.mark.parametrize("c", TC.TRAIN_CASES, ids=str)
def test_train_case_is_exact(c):
    """conv_cases.exactness on the case's own reference, the lists the mask was built for, and for the dgrad the numpy
    packing against the forward restatement applied to the GEMM view of the same weights."""
    for plant in ((True, False) if c.overflow else (True,)):
        o, ref = TC.operands_and_reference(c, plant)
        assert TC.exactness(c, o, ref) == [], c.name
        assert bool(torch.isfinite(ref.y).all()) and tuple(ref.y.shape) == (c.B, c.n, c.H, c.W)
        assert len(o.planted) == (2 if c.overflow and plant else 0)
        assert (ref.s1 is not None) == c.stats
    o, ref = TC.operands_and_reference(c)
    assert tuple(o.w.shape) == tuple(o.mask.shape) == (c.cout, c.cin, c.k, c.k)
    packed, count, lst = TC.lists_ref(c, o)
    nch = c.nchunks
    assert packed.shape == (ops.round_up(c.n, 256), c.ktot)
    assert count.shape == (c.ntiles,) and lst.shape == (c.ntiles, nch)
    for t in range(c.ntiles):
        assert (np.diff(lst[t, :count[t]]) > 0).all() and (lst[t, count[t]:] == 0).all()
    if c.dgrad:
        # the dgrad packing is the forward packing of the transposed, tap-flipped, cout-padded tensor
        wm = (o.w * o.mask).numpy()
        v = np.zeros((c.cin, c.kpad, c.k, c.k), np.float32)
        v[:, :c.cout] = wm.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]
        assert np.array_equal(packed.view(np.uint16), R.pack_fwd(v).view(np.uint16))
        # ... and element by element from the header's formula, on a few places
        rng = np.random.RandomState(1)
        for _ in range(64):
            n, ci, ty, tx = rng.randint(c.cout), rng.randint(c.cin), rng.randint(c.k), rng.randint(c.k)
            tt = ty * c.k + tx
            kpos = (n // c.kb) * c.ntaps * c.kb + tt * c.kb + n % c.kb
            assert packed[ci, kpos] == np.float16(wm[n, ci, c.k - 1 - ty, c.k - 1 - tx])
    bits = packed.view(np.uint16)
    if c.mask == "block":
        for t, n in enumerate(c.counts):
            if n is not TC.RANDOM:
                assert count[t] == (nch if n == TC.ALL else n), (c.name, t, count[t], n)
    elif c.mask == "unstructured":
        assert (count == nch).all() and float((o.mask == 0).float().mean()) > 0.5
    elif c.mask == "single":
        listed = 0
        for t in range(c.ntiles):
            for q in range(nch):
                nz = int((packed[t * 64:(t + 1) * 64, q * c.kb:(q + 1) * c.kb] != 0).sum())
                assert nz <= 1 and (nz == 1) == (q in lst[t, :count[t]])
                listed += nz
        assert listed >= c.ntiles * nch // 2          # (a kept weight may fall on a padded cout column of the dgrad: then the block is empty)
    else:
        for t in range(c.ntiles):
            q = t % nch
            blk = bits[t * 64:min((t + 1) * 64, c.n), q * c.kb:(q + 1) * c.kb].reshape(-1, c.kb)[:, :min(c.kb, c.kreal)]
            assert (blk == 0x8000).all() and q not in lst[t, :count[t]], (c.name, t)
        assert (count > 0).all()
    if c.stats:
        s1, s2 = TC.stats_reference(ref)
        assert torch.equal(s1, ref.y.sum((0, 2, 3))) and torch.equal(s2, (ref.y * ref.y).sum((0, 2, 3)))


def test_an_empty_list_and_a_shifted_read_are_visible():
    """Every form has a tile with an empty list (zeros and zero statistics must be STORED: the outputs start as NaN), and on
    every instance in both directions a tile whose list is shorter than the chunk count and does not start with chunk 0."""
    for f in ("fwd-stats", "dgrad"):
        assert any((TC.lists_ref(c, TC.operands_and_reference(c)[0])[1] == 0).any() for c in TC.TRAIN_CASES if c.form == f), f
    for d in (False, True):
        for inst in TC.INSTANCES:
            found = False
            for c in (c for c in TC.TRAIN_CASES if c.expect == inst and c.dgrad == d):
                _, count, lst = TC.lists_ref(c, TC.operands_and_reference(c)[0])
                found |= any(0 < count[t] < c.nchunks and lst[t, 0] != 0 for t in range(c.ntiles))
            assert found, (d, inst)


def test_the_statistics_convention_is_visible(setenv):
    """On every instance a forward with statistics clamps: sums of the stored values differ from sums of the accumulators,
    and the reference's sums are exact fp32 numbers in every order (bsparse_train_cases.stats_saturate_exactness)."""
    for inst in TC.INSTANCES:
        c = TC.stats_saturate_case(inst)
        TC.apply_env(c, setenv)
        r = TC.info_of(c)
        assert (r.bm, r.bk, r.stages) == inst and c.stats and c.overflow and c.M % r.bm
        o, ref = TC.operands_and_reference(c)
        assert TC.stats_saturate_exactness(c, o, ref) == []
        assert len(o.planted) == 2 and all(abs(float(ref.y[b, ch, h, x])) == 65504.0 for (b, ch, h, x, _) in o.planted)
