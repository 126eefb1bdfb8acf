"""Coverage of tests/test_sparse_instances_gpu.py, proved without a GPU: what mcamd_conv_fwd_sparse24 can launch (asked from
the launch's own choice through mcamd_conv_fwd_sparse24_info), that the cases of tests/sparse_cases.py reach all of it with
every destination form and every named boundary condition, and that EQUAL is the right comparison for every case."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops, _lib as L  # noqa: E402
import sparse_cases as SC  # noqa: E402
from util import fill_padded  # noqa: E402


def test_sparse24_instances_are_the_expected_set(setenv):
    """The five sparse24_kernel instances, and no other, over both settings of MCAMD_SPARSE_WIDE, every filter and channel
    count from 8 to 1344 in steps of 8, both kernel sizes and images from one pixel to the training batch."""
    assert SC.reachable(setenv) == {i + (2,) for i in SC.INSTANCES}


def test_sparse24_info_follows_the_switch(setenv):
    g = ops.geom(2, 13, 13, 3, 64, 512, 64)
    setenv("MCAMD_SPARSE_WIDE", "1")
    assert tuple(ops.conv_fwd_sparse24_info(g)) == (256, 128, 64, 2, 3, 2, 16)
    setenv("MCAMD_SPARSE_WIDE", "0")
    assert tuple(ops.conv_fwd_sparse24_info(g)) == (128, 128, 64, 2, 3, 4, 32)
    with pytest.raises(L.McamdError):
        ops.conv_fwd_sparse24_info(ops.geom(2, 13, 13, 3, 62, 512, 64))       # cin % 4 != 0: no 2:4 form


def test_sparse_cases_reach_every_instance_and_boundary(setenv):
    cs = SC.SPARSE_CASES
    assert len({c.name for c in cs}) == len(cs)
    tags_of = {"64": set(), "wide": set()}
    for c in cs:
        SC.apply_env(c, setenv)
        assert ops.conv_fwd_sparse24_ok(SC.geom_of(c)), c.name
        r = SC.info_of(c)
        assert (r.bmw, r.bnp, r.bk) == c.expect, (c.name, r)
        t = SC.boundary_tags(c, r)
        assert set(c.tags) <= t, (c.name, r, set(c.tags) - t)
        tags_of["64" if r.bmw == 64 else "wide"] |= t
    missing = {"64": set(SC.BOUNDARIES_BOTH + SC.BOUNDARIES_64) - tags_of["64"],
               "wide": set(SC.BOUNDARIES_BOTH + SC.BOUNDARIES_WIDE) - tags_of["wide"]}
    assert missing == {"64": set(), "wide": set()}, missing
    for inst in SC.INSTANCES:
        mine = [c for c in cs if c.expect == inst]
        assert {c.dst for c in mine} == set(SC.DSTS), (inst, {c.dst for c in mine})
        assert {c.k for c in mine} == {1, 3}, inst
        assert {c.mask for c in mine} >= {"two", "upto2"}, inst
    for kind in SC.MASK_KINDS:
        assert sum(1 for c in cs if c.mask == kind) >= 3, kind
    assert {c.cin for c in cs if c.k_tap > c.cin} >= set(SC.PADDED_CINS)
    assert any(c.cin == 1280 and c.k == 3 and (c.B, c.H, c.W) == (2, 13, 13) and (c.draw, c.wdraw) == ("s4", "s4u") for c in cs)
    assert all(c.cin <= 264 or c.cin == 1280 for c in cs)
    # the 32-channel K order [channel block][tap][32] with more than one block, 3x3
    assert any(c.kb == 32 and c.k == 3 and c.k_tap > 32 for c in cs)
    assert sum(1 for c in cs if c.overflow) == 1
    assert {next(c for c in cs if c.name == n).expect for n in SC.DETERMINISM_CASES} == set(SC.INSTANCES)
    # one-hot filters: both channel blocks, both kernel sizes, a padded channel count each; every instance
    hs = SC.ONEHOT_CASES
    for h in hs:
        c = SC.onehot_case(h)
        SC.apply_env(c, setenv)
        assert ops.conv_fwd_sparse24_ok(SC.geom_of(c)), c.name
        r = SC.info_of(c)
        assert (r.bmw, r.bnp, r.bk) == h.expect, (c.name, r)
    assert {(SC.onehot_case(h).kb, h.k) for h in hs} == {(32, 1), (64, 1), (32, 3), (64, 3)}
    assert {(SC.onehot_case(h).kb, h.k) for h in hs if h.cin % 32} == {(32, 1), (64, 1), (32, 3), (64, 3)}
    assert {h.expect for h in hs} == set(SC.INSTANCES)
    assert any(h.env for h in hs)
    assert all(h.image == "1x1" or h.k == 3 for h in hs) and {h.image for h in hs if h.k == 3} == {"1x1", "3x3"}


@pytest.mark.parametrize("c", SC.SPARSE_CASES, ids=str)
def test_sparse_case_is_exact(c):
    """The conditions under which the kernel output must EQUAL the reference (conv_cases.exactness: accumulator bound below
    2^24, every reference value an fp16 number), the mask of the kind the case names, a packing with ascending offsets, and
    a sentinel arrangement that leaves the reference finite: the convolution of the NaN-surrounded operand buffer's slice
    (zero halo, zero channels beyond cin) with the effective weights IS the reference's accumulator."""
    for plant in ((True, False) if c.overflow else (True,)):
        o, ref = SC.operands_and_reference(c, plant)
        assert SC.exactness(c, o, ref) == [], c.name
        assert bool(torch.isfinite(ref.y).all()) and (ref.y2 is None or bool(torch.isfinite(ref.y2).all()))
        assert (ref.y2 is not None) == (c.dst == "pool+y2")
        assert len(o.planted) == (2 if c.overflow and plant else 0)
    o, ref = SC.operands_and_reference(c)
    v = o.w if o.mask is None else o.w * o.mask
    cnt = SC.group_counts(v)
    weff = SC.effective(o)
    if c.mask == "bad":
        assert int(cnt.max()) == 4 and bool((cnt == 3).any()) and not torch.equal(weff, v)
        assert int(SC.group_counts(weff).max()) == 2
    else:
        assert int(cnt.max()) == 2 and torch.equal(weff, v)
    if c.mask == "two" and not c.wdraw.startswith("s"):
        assert int(cnt.min()) == 2
        g = (SC._groups(v) != 0)
        for (a, b) in SC.PAIRS:
            assert bool((g[:, :, a] & g[:, :, b]).any()), (c.name, a, b)
    if c.mask == "upto2":
        per_filter = (v != 0).sum((1, 2, 3))
        assert bool((cnt == 0).any()) and bool((cnt == 1).any()) and int(per_filter.min()) == 0 and int(per_filter.max()) > 0
        if c.k == 3:
            assert int((v[:, :, 2, 0] != 0).sum()) == 0
    if c.mask == "none":
        assert o.mask is None and bool((cnt < 2).any())      # kept positions whose weight is exactly 0
    p = SC.pack_ref(c, o.w, o.mask)
    assert bool((p.p0 < p.p1).all())
    assert torch.equal(p.dense, SC.packed_k_order(v, c))
    # (the kept values and offsets rebuild the effective weights, nothing else)
    rebuilt = torch.zeros(c.cout, c.ktot // 4, 4)
    pv = p.vals.float().view(c.cout, c.ktot // 4, 2)
    rebuilt.scatter_(-1, p.p1.unsqueeze(-1), pv[..., 1:2])
    rebuilt.scatter_(-1, p.p0.unsqueeze(-1), pv[..., 0:1])
    assert torch.equal(rebuilt.view(c.cout, c.ktot), SC.packed_k_order(weff, c))
    # the sentinels
    ld = c.ld or c.k_tap
    buf = fill_padded(torch.device("cpu"), c, o.act, ld, c.choff, c.k_tap, c.pad)
    view = ops.padded_view(buf, c.B, c.H, c.W, ld, c.pad)
    sl = view[..., c.choff:c.choff + c.k_tap]
    assert bool(torch.isfinite(sl).all())
    assert bool(torch.isnan(view[..., :c.choff]).all()) and bool(torch.isnan(view[..., c.choff + c.k_tap:]).all())
    wp = torch.zeros(c.cout, c.k_tap, c.k, c.k)
    wp[:, :c.cin] = weff
    xs = sl.permute(0, 3, 1, 2).float()
    if c.k == 1:
        xs = xs[:, :, 1:-1, 1:-1]
    acc = F.conv2d(xs, wp)                                   # fp32: exact under the accumulator bound
    assert torch.equal(acc.double(), ref.acc)


@pytest.mark.parametrize("h", SC.ONEHOT_CASES, ids=SC.onehot_id)
def test_onehot_filters_cover_every_k(h):
    """One filter per real (channel, tap): every k of the packed order that a real channel occupies is selected by exactly
    one filter, the values are fp16 integers, and the reference output is +-(the value that filter selects)."""
    c = SC.onehot_case(h)
    x, w, which = SC.onehot_operands(h)
    assert bool((x.half().float() == x).all()) and float(x.max()) < 2048
    assert x.flatten().unique().numel() == x.numel()
    dense = SC.packed_k_order(w, c)
    hits = (dense != 0).sum(0).view(c.k_tap // c.kb, c.ntaps, c.kb)
    for cb in range(c.k_tap // c.kb):
        for ch in range(c.kb):
            assert hits[cb, :, ch].tolist() == [1 if cb * c.kb + ch < c.cin else 0] * c.ntaps
    assert bool(((dense != 0).sum(1) == 1).all())
    p = SC.pack_ref(c, w, None)
    assert bool((p.p0 < p.p1).all())
    y = F.conv2d(x.double(), w.double(), None, 1, (c.k - 1) // 2)
    mid = c.H // 2
    for f, (chan, tap, sign) in enumerate(which):
        if c.H == 3:
            assert float(y[0, f, mid, mid]) == sign * (9 * chan + tap + 1)
        elif c.k == 1 or tap == 4:
            assert float(y[0, f, 0, 0]) == sign * (chan + 1)
        else:
            assert float(y[0, f, 0, 0]) == 0.0
