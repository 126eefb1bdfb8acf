"""What tests/test_split_instances_gpu.py runs, proven on the CPU: the case table of tests/split_cases.py reaches every
kernel instance the route rules can name for the split-operand (x_wrap) and fp8-correction (x_f8) forward forms and every
named boundary condition; every case's reference meets the conditions under which EQUAL is the right comparison; and that
comparison rejects references that are wrong in the ways such kernels go wrong.  No GPU: the route answers come from
mcamd_conv_route_info, the launches' own route function."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops, _lib as L  # noqa: E402
import split_cases as SC  # noqa: E402

I, PP, S7 = SC.IGEMM, SC.PP, SC.SPLIT
IGEMM_TILES = {(I, 128, 32, 32), (I, 128, 32, 64), (I, 128, 64, 32), (I, 128, 64, 64), (I, 128, 128, 32), (I, 128, 128, 64), (I, 192, 128, 64)}
PP_TILES = {(PP, 256, 256, 32), (PP, 192, 256, 32), (PP, 256, 128, 32), (PP, 192, 128, 32)}


def test_reachable_instances_are_the_expected_sets(setenv):
    """A changed route rule fails here: the sets are literals."""
    reach = SC.reachable_cached(setenv)
    assert reach["wrap-raw32"] == IGEMM_TILES | PP_TILES | {(S7, 32, 64, 96)}
    assert reach["wrap-nchw"] == IGEMM_TILES | PP_TILES
    assert reach["f8-raw32"] == PP_TILES                       # what mcamd_conv_fwd_f8_ok accepts: the four F8 instances
    assert reach["f8-nchw"] == IGEMM_TILES | PP_TILES          # answered by the route function, refused by the launch


def test_cases_reach_every_instance_and_boundary(setenv):
    reach = SC.reachable_cached(setenv)
    inst, tags_of, nchw_tags = set(), {key: set() for key in SC.BOUNDARIES}, {I: set(), PP: set()}
    for c in SC.SPLIT_CASES:
        SC.apply_env(c, setenv)
        r = SC.route_of(c)
        assert (r.kernel, r.bm, r.bn, r.bk) == c.expect, (c.name, r)
        t = SC.boundary_tags(c, r)
        assert set(c.tags) <= t, (c.name, set(c.tags) - t)
        inst.add(SC.instance_of(c, r))
        if c.epi == "raw32":
            tags_of[(c.form, r.kernel)] |= t
            assert ops.stats_rows(SC.geom_of(c), L.EPI_RAW_F32) == r.rows and ops.tile_info(SC.geom_of(c)) == (r.bm, r.bn, r.bk, r.kernel), c.name
        else:
            nchw_tags[r.kernel] |= t
        if c.form == "f8":
            for e in c.wexps:
                assert ops.conv_fwd_f8_ok(SC.geom_of(c, e)), (c.name, e)
            assert len(c.wexps) >= 3 and min(c.wexps) < 0, c.name
    assert len({c.name for c in SC.SPLIT_CASES}) == len(SC.SPLIT_CASES)
    for key in SC.CASE_FORMS:
        want = {(key, i) for i in reach[key]}
        assert {i for i in inst if i[0] == key} == want, (key, want ^ {i for i in inst if i[0] == key})
    for key, need in SC.BOUNDARIES.items():
        assert tags_of[key] >= set(need), (key, set(need) - tags_of[key])
    for kernel in (I, PP):
        assert nchw_tags[kernel] >= set(SC.BOUNDARIES_NCHW), kernel
    # the one-hot cases: both byte halves, in every F8 tile
    assert {(c.expect, c.special) for c in SC.SPLIT_CASES if c.special} == {(t, s) for t in PP_TILES for s in SC.WEXPS_ONEHOT}
    # the Gaussian bit-equality tests cover every instance that has the property
    assert {c.expect for c in SC.one_case_per_instance("wrap", (I, PP)) if c.epi == "raw32"} == IGEMM_TILES | PP_TILES
    assert {c.expect for c in SC.one_case_per_instance("wrap", (I, PP)) if c.epi == "nchw"} == IGEMM_TILES | PP_TILES
    assert {c.expect for c in SC.one_case_per_instance("f8", (PP,))} == PP_TILES


def test_no_case_is_left_out_of_the_gpu_run():
    """Every table case is a parameter of test_split_instance_exact, with no skip or xfail mark in the file."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_split_instances_gpu.py")).read()
    assert '@pytest.mark.parametrize("c", SC.SPLIT_CASES, ids=str)\ndef test_split_instance_exact(' in src
    assert "skip" not in src and "xfail" not in src


@pytest.mark.parametrize("c", SC.SPLIT_CASES, ids=str)
def test_case_meets_the_conditions_of_exactness(c):
    o = SC.operands(c)
    ref = SC.reference(c, o)
    assert SC.exactness(c, o, ref) == [], c.name
    if c.form == "wrap":
        W0, W1, W2 = o.w[:, :c.P], o.w[:, c.P:2 * c.P], o.w[:, 2 * c.P:]
        assert not torch.equal(o.x_hi, o.x_lo) and not torch.equal(W0, W2) and torch.equal(W0, W1) == c.tie
    else:
        # the byte planes decode to the intended integers, drawn independently of the hi plane
        for plane in (o.lo8, o.x8):
            assert torch.equal(SC.e4m3_values(SC.e4m3_codes(plane)), plane.double())
            assert c.special or not torch.equal(plane, o.x_hi)
        assert bool(((o.a != 0) | (o.b == 0)).all())                 # no lo part without a hi part
        b1, b2 = SC.stats_bounds(c, ref)
        assert float((b1 / ref.y.abs().sum((0, 2, 3)).clamp(min=1e-300)).max()) < 2e-3          # the derived bound stays a tight one
    if c.special:
        # one non-zero byte per pixel, every position of every fp8 chunk once; 64 distinct codes along k in every filter
        planes = torch.cat([o.lo8, o.x8], 1).permute(0, 2, 3, 1).reshape(c.M, 2 * c.P)
        assert bool(((planes != 0).sum(1) == 1).all()) and sorted(planes.ne(0).nonzero()[:, 1].tolist()) == list(range(256))
        t = (o.a if c.special == "onehot-w8" else o.b).view(c.n, c.P)
        for chunk in (t[:, :64], t[:, 64:]):
            assert all(len(set(row.tolist())) == 64 for row in chunk)


def test_f8_packing_layout_is_the_headers():
    """split_cases.f8_packing against a literal reading of include/mcamd.h for a few entries: w_hi of (filter, tap, channel)
    at fp16 unit kpos(t, c); w8 byte of channel c at byte (c & 1) of unit P + c / 2; wlo8 byte at element P + c."""
    for name, e, samples in (("f8-pp256x256-3x3", 4, ((0, 0, 0), (5, 4, 33), (135, 8, 63), (77, 2, 17))),
                             ("f8-pp256x128", -2, ((0, 0, 0), (135, 0, 127), (9, 0, 64), (77, 0, 63))),
                             ("f8-pp192x128-onehot-wlo8", 1, ((3, 0, 5), (127, 0, 126)))):
        c = next(c for c in SC.SPLIT_CASES if c.name == name)
        o = SC.operands(c)
        P, kk, npad = c.P, c.k * c.k, ops.round_up(c.n, 256)
        rows = SC.f8_packing(o.a, o.b, e)
        assert rows.shape == (npad, kk * 2 * P) and not bool(rows[c.n:].any())
        raw = rows.contiguous().view(torch.uint8).view(npad, kk * 2 * P, 2)
        for f, t, ch in samples:
            ty, tx = divmod(t, c.k)
            a, b = float(o.a[f, ch, ty, tx]), float(o.b[f, ch, ty, tx])
            assert rows[f, SC.kpos(t, ch, kk, 2 * P)].view(torch.float16).item() == a
            for el, v in ((ch, a), (P + ch, b)):
                byte = raw[f, SC.kpos(t, P + el // 2, kk, 2 * P), el & 1]
                assert float(SC.e4m3_values(byte.reshape(1))) == v * 2.0 ** e, (name, f, t, ch, el)


def test_geometry_refusals(setenv):
    """The refusals that are host logic (the geometry check every entry starts with): x_f8 with x_choff != 0, x_wrap together
    with x_f8, planes that are no whole channel blocks, an exponent out of range."""
    ok = ops.geom(1, 16, 16, 1, 256, 128, 256, x_f8=128, x_f8_wexp=0)
    ops.conv_route_info(ok, ops.DIR_FWD, L.EPI_RAW_F32, L.DST_PLAIN, True)
    for bad in (ops.geom(1, 16, 16, 1, 256, 128, 320, 64, x_f8=128, x_f8_wexp=0),             # slice not at channel 0
                ops.geom(1, 16, 16, 1, 256, 128, 256, x_wrap=256, x_f8=128, x_f8_wexp=0),     # both forms at once
                ops.geom(1, 16, 16, 1, 192, 128, 192, x_f8=96, x_f8_wexp=0),                  # P % 64 != 0
                ops.geom(1, 16, 16, 1, 384, 128, 256, x_f8=128, x_f8_wexp=0),                 # cin != 2 P
                ops.geom(1, 16, 16, 1, 256, 128, 256, x_f8=128, x_f8_wexp=41),                # exponent outside [-24, 40]
                ops.geom(1, 16, 16, 1, 256, 128, 256, x_f8=128, x_f8_wexp=-25),
                ops.geom(1, 16, 16, 1, 96, 128, 64, x_wrap=48),                               # x_wrap % 64 != 0
                ops.geom(1, 16, 16, 1, 128, 128, 64, x_wrap=64),                              # cin != 3 P
                ops.geom(1, 16, 16, 1, 96, 128, 56, x_wrap=64)):                              # the slice does not hold x_wrap channels
        with pytest.raises(L.McamdError):
            ops.conv_route_info(bad, ops.DIR_FWD, L.EPI_RAW_F32, L.DST_PLAIN, True)
        assert not ops.conv_fwd_f8_ok(bad)


# ---------------------------------------------------------------------------------------------------------------------
# the tests' own sanity: the GPU test's comparison (split_cases.count_unequal) rejects wrong references
# ---------------------------------------------------------------------------------------------------------------------
def _conv(c, x, w):
    return F.conv2d(x.double(), w.double(), None, 1, (c.k - 1) // 2)


def _swap_taps(w):
    """tap (0, 0) reads the pixel of tap (0, 1) and the other way round: one pixel off"""
    v = w.clone()
    v[:, :, 0, 0], v[:, :, 0, 1] = w[:, :, 0, 1], w[:, :, 0, 0]
    return v


@pytest.mark.parametrize("name", ("w-i128x32k64-raw32", "w-pp192x128-raw32", "w-small-split-n40", "w-i128x64k64-nchw"))
def test_comparison_rejects_wrong_wrap_references(name):
    c = next(c for c in SC.SPLIT_CASES if c.name == name)
    o = SC.operands(c)
    ref = SC.reference(c, o)
    P = c.P
    W0, W1, W2 = o.w[:, :P], o.w[:, P:2 * P], o.w[:, 2 * P:]
    bias = o.bias.double().view(1, -1, 1, 1) if o.bias is not None else 0.0
    full = lambda w0, w1, w2, third=o.x_hi: _conv(c, o.x_hi, w0) + _conv(c, o.x_lo, w1) + _conv(c, third, w2) + bias
    assert SC.count_unequal(full(W0, W1, W2), ref.y) == 0
    wrong = {"no wrap: the third part reads the lo plane": full(W0, W1, W2, o.x_lo),
             "a tap one pixel off": full(W0, W1, _swap_taps(W2)),
             "planes swapped": _conv(c, o.x_lo, W0) + _conv(c, o.x_hi, W1) + _conv(c, o.x_lo, W2) + bias}
    last = W2.clone()                                   # the last K chunk: last channel block, last tap, its last 32 channels
    last[:min(c.n, c.expect[2]), P - 32:, c.k - 1, c.k - 1] = 0
    wrong["the last K chunk of the first column tile dropped"] = full(W0, W1, last)
    for what, y in wrong.items():
        assert SC.count_unequal(y, ref.y) > 0, (name, what)
        if ref.s1 is not None:
            assert SC.stats_violations(c, y.sum((0, 2, 3)), (y * y).sum((0, 2, 3)), ref) > 0, (name, what)
    one = ref.y.clone()                                 # one element off by one unit; one element never written
    one[-1, -1, -1, -1] += 1.0
    assert SC.count_unequal(one, ref.y) == 1
    one[-1, -1, -1, -1] = float("nan")
    assert SC.count_unequal(one, ref.y) == 1


@pytest.mark.parametrize("name", ("f8-pp256x256-3x3", "f8-pp192x128-8-columns-of-tiles", "f8-pp256x128-onehot-w8", "f8-pp256x128-onehot-wlo8"))
def test_comparison_rejects_wrong_f8_references(name):
    c = next(c for c in SC.SPLIT_CASES if c.name == name)
    o = SC.operands(c)
    ref = SC.reference(c, o)
    U = SC.UNIT_F8
    full = lambda lo8, x8, a=o.a, b=o.b, unit=U: _conv(c, o.x_hi, a) + unit * (_conv(c, lo8, a) + _conv(c, x8, b))
    assert SC.count_unequal(full(o.lo8, o.x8), ref.y) == 0
    last = o.b.clone()                                  # the last fp8 chunk: the last 64 x8 bytes of the last tap
    last[:min(c.n, c.expect[2]), c.P - 64:, c.k - 1, c.k - 1] = 0
    first = o.a.clone()                                 # the first fp8 chunk: the first 64 lo8 bytes of the first tap
    first[:min(c.n, c.expect[2]), :64, 0, 0] = 0
    wrong = {"lo8 and x8 swapped": full(o.x8, o.lo8),
             "2^-(11 + e) instead of 2^-(12 + e)": full(o.lo8, o.x8, unit=2 * U),
             "the first fp8 chunk of the first column tile dropped": _conv(c, o.x_hi, o.a) + U * (_conv(c, o.lo8, first) + _conv(c, o.x8, o.b)),
             "a byte pair swapped": full(o.lo8[:, [1, 0] + list(range(2, c.P))], o.x8[:, [1, 0] + list(range(2, c.P))])}
    if c.special != "onehot-w8":                        # (those filters have no lo parts)
        wrong["the last K chunk of the first column tile dropped"] = full(o.lo8, o.x8, b=last)
    if c.k == 3:
        wrong["a tap one pixel off"] = _conv(c, o.x_hi, o.a) + U * (_conv(c, o.lo8, _swap_taps(o.a)) + _conv(c, o.x8, o.b))
    for what, y in wrong.items():
        assert SC.count_unequal(y, ref.y) > 0, (name, what)
    # a slab off by one unit of the last place of a channel's sum is outside the derived bound only if the bound is tight:
    # it is wide enough for fp32 summation in any order, and far too narrow for a missing pixel
    y = ref.y.clone()
    y[0, :, 0, 0] = 0.0
    if c.M < 1000 and bool((ref.y[0, :, 0, 0].abs() >= 1.0).any()):          # (gamma_n sum |y| < 1 at this size)
        assert SC.stats_violations(c, y.sum((0, 2, 3)), (y * y).sum((0, 2, 3)), ref) > 0
    assert SC.stats_violations(c, ref.s1.float(), ref.s2.float(), ref) == 0
