"""Every forward kernel instance of the default training precision's two operand forms -- the split-operand form
(mcamd_conv_geom.x_wrap: igemm_kernel, igemm_pp_kernel, small3x3_split_kernel) and the fp8-correction form
(mcamd_conv_geom.x_f8: igemm_pp_kernel<.., F8 = true>) -- against an EXACT reference.

tests/split_cases.py holds the cases, their operands (small integers, integer-valued e4m3 codes, weights a + b 2^-11), the
float64 reference and the conditions under which the kernel output must EQUAL it; test_split_cases_cpu.py proves without a
GPU that the cases reach every instance the route rules can name and every boundary condition, and that every reference
meets the conditions.  Channels outside the activation slice hold NaN; the output, the whole statistics slab and the NCHW
tensor start as NaN, so a third part that does not wrap, an unwritten element, a store outside the slice and a slab row
nobody wrote all show.  There is no tolerance in this file except the derived fp32-summation bound on the statistics of the
fp8-correction form (split_cases.stats_bounds: its outputs are multiples of 2^-12, whose squares fp32 cannot sum exactly).

The accuracy of both forms against the unrounded product is what the four Gaussian tests of test_kernels_gpu.py check
(test_split_forward_two_planes_equals_three, test_f8_correction_forward, test_small3x3_split_kernel,
test_split_conv2_at_channel_offset); bn_conv1x1.hip has its own bit-equality tests
(test_bn_conv1x1_gpu.py) and its own exact per-instance tests (test_bn1x1_instances_gpu.py)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops, _lib as L  # noqa: E402
import split_cases as SC  # noqa: E402
from util import NAN, fill_padded  # noqa: E402

pytestmark = pytest.mark.gpu


def _check_route(c, setenv):
    """The query must still name the instance and the boundary conditions the case was written for."""
    SC.apply_env(c, setenv)
    r = SC.route_of(c)
    assert (r.kernel, r.bm, r.bn, r.bk) == c.expect, (c.name, r)
    assert set(c.tags) <= SC.boundary_tags(c, r), (c.name, r, SC.boundary_tags(c, r))
    if c.epi == "raw32":
        assert ops.stats_rows(SC.geom_of(c), L.EPI_RAW_F32) == r.rows, c.name
    return r


def _pack_job(w, c, wp, split, wexp=0):
    return dict(w=w, mask=None, rows=None, cols=None, cout=c.n, cin=c.P, ksize=c.k, dst_fwd=wp, dst_dgrad=None, split=split, f8_wexp=wexp)


def _activations(dev, c, o):
    """[x_hi | x_lo] (wrap) or [x_hi | lo8 | x8 bytes] (f8) in a NaN-fenced buffer of the case's ld and form"""
    P, ld = c.P, c.ld or 2 * c.P
    if c.form == "wrap":
        return fill_padded(dev, c, torch.cat([o.x_hi, o.x_lo], 1), ld, c.choff, 2 * P, c.pad)
    buf = fill_padded(dev, c, o.x_hi, ld, 0, 2 * P, c.pad)
    inner = ops.padded_view(buf.view(torch.uint8), c.B, c.H, c.W, 2 * ld, pad=c.pad)[:, 1:-1, 1:-1]
    inner[..., 2 * P:3 * P] = SC.e4m3_codes(o.lo8).permute(0, 2, 3, 1).to(dev)
    inner[..., 3 * P:4 * P] = SC.e4m3_codes(o.x8).permute(0, 2, 3, 1).to(dev)
    return buf


def _weights(dev, c, o, wexp):
    if c.form == "wrap":      # plain packing of the 3 P channel filter (test_split_packing_is_plain_packing_of_concatenation)
        return ops.pack_weights(SC.plain_geom_of(c), o.w.to(dev).contiguous(), None, want_fwd=True, want_dgrad=False)[0]
    wp = torch.zeros(ops.packed_elems(SC.geom_of(c, wexp))[0], dtype=torch.float16, device=dev)
    w = o.w.to(dev).contiguous()
    ops.pack_many(*ops.pack_table([_pack_job(w, c, wp, 2, wexp)], dev))
    return wp


def _launch(dev, c, r, g, xb, wp, bias=None):
    """One launch into NaN-filled outputs -> (y [B][n][H][W] cpu, everything outside the slice, slab cpu or None)"""
    n, M = c.n, c.M
    if c.epi == "nchw":
        y = torch.full((c.B, n, c.H, c.W), NAN, device=dev)
        ops.conv_fwd_nchw(g, xb, wp, y, bias.to(dev) if bias is not None else None)
        torch.cuda.synchronize()
        return y.cpu(), torch.empty(0), None
    y_ld = c.y_ld or n
    y = torch.full((M * y_ld,), NAN, device=dev)
    stats = torch.full((r.rows, 2, ops.round_up(n, 256)), NAN, device=dev)
    ops.conv_fwd_raw32(g, xb, wp, y, y_ld, c.y_choff, stats)
    torch.cuda.synchronize()
    v = y.view(c.B, c.H, c.W, y_ld)
    rest = torch.cat([v[..., :c.y_choff].reshape(-1), v[..., c.y_choff + n:].reshape(-1)])
    return v[..., c.y_choff:c.y_choff + n].permute(0, 3, 1, 2).cpu(), rest.cpu(), stats.cpu()


def _assert_equal(c, r, what, got, want):
    if SC.count_unequal(got, want) == 0:
        return
    got = got.double()
    bad = ~(got == want)
    idx = bad.nonzero()
    unit = SC.UNIT_F8 if c.form == "f8" else 1.0
    diff = ((got - want) / unit)[bad]
    diff = diff[~torch.isnan(diff)]
    mt = sorted(set((((idx[:, 0] * c.H + idx[:, 2]) * c.W + idx[:, 3]) // r.bm).tolist()))
    nt = sorted(set((idx[:, 1] // r.bn).tolist()))
    raise AssertionError("%s (%s): %d of %d elements of %s differ from the exact result; first (image, channel, y, x) %s, got %r want %r; "
                         "difference in units of %g: min %r max %r (%d NaN); M tiles of %d rows touched %s, N tiles of %d columns %s"
                         % (c.name, SC.KERNEL_NAMES[r.kernel], int(bad.sum()), got.numel(), what, idx[0].tolist(), float(got[bad][0]),
                            float(want[bad][0]), unit, float(diff.min()) if diff.numel() else NAN, float(diff.max()) if diff.numel() else NAN,
                            int(bad.sum()) - diff.numel(), r.bm, mt[:16], r.bn, nt[:16]))


def _check_slab(c, r, stats, ref, what):
    n, own = c.n, SC.owned_columns(c, r)
    assert not bool(torch.isnan(stats[:, :, :n]).any()), "%s %s: slab rows with NaN: %s" % (
        c.name, what, torch.isnan(stats[:, :, :n]).any(2).any(1).nonzero().flatten().tolist()[:16])
    # columns of the last column tile beyond the filters: zero filters, so zero sums; further columns belong to nobody
    assert bool((stats[:, :, n:own] == 0).all()), "%s %s: slab columns [%d, %d) must hold the zero sums of the pad filters" % (c.name, what, n, own)
    assert bool(torch.isnan(stats[:, :, own:]).all()), "%s %s: slab columns >= %d were written" % (c.name, what, own)
    s = stats.double().sum(0)[:, :n]
    if SC.stats_violations(c, s[0], s[1], ref):
        b1, b2 = SC.stats_bounds(c, ref) if c.form == "f8" else (torch.zeros(n, dtype=torch.float64),) * 2
        e1, e2 = (s[0] - ref.s1).abs(), (s[1] - ref.s2).abs()
        k1, k2 = int((e1 - b1).argmax()), int((e2 - b2).argmax())
        raise AssertionError("%s %s: statistics miss; sum y: channel %d got %r want %r (allowed %r); sum y^2: channel %d got %r want %r (allowed %r)"
                             % (c.name, what, k1, float(s[0][k1]), float(ref.s1[k1]), float(b1[k1]), k2, float(s[1][k2]), float(ref.s2[k2]),
                                float(b2[k2])))


@pytest.mark.parametrize("c", SC.SPLIT_CASES, ids=str)
def test_split_instance_exact(dev, c, setenv):
    """One launch per case (per weight exponent for the fp8-correction form: the results must equal the reference, hence
    each other) into NaN-filled outputs."""
    r = _check_route(c, setenv)
    o = SC.operands(c)
    ref = SC.reference(c, o)
    assert SC.exactness(c, o, ref) == [], c.name           # the conditions of exactness, on this case's own reference
    xb = _activations(dev, c, o)
    for wexp in c.wexps:
        what = "y" if wexp is None else "y (x_f8_wexp %d)" % wexp
        g = SC.geom_of(c, wexp or 0)
        if c.form == "f8":
            assert ops.conv_fwd_f8_ok(g), c.name
        got, rest, stats = _launch(dev, c, r, g, xb, _weights(dev, c, o, wexp), o.bias)
        _assert_equal(c, r, what, got, ref.y)
        assert bool(torch.isnan(rest).all()), "%s: %d elements of %s outside the slice were written" % (c.name, int((~torch.isnan(rest)).sum()), what)
        if stats is not None:
            _check_slab(c, r, stats, ref, what)


# ---- Gaussian operands: sums that DO depend on the order
def _gaussian(c):
    gen = SC._gen(c)
    x = torch.randn(c.B, c.P, c.H, c.W, generator=gen)
    w = torch.randn(c.n, c.P, c.k, c.k, generator=gen) * (2.0 / (c.P * c.k * c.k)) ** 0.5
    bias = torch.randn(c.n, generator=gen) if c.epi == "nchw" else None
    return x, w, bias


def _split_weights(dev, c, w):
    wp = torch.zeros(ops.packed_elems(SC.plain_geom_of(c))[0], dtype=torch.float16, device=dev)
    wd = w.to(dev).contiguous()
    ops.pack_many(*ops.pack_table([_pack_job(wd, c, wp, True)], dev))
    return wp


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_bit_equal(c, a, b, what):
    (ya, _, sa), (yb, _, sb) = a, b
    assert not bool(torch.isnan(ya).any()), (c.name, what)
    assert torch.equal(_bits(ya), _bits(yb)), "%s: %s: %d outputs differ" % (c.name, what, int((_bits(ya) != _bits(yb)).sum()))
    if sa is not None and sb is not None:
        assert sa.shape == sb.shape and not bool(torch.isnan(sa[:, :, :c.n]).any()), (c.name, what)
        assert torch.equal(_bits(sa[:, :, :c.n]), _bits(sb[:, :, :c.n])), "%s: %s: the statistics slabs differ" % (c.name, what)


@pytest.mark.parametrize("c", SC.one_case_per_instance("wrap", (SC.IGEMM, SC.PP)), ids=str)
def test_two_planes_equal_three_planes(dev, c, setenv):
    """Every igemm_kernel / igemm_pp_kernel instance of the split-operand form: the launch on two planes [x_hi | x_lo] with
    x_wrap is bit-equal, output and slab, to the launch on three planes [x_hi | x_lo | x_hi] without it (same K order, same
    operands).  small3x3_split_kernel has no three-plane launch: that geometry goes to igemm_kernel."""
    r = _check_route(c, setenv)
    x, w, bias = _gaussian(c)
    hi = x.half().float()
    lo = (x - hi).half().float()
    wp = _split_weights(dev, c, w)
    two = _launch(dev, c, r, SC.geom_of(c), fill_padded(dev, c, torch.cat([hi, lo], 1), c.ld or 2 * c.P, c.choff, 2 * c.P, c.pad), wp, bias)
    ld3 = (c.ld or 2 * c.P) + c.P
    g3 = ops.geom(c.B, c.H, c.W, c.k, 3 * c.P, c.n, ld3, c.choff, pad=c.pad)
    mode, stats = SC.FORMS[c.key]
    r3 = ops.conv_route_info(g3, ops.DIR_FWD, mode, L.DST_PLAIN, stats)
    assert r3 == r, (c.name, r, r3)
    three = _launch(dev, c, r3, g3, fill_padded(dev, c, torch.cat([hi, lo, hi], 1), ld3, c.choff, 3 * c.P, c.pad), wp, bias)
    _assert_bit_equal(c, two, three, "two planes with x_wrap against three planes")


@pytest.mark.parametrize("c", SC.one_case_per_instance("wrap", (SC.PP,)), ids=str)
def test_pingpong_equals_igemm_on_split_operands(dev, c, setenv):
    """Every ping-pong tile of the split-operand form is bit-equal to igemm_kernel (MCAMD_PP=0) on the same operands: "the
    accumulation order over K equals igemm_kernel's" (conv_igemm_pp.hip).  Outputs only: the slabs have other rows."""
    r = _check_route(c, setenv)
    x, w, bias = _gaussian(c)
    hi = x.half().float()
    lo = (x - hi).half().float()
    wp = _split_weights(dev, c, w)
    xb = fill_padded(dev, c, torch.cat([hi, lo], 1), c.ld or 2 * c.P, c.choff, 2 * c.P, c.pad)
    pp = _launch(dev, c, r, SC.geom_of(c), xb, wp, bias)
    setenv("MCAMD_PP", "0")
    r0 = SC.route_of(c)
    assert r0.kernel == SC.IGEMM, (c.name, r0)
    ig = _launch(dev, c, r0, SC.geom_of(c), xb, wp, bias)
    _assert_bit_equal(c, (pp[0], None, None), (ig[0], None, None), "igemm_pp_kernel against igemm_kernel")


@pytest.mark.parametrize("c", SC.one_case_per_instance("f8", (SC.PP,)), ids=str)
def test_f8_is_deterministic(dev, c, setenv):
    """Two launches of every F8 tile on Gaussian operands (the production packer's bytes; byte planes e4m3(x_lo 2^12) and
    e4m3(2 x) made here with torch) into fresh buffers: output and slab bit-equal."""
    r = _check_route(c, setenv)
    x, w, _ = _gaussian(c)
    hi = x.half().float()
    q = lambda v: v.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()
    o = SC.Operands(hi, None, q((x - hi) * 2.0 ** 12), q(x * 2.0), w, None, None, None)
    g = SC.geom_of(c, ops.F8_WEXP_DEFAULT)
    wp = _weights(dev, c, o, ops.F8_WEXP_DEFAULT)
    a = _launch(dev, c, r, g, _activations(dev, c, o), wp)
    b = _launch(dev, c, r, g, _activations(dev, c, o), wp)
    _assert_bit_equal(c, a, b, "two launches")


# ---- the packers
@pytest.mark.parametrize("k,P,n", [(3, 32, 64), (1, 96, 125), (3, 64, 40), (1, 128, 264)])
def test_split_packing_is_plain_packing_of_concatenation(dev, k, P, n):
    """The licence for the wrap cases' weights: pack_many(split=True) of w is bit for bit the plain forward packing of
    cat([w_hi, w_hi, w_lo], 1) in the 3 P channel geometry -- so any three parts [W0 | W1 | W2] packed plainly are a packing
    the split-operand kernels may be given."""
    gen = torch.Generator().manual_seed(k * 1000 + P + n)
    w = (torch.randn(n, P, k, k, generator=gen) * 0.1).to(dev).contiguous()
    hi = w.half().float()
    g3 = ops.geom(2, 8, 8, k, 3 * P, n, 3 * P)
    want, _ = ops.pack_weights(g3, torch.cat([hi, hi, w - hi], 1).contiguous(), None, True, False)
    got = torch.zeros_like(want)
    ops.pack_many(*ops.pack_table([dict(w=w, mask=None, rows=None, cols=None, cout=n, cin=P, ksize=k, dst_fwd=got, dst_dgrad=None, split=True)], dev))
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("name", ("f8-pp256x256-3x3", "f8-pp256x128", "f8-pp192x128-onehot-w8", "f8-pp192x128-onehot-wlo8"))
def test_f8_packing_layout(dev, name):
    """pack_many(split = 2), read through the layout include/mcamd.h states (split_cases.f8_packing), has exactly the fp16
    values and e4m3 bytes of the reference in every tap and channel block, at every exponent; pad rows stay zero."""
    c = next(c for c in SC.SPLIT_CASES if c.name == name)
    o = SC.operands(c)
    for wexp in c.wexps:
        got = _weights(dev, c, o, wexp).view(torch.int16).view(ops.round_up(c.n, 256), -1).cpu()
        want = SC.f8_packing(o.a, o.b, wexp)
        bad = (got != want).nonzero()
        assert bad.numel() == 0, "%s, exponent %d: %d fp16 units differ; first (filter, K position) %s: got 0x%04x want 0x%04x" % (
            name, wexp, bad.shape[0], bad[0].tolist(), int(got[tuple(bad[0])]) & 0xFFFF, int(want[tuple(bad[0])]) & 0xFFFF)


def test_split_refusals(dev):
    """The launch-side refusals that need a device pointer: a non-fp32 epilogue for either form, and an fp8-correction shape
    without a ping-pong tile.  (x_f8 with x_choff != 0 and x_wrap together with x_f8 are refused by the geometry check:
    test_split_cases_cpu.py.)"""
    B, H, W, P, n = 1, 16, 16, 128, 128
    xb = ops.alloc_padded(B, H, W, 2 * P, dev)
    wp = torch.zeros(256 * 3 * P, dtype=torch.float16, device=dev)
    y16 = torch.zeros(B * H * W * n, dtype=torch.float16, device=dev)
    y32 = torch.zeros(B * H * W * n, device=dev)
    gw = ops.geom(B, H, W, 1, 3 * P, n, 2 * P, x_wrap=2 * P)
    g8 = ops.geom(B, H, W, 1, 2 * P, n, 2 * P, x_f8=P, x_f8_wexp=0)
    for g in (gw, g8):
        with pytest.raises(L.McamdError):
            ops.conv_fwd_raw(g, xb, wp, y16, n, 0, None)
        with pytest.raises(L.McamdError):
            ops.conv_fwd_padded(g, xb, wp, ops.alloc_padded(B, H, W, n, dev), n)
    with pytest.raises(L.McamdError):
        ops.conv_fwd_nchw(g8, xb, wp, y32.view(B, n, H, W))
    small = ops.geom(B, 8, 8, 1, 2 * P, n, 2 * P, x_f8=P, x_f8_wexp=0)          # M = 64: no ping-pong tile
    assert not ops.conv_fwd_f8_ok(small)
    with pytest.raises(L.McamdError):
        ops.conv_fwd_raw32(small, xb, wp, y32, n, 0, None)
    torch.cuda.synchronize()
