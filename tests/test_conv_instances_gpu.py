"""Every kernel instance mcamd_conv_fwd and mcamd_conv_dgrad can launch, against an EXACT reference.

The operands hold small integers, which fp16 represents exactly.  Every product is an integer, and while
max|x| * max|w| * (taps * padded channels) < 2^24 every partial sum, in every summation order, is an integer that fp32
represents exactly: MFMA accumulation over K in any chunking, the bias, the BatchNorm partial sums (while the sum of y^2
over all pixels of a channel stays below 2^24) and the inference epilogue (power-of-two scale and slope, shifts that are
multiples of 1/4) are all exact.  The reference is the same convolution in float64 on the CPU (float32, exact under the same
bound, for the one big case) and the result must EQUAL it: a kernel that gets the last row of a ragged M tile wrong, reads
a tap one pixel off at an image border, drops the last K chunk of one column tile or counts a halo pixel twice is off by
at least one integer unit.  There is no tolerance in this file.

tests/conv_cases.py holds the cases, their operands, the reference and the conditions of exactness; test_host_cpu.py proves
(without a GPU) that the cases reach every (kernel, tile, epilogue) instance the route rules can name, every boundary
condition, and that every reference meets the conditions.  Channels outside the operand slice hold NaN, the slice beyond
the real channels and the halo hold zero; every output starts as NaN everywhere (padded destinations: halo and guard
bands included) and the statistics slab starts as NaN, so a leak from a neighbour's channels, an unwritten element, a
store outside the slice and a slab row nobody wrote all show.

The split-operand and fp8-correction operand forms (x_wrap, x_f8, small3x3_split_kernel) have the same kind of test in
test_split_instances_gpu.py (cases: split_cases.py, proven on the CPU by test_split_cases_cpu.py).  Out of scope: the dgrad
instances that take BatchNorm sums (test_dgrad_bn_sums_gpu.py); the split-K, sparse and q8 kernels, each of which has its
own exact tests (the 2:4 fp16 forward: test_sparse_instances_gpu.py); the MCAMD_PP_MFMA=32 instances, which are off by default and selected by a switch the library reads once
per process."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops, _lib as L  # noqa: E402
import conv_cases as CC  # noqa: E402
from util import NAN, whole as _whole, fill_padded as _fill, padded_split as _padded_to_nchw  # noqa: E402

pytestmark = pytest.mark.gpu


def _rows_to_nchw(y, c, ld, choff, n):
    """[M][ld] row-major output -> the slice as [B][n][H][W] and everything else as a flat vector"""
    v = y.view(c.B, c.H, c.W, ld)
    rest = torch.cat([v[..., :choff].reshape(-1), v[..., choff + n:].reshape(-1)])
    return v[..., choff:choff + n].permute(0, 3, 1, 2).cpu(), rest.cpu()


def _launch(dev, c, r, o):
    """One launch of the case into NaN-filled outputs.  Returns {name: (got NCHW, everything outside the slice)}, the
    statistics slab (or None) and the overflow flag (or None)."""
    g = CC.geom_of(c)
    act_ld = 4 if c.stem else (c.ld or c.k_tap)
    ab = _fill(dev, c, o.act, act_ld, c.choff, 4 if c.stem else c.k_tap, c.pad)
    wdev = o.w.to(dev).contiguous()
    mdev = o.mask.to(dev).contiguous() if o.mask is not None else None
    wp, wd = ops.pack_weights(g, wdev, mdev, want_fwd=c.fwd, want_dgrad=not c.fwd)
    n, M = c.n, c.M
    y_ld = c.y_ld or n
    out, stats, flag = {}, None, None
    if c.epi in ("fwd-raw16-stats", "fwd-raw32-stats", "fwd-raw16"):
        f32 = c.epi == "fwd-raw32-stats"
        y = torch.full((M * y_ld,), NAN, dtype=torch.float32 if f32 else torch.float16, device=dev)
        if c.epi != "fwd-raw16":
            stats = torch.full((r.rows, 2, ops.round_up(n, 256)), NAN, dtype=torch.float32, device=dev)
        (ops.conv_fwd_raw32 if f32 else ops.conv_fwd_raw)(g, ab, wp, y, y_ld, c.y_choff, stats)
        out["y"] = _rows_to_nchw(y, c, y_ld, c.y_choff, n)
    elif c.epi == "fwd-nchw":
        y = torch.full((c.B, n, c.H, c.W), NAN, device=dev)
        ops.conv_fwd_nchw(g, ab, wp, y, o.bias.to(dev))
        out["y"] = (y.cpu(), torch.empty(0))
    elif c.epi == "fwd-pad":
        Ho, Wo = (c.H, c.W) if c.dst == "plain" else (c.H // 2, c.W // 2)
        cdst = 4 * n if c.dst == "reorg" else n
        y_ld = c.y_ld or cdst
        y = ops.alloc_padded(c.B, Ho, Wo, y_ld, dev)
        _whole(y).fill_(NAN)
        y2, y2_ld, y2_choff = None, 0, 0
        if c.dst == "pool+y2":
            y2_ld, y2_choff = ops.round_up(n + 40, 32), 32
            y2 = ops.alloc_padded(c.B, c.H, c.W, y2_ld, dev)
            _whole(y2).fill_(NAN)
        ops.conv_fwd_padded(g, ab, wp, y, y_ld, c.y_choff, o.scale.to(dev), o.shift.to(dev), CC.SLOPE, dst_mode=CC.DSTS[c.dst],
                            y2=y2, y2_ld=y2_ld, y2_choff=y2_choff)
        out["y"] = _padded_to_nchw(y, c.B, Ho, Wo, y_ld, c.y_choff, cdst)
        if y2 is not None:
            out["y2"] = _padded_to_nchw(y2, c.B, c.H, c.W, y2_ld, y2_choff, n)
    elif c.epi == "dgrad-raw16":
        y = torch.full((M * y_ld,), NAN, dtype=torch.float16, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if c.overflow else None
        ops.conv_dgrad_raw(g, ab, act_ld, c.choff, wd, y, y_ld, c.y_choff, overflow=flag, concurrent=c.concurrent)
        out["y"] = _rows_to_nchw(y, c, y_ld, c.y_choff, n)
    else:
        assert c.epi == "dgrad-nchw" and not c.concurrent
        y = torch.full((c.B, n, c.H, c.W), NAN, device=dev)
        ops.conv_dgrad_nchw(g, ab, act_ld, c.choff, wd, y)
        out["y"] = (y.cpu(), torch.empty(0))
    torch.cuda.synchronize()
    return out, (stats.cpu() if stats is not None else None), (int(flag.item()) if flag is not None else None)


def _check_route(c, setenv):
    """The query must still name the instance and the boundary conditions the case was written for."""
    CC.apply_env(c, setenv)
    r = CC.route_of(c)
    assert (r.kernel, r.bm, r.bn, r.bk) == c.expect, (c.name, r)
    assert set(c.tags) <= CC.boundary_tags(c, r), (c.name, r, CC.boundary_tags(c, r))
    return r


def _assert_equal(c, r, what, got, want):
    """got, want: [B][n][h][w] (want float64).  NaN compares unequal: an unwritten or polluted element is `bad`."""
    got = got.double()
    assert got.shape == want.shape, (c.name, what, got.shape, want.shape)
    bad = ~(got == want)
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    diff = (got - want)[bad]
    diff = diff[~torch.isnan(diff)]
    B, n, h, w = want.shape
    full = (h, w) == (c.H, c.W)
    mt = sorted(set((((idx[:, 0] * h + idx[:, 2]) * w + idx[:, 3]) // r.bm).tolist())) if full else "(pooled order)"
    nt = sorted(set((idx[:, 1] % c.n // r.bn).tolist()))
    raise AssertionError("%s (%s): %d of %d elements of %s differ from the exact result; first (image, channel, y, x) %s, got %r want %r; "
                         "difference in integer units: min %r max %r (%d NaN); M tiles of %d rows touched %s, N tiles of %d columns %s"
                         % (c.name, CC.KERNEL_NAMES[r.kernel], int(bad.sum()), got.numel(), what, idx[0].tolist(), float(got[bad][0]), float(want[bad][0]),
                            float(diff.min()) if diff.numel() else NAN, float(diff.max()) if diff.numel() else NAN,
                            int(bad.sum()) - diff.numel(), r.bm, mt[:16] if full else mt, r.bn, nt[:16]))


@pytest.mark.parametrize("c", CC.CONV_CASES, ids=str)
def test_conv_instance_exact(dev, c, setenv):
    r = _check_route(c, setenv)
    o = CC.operands(c)
    ref = CC.reference(c, o)
    assert CC.exactness(c, o, ref) == [], c.name           # the conditions of exactness, on this case's own reference

    out, stats, flag = _launch(dev, c, r, o)

    for name, want in (("y", ref.y), ("y2", ref.y2)):
        if want is None:
            continue
        got, rest = out[name]
        _assert_equal(c, r, name, got, want)
        assert bool(torch.isnan(rest).all()), "%s: %d elements of %s outside the slice were written" % (
            c.name, int((~torch.isnan(rest)).sum()), name)
    if stats is not None:
        # every per-row partial is an exact integer, so the float64 sum of the slab rows IS the sum over all pixels
        s = stats.double().sum(0)[:, :c.n]
        for which, want in ((0, ref.s1), (1, ref.s2)):
            bad = ~(s[which] == want)
            assert not bool(bad.any()), "%s: statistics %s of %d channels differ; first channel %d got %r want %r; slab rows with NaN: %s" % (
                c.name, ("sum y", "sum y^2")[which], int(bad.sum()), int(bad.nonzero()[0]), float(s[which][bad][0]), float(want[bad][0]),
                torch.isnan(stats[:, which, :c.n]).any(1).nonzero().flatten().tolist()[:16])
    if c.overflow:
        assert flag == 1, "a value was clamped to +-65504: the overflow flag must be set"
        got = out["y"][0]
        for (b, ch, h, x, sign) in o.planted:
            assert float(got[b, ch, h, x]) == sign * 65504.0
        o2 = CC.operands(c, plant=False)
        ref2 = CC.reference(c, o2)
        assert CC.exactness(c, o2, ref2) == []
        out2, _, flag2 = _launch(dev, c, r, o2)
        _assert_equal(c, r, "y (nothing planted)", out2["y"][0], ref2.y)
        assert flag2 == 0, "nothing was clamped: the overflow flag must stay 0"


@pytest.mark.parametrize("name", CC.DETERMINISM_CASES)
def test_conv_is_deterministic(dev, name, setenv):
    """Gaussian operands (sums that DO depend on the order) and two launches into fresh buffers: output and statistics are
    bit-equal (mcamd_conv_epilogue.stats: "fixed order: deterministic").  The ping-pong kernel has this test in
    test_kernels_gpu.py."""
    c = next(c for c in CC.CONV_CASES if c.name == name)
    r = _check_route(c, setenv)
    o = CC.operands(c, gaussian=True)
    a = _launch(dev, c, r, o)
    b = _launch(dev, c, r, o)
    ya, yb = a[0]["y"][0], b[0]["y"][0]
    bits = torch.int16 if ya.dtype == torch.float16 else torch.int32
    assert not bool(torch.isnan(ya).any())
    assert torch.equal(ya.contiguous().view(bits), yb.contiguous().view(bits))
    if a[1] is not None:
        assert not bool(torch.isnan(a[1][:, :, :c.n]).any())
        assert torch.equal(a[1][:, :, :c.n].contiguous().view(torch.int32), b[1][:, :, :c.n].contiguous().view(torch.int32))
