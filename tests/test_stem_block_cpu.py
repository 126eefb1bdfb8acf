"""csrc/conv_stem_block.hip without a device: the float64 reference of the fused first block (stem_block_ref.py) against
float64 autograd of the four torch ops, the float32 restatements against that reference on every input of
test_stem_block_gpu.py -- which yields the GPU tests' tolerances --, what those inputs contain, and the launch plan query
(mcamd_stem_block_plan_info).

Measured yardsticks, in units of EPS32 * scale (printed by test_restatements_give_the_gpu_tolerances): forward 2.14
-> K_FWD = 16; statistics 4.42 -> K_STATS = 32; backward 0.148 -> K_BWD = 1 (stem_block_cases.py).
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from modelcompression_amd import _lib, ops
import stem_block_ref as R
import stem_block_cases as SC

EPS32 = R.EPS32
BWD = ([(SC.make, s + (m,)) for s in SC.SHAPES for m in (False, True)] + [(SC.make_ties, (k,)) for k in ("rows", "cols", "bands")]
       + [(SC.make_multipass, ())])                                   # the inputs the backward pass is run on
ALL = BWD + [(SC.make_stats, (i,)) for i in "abc"]
ids = lambda cases: ["%s%s" % (f.__name__[5:] or "plain", "-".join(str(a) for a in args)) for f, args in cases]
IDS = ids(ALL)


def own_coeffs(fn, args):
    """(case, pre, stats, sc, sh) with the reference's own batch statistics."""
    c, st = fn(*args), SC.stats(fn, *args)
    sc, sh = R.coeffs(st, c.gamma.double(), c.beta.double())
    return c, SC.pre(fn, *args), st, sc, sh


def test_reference_matches_float64_autograd():
    """Forward, statistics and backward of stem_block_ref.py against autograd of F.conv2d, F.batch_norm, F.leaky_relu and
    F.max_pool2d in float64, on one small masked input without a tie.  slope = 1/8 and fp16 values of G make the
    reference's fp16 rounding of g_z exact, so both sides compute the same function."""
    c = SC.make(2, 8, 32, True)
    slope, mo = 0.125, R.f32(0.1)
    w = c.w16.clone().requires_grad_(True)
    gamma, beta = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    rm, rv = c.rm0.double().clone(), c.rv0.double().clone()
    y = F.conv2d(c.x16, w, None, 1, 1)
    out = F.max_pool2d(F.leaky_relu(F.batch_norm(y, rm, rv, gamma, beta, True, mo, R.f32(SC.EPS)), slope), 2, 2)
    (out * c.G.double()).sum().backward()

    p, st = R.pre(c.x16, c.w16), R.stats(c.x16, c.w16, SC.EPS)
    sc, sh = R.coeffs(st, c.gamma.double(), c.beta.double())
    fw = R.forward(p, sc, sh, slope)
    live = [n for n in range(32) if n != 5]                         # (the fully pruned filter ties everywhere, with no effect)
    assert float(fw.gap[:, live].min()) > 0.0                      # no tie: autograd's choice cannot differ
    yd = y.detach()
    assert torch.allclose(st.mean, yd.mean((0, 2, 3)), rtol=0, atol=1e-13)
    assert torch.allclose(st.var, yd.var((0, 2, 3), unbiased=False), rtol=1e-12, atol=1e-14)
    rm1, rv1, _, _ = R.running(st, c.rm0.double(), c.rv0.double(), 0.1)
    assert torch.allclose(rm1, rm, rtol=0, atol=1e-13) and torch.allclose(rv1, rv, rtol=1e-12, atol=1e-14)
    assert float(((fw.m - out.detach()).abs() / fw.scale).max()) < 1e-12
    bw = R.backward(p, c.gamma.double(), st.mean, st.invstd, sc, sh, slope, c.G, st, mask=c.mask.double())
    for name, got, want, scale in (("dW", bw.dw, w.grad * c.mask.double(), bw.scale_dw), ("dgamma", bw.dgamma, gamma.grad, bw.scale_dgamma),
                                   ("dbeta", bw.dbeta, beta.grad, bw.scale_dbeta)):
        live = scale > 0
        err = float(((got - want).abs()[live] / scale[live]).max())
        print("%s: largest |reference - autograd| / scale %.1e" % (name, err))
        assert err < 1e-11 and not got[~live].any() and not want[~live].any()
    assert not bw.dw[5].any() and float(bw.dgamma[5]) == 0.0       # the fully pruned filter


def test_reference_takes_the_first_maximum():
    """Four equal values, and every pair of equal maxima: the gradient goes to the first in (row, column) order."""
    y = torch.zeros(1, 2, 12, 1, dtype=torch.float64)
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    for i, (a, b) in enumerate(pairs):
        for pos in (a, b):
            y[0, pos // 2, 2 * i + pos % 2, 0] = 1.0
    G = torch.ones(1, 1, 1, 6)
    gz = R.routed(y, torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), 0.1, G)
    for i, (a, b) in enumerate(pairs):
        win = gz[0, :, 2 * i:2 * i + 2, 0].reshape(-1).tolist()
        assert win == [1.0 if k == a else 0.0 for k in range(4)], (a, b, win)
    gz = R.routed(torch.zeros(1, 2, 2, 1, dtype=torch.float64), torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64),
                  0.1, torch.ones(1, 1, 1, 1))
    assert gz.reshape(-1).tolist() == [float(torch.tensor(0.1).half()), 0.0, 0.0, 0.0]        # z_win == 0: the slope side


def units_of(got, ref, scale):
    live = scale > 0
    assert torch.equal(got[~live], ref[~live])
    return float(((got - ref).abs()[live] / (EPS32 * scale[live])).max()) if live.any() else 0.0


def test_restatements_give_the_gpu_tolerances():
    """The yardsticks of test_stem_block_gpu.py: the largest |float32 restatement - reference| in units of EPS32 * scale
    over all elements of all its inputs.  Forward: F.conv2d and one fma in float32.  Statistics: S and C accumulated in
    float32 in sequential chains of 128 steps of 32 pixels, chains summed in double (the kernel's documented arithmetic).
    Backward: T and sum g_z accumulated the same way."""
    worst = {"fwd": 0.0, "stats": 0.0, "bwd": 0.0}
    for (fn, args), name in zip(ALL, IDS):
        c, p, st, sc, sh = own_coeffs(fn, args)
        z32 = R.forward_f32(c.x16, c.w16, sc, sh)
        u_f = float(((z32 - (p.y * sc + sh)).abs() / (EPS32 * (p.ay.double() * sc.abs() + sh.abs()).clamp_min(1e-300))).max())
        mean32, var32 = R.stats_f32(c.x16, c.w16, SC.EPS)
        u_s = max(units_of(mean32, st.mean, st.scale_mean), units_of(var32, st.var, st.scale_var))
        u_b = 0.0
        if (fn, args) in BWD:
            fw = R.forward(p, sc, sh, SC.SLOPE)
            G = torch.where(R.excluded(fw, SC.TAU), torch.zeros(()), c.G)
            mask = c.mask.double() if c.mask is not None else None
            a = (p, c.gamma.double(), st.mean, st.invstd, sc, sh, SC.SLOPE, G, st)
            ref, f32 = R.backward(*a, mask=mask), R.backward(*a, mask=mask, f32_sums=True)
            u_b = max(units_of(f32.dw, ref.dw, ref.scale_dw), units_of(f32.dgamma, ref.dgamma, ref.scale_dgamma),
                      units_of(f32.dbeta, ref.dbeta, ref.scale_dbeta))
        print("%-16s forward %.3f  statistics %.3f  backward %.3f units; kappa up to %.3g" % (name, u_f, u_s, u_b, float(st.kappa.max())))
        for k, u in (("fwd", u_f), ("stats", u_s), ("bwd", u_b)):
            worst[k] = max(worst[k], u)
    print("yardsticks: forward %.3f (K_FWD %g), statistics %.3f (K_STATS %g), backward %.3f (K_BWD %g) units of eps32 * scale"
          % (worst["fwd"], SC.K_FWD, worst["stats"], SC.K_STATS, worst["bwd"], SC.K_BWD))
    # each K was derived from its figure (stem_block_cases.py): 4 x, rounded up to a power of two; should a figure move, K has to follow
    for k, (yard, K) in (("fwd", (SC.YARDSTICK_FWD, SC.K_FWD)), ("stats", (SC.YARDSTICK_STATS, SC.K_STATS)), ("bwd", (SC.YARDSTICK_BWD, SC.K_BWD))):
        assert K == 2.0 ** math.ceil(math.log2(4.0 * yard)), (k, yard, K)
        assert 4.0 * worst[k] <= K, (k, worst[k], K)                # (F.conv2d's float32 summation order may differ between hosts)


@pytest.mark.parametrize("fn, args", BWD, ids=ids(BWD))
def test_few_pooled_pixels_are_near_a_discontinuity(fn, args):
    """At most 1e-3 of a case's pooled pixels have z_win, or the gap to the runner-up, inside (0, TAU): the share the
    backward comparison may exclude (G = 0 on both sides).  Here for the reference's own statistics; the GPU test asserts
    it again for the device's."""
    c, p, st, sc, sh = own_coeffs(fn, args)
    fw = R.forward(p, sc, sh, SC.SLOPE)
    share = float(R.excluded(fw, SC.TAU).double().mean())
    print("excluded share %.2e, exact ties %.3f" % (share, float((fw.gap == 0).double().mean())))
    assert share <= SC.MAX_EXCLUDED


@pytest.mark.parametrize("kind", ["rows", "cols", "bands"])
def test_tie_inputs_tie(kind):
    c, p, st, sc, sh = own_coeffs(SC.make_ties, (kind,))
    assert torch.equal(c.x16, c.x.double()) and torch.equal(c.w16, c.w.double())
    assert torch.equal(c.x16 * 16, (c.x16 * 16).round()) and torch.equal(c.w16 * 8, (c.w16 * 8).round())
    y32 = F.conv2d(c.x, c.w, None, 1, 1).permute(0, 2, 3, 1).double()
    assert torch.equal(y32, p.y)                                   # exact in float32 as well
    fw = R.forward(p, sc, sh, SC.SLOPE)
    live = sc != 0
    tied = float((fw.gap[:, live] == 0).double().mean())
    print("%s: %.1f %% of the windows tie" % (kind, 100 * tied))
    assert tied >= 0.25
    assert not ((fw.gap > 0) & (fw.gap < SC.TAU)).any()
    yw = R.windows(p.y)
    if kind == "rows":
        assert torch.equal(yw[..., 0], yw[..., 2]) and torch.equal(yw[..., 1], yw[..., 3])
        assert not torch.equal(c.x16[:, :, 1::2][:, :, :-1], c.x16[:, :, 2::2])        # neighbouring pairs differ
    if kind == "cols":
        assert torch.equal(yw[..., 0], yw[..., 1]) and torch.equal(yw[..., 2], yw[..., 3])
    # the choice shows: the LAST maximum of every window (the first maximum of the image turned by 180 degrees) moves T by
    # far more than the bound of the comparison
    turned = R.Pre(p.x.flip(2, 3), p.w.flip(2, 3), p.y.flip(1, 2), p.ay.flip(1, 2))
    a = (c.gamma.double(), st.mean, st.invstd, sc, sh, SC.SLOPE)
    ref, last = R.backward(p, *a, c.G, st), R.backward(turned, *a, c.G.flip(2, 3), st)
    moved = ((last.T.view(32, 3, 3, 3).flip(2, 3).reshape(32, 27) - ref.T).abs() / (EPS32 * ref.A)).max()
    print("%s: the last maximum instead of the first moves T by %.3g units" % (kind, float(moved)))
    assert float(moved) > 1e3 * SC.K_BWD


@pytest.mark.parametrize("image", ["a", "b", "c"])
def test_statistics_inputs_are_conditioned_as_intended(image):
    c, st = SC.make_stats(image), SC.stats(SC.make_stats, image)
    w = c.w16
    assert (w[SC.BLOB] > 0).all() and float(w[SC.EDGE].sum()) == 0.0 and w[SC.EDGE].any() and not w[SC.PRUNED].any()
    assert float(st.var[SC.TINY]) < R.f32(SC.EPS) and float(st.var[SC.PRUNED]) == 0.0
    assert float(st.var[SC.HUGE]) > 100.0 * float(st.var[5:].median())
    print("image %s: kappa blob %.3g edge %.3g tiny %.3g huge %.3g, others up to %.3g" % (
        image, st.kappa[SC.BLOB], st.kappa[SC.EDGE], st.kappa[SC.TINY], st.kappa[SC.HUGE], st.kappa[5:].max()))
    if image != "a":
        assert torch.equal((c.x * 255).round() / 255, c.x)
    # the blob is the badly centred channel, the more so the lower the contrast (the zero halo keeps kappa of "c" near 100:
    # 9 % of the pixels are border pixels, whose windows hold zeros)
    kb = [float(SC.stats(SC.make_stats, i).kappa[SC.BLOB]) for i in "abc"]
    assert 20.0 < kb[0] < kb[1] < kb[2] and kb[2] > 100.0 and float(st.kappa[SC.BLOB]) == float(st.kappa.max())


def test_plan_info_multipass_and_chain_lengths():
    """The launch plan, from the function the launches ask: the multi-pass shape gives every kernel at least two passes,
    and the chains of the single-pass shapes stay within the 128 steps of the yardstick's chains."""
    plan = ops.stem_block_plan_info(*SC.MULTIPASS)
    print(plan)
    for l in plan:
        assert l.passes >= 2 and l.grid * (l.per_pass // l.grid) == l.per_pass
    assert plan.fwd.items == plan.bwd.items == 32820 and plan.gram.items == 65640
    for shape in SC.SHAPES + [SC.STATS_SHAPE, SC.TIES_SHAPE, SC.MULTIPASS]:
        for l in ops.stem_block_plan_info(*shape):
            assert 1 <= l.per_wave <= 128 and l.per_pass * l.passes >= l.items > l.per_pass * (l.passes - 1)


@pytest.mark.parametrize("B, H, W", [(1, 2, 32), (3, 6, 64), (2, 416, 416), (64, 416, 416), (5470, 6, 64), (7, 30, 96)])
def test_plan_info_keeps_the_grids(B, H, W):
    """The grids the launches took before they asked one function, and mcamd_stem_block_stats_rows as it was."""
    units, steps = B * (H // 2) * (W // 32), B * H * (W // 32)
    plan = ops.stem_block_plan_info(B, H, W)
    assert plan.fwd.grid == plan.fwd_planes.grid == min(max((units + 7) // 8, 1), 2048)
    assert plan.stats.grid == min(max((units + 7) // 8, 1), 1024) == ops.stem_block_stats_rows(B, H, W)
    assert plan.gram.grid == min(max((steps + 31) // 32, 1), 512) and plan.bwd.grid == min(max((units + 31) // 32, 1), 256)
    assert (plan.fwd.per_pass, plan.fwd_planes.per_pass, plan.stats.per_pass) == (16 * plan.fwd.grid, 8 * plan.fwd.grid, 8 * plan.stats.grid)
    assert (plan.gram.per_pass, plan.bwd.per_pass) == (32 * plan.gram.grid, 8 * plan.bwd.grid)


@pytest.mark.parametrize("bad, text", [(dict(B=0), "non-positive"), (dict(H=3), "even H"), (dict(W=48), "W % 32"),
                                       (dict(B=1 << 20, H=64, W=64), "2^31")])
def test_plan_info_refuses_bad_shapes(bad, text):
    d = _lib.StemBlockDesc()
    d.B, d.H, d.W = 2, 4, 32
    for k, v in bad.items():
        setattr(d, k, v)
    out = (C.c_int32 * _lib.STEM_PLAN_INFO_N)()
    lib = _lib.lib()
    assert lib.mcamd_stem_block_plan_info(C.byref(d), out) == -1
    msg = lib.mcamd_last_error().decode()
    assert msg.startswith("stem_block_plan_info:") and text in msg, msg
    assert lib.mcamd_stem_block_plan_info(None, out) == -1 and lib.mcamd_stem_block_plan_info(C.byref(d), None) == -1
