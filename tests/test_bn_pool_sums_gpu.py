"""Pass 0 of a MaxPool block's BatchNorm backward from the POOLED tensors (mcamd_act_bwd_desc.pool_out, bn_pool_sums_kernel).

Only the pooled element of a 2x2 window has a gradient at the pre-activation, so the two per-channel sums need that
element's activation alone.  The forward pass stores it twice -- as the pooled output and, in the full-resolution copy
(mcamd_act_desc.pool_act), as the window's strict maximum -- so the sums can be formed from pooled G + pooled activation
(4 bytes per window and channel) instead of pooled G + the four copies (10 bytes).  At the shapes of YOLOv2's conv2 /
conv5 / conv8 (the MaxPool blocks with one consumer), B reduced and one at B = 64:

1. the premise, on the forward pass's own output: the hi plane of the pooled output equals the maximum of the four stored
   copies BIT FOR BIT (windows that tie after rounding, exact ties and all-negative windows included);
2. dgamma, dbeta and dY of the new route against the present one (MCAMD_BN_POOL_SUMS_POOLED=0) within 4x the
   summation-order noise of the PRESENT pass, measured as the difference between two of its grid sizes on the same inputs;
3. both routes against a float64 host reference, to the bounds of tests/test_kernels_gpu.py (layer-wide) and
   tests/test_bn_conditioning_gpu.py (per channel) for this block kind;
4. channels with gamma in {1e-3, 1e-2} and |beta| about 1 (and gamma == 0) take the fallback -- argmax from the copy, z
   from the saved fp32 y -- and match the float64 reference and the fp32-y kernel at fp32-accumulation accuracy;
5. two runs are bit-equal.

Every case also runs WITHOUT the full-resolution copy (engines with filter compaction switch it off): the present pass 0
is then bn_pool_bwd_kernel<0, BN_SRC_Y32, false> on the saved fp32 y, the pooled route bn_pool_sums_kernel<false>, whose
ill-conditioned channels take the argmax from the unrounded activations of y.  There the two routes differ by the fp16
rounding of the pooled activation (the trade the PLAIN blocks made), not by summation order: check 2 does not apply and
its figures are only printed; the premise is checked against the unrounded activations, and 3 - 5 hold with the y
kernels' tolerance for the present route and the stored-activation tolerance for the pooled one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops  # noqa: E402
from modelcompression_amd import _lib as L  # noqa: E402
from util import halo_is_zero, rel_l2  # noqa: E402

EPS = 1e-5
T = 2.0 ** -5          # BN_ACT_T of csrc/bn_act.hip
U16 = 2.0 ** -11       # unit roundoff of fp16
S = 4.0                # grad_scale
SLOPE = 0.1
ZERO, PRUNED = 3, 7                                   # gamma == 0; dy_keep 0
LOW = {8: (1e-3, 1.0), 9: (-1e-3, -1.0), 10: (1e-2, -1.1), 11: (-1e-2, 0.9)}      # channel: (gamma, beta)

# (name, C, B, H, W, storage form of the pooled buffer (0 padded, 1 shared-halo), skip_dead_from)
CASES = [
    ("conv2-b2", 64, 2, 208, 208, 0, 0),
    ("conv5-b4", 128, 4, 104, 104, 1, 0),
    ("conv8-b8", 256, 8, 52, 52, 0, 248),
    ("conv8-b64", 256, 64, 52, 52, 1, 0),
]
# Summation-order noise of the PRESENT pass 0 (bn_pool_bwd_kernel<0, BN_SRC_ACT, false>): 1024 against 384 workgroups on the inputs
# of each case with the copy, as measured on an MI355X (the test prints the figures of its own run beside them):
#   dgamma: max over channels of |difference| / sum|g_z xhat|,  dbeta: of |difference| / sum|g_z|,  dY: rel-L2.
# The new route may differ from the present one by 4x these.  (Measured difference: 0 in all three, at every case -- at the
# same grid a thread of either pass adds the same fp32 terms for the same windows in the same order.)
# dY is an fp16 tensor that depends on the sums through two fp32 coefficients per channel only: the noise there is the
# occasional element whose rounding flips.
NOISE = {
    "conv2-b2": (7.93e-08, 8.88e-08, 7.2e-07),
    "conv5-b4": (1.12e-07, 7.06e-08, 1.76e-06),
    "conv8-b8": (9.24e-08, 8.15e-08, 1.89e-07),
    "conv8-b64": (1.0e-07, 1.13e-07, 6.48e-07),
}
MARGIN = 4.0
BLOCKS_B = "384"       # every case has more than 384 workgroups of 256 items


def _win(t, B, H, W):
    """[B, H, W, C] -> the 2x2 windows [B, H/2, W/2, 4, C], k = 2 dh + dw (the kernels' scan order)."""
    C = t.shape[-1]
    return t.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4, C)


def _unwin(t, B, H, W):
    C = t.shape[-1]
    return t.reshape(B, H // 2, W // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * H * W, C)


def _inputs(C, B, H, W, gen):
    """fp32 y with windows whose two largest activations differ by less than an fp16 step, exact ties, and windows that
    are negative in all four elements; gamma > 0 except the LOW / ZERO channels."""
    y4 = torch.randn(B, H, W, C, generator=gen) * 0.7 + 0.4
    q = C // 4
    y4[:, 0::2, 0::2, :q] = y4[:, 0::2, 1::2, :q].abs() + 2.0
    y4[:, 0::2, 1::2, :q] = y4[:, 0::2, 0::2, :q] * (1.0 + 3e-5)          # the later element larger, by less than 2^-11
    y4[:, 1::2, 1::2, :4] = y4[:, 0::2, 1::2, :4]                          # exact ties
    y4[:, : H // 2, :, q:2 * q] = -y4[:, : H // 2, :, q:2 * q].abs() - 1.5   # all-negative windows (z < 0 at gamma > 0)
    gamma = torch.rand(C, generator=gen, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=gen, dtype=torch.float64) * 0.2
    gamma[ZERO] = 0.0
    for c, (gv, bv) in LOW.items():
        gamma[c], beta[c] = gv, bv
    return y4, gamma, beta


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pool_sums_from_pooled_tensors(dev, setenv, case, copy):
    name, C, B, H, W, ppad, skip_from = case
    gen = torch.Generator().manual_seed(41 + C + B)
    M, Ho, Wo = B * H * W, H // 2, W // 2
    P = M // 4
    y4, gamma, beta = _inputs(C, B, H, W, gen)
    yk = y4.reshape(M, C)
    ykd = yk.double()
    mean = ykd.mean(0)
    invstd = 1.0 / torch.sqrt(ykd.var(0, unbiased=False) + EPS)
    scale = (gamma * invstd).float()                                 # as bn_coeffs forms them
    shift = (beta - mean * scale.double()).float()
    keep = torch.ones(C)
    keep[PRUNED] = 0.0
    xhat = (ykd - mean) * invstd                                     # [M, C] float64
    del ykd
    # gradients correlated with the pooled xhat in some channels, so that c1 and c2 are both O(rms g) there
    alpha = torch.tensor([1.0, 3.0, 0.0], dtype=torch.float32)[(torch.arange(C) // 5) % 3]
    offset = torch.tensor([0.0, 1.0], dtype=torch.float32)[(torch.arange(C) // 3) % 2]
    gsig = _win(xhat.float().view(B, H, W, C), B, H, W).amax(3).reshape(P, C)
    gq = ((alpha * gsig + torch.randn(P, C, generator=gen) + offset) * S).half()
    del gsig

    # ---- device: the forward pass itself writes the pooled output (two planes, a channel slice of a wider buffer) and the copy
    ydev = yk.to(dev)
    sc, sh, mu, ist = (t.contiguous().to(dev) for t in (scale, shift, mean.float(), invstd.float()))
    pld, pch = 2 * C + 64, 32
    pooled = ops.alloc_padded(B, Ho, Wo, pld, dev, pad=ppad)
    ald = C + 8
    abuf = ops.alloc_padded(B, H, W, ald, dev) if copy else None
    ops.bn_act_fwd(B, H, W, C, ydev.view(-1), C, 0, sc, sh, SLOPE, L.DST_POOL, pooled, pld, pch, None, 0, 0,
                   planes=2, dst_plane=C, dst_pad=ppad, pool_act=abuf, pool_act_ld=ald if copy else 0, pool_act_pad=0)
    g_ld = C + 16
    gdev = torch.zeros(P, g_ld, dtype=torch.float16, device=dev)
    gdev[:, 8:8 + C] = gq.to(dev)
    keepd = keep.to(dev)

    # ---- 1. the premise: pooled hi plane == maximum of the four stored copies, bit for bit
    # (without the copy: == the fp16 rounding of the maximum of the four unrounded activations)
    z32 = (yk.double() * scale.double() + shift.double()).float()                    # fp32 fma, emulated through float64
    a32 = torch.where(z32 > 0, z32, z32 * torch.tensor(SLOPE, dtype=torch.float32))
    aw = _win(a32.view(B, H, W, C), B, H, W)
    arg = aw.argmax(3, keepdim=True)                                                 # first maximum of the unrounded values
    pos_arg = _win((z32 > 0).view(B, H, W, C), B, H, W).gather(3, arg).squeeze(3).reshape(P, C)
    del z32
    hi_d = ops.padded_view(pooled, B, Ho, Wo, pld, pad=ppad)[:, 1:-1, 1:-1, pch:pch + C]
    if copy:
        stored_d = ops.padded_view(abuf, B, H, W, ald, pad=0)[:, 1:-1, 1:-1, :C]
        sw_d = _win(stored_d, B, H, W)
        top_d = sw_d.amax(3)
        assert int((sw_d == top_d.unsqueeze(3)).sum(3).max()) == 1                   # the maximum is strict
        stored = stored_d.float().cpu()
    else:
        top_d = aw.amax(3).half().to(dev)
        stored = a32.half().float().view(B, H, W, C)
    assert torch.equal(hi_d.contiguous().view(torch.int16), top_d.contiguous().view(torch.int16)), \
        "%s: the pooled output is not the maximum of the stored copies bit for bit" % name
    sw = _win(stored, B, H, W)
    if copy:
        assert torch.equal(sw.argmax(3, keepdim=True), arg), "%s: the pooled element is not the stored maximum" % name
    n_tied = int(((aw.half() == aw.half().amax(3, keepdim=True)).sum(3) > 1).sum())
    n_neg = int((sw.amax(3) < 0).sum())
    print("%s: %d windows x channels, %d tie after rounding, %d negative in all four elements" % (name, P * C, n_tied, n_neg))
    assert n_tied > P * C // 8 and n_neg > P * C // 16
    del a32, aw

    # ---- the float64 host reference, with the kernels' decisions (side: sign of the stored value; pooled element: arg)
    top = sw.gather(3, arg).squeeze(3).reshape(P, C)
    # (the y kernels take the side from the unrounded z: the same decision unless an activation underflows in fp16)
    assert bool(((top > 0) == pos_arg).all())
    gz_p = gq.double() / S * torch.where(top > 0, 1.0, SLOPE).double()               # g_z of the pooled element [P, C]
    xh_p = _win(xhat.view(B, H, W, C), B, H, W).gather(3, arg).squeeze(3).reshape(P, C)
    dg_ref, db_ref = (gz_p * xh_p).sum(0), gz_p.sum(0)
    sgx, sg = (gz_p * xh_p).abs().sum(0), gz_p.abs().sum(0)
    gz4 = torch.zeros(B, Ho, Wo, 4, C, dtype=torch.float64)
    gz4.scatter_(3, arg, gz_p.view(B, Ho, Wo, 1, C))
    gz = _unwin(gz4, B, H, W)                                                        # [M, C]
    del gz4, gz_p, xh_p, sw, stored
    dm = gamma * invstd * keep.double()
    dy_ref = dm * (gz - db_ref / M - xhat * (dg_ref / M))
    del gz

    def run(pooled_route, blocks=None, with_act=True):
        setenv("MCAMD_BN_POOL_SUMS_POOLED", "1" if pooled_route else "0")
        setenv("MCAMD_BN_BWD_BLOCKS", blocks or "0")
        dy = ops.alloc_padded(B, H, W, C, dev)
        dgm, dbt = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
        kw = {}
        if with_act:
            kw = dict(pool_out=pooled, pool_out_ld=pld, pool_out_choff=pch, pool_out_pad=ppad)
            if copy:
                kw.update(act=abuf, act_ld=ald, act_choff=0, act_pad=0)
        ops.bn_act_bwd(B, H, W, C, ydev.view(-1), C, 0, sc, sh, mu, ist, SLOPE, L.DST_POOL, gdev.view(-1), g_ld, 8, dy, C, 0,
                       dgm, dbt, grad_scale=S, dy_keep=keepd, skip_dead_from=skip_from, **kw)
        torch.cuda.synchronize()
        assert halo_is_zero(dy, B, H, W, C)
        dyv = ops.padded_view(dy, B, H, W, C, pad=0)[:, 1:-1, 1:-1].reshape(M, C)
        return dyv, dgm.cpu().double(), dbt.cpu().double()

    new = run(True)
    new2 = run(True)
    old = run(False)
    old_b = run(False, BLOCKS_B)
    ykern = run(False, with_act=False)                               # bn_pool_bwd_kernel<., BN_SRC_Y32, false>: the fp32-y kernel

    written = torch.ones(C, dtype=torch.bool)
    if skip_from:
        written[skip_from:] = False
        for r in (new, old):
            assert bool(torch.isnan(r[1][~written]).all()) and bool(torch.isnan(r[2][~written]).all())
    if not copy:                                                     # the fp32-y kernel IS the present route without the copy
        assert torch.equal(ykern[0], old[0])
        assert torch.equal(ykern[1][written], old[1][written]) and torch.equal(ykern[2][written], old[2][written])
    ill = gamma.abs() < T * beta.abs().clamp_min(1.0)
    assert bool(ill[ZERO]) and all(bool(ill[c]) for c in LOW) and int(ill.sum()) == 1 + len(LOW)

    # ---- 5. two runs are bit-equal
    assert torch.equal(new[0], new2[0])
    assert torch.equal(new[1][written], new2[1][written]) and torch.equal(new[2][written], new2[2][written])

    # ---- 2. new route against the present one, within 4x the present pass's own summation-order noise
    def diff(a, b):
        eg = float(((a[1] - b[1]).abs() / sgx.clamp_min(1e-30))[written].max())
        eb = float(((a[2] - b[2]).abs() / sg.clamp_min(1e-30))[written].max())
        return eg, eb, rel_l2(a[0].float(), b[0].float())
    noise_now, d_new = diff(old, old_b), diff(new, old)
    ng, nb, ny = NOISE[name]
    print("%s: present pass, 1024 vs %s workgroups: dgamma %.3g  dbeta %.3g  dY rel-L2 %.3g   (recorded %.3g %.3g %.3g)"
          % ((name, BLOCKS_B) + noise_now + (ng, nb, ny)))
    print("%s: pooled route vs present route:       dgamma %.3g  dbeta %.3g  dY rel-L2 %.3g" % ((name,) + d_new))

    # ---- 3. + 4. both routes against the float64 reference
    xmax, xrms = xhat.abs().amax(0), xhat.pow(2).mean(0).sqrt()
    del xhat
    healthy = ~ill
    c2 = dg_ref / M
    rms_ref = dy_ref.pow(2).mean(0).sqrt()
    zeros = torch.zeros(C, dtype=torch.float64)
    dy_ref_d = dy_ref.to(dev)
    figures = {}
    for rname, r in (("pooled", new), ("present", old)):
        # test_bn_conditioning_gpu._check: e is the xhat error of a well-conditioned channel recovered from an fp16 activation
        # (the pooled route always, the present one with the copy); 0 where xhat comes from the fp32 y
        from_act = healthy if (copy or rname == "pooled") else torch.zeros(C, dtype=torch.bool)
        e = torch.where(from_act, U16 * (1.0 / T + xmax), zeros)
        tg, tb = 1e-5 * sgx + e * sg + 1e-30, 1e-5 * sg + 1e-30
        tol_dy = 2e-3 * rms_ref + torch.where(from_act, dm.abs() * e * (c2.abs() + xrms * sg / M), zeros)
        eg, eb = (r[1] - dg_ref).abs(), (r[2] - db_ref).abs()
        err = ((r[0].double() / S - dy_ref_d).pow(2).mean(0).sqrt()).cpu()
        lw = (rel_l2(r[0].double().cpu() / S, dy_ref), rel_l2(r[1][written & healthy], dg_ref[written & healthy]),
              rel_l2(r[2][written], db_ref[written]))
        print("%s: %s route vs float64: dY rel-L2 %.3g  dgamma rel-L2 (healthy) %.3g  dbeta rel-L2 %.3g; worst per channel "
              "dgamma err / tol %.3g  dbeta %.3g  dY %.3g; ill-conditioned dgamma err / sum|g_z xhat| %.3g"
              % ((name, rname) + lw + (float((eg / tg)[written].max()), float((eb / tb)[written].max()),
                                        float((err / tol_dy.clamp_min(1e-30))[keep > 0].max()),
                                        float((eg / sgx.clamp_min(1e-30))[ill & written].max()))))
        figures[rname] = (eg, eb, err, lw, tg, tb, tol_dy)
    low = torch.tensor(sorted(LOW) + [ZERO])
    fb_g = float(((new[1] - ykern[1]).abs() / sgx.clamp_min(1e-30))[low].max())
    fb_b = float(((new[2] - ykern[2]).abs() / sg.clamp_min(1e-30))[low].max())
    fb_y = rel_l2(new[0][:, sorted(LOW)].float(), ykern[0][:, sorted(LOW)].float())
    print("%s: fallback channels, pooled route vs the fp32-y kernel: dgamma %.3g  dbeta %.3g  dY rel-L2 %.3g" % (name, fb_g, fb_b, fb_y))

    for rname in ("pooled", "present"):
        eg, eb, err, lw, tg, tb, tol_dy = figures[rname]
        assert lw[0] < 3e-3 and lw[1] < 2e-3 and lw[2] < 1e-4, (rname, lw)          # test_bn_pool_bwd_from_stored_activation
        assert bool((eg <= tg)[written].all()) and bool((eb <= tb)[written].all()), rname
        assert bool((err <= tol_dy)[keep > 0].all()), rname
    assert float(new[0][:, PRUNED].abs().max()) == 0.0 and float(new[0][:, ZERO].abs().max()) == 0.0
    # 4.: both within 1e-5 of the float64 sums (asserted above for the pooled route, by construction of the fp32-y kernel for
    # the other), hence within 2e-5 of each other; their dY are two fp16 roundings of coefficients that close
    assert fb_g <= 2e-5 and fb_b <= 2e-5 and fb_y < 2e-3
    # 2.
    if copy:
        assert d_new[0] <= MARGIN * ng and d_new[1] <= MARGIN * nb and d_new[2] <= MARGIN * ny, (d_new, NOISE[name])


def test_pool_out_is_refused_where_it_does_not_apply(dev):
    """pool_out goes with a MaxPool block that has `act` or an fp32 `y`, and no second gradient; anything else is an error,
    not a silent full-resolution pass."""
    C, B, H, W = 32, 1, 8, 8
    M = B * H * W
    f = lambda n: torch.ones(n, device=dev)
    y = torch.zeros(M * C, device=dev)
    g = torch.zeros(M // 4 * C, dtype=torch.float16, device=dev)
    g2 = torch.zeros(M * C, dtype=torch.float16, device=dev)
    dy, abuf = ops.alloc_padded(B, H, W, C, dev), ops.alloc_padded(B, H, W, C, dev)
    pooled = ops.alloc_padded(B, H // 2, W // 2, C, dev)
    po = dict(pool_out=pooled, pool_out_ld=C, pool_out_choff=0, pool_out_pad=0)
    act = dict(act=abuf, act_ld=C, act_choff=0, act_pad=0)
    args = (B, H, W, C, y, C, 0, f(C), f(C), f(C), f(C), SLOPE, L.DST_POOL, g, C, 0, dy, C, 0, f(C), f(C))
    for kw in (dict(po, **act, g2=g2, g2_ld=C), dict(po, g2=g2, g2_ld=C), dict(act, pool_out=pooled, pool_out_ld=C, pool_out_choff=8)):
        with pytest.raises(L.McamdError):
            ops.bn_act_bwd(*args, **kw)
    args16 = args[:4] + (y.half(),) + args[5:]
    with pytest.raises(L.McamdError):                     # an fp16 y: its xhat is exact, the pooled activation's is not
        ops.bn_act_bwd(*args16, **po)
    ops.bn_act_bwd(*args, **dict(po, **act))
    ops.bn_act_bwd(*args, **po)
    torch.cuda.synchronize()
