"""BatchNorm backward per channel, including the channels where the stored-activation kernels are ill-conditioned.

Every dispatch target of mcamd_bn_act_bwd is checked against ONE float64 reference: nn.BatchNorm2d with batch statistics
(F.batch_norm, training) -> LeakyReLU -> plain / MaxPool2d(2, 2) / Darknet reorg, plus an optional second full-resolution
gradient, under autograd on exactly the y the kernel reads (fp16 values for the fp16-y kernels, the fp32 y otherwise).
The discrete decisions are the kernel's own contract and are given to the reference: the LeakyReLU side is the sign of
the fp32 z = fma(y, scale, shift) (of the STORED activation for the act kernels), and the pooled element is the first
maximum of the activation as the forward pass kept it (fp16-rounded for the fp16-y kernels, unrounded otherwise; the
act kernels find it as the strict maximum of the stored copy, which is checked against the unrounded one here).

Assertions are per channel, with tolerances derived from the channel's own terms -- never a layer-wide norm, in which a
few wrong channels vanish.  See _check for the derivation."""
import inspect
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops  # noqa: E402
from modelcompression_amd import _lib as L  # noqa: E402
from oracle.darknet_ref import reorg  # noqa: E402
from util import halo_is_zero, rel_l2  # noqa: E402

EPS = 1e-5
T = 2.0 ** -5          # BN_ACT_T of csrc/bn_act.hip: |gamma| < T max(|beta|, 1) is ill-conditioned for the act kernels
U16 = 2.0 ** -11       # unit roundoff of fp16
S = 4.0                # grad_scale

GAMMAS = [0.0, 1e-4, -1e-4, 1e-3, -1e-3, 1e-2, -1e-2, 0.05, -0.05, 1.0, -1.0]
BETAS = [0.0, 0.5, -0.5, 2.0, -2.0, 8.0, -8.0]
RATIOS = [0.0, 3.0, 10.0]          # |mean| / std of y
PRUNED = 7                         # dy_keep 0
STRADDLE = (20, 21)                # beta 2, |gamma| just below / just above T max(|beta|, 1)


def _channels(C, gen):
    c = torch.arange(C)
    gamma = torch.tensor(GAMMAS, dtype=torch.float64)[c % len(GAMMAS)]
    beta = torch.tensor(BETAS, dtype=torch.float64)[(c // len(GAMMAS) + c) % len(BETAS)]
    ratio = torch.tensor(RATIOS, dtype=torch.float64)[(c // 2) % len(RATIOS)]
    s0, s1 = STRADDLE
    beta[s0] = beta[s1] = 2.0
    gamma[s0], gamma[s1] = T * 2.0 * (1 - 2e-3), -T * 2.0 * (1 + 2e-3)
    ratio[s0] = ratio[s1] = 0.0
    std = 0.5 + torch.rand(C, generator=gen, dtype=torch.float64)
    sign = torch.where(torch.rand(C, generator=gen) < 0.5, -1.0, 1.0).double()
    alpha = torch.tensor([1.0, 3.0, 0.0], dtype=torch.float64)[(c // 5) % 3]       # g = alpha xhat + noise + offset
    offset = torch.tensor([0.0, 1.0], dtype=torch.float64)[(c // 3) % 2]
    return gamma, beta, sign * ratio * std, std, alpha, offset


def _win(t, B, H, W):
    """[B, H, W, C] -> the 2x2 windows [B, H/2, W/2, 4, C], k = 2 dh + dw (the kernels' scan order)."""
    C = t.shape[-1]
    return t.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4, C)


def _reference(y, gamma, beta, slope, mode, pos, arg, g, g2, B, H, W):
    """float64 autograd.  y [M, C] (what the kernel reads); pos [M, C] bool (LeakyReLU side); arg [B, H/2, W/2, 1, C] (pool);
    g at the mode's resolution ([M, C], [M/4, C], [M/4, 4C] in the kernel's layout); g2 [M, C] or None.
    Returns dY [M, C], dgamma, dbeta and, per channel, g_z [M, C] and xhat [M, C]."""
    C = y.shape[1]
    yl = y.detach().double().clone().requires_grad_(True)
    gm, bt = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    z = F.batch_norm(yl, None, None, gm, bt, True, 0.0, EPS)
    z.retain_grad()
    a = torch.where(pos, z, z * slope)
    if mode == L.DST_PLAIN:
        loss = (a * g).sum()
    elif mode == L.DST_POOL:
        loss = (_win(a.view(B, H, W, C), B, H, W).gather(3, arg).squeeze(3) * g.view(B, H // 2, W // 2, C)).sum()
    else:
        nchw = a.view(B, H, W, C).permute(0, 3, 1, 2)
        loss = (reorg(nchw, 2) * g.view(B, H // 2, W // 2, 4 * C).permute(0, 3, 1, 2)).sum()
    if g2 is not None:
        loss = loss + (a * g2).sum()
    loss.backward()
    y64 = y.double()
    xhat = (y64 - y64.mean(0)) / torch.sqrt(y64.var(0, unbiased=False) + EPS)
    return yl.grad, gm.grad, bt.grad, z.grad, xhat


def _decisions(y32, scale, shift, slope, B, H, W, mode, y16):
    """The kernels' LeakyReLU sides (z32 > 0) and pooled elements (first maximum of the activation as the forward pass kept
    it), from z32 = fma(y, scale, shift) in fp32 -- emulated through float64, where y * scale is exact."""
    z32 = (y32.double() * scale.double() + shift.double()).float()
    a32 = torch.where(z32 > 0, z32, z32 * torch.tensor(slope, dtype=torch.float32))
    arg = None
    if mode == L.DST_POOL:
        key = a32.half().float() if y16 else a32
        arg = _win(key.view(B, H, W, -1), B, H, W).argmax(3, keepdim=True)      # first maximum
    return z32 > 0, arg, a32


# (name, mode, y dtype, act storage form (None: y kernel; 0 padded, 1 shared-halo), g2, environment, slope)
VARIANTS = [
    ("plain-y16", L.DST_PLAIN, 16, None, False, {}, 0.1),              # bn_plain_bwd_kernel<., BN_SRC_Y16>
    ("plain-y32", L.DST_PLAIN, 32, None, False, {}, 1.0),              # bn_plain_bwd_kernel<., BN_SRC_Y32>
    ("plain-act", L.DST_PLAIN, 32, 0, False, {}, 0.1),                 # bn_plain_bwd_kernel<., BN_SRC_ACT>
    ("plain-act-halo", L.DST_PLAIN, 32, 1, False, {}, 1.0),
    ("plain-generic-y16", L.DST_PLAIN, 16, None, False, {"MCAMD_BN_PLAIN_FAST": "0"}, 0.1),   # bn_act_bwd_kernel
    ("plain-generic-y32", L.DST_PLAIN, 32, None, False, {"MCAMD_BN_PLAIN_FAST": "0"}, 0.1),
    ("plain-g2-y16", L.DST_PLAIN, 16, None, True, {}, 0.1),            # PLAIN with g2: the generic kernel
    ("plain-g2-y32", L.DST_PLAIN, 32, None, True, {}, 0.1),
    ("pool-y16", L.DST_POOL, 16, None, False, {}, 0.1),                # bn_pool_bwd_kernel<., SRC, G2>
    ("pool-y16-g2", L.DST_POOL, 16, None, True, {}, 0.1),
    ("pool-y32", L.DST_POOL, 32, None, False, {}, 1.0),
    ("pool-y32-g2", L.DST_POOL, 32, None, True, {}, 0.1),
    ("pool-act", L.DST_POOL, 32, 0, False, {}, 0.1),                   # bn_pool_bwd_kernel<., BN_SRC_ACT, G2>
    ("pool-act-g2-halo", L.DST_POOL, 32, 1, True, {}, 0.1),
    ("pool-generic-y16", L.DST_POOL, 16, None, False, {"MCAMD_BN_POOL_FAST": "0"}, 0.1),
    ("pool-generic-y32-g2", L.DST_POOL, 32, None, True, {"MCAMD_BN_POOL_FAST": "0"}, 0.1),
    ("reorg-y16", L.DST_REORG, 16, None, False, {}, 0.1),              # the generic kernel
    ("reorg-y32", L.DST_REORG, 32, None, False, {}, 0.1),
]
# C = 64: one item per thread, a channel slice of a wider y with `perm` (filter compaction); C = 256: a grid-stride loop
SHAPES = {64: (2, 20, 12), 256: (2, 136, 128)}


def _check(name, C, ill, act, dy, dg, db, ref, keep, gamma, invstd, failures):
    """Per channel c, with N = B H W, g_z = dL/dz and xhat of the float64 reference:

    fp32 accumulation (every channel of the y kernels, the ill-conditioned channels of the act kernels, which read y):
        |dgamma - ref| <= 1e-5 sum|g_z xhat|,   |dbeta - ref| <= 1e-5 sum|g_z|,
        rel-L2(dY) <= 2e-3 (fp16 output rounding, 2^-11 per element).
    Well-conditioned channels of the act kernels (|gamma| >= T max(|beta|, 1)): the stored activation a = fp16(leaky(z))
    carries |dz| <= 2^-11 |z|, and z = gamma xhat + beta, so xhat = (z - beta) / gamma is off by
        |dxhat| <= 2^-11 (|xhat| + |beta / gamma|) <= e := 2^-11 (1 / T + max|xhat|).
    Hence |dgamma - ref| <= 1e-5 sum|g_z xhat| + e sum|g_z|.  dY = dm (g_z - c1 - xhat c2) with dm = gamma invstd,
    c1 = sum g_z / N, c2 = sum g_z xhat / N: the kernel's c2 is off by at most e mean|g_z|, so per element
    |ddY| <= |dm| e (|c2| + |xhat| mean|g_z|), and
        rms(dY - ref) <= 2e-3 rms(ref) + |dm| e (|c2| + rms(xhat) mean|g_z|).
    Pruned channels (dy_keep 0): dY exactly 0."""
    dY_ref, dg_ref, db_ref, gz, xhat = ref
    N = gz.shape[0]
    worst_ill = 0.0
    for c in range(C):
        sgx, sg = float((gz[:, c] * xhat[:, c]).abs().sum()), float(gz[:, c].abs().sum())
        healthy_act = act and not bool(ill[c])
        e = U16 * (1.0 / T + float(xhat[:, c].abs().max())) if healthy_act else 0.0
        tg, tb = 1e-5 * sgx + e * sg + 1e-30, 1e-5 * sg + 1e-30
        eg, eb = abs(float(dg[c]) - float(dg_ref[c])), abs(float(db[c]) - float(db_ref[c]))
        if eg > tg:
            failures.append("%s C=%d ch %d (gamma %.3g): dgamma %.6g ref %.6g, |err| %.3g > %.3g (= %.3g sum|g_z xhat|)"
                            % (name, C, c, float(gamma[c]), float(dg[c]), float(dg_ref[c]), eg, tg, eg / max(sgx, 1e-30)))
        if eb > tb:
            failures.append("%s C=%d ch %d: dbeta |err| %.3g > %.3g" % (name, C, c, eb, tb))
        if act and bool(ill[c]):
            worst_ill = max(worst_ill, eg / max(sgx, 1e-30))
        d, r = dy[:, c].double(), dY_ref[:, c]
        if float(keep[c]) == 0.0:
            if float(d.abs().max()) != 0.0:
                failures.append("%s C=%d ch %d: pruned channel's dY is not 0" % (name, C, c))
            continue
        rms_ref = float(r.norm()) / N ** 0.5
        err = float((d - r).norm()) / N ** 0.5
        if rms_ref == 0.0:
            if err != 0.0:
                failures.append("%s C=%d ch %d: dY %.3g where the reference is 0" % (name, C, c, err))
            continue
        tol = 2e-3 * rms_ref
        if healthy_act:
            dm = abs(float(gamma[c]) * float(invstd[c]))
            c2 = float((gz[:, c] * xhat[:, c]).sum()) / N
            tol += dm * e * (abs(c2) + float(xhat[:, c].pow(2).mean().sqrt()) * sg / N)
        if err > tol:
            failures.append("%s C=%d ch %d (gamma %.3g): dY rms error %.3g > %.3g (rel-L2 %.3g)"
                            % (name, C, c, float(gamma[c]), err, tol, err / rms_ref))
    return worst_ill


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_bn_bwd_per_channel_vs_float64(dev, setenv, variant, C):
    name, mode, ybits, act_pad, dual, env, slope = variant
    for k, v in env.items():
        setenv(k, v)
    B, H, W = SHAPES[C]
    M = B * H * W
    gen = torch.Generator().manual_seed(101 + C + 7 * len(name))
    gamma, beta, mean_t, std_t, alpha, offset = _channels(C, gen)
    y64 = mean_t + std_t * torch.randn(M, C, generator=gen, dtype=torch.float64)
    yk = y64.half().float() if ybits == 16 else y64.float()          # the values the kernel reads
    ykd = yk.double()
    mean = ykd.mean(0)
    invstd = 1.0 / torch.sqrt(ykd.var(0, unbiased=False) + EPS)
    scale = (gamma * invstd).float()                                 # as bn_coeffs forms them
    shift = (beta - mean * scale.double()).float()
    mean32, invstd32 = mean.float(), invstd.float()
    keep = torch.ones(C)
    keep[PRUNED] = 0.0
    compact = C == 64
    y_ld, y_choff = (C + 64, 32) if compact else (C, 0)
    perm = torch.randperm(C, generator=gen).to(torch.int32) if compact else None
    # gradients correlated with xhat, so that c1 and c2 are both O(rms g) in some channels
    xh = (ykd - mean) * invstd
    if mode == L.DST_PLAIN:
        gsig = xh
    elif mode == L.DST_POOL:
        gsig = _win(xh.view(B, H, W, C), B, H, W).amax(3).reshape(-1, C)
    else:
        gsig = _win(xh.view(B, H, W, C), B, H, W).reshape(-1, 4, C)
    noise = torch.randn(gsig.shape, generator=gen, dtype=torch.float64)
    gval = (alpha * gsig + noise + offset).reshape(gsig.shape[0], -1)            # [P, C] or [P, 4C] (reorg: k C + c)
    gq = (gval * S).half()                                                        # fp16 as the kernels read it
    g2q = ((alpha * xh + torch.randn(M, C, generator=gen, dtype=torch.float64)) * S).half() if dual else None

    # ---- device buffers
    ydev = torch.zeros(M, y_ld, dtype=torch.float16 if ybits == 16 else torch.float32, device=dev)
    ydev[:, y_choff:y_choff + C] = yk.to(dev).to(ydev.dtype)
    g_ld = gq.shape[1] + 16
    gdev = torch.zeros(gq.shape[0], g_ld, dtype=torch.float16, device=dev)
    gdev[:, 8:8 + gq.shape[1]] = gq.to(dev)
    g2dev = None
    if dual:
        g2dev = torch.zeros(M, C + 8, dtype=torch.float16, device=dev)
        g2dev[:, 8:] = g2q.to(dev)
    sc, sh, mu, ist = (t.contiguous().to(dev) for t in (scale, shift, mean32, invstd32))
    pad = act_pad or 0
    act_kw, stored = {}, None
    if act_pad is not None:
        if mode == L.DST_PLAIN:          # the forward pass itself stores the activation: two planes, a channel slice
            ld = 2 * C + 64
            abuf = ops.alloc_padded(B, H, W, ld, dev, pad=pad)
            ops.bn_act_fwd(B, H, W, C, ydev.view(-1), y_ld, y_choff, sc, sh, slope, L.DST_PLAIN, abuf, ld, 32, None, 0, 0,
                           planes=2, dst_plane=C, dst_pad=pad)
            act_kw = dict(act=abuf, act_ld=ld, act_choff=32, act_pad=pad)
            stored = ops.padded_view(abuf, B, H, W, ld, pad=pad)[:, 1:-1, 1:-1, 32:32 + C]
        else:                            # ... and the pool's full-resolution copy (pooled element the strict maximum)
            ald = C + 8
            abuf = ops.alloc_padded(B, H, W, ald, dev, pad=pad)
            pooled = ops.alloc_padded(B, H // 2, W // 2, 2 * C, dev)
            ops.bn_act_fwd(B, H, W, C, ydev.view(-1), y_ld, y_choff, sc, sh, slope, L.DST_POOL, pooled, 2 * C, 0, None, 0, 0,
                           planes=2, dst_plane=C, pool_act=abuf, pool_act_ld=ald, pool_act_pad=pad)
            act_kw = dict(act=abuf, act_ld=ald, act_choff=0, act_pad=pad)
            stored = ops.padded_view(abuf, B, H, W, ald, pad=pad)[:, 1:-1, 1:-1, :C]
        stored = stored.float().cpu().reshape(M, C)

    def run(y_arg):
        dy = ops.alloc_padded(B, H, W, C, dev, pad=pad)
        dgm, dbt = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
        ops.bn_act_bwd(B, H, W, C, y_arg, y_ld, y_choff, sc, sh, mu, ist, slope, mode, gdev.view(-1), g_ld, 8, dy, C, 0, dgm, dbt,
                       grad_scale=S, g2=g2dev, g2_ld=C + 8 if dual else 0, g2_choff=8 if dual else 0, dy_keep=keep.to(dev),
                       perm=None if perm is None else perm.to(dev), dy_pad=pad, **act_kw)
        torch.cuda.synchronize()
        assert halo_is_zero(dy, B, H, W, C)
        dyv = ops.padded_view(dy, B, H, W, C, pad=pad)[:, 1:-1, 1:-1].float().cpu().reshape(M, C) / S
        dgc, dbc = dgm.cpu(), dbt.cpu()
        if perm is not None:             # written in parameter order: dgamma[perm[c]] belongs to physical channel c
            dgc, dbc = dgc[perm.long()], dbc[perm.long()]
        return dyv, dgc, dbc

    dy, dg, db = run(ydev.view(-1))

    # ---- the reference, with the kernel's decisions
    pos, arg, a32 = _decisions(yk, scale, shift, slope, B, H, W, mode, ybits == 16)
    if stored is not None:
        pos = stored > 0                                    # the act kernels take the side from the stored activation
        if mode == L.DST_POOL:
            sarg = _win(stored.view(B, H, W, C), B, H, W).argmax(3, keepdim=True)
            assert torch.equal(sarg, arg), "stored copy: the pooled element is not the strict maximum"
    ref = _reference(ykd, gamma, beta, slope, mode, pos, arg, gq.double() / S, g2q.double() / S if dual else None, B, H, W)
    ill = gamma.abs() < T * beta.abs().clamp_min(1.0)
    assert bool(ill[STRADDLE[0]]) and not bool(ill[STRADDLE[1]])
    failures = []
    worst = _check(name, C, ill, act_pad is not None, dy, dg, db, ref, keep, gamma, invstd, failures)
    if act_pad is not None:
        print("%s C=%d: worst ill-conditioned |ddgamma| / sum|g_z xhat| = %.3g" % (name, C, worst))
        # y = NULL: a channel without an xhat source (gamma == 0) gets dgamma 0; the well-conditioned channels and every
        # dbeta are unchanged, bit for bit
        dy0, dg0, db0 = run(None)
        zero = gamma == 0
        assert bool((dg0[zero] == 0).all())
        assert torch.equal(db0, db)
        assert torch.equal(dg0[~ill], dg[~ill]) and torch.equal(dy0[:, ~ill], dy[:, ~ill])
        assert float(dy0[:, zero].abs().max()) == 0.0
    assert not failures, "%d per-channel failures, first %s" % (len(failures), "\n".join(failures[:12]))


# ------------------------------------------------------------------ the default training engine, A/B on the act path
def _mini_engine_ab(dev, monkeypatch, masked, inject_low_gamma=True):
    from modelcompression_amd import nets
    from oracle import darknet_ref as O
    from modelcompression_amd.pruning.weightPruning.methods import quick_filter_prune
    monkeypatch.setenv("MCAMD_PLAN", "0")          # every launch goes through ops.bn_act_bwd (wrapped below)
    mini = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini.cfg")
    blocks = O.parse_cfg(mini)
    state = O.init_state(blocks, seed=4)
    gen = torch.Generator().manual_seed(9)
    x = torch.rand(4, 3, 64, 64, generator=gen)
    masks = None
    if masked:
        m0 = nets.Darknet(mini)
        m0.load_state_dict(state)
        m0.to(dev)
        masks = [mk.detach().clone() for mk in quick_filter_prune(m0, 40.0)]
    bn_keys = [k[:-len(".weight")] for k in O.param_keys(blocks) if ".bn" in k and k.endswith(".weight")]
    inject = {}
    vals = [(1e-4, 1.5), (1e-3, -2.0), (-1e-3, 4.0), (1e-2, 1.0)]
    for i, k in enumerate(bn_keys):
        n = state[k + ".weight"].numel()
        kept = torch.arange(n)
        if masks is not None:
            kept = kept[masks[i].reshape(n, -1).abs().sum(1).cpu() != 0]
        n_k = len(kept)        # (a masked layer may keep only a few filters: at least two stay healthy)
        pos = sorted({1, 3, n_k // 2, n_k - 2}) if n_k >= 8 else list(range(max(0, n_k - 2)))[:4]
        chans = [int(kept[j]) for j in pos]
        for c, (gv, bv) in zip(chans, vals):
            if inject_low_gamma:
                state[k + ".weight"][c], state[k + ".bias"][c] = gv, bv
        inject[k] = (chans, kept)
    gout = torch.randn(O.forward(blocks, state, x[:1], training=True).shape[1:], generator=gen).expand(4, -1, -1, -1).contiguous()
    gout = gout * (1.0 + torch.rand(4, 1, 1, 1, generator=gen))

    orig = ops.bn_act_bwd
    sig = inspect.signature(orig)
    calls = []

    def wrapped(*a, **kw):
        args = sig.bind(*a, **kw).arguments
        C, B, H, W = args["C_"], args["B"], args["H"], args["W"]
        Mfull = B * H * W
        P = Mfull if args["mode"] == L.DST_PLAIN else Mfull // 4
        Cg = 4 * C if args["mode"] == L.DST_REORG else C
        rec = dict(act=args.get("act") is not None, mode=args["mode"], B=B, H=H, W=W, C=C, slope=args["slope"],
                   yptr=args["y"].data_ptr(), S=args.get("grad_scale", 1.0),
                   y=args["y"].view(-1)[:Mfull * args["y_ld"]].view(Mfull, args["y_ld"])[:, args["y_choff"]:args["y_choff"] + C].float().cpu(),
                   g=args["g"].view(-1)[:P * args["g_ld"]].view(P, args["g_ld"])[:, args["g_choff"]:args["g_choff"] + Cg].float().cpu(),
                   scale=args["scale"][:C].cpu(), shift=args["shift"][:C].cpu(),
                   perm=None if args.get("perm") is None else args["perm"].long().cpu())
        g2 = args.get("g2")
        rec["g2"] = None if g2 is None else g2.view(-1)[:Mfull * args["g2_ld"]].view(Mfull, args["g2_ld"])[
            :, args["g2_choff"]:args["g2_choff"] + C].float().cpu()
        calls.append(rec)
        return orig(*a, **kw)
    monkeypatch.setattr(ops, "bn_act_bwd", wrapped)

    runs = {}
    for from_act in (True, False):
        m = nets.Darknet(mini)
        m.load_state_dict(state)
        m.to(dev).train()      # the default precision ("auto": split-operand training engine)
        if masks is not None:
            m.set_masks([mk.to(dev) for mk in masks])
        del calls[:]
        out = m(x.to(dev))
        eng = list(m._engines.values())[0]
        assert eng.precise and not eng.use_plan
        eng.bwd_from_act = from_act
        m.zero_grad()
        out.backward(gout.to(dev))
        lay_of = {lay.y.data_ptr(): lay for lay in eng.layers if getattr(lay, "y", None) is not None}
        bn_name = {id(mod): k for k in bn_keys for mod in [m.get_submodule(k)]}
        per_bn = {}
        for rec in calls:
            lay = lay_of.get(rec["yptr"])
            if lay is not None and lay.bn is not None:
                per_bn[bn_name[id(lay.bn)]] = rec
        grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
        runs[from_act] = (grads, per_bn, [rec["act"] for rec in calls], eng.pool_act_on)
    monkeypatch.setattr(ops, "bn_act_bwd", orig)
    return blocks, state, x, gout, masks, bn_keys, inject, runs


def _sums(rec, n_param):
    """sum|g_z xhat| and sum|g_z| per channel of one recorded launch, in parameter order (float64 reference)."""
    B, H, W, C, mode = rec["B"], rec["H"], rec["W"], rec["C"], rec["mode"]
    pos, arg, _ = _decisions(rec["y"], rec["scale"], rec["shift"], rec["slope"], B, H, W, mode, False)
    gamma = torch.ones(C, dtype=torch.float64)
    _, _, _, gz, xhat = _reference(rec["y"].double(), gamma, torch.zeros(C, dtype=torch.float64), rec["slope"], mode, pos, arg,
                                   rec["g"].double() / rec["S"], None if rec["g2"] is None else rec["g2"].double() / rec["S"],
                                   B, H, W)
    sgx, sg = (gz * xhat).abs().sum(0), gz.abs().sum(0)
    outx, out = torch.full((n_param,), float("nan"), dtype=torch.float64), torch.full((n_param,), float("nan"), dtype=torch.float64)
    idx = rec["perm"] if rec["perm"] is not None else torch.arange(C)
    outx[idx], out[idx] = sgx, sg
    return outx, out


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "filter40"])
def test_engine_low_gamma_channels_act_vs_y(dev, monkeypatch, masked):
    """The mini network in the default training precision with four channels per BatchNorm layer at gamma in
    {1e-4, 1e-3, -1e-3, 1e-2}, |beta| in [1, 4]: one forward + backward pass with the BatchNorm backward from the stored
    activation (bwd_from_act, the default) and one from the saved fp32 y.  The last BatchNorm layer sees the same incoming
    gradient in both runs: its injected channels' dgamma / dbeta agree to 1e-4.  In earlier layers the incoming gradients
    differ by the act path's usual error: there an injected channel may differ by no more than the worst healthy channel
    of its layer, each normalised by its own sum|g_z xhat| (sum|g_z| for dbeta).  Every other gradient agrees as closely
    as the act path already does; the injected channels' dgamma matches the CPU oracle within 4x the worst healthy channel
    of the layer (or 1e-3), normalised the same way (storage noise, a per-channel statistic) -- the oracle with fp16 storage for PLAIN and reorg blocks, the fp32 oracle for MaxPool
    blocks: the fp16-storage oracle pools ROUNDED activations, and at gamma 1e-4 every window of such a channel ties after
    rounding (the default precision pools the unrounded ones).  With the filter mask the PLAIN act path runs with `perm`,
    the pool act path is off."""
    from oracle import darknet_ref as O
    blocks, state, x, gout, masks, bn_keys, inject, runs = _mini_engine_ab(dev, monkeypatch, masked)
    (ga, per_a, acts_a, pool_on), (gy, per_y, acts_y, _) = runs[True], runs[False]
    assert any(acts_a) and not any(acts_y)                    # the act kernels really ran in the first run, not in the second
    assert pool_on == (not masked)
    oracle = {}
    for storage in ("fp16", None):
        st = {k: v.clone() for k, v in state.items()}
        for k in O.param_keys(blocks):
            st[k].requires_grad_(True)
        O.forward(blocks, st, x, training=True, storage=storage, masks=masks and [mk.cpu() for mk in masks]).backward(gout)
        oracle[storage] = st
    last = [k for k in bn_keys if k in per_a][-1]
    injected_idx = {}
    for k in bn_keys:
        if k not in per_a:
            continue                                           # the fused first block has its own backward kernel
        chans, kept = inject[k]
        n = ga[k + ".weight"].numel()
        injected_idx[k] = chans
        sgx, sg = _sums(per_a[k], n)
        dga, dgy = ga[k + ".weight"].double(), gy[k + ".weight"].double()
        dba, dby = ga[k + ".bias"].double(), gy[k + ".bias"].double()
        dgo = oracle[None if per_a[k]["mode"] == L.DST_POOL else "fp16"][k + ".weight"].grad.double()
        healthy = [int(c) for c in kept if int(c) not in chans]
        hg = max(float((dga[c] - dgy[c]).abs() / sgx[c].clamp_min(1e-30)) for c in healthy)
        hb = max(float((dba[c] - dby[c]).abs() / sg[c].clamp_min(1e-30)) for c in healthy)
        ho = max(float((dga[c] - dgo[c]).abs() / sgx[c].clamp_min(1e-30)) for c in healthy)
        for c in chans:
            eg, eb = float((dga[c] - dgy[c]).abs()), float((dba[c] - dby[c]).abs())
            eo = float((dga[c] - dgo[c]).abs() / sgx[c])
            print("%s ch %d gamma %.0e: act vs y dgamma %.3g (%.3g of sum|g_z xhat|; healthy worst %.3g), dbeta %.3g; "
                  "vs oracle %.3g (healthy worst %.3g)" % (k, c, float(state[k + ".weight"][c]), eg, eg / float(sgx[c]), hg,
                                                            eb, eo, ho))
            if k == last:
                assert eg <= 1e-4 * abs(float(dgy[c])), (k, c, eg, float(dgy[c]))
                assert eb <= 1e-4 * abs(float(dby[c])), (k, c, eb, float(dby[c]))
            else:
                assert eg / float(sgx[c]) <= hg, (k, c, eg / float(sgx[c]), hg)
                assert eb / float(sg[c]) <= hb, (k, c, eb / float(sg[c]), hb)
            assert eo <= max(4.0 * ho, 1e-3), (k, c, eo, ho)
    # every other gradient: as close as the act path keeps them
    worst = 0.0
    for name in ga:
        a, b = ga[name].double().clone(), gy[name].double().clone()
        k = name.rsplit(".", 1)[0]
        if k in injected_idx:
            a[injected_idx[k]] = b[injected_idx[k]] = 0.0
        e = rel_l2(a, b)
        print("  %-28s act vs y rel-L2 %.2e" % (name, e))
        worst = max(worst, e)
    print("worst other-gradient rel-L2, act vs y: %.2e" % worst)
    assert worst < OTHER_GRAD_BOUND[masked]


# the act path's worst other-gradient rel-L2 against the y path on the same network, batch and mask WITHOUT the injected
# channels (measured 1.38e-3 dense, 2.11e-3 filter40), rounded up
OTHER_GRAD_BOUND = {False: 1.4e-3, True: 2.2e-3}


# ------------------------------------------------------------------ forward: batch statistics at a large |mean| / std
@pytest.mark.parametrize("case", [(2, 32, 32, 512, 64, 1), (1, 26, 26, 384, 128, 1), (4, 48, 48, 512, 64, 1)])
def test_bn_coeffs_large_mean_over_std(dev, case):
    """bn_coeffs_kernel: var = E[y^2] - mean^2 from the fp32 per-row slab sums of the conv epilogue, which loses about
    2^-24 k (1 + r^2) relative at r = |mean| / std.  y from the real conv_fwd_raw (1x1: no zero padding, whose border
    pixels would cap r) on non-negative inputs with weights
    w = o_c + s n (n centred per filter), so that mean = o_c K / 2 and std^2 = K (o_c^2 + s^2) / 12 give r in
    {0.5, 3, 10, 30}.  mean and invstd against a float64 two-pass over the fp16 raw output of the same call: invstd
    within 1e-4 relative up to r = 10; the r = 30 figure is printed."""
    B, H, W, cin, cout, k = case
    gen = torch.Generator().manual_seed(3 + cin)
    K = cin * k * k
    ratios = torch.tensor([0.5, 3.0, 10.0, 30.0], dtype=torch.float64)[torch.arange(cout) % 4]
    t = ratios / torch.sqrt(3.0 * K - ratios ** 2)                           # o / s
    s = 1.0 / K ** 0.5
    n = torch.randn(cout, K, generator=gen, dtype=torch.float64)
    n = n - n.mean(1, keepdim=True)
    w = ((t * s)[:, None] + s * n).view(cout, cin, k, k).float()
    x = torch.rand(B, cin, H, W, generator=gen)
    from util import to_padded
    xb, ld = to_padded(x.to(dev))
    g = ops.geom(B, H, W, k, cin, cout, ld)
    wp, _ = ops.pack_weights(g, w.to(dev).contiguous())
    y = torch.zeros(B * H * W * cout, dtype=torch.float16, device=dev)
    stats = torch.zeros(ops.stats_rows(g), 2, ops.round_up(cout, 256), dtype=torch.float32, device=dev)
    ops.conv_fwd_raw(g, xb, wp, y, cout, 0, stats)
    gamma, beta = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
    rm, rv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
    scale, shift, mean, invstd = (torch.empty(cout, device=dev) for _ in range(4))
    ops.bn_coeffs(stats, cout, B * H * W, gamma, beta, rm, rv, True, scale, shift, mean, invstd)
    yd = y.view(-1, cout).double().cpu()
    mref = yd.mean(0)
    vref = ((yd - mref) ** 2).mean(0)
    iref = 1.0 / torch.sqrt(vref + EPS)
    r = mref.abs() / vref.sqrt()
    ei = (invstd.cpu().double() - iref).abs() / iref
    em = (mean.cpu().double() - mref).abs() / vref.sqrt()
    for rr in (0.5, 3.0, 10.0, 30.0):
        sel = ratios == rr
        print("%s r ~ %4.1f (measured %5.2f .. %5.2f): invstd rel err max %.2e, mean err / std max %.2e"
              % (case, rr, float(r[sel].min()), float(r[sel].max()), float(ei[sel].max()), float(em[sel].max())))
    assert float(r[ratios == 10.0].min()) > 8.0 and float(r[ratios == 30.0].min()) > 25.0     # the populations are real
    ok = ratios <= 10.0
    assert float(ei[ok].max()) < 1e-4
    assert float(em[ok].max()) < 1e-4
