"""The cases of tests/test_grad_saturation_gpu.py (BatchNorm backward) and their float64 proofs in
tests/test_saturation_cases_cpu.py.  Test-side only, no GPU needed.

A case is one dispatch target of mcamd_bn_act_bwd (a row of test_bn_conditioning_gpu.VARIANTS) at one shape, with that
file's random channels -- except four:

  PPOS     scale = gamma invstd = 4; its g is zero but for ONE element of value G0, planted on the positive LeakyReLU side
  PNEG     scale = -64; the same on the negative side, so the stored value is G0 kappa with kappa < 0 through g * slope
  PRUNED   dy_keep 0, scale 64, g = 65504 at several pixels: its dY is exactly 0 and never raises the flag
  PMEAN    used by the "mean" and "nonarg" kinds only (below); otherwise random like the rest

With one non-zero g_z at element p of a channel of N elements, dY = dm (g_z - c1 - xhat c2) gives
    dY[p] = G0 kappa,   kappa = dm s (1 - 1/N - xhat_p^2 / N)          (s = 1 or the slope)
    dY[j] = -G0 dm s (1 + xhat_j xhat_p) / N                            (every other element)
so G0 = 0.97 x 65504 / |kappa| stays below the clamp and 1.03 x 65504 / |kappa| goes beyond it, in that element alone.
kappa is read off the float64 reference (_reference of test_bn_conditioning_gpu) run on the kernel's own inputs.

kinds:
  "plant"   the above, at the first, a middle and the last item (for MaxPool / reorg: window element k = 0, 2, 3);
            variants with a second gradient plant once in g and once in g2 (MaxPool: at a NON-argmax element)
  "mean"    PMEAN has scale 64 and g = MEAN_G at every (pooled) pixel: whole channel beyond the clamp through the mean terms
  "nonarg"  MaxPool without g2: PMEAN's y is -1 at element 0 of every window (the argmax under scale -4), about 1/3
            elsewhere and +10 at ONE non-argmax element j; with g constant, dY[j] = -dm (c1 + xhat_j c2) is an order of
            magnitude beyond every other element of the channel, so j alone crosses the clamp."""
import torch

from modelcompression_amd import _lib as L
import test_bn_conditioning_gpu as BC
from test_bn_conditioning_gpu import VARIANTS, _channels, _decisions, _reference, _win, EPS, S, T

F16_MAX = 65504.0
PPOS, PNEG, PRUNED, PMEAN = 3, 12, BC.PRUNED, 25
SCALE = {PPOS: 4.0, PNEG: -64.0, PRUNED: 64.0}
MEAN_SCALE, MEAN_G = 64.0, 16384.0
NONARG_SCALE = -4.0
BELOW, ABOVE = 0.97, 1.03

# name -> (C, (B, H, W), environment).  c64-blocks3: 3 workgroups, five trips of the grid-stride loop over the 3840 items of
# a PLAIN block; c256: 32 threads share a pixel
SHAPES = {
    "c64": (64, (2, 20, 12), {}),
    "c64-blocks3": (64, (2, 20, 12), {"MCAMD_BN_BWD_BLOCKS": "3"}),
    "c256": (256, (2, 4, 6), {}),
}
POSITIONS = ("first", "middle", "last")
WINDOW_K = {"first": 0, "middle": 2, "last": 3}          # the planted element of a 2x2 window, k = 2 dh + dw

# one variant per route family for the "mean" kind (slope 0.1: with slope 1 a constant g has no gradient at all)
MEAN_VARIANTS = ("plain-y16", "pool-y16", "pool-y16-g2", "reorg-y16", "plain-generic-y16", "pool-generic-y16")
NONARG_VARIANTS = ("pool-y16", "pool-y32", "pool-act", "pool-generic-y16")

VARIANT = {v[0]: v for v in VARIANTS}


def sources(variant):
    """Where a "plant" case puts G0: in g, and for a variant with a second gradient also (separately) in g2."""
    return ("g", "g2") if variant[4] else ("g",)


def plant_cases():
    return [(v[0], s, p) for v in VARIANTS for s in SHAPES for p in POSITIONS]


def f16(v):
    """The fp16 number nearest v, as a float."""
    return float(torch.tensor(v, dtype=torch.float64).half())


class Case:
    pass


def build(vname, shape, position="first", kind="plant"):
    """The host side of one case: what the kernel reads (fp16 / fp32 values as float tensors) and where G0 goes."""
    variant = VARIANT[vname]
    name, mode, ybits, act_pad, dual, env, slope = variant
    C, (B, H, W), shape_env = SHAPES[shape]
    M, Mq = B * H * W, B * H * W // 4
    c = Case()
    c.variant, c.name, c.mode, c.ybits, c.act_pad, c.dual, c.slope = variant, name, mode, ybits, act_pad, dual, slope
    c.env = dict(env, **shape_env)
    c.B, c.H, c.W, c.C, c.M, c.kind, c.position = B, H, W, C, M, kind, position
    c.P = M if mode == L.DST_PLAIN else Mq                                   # rows of g
    gen = torch.Generator().manual_seed(977 + 13 * [v[0] for v in VARIANTS].index(name) + C + len(kind))
    gamma, beta, mean_t, std_t, alpha, offset = _channels(C, gen)
    y64 = mean_t + std_t * torch.randn(M, C, generator=gen, dtype=torch.float64)
    widx = _win(torch.arange(M).view(B, H, W, 1), B, H, W).reshape(Mq, 4)    # pooled pixel, k -> full-resolution pixel

    def at(ch, xh):                                                          # a y value at about xhat = xh
        return mean_t[ch] + xh * std_t[ch]

    # ---- where the plants go, and the y values that fix their LeakyReLU side and window position
    c.plants = {}
    if kind == "plant":
        row = {"first": 0, "middle": c.P // 2 + 1, "last": c.P - 1}[position]
        k = 0 if mode == L.DST_PLAIN else WINDOW_K[position]
        p = row if mode == L.DST_PLAIN else int(widx[row, k])
        k2 = (k + 1) % 4
        p2 = p if mode != L.DST_POOL else int(widx[row, k2])
        if mode == L.DST_POOL:
            # PPOS (scale > 0): argmax at xhat ~ 1, the g2 element at 0.6, both on the positive side, the rest below;
            # PNEG (scale < 0): argmax at the LOWEST xhat, every element on the negative side
            rest = [kk for kk in range(4) if kk not in (k, k2)]
            for ch, vals in ((PPOS, (1.0, 0.6, -0.5, -1.0)), (PNEG, (0.5, 1.0, 1.5, 2.0))):
                for kk, xh in zip([k, k2] + rest, vals):
                    y64[widx[row, kk], ch] = at(ch, xh)
        else:
            for ch in (PPOS, PNEG):
                y64[p, ch] = at(ch, 1.0)
        for src in sources(variant):
            c.plants[src] = {}
            for ch in (PPOS, PNEG):
                if src == "g":
                    col = k * C + ch if mode == L.DST_REORG else ch
                    c.plants[src][ch] = dict(row=row, col=col, p=p, k=k, positive=ch == PPOS)
                else:
                    c.plants[src][ch] = dict(row=p2, col=ch, p=p2, k=k2, positive=ch == PPOS)
    elif kind == "nonarg":
        assert mode == L.DST_POOL and not dual
        row = Mq // 2 + 1
        c.nonarg_p = int(widx[row, 2])
        col = 1.0 / 3.0 + 0.05 * torch.randn(M, generator=gen, dtype=torch.float64)
        col[widx[:, 0]] = -1.0
        col[c.nonarg_p] = 10.0
        y64[:, PMEAN] = col
    else:
        assert kind == "mean"

    # ---- what the kernel reads, as in test_bn_conditioning_gpu
    c.yk = y64.half().float() if ybits == 16 else y64.float()
    ykd = c.yk.double()
    mean = ykd.mean(0)
    c.invstd = 1.0 / torch.sqrt(ykd.var(0, unbiased=False) + EPS)
    for ch, sc in SCALE.items():
        gamma[ch], beta[ch] = sc / c.invstd[ch], 0.0
    if kind != "plant":
        gamma[PMEAN], beta[PMEAN] = (MEAN_SCALE if kind == "mean" else NONARG_SCALE) / c.invstd[PMEAN], 0.0
    c.gamma, c.beta = gamma, beta
    c.scale = (gamma * c.invstd).float()
    c.shift = (beta - mean * c.scale.double()).float()
    c.mean32, c.invstd32 = mean.float(), c.invstd.float()
    c.keep = torch.ones(C)
    c.keep[PRUNED] = 0.0
    c.compact = C == 64
    c.y_ld, c.y_choff = (C + 64, 32) if c.compact else (C, 0)
    c.perm = torch.randperm(C, generator=gen).to(torch.int32) if c.compact else None
    c.ill = gamma.abs() < T * beta.abs().clamp_min(1.0)
    xh = (ykd - mean) * c.invstd
    if mode == L.DST_PLAIN:
        gsig = xh
    elif mode == L.DST_POOL:
        gsig = _win(xh.view(B, H, W, C), B, H, W).amax(3).reshape(-1, C)
    else:
        gsig = _win(xh.view(B, H, W, C), B, H, W).reshape(-1, 4, C)
    noise = torch.randn(gsig.shape, generator=gen, dtype=torch.float64)
    gq = ((alpha * gsig + noise + offset) * S).half().reshape(c.P, -1, C)          # [P, 1 or 4, C], fp16 as the kernels read it
    g2q = ((alpha * xh + torch.randn(M, C, generator=gen, dtype=torch.float64)) * S).half() if dual else None
    rows = sorted({0, 1, c.P // 2, c.P - 1})
    gq[:, :, [PPOS, PNEG]] = 0
    gq[:, :, PRUNED] = 0
    gq[rows, :, PRUNED] = F16_MAX
    if dual:
        g2q[:, [PPOS, PNEG]] = 0
        g2q[[0, M // 3, M - 1], PRUNED] = F16_MAX
    if kind != "plant":
        gq[:, :, PMEAN] = 0
        if dual:
            g2q[:, PMEAN] = 0
    c.gq, c.g2q = gq.reshape(c.P, -1), g2q
    return c


def with_g(c, src=None, values=None, channel_g=None):
    """(g, g2) of a run: the base tensors with `values` {channel: G0} planted at the case's positions of source `src`, or with
    PMEAN's g set to the constant `channel_g` (kinds "mean" and "nonarg")."""
    gq, g2q = c.gq.clone(), None if c.g2q is None else c.g2q.clone()
    for ch, v in (values or {}).items():
        pl = c.plants[src][ch]
        assert f16(v) == v
        (gq if src == "g" else g2q)[pl["row"], pl["col"]] = v
    if channel_g is not None:
        assert f16(channel_g) == channel_g
        gq.view(c.P, -1, c.C)[:, :, PMEAN] = channel_g
    return gq, g2q


def decisions(c, stored=None):
    """The kernel's LeakyReLU sides [M, C] and pooled elements: from the fp32 z of the y kernels, or -- the act kernels --
    from the activation the forward pass `stored` ([M, C] fp32 of the fp16 copy; without it the y kernels' rule stands in,
    which agrees wherever the stored value did not round to zero)."""
    pos, arg, _ = _decisions(c.yk, c.scale, c.shift, c.slope, c.B, c.H, c.W, c.mode, c.ybits == 16)
    if stored is not None:
        pos = stored > 0
        if c.mode == L.DST_POOL:
            sarg = _win(stored.view(c.B, c.H, c.W, c.C), c.B, c.H, c.W).argmax(3, keepdim=True)
            assert torch.equal(sarg, arg), "stored copy: the pooled element is not the strict maximum"
    return pos, arg


def reference(c, gq, g2q, dec):
    """_reference on the run's inputs; (dY / S, dgamma, dbeta, g_z, xhat) as test_bn_conditioning_gpu._check takes them."""
    pos, arg = dec
    return _reference(c.yk.double(), c.gamma, c.beta, c.slope, c.mode, pos, arg, gq.double() / S,
                      None if g2q is None else g2q.double() / S, c.B, c.H, c.W)


def kappas(c, src, dec):
    """kappa of PPOS and PNEG for source `src`: the reference's stored dY at the planted element per unit of G0."""
    gq, g2q = with_g(c, src, {PPOS: 1.0, PNEG: 1.0})
    dy = reference(c, gq, g2q, dec)[0] * S
    return {ch: float(dy[c.plants[src][ch]["p"], ch]) for ch in (PPOS, PNEG)}


def g0(kappa, factor):
    """The fp16 G0 that puts the planted element at factor x 65504."""
    return f16(factor * F16_MAX / abs(kappa))


def kappa_channel(c, dec, p):
    """kinds "mean" / "nonarg": the reference's stored dY[p, PMEAN] per unit of the constant g."""
    gq, g2q = with_g(c, channel_g=1.0)
    return float(reference(c, gq, g2q, dec)[0][p, PMEAN] * S)
