"""float64 reference of the fused first block (csrc/conv_stem_block.hip): conv1 (3 -> 32, 3x3, zero halo) + BatchNorm +
LeakyReLU + MaxPool(2, 2), its batch statistics and its backward, each value with an error scale.

Everything works from the operands the kernels multiply: the fp16-rounded image and the fp16-rounded, masked weights, held
in float64.  v_m is the im2col row of output pixel m (27 values, k = c * 9 + ty * 3 + tx, zeros in the halo) and
y[m][n] = W[n] . v_m.  A SCALE is the value's own formula with every difference of like quantities replaced by the sum of
their magnitudes: what a float32 evaluation in any order loses is a small multiple of EPS32 * scale, however the terms
cancel.  Errors are counted in units of EPS32 * scale.

    forward      z = sc y + sh,  m = leaky(max of the 2x2 window);  scale: max over the window of |sc| sum_k |w_k||v_k| + |sh|
    statistics   S = sum_m v_m, C = sum_m v_m v_m^T, mean = W S / M, var = W^T C W / M - mean^2 (biased), invstd,
                 running mean / var after one update (unbiased factor M / (M - 1));
                 scale_mean = |W| sum_m |v_m| / M,  scale_var = |W|^T (sum_m |v_m||v_m|^T) |W| / M + scale_mean^2,
                 kappa = E[y^2] / (var + eps): the factor by which a relative error of the sums grows in var
    backward     teacher-forced on the saved mean / invstd / scale / shift it is given.  Winner of a window: its first
                 maximum in (row, column) order.  g_z = fp16(float32(G) * (z_win > 0 ? 1 : float32(slope))), the one fp16
                 rounding of the kernel, at the winner.  T = sum_m g_z v_m^T, dbeta = sum_m g_z,
                 dgamma = invstd (W . T - mean dbeta),
                 dW = gamma invstd (T - dbeta / M S - dgamma / M invstd (W C - mean S)) x mask;
                 scales: A = sum_m |g_z||v_m|, sum_m |g_z|, and the dgamma / dW formulas on magnitudes.
"""
import collections

import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -23
CHUNK = 256                 # images per step of the chunked passes

Pre = collections.namedtuple("Pre", "x w y ay")              # operands (float64), y = W . v (float64), sum_k |w_k||v_k| (float32)
Forward = collections.namedtuple("Forward", "m scale z_win gap")
Stats = collections.namedtuple("Stats", "M S C S_abs C_abs mean var invstd ey2 scale_mean scale_var kappa ymax")
Backward = collections.namedtuple("Backward", "dw dgamma dbeta scale_dw scale_dgamma scale_dbeta T A")


def f32(v):
    """A Python float rounded to float32 (what a float argument of the library holds)."""
    return float(torch.tensor(v, dtype=torch.float32))


def cols(x):
    """x [B, 3, H, W] float64 -> im2col rows [B, H * W, 27], k = c * 9 + ty * 3 + tx."""
    return F.unfold(x, 3, padding=1).transpose(1, 2)


def conv(x, w):
    """(y, ay) [B, H, W, 32]: W . v and sum_k |w_k||v_k| in float64."""
    B, _, H, W = x.shape
    v = cols(x)
    wm = w.reshape(w.shape[0], 27).t()
    return (v @ wm).view(B, H, W, -1), (v.abs() @ wm.abs()).view(B, H, W, -1)


def pre(x, w):
    """The convolution of the fp16-valued float64 operands x [B, 3, H, W] and w [n, 3, 3, 3], computed once per input."""
    ys, ays = [], []
    for b0 in range(0, x.shape[0], CHUNK):
        y, ay = conv(x[b0:b0 + CHUNK], w)
        ys.append(y), ays.append(ay.float())
    return Pre(x, w, torch.cat(ys), torch.cat(ays))


def windows(t):
    """[B, H, W, C] -> [B, H/2, W/2, C, 4] in (row, column) order: (0, 0), (0, 1), (1, 0), (1, 1)."""
    B, H, W, C = t.shape
    return t.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)


def forward(p, sc, sh, slope):
    """Pooled output m [B, n, H/2, W/2] with its scale, the window maximum z_win of the pre-activation and its gap to the
    runner-up (0: an exact tie).  p: pre(x, w); sc, sh float64 [n]; chunked over images."""
    outs = [[], [], [], []]
    for b0 in range(0, p.y.shape[0], CHUNK):
        zw = windows(p.y[b0:b0 + CHUNK] * sc + sh)
        sw = windows(p.ay[b0:b0 + CHUNK].double() * sc.abs() + sh.abs())
        top = zw.topk(2, dim=-1).values
        zwin = top[..., 0]
        m = torch.where(zwin > 0, zwin, zwin * slope)
        for o, t in zip(outs, (m, sw.max(-1).values, zwin, top[..., 0] - top[..., 1])):
            o.append(t.permute(0, 3, 1, 2))
    return Forward(*(torch.cat(o).contiguous() for o in outs))


def stats(x, w, eps=1e-5):
    """Batch statistics of y = W v over all pixels, from S and C as the kernel forms them, in float64."""
    S = torch.zeros(27, dtype=torch.float64)
    C = torch.zeros(27, 27, dtype=torch.float64)
    S_abs, C_abs = S.clone(), C.clone()
    ymax = torch.zeros(w.shape[0], dtype=torch.float64)
    wm = w.reshape(w.shape[0], 27)
    for b0 in range(0, x.shape[0], CHUNK):
        v = cols(x[b0:b0 + CHUNK]).reshape(-1, 27)
        S += v.sum(0)
        C += v.t() @ v
        S_abs += v.abs().sum(0)
        C_abs += v.abs().t() @ v.abs()
        ymax = torch.maximum(ymax, (v @ wm.t()).abs().max(0).values)
    M = float(x.shape[0] * x.shape[2] * x.shape[3])
    mean = wm @ S / M
    ey2 = ((wm @ C) * wm).sum(1) / M
    var = (ey2 - mean * mean).clamp_min(0.0)
    e = f32(eps)
    scale_mean = wm.abs() @ S_abs / M
    scale_var = ((wm.abs() @ C_abs) * wm.abs()).sum(1) / M + scale_mean * scale_mean
    return Stats(M, S, C, S_abs, C_abs, mean, var, 1.0 / torch.sqrt(var + e), ey2, scale_mean, scale_var, ey2 / (var + e), ymax)


def stats_of(y, ay, eps=1e-5):
    """The same statistics from a given y and sum_k |w_k||v_k| ([B, H, W, n] each): sum_m (sum_k |w_k||v_k|)^2 is
    |W|^T (sum_m |v_m||v_m|^T) |W|.  For products that are not one W . v (split operands); S and C are not formed."""
    n = y.shape[-1]
    y, ay = y.reshape(-1, n), ay.reshape(-1, n).double()
    M = float(y.shape[0])
    mean, ey2 = y.sum(0) / M, (y * y).sum(0) / M
    var = (ey2 - mean * mean).clamp_min(0.0)
    e = f32(eps)
    scale_mean = ay.sum(0) / M
    return Stats(M, None, None, None, None, mean, var, 1.0 / torch.sqrt(var + e), ey2, scale_mean,
                 (ay * ay).sum(0) / M + scale_mean * scale_mean, ey2 / (var + e), y.abs().max(0).values)


def split(t):
    """(hi, lo) of a float32 tensor as the split-operand block holds it: fp16(t) and fp16(t - fp16(t)), in float64."""
    hi = t.half().float()
    return hi.double(), (t - hi).half().double()


def split_product(x, w):
    """(y, ay) of the three products the split-operand kernels accumulate, x_hi w_hi + x_lo w_hi + x_hi w_lo, in float64
    from float32 x [B, 3, H, W] and w [n, 3, 3, 3] (x_lo w_lo is dropped)."""
    (xh, xl), (wh, wl) = split(x), split(w)
    parts = [conv(a, b) for a, b in ((xh, wh), (xl, wh), (xh, wl))]
    return sum(p[0] for p in parts), sum(p[1] for p in parts)


def running(st, rmean0, rvar0, momentum):
    """(running mean, running var, their scales) after one update; momentum as the library holds it (float32)."""
    mo = f32(momentum)
    unb = st.M / (st.M - 1.0) if st.M > 1 else 1.0
    rm = (1.0 - mo) * rmean0 + mo * st.mean
    rv = (1.0 - mo) * rvar0 + mo * st.var * unb
    return rm, rv, (1.0 - mo) * rmean0.abs() + mo * st.scale_mean, (1.0 - mo) * rvar0.abs() + mo * st.scale_var * unb


def coeffs(st, gamma, beta):
    sc = gamma * st.invstd
    return sc, beta - st.mean * sc


def routed(y, sc, sh, slope, G, round_gz=True):
    """g_z [B, H, W, n] float64: G * leaky'(z_win) at the first maximum of every window, 0 elsewhere.  y [B, H, W, n];
    G [B, n, H/2, W/2] holds fp16 values."""
    B, H, W, _ = y.shape
    zw = windows(y * sc + sh)                                   # [B, H2, W2, C, 4]
    zwin = zw.max(-1).values
    first = (zw == zwin.unsqueeze(-1)).to(torch.uint8).argmax(-1)          # argmax of a 0 / 1 tensor: the first 1
    fac = torch.where(zwin > 0, torch.ones((), dtype=torch.float32), torch.tensor(slope, dtype=torch.float32))
    gz = G.permute(0, 2, 3, 1).float() * fac                    # one float32 product, as the kernel's
    gz = (gz.half() if round_gz else gz).double()
    onehot = F.one_hot(first, 4).to(torch.float64) * gz.unsqueeze(-1)      # [B, H2, W2, C, 4]
    C_ = onehot.shape[3]
    return onehot.view(B, H // 2, W // 2, C_, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, H, W, C_)


def backward(p, gamma, mean, invstd, sc, sh, slope, G, st, mask=None, round_gz=True, f32_sums=False):
    """dW [n, 3, 3, 3], dgamma, dbeta of sum(G * out) with their scales; G is the gradient the kernel is handed (fp16
    values; a grad_scale is divided out of the results by the caller).  p: pre(x, w), st: stats(x, w).  Chunked.
    f32_sums: the float32 restatement -- T and sum g_z accumulated by chained_f32, the rest in float64 as the kernel's."""
    x, w = p.x, p.w
    n = w.shape[0]
    wm = w.reshape(n, 27)
    T = torch.zeros(n, 27, dtype=torch.float64)
    A = T.clone()
    db = torch.zeros(n, dtype=torch.float64)
    dba = db.clone()
    keep = []
    for b0 in range(0, x.shape[0], CHUNK):
        gz = routed(p.y[b0:b0 + CHUNK], sc, sh, slope, G[b0:b0 + CHUNK], round_gz).reshape(-1, n)
        v = cols(x[b0:b0 + CHUNK]).reshape(-1, 27)
        T += gz.t() @ v
        A += gz.abs().t() @ v.abs()
        db += gz.sum(0)
        dba += gz.abs().sum(0)
        if f32_sums:
            keep.append((gz.float(), v.float()))
    if f32_sums:
        gz, v = torch.cat([k[0] for k in keep]), torch.cat([k[1] for k in keep])
        T, db = chained_f32(gz, v), chained_f32(gz, torch.ones(gz.shape[0], 1)).view(n)
    M = st.M
    dg = invstd * ((wm * T).sum(1) - mean * db)
    dg_s = invstd * ((wm.abs() * A).sum(1) + mean.abs() * dba)
    WC, WC_abs = wm @ st.C, wm.abs() @ st.C_abs
    gi = (gamma * invstd).unsqueeze(1)
    dw = gi * (T - db.unsqueeze(1) / M * st.S - (dg * invstd).unsqueeze(1) / M * (WC - mean.unsqueeze(1) * st.S))
    dw_s = gi.abs() * (A + dba.unsqueeze(1) / M * st.S_abs
                       + (dg_s * invstd).unsqueeze(1) / M * (WC_abs + mean.abs().unsqueeze(1) * st.S_abs))
    dw, dw_s = dw.view(n, 3, 3, 3), dw_s.view(n, 3, 3, 3)
    if mask is not None:
        dw, dw_s = dw * mask, dw_s * mask
    return Backward(dw, dg, db, dw_s, dg_s, dba, T, A)


def excluded(fw, tau):
    """Pooled pixels a float32 evaluation may route or activate differently from float64: |z_win| < tau, or a runner-up
    within (0, tau) of the maximum.  Exact ties (gap == 0) stay in: both sides must take the first maximum."""
    return (fw.z_win.abs() < tau) | ((fw.gap > 0) & (fw.gap < tau))


def half_ulp16(v):
    """Half the fp16 spacing at |v| (float64 tensor): 2^(floor(log2 |v|) - 11), the subnormal spacing 2^-24 below 2^-14."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 11.0)


# ---------------------------------------------------------------------------------------------------------------------
# float32 restatements: what a straightforward float32 evaluation on the CPU loses against the reference (the yardsticks)

CHAIN = 128                 # 32-pixel steps of one sequential float32 accumulation chain (a wave's accumulators)


def chained_f32(a, b):
    """sum_m a[m]^T b[m] ([M, p], [M, q] float32 -> [p, q] float64): products and sums in float32 in sequential chains of
    CHAIN steps of 32 rows, the chains summed in float64 -- the kernels' documented arithmetic (fp32 MFMA accumulators
    per wave, slabs combined in double)."""
    M = a.shape[0]
    pad = (-M) % (32 * CHAIN)
    if pad:
        a = torch.cat((a, a.new_zeros(pad, a.shape[1])))
        b = torch.cat((b, b.new_zeros(pad, b.shape[1])))
    a, b = a.view(-1, CHAIN, 32, a.shape[1]), b.view(-1, CHAIN, 32, b.shape[1])
    acc = torch.zeros(a.shape[0], a.shape[3], b.shape[3], dtype=torch.float32)
    for s in range(CHAIN):
        for r in range(32):             # one product and one add per row: no wider intermediate anywhere
            acc = acc + a[:, s, r, :, None] * b[:, s, r, None, :]
    return acc.double().sum(0)


def stats_f32(x, w, eps=1e-5):
    """(mean, var) from S and C accumulated by chained_f32, finished in float64 as stem_coeffs_kernel does."""
    v = torch.cat([cols(x[b0:b0 + CHUNK]).reshape(-1, 27) for b0 in range(0, x.shape[0], CHUNK)]).float()
    C = chained_f32(v, v)
    S = chained_f32(v, torch.ones(v.shape[0], 1)).view(27)
    wm = w.reshape(w.shape[0], 27)
    M = float(v.shape[0])
    mean = wm @ S / M
    return mean, (((wm @ C) * wm).sum(1) / M - mean * mean).clamp_min(0.0)


def forward_f32(x, w, sc, sh):
    """z [B, H, W, 32] of F.conv2d and one fused multiply-add in float32."""
    y = F.conv2d(x.float(), w.float(), None, 1, 1).permute(0, 2, 3, 1)
    return (y.double() * sc.float().double() + sh.float().double()).float().double()       # an exact product, one rounding
