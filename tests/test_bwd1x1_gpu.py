"""The one-launch backward of the narrow dense 1x1 blocks (mcamd_conv_bwd1x1, csrc/conv_bwd1x1.hip): input gradient G, the
BatchNorm-backward sums of the block that produced the input, and the weight gradient from one pass over dY and x.

a. Exact, per instance, against a float64 reference.  dY holds small integers, x positive multiples of 1/8, every filter has
   three +-1 weights at columns that are no symmetric function of the filter (5 n + 2, 7 n + 3, 11 n + 5 mod cin), the
   producer's BatchNorm is the identity (mean 0, invstd 1, gamma 1, beta 0: xhat = x).  Every fp32 partial sum is then an
   exact number whatever the order, so G, dW (x mask / grad_scale, a power of two) and the two sums must equal the float64
   evaluation bit for bit.  Shapes: 25 pixels (less than a tile: most workgroups have none and write zeros), ragged last
   tiles with an odd width, and the smallest B x 64 x 64 with more tiles than workgroups; both pad forms; G and x at a
   channel offset of a wider row; with and without a mask.  The G buffer keeps its sentinel outside its slice, the NaN-filled
   slabs are fully overwritten, two runs give the same bits.
b. A G beyond 65504 saturates and raises the flag exactly as ops.conv_dgrad_raw does on the same inputs.
c. Random data with both LeakyReLU sides and ill-conditioned channels (the fp32 y fallback): per channel the fused sums'
   deviation from float64 within the bound of tests/test_dgrad_bn_sums_gpu.py (twice the two-pass kernels' + 4 x 2^-24); G
   bit-equal to conv_dgrad_raw, dW within fp32 summation-order room of conv_wgrad.
d. The engine with MCAMD_BWD1X1 1 against 0, default precision, on a 3x3 -> 1x1 -> 3x3 chain at both instance shapes and
   on YOLOv2 at B = 2: logits and running statistics bit-equal, every parameter gradient against the float64 oracle -- the
   one-launch route's distance may exceed the two-launch route's by at most 10 %."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, ops, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd import _lib as L  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402

SLOPE = 0.1
T = 2.0 ** -5            # BN_ACT_T of csrc/common.h
EPS24 = 2.0 ** -24
SLAB_ROWS = 1024         # rows of the two-pass slab in front of the coefficients in mcamd_bn_act_bwd's workspace
INSTANCES = {(64, 128): 128, (128, 256): 64}      # (cout, cin) -> pixels per tile (BWD1X1_INSTANCES, csrc/conv_bwd1x1.hip)
SENTINEL = 777.0


class Problem:
    """One 1x1 block: dY [B, H, W, cout], x [B, H, W, cin] at channel `x_choff` of an `x_ld`-wide padded buffer (either
    form), G at `g_choff` of a `g_ld`-wide raw buffer; the producer owns the G columns [ch_lo, ch_lo + C)."""

    def __init__(self, dev, B, H, W, cout, cin, w, gy, x, pad=0, x_extra=0, g_extra=0, C=None, ch_lo=0, coef=None, y=None):
        self.dev, self.B, self.H, self.W, self.cout, self.cin, self.pad = dev, B, H, W, cout, cin, pad
        self.M = B * H * W
        self.x_ld, self.x_choff = cin + 2 * x_extra, x_extra
        self.g_ld, self.g_choff = cin + 2 * g_extra, g_extra
        self.g = ops.geom(B, H, W, 1, cin, cout, self.x_ld, self.x_choff, pad=pad)
        _, self.wd = ops.pack_weights(self.g, w.contiguous(), want_fwd=False)
        self.dyb = ops.alloc_padded(B, H, W, cout, dev, pad=pad)
        ops.padded_view(self.dyb, B, H, W, cout, pad=pad)[:, 1:-1, 1:-1, :] = gy.half()
        self.xb = ops.alloc_padded(B, H, W, self.x_ld, dev, pad=pad)
        ops.padded_view(self.xb, B, H, W, self.x_ld, pad=pad)[:, 1:-1, 1:-1, self.x_choff:self.x_choff + cin] = x.half()
        self.C, self.ch_lo = (cin if C is None else C), ch_lo
        ones, zeros = torch.ones(self.C), torch.zeros(self.C)
        self.coef = [t.float().contiguous().to(dev) for t in (coef or (ones, zeros, zeros, ones))]
        self.y = y
        self.overflow = torch.zeros(1, dtype=torch.int32, device=dev)

    def fused(self, mask=None, grad_scale=1.0, sums=True):
        """(G buffer [M, g_ld], sums slab or None, dW, workspace as fp32)"""
        gbuf = torch.full((self.M * self.g_ld,), SENTINEL, dtype=torch.float16, device=self.dev)
        ws = torch.full((ops.conv_bwd1x1_workspace_bytes(self.g) // 4,), float("nan"), device=self.dev)
        dw = torch.full((self.cout, self.cin, 1, 1), float("nan"), device=self.dev)
        slab = desc = None
        if sums:
            slab = torch.full((ops.conv_bwd1x1_sums_rows(self.g), 2, self.C + 8), float("nan"), device=self.dev)      # ld > C
            desc = ops.dgrad_sums(slab, self.xb, self.x_ld, self.x_choff + self.ch_lo, self.pad, *self.coef, SLOPE, self.C,
                                  ch_lo=self.ch_lo, y=self.y, y_ld=self.C, y_choff=0)
        self.overflow.zero_()
        ops.conv_bwd1x1(self.g, self.xb, self.dyb, self.cout, 0, self.wd, gbuf, self.g_ld, self.g_choff, dw, mask=mask,
                        grad_scale=grad_scale, workspace=ws.view(torch.uint8), overflow=self.overflow, sums=desc)
        torch.cuda.synchronize()
        return gbuf.view(self.M, self.g_ld), slab, dw, ws

    def two_launch(self, mask=None, grad_scale=1.0):
        """(G buffer, dW) of conv_dgrad_raw + conv_wgrad on the same inputs"""
        gbuf = torch.full((self.M * self.g_ld,), SENTINEL, dtype=torch.float16, device=self.dev)
        dw = torch.full((self.cout, self.cin, 1, 1), float("nan"), device=self.dev)
        self.overflow.zero_()
        ops.conv_dgrad_raw(self.g, self.dyb, self.cout, 0, self.wd, gbuf, self.g_ld, self.g_choff, overflow=self.overflow)
        ops.conv_wgrad(self.g, self.xb, self.dyb, self.cout, 0, dw, mask=mask, grad_scale=grad_scale)
        torch.cuda.synchronize()
        return gbuf.view(self.M, self.g_ld), dw

    def bn_bwd(self, gbuf, slab):
        """(dY [M, C] fp16, dgamma, dbeta, coefficients [2, C]) of the producer from G -- two passes, or from `slab`"""
        C_ = self.C
        ws = torch.zeros(ops.bn_act_bwd_workspace_bytes(C_), dtype=torch.uint8, device=self.dev)
        dy = ops.alloc_padded(self.B, self.H, self.W, C_, self.dev)
        dgm, dbt = (torch.full((C_,), float("nan"), device=self.dev) for _ in range(2))
        sc, sh, mu, ist = self.coef
        ops.bn_act_bwd(self.B, self.H, self.W, C_, self.y, C_, 0, sc, sh, mu, ist, SLOPE, L.DST_PLAIN, gbuf.view(-1), self.g_ld,
                       self.g_choff + self.ch_lo, dy, C_, 0, dgm, dbt, grad_scale=1.0, workspace=ws, act=self.xb, act_ld=self.x_ld,
                       act_choff=self.x_choff + self.ch_lo, act_pad=self.pad, sums=slab)
        torch.cuda.synchronize()
        coef = ws.view(torch.float32)[SLAB_ROWS * 2 * C_: SLAB_ROWS * 2 * C_ + 2 * C_].view(2, C_).clone()
        dyv = ops.padded_view(dy, self.B, self.H, self.W, C_)[:, 1:-1, 1:-1].reshape(self.M, C_)
        return dyv, dgm, dbt, coef


def _weights(cout, cin, gen, dev):
    w = torch.zeros(cout, cin, device=dev)
    n = torch.arange(cout, device=dev)
    for mul, add in ((5, 2), (7, 3), (11, 5)):
        sign = torch.randint(0, 2, (cout,), generator=gen, device=dev).float() * 2 - 1
        w[n, (mul * n + add) % cin] += sign
    return w.view(cout, cin, 1, 1)


def _grid(cout, cin):
    return ops.conv_bwd1x1_sums_rows(ops.geom(1, 8, 8, 1, cin, cout, cin))


def _exact_cases():
    cases = []
    for (cout, cin), P in INSTANCES.items():
        # (name, B, H, W, pad, x_extra, g_extra, mask, grad_scale, producer C, ch_lo, value bound)
        cases += [("%dx%d-25px" % (cout, cin), cout, cin, 1, 5, 5, 0, 0, 0, False, 4.0, None, 0, 4),
                  ("%dx%d-12x12-pad1-off" % (cout, cin), cout, cin, 2, 12, 12, 1, 16, 24, True, 0.5, cin // 2, 24, 4),
                  ("%dx%d-13x11-off" % (cout, cin), cout, cin, 3, 13, 11, 0, 8, 0, True, 8.0, None, 0, 4),
                  ("%dx%d-13x11-pad1" % (cout, cin), cout, cin, 3, 13, 11, 1, 0, 40, False, 2.0, 64, 8, 4),
                  ("%dx%d-loop" % (cout, cin), cout, cin, "loop", 64, 64, 1, 0, 0, False, 16.0, None, 0, 2)]
    return cases


EXACT = _exact_cases()


@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_bwd1x1_exact(dev, case):
    name, cout, cin, B, H, W, pad, x_extra, g_extra, masked, grad_scale, C_, ch_lo, vmax = case
    P = INSTANCES[(cout, cin)]
    grid = _grid(cout, cin)
    if B == "loop":                      # the smallest B x 64 x 64 with more tiles than workgroups
        B = grid * P // (H * W) + 1
        assert -(-B * H * W // P) > grid >= -(-(B - 1) * H * W // P)
    C_ = cin if C_ is None else C_
    M = B * H * W
    gen = torch.Generator(device=dev).manual_seed(11 + M + cin)
    gy = torch.randint(-vmax, vmax + 1, (B, H, W, cout), generator=gen, device=dev).float()
    x = torch.randint(1, 8 * vmax + 1, (B, H, W, cin), generator=gen, device=dev).float() / 8.0
    w = _weights(cout, cin, gen, dev)
    mask = (torch.rand(cout, cin, 1, 1, generator=gen, device=dev) < 0.7).float() if masked else None
    p = Problem(dev, B, H, W, cout, cin, w, gy, x, pad=pad, x_extra=x_extra, g_extra=g_extra, C=C_, ch_lo=ch_lo)
    gbuf, slab, dw, ws = p.fused(mask=mask, grad_scale=grad_scale)
    tiles = -(-M // P)
    print("%s: M %d, %d tiles of %d pixels on %d workgroups" % (name, M, tiles, P, grid))
    assert slab.shape[0] == grid and ops.conv_bwd1x1_wgrad_splits(p.g) == grid

    # ---- float64 reference
    gy64, x64, w64 = gy.view(M, cout).double(), x.view(M, cin).double(), w.view(cout, cin).double()
    G_ref = gy64 @ w64
    dw_ref = gy64.t() @ x64
    assert float(G_ref.abs().max()) <= 2048 and float((gy64.abs().t() @ x64).max()) * 8 < 2 ** 24
    if mask is not None:
        dw_ref = dw_ref * mask.view(cout, cin).double()
    dw_ref = dw_ref / grad_scale

    # ---- G: exact inside its slice, sentinel outside, no flag
    assert torch.equal(gbuf[:, p.g_choff:p.g_choff + cin].double(), G_ref), name
    outside = torch.cat((gbuf[:, :p.g_choff], gbuf[:, p.g_choff + cin:]), 1)
    assert bool((outside == SENTINEL).all())
    assert int(p.overflow.item()) == 0
    # ---- dW: exact; every split of the workspace written, the splits of workgroups without a tile are zeros
    assert torch.equal(dw.view(cout, cin).double(), dw_ref), name
    splits = ws.view(grid, cout, cin)
    assert bool(torch.isfinite(splits).all())
    idle = [i for i in range(grid) if (i * tiles) // grid == ((i + 1) * tiles) // grid]
    assert len(idle) == max(grid - tiles, 0)
    if idle:
        assert not bool(splits[idle].any()) and not bool(slab[idle][:, :, :C_].any())
    # ---- sums: every row and every producer channel written, nothing behind them; exact totals
    assert bool(torch.isfinite(slab[:, :, :C_]).all()) and bool(torch.isnan(slab[:, :, C_:]).all())
    Gd = gbuf[:, p.g_choff + ch_lo:p.g_choff + ch_lo + C_].double()
    ad = x64[:, ch_lo:ch_lo + C_]
    s_b, s_g = Gd.sum(0), (Gd * ad).sum(0)
    assert float((Gd * ad).abs().sum(0).max()) * 8 < 2 ** 24
    tot = slab[:, :, :C_].double().sum(0)
    assert torch.equal(tot[0], s_b) and torch.equal(tot[1], s_g), name
    # ... in the format mcamd_bn_act_bwd finishes from
    dyv, dgm, dbt, coef = p.bn_bwd(gbuf, slab)
    assert torch.equal(dbt, s_b.float()) and torch.equal(dgm, s_g.float()), name
    dyv2, dgm2, dbt2, coef2 = p.bn_bwd(gbuf, None)
    assert torch.equal(dgm2, dgm) and torch.equal(dbt2, dbt) and torch.equal(coef2, coef)
    assert torch.equal(dyv.view(torch.int16), dyv2.view(torch.int16))
    # ---- a second run: the same bits; without the descriptor: the same G and dW
    gbuf2, slab2, dw2, ws2 = p.fused(mask=mask, grad_scale=grad_scale)
    assert torch.equal(gbuf2.view(torch.int16), gbuf.view(torch.int16)) and torch.equal(dw2, dw)
    assert torch.equal(slab2[:, :, :C_], slab[:, :, :C_]) and torch.equal(ws2, ws)
    gbuf3, _, dw3, _ = p.fused(mask=mask, grad_scale=grad_scale, sums=False)
    assert torch.equal(gbuf3.view(torch.int16), gbuf.view(torch.int16)) and torch.equal(dw3, dw)
    # ---- and the two launches it replaces
    gbuf0, dw0 = p.two_launch(mask=mask, grad_scale=grad_scale)
    assert torch.equal(gbuf0.view(torch.int16), gbuf.view(torch.int16)) and torch.equal(dw0, dw)


@pytest.mark.parametrize("inst", sorted(INSTANCES), ids=["%dx%d" % i for i in sorted(INSTANCES)])
def test_bwd1x1_saturates_like_dgrad(dev, inst):
    cout, cin = inst
    B, H, W = 2, 9, 7
    gen = torch.Generator(device=dev).manual_seed(3)
    gy = torch.randint(-2, 3, (B, H, W, cout), generator=gen, device=dev).float()
    gy[1, 4, 3, 0], gy[1, 4, 3, 1] = 60000.0, 60000.0         # two filters that feed column 5 with weight +1 ...
    gy[0, 2, 6, 2], gy[0, 2, 6, 3] = -50000.0, -40000.0       # ... and column 9 with weight +1
    x = torch.randint(1, 9, (B, H, W, cin), generator=gen, device=dev).float() / 8.0
    w = torch.zeros(cout, cin, 1, 1, device=dev)
    w[0, 5], w[1, 5], w[2, 9], w[3, 9], w[4, 17] = 1.0, 1.0, 1.0, 1.0, 1.0
    p = Problem(dev, B, H, W, cout, cin, w, gy, x)
    gbuf, _, _, _ = p.fused(sums=False)
    flag = int(p.overflow.item())
    gbuf0, _ = p.two_launch()
    assert flag == 1 and int(p.overflow.item()) == 1
    assert torch.equal(gbuf.view(torch.int16), gbuf0.view(torch.int16))
    G = gbuf.view(B, H, W, cin)
    assert float(G[1, 4, 3, 5]) == 65504.0 and float(G[0, 2, 6, 9]) == -65504.0 and bool(torch.isfinite(gbuf).all())
    gy[1, 4, 3, 1], gy[0, 2, 6, 3] = 0.0, 0.0                 # 60000 and -50000 alone fit: no flag
    q = Problem(dev, B, H, W, cout, cin, w, gy, x)
    q.fused(sums=False)
    assert int(q.overflow.item()) == 0


ZERO = 3
LOW = {8: (1e-3, 1.0), 9: (-1e-3, -1.0), 10: (1e-2, -1.1), 11: (-1e-2, 0.9)}       # channel: (gamma, beta)


@pytest.mark.parametrize("inst", sorted(INSTANCES), ids=["%dx%d" % i for i in sorted(INSTANCES)])
def test_bwd1x1_random_data_against_two_pass(dev, inst):
    cout, cin = inst
    B, H, W, C_, ch_lo = 3, 26, 22, cin // 2, 8          # (BatchNorm passes take 8 x a power of two channels)
    M = B * H * W
    gen = torch.Generator(device=dev).manual_seed(23 + cin)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)         # noqa: E731
    # the producer's forward: fp32 y, batch statistics, the coefficients as bn_coeffs forms them, the stored activation
    y = (rnd(M, C_) * 0.7 + 0.4).contiguous()
    gamma = torch.rand(C_, generator=gen, device=dev, dtype=torch.float64) + 0.5
    beta = rnd(C_).double() * 0.2
    gamma[ZERO] = 0.0
    for c, (gv, bv) in LOW.items():
        gamma[c], beta[c] = gv, bv
    mean = y.double().mean(0)
    invstd = 1.0 / torch.sqrt(y.double().var(0, unbiased=False) + 1e-5)
    scale = (gamma * invstd).float()
    shift = (beta - mean * scale.double()).float()
    z32 = y * scale + shift
    act = torch.where(z32 > 0, z32, z32 * SLOPE).half()
    assert 0.2 < float((act > 0).float().mean()) < 0.8                   # both LeakyReLU sides
    x = rnd(B, H, W, cin).half()                                         # the other members of the concat
    x[..., ch_lo:ch_lo + C_] = act.view(B, H, W, C_)
    w = rnd(cout, cin, 1, 1) * (1.0 / cout) ** 0.5
    gy = rnd(B, H, W, cout) * 4.0
    p = Problem(dev, B, H, W, cout, cin, w, gy, x.float(), pad=1, x_extra=8, C=C_, ch_lo=ch_lo,
                coef=(scale, shift, mean.float(), invstd.float()), y=y.view(-1))
    gbuf, slab, dw, _ = p.fused(grad_scale=4.0)
    gbuf0, dw0 = p.two_launch(grad_scale=4.0)
    assert torch.equal(gbuf.view(torch.int16), gbuf0.view(torch.int16))
    # dW: the same fp16 products summed in fp32 in another order; float64 of the stored operands is the reference
    dw_ref = (gy.half().view(M, cout).double().t() @ x.view(M, cin).double()) / 4.0
    absum = (gy.half().view(M, cout).double().abs().t() @ x.view(M, cin).double().abs()) / 4.0
    e1 = float(((dw.view(cout, cin).double() - dw_ref).abs() / absum).max())
    e0 = float(((dw0.view(cout, cin).double() - dw_ref).abs() / absum).max())
    print("%dx%d: dW worst |error| / sum|terms|: one launch %.3g, conv_wgrad %.3g" % (cout, cin, e1, e0))
    # (every product is exact in fp32; each of the at most M + splits additions rounds a partial sum that is at most
    # sum|terms|: the worst case of any summation order)
    bound = (M + ops.conv_bwd1x1_wgrad_splits(p.g) + 1024) * EPS24
    assert e1 < bound and e0 < bound

    # ---- float64 evaluation of the sums from the tensors as stored, with the kernels' rule
    sc64, sh64, mu64, is64 = (t.double() for t in p.coef)
    Gd, ad = gbuf[:, ch_lo:ch_lo + C_].double(), act.double()
    slope64 = float(np.float32(SLOPE))
    beta64 = sh64 + mu64 * sc64
    ill = sc64.abs() < T * beta64.abs().clamp_min(1.0) * is64
    assert bool(ill[ZERO]) and all(bool(ill[c]) for c in LOW) and int(ill.sum()) == 1 + len(LOW)
    pos = ad > 0
    gz = torch.where(pos, Gd, Gd * slope64)
    zz = torch.where(pos, ad, ad / slope64)
    xh = torch.where(ill, (y.double() - mu64) * is64, (zz - beta64) * torch.where(sc64 != 0, is64 / sc64, torch.zeros_like(sc64)))
    tb, tg = gz.sum(0), (gz * xh).sum(0)
    nb, ng = gz.abs().sum(0).clamp_min(1e-30), (gz * xh).abs().sum(0).clamp_min(1e-30)
    dy_ref = sc64 * (gz - tb / M - xh * (tg / M))
    rms = dy_ref.pow(2).mean(0).sqrt().clamp_min(1e-30)
    fused = p.bn_bwd(gbuf, slab)
    two = p.bn_bwd(gbuf, None)

    def dev_of(r):
        dyv, dgm, dbt, _ = r
        return ((dbt.double() - tb).abs() / nb, (dgm.double() - tg).abs() / ng, (dyv.double() - dy_ref).pow(2).mean(0).sqrt() / rms)
    df, dt = dev_of(fused), dev_of(two)
    for what, f_, t_ in zip(("dbeta / sum|g_z|", "dgamma / sum|g_z xhat|", "dY rms / rms"), df, dt):
        print("%dx%d: %-24s worst deviation from float64: fused %.3g  two-pass %.3g  (worst fused - 2 two-pass: %.3g; 4 x 2^-24 = %.3g)"
              % (cout, cin, what, float(f_.max()), float(t_.max()), float((f_ - 2 * t_).max()), 4 * EPS24))
    for f_, t_ in zip(df, dt):
        assert bool((f_ <= 2 * t_ + 4 * EPS24).all())
    assert float(fused[0][:, ZERO].abs().max()) == 0.0


def test_bwd1x1_arguments_are_checked(dev):
    cout, cin = 64, 128
    z = torch.zeros(2, 6, 6, cout, device=dev)
    p = Problem(dev, 2, 6, 6, cout, cin, torch.zeros(cout, cin, 1, 1, device=dev), z, torch.zeros(2, 6, 6, cin, device=dev))
    gbuf = torch.zeros(p.M * cin, dtype=torch.float16, device=dev)
    dw = torch.zeros(cout, cin, 1, 1, device=dev)
    rows = ops.conv_bwd1x1_sums_rows(p.g)
    slab = torch.zeros(rows + 1, 2, cin, device=dev)
    bad = [ops.dgrad_sums(slab, p.xb, p.x_ld, 0, 0, *p.coef, SLOPE, cin),                         # rows
           ops.dgrad_sums(slab[:rows], p.dyb, p.x_ld, 0, 0, *p.coef, SLOPE, cin),                  # not the block's input
           ops.dgrad_sums(slab[:rows], p.xb, p.x_ld, 8, 0, *p.coef, SLOPE, cin - 8),               # act_choff != x_choff + ch_lo
           ops.dgrad_sums(slab[:rows], p.xb, p.x_ld, 0, 1, *p.coef, SLOPE, cin)]                   # the other pad form
    for d in bad:
        with pytest.raises(L.McamdError):
            ops.conv_bwd1x1(p.g, p.xb, p.dyb, cout, 0, p.wd, gbuf, cin, 0, dw, sums=d)
    with pytest.raises(L.McamdError):                                                            # workspace too small
        ops.conv_bwd1x1(p.g, p.xb, p.dyb, cout, 0, p.wd, gbuf, cin, 0, dw, workspace=torch.zeros(1024, dtype=torch.uint8, device=dev))
    with pytest.raises(L.McamdError):                                                            # G slice past its row
        ops.conv_bwd1x1(p.g, p.xb, p.dyb, cout, 0, p.wd, gbuf, cin, 8, dw)
    g3 = ops.geom(2, 6, 6, 1, 96, 64, 96)
    with pytest.raises(L.McamdError, match="no kernel instance"):
        ops.conv_bwd1x1(g3, p.xb, p.dyb, cout, 0, p.wd, gbuf, 96, 0, dw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
# d. the engine, route on against off
# ------------------------------------------------------------------------------------------------------------------
CHAIN_CFG = """[net]
batch=1
height=32
width=32
channels=3
momentum=0.9
decay=0.0005
learning_rate=0.001
max_batches=100
policy=steps
steps=40,60
scales=.1,.1
""" + "".join("""
[convolutional]
batch_normalize=1
filters=%d
size=%d
stride=1
pad=1
activation=leaky
""" % fk for fk in ((32, 3), (128, 3), (64, 1), (256, 3), (128, 1), (64, 3))) + """
[convolutional]
filters=125
size=1
stride=1
pad=1
activation=linear

[region]
anchors=1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071
bias_match=1
classes=20
coords=4
num=5
softmax=1
jitter=.3
rescore=1
object_scale=5
noobject_scale=1
class_scale=1
coord_scale=1
absolute=1
thresh=.6
random=1
"""


def _oracle_grads(blocks, state, x, gout):
    st = {k: v.clone() for k, v in state.items()}
    for k in O.param_keys(blocks):
        st[k].requires_grad_(True)
    O.forward(blocks, st, x, training=True, storage=None).backward(gout)
    return {k: st[k].grad for k in O.param_keys(blocks)}


# cfg, input shape, logit shape, the 1-based blocks that take the route
ENGINE = [("chain", None, (2, 3, 32, 32), (2, 125, 32, 32), {3, 5}),
          ("yolov2-b2", YOLOV2_VOC_CFG, (2, 3, 416, 416), (2, 125, 13, 13), {4, 7})]


@pytest.mark.parametrize("case", ENGINE, ids=[c[0] for c in ENGINE])
def test_engine_route_on_against_off(dev, monkeypatch, tmp_path, case):
    name, cfg, xshape, oshape, covered = case
    if cfg is None:
        cfg = str(tmp_path / "chain.cfg")
        with open(cfg, "w") as f:
            f.write(CHAIN_CFG)
    blocks = O.parse_cfg(cfg)
    state = O.init_state(blocks, seed=1)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(*xshape, generator=g)
    gout = torch.randn(*oshape, generator=g)
    res = {}
    calls, bwd1x1 = [], ops.conv_bwd1x1

    def counting(*a, **kw):
        calls.append(a[0])
        return bwd1x1(*a, **kw)
    monkeypatch.setattr(ops, "conv_bwd1x1", counting)
    for on in ("1", "0"):
        monkeypatch.setenv("MCAMD_BWD1X1", on)
        del calls[:]
        m = nets.Darknet(cfg)
        m.load_state_dict(state)
        m.to(dev).train()                                   # default precision
        out = m(x.to(dev))
        out.backward(gout.to(dev))
        eng = [e for e in m._engines.values() if e.precision == "mixed"][-1]
        took = {lay.li + 1 for lay in eng.layers if eng._bwd1x1_route(lay)}
        stats = {n_: b_.clone() for n_, b_ in m.named_buffers() if "running" in n_}
        res[on] = (out.detach().clone(), {n_: p_.grad.clone() for n_, p_ in m.named_parameters()}, took, len(calls), stats)
        del m
    print("%s: blocks on the one-launch backward: %s" % (name, sorted(res["1"][2])))
    assert res["1"][2] == covered and not res["0"][2]
    assert res["1"][3] == len(covered) and res["0"][3] == 0
    assert torch.equal(res["1"][0], res["0"][0])            # the forward pass is untouched
    for n_ in res["1"][4]:
        assert torch.equal(res["1"][4][n_], res["0"][4][n_]), n_
    ref = _oracle_grads(blocks, state, x, gout)
    worst = (0.0, 0.0, "")
    for n_ in res["1"][1]:
        g1, g0 = res["1"][1][n_].cpu(), res["0"][1][n_].cpu()
        e1, e0 = rel_l2(g1, ref[n_]), rel_l2(g0, ref[n_])
        print("%s: %-28s distance to the float64 oracle: one launch %.4g, two launches %.4g" % (name, n_, e1, e0))
        if e1 - e0 > worst[0] - worst[1]:
            worst = (e1, e0, n_)
        # summation-order room only: 10 % of the two-launch route's own distance
        assert e1 <= 1.10 * e0, (n_, e1, e0)
    print("%s: largest excess at %s: one launch %.4g, two launches %.4g" % (name, worst[2], worst[0], worst[1]))
