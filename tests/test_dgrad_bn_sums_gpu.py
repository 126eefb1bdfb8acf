"""A PLAIN block's BatchNorm-backward sums taken in the epilogue of the dgrad launch that stores its G (mcamd_conv_dgrad_sums,
conv_epi.h store_raw_tile_sums), and mcamd_bn_act_bwd finishing from them (mcamd_act_bwd_desc.sums).

Every case drives the real conv_dgrad_raw launch with the descriptor, then bn_act_bwd with the slab: the inputs of the sums
are what the dgrad stored.

a. Every element counted once, exactly: a dgrad whose G is exact in fp16 (1x1 with identity weights: G == dY; 3x3 with a few
   +-1 weights per row), integer dY, activations positive multiples of 1/8, mean 0, invstd 1, gamma 1, beta 0.  Every
   partial sum is then an exact fp32 number whatever the order, so dbeta, dgamma and the two coefficients must equal the
   float64 evaluation BIT FOR BIT.  Shapes: a ragged last M tile for every tile height (M = 507), more M tiles than
   persistent slots (the per-slot tile loop of either kernel), the 128- and 64-column tiles, a producer at channel offset
   256 of a 1280-wide G row, a channel count that is no multiple of the tile width (padded columns stay out).
b. Random data with both LeakyReLU sides, gamma in {0, 1e-3, 1e-2} at |beta| ~ 1 among healthy channels, one ping-pong and
   one igemm_kernel instance: per channel the fused route's deviation from the float64 evaluation of the two sums (from the
   tensors as stored, same rule), normalised by sum|g_z| resp. sum|g_z xhat|, is at most twice that of the two-pass route
   on identical inputs plus 4 x 2^-24 (the final fp32 rounding) -- the two differ only in the order of fp32 partial sums
   of the same terms; dY of the second pass likewise.
c. The engine with the route on against off (MCAMD_DGRAD_BN_SUMS), mini cfg and YOLOv2 at B = 2, default precision: logits
   bit-equal, every parameter gradient between the routes and against the bars of tests/test_model_gpu.py, the step
   bit-reproducible with the route on."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, ops, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd import _lib as L  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "golden", "mini.cfg")
SLOPE = 0.1
T = 2.0 ** -5            # BN_ACT_T of csrc/common.h
SLAB_ROWS = 1024         # rows of the two-pass slab in front of the coefficients in mcamd_bn_act_bwd's workspace (kBwdBlocks)

# tile switches of a case: None = the route the library picks; (bm, bn) = that ping-pong tile whenever legal
PP = lambda bm, bn: {"MCAMD_PP": "2", "MCAMD_PP_BM": str(bm), "MCAMD_PP_BN": str(bn)}  # noqa: E731


class Problem:
    """One consumer convolution (cin input channels = the width of G, cout filters) whose producer owns the G columns
    [ch_lo, ch_lo + C): device tensors of the dgrad launch and of the producer's BatchNorm backward."""

    def __init__(self, dev, B, H, W, k, cin, cout, w, gy, C, ch_lo, act, scale, shift, mean, invstd, y=None, act_pad=0):
        self.dev, self.B, self.H, self.W, self.C, self.ch_lo, self.cin = dev, B, H, W, C, ch_lo, cin
        self.M = B * H * W
        self.g = ops.geom(B, H, W, k, cin, cout, ops.round_up(cin, 32))
        _, self.wd = ops.pack_weights(self.g, w.contiguous(), want_fwd=False)
        self.dy_ld = ops.round_up(cout, 32)
        self.dyb = ops.alloc_padded(B, H, W, self.dy_ld, dev)
        ops.padded_view(self.dyb, B, H, W, self.dy_ld)[:, 1:-1, 1:-1, :cout] = gy.half()            # gy: [B, H, W, cout]
        # the producer's stored activation: a channel slice of a wider padded buffer, as in the engine
        self.act_ld, self.act_choff, self.act_pad = ops.round_up(cin, 8) + 16, ch_lo + 8, act_pad
        self.abuf = ops.alloc_padded(B, H, W, self.act_ld, dev, pad=act_pad)
        ops.padded_view(self.abuf, B, H, W, self.act_ld, pad=act_pad)[:, 1:-1, 1:-1, self.act_choff:self.act_choff + C] = act
        self.coef = [t.float().contiguous().to(dev) for t in (scale, shift, mean, invstd)]
        self.y = y

    def dgrad(self, fused, concurrent=False):
        """(G [M, cin] fp16, slab or None, tile)"""
        out = torch.full((self.M * self.cin,), float("nan"), dtype=torch.float16, device=self.dev)
        slab = desc = None
        if fused:
            rows = ops.dgrad_sums_rows(self.g, concurrent)
            assert rows > 0, "this geometry's dgrad kernel cannot take sums: %s" % (ops.tile_info(self.g, True, concurrent),)
            slab = torch.full((rows, 2, self.C + 8), float("nan"), device=self.dev)          # ld > C
            desc = ops.dgrad_sums(slab, self.abuf, self.act_ld, self.act_choff, self.act_pad, *self.coef, SLOPE, self.C,
                                  ch_lo=self.ch_lo, y=self.y, y_ld=self.C, y_choff=0)
        ops.conv_dgrad_raw(self.g, self.dyb, self.dy_ld, 0, self.wd, out, self.cin, concurrent=concurrent, sums=desc)
        return out.view(self.M, self.cin), slab, ops.tile_info(self.g, True, concurrent)

    def bn_bwd(self, G, slab, grad_scale=1.0):
        """(dY [M, C] fp16, dgamma, dbeta, coefficients [2, C]) of the producer from G -- the two passes, or with `slab` the
        coefficient kernel and the dY pass only."""
        C_ = self.C
        ws = torch.zeros(ops.bn_act_bwd_workspace_bytes(C_), dtype=torch.uint8, device=self.dev)
        dy = ops.alloc_padded(self.B, self.H, self.W, C_, self.dev)
        dgm, dbt = (torch.full((C_,), float("nan"), device=self.dev) for _ in range(2))
        sc, sh, mu, ist = self.coef
        ops.bn_act_bwd(self.B, self.H, self.W, C_, self.y, C_, 0, sc, sh, mu, ist, SLOPE, L.DST_PLAIN, G.view(-1), self.cin,
                       self.ch_lo, dy, C_, 0, dgm, dbt, grad_scale=grad_scale, workspace=ws, act=self.abuf, act_ld=self.act_ld,
                       act_choff=self.act_choff, act_pad=self.act_pad, sums=slab)
        torch.cuda.synchronize()
        coef = ws.view(torch.float32)[SLAB_ROWS * 2 * C_: SLAB_ROWS * 2 * C_ + 2 * C_].view(2, C_).clone()
        dyv = ops.padded_view(dy, self.B, self.H, self.W, C_)[:, 1:-1, 1:-1].reshape(self.M, C_)
        return dyv, dgm, dbt, coef


# ------------------------------------------------------------------------------------------------------------------
# a. exact
# ------------------------------------------------------------------------------------------------------------------
# (name, B, H, W, k, consumer cin (= cout), producer C, ch_lo, tile switches, dY / activation magnitude bound, expect)
# expect: (kernel kind, BM, BN) of ops.tile_info or None; "loop": the launch has more M tiles than slab rows
EXACT = [
    # M = 507: ragged last M tile for BM = 128, 192 and 256
    ("m507-route", 3, 13, 13, 1, 256, 256, 0, None, 4, (0, 128, 64)),
    ("m507-pp192x256", 3, 13, 13, 1, 256, 256, 0, PP(192, 256), 4, (2, 192, 256)),
    ("m507-pp192x128", 3, 13, 13, 1, 256, 256, 0, PP(192, 128), 4, (2, 192, 128)),
    ("m507-pp256x128", 3, 13, 13, 1, 256, 256, 0, PP(256, 128), 4, (2, 256, 128)),
    ("m507-pp256x256", 3, 13, 13, 1, 256, 256, 0, PP(256, 256), 4, (2, 256, 256)),
    # the 128-column tile of igemm_kernel on many M tiles
    ("b16-52-c128", 16, 52, 52, 1, 128, 128, 0, None, 4, (0, 128, 128)),
    # more M tiles than persistent slots: ping-pong (226 tiles on 128 slots) and igemm_kernel (1 352 tiles on 1 024 slots;
    # |dY|, act <= 2 keep every partial sum below 2^24 / 8 at M = 173 056)
    ("b16-52-c256-pp192x128-loop", 16, 52, 52, 1, 256, 256, 0, PP(192, 128), 4, (2, 192, 128)),
    ("b64-52-c256-loop", 64, 52, 52, 1, 256, 256, 0, None, 2, (0, 128, 128)),
    # conv22's dgrad: a 1280-wide G row, the producer at channel offset 256
    ("off256-route", 2, 13, 13, 1, 1280, 1024, 256, None, 4, None),
    ("off256-pp192x256", 2, 13, 13, 1, 1280, 1024, 256, PP(192, 256), 4, (2, 192, 256)),
    # a 248-wide G row: the last column tile is padded, and the producer's 128 channels (BatchNorm passes take 8 x a
    # power of two) end at its last real column
    ("c248-route", 3, 13, 13, 1, 248, 128, 120, None, 4, (0, 128, 64)),
    ("c248-pp192x256", 3, 13, 13, 1, 248, 128, 120, PP(192, 256), 4, (2, 192, 256)),
    ("c248-pp256x128", 3, 13, 13, 1, 248, 128, 120, PP(256, 128), 4, (2, 256, 128)),
    # igemm_kernel's other instances: 32-channel K chunks (96 filters), and the 192 x 128 tile (3x3 with the centre tap an
    # identity, ping-pong off: 676 tiles of 128 rows would need two rounds, 452 of 192 rows one)
    ("bk32-cout96", 3, 13, 13, 1, 128, 128, 0, None, 4, (0, 128, 64)),
    ("k3id-igemm192x128", 16, 52, 52, 3, 256, 256, 0, {"MCAMD_PP": "0"}, 4, (0, 192, 128)),
    # 3x3 on the ping-pong kernel: 8 filters x 9 taps of weight +-1 per input channel, |G| <= 288 exact in fp16
    ("k3-pp192x256", 4, 13, 13, 3, 256, 256, 0, PP(192, 256), 4, (2, 192, 256)),
    ("k3-pp256x128", 4, 13, 13, 3, 256, 256, 0, PP(256, 128), 4, (2, 256, 128)),
]


@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_sums_count_every_element_once_exactly(dev, setenv, case):
    name, B, H, W, k, cin, C_, ch_lo, env, vmax, expect = case
    for kv in (env or {}).items():
        setenv(*kv)
    gen = torch.Generator(device=dev).manual_seed(5 + B + cin)
    M, cout = B * H * W, 96 if "cout96" in name else cin
    gy = torch.randint(-vmax, vmax + 1, (B, H, W, cout), generator=gen, device=dev).float()
    act = (torch.randint(1, 8 * vmax + 1, (B, H, W, C_), generator=gen, device=dev).float() / 8.0).half()
    w = torch.zeros(cout, cin, k, k, device=dev)
    if k == 1 or "k3id" in name:
        w[torch.arange(cout), torch.arange(cout), k // 2, k // 2] = 1.0           # G[:, :cout] == dY, the other columns 0
    else:
        n, c = torch.meshgrid(torch.arange(cout), torch.arange(cin), indexing="ij")
        sel = (n % 32) == (c % 32)                          # 8 filters per input channel
        sign = (torch.randint(0, 2, (cout, cin, k, k), generator=gen, device=dev).float() * 2 - 1)
        w = sign * sel.to(dev).view(cout, cin, 1, 1)
    ones, zeros = torch.ones(C_), torch.zeros(C_)
    p = Problem(dev, B, H, W, k, cin, cout, w, gy, C_, ch_lo, act, ones, zeros, zeros, ones)
    G, slab, tile = p.dgrad(True)
    G0, _, _ = p.dgrad(False)
    print("%s: M %d, tile %s, slab rows %d, M tiles %d" % (name, M, tile, slab.shape[0], -(-M // tile[0])))
    if expect is not None:
        assert (tile[3], tile[0], tile[1]) == expect, tile
    if name.endswith("loop"):
        assert -(-M // tile[0]) > slab.shape[0]
    # the tile store itself: same bits as the launch without the descriptor; a 1x1 identity makes G == dY
    assert torch.equal(G.view(torch.int16), G0.view(torch.int16))
    if k == 1 or "k3id" in name:
        assert torch.equal(G[:, :cout], gy.view(M, cout).half()) and not bool(G[:, cout:].any())
    else:
        assert float(G.float().abs().max()) <= 72 * vmax and torch.equal(G.float(), G.float().round())
    assert bool(torch.isfinite(slab[:, :, :C_]).all()) and bool(torch.isnan(slab[:, :, C_:]).all())
    Gd, ad = G[:, ch_lo:ch_lo + C_].double(), act.view(M, C_).double()
    s_b, s_g = Gd.sum(0), (Gd * ad).sum(0)                  # float64: exact
    assert float((Gd * ad).abs().sum(0).max()) * 8 < 2 ** 24
    dyv, dgm, dbt, coef = p.bn_bwd(G, slab)
    assert torch.equal(dbt, s_b.float()) and torch.equal(dgm, s_g.float()), name
    assert torch.equal(coef[0], (s_b / M).float()) and torch.equal(coef[1], (s_g / M).float()), name
    # ... and the same four from the two passes (exact in any order): the dY pass sees the same coefficients
    dyv2, dgm2, dbt2, coef2 = p.bn_bwd(G, None)
    assert torch.equal(dgm2, dgm) and torch.equal(dbt2, dbt) and torch.equal(coef2, coef)
    assert torch.equal(dyv.view(torch.int16), dyv2.view(torch.int16))


def test_sums_descriptor_is_checked(dev, setenv):
    """rows must be the query's answer; a launch whose kernel has no sums-taking form refuses the descriptor instead of
    ignoring it; bn_act_bwd takes a slab for PLAIN blocks with `act` only."""
    B, H, W, C_ = 2, 13, 13, 64
    z = torch.zeros(B, H, W, C_, device=dev)
    mk = lambda cin: Problem(dev, B, H, W, 1, cin, cin, torch.zeros(cin, cin, 1, 1, device=dev),  # noqa: E731
                             torch.zeros(B, H, W, cin, device=dev), C_, 0, z.half(), torch.ones(C_), torch.zeros(C_), torch.zeros(C_),
                             torch.ones(C_))
    p = mk(64)
    rows = ops.dgrad_sums_rows(p.g)
    assert rows > 0
    out = torch.zeros(p.M * 64, dtype=torch.float16, device=dev)
    for bad_rows in (rows + 1, 0):
        slab = torch.zeros(max(bad_rows, 1), 2, C_, device=dev)
        d = ops.dgrad_sums(slab, p.abuf, p.act_ld, p.act_choff, 0, *p.coef, SLOPE, C_)
        d.rows = bad_rows
        with pytest.raises(L.McamdError):
            ops.conv_dgrad_raw(p.g, p.dyb, p.dy_ld, 0, p.wd, out, 64, sums=d)
    slab = torch.zeros(rows, 2, C_, device=dev)
    for kw in (dict(ch_lo=4), dict(ch_lo=8), dict(C_=C_ + 8)):            # off the 8-channel grid / past the G row
        args = dict(C_=C_)
        args.update(kw)
        d = ops.dgrad_sums(slab, p.abuf, p.act_ld, p.act_choff, 0, *p.coef, SLOPE, args.pop("C_"), **args)
        with pytest.raises(L.McamdError):
            ops.conv_dgrad_raw(p.g, p.dyb, p.dy_ld, 0, p.wd, out, 64, sums=d)
    q = mk(96)                                                          # 96 columns take the 32-column tile: no sums form
    assert ops.tile_info(q.g, True)[1] == 32 and ops.dgrad_sums_rows(q.g) == 0
    d = ops.dgrad_sums(slab, q.abuf, q.act_ld, q.act_choff, 0, *q.coef, SLOPE, C_)
    with pytest.raises(L.McamdError):
        ops.conv_dgrad_raw(q.g, q.dyb, q.dy_ld, 0, q.wd, torch.zeros(q.M * 96, dtype=torch.float16, device=dev), 96, sums=d)
    # bn_act_bwd: a slab without `act`
    sc, sh, mu, ist = p.coef
    y = torch.zeros(p.M * C_, device=dev)
    with pytest.raises(L.McamdError):
        ops.bn_act_bwd(B, H, W, C_, y, C_, 0, sc, sh, mu, ist, SLOPE, L.DST_PLAIN, out, 64, 0, ops.alloc_padded(B, H, W, C_, dev), C_, 0,
                       None, None, sums=slab)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
# b. random data
# ------------------------------------------------------------------------------------------------------------------
ZERO = 3
LOW = {8: (1e-3, 1.0), 9: (-1e-3, -1.0), 10: (1e-2, -1.1), 11: (-1e-2, 0.9)}       # channel: (gamma, beta)
RANDOM = [
    ("pp192x256-k3-m507", 3, 13, 13, 3, 256, 256, 0, PP(192, 256), (2, 192, 256)),
    ("igemm-off256", 2, 13, 13, 1, 1280, 1024, 256, None, None),
    ("igemm128x128-b16-52", 16, 52, 52, 1, 128, 128, 0, None, (0, 128, 128)),
]
EPS24 = 2.0 ** -24


@pytest.mark.parametrize("case", RANDOM, ids=[c[0] for c in RANDOM])
def test_sums_random_data_against_two_pass(dev, setenv, case):
    name, B, H, W, k, cin, C_, ch_lo, env, expect = case
    for kv in (env or {}).items():
        setenv(*kv)
    gen = torch.Generator(device=dev).manual_seed(23 + B + cin)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)         # noqa: E731
    M, cout = B * H * W, 256 if k == 3 else min(cin, 512)
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
    # the consumer's weights and dY: G is O(1)
    w = rnd(cout, cin, k, k) * (1.0 / (cout * k * k)) ** 0.5
    gy = rnd(B, H, W, cout) * 4.0
    p = Problem(dev, B, H, W, k, cin, cout, w, gy, C_, ch_lo, act.view(B, H, W, C_), scale, shift, mean.float(), invstd.float(), y=y.view(-1))
    G, slab, tile = p.dgrad(True)
    G0, _, _ = p.dgrad(False)
    if expect is not None:
        assert (tile[3], tile[0], tile[1]) == expect, tile
    assert torch.equal(G.view(torch.int16), G0.view(torch.int16))

    # ---- float64 evaluation from the tensors as stored, with the kernels' rule
    sc64, sh64, mu64, is64 = (t.double() for t in p.coef)
    Gd, ad = G[:, ch_lo:ch_lo + C_].double(), act.double()
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
    dm = sc64
    dy_ref = dm * (gz - tb / M - xh * (tg / M))
    rms = dy_ref.pow(2).mean(0).sqrt().clamp_min(1e-30)

    fused = p.bn_bwd(G, slab)
    G2, slab2, _ = p.dgrad(True)
    assert torch.equal(slab2[:, :, :C_], slab[:, :, :C_])
    fused2 = p.bn_bwd(G2, slab2)
    two = p.bn_bwd(G, None)
    for a_, b_ in zip(fused, fused2):
        assert torch.equal(a_, b_), "two fused runs differ"

    def dev_of(r):
        dyv, dgm, dbt, _ = r
        return ((dbt.double() - tb).abs() / nb, (dgm.double() - tg).abs() / ng, (dyv.double() - dy_ref).pow(2).mean(0).sqrt() / rms)
    df, dt = dev_of(fused), dev_of(two)
    for what, f_, t_ in zip(("dbeta / sum|g_z|", "dgamma / sum|g_z xhat|", "dY rms / rms"), df, dt):
        print("%s: %-24s worst deviation from float64: fused %.3g  two-pass %.3g  (worst fused - 2 two-pass: %.3g; 4 x 2^-24 = %.3g)"
              % (name, what, float(f_.max()), float(t_.max()), float((f_ - 2 * t_).max()), 4 * EPS24))
    for f_, t_ in zip(df, dt):
        assert bool((f_ <= 2 * t_ + 4 * EPS24).all())
    assert float(fused[0][:, ZERO].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------
# c. the engine, route on against off
# ------------------------------------------------------------------------------------------------------------------
def _oracle_grads(blocks, state, x, gout, storage):
    st = {k: v.clone() for k, v in state.items()}
    for k in O.param_keys(blocks):
        st[k].requires_grad_(True)
    O.forward(blocks, st, x, training=True, storage=storage).backward(gout)
    return {k: st[k].grad for k in O.param_keys(blocks)}


# cfg, input size, logit shape, the slack test_model_gpu.py adds to 1.5 x the oracle's fp16-storage floor for this engine,
# the 1-based blocks whose sums the dgrad epilogues take (None: at least one)
ENGINE = [("mini", MINI, None, 2e-3, None),
          ("yolov2-b2", YOLOV2_VOC_CFG, (2, 3, 416, 416), 5e-3, {3, 4, 6, 7, 9, 10, 11, 12, 14, 15, 16, 17, 18, 19, 20, 22})]


@pytest.mark.parametrize("case", ENGINE, ids=[c[0] for c in ENGINE])
def test_engine_route_on_against_off(dev, monkeypatch, case):
    name, cfg, xshape, slack, covered = case
    blocks = O.parse_cfg(cfg)
    state = O.init_state(blocks, seed=1)
    if xshape is None:
        gold = np.load(os.path.join(HERE, "golden", "mini_fwd_bwd.npz"))
        x, gout = torch.from_numpy(gold["x"]), torch.from_numpy(gold["gout"])
    else:
        g = torch.Generator().manual_seed(7)
        x = torch.rand(*xshape, generator=g)
        gout = torch.randn(xshape[0], 125, xshape[2] // 32, xshape[3] // 32, generator=g)
    res = {}
    with_sums, bn_act_bwd = [], ops.bn_act_bwd

    def counting(*a, **kw):
        if kw.get("sums") is not None:
            with_sums.append(kw["sums"])
        return bn_act_bwd(*a, **kw)
    monkeypatch.setattr(ops, "bn_act_bwd", counting)
    for on in ("1", "0", "1"):
        monkeypatch.setenv("MCAMD_DGRAD_BN_SUMS", on)
        del with_sums[:]
        m = nets.Darknet(cfg)
        m.load_state_dict(state)
        m.to(dev).train()                                   # default precision
        out = m(x.to(dev))
        out.backward(gout.to(dev))
        eng = [e for e in m._engines.values() if e.precision == "mixed"][-1]
        took = sorted(v[2].li + 1 for v in eng._dgrad_sums_cache.values() if v is not None)
        run = (out.detach().clone(), {n_: p_.grad.clone() for n_, p_ in m.named_parameters()}, took, len(with_sums))
        if on == "1" and "1" in res:
            # bit-reproducible run to run with the route on
            assert torch.equal(run[0], res["1"][0])
            for n_ in run[1]:
                assert torch.equal(run[1][n_], res["1"][1][n_]), n_
        res[on] = run
        del m
    print("%s: blocks whose sums the dgrad epilogues took: %s" % (name, res["1"][2]))
    assert res["1"][2] and not res["0"][2]
    # every covered block's BatchNorm backward was given its slab (and nobody else's was)
    assert res["1"][3] == len(res["1"][2]) and res["0"][3] == 0, (res["1"][3], res["0"][3])
    if covered is not None:
        assert set(res["1"][2]) == covered, res["1"][2]
    assert torch.equal(res["1"][0], res["0"][0])            # the forward pass is untouched
    ref = _oracle_grads(blocks, state, x, gout, None)
    floor = _oracle_grads(blocks, state, x, gout, "fp16")
    worst = 0.0
    for n_ in res["1"][1]:
        g1, g0 = res["1"][1][n_].cpu(), res["0"][1][n_].cpu()
        between = rel_l2(g1, g0)
        e1, e0, fl = rel_l2(g1, ref[n_]), rel_l2(g0, ref[n_]), rel_l2(floor[n_], ref[n_])
        worst = max(worst, between)
        assert e1 < 1.5 * fl + slack and e0 < 1.5 * fl + slack, (n_, e1, e0, fl)
        # the two routes add the same fp32 terms in another order, then everything downstream is fp16: well inside the bar
        assert between < slack, (n_, between)
    print("%s: worst parameter-gradient rel-L2 between the routes %.3g" % (name, worst))
