"""The forward / dgrad cases of tests/test_conv_instances_gpu.py, their operands and exact references, and the enumeration
of what mcamd_conv_fwd and mcamd_conv_dgrad can launch.

test_host_cpu.py proves on the CPU (through mcamd_conv_route_info, which is answered by the launches' own conv_route())
that CONV_CASES reaches every (kernel, tile, epilogue) instance the route rules can name and every named boundary
condition, and that every case's reference meets the conditions of exactness; test_conv_instances_gpu.py runs each case
against that reference.  Test-side only."""
import collections
import ctypes as C
import zlib

import torch
import torch.nn.functional as F

from modelcompression_amd import ops
from modelcompression_amd import _lib as L

ENV_DEFAULTS = {"MCAMD_PP": "1", "MCAMD_PP_BM": "256", "MCAMD_PP_BN": "256", "MCAMD_BK": "64", "MCAMD_SMALL3X3": "1",
                "MCAMD_WRES": "1", "MCAMD_WRES_MIN_ROUNDS": "4"}

IGEMM, STEM, PP, SMALL, WIN, WRES = (ops.ROUTE_IGEMM, ops.ROUTE_STEM, ops.ROUTE_PP, ops.ROUTE_SMALL3X3, ops.ROUTE_WIN3X3,
                                     ops.ROUTE_WRES)
KERNEL_NAMES = {IGEMM: "igemm_kernel", STEM: "stem_fwd_kernel", PP: "igemm_pp_kernel", SMALL: "small3x3_kernel",
                WIN: "win3x3_kernel", WRES: "wres_kernel", ops.ROUTE_SMALL3X3_SPLIT: "small3x3_split_kernel"}

# epilogue -> (dir, mode, dst_mode, stats) of mcamd_conv_route_info.  The first six are the epilogues a case can have (the
# padded one with its destination form as a run-time argument, `dst`); the others only exist in the sweep of reachable().
EPILOGUES = {
    "fwd-raw16-stats": (ops.DIR_FWD, L.EPI_RAW_F16, L.DST_PLAIN, True),
    "fwd-raw32-stats": (ops.DIR_FWD, L.EPI_RAW_F32, L.DST_PLAIN, True),
    "fwd-nchw": (ops.DIR_FWD, L.EPI_NCHW_F32, L.DST_PLAIN, False),
    "fwd-pad": (ops.DIR_FWD, L.EPI_PAD_F16, L.DST_PLAIN, False),
    "dgrad-raw16": (ops.DIR_DGRAD, L.EPI_RAW_F16, L.DST_PLAIN, False),
    "dgrad-nchw": (ops.DIR_DGRAD, L.EPI_NCHW_F32, L.DST_PLAIN, False),
    "fwd-raw16": (ops.DIR_FWD, L.EPI_RAW_F16, L.DST_PLAIN, False),
    "fwd-raw32": (ops.DIR_FWD, L.EPI_RAW_F32, L.DST_PLAIN, False),
    "fwd-pad-pool": (ops.DIR_FWD, L.EPI_PAD_F16, L.DST_POOL, False),
    "fwd-pad-reorg": (ops.DIR_FWD, L.EPI_PAD_F16, L.DST_REORG, False),
    "dgradc-raw16": (ops.DIR_DGRAD_CONCURRENT, L.EPI_RAW_F16, L.DST_PLAIN, False),
    "dgradc-nchw": (ops.DIR_DGRAD_CONCURRENT, L.EPI_NCHW_F32, L.DST_PLAIN, False),
}
CASE_EPILOGUES = ("fwd-raw16-stats", "fwd-raw32-stats", "fwd-nchw", "fwd-pad", "dgrad-raw16", "dgrad-nchw", "fwd-raw16")
DSTS = {"plain": L.DST_PLAIN, "pool": L.DST_POOL, "pool+y2": L.DST_POOL, "reorg": L.DST_REORG}

# Uneven draws (errors do not cancel); "s4": a quarter non-zero, for long K and for the statistics of many pixels
DRAWS = {"d3": (-3, -2, -1, 0, 1, 1, 2, 3), "d2": (-2, -1, 0, 1, 1, 2), "d1": (-1, -1, 0, 0, 0, 1, 1, 1),
         "s4": (-1, -1, 1, 1) + (0,) * 12, "s4u": (-2, -1, 1, 1, 1) + (0,) * 15}

_FIELDS = ("name epi B H W k cin cout stem pad ld choff y_ld y_choff dst mask concurrent overflow draw wdraw env expect tags")


class Case(collections.namedtuple("Case", _FIELDS)):
    """One launch of mcamd_conv_fwd (epi "fwd-...") or mcamd_conv_dgrad ("dgrad-...").
    ld / choff: the operand slice -- x_ld / x_choff forward, dy_ld / dy_choff dgrad (ld 0: the slice is the whole buffer).
    y_ld / y_choff: the output slice of the fp16 / fp32 row-major and padded epilogues (y_ld 0: the slice is the whole
    buffer).  dst: destination form of "fwd-pad".  mask (dgrad): the weights are packed with a mask that removes scattered
    weights and whole filters.  draw / wdraw: DRAWS keys of the activation and the weight values.
    expect: (kernel, bm, bn, bk) of the route; with epi it names the instance.  tags: the boundary conditions the case was
    written for, each re-derived from the route query by boundary_tags()."""
    __slots__ = ()

    def __str__(self):
        return self.name

    @property
    def fwd(self):
        return self.epi.startswith("fwd")

    @property
    def n(self):
        """output columns of the implicit GEMM"""
        return self.cout if self.fwd else self.cin

    @property
    def M(self):
        return self.B * self.H * self.W

    @property
    def k_tap(self):
        """padded operand channels per tap"""
        return 32 if self.stem else ops.round_up(self.cin if self.fwd else self.cout, 32)

    @property
    def ktot(self):
        return (3 if self.stem else self.k * self.k) * self.k_tap


def case(name, epi, B, H, W, k, cin, cout, expect, stem=0, pad=0, ld=0, choff=0, y_ld=0, y_choff=0, dst="plain", mask=False,
         concurrent=False, overflow=False, draw="d3", wdraw=None, env=None, tags=()):
    assert epi in CASE_EPILOGUES and dst in DSTS and (dst == "plain" or epi == "fwd-pad")
    return Case(name, epi, B, H, W, k, cin, cout, stem, pad, ld, choff, y_ld, y_choff, dst, mask, concurrent, overflow, draw,
                wdraw or draw, dict(env or {}), tuple(expect), tuple(tags))


def geom_of(c):
    if c.stem:
        return ops.geom(c.B, c.H, c.W, 3, 3, c.cout, 4, 0, stem=1)
    if c.fwd:
        return ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, c.ld or c.k_tap, c.choff, pad=c.pad)
    return ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, ops.round_up(c.cin, 32), 0, pad=c.pad)    # (x_ld: unused by dgrad)


def apply_env(c, setenv):
    """Set the route switches for this case (the defaults where the case names none)."""
    for name, default in ENV_DEFAULTS.items():
        setenv(name, c.env.get(name, default))


def route_of(c):
    d, mode, _, stats = EPILOGUES[c.epi]
    if c.concurrent:
        d = ops.DIR_DGRAD_CONCURRENT
    return ops.conv_route_info(geom_of(c), d, mode, DSTS[c.dst], stats)


def instance_of(c, r):
    return (c.epi, (r.kernel, r.bm, r.bn, r.bk))


def stages_of(r):
    """LDS ring stages of the igemm_kernel instance (mcamd_igemm_launch); the ping-pong kernel has two buffers"""
    return 3 if (r.kernel == IGEMM and r.bk == 32) else 2


def boundary_tags(c, r):
    """The named boundary conditions this launch meets, from the route query's tile and rows and the case's shape alone."""
    t = set()
    if r.kernel not in (IGEMM, PP):
        return t
    M, n = c.M, c.n
    mtiles = -(-M // r.bm)
    if M < r.bm:
        t.add("M<bm")
    elif M % r.bm:
        t.add("M%bm!=0")
    if M % r.bm == 0:
        t.add("M%bm==0")
    if c.B > 1 and (c.H * c.W) % r.bm:
        t.add("tile-spans-images")
    if c.B > 1 and c.H * c.W < r.bm:
        t.add("HW<bm")
    if c.W < r.bm and c.H > 1:
        t.add("rows-shorter-than-tile")
    if n % r.bn:
        t.add("n%bn!=0")
    if n % 8:
        t.add("n%8!=0")
    if n < r.bn:
        t.add("n<bn")
    real = c.cin if c.fwd else c.cout
    if not c.stem and c.k_tap > real:
        t.add("k-padded")
    if not c.stem and c.k_tap % 64 and r.bk == 32 and c.env.get("MCAMD_BK", "64") == "64":
        t.add("bk32-by-k_tap%64")
    chunks = c.ktot // r.bk
    if chunks < stages_of(r):
        t.add("chunks<stages")
    if r.kernel == PP and chunks == 8:
        t.add("pp-8-chunks")
    if mtiles > r.rows:
        t.add("persistent-walk")
    if c.choff > 0 and c.ld > c.choff + c.k_tap:
        t.add("x_choff>0" if c.fwd else "dy_choff>0")
    elif c.choff > 0:
        t.add("dy_choff>0" if not c.fwd else "x_choff-at-end")
    if c.y_choff > 0 and c.y_ld > c.y_choff + n:
        t.add("y_choff>0")
    t.add("shared-halo" if c.pad else "padded")
    t.add("1x1" if c.k == 1 else "3x3")
    if not c.fwd:
        t.add("dgrad-mask" if c.mask else "dgrad-no-mask")
        if c.concurrent:
            t.add("dgrad-concurrent")
    return t


# each of these on an igemm_kernel tile and on a ping-pong tile
BOUNDARIES_BOTH = ("M%bm!=0", "M%bm==0", "tile-spans-images", "HW<bm", "rows-shorter-than-tile", "n%bn!=0", "n%8!=0", "n<bn",
                   "k-padded", "persistent-walk", "x_choff>0", "y_choff>0", "dy_choff>0", "shared-halo", "padded", "1x1",
                   "3x3", "dgrad-mask", "dgrad-no-mask", "dgrad-concurrent")
# where it applies: the ping-pong tile needs M >= 256 (no single ragged tile), always has bk 32, and ktot >= 256 (8 chunks)
BOUNDARIES_IGEMM = ("M<bm", "bk32-by-k_tap%64", "chunks<stages")
BOUNDARIES_PP = ("pp-8-chunks",)


# ---------------------------------------------------------------------------------------------------------------------
# what the route rules can name
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_ENVS = ({}, {"MCAMD_PP": "0"}, {"MCAMD_BK": "32"}, {"MCAMD_SMALL3X3": "0"}, {"MCAMD_SMALL3X3": "2"}, {"MCAMD_WRES": "0"},
              {"MCAMD_WRES_MIN_ROUNDS": "0"}, {"MCAMD_PP": "2"}, {"MCAMD_PP": "2", "MCAMD_PP_BM": "192"},
              {"MCAMD_PP": "2", "MCAMD_PP_BN": "128"}, {"MCAMD_PP": "2", "MCAMD_PP_BM": "192", "MCAMD_PP_BN": "128"},
              {"MCAMD_PP": "2", "MCAMD_BK": "32", "MCAMD_SMALL3X3": "2", "MCAMD_WRES_MIN_ROUNDS": "0"})
# M from one ragged tile to > 65536: around 128 / 256 (tiles), 4096 (small3x3), 65536 (win3x3), the 512-tile rounds of the
# 192-row rule, the training batch at every resolution of the network; odd and even sizes, W % 16 == 0 and not
SWEEP_IMAGES = ((1, 8, 8), (4, 6, 6), (2, 13, 13), (1, 16, 16), (4, 26, 26), (1, 64, 64), (2, 48, 50), (8, 52, 52), (3, 104, 112),
                (5, 90, 90), (1, 256, 256), (2, 256, 208), (64, 13, 13), (32, 13, 13), (64, 26, 26), (64, 52, 52), (16, 104, 104),
                (64, 104, 104), (4, 208, 208), (64, 208, 208))
SWEEP_N = (8, 16, 24, 32, 40, 48, 56, 64, 72, 96, 120, 125, 128, 136, 192, 256, 264, 512, 1024, 1056, 1344)
SWEEP_K = (8, 32, 40, 64, 72, 96, 128, 256, 512, 1024, 1344)


def reachable(setenv):
    """{epilogue: set of (kernel, bm, bn, bk)} over every key of EPILOGUES, by asking the library: every switch setting of
    SWEEP_ENVS x SWEEP_IMAGES x both kernel sizes and the stem x the column counts SWEEP_N x the K-side channel counts
    SWEEP_K, and under the default switches every column count and every K-side channel count from 8 to 1344 in steps of
    8 (a tile is a function of the column count, the K-side count's padding and kernel size, M and the image shape)."""
    lib = L.lib()
    g = ops.geom(1, 8, 8, 3, 32, 32, 32)
    out = (C.c_int32 * 5)()
    ref = C.byref(g)
    fn = lib.mcamd_conv_route_info
    seen = {e: set() for e in EPILOGUES}

    def ask(B, H, W, k, n, kch, stem, epis):
        g.B, g.H, g.W, g.ksize, g.stem = B, H, W, k, stem
        for e in epis:
            d, mode, dst, stats = EPILOGUES[e]
            if (mode != L.EPI_NCHW_F32 and n % 8) or (dst != L.DST_PLAIN and (H % 2 or W % 2)):
                continue
            if d == ops.DIR_FWD:
                g.cin, g.cout = (3 if stem else kch), n
            elif stem:
                continue
            else:
                g.cin, g.cout = n, kch
            g.x_ld = 4 if stem else ops.round_up(g.cin, 32)
            rc = fn(ref, d, mode, dst, 1 if stats else 0, out)
            assert rc == 0, (B, H, W, k, n, kch, stem, e)
            seen[e].add((out[3], out[0], out[1], out[2]))

    every = tuple(EPILOGUES)
    for env in SWEEP_ENVS:
        for name, default in ENV_DEFAULTS.items():
            setenv(name, env.get(name, default))
        for (B, H, W) in SWEEP_IMAGES:
            for n in SWEEP_N:
                ask(B, H, W, 3, n, 3, 1, every)
                for kch in SWEEP_K:
                    for k in (1, 3):
                        ask(B, H, W, k, n, kch, 0, every)
    for name, default in ENV_DEFAULTS.items():
        setenv(name, default)
    for (B, H, W) in ((2, 13, 13), (3, 104, 112)):
        for n in range(8, 1345, 8):
            for kch in range(8, 1345, 8):
                for k in (1, 3):
                    ask(B, H, W, k, n, kch, 0, ("fwd-raw16-stats", "fwd-pad", "dgrad-raw16"))
    return seen


_REACHABLE = None


def reachable_cached(setenv):
    """reachable() once per process: the answer does not depend on anything a test changes."""
    global _REACHABLE
    if _REACHABLE is None:
        _REACHABLE = reachable(setenv)
    return _REACHABLE


# ---------------------------------------------------------------------------------------------------------------------
# operands and the exact reference (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
SLOPE = 0.125                     # a power of two: leaky() of the inference epilogue is exact
OVERFLOW_PLANT = 32.0             # 64 filters x 32 x 32 = 65536 > 65504


def _draw(gen, values, shape):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=gen)]


Operands = collections.namedtuple("Operands", "act w mask bias scale shift planted")


def operands(c, gaussian=False, plant=True):
    """act: x [B][cin][H][W] forward, dy [B][cout][H][W] dgrad; w OIHW; mask OIHW or None; bias (fwd-nchw), scale / shift
    (fwd-pad) per filter or None; planted: [(b, channel, h, w, sign)] of the elements an `overflow` case drives beyond the
    fp16 range."""
    # (seeded by the name up to its first ".": cases named "x.a", "x.b" of one shape and direction share activations and weights)
    gen = torch.Generator().manual_seed(zlib.crc32(c.name.split(".")[0].encode()))
    ach = c.cin if c.fwd else c.cout
    if gaussian:
        act = torch.randn(c.B, ach, c.H, c.W, generator=gen)
        w = torch.randn(c.cout, c.cin, c.k, c.k, generator=gen) * (2.0 / c.ktot) ** 0.5
    else:
        act = _draw(gen, (0, 1, 1, 2) if c.stem else DRAWS[c.draw], (c.B, ach, c.H, c.W))
        w = _draw(gen, DRAWS[c.wdraw], (c.cout, c.cin, c.k, c.k))
    mask = None
    if c.mask:
        mask = (torch.rand(c.cout, c.cin, c.k, c.k, generator=gen) > 0.3).float()          # scattered weights ...
        mask[torch.randperm(c.cout, generator=gen)[:max(1, c.cout // 8)]] = 0.0            # ... and whole filters removed
    bias = scale = shift = None
    if c.epi == "fwd-nchw":
        bias = torch.randint(-40, 41, (c.cout,), generator=gen).float()
    if c.epi == "fwd-pad":
        scale = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (c.cout,), generator=gen)]
        shift = torch.randint(-8, 9, (c.cout,), generator=gen).float() * 0.25
    planted = []
    if c.overflow:
        assert not c.fwd and c.k == 1 and c.cout == 64 and not c.mask
        w[:, 5] = OVERFLOW_PLANT
        if plant:
            act[0, :, 1, 2] = OVERFLOW_PLANT
            act[c.B - 1, :, c.H - 1, c.W - 2] = -OVERFLOW_PLANT
            planted = [(0, 5, 1, 2, 1.0), (c.B - 1, 5, c.H - 1, c.W - 2, -1.0)]
    return Operands(act, w, mask, bias, scale, shift, planted)


def reorg(x, stride=2):
    """Reorg(2) of the reference network (nets.py:648-667), as oracle/darknet_ref.py states it."""
    from oracle import darknet_ref as O
    return O.reorg(x, stride)


Reference = collections.namedtuple("Reference", "y y2 s1 s2 acc")
_BIG_ACC = {}


def reference(c, o):
    """The exact result of the launch.  y: what the output slice must hold, NCHW float64 (at the pooled resolution / with the
    reorg'ed channels for those destinations); y2: the full-resolution copy of "pool+y2"; s1, s2: the per-channel sums and
    sums of squares of the statistics epilogues; acc: the integer accumulators.  float32 for the one big case: it is exact
    under the same bound (condition 1) and faster."""
    big = c.M * c.n * c.ktot > 4e9
    key = (c.name.split(".")[0], c.fwd, c.B, c.H, c.W, c.k, c.cin, c.cout, c.mask, c.draw, c.wdraw)
    if big and key in _BIG_ACC:
        acc = _BIG_ACC[key]                          # the big cases of one tile share their operands: one convolution
    else:
        dt = torch.float32 if big else torch.float64
        w = o.w if o.mask is None else o.w * o.mask
        r = (c.k - 1) // 2
        if c.fwd:
            acc = F.conv2d(o.act.to(dt), w.to(dt), None, 1, r)
        else:
            acc = F.conv_transpose2d(o.act.to(dt), w.to(dt), None, 1, r)
        acc = acc.double()
        if big:
            _BIG_ACC.clear()
            _BIG_ACC[key] = acc
    y, y2, s1, s2 = acc, None, None, None
    if c.epi == "fwd-nchw":
        y = acc + o.bias.double().view(1, -1, 1, 1)
    elif c.epi == "fwd-pad":
        v = acc * o.scale.double().view(1, -1, 1, 1) + o.shift.double().view(1, -1, 1, 1)
        act = torch.where(v > 0, v, v * SLOPE)
        y = act
        if c.dst in ("pool", "pool+y2"):
            y = F.max_pool2d(act, 2, 2)
            y2 = act if c.dst == "pool+y2" else None
        elif c.dst == "reorg":
            y = reorg(act, 2)
    elif c.epi in ("fwd-raw16-stats", "fwd-raw32-stats"):
        s1, s2 = acc.sum((0, 2, 3)), (acc * acc).sum((0, 2, 3))
    if c.overflow:
        y = y.clone()
        for (b, ch, h, x, sign) in o.planted:
            assert abs(float(y[b, ch, h, x])) > 65504.0 and float(y[b, ch, h, x]) * sign > 0
            y[b, ch, h, x] = sign * 65504.0
    return Reference(y, y2, s1, s2, acc)


def exactness(c, o, ref):
    """The conditions under which the kernel output must EQUAL `ref`, as a list of violations (empty: all met).
    1. fp32 outputs: max|act| max|w| (taps x padded channels) + max|bias| < 2^24 -- every partial sum in every order is an
       integer that fp32 holds (the bias values are integers too).  Asserted for every case: the accumulators are fp32.
    2. fp16 outputs: every reference value is an fp16 number (the planted elements of an overflow case are +-65504).
    3. statistics: per channel, the sum of y^2 over ALL pixels is below 2^24, so every partial sum of y and of y^2 is an
       exact fp32 integer whatever pixels a slab row covers."""
    bad = []
    bound = float(o.act.abs().max()) * float(o.w.abs().max()) * c.ktot + (float(o.bias.abs().max()) if o.bias is not None else 0.0)
    if not bound < 2 ** 24:
        bad.append("condition 1: bound %r" % bound)
    if c.epi in ("fwd-raw16-stats", "fwd-raw16", "fwd-pad", "dgrad-raw16"):
        for t in (ref.y, ref.y2):
            if t is not None and not bool((t.half().double() == t).all()):
                bad.append("condition 2: %d values are no fp16 numbers, max |y| %r" % (int((t.half().double() != t).sum()), float(t.abs().max())))
    else:
        if not bool((ref.y.float().double() == ref.y).all()):
            bad.append("condition 2: the reference is no fp32 number")
    if ref.s2 is not None and not float(ref.s2.max()) < 2 ** 24:
        bad.append("condition 3: sum of y^2 over all pixels %r" % float(ref.s2.max()))
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
R16, R32, NCHW, PAD, D16, DNCHW, R16N = CASE_EPILOGUES
PP2 = {"MCAMD_PP": "2"}
PP2_192 = {"MCAMD_PP": "2", "MCAMD_PP_BM": "192"}
PP2_N128 = {"MCAMD_PP": "2", "MCAMD_PP_BN": "128"}
PP2_192_N128 = {"MCAMD_PP": "2", "MCAMD_PP_BM": "192", "MCAMD_PP_BN": "128"}
SMALL2 = {"MCAMD_SMALL3X3": "2"}
WRES0 = {"MCAMD_WRES_MIN_ROUNDS": "0"}

E = (IGEMM, 128, 32, 32)
CONV_CASES = [
    # ---- igemm_kernel<128, 32, .., 32, 3>: 32 columns; K chunks of 32 because the padded channel count is no multiple of 64
    case("i128x32k32-raw16", R16, 2, 9, 7, 1, 32, 32, E, draw="d3",
         tags=("M<bm", "tile-spans-images", "HW<bm", "chunks<stages", "bk32-by-k_tap%64", "1x1", "padded")),
    case("i128x32k32-raw32", R32, 2, 9, 7, 3, 72, 24, E, y_ld=40, y_choff=8, draw="d3",
         tags=("n<bn", "k-padded", "bk32-by-k_tap%64", "y_choff>0", "3x3")),
    case("i128x32k32-nchw", NCHW, 2, 9, 7, 1, 32, 29, E, ld=96, choff=32, draw="d3", tags=("n%8!=0", "x_choff>0", "chunks<stages")),
    case("i128x32k32-pad", PAD, 2, 10, 8, 3, 32, 32, E, pad=1, y_ld=64, y_choff=16, tags=("shared-halo", "y_choff>0", "M%bm!=0")),
    case("i128x32k32-dgrad16", D16, 2, 9, 7, 3, 32, 72, E, mask=True, ld=160, choff=32, draw="d3",
         tags=("dgrad-mask", "dy_choff>0", "k-padded", "bk32-by-k_tap%64")),
    case("i128x32k32-dgradnchw", DNCHW, 1, 16, 16, 1, 27, 32, E, draw="d3", tags=("n%8!=0", "M%bm==0", "dgrad-no-mask", "chunks<stages")),
    case("i128x32k32-raw16-33-columns-of-tiles", R16, 3, 53, 51, 1, 32, 1056, E, draw="d3", tags=("persistent-walk", "M%bm!=0")),
    case("i128x32k32-stem-form", R16, 2, 12, 20, 3, 3, 24, E, stem=1),
]

E = (IGEMM, 128, 32, 64)
CONV_CASES += [
    # ---- igemm_kernel<128, 32, .., 64, 2>
    case("i128x32k64-raw16", R16, 3, 13, 13, 3, 64, 96, E, tags=("M%bm!=0", "tile-spans-images", "rows-shorter-than-tile", "3x3")),
    case("i128x32k64-raw32", R32, 3, 13, 13, 1, 40, 96, E, draw="d3", tags=("k-padded", "chunks<stages")),
    case("i128x32k64-nchw", NCHW, 2, 13, 13, 3, 64, 93, E, draw="d3", tags=("n%8!=0", "n%bn!=0")),
    case("i128x32k64-pad", PAD, 2, 12, 12, 3, 64, 32, E, ld=160, choff=64, draw="d1", tags=("x_choff>0",)),
    case("i128x32k64-dgrad16", D16, 3, 13, 13, 3, 96, 64, E, pad=1, concurrent=True, tags=("shared-halo", "dgrad-concurrent", "dgrad-no-mask")),
    case("i128x32k64-dgradnchw", DNCHW, 3, 13, 13, 1, 96, 40, E, mask=True, ld=96, choff=32, draw="d3", tags=("dy_choff>0", "k-padded", "dgrad-mask")),
]

E = (IGEMM, 128, 64, 32)
CONV_CASES += [
    # ---- igemm_kernel<128, 64, .., 32, 3>; every destination form of the padded epilogue
    case("i128x64k32-raw16", R16, 2, 13, 13, 3, 32, 64, E, y_ld=96, y_choff=24, tags=("y_choff>0", "tile-spans-images")),
    case("i128x64k32-raw32", R32, 1, 12, 10, 1, 96, 48, E, draw="d3", tags=("M<bm", "n<bn", "bk32-by-k_tap%64")),
    case("i128x64k32-nchw", NCHW, 2, 13, 13, 3, 32, 61, E, pad=1, tags=("shared-halo", "n%8!=0")),
    case("i128x64k32-pad-plain", PAD, 2, 12, 14, 3, 32, 64, E, y_ld=96, y_choff=8, tags=("y_choff>0",)),
    case("i128x64k32-pad-pool", PAD, 2, 12, 14, 3, 32, 64, E, dst="pool", y_ld=96, y_choff=8),
    case("i128x64k32-pad-pool+y2", PAD, 2, 12, 14, 3, 72, 40, E, dst="pool+y2", y_ld=64, y_choff=16, draw="d1"),
    case("i128x64k32-pad-reorg", PAD, 2, 12, 14, 1, 96, 64, E, dst="reorg", y_ld=320, y_choff=32),
    case("i128x64k32-dgrad16", D16, 2, 13, 13, 1, 64, 32, E, mask=True, draw="d3", tags=("chunks<stages", "dgrad-mask")),
    case("i128x64k32-dgradnchw", DNCHW, 2, 13, 13, 3, 50, 96, E, tags=("n%8!=0", "n<bn")),
]

E = (IGEMM, 128, 64, 64)
CONV_CASES += [
    # ---- igemm_kernel<128, 64, .., 64, 2>: the few-tile rule at 128 columns
    case("i128x64k64-raw16", R16, 3, 13, 13, 1, 64, 128, E, draw="d3", tags=("chunks<stages", "1x1")),
    case("i128x64k64-raw32", R32, 2, 13, 13, 3, 128, 64, E),
    case("i128x64k64-nchw", NCHW, 2, 13, 13, 1, 128, 125, E, draw="d3", tags=("n%8!=0",)),
    case("i128x64k64-pad", PAD, 2, 13, 13, 3, 64, 128, E, ld=128, choff=32, draw="d1"),
    case("i128x64k64-dgrad16", D16, 2, 13, 13, 3, 128, 64, E, concurrent=True, tags=("dgrad-concurrent",)),
    case("i128x64k64-dgradnchw", DNCHW, 2, 13, 13, 1, 64, 128, E, draw="d3"),
    case("i128x64k64-dgrad16-overflow", D16, 2, 13, 13, 1, 64, 64, E, overflow=True),
]

E = (IGEMM, 128, 128, 32)
CONV_CASES += [
    # ---- igemm_kernel<128, 128, .., 32, 3>: 256 tiles of 128 x 128 or more
    case("i128x128k32-raw16", R16, 4, 64, 64, 1, 32, 256, E, tags=("M%bm==0", "chunks<stages")),
    case("i128x128k32-raw32", R32, 2, 91, 90, 1, 32, 256, E, tags=("M%bm!=0",)),
    case("i128x128k32-nchw", NCHW, 2, 91, 90, 1, 32, 253, E, tags=("n%8!=0", "n%bn!=0")),
    case("i128x128k32-pad", PAD, 4, 64, 64, 1, 64, 256, E, env={"MCAMD_BK": "32"}),
    case("i128x128k32-dgrad16", D16, 2, 91, 90, 1, 256, 32, E, mask=True),
    case("i128x128k32-dgradnchw", DNCHW, 2, 91, 90, 3, 256, 32, E, draw="d1"),
]

E = (IGEMM, 128, 128, 64)
CONV_CASES += [
    # ---- igemm_kernel<128, 128, .., 64, 2>
    case("i128x128k64-raw16", R16, 4, 64, 64, 1, 64, 256, E, draw="d1", tags=("M%bm==0", "chunks<stages")),
    case("i128x128k64-raw32", R32, 2, 91, 90, 3, 64, 256, E, draw="d1"),
    case("i128x128k64-nchw", NCHW, 2, 91, 90, 1, 64, 250, E, tags=("n%8!=0",)),
    case("i128x128k64-pad", PAD, 2, 91, 90, 1, 64, 256, E),
    case("i128x128k64-dgrad16", D16, 2, 91, 90, 1, 256, 64, E, concurrent=True),
    case("i128x128k64-dgradnchw", DNCHW, 4, 64, 64, 1, 256, 64, E, mask=True),
]

E = (IGEMM, 192, 128, 64)
CONV_CASES += [
    # ---- igemm_kernel<192, 128, 96, 64, 64, 2>: K >= 2048 and more than 512 tiles of 128 rows.  The heavy cases: the four
    # forward ones share one convolution on the CPU, the two dgrad ones another
    case("i192x128k64.raw16", R16, 3, 104, 106, 3, 256, 256, E, draw="s4", wdraw="s4u", tags=("M%bm!=0",)),
    case("i192x128k64.raw32", R32, 3, 104, 106, 3, 256, 256, E, draw="s4", wdraw="s4u"),
    case("i192x128k64.nchw", NCHW, 3, 104, 106, 3, 256, 256, E, draw="s4", wdraw="s4u"),
    case("i192x128k64.pad", PAD, 3, 104, 106, 3, 256, 256, E, draw="s4", wdraw="s4u"),
    case("i192x128k64.dgrad16", D16, 3, 104, 106, 3, 256, 256, E, draw="s4", wdraw="s4u"),
    case("i192x128k64.dgradnchw", DNCHW, 3, 104, 106, 3, 256, 256, E, draw="s4", wdraw="s4u"),
]

E = (PP, 256, 256, 32)
CONV_CASES += [
    # ---- igemm_pp_kernel, 256 x 256 (MCAMD_PP=2: whenever legal); every destination form of the padded epilogue
    case("pp256x256-raw16", R16, 1, 16, 16, 1, 256, 256, E, env=PP2, tags=("M%bm==0", "pp-8-chunks", "1x1")),
    case("pp256x256-raw32", R32, 2, 13, 13, 3, 40, 136, E, env=PP2, draw="d1", tags=("M%bm!=0", "tile-spans-images", "HW<bm", "n<bn", "k-padded", "3x3")),
    case("pp256x256-nchw", NCHW, 2, 13, 13, 1, 256, 253, E, env=PP2, pad=1, tags=("n%8!=0", "shared-halo")),
    case("pp256x256-pad-plain", PAD, 2, 14, 14, 3, 32, 256, E, env=PP2, y_ld=288, y_choff=16, tags=("y_choff>0",)),
    case("pp256x256-pad-pool", PAD, 2, 14, 14, 3, 32, 256, E, env=PP2, dst="pool"),
    case("pp256x256-pad-pool+y2", PAD, 2, 14, 14, 3, 32, 264, E, env=PP2, dst="pool+y2", draw="d1", y_ld=288, y_choff=8, tags=("n%bn!=0",)),
    case("pp256x256-pad-reorg", PAD, 2, 14, 14, 1, 256, 128, E, env=PP2, dst="reorg", y_ld=576, y_choff=64, draw="d1"),
    case("pp256x256-dgrad16", D16, 2, 13, 13, 3, 264, 32, E, env=PP2, mask=True, ld=96, choff=64, tags=("n%bn!=0", "dgrad-mask", "dy_choff>0")),
    case("pp256x256-dgradnchw", DNCHW, 3, 13, 13, 1, 253, 256, E, env=PP2, tags=("n%8!=0", "dgrad-no-mask")),
]

E = (PP, 192, 256, 32)
CONV_CASES += [
    # ---- igemm_pp_kernel, 192 x 256
    case("pp192x256-raw16", R16, 2, 16, 12, 3, 32, 256, E, env=PP2_192, y_ld=320, y_choff=32, tags=("M%bm==0", "y_choff>0")),
    case("pp192x256-raw32", R32, 2, 13, 13, 1, 256, 264, E, env=PP2_192, ld=320, choff=32, tags=("x_choff>0", "n%bn!=0", "pp-8-chunks")),
    case("pp192x256-nchw", NCHW, 2, 13, 13, 3, 72, 131, E, env=PP2_192, draw="d1", tags=("n%8!=0", "n<bn", "k-padded")),
    case("pp192x256-pad", PAD, 2, 13, 13, 3, 32, 256, E, env=PP2_192, pad=1),
    case("pp192x256-dgrad16", D16, 2, 13, 13, 1, 256, 256, E, env=PP2_192, pad=1, concurrent=True, tags=("shared-halo", "dgrad-concurrent")),
    case("pp192x256-dgradnchw", DNCHW, 2, 13, 13, 3, 256, 40, E, env=PP2_192, mask=True, draw="d1", tags=("k-padded",)),
]

E = (PP, 256, 128, 32)
CONV_CASES += [
    # ---- igemm_pp_kernel, 256 x 128
    case("pp256x128-raw16", R16, 2, 13, 13, 3, 32, 136, E, env=PP2_N128, tags=("n%bn!=0",)),
    case("pp256x128-raw32", R32, 1, 16, 16, 1, 256, 128, E, env=PP2_N128),
    case("pp256x128-nchw", NCHW, 3, 13, 13, 1, 256, 125 + 128, E, env=PP2_N128),
    case("pp256x128-pad", PAD, 2, 13, 13, 1, 256, 128, E, env=PP2_N128, draw="d1"),
    case("pp256x128-dgrad16", D16, 2, 13, 13, 3, 128, 32, E, env=PP2_N128),
    case("pp256x128-dgradnchw", DNCHW, 2, 13, 13, 1, 131, 256, E, env=PP2_N128, tags=("n%8!=0",)),
]

E = (PP, 192, 128, 32)
CONV_CASES += [
    # ---- igemm_pp_kernel, 192 x 128
    case("pp192x128-raw16", R16, 2, 13, 13, 1, 256, 128, E, env=PP2_192_N128),
    case("pp192x128-raw16-8-columns-of-tiles", R16, 3, 46, 45, 1, 256, 1024, E, env=PP2_192_N128, draw="d1", tags=("persistent-walk", "M%bm!=0")),
    case("pp192x128-raw32", R32, 2, 13, 13, 3, 32, 128, E, env=PP2_192_N128),
    case("pp192x128-nchw", NCHW, 2, 13, 13, 1, 256, 135, E, env=PP2_192_N128),
    case("pp192x128-pad", PAD, 2, 13, 13, 3, 64, 128, E, env=PP2_192_N128, draw="d1"),
    case("pp192x128-dgrad16", D16, 2, 13, 13, 1, 128, 256, E, env=PP2_192_N128),
    case("pp192x128-dgradnchw", DNCHW, 2, 13, 13, 3, 128, 64, E, env=PP2_192_N128, draw="d1"),
]

CONV_CASES += [
    # ---- small3x3_kernel<CT, NB>: no LDS staging, M >= 4096, at most 64 columns.  The route's (bn, bk) = (round_up(n, 32), CT);
    # NB = 1 / 2 / 4 blocks of 16 columns for n <= 16 / <= 32 / <= 64
    case("small32-nb1-raw16", R16, 1, 70, 61, 3, 24, 16, (SMALL, 32, 32, 32)),
    case("small32-nb2-raw16", R16, 2, 48, 48, 3, 32, 24, (SMALL, 32, 32, 32), draw="d1", ld=64, choff=32, y_ld=40, y_choff=8),
    case("small32-nb4-raw16", R16, 1, 70, 61, 3, 32, 64, (SMALL, 32, 64, 32), draw="d1", pad=1),
    case("small64-nb1-raw16", R16, 1, 70, 61, 3, 64, 8, (SMALL, 32, 32, 64), env=SMALL2, draw="d1"),
    case("small64-nb2-raw16", R16, 2, 48, 50, 3, 40, 32, (SMALL, 32, 32, 64), env=SMALL2, draw="d1"),
    case("small32-nb1-dgrad16", D16, 1, 70, 61, 3, 16, 32, (SMALL, 32, 32, 32), mask=True),
    case("small32-nb2-dgrad16", D16, 2, 48, 48, 3, 32, 24, (SMALL, 32, 32, 32), ld=64, choff=32),
    case("small32-nb4-dgrad16", D16, 1, 70, 61, 3, 40, 32, (SMALL, 32, 64, 32), pad=1, y_ld=64, y_choff=8),
    case("small64-nb1-dgrad16", D16, 2, 48, 50, 3, 16, 64, (SMALL, 32, 32, 64), env=SMALL2, draw="d1"),
    case("small64-nb2-dgrad16", D16, 1, 70, 61, 3, 32, 40, (SMALL, 32, 32, 64), env=SMALL2, draw="d1", mask=True),
    # ---- win3x3_kernel<NB>: rolling LDS window, M >= 65536, 64 padded K-side channels, at most 32 columns, fp16 rows without
    # statistics -- the input gradient of the second layer, and a forward launch of that shape that takes no statistics
    case("win-nb2-dgrad16", D16, 4, 128, 144, 3, 32, 64, (WIN, 32, 32, 64), draw="d1"),
    case("win-nb2-dgrad16-ragged", D16, 2, 168, 208, 3, 24, 48, (WIN, 32, 32, 64), draw="d1", mask=True, ld=96, choff=32, y_ld=32),
    case("win-nb1-dgrad16", D16, 2, 168, 208, 3, 16, 64, (WIN, 32, 16, 64), draw="d1", pad=1),
    case("win-nb2-raw16-no-stats", R16N, 4, 128, 144, 3, 64, 32, (WIN, 32, 32, 64), draw="d1"),
    case("win-nb1-raw16-no-stats", R16N, 2, 168, 208, 3, 40, 8, (WIN, 32, 16, 64), draw="d1", y_ld=16, y_choff=8),
    # ---- wres_kernel: weights resident in registers, tiles of 128 PADDED pixels (plain destinations only: the pooled forms
    # of the same layer go to igemm_kernel)
    case("wres-raw16", R16, 3, 40, 36, 3, 64, 128, (WRES, 128, 128, 64), env=WRES0, draw="d1", y_ld=136, y_choff=8),
    case("wres-raw16-ragged", R16, 2, 27, 104, 3, 48, 264, (WRES, 128, 128, 64), env=WRES0, draw="d1", ld=128, choff=64),
    case("wres-pad", PAD, 5, 21, 13, 3, 64, 192, (WRES, 128, 128, 64), env=WRES0, draw="d1", y_ld=320, y_choff=32),
    # ---- stem_fwd_kernel<1, 4> / <2, 4>: the first layer, weights in registers
    case("stem32-raw16", R16, 2, 32, 48, 3, 3, 32, (STEM, 32, 32, 48), stem=1),
    case("stem64-raw16", R16, 3, 33, 17, 3, 3, 64, (STEM, 32, 64, 48), stem=1, y_ld=72, y_choff=8),
]

# one igemm_kernel tile, small3x3, win3x3, wres and the stem: run twice on Gaussian data, bit-equal
DETERMINISM_CASES = ("i128x64k32-raw16", "small32-nb4-raw16", "win-nb2-dgrad16", "wres-raw16", "stem64-raw16")
