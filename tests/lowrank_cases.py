"""The cases of tests/test_lowrank_instances_gpu.py: launches of mcamd_conv_fwd_lowrank (csrc/conv_lowrank.hip: the four
instances lowrank_kernel<64> / <128> / <192> / <256>), their operands and the exact float64 reference of the contract of
include/mcamd.h, and the enumeration of what the launch can choose.

test_lowrank_cases_cpu.py proves on the CPU (through mcamd_conv_fwd_lowrank_info, which is answered by the launch's own
mcamd_lowrank_choice()) that LOWRANK_CASES reaches every instance with its padded and its unpadded rank, both kernel sizes,
both K orders, every destination form and every named boundary condition, that every case's reference meets the conditions
of exactness, and that every K chunk of either GEMM is visible in every tile; test_lowrank_instances_gpu.py runs each case
against that reference.  Test-side only.

Why EQUAL is the comparison: the operands are small integers with max|x| max|U| Ktot < 2^24, so H before its rounding is an
integer that every order of the fp32 sum reaches exactly; H as rounded (and saturated) is an integer again, V holds integers
(or, in one column of one case, 2^-6) and the sum over j of |H[m][j] V[n][j]| stays below 2^24 units of the smallest term,
so Y is exact in every order too; Y * scale + shift is an fp32 number (asserted per case), so the one rounding left is the
final one to fp16, which the reference performs on the exact value."""
import collections
import functools
import types
import zlib

import torch
import torch.nn.functional as F

from modelcompression_amd import ops
from modelcompression_amd import _lib as L
import splitk_cases as SK
from conv_cases import _draw, DRAWS, SLOPE, reorg, OVERFLOW_PLANT  # noqa: F401  (shared with the dense cases)

DST = {"plain": L.DST_PLAIN, "pool": L.DST_POOL, "pool+y2": L.DST_POOL, "reorg": L.DST_REORG}
FORMS = tuple(DST)
INSTANCES = (64, 128, 192, 256)           # lowrank_kernel<R>: rank_padded of mcamd_conv_fwd_lowrank_info
RANKS = tuple(range(32, 257, 32))
BM, BN, BK = 64, 128, 32                  # pixels per workgroup, filters per N tile of phase 2, K chunk of both phases
F16_MAX = 65504.0


# ---------------------------------------------------------------------------------------------------------------------
# the reference (moved here from test_lowrank_kernels_gpu.py, which imports it back)
# ---------------------------------------------------------------------------------------------------------------------
def reference(c, x=None, clamp_h=True):
    """(full-resolution fp16 output, the float64 intermediate before its rounding, whether either had to be clamped).
    clamp_h=False: the intermediate keeps the values beyond the fp16 range as they are (what a kernel without sat_half and
    with an unbounded format would compute) -- only to show that the clamp of H is visible in the output."""
    h = F.conv2d((c.x if x is None else x).double(), c.u.double(), padding=c.k // 2)
    hh = h.clamp(-65504.0, 65504.0).half().double()
    if not clamp_h:
        hh = torch.where(h.abs() > 65504.0, h, hh)
    scale = torch.ones(c.cout) if c.scale is None else c.scale
    shift = torch.zeros(c.cout) if c.shift is None else c.shift
    z = F.conv2d(hh, c.v.double().view(c.cout, c.r, 1, 1)) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    z = torch.where(z > 0, z, z * SLOPE)
    return z.clamp(-65504.0, 65504.0).half(), h, bool((z.abs() > 65504).any() or (h.abs() > 65504).any())


def destinations(c, ref):
    """full-resolution fp16 reference -> what [y] or [y, y2] must hold"""
    return {"plain": lambda: [ref], "pool": lambda: [F.max_pool2d(ref.float(), 2, 2).half()], "reorg": lambda: [reorg(ref)],
            "pool+y2": lambda: [F.max_pool2d(ref.float(), 2, 2).half(), ref]}[c.dst]()


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
_FIELDS = "name B H W k cin cout r dst x_ld x_choff y_ld y_choff y2_ld y2_choff draws absolute no_scale plant expect tags"


class Case(collections.namedtuple("Case", _FIELDS)):
    """One launch of mcamd_conv_fwd_lowrank.
    x_ld / x_choff: the operand slice; y_ld / y_choff: the output slice; y2_ld / y2_choff: that of the full-resolution copy
    of "pool+y2".  draws: conv_cases.DRAWS keys of (x, U, V); absolute: x and U are drawn non-negative (H beyond fp16's exact
    integers; V is sparse and the scales at most 1/2).  no_scale: the launch passes scale = None.  plant: None, or which of the three saturation arrangements the
    case carries ("h", "y", "both"); its twin "<name>.twin" has the same operands without the plant.
    expect: (rank_padded, mtiles, ntiles, grid) of mcamd_conv_fwd_lowrank_info.  tags: the boundary conditions the case was
    written for, each re-derived from the info query by boundary_tags().
    The part of the name in front of the first "." seeds the operands."""
    __slots__ = ()

    def __str__(self):
        return self.name

    @property
    def base(self):
        return self.name.split(".")[0]

    @property
    def twin(self):
        return self.name.endswith(".twin")

    @property
    def pooled(self):
        """the M tile is enumerated in pooled order (four consecutive rows = one 2x2 window)"""
        return self.dst != "plain"

    @property
    def M(self):
        return self.B * self.H * self.W

    @property
    def k_tap(self):
        """padded operand channels per tap (cin_tap)"""
        return ops.round_up(self.cin, 32)

    @property
    def kb(self):
        """channel block of the packed K order [channel block][tap][kb] (kblock_of)"""
        return 64 if self.k_tap % 64 == 0 else 32

    @property
    def ntaps(self):
        return self.k * self.k

    @property
    def ktot(self):
        return self.ntaps * self.k_tap

    @property
    def cdst(self):
        return 4 * self.cout if self.dst == "reorg" else self.cout

    @property
    def instance(self):
        return self.expect[0]


def case(name, B, H, W, k, cin, cout, r, dst, draws, x_slice=None, y_slice=None, y2_slice=None, absolute=False, no_scale=False,
         plant=None, tags=()):
    assert dst in DST and (dst == "plain" or (H % 2 == 0 and W % 2 == 0)) and (y2_slice is None or dst == "pool+y2")
    x_ld, x_choff = x_slice or (ops.round_up(cin, 32), 0)
    cdst = 4 * cout if dst == "reorg" else cout
    y_ld, y_choff = y_slice or (ops.round_up(cdst, 8), 0)
    y2_ld, y2_choff = y2_slice or ((y_ld, y_choff) if dst == "pool+y2" else (0, 0))
    M = B * H * W
    mtiles = -(-M // BM)
    expect = (ops.round_up(r, 64), mtiles, -(-cout // BN), ops.round_up(mtiles, 8))
    return Case(name, B, H, W, k, cin, cout, r, dst, x_ld, x_choff, y_ld, y_choff, y2_ld, y2_choff, tuple(draws), absolute, no_scale,
                plant, expect, tuple(tags))


def geom_of(c):
    return ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, c.x_ld, c.x_choff)


def info_of(c):
    return ops.conv_fwd_lowrank_info(geom_of(c), c.r)


def expect_of(info):
    return (info.rank_padded, info.mtiles, info.ntiles, info.grid)


def boundary_tags(c, info):
    """The named boundary conditions this launch meets, from the info query and the case's shape alone."""
    t = set()
    M, HW = c.M, c.H * c.W
    # ---- the pixel axis: tiles of 64 rows, dealt round the 8 XCDs in rounds of 8 (xcd_tile)
    if M % info.bm == 0:
        t.add("M%64==0")
    if M % info.bm == 1:
        t.add("M%64==1")
    if info.mtiles > 8:
        t.add("mtiles>8")                          # xcd_tile's second round: jb = 1
        if info.grid > info.mtiles:
            t.add("second-round-padded")           # ... with blocks that return early in it
        if c.pooled:
            t.add("mtiles>8-pooled")
    if c.B > 1 and HW % info.bm:
        t.add("tile-spans-images-pooled" if c.pooled else "tile-spans-images")
    # ---- the filter axis: N tiles of 128, K chunks of 32 rank columns
    if c.cout < info.bn:
        t.add("n<bn")
    if c.cout == info.bn:
        t.add("n==bn")
    if c.cout == info.bn + 8:
        t.add("n==bn+8")
    if c.r == BK and info.ntiles > 1:
        t.add("kc2==1,ntiles>1")                   # every ring item of phase 2 ends a tile
    if c.r == BK and info.ntiles == 4:
        t.add("kc2==1,ntiles==4")
    # ---- the K order and the operand forms
    t.add("kb64" if c.kb == 64 else "kb32")
    if c.kb == 64 and c.k_tap == 128:
        t.add("kb64-two-blocks")
    if c.kb == 32 and c.k_tap == 96:
        t.add("kb32-three-blocks")
    t.add("1x1" if c.k == 1 else "3x3")
    if c.k_tap > c.cin:
        t.add("ragged-cin-kb%d" % c.kb)
    t.add("rank-padded" if info.rank_padded > c.r else "rank-unpadded")
    if c.x_choff > 0 and c.x_ld > c.x_choff + c.k_tap:
        t.add("x_choff>0")
        if c.dst in ("pool", "pool+y2"):
            t.add("x_choff>0-pool")
        if c.dst == "reorg":
            t.add("x_choff>0-reorg")
    if c.y_choff > 0 and c.y_ld > c.y_choff + c.cdst:
        t.add("y_choff>0")
        if c.dst in ("pool", "pool+y2"):
            t.add("y_choff>0-pool")
        if c.dst == "reorg":
            t.add("y_choff>0-reorg")
    if c.dst == "pool+y2" and (c.y2_ld, c.y2_choff) != (c.y_ld, c.y_choff) and c.y2_choff > 0 and c.y2_ld > c.y2_choff + c.cout:
        t.add("y2-own-slice")
    if c.no_scale:
        t.add("scale-none")
    if c.plant and not c.twin:
        t.add("sat-" + c.plant)
        if c.plant == "both" and M % info.bm and c.cout % info.bn:
            t.add("sat-in-tail-tile")              # (the planted pixel lies in the last tile: operands())
    return t


BOUNDARIES = ("M%64==0", "M%64==1", "mtiles>8", "second-round-padded", "mtiles>8-pooled", "tile-spans-images",
              "tile-spans-images-pooled", "n<bn", "n==bn", "n==bn+8", "kc2==1,ntiles>1", "kc2==1,ntiles==4", "kb64", "kb32",
              "kb64-two-blocks", "kb32-three-blocks", "1x1", "3x3", "ragged-cin-kb64", "ragged-cin-kb32", "rank-padded",
              "rank-unpadded", "x_choff>0-pool", "x_choff>0-reorg", "y_choff>0-pool", "y_choff>0-reorg", "y2-own-slice",
              "scale-none", "sat-h", "sat-y", "sat-both", "sat-in-tail-tile")

I1, I13, P2, P16, T65, B4 = (1, 8, 8), (1, 13, 13), (2, 6, 6), (16, 6, 6), (1, 5, 13), (4, 13, 13)
_BASE = [
    # ---- lowrank_kernel<64>: ranks 64 and 32; waves 2 x 2, wave tile 32 pixels x 32 columns
    case("r64-plain-k3-c64", *I1, 3, 64, 128, 64, "plain", ("d1", "d2", "d2"), tags=("M%64==0", "n==bn", "kb64", "3x3", "rank-unpadded")),
    case("r32-pool-k1-c96", *P2, 1, 96, 72, 32, "pool", ("d2", "d2", "d2"), x_slice=(160, 32), y_slice=(96, 16),
         tags=("kb32-three-blocks", "1x1", "rank-padded", "x_choff>0-pool", "y_choff>0-pool", "tile-spans-images-pooled")),
    case("r32-pool+y2-k3-c128", *P2, 3, 128, 136, 32, "pool+y2", ("d1", "d1", "d2"), y_slice=(160, 8), y2_slice=(192, 40),
         tags=("kb64-two-blocks", "y2-own-slice", "kc2==1,ntiles>1", "n==bn+8")),
    case("r64-reorg-k3-c96", *P2, 3, 96, 8, 64, "reorg", ("d1", "d2", "d2"), tags=("n<bn", "kb32")),
    case("r32-plain-k3-c64-n392", *B4, 3, 64, 392, 32, "plain", ("d1", "d2", "d2"),
         tags=("mtiles>8", "second-round-padded", "kc2==1,ntiles==4", "tile-spans-images")),
    # ---- lowrank_kernel<128>: ranks 128 and 96; waves 1 x 4, wave tile 64 pixels x 32 columns
    case("r128-plain-k1-c128", *I13, 1, 128, 136, 128, "plain", ("d2", "d2", "d1"), tags=("n==bn+8", "kb64-two-blocks", "1x1", "rank-unpadded")),
    case("r96-pool-k3-c64", *P16, 3, 64, 72, 96, "pool", ("d1", "d2", "d2"), tags=("mtiles>8-pooled", "tile-spans-images-pooled", "rank-padded", "3x3")),
    case("r128-pool+y2-k3-c96", *P2, 3, 96, 136, 128, "pool+y2", ("d1", "d2", "d1"), tags=("kb32-three-blocks",)),
    case("r96-reorg-k1-c64", *P2, 1, 64, 72, 96, "reorg", ("d2", "d2", "d2"), x_slice=(128, 32), y_slice=(320, 16),
         tags=("x_choff>0-reorg", "y_choff>0-reorg", "kb64")),
    case("r96-plain-k3-c40", *I13, 3, 40, 72, 96, "plain", ("d2", "d2", "d2"), x_slice=(96, 16), tags=("ragged-cin-kb64",)),
    # ---- lowrank_kernel<192>: ranks 192 and 160; waves 2 x 2, wave tile 32 pixels x 96 columns (TN = 3)
    case("r192-plain-k3-c128", *B4, 3, 128, 136, 192, "plain", ("d1", "d1", "d1"),
         tags=("mtiles>8", "second-round-padded", "kb64-two-blocks", "3x3", "rank-unpadded", "tile-spans-images")),
    case("r160-pool-k1-c96", *P2, 1, 96, 72, 160, "pool", ("d2", "d2", "d1"), tags=("kb32-three-blocks", "1x1", "rank-padded")),
    case("r160-pool+y2-k3-c64", *P16, 3, 64, 264, 160, "pool+y2", ("d1", "d2", "d1"), y_slice=(288, 8), y2_slice=(320, 32),
         tags=("mtiles>8-pooled", "y2-own-slice", "kb64")),
    case("r192-reorg-k3-c96", *P2, 3, 96, 8, 192, "reorg", ("d1", "d2", "d1"), tags=("n<bn", "kb32")),
    case("r160-plain-k1-c64-tail1", *T65, 1, 64, 8, 160, "plain", ("d2", "d2", "d1"), tags=("M%64==1", "n<bn")),
    case("r192-plain-k1-c64-noscale", *I1, 1, 64, 128, 192, "plain", ("d2", "d2", "d1"), no_scale=True, tags=("scale-none", "M%64==0", "n==bn")),
    # ---- lowrank_kernel<256>: ranks 256 and 224; waves 1 x 4, wave tile 64 pixels x 64 columns
    case("r224-plain-k3-c64", *I13, 3, 64, 136, 224, "plain", ("d1", "d2", "d1"), tags=("rank-padded", "kb64", "3x3")),
    case("r256-pool-k3-c96", *P2, 3, 96, 72, 256, "pool", ("d1", "d2", "d1"), tags=("kb32-three-blocks", "rank-unpadded")),
    case("r224-pool+y2-k1-c128", *P2, 1, 128, 264, 224, "pool+y2", ("d2", "d2", "d1"), tags=("kb64-two-blocks", "1x1")),
    case("r256-reorg-k1-c96", *P2, 1, 96, 72, 256, "reorg", ("d2", "d2", "d1"), tags=("kb32",)),
    case("r224-plain-k3-c72", *I13, 3, 72, 72, 224, "plain", ("d1", "d2", "d1"), tags=("ragged-cin-kb32",)),
    # all-positive draws: H is 864 x 1.6 x 1.6 = 2 300 on average -- the large-valued launch in front of test_no_history's
    # small-rank ones, and a rounding of H that shows
    case("r256-plain-k3-c96-bigH", *I13, 3, 96, 136, 256, "plain", ("d3", "d3", "s4"), absolute=True, tags=("kb32-three-blocks",)),
    # ---- saturation: 64 channels x 32 x 32 = 65536 at one pixel and one U row (operands())
    # (a) H alone clamps: that V column is 2^-6
    case("sat-h-r160-k3-c64", *I13, 3, 64, 72, 160, "plain", ("d1", "d2", "d1"), plant="h", tags=("sat-h",)),
    # (b) an output alone clamps, through the scale 2^12 of one filter
    case("sat-y-r128-k1-c128", *I13, 1, 128, 136, 128, "plain", ("d1", "d2", "d1"), plant="y", tags=("sat-y",)),
    # (c) both clamp, at a pixel of the tail tile (41 real rows, 23 pad rows), 72 of 128 filters
    case("sat-both-r64-k3-c64", *I13, 3, 64, 72, 64, "plain", ("d1", "d2", "d2"), plant="both", tags=("sat-both", "sat-in-tail-tile")),
]
LOWRANK_CASES = _BASE + [c._replace(name=c.name + ".twin", tags=()) for c in _BASE if c.plant]
BY_NAME = {c.name: c for c in LOWRANK_CASES}

NO_HISTORY = ("r256-plain-k3-c96-bigH", "r32-pool-k1-c96", "r160-pool+y2-k3-c64")     # large values at rank 256, then 32, then 160
DETERMINISM_CASES = ("r64-reorg-k3-c96", "r96-pool-k3-c64", "r192-plain-k3-c128", "r224-pool+y2-k1-c128")

# the planted arrangement
PLANT_ROW = 5                                      # the U row / H column / V column
PLANT_PIXEL = (11, 7)                              # pixel 150 of 169: in the tail tile (rows 128 .. 168)
PLANT_FILTER, PLANT_SCALE = 3, 4096.0              # (b)


# ---------------------------------------------------------------------------------------------------------------------
# operands and the exact reference (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def operands(name):
    """What test_lowrank_kernels_gpu.launch() reads: the case's fields and x [B][cin][H][W], u [r][cin][k][k], v [cout][r],
    scale / shift per filter (scale None for a no_scale case).  Once per process and case; shared and never modified."""
    c = BY_NAME[name]
    gen = torch.Generator().manual_seed(zlib.crc32(c.base.encode()))
    x, u, v = (_draw(gen, DRAWS[d], s) for d, s in zip(c.draws, ((c.B, c.cin, c.H, c.W), (c.r, c.cin, c.k, c.k), (c.cout, c.r))))
    scale = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (c.cout,), generator=gen)]
    if c.absolute:                                 # (sums of 64 values of +-2 300: small scales keep the outputs in range)
        x, u, scale = x.abs(), u.abs(), scale.clamp(max=0.5)
    shift = torch.randint(-8, 9, (c.cout,), generator=gen).float() * 0.25
    if c.plant in ("h", "both"):
        assert c.cin >= 64
        u[PLANT_ROW] = 0.0
        u[PLANT_ROW, :64, c.k // 2, c.k // 2] = OVERFLOW_PLANT
        v[:, PLANT_ROW] = 2.0 ** -6 if c.plant == "h" else 2.0
        if not c.twin:
            x[0, :64, PLANT_PIXEL[0], PLANT_PIXEL[1]] = OVERFLOW_PLANT
    if c.plant == "y" and not c.twin:
        scale[PLANT_FILTER] = PLANT_SCALE
    o = types.SimpleNamespace(**c._asdict())
    o.case, o.x, o.u, o.v, o.scale, o.shift = c, x, u, v, (None if c.no_scale else scale), shift
    return o


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """(what [y] or [y, y2] must hold, the float64 H before its rounding, clamped, the full-resolution fp16 output)"""
    o = operands(name)
    ref, h, clamped = reference(o)
    return destinations(o, ref), h, clamped, ref


def gaussian(c):
    """Gaussian operands on the case's shape: sums that DO depend on their order"""
    gen = torch.Generator().manual_seed(zlib.crc32(c.base.encode()))
    o = types.SimpleNamespace(**c._asdict())
    o.case = c
    o.x = torch.randn(c.B, c.cin, c.H, c.W, generator=gen).half().float()
    o.u = (torch.randn(c.r, c.cin, c.k, c.k, generator=gen) * (2.0 / c.ktot) ** 0.5).half().float()
    o.v = (torch.randn(c.cout, c.r, generator=gen) * (2.0 / c.r) ** 0.5).half().float()
    o.scale, o.shift = torch.rand(c.cout, generator=gen) + 0.5, torch.randn(c.cout, generator=gen) * 0.2
    return o


# ---------------------------------------------------------------------------------------------------------------------
# both GEMMs restated: rows in the launch's pixel order, columns in the packed K order / the rank order
# ---------------------------------------------------------------------------------------------------------------------
def sat_half(h):
    return h.clamp(-F16_MAX, F16_MAX).half().double()


def in_row_order(c, t):
    """[B][ch][H][W] -> [M][ch] in the launch's pixel order (conv_epi.h: tile_pixel)"""
    return t.permute(0, 2, 3, 1).reshape(c.M, t.shape[1])[SK.row_pixels(c)]


def phase1_chunks(c, o):
    """float64 [ktot / 32][M][r]: the contribution of every K chunk of 32 packed values to H"""
    X, Up = SK.gemm_operands(c, o.x, o.u)
    n = c.ktot // BK
    return torch.einsum("mqk,jqk->qmj", X.double().view(c.M, n, BK), Up.double().view(c.r, n, BK))


def phase2_chunks(c, o, h):
    """float64 [r / 32][M][cout]: the contribution of every chunk of 32 rank columns of the rounded H to Y"""
    hs = in_row_order(c, sat_half(h))
    n = c.r // BK
    return torch.einsum("mqj,nqj->qmn", hs.view(c.M, n, BK), o.v.double().view(c.cout, n, BK))


# ---------------------------------------------------------------------------------------------------------------------
# what the launch can choose
# ---------------------------------------------------------------------------------------------------------------------
def reachable():
    """set of rank_padded over ranks 32 .. 256 x both kernel sizes x every input-channel count from 8 to 1024 and every filter
    count from 8 to 1344 in steps of 8, by asking the library; every answer's tiles and grid are checked on the way."""
    import ctypes as C
    fn = L.lib().mcamd_conv_fwd_lowrank_info
    B, H, W = 4, 13, 13
    g = ops.geom(B, H, W, 3, 32, 32, 32)
    info = L.LowrankInfo()
    ref, out = C.byref(g), C.byref(info)
    mtiles = -(-B * H * W // BM)
    seen = set()
    for k in (1, 3):
        g.ksize = k
        for cin in range(8, 1025, 8):
            g.cin, g.x_ld = cin, ops.round_up(cin, 32)
            for cout in range(8, 1345, 8):
                g.cout = cout
                for r in RANKS:
                    assert fn(ref, r, out) == 0, (k, cin, cout, r)
                    assert (info.bm, info.bn, info.bk, info.stages) == (BM, BN, BK, 3)
                    assert (info.rank_padded, info.mtiles, info.ntiles, info.grid) == (ops.round_up(r, 64), mtiles, -(-cout // BN), 16)
                    seen.add(info.rank_padded)
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# one-hot tables: which k every operand lane selects and where the hand-over puts every H column
# ---------------------------------------------------------------------------------------------------------------------
OneHot = collections.namedtuple("OneHot", "k cin")
# a 3 x 3 image, channel c of pixel p holds 9 c + p + 1; one filter per real (channel, tap) in a shuffled order, in batches of
# at most 256 (one launch each, cout = r, V the identity); the last batch is filled with zero filters to a multiple of 32
ONEHOT_CASES = [OneHot(k, cin) for k in (1, 3) for cin in (64, 128, 96, 40)]


def onehot_id(h):
    return "k%d-cin%d" % (h.k, h.cin)


@functools.lru_cache(maxsize=None)
def onehot_operands(h):
    """(x [1][cin][3][3], U of all filters [k k cin][cin][k][k], [(channel, tap)] per filter, [launch operands per batch]).
    Every value stays below 2048: exact in fp16."""
    gen = torch.Generator().manual_seed(zlib.crc32(("onehot-" + onehot_id(h)).encode()))
    ntaps, total = h.k * h.k, h.k * h.k * h.cin
    x = torch.arange(h.cin, dtype=torch.float32).view(1, -1, 1, 1) * 9.0 + torch.arange(9, dtype=torch.float32).view(1, 1, 3, 3) + 1.0
    order = torch.randperm(total, generator=gen).tolist()
    u = torch.zeros(total, h.cin, h.k, h.k)
    which = []
    for f in range(total):
        chan, tap = divmod(order[f], ntaps)
        u[f, chan, tap // h.k, tap % h.k] = 1.0
        which.append((chan, tap))
    batches = []
    for f0 in range(0, total, 256):
        ub = u[f0:f0 + 256]
        r = ops.round_up(ub.shape[0], 32)
        ub = torch.cat([ub, torch.zeros(r - ub.shape[0], h.cin, h.k, h.k)])
        c = case("onehot-%s.b%d" % (onehot_id(h), f0 // 256), 1, 3, 3, h.k, h.cin, r, r, "plain", ("d1", "d1", "d1"))
        o = types.SimpleNamespace(**c._asdict())
        o.case, o.x, o.u, o.v, o.scale, o.shift, o.f0 = c, x, ub, torch.eye(r), None, None, f0
        batches.append(o)
    return x, u, which, batches
