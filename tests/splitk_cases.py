"""The cases of tests/test_splitk_instances_gpu.py: launches of mcamd_conv_fwd_splitk (csrc/conv_splitk.hip: the partial
kernels splitk_partial_kernel<64, 3> / <32, 4> and the finish kernels splitk_finish_kernel<PAD> / <RAW>), their operands
and exact references, and the enumeration of what the launch can choose.

test_splitk_cases_cpu.py proves on the CPU (through mcamd_conv_fwd_splitk_info, which is answered by the launch's own
mcamd_splitk_plan()) that SPLITK_CASES reaches both partial instances with every destination form, the raw form and every
named boundary condition, that every case's reference meets the conditions of exactness of conv_cases.py, and that every
slice of every (M tile, N tile) of every launch carries a non-zero partial sum; test_splitk_instances_gpu.py runs each case
against that reference.  Test-side only.

Why the unsplit reference applies whatever the slice count: the operands are small integers and max|x| max|w| ktot < 2^24
(conv_cases.exactness, condition 1), so every slab value and every sum of slabs in slice order is an integer that fp32
holds."""
import collections
import zlib

import torch
import torch.nn.functional as F

from modelcompression_amd import ops
from modelcompression_amd import _lib as L
import conv_cases as CC
from conv_cases import DRAWS, SLOPE, _draw, reorg, exactness, Operands  # noqa: F401  (shared with the dense cases)

ENV = {"MCAMD_SPLITK_MIN_CHUNKS": "8", "MCAMD_SPLITK_CUS": "256"}
POLICY = 0                                # slices = 0: the library's policy
MAX_SLICES = 16                           # the policy's ceiling (a forced count may exceed it, up to the chunk count)

K64, K32 = (64, 3), (32, 4)               # splitk_partial_kernel<BK, NSTAGE> as (bk, stages)
INSTANCES = (K64, K32)
FORMS = ("plain", "pool", "pool+y2", "reorg", "raw")
DSTS = CC.DSTS

_FIELDS = "name form B H W k cin cout ld choff y_ld y_choff y2_ld y2_choff draw wdraw slices overflow expect tags"


class Case(collections.namedtuple("Case", _FIELDS)):
    """One launch of mcamd_conv_fwd_splitk.
    form: the destination form of the MCAMD_EPI_PAD_F16 epilogue ("plain", "pool", "pool+y2", "reorg"), or "raw"
    (MCAMD_EPI_RAW_F16: y[M][y_ld]).  ld / choff: the operand slice (ld 0: the slice is the whole buffer).  y_ld / y_choff:
    the output slice (y_ld 0: the whole buffer); y2_ld / y2_choff: that of the full-resolution copy of "pool+y2".
    draw / wdraw: conv_cases.DRAWS keys of the activation and the weight values.  slices: the slice count asked for, 0 = the
    policy's.  overflow: two planted elements beyond the fp16 range.  expect: (bk, stages), the partial kernel instance.
    tags: the boundary conditions the case was written for, each re-derived from the info query by boundary_tags().
    The part of the name in front of the first "." seeds the operands: the launches of one row share them and the reference.
    (epi, dst, fwd, n, M, k_tap, ktot, stem, concurrent, pad, mask: what conv_cases.reference / exactness and util.fill_padded
    read from a dense case.)"""
    __slots__ = ()
    fwd, stem, concurrent, pad, mask = True, 0, False, 0, False

    def __str__(self):
        return self.name

    @property
    def base(self):
        return self.name.split(".")[0]

    @property
    def epi(self):
        return "fwd-raw16" if self.form == "raw" else "fwd-pad"

    @property
    def dst(self):
        return "plain" if self.form == "raw" else self.form

    @property
    def pooled(self):
        """the M tile is enumerated in pooled order (four consecutive rows = one 2x2 window)"""
        return self.form in ("pool", "pool+y2", "reorg")

    @property
    def n(self):
        return self.cout

    @property
    def M(self):
        return self.B * self.H * self.W

    @property
    def k_tap(self):
        """padded operand channels per tap"""
        return ops.round_up(self.cin, 32)

    @property
    def kb(self):
        """channel block of the packed K order [channel block][tap][kb] (include/mcamd.h)"""
        return 64 if self.k_tap % 64 == 0 else 32

    @property
    def ntaps(self):
        return self.k * self.k

    @property
    def ktot(self):
        return self.ntaps * self.k_tap

    @property
    def cdst(self):
        """channels of the destination slice"""
        return 4 * self.cout if self.form == "reorg" else self.cout

    @property
    def y2_slice(self):
        """(ld, choff) of the full-resolution copy"""
        return (self.y2_ld or ops.round_up(self.cout + 40, 32), self.y2_choff if self.y2_ld else 32)


def case(name, form, B, H, W, k, cin, cout, expect, slices, ld=0, choff=0, y_choff=0, y2_choff=0, overflow=False, draw="d1",
         wdraw=None, tags=()):
    assert form in FORMS and (form in ("plain", "raw") or (H % 2 == 0 and W % 2 == 0))
    assert y2_choff == 0 or form == "pool+y2"
    cdst = 4 * cout if form == "reorg" else cout
    y_ld = ops.round_up(y_choff + cdst + 8, 32) if y_choff else 0
    y2_ld = ops.round_up(y2_choff + cout + 8, 32) if y2_choff else 0
    return Case(name, form, B, H, W, k, cin, cout, ld, choff, y_ld, y_choff, y2_ld, y2_choff, draw, wdraw or draw, slices,
                overflow, tuple(expect), tuple(tags))


def geom_of(c):
    return ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, c.ld or c.k_tap, c.choff)


def apply_env(setenv):
    """pin the policy's switches to their defaults"""
    for name, value in ENV.items():
        setenv(name, value)


def info_of(c, slices=None):
    return ops.conv_fwd_splitk_info(geom_of(c), L.EPI_RAW_F16 if c.form == "raw" else L.EPI_PAD_F16, DSTS[c.dst],
                                    c.slices if slices is None else slices)


def slice_ranges(chunks, S):
    """the K chunks [q0, q1) of every slice (conv_splitk.hip: floor(s n / S) .. floor((s + 1) n / S))"""
    return [(s * chunks // S, (s + 1) * chunks // S) for s in range(S)]


def boundary_tags(c, r):
    """The named boundary conditions this launch meets, from the info query and the case's shape alone."""
    t = set()
    M, S = c.M, r.slices
    # ---- the M axis: the partial tile of bm rows and the finish tile of finish_rows rows
    if M < r.bm:
        t.add("M<bm")
    elif M % r.bm:
        t.add("M%bm!=0")
    if M % r.bm == 0:
        t.add("M%bm==0")
    if M % r.finish_rows:
        t.add("M%16!=0")
    if c.B > 1 and (c.H * c.W) % r.bm:            # (pooled order: 4 rows per pooled pixel, the same condition)
        t.add("tile-spans-images-pooled" if c.pooled else "tile-spans-images")
    if c.B > 1 and (c.H * c.W) % r.finish_rows:
        t.add("finish-tile-spans-images")
    # ---- the N axis
    if c.cout < r.bn:
        t.add("n<bn")
    if c.cout % r.bn:
        t.add("n%bn!=0")
    if r.ntiles > 1:
        t.add("ntiles>1")
    # ---- the K axis and the operand slices
    if c.k_tap > c.cin:
        t.add("k-padded")
    if r.bk == 32 and c.k_tap % 64:
        t.add("bk32-by-k_tap%64")
    if c.choff > 0 and c.ld > c.choff + c.k_tap:
        t.add("x_choff>0")
    if c.y_choff > 0 and c.y_ld > c.y_choff + c.cdst:
        t.add("y_choff>0")
    if c.form == "pool+y2" and c.y2_slice[1] > 0 and c.y2_slice[0] > c.y2_slice[1] + c.cout:
        t.add("y2_choff>0")
    t.add("1x1" if c.k == 1 else "3x3")
    # ---- the slices
    lens = [q1 - q0 for q0, q1 in slice_ranges(r.chunks, S)]
    if S == 1:
        t.add("S==1")
    if S == r.chunks:
        t.add("S==chunks")
    if r.chunks % S:
        t.add("chunks%S!=0")
    if min(lens) < r.stages - 1:
        t.add("slice-shorter-than-ring")          # the prologue fills part of the ring only
    if max(lens) > r.stages:
        t.add("slice-longer-than-ring")           # the ring wraps
    if S == MAX_SLICES:
        t.add("S==16")
    if c.slices == POLICY and S > 1:
        t.add("policy-splits")
    # ---- the grid of the partial launch: (N tile, slice) groups in whole rounds of 8, times the M tiles
    groups = r.ntiles * S
    if groups % 8 and r.mtiles > 1:
        t.add("groups%8!=0,mtiles>1")
    if groups > 8:
        t.add("groups>8")
    return t


# each of these on both partial instances
BOUNDARIES_BOTH = ("M<bm", "M%bm!=0", "M%bm==0", "M%16!=0", "tile-spans-images", "tile-spans-images-pooled",
                   "finish-tile-spans-images", "n<bn", "n%bn!=0", "ntiles>1", "k-padded", "x_choff>0", "y_choff>0", "y2_choff>0",
                   "1x1", "3x3", "S==1", "S==chunks", "chunks%S!=0", "slice-shorter-than-ring", "slice-longer-than-ring", "S==16",
                   "policy-splits", "groups%8!=0,mtiles>1", "groups>8")
BOUNDARIES_K32 = ("bk32-by-k_tap%64",)
PADDED_CINS = (40, 72)                            # 40 -> 64 channels per tap (chunks of 64), 72 -> 96 (chunks of 32)


# ---------------------------------------------------------------------------------------------------------------------
# what the launch can choose
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_IMAGES = ((1, 1, 1), (2, 9, 7), (1, 13, 13), (1, 16, 16), (2, 12, 14), (64, 26, 26))
# (mode, dst_mode) of every form
SWEEP_FORMS = ((L.EPI_PAD_F16, L.DST_PLAIN), (L.EPI_PAD_F16, L.DST_POOL), (L.EPI_PAD_F16, L.DST_REORG), (L.EPI_RAW_F16, L.DST_PLAIN))


def reachable(setenv):
    """set of (bk, stages) over both epilogue modes and all destination forms x SWEEP_IMAGES x both kernel sizes x every
    filter and input-channel count from 8 to 1344 in steps of 8 x forced slice counts 0 .. 16, by asking the library.  The
    tile, the tile counts and the finish tile of every answer are checked on the way, and the policy's answer (and every
    accepted forced one) lies in [1, min(16, chunks)]."""
    import ctypes as C
    apply_env(setenv)
    fn = L.lib().mcamd_conv_fwd_splitk_info
    g = ops.geom(1, 8, 8, 3, 32, 32, 32)
    info = L.SplitkInfo()
    ref, out = C.byref(g), C.byref(info)
    seen = set()
    for (B, H, W) in SWEEP_IMAGES:
        g.B, g.H, g.W = B, H, W
        M = B * H * W
        forms = [f for f in SWEEP_FORMS if f[1] == L.DST_PLAIN or (H % 2 == 0 and W % 2 == 0)]
        for k in (1, 3):
            g.ksize = k
            for cin in range(8, 1345, 8):
                g.cin, g.x_ld = cin, ops.round_up(cin, 32)
                bk = 64 if g.x_ld % 64 == 0 else 32
                chunks = k * k * g.x_ld // bk
                for cout in range(8, 1345, 8):
                    g.cout = cout
                    # (the plan does not depend on the form: every form for the policy, the plain one for the forced counts)
                    for S in range(0, MAX_SLICES + 1):
                        for (mode, dst) in (forms if S == 0 else forms[:1]):
                            rc = fn(ref, mode, dst, S, out)
                            if S > chunks:
                                assert rc != 0, (B, H, W, k, cin, cout, S)      # refused: more slices than chunks
                                continue
                            assert rc == 0, (B, H, W, k, cin, cout, mode, dst, S)
                            assert (info.bm, info.bn, info.bk, info.chunks) == (64, 64, bk, chunks)
                            assert info.mtiles == -(-M // info.bm) and info.ntiles == -(-cout // info.bn)
                            assert info.tiles == info.mtiles * info.ntiles
                            assert (info.finish_rows, info.finish_cols) == (16, 64) and info.bm % info.finish_rows == 0
                            assert 1 <= info.slices <= min(MAX_SLICES, chunks) and (S == 0 or info.slices == S)
                            assert info.workspace_bytes == info.slices * info.mtiles * info.bm * info.ntiles * info.bn * 4
                            seen.add((info.bk, info.stages))
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# operands and the exact reference (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
SAT_FILTER = 5
SAT_W, SAT_POS, SAT_NEG = 32.0, 64.0, -256.0      # 128 channels: 128 * 32 * 64 = 262144; 128 * 32 * -256 * 2 / 8 = -262144


def operands(c, gaussian=False, plant=True):
    """conv_cases.Operands: act x [B][cin][H][W]; w OIHW; scale / shift per filter (None in the raw form); planted [(b,
    channel, h, w, sign)] of an `overflow` case."""
    gen = torch.Generator().manual_seed(zlib.crc32(c.base.encode()))
    if gaussian:
        act = torch.randn(c.B, c.cin, c.H, c.W, generator=gen)
        w = torch.randn(c.cout, c.cin, c.k, c.k, generator=gen) * (2.0 / c.ktot) ** 0.5
    else:
        act = _draw(gen, DRAWS[c.draw], (c.B, c.cin, c.H, c.W))
        w = _draw(gen, DRAWS[c.wdraw], (c.cout, c.cin, c.k, c.k))
    scale = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (c.cout,), generator=gen)]
    shift = torch.randint(-8, 9, (c.cout,), generator=gen).float() * 0.25
    planted = []
    if c.overflow and not gaussian:
        assert c.k == 1 and c.cin == 128
        # (every filter sees the planted pixels: scales 1 and 2 and shifts in steps of 64 keep those values fp16 numbers)
        w[SAT_FILTER] = SAT_W
        scale, shift = torch.where(scale < 1.0, scale * 4.0, scale), shift * 256.0
        scale[SAT_FILTER], shift[SAT_FILTER] = 2.0, 0.0
        if plant:
            act[0, :, 1, 2] = SAT_POS
            act[c.B - 1, :, c.H - 1, c.W - 2] = SAT_NEG
            planted = [(0, SAT_FILTER, 1, 2, 1.0), (c.B - 1, SAT_FILTER, c.H - 1, c.W - 2, -1.0)]
    if c.form == "raw":
        scale = shift = None
    return Operands(act, w, None, None, scale, shift, planted)


_CACHE = {}


def operands_and_reference(c, plant=True):
    """Once per process and row (the launches of a row differ in the slice count only); shared by the tests and never
    modified."""
    key = (c.base, plant)
    if key not in _CACHE:
        o = operands(c, plant=plant)
        _CACHE[key] = (o, CC.reference(c, o))
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------
# the implicit GEMM restated: rows in the launch's pixel order, columns in the packed K order
# ---------------------------------------------------------------------------------------------------------------------
def row_pixels(c):
    """int64 [M]: the row-major pixel index b HW + h W + w of GEMM row m (conv_epi.h: tile_pixel) -- row-major, or in pooled
    order m = 4 * pooled pixel + (dy * 2 + dx)."""
    m = torch.arange(c.M)
    if not c.pooled:
        return m
    Wo, HWo = c.W // 2, (c.H // 2) * (c.W // 2)
    q, p = m % 4, m // 4
    b, r = p // HWo, p % HWo
    h, w = 2 * (r // Wo) + q // 2, 2 * (r % Wo) + q % 2
    return b * c.H * c.W + h * c.W + w


def packed_k_order(v, c):
    """OIHW [cout][cin][k][k] -> [cout][ktot] in the packed K order [channel block][tap][kb], channels zero-padded to k_tap"""
    cout = v.shape[0]
    p = torch.zeros(cout, c.k_tap, c.ntaps, dtype=v.dtype)
    p[:, :c.cin] = v.reshape(cout, c.cin, c.ntaps)
    return p.view(cout, c.k_tap // c.kb, c.kb, c.ntaps).permute(0, 1, 3, 2).reshape(cout, c.ktot).contiguous()


def gemm_operands(c, act, w):
    """(X [M][ktot], Wp [cout][ktot]) in fp32 (exact: small integers): X's rows in the launch's pixel order, both in the packed
    K order, so that chunk q of `bk` columns is what one stage of the K loop multiplies."""
    x = torch.zeros(c.B, c.k_tap, c.H, c.W)
    x[:, :c.cin] = act
    cols = F.unfold(x, c.k, padding=(c.k - 1) // 2)                                     # [B][k_tap * ntaps][HW], channel-major
    cols = cols.view(c.B, c.k_tap // c.kb, c.kb, c.ntaps, c.H * c.W).permute(0, 4, 1, 3, 2).reshape(c.M, c.ktot)
    return cols[row_pixels(c)].contiguous(), packed_k_order(w, c)


def tile_any(t, bm, bn):
    """bool [..][M][N] -> bool [..][mtiles][ntiles]: does a tile hold a True?"""
    M, N = t.shape[-2:]
    mt, nt = -(-M // bm), -(-N // bn)
    p = torch.zeros(t.shape[:-2] + (mt * bm, nt * bn), dtype=torch.bool)
    p[..., :M, :N] = t
    return p.view(t.shape[:-2] + (mt, bm, nt, bn)).any(-1).any(-2)


def clamped_mask(c, o):
    """bool [M][cout] in GEMM row order: the elements an overflow case clamps"""
    m = torch.zeros(c.M, c.cout, dtype=torch.bool)
    if o.planted:
        where = {int(p): i for i, p in enumerate(row_pixels(c).tolist())}
        for (b, ch, h, x, _) in o.planted:
            m[where[b * c.H * c.W + h * c.W + x], ch] = True
    return m


def chunk_sums(c, o, bk):
    """float64 [chunks + 1][M][cout]: the running sum of the first q chunks' contributions, q = 0 .. chunks"""
    X, Wp = gemm_operands(c, o.act, o.w)
    nch = c.ktot // bk
    P = torch.einsum("mqk,nqk->qmn", X.double().view(c.M, nch, bk), Wp.double().view(c.cout, nch, bk))
    return torch.cat([torch.zeros(1, c.M, c.cout, dtype=torch.float64), P.cumsum(0)])


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
# (row, form, image, k, cin, cout, keywords of case(), slice counts, tags of the row's launches as {slices: tags} or tags for all)
_ROWS = [
    # ---- splitk_partial_kernel<64, 3>: 64 padded channels per tap or a multiple
    ("a64-plain", "plain", (1, 13, 13), 3, 128, 72, K64, dict(y_choff=8), (1, 2, 5, 16, 18, POLICY),
     ("M%bm!=0", "M%16!=0", "n%bn!=0", "ntiles>1", "y_choff>0", "3x3")),
    ("b64-pool", "pool", (2, 12, 14), 1, 128, 40, K64, dict(draw="d3"), (1, 2), ("tile-spans-images-pooled", "n<bn", "1x1")),
    ("c64-pool+y2", "pool+y2", (2, 12, 14), 3, 64, 136, K64, dict(ld=128, choff=32, y_choff=16, y2_choff=16, draw="d2"), (1, 4, 7, 9),
     ("x_choff>0", "y_choff>0", "y2_choff>0", "finish-tile-spans-images")),
    ("d64-reorg", "reorg", (1, 16, 16), 1, 128, 24, K64, dict(y_choff=32, draw="d3"), (1, 2), ("M%bm==0", "n<bn", "y_choff>0")),
    ("e64-padded-k", "plain", (1, 12, 12), 3, 40, 264, K64, dict(draw="d2"), (1, 3, 9), ("k-padded", "ntiles>1", "M%bm!=0")),
    ("f64-raw", "raw", (2, 9, 7), 3, 64, 40, K64, dict(y_choff=8, draw="d2"), (1, 3, 9),
     ("tile-spans-images", "finish-tile-spans-images", "M%16!=0", "n<bn", "y_choff>0")),
    ("g64-one-tile", "plain", (1, 6, 6), 3, 64, 64, K64, dict(draw="d2"), (2,), ("M<bm",)),
    # the longest chunk loop of the network (conv21: 1280 channels, 3x3 -- 180 chunks), sparse draws
    ("h64-long-k", "plain", (1, 13, 13), 3, 1280, 392, K64, dict(draw="s4", wdraw="s4u"), (16, POLICY), ()),
    ("i64-saturate", "plain", (2, 13, 13), 1, 128, 72, K64, dict(overflow=True, draw="d3"), (2,), ("M%bm!=0", "n%bn!=0")),
    ("j64-saturate-raw", "raw", (2, 9, 7), 1, 128, 64, K64, dict(overflow=True, draw="d3"), (2,), ()),
    # ---- splitk_partial_kernel<32, 4>: the padded channel count is no multiple of 64 (K order [channel block][tap][32])
    ("a32-pool", "pool", (2, 12, 14), 1, 96, 72, K32, dict(draw="d3"), (1, 2, 3), ("tile-spans-images-pooled", "1x1", "n%bn!=0")),
    ("b32-pool+y2", "pool+y2", (2, 12, 14), 3, 96, 136, K32, dict(y_choff=8, y2_choff=16), (1, 4, 7, 16, POLICY),
     ("y_choff>0", "y2_choff>0", "3x3", "ntiles>1", "finish-tile-spans-images")),
    ("c32-reorg", "reorg", (2, 6, 10), 1, 96, 64, K32, dict(draw="d3"), (1, 2, 3), ("M%bm!=0", "M%16!=0")),
    ("d32-padded-k", "plain", (1, 12, 12), 3, 72, 264, K32, dict(ld=160, choff=32), (1, 3, 27),
     ("k-padded", "bk32-by-k_tap%64", "x_choff>0", "ntiles>1")),
    ("e32-raw", "raw", (2, 9, 7), 3, 32, 40, K32, dict(draw="d3"), (1, 3, 9), ("tile-spans-images", "finish-tile-spans-images", "n<bn")),
    ("f32-one-tile", "plain", (1, 6, 6), 1, 96, 24, K32, dict(draw="d3"), (2,), ("M<bm", "n<bn")),
    ("g32-whole-tiles", "plain", (1, 8, 8), 3, 32, 64, K32, dict(draw="d3"), (1, 9), ("M%bm==0",)),
]
# what a slice count adds to its row's tags
_SLICE_TAGS = {
    ("a64-plain", 1): ("S==1", "slice-longer-than-ring"), ("a64-plain", 5): ("chunks%S!=0", "groups%8!=0,mtiles>1", "groups>8"),
    ("a64-plain", 16): ("S==16", "slice-shorter-than-ring"), ("a64-plain", 18): ("S==chunks",), ("a64-plain", POLICY): ("policy-splits",),
    ("b32-pool+y2", 1): ("S==1", "slice-longer-than-ring"), ("b32-pool+y2", 7): ("chunks%S!=0", "groups%8!=0,mtiles>1", "groups>8"),
    ("b32-pool+y2", 16): ("S==16", "slice-shorter-than-ring"), ("b32-pool+y2", POLICY): ("policy-splits",),
    ("a32-pool", 3): ("S==chunks",), ("d32-padded-k", 27): ("S==chunks",), ("h64-long-k", 16): ("S==16",),
}


def _build():
    out = []
    for (row, form, (B, H, W), k, cin, cout, expect, kw, slices, tags) in _ROWS:
        for S in slices:
            out.append(case("%s.S%s" % (row, "policy" if S == POLICY else S), form, B, H, W, k, cin, cout, expect, S,
                            tags=tuple(tags) + _SLICE_TAGS.get((row, S), ()), **kw))
    return out


SPLITK_CASES = _build()
LONG_K = "h64-long-k"

# one launch per partial instance and finish form: run twice on Gaussian data, bit-equal
DETERMINISM_CASES = ("a64-plain.S5", "f64-raw.S3", "b32-pool+y2.S7", "e32-raw.S3")


# ---------------------------------------------------------------------------------------------------------------------
# one-hot filters: which chunk lands in which slice and which k every lane selects
# ---------------------------------------------------------------------------------------------------------------------
OneHot = collections.namedtuple("OneHot", "k cin image expect")
# image "1x1": one pixel, channel c holds c + 1; "3x3": nine pixels, channel c of pixel p holds 9 c + p + 1 (3x3 filters only:
# the tap is identified too).  One filter per (channel, tap), in a shuffled order: cout = k * k * cin.
ONEHOT_CASES = [
    OneHot(1, 128, "1x1", K64), OneHot(3, 64, "3x3", K64), OneHot(3, 128, "3x3", K64), OneHot(3, 40, "3x3", K64),
    OneHot(1, 96, "1x1", K32), OneHot(3, 96, "3x3", K32), OneHot(3, 72, "3x3", K32), OneHot(3, 32, "1x1", K32),
]


def onehot_id(h):
    return "k%d-cin%d-%s" % (h.k, h.cin, h.image)


def onehot_case(h, slices):
    n = 3 if h.image == "3x3" else 1
    return case("onehot-%s.S%d" % (onehot_id(h), slices), "plain", 1, n, n, h.k, h.cin, h.k * h.k * h.cin, h.expect, slices)


def onehot_slices(h):
    """every slice one chunk, and two slices"""
    chunks = h.k * h.k * ops.round_up(h.cin, 32) // h.expect[0]
    return sorted({chunks, 2})


def onehot_operands(h):
    """(x [1][cin][n][n], w OIHW, [(channel, tap, sign)] per filter).  Every value stays below 2048: exact in fp16."""
    c = onehot_case(h, 1)
    gen = torch.Generator().manual_seed(zlib.crc32(c.base.encode()))
    n = c.H
    ch = torch.arange(h.cin, dtype=torch.float32).view(1, -1, 1, 1)
    x = (ch + 1.0).expand(1, h.cin, 1, 1).clone() if n == 1 else ch * 9.0 + torch.arange(9, dtype=torch.float32).view(1, 1, 3, 3) + 1.0
    assert float(x.max()) < 2048
    order = torch.randperm(c.cout, generator=gen).tolist()
    sign = (torch.randint(0, 2, (c.cout,), generator=gen) * 2 - 1).tolist()
    w = torch.zeros(c.cout, h.cin, h.k, h.k)
    which = []
    for f in range(c.cout):
        chan, tap = divmod(order[f], c.ntaps)
        w[f, chan, tap // h.k, tap % h.k] = float(sign[f])
        which.append((chan, tap, sign[f]))
    return x, w, which
