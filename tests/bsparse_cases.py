"""The cases of tests/test_bsparse_instances_gpu.py: launches of mcamd_bsparse_lists and mcamd_conv_fwd_bsparse
(csrc/conv_bsparse.hip: bsparse_kernel<64 | 128, 64, 3>, <64 | 128, 32, 4> and bsparse_lists_kernel), their operands, masks
and exact references, and the enumeration of what the launch can choose.

test_bsparse_cases_cpu.py proves on the CPU (through mcamd_conv_fwd_bsparse_info, which is answered by the launch's own
mcamd_bsparse_choice()) that BSPARSE_CASES reaches every instance with every destination form, both `pad` forms on both
kernel sizes, every named boundary condition and every per-tile list length around the LDS ring's depth, that every
reference meets the conditions of exactness of conv_cases.py, and that every listed chunk of every tile carries a non-zero
contribution; test_bsparse_instances_gpu.py runs each case against that reference.  Test-side only."""
import collections
import ctypes as C
import zlib

import numpy as np
import torch

from modelcompression_amd import ops
from modelcompression_amd import _lib as L
import bsparse_ref as R
import conv_cases as CC
from conv_cases import DRAWS, SLOPE, _draw, reorg, exactness, Operands  # noqa: F401  (shared with the dense cases)
from splitk_cases import row_pixels, packed_k_order, gemm_operands, tile_any, clamped_mask  # noqa: F401

BM_ENV = "MCAMD_BSPARSE_BM"
# bsparse_kernel<BM, BK, NSTAGE> as (bm, bk, stages); the N tile is always 64 filters
INSTANCES = ((64, 64, 3), (128, 64, 3), (64, 32, 4), (128, 32, 4))
DSTS = CC.DSTS
MASK_KINDS = ("block", "unstructured", "single", "negzero")
ALL, RANDOM = -1, None      # per-tile list lengths of a block mask: every chunk / about half of them, at random

_FIELDS = "name B H W k cin cout pad ld choff y_ld y_choff dst y2_ld y2_choff bm mask counts overflow draw wdraw expect tags"


class Case(collections.namedtuple("Case", _FIELDS)):
    """One launch of mcamd_conv_fwd_bsparse on the lists of mcamd_bsparse_lists (and one with all_chunks).
    pad: the form of x (0 padded, 1 shared halo).  ld / choff, y_ld / y_choff, y2_ld / y2_choff: the slices, as in
    sparse_cases.  bm: the setting of MCAMD_BSPARSE_BM.  mask:
      "block"         a block mask; tile t keeps counts[t] chunks (ALL: every chunk, RANDOM: about half) at random places;
      "unstructured"  about 40 % of the weights at random: every block keeps some, the lists are full;
      "single"        four blocks of five are kept by ONE non-zero weight each, whose place moves through the 64 x kb block
                      from block to block (every 16-byte piece column, the first and the last row); the fifth is empty;
      "negzero"       a block mask (RANDOM) in which one dropped block per tile holds negative weights: w * 0 = -0.0 is all
                      the packing holds there, and the block must stay dropped.
    overflow: two planted elements beyond the fp16 range.  expect: (bm, bk, stages), the instance.  tags: the boundary
    conditions the case was written for, each re-derived from the info query by boundary_tags().
    (epi, fwd, form, pooled, n, M, k_tap, ...: what conv_cases.reference / exactness and splitk_cases.gemm_operands read.)"""
    __slots__ = ()
    epi, fwd, stem, concurrent = "fwd-pad", True, 0, False

    def __str__(self):
        return self.name

    @property
    def base(self):
        return self.name.split(".")[0]

    @property
    def pooled(self):
        return self.dst != "plain"

    @property
    def n(self):
        return self.cout

    @property
    def M(self):
        return self.B * self.H * self.W

    @property
    def k_tap(self):
        return self.cin                     # (cin % 32 == 0: no padded channels in this form)

    @property
    def kb(self):
        return R.block_kb(self.cin)

    @property
    def ntaps(self):
        return self.k * self.k

    @property
    def ktot(self):
        return self.ntaps * self.cin

    @property
    def nchunks(self):
        return self.ktot // self.kb

    @property
    def ntiles(self):
        return -(-self.cout // R.FILTERS)

    @property
    def cdst(self):
        return 4 * self.cout if self.dst == "reorg" else self.cout

    @property
    def y2_slice(self):
        return (self.y2_ld or ops.round_up(self.cout + 40, 32), self.y2_choff if self.y2_ld else 32)


def case(name, B, H, W, k, cin, cout, bm, mask="block", counts=(), pad=0, ld=0, choff=0, y_choff=0, dst="plain", y2_choff=0,
         overflow=False, draw="d1", wdraw=None, tags=()):
    assert dst in DSTS and mask in MASK_KINDS and (dst == "plain" or (H % 2 == 0 and W % 2 == 0)) and cin % 32 == 0
    assert y2_choff == 0 or dst == "pool+y2"
    cdst = 4 * cout if dst == "reorg" else cout
    y_ld = ops.round_up(y_choff + cdst + 8, 32) if y_choff else 0
    y2_ld = ops.round_up(y2_choff + cout + 8, 32) if y2_choff else 0
    kb = R.block_kb(cin)
    assert mask != "block" or len(counts) == -(-cout // R.FILTERS)
    return Case("%s.m%d" % (name, bm), B, H, W, k, cin, cout, pad, ld, choff, y_ld, y_choff, dst, y2_ld, y2_choff, bm, mask, tuple(counts),
                overflow, draw, wdraw or draw, (bm, kb, 3 if kb == 64 else 4), tuple(tags))


def geom_of(c):
    return ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, c.ld or c.cin, c.choff, pad=c.pad)


def apply_env(c, setenv):
    setenv(BM_ENV, str(c.bm))


def info_of(c):
    return ops.conv_fwd_bsparse_info(geom_of(c))


def boundary_tags(c, r):
    """The named boundary conditions this launch meets, from the info query's tile and the case's shape alone."""
    t = set()
    M = c.M
    if M < r.bm:
        t.add("M<bm")
    elif M % r.bm:
        t.add("M%bm!=0")
    if M % r.bm == 0:
        t.add("M%bm==0")
    if c.B > 1 and (c.H * c.W) % r.bm:           # (pooled order: 4 rows per pooled pixel, the same condition)
        t.add("tile-spans-images-pooled" if c.pooled else "tile-spans-images")
    if c.cout < r.bn:
        t.add("n<bn")
    if c.cout % r.bn:
        t.add("n%bn!=0")
    if r.ntiles > 1:
        t.add("ntiles>1")
    if r.bk == 32 and c.k == 3 and c.cin > 32:
        t.add("bk32")                            # the K order [channel block][tap][32] with several blocks
    if c.choff > 0 and c.ld > c.choff + c.cin:
        t.add("x_choff>0")
    if c.y_choff > 0 and c.y_ld > c.y_choff + c.cdst:
        t.add("y_choff>0")
    if c.dst == "pool+y2" and c.y2_slice[1] > 0 and c.y2_slice[0] > c.y2_slice[1] + c.cout:
        t.add("y2_choff>0")
    t.add(("1x1" if c.k == 1 else "3x3") + (",shared-halo" if c.pad else ",padded"))
    return t


# each of these on every instance
BOUNDARIES_ALL = ("M<bm", "M%bm!=0", "M%bm==0", "tile-spans-images", "tile-spans-images-pooled", "n<bn", "n%bn!=0", "ntiles>1",
                  "x_choff>0", "y_choff>0", "y2_choff>0", "1x1,padded", "1x1,shared-halo", "3x3,padded", "3x3,shared-halo")
BOUNDARIES_K32 = ("bk32",)


def ring_lengths(stages, nchunks):
    """the per-tile list lengths around the ring's depth: nothing staged, part of the prologue, the whole prologue, the
    first steady-state iterations, everything"""
    return {0, 1, stages - 2, stages - 1, stages, stages + 1, nchunks}


# ---------------------------------------------------------------------------------------------------------------------
# what the launch can choose
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_IMAGES = ((1, 1, 1), (2, 9, 7), (1, 13, 13), (3, 20, 20), (64, 26, 26))


def reachable(setenv):
    """set of (bm, bk, stages) over both settings of MCAMD_BSPARSE_BM x SWEEP_IMAGES x both kernel sizes x both `pad` forms x
    every accepted input-channel count (a multiple of 32) and every filter count (a multiple of 8) up to 1344, by asking the
    library; the N tile, the tile counts and the grid of every answer are checked on the way."""
    fn = L.lib().mcamd_conv_fwd_bsparse_info
    g = ops.geom(1, 8, 8, 3, 32, 32, 32)
    out = (C.c_int32 * 7)()
    ref = C.byref(g)
    seen = set()
    for bm_env in ("64", "128"):
        setenv(BM_ENV, bm_env)
        for (B, H, W) in SWEEP_IMAGES:
            g.B, g.H, g.W = B, H, W
            M = B * H * W
            for k in (1, 3):
                g.ksize = k
                for cin in range(8, 1345, 8):
                    g.cin = g.x_ld = cin
                    for cout in range(8, 1345, 8) if cin % 32 == 0 else (64,):
                        g.cout = cout
                        for pad in (0, 1):
                            g.pad = pad
                            rc = fn(ref, out)
                            if cin % 32:
                                assert rc != 0 and not ops.conv_fwd_bsparse_ok(g), cin      # refused: no block form
                                continue
                            assert rc == 0, (B, H, W, k, cin, cout, pad)
                            bm, bn, bk, stages, mtiles, ntiles, grid = out
                            assert bm == int(bm_env) and bn == R.FILTERS and bk == R.block_kb(cin)
                            assert mtiles == -(-M // bm) and ntiles == -(-cout // bn) and grid == -(-mtiles // 8) * 8 * ntiles
                            seen.add((bm, bk, stages))
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# masks, operands and the exact reference (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
SAT_FILTER = 5
SAT_W, SAT_POS, SAT_NEG = 32.0, 64.0, -256.0      # 96 channels or more: 96 * 32 * 64 = 196608; 96 * 32 * -256 * 2 / 8 = -196608


def single_position(c, j):
    """(row, column) in the 64 x kb block of the only non-zero weight of block j = tile * nchunks + chunk of a "single" mask:
    the 16-byte piece column advances with j, the row visits the first and the last row of the tile"""
    cpr = c.kb // 8
    col = (j % cpr) * 8 + (j // cpr * 3 + 1) % 8
    row = (0, R.FILTERS - 1, (j * 7 + 3) % R.FILTERS)[(j // cpr) % 3]
    return row, col


def build_mask(c, gen, w):
    """(mask OIHW, w) of the case's kind (w: the weights with the signs a "negzero" mask needs)."""
    shape = (c.cout, c.cin, c.k, c.k)
    nfb, nch, kb = c.ntiles, c.nchunks, c.kb
    if c.mask == "unstructured":
        return (torch.rand(shape, generator=gen) > 0.6).float(), w
    if c.mask == "single":
        assert c.cout % R.FILTERS == 0
        m = torch.zeros(c.cout, c.cin, c.ntaps)
        for t in range(nfb):
            for q in range(nch):
                j = t * nch + q
                if j % 5 == 4:
                    continue
                row, col = single_position(c, j)
                cb, tap = divmod(q, c.ntaps)              # chunk q = (channel block, tap) of the packed K order
                m[t * R.FILTERS + row, cb * kb + col, tap] = 1.0
        return m.view(shape), w
    keep = (torch.rand(nfb, nch, generator=gen) > 0.5).to(torch.int32).numpy()
    counts = c.counts if c.mask == "block" else (RANDOM,) * nfb
    for t, n in enumerate(counts):
        if n is RANDOM:
            continue
        keep[t] = 0
        keep[t, torch.randperm(nch, generator=gen)[:nch if n == ALL else n].numpy()] = 1
    if c.mask == "negzero":
        w = w.clone()
        blocks = torch.from_numpy(R.block_index(c.cout, c.cin, c.ntaps)).view(shape)
        for t in range(nfb):
            keep[t, t % nch] = 0                          # (a dropped chunk in every tile, at a place that moves)
            sel = blocks == t * nch + t % nch
            w[sel] = -w[sel].abs()
    return torch.from_numpy(R.block_mask(keep.reshape(-1), shape)), w


def operands(c, gaussian=False, plant=True):
    """conv_cases.Operands: act x [B][cin][H][W]; w OIHW; mask OIHW; scale / shift per filter; planted [(b, channel, h, w,
    sign)] of an `overflow` case."""
    gen = torch.Generator().manual_seed(zlib.crc32(c.base.encode()))
    if gaussian:
        act = torch.randn(c.B, c.cin, c.H, c.W, generator=gen)
        w = torch.randn(c.cout, c.cin, c.k, c.k, generator=gen) * (4.0 / c.ktot) ** 0.5
        w = w + 0.5 * torch.sign(w)                       # no value rounds to zero in fp16
    else:
        act = _draw(gen, DRAWS[c.draw], (c.B, c.cin, c.H, c.W))
        w = _draw(gen, DRAWS[c.wdraw], (c.cout, c.cin, c.k, c.k))
        if not c.wdraw.startswith("s"):
            w[w == 0] = 1.0                               # every kept weight counts (the sparse draws keep their zeros)
    mask, w = build_mask(c, gen, w)
    scale = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (c.cout,), generator=gen)]
    shift = torch.randint(-8, 9, (c.cout,), generator=gen).float() * 0.25
    planted = []
    if c.overflow and not gaussian:
        assert c.k == 1 and c.cin >= 96 and c.mask == "block" and c.counts[0] == ALL
        # (every filter sees the planted pixels: scales 1 and 2 and shifts in steps of 64 keep those values fp16 numbers)
        w[SAT_FILTER] = SAT_W
        scale, shift = torch.where(scale < 1.0, scale * 4.0, scale), shift * 256.0
        scale[SAT_FILTER], shift[SAT_FILTER] = 2.0, 0.0
        if plant:
            act[0, :, 1, 2] = SAT_POS
            act[c.B - 1, :, c.H - 1, c.W - 2] = SAT_NEG
            planted = [(0, SAT_FILTER, 1, 2, 1.0), (c.B - 1, SAT_FILTER, c.H - 1, c.W - 2, -1.0)]
    return Operands(act, w, mask, None, scale, shift, planted)


def lists_ref(c, o):
    """(packed fp16 [Npad][ktot], count, list): bsparse_ref's restatement of the packing and of mcamd_bsparse_lists"""
    packed = R.pack_fwd(o.w.numpy(), o.mask.numpy())
    return (packed,) + R.chunk_lists(packed, c.cout, c.kb)


_CACHE = {}


def operands_and_reference(c, plant=True):
    """Once per process and case; shared by the tests and never modified."""
    key = (c.name, plant)
    if key not in _CACHE:
        o = operands(c, plant=plant)
        _CACHE[key] = (o, CC.reference(c, o))
    return _CACHE[key]


def chunk_contributions(c, o):
    """float64 [nchunks][M][cout]: what chunk q adds to every accumulator (rows in the launch's pixel order)"""
    X, Wp = gemm_operands(c, o.act, o.w * o.mask)
    return torch.einsum("mqk,nqk->qmn", X.double().view(c.M, c.nchunks, c.kb), Wp.double().view(c.cout, c.nchunks, c.kb))


# ---------------------------------------------------------------------------------------------------------------------
# the cases: the same rows on the 64-row and on the 128-row M tile
# ---------------------------------------------------------------------------------------------------------------------
def _rows(bm):
    return [
        # ---- bsparse_kernel<bm, 64, 3>: 64-channel blocks
        case("k64-plain-lengths", 2, 13, 13, 3, 64, 440, bm, "block", (0, 1, 2, 3, 4, ALL, RANDOM), pad=1, y_choff=8, draw="d2",
             tags=("M%bm!=0", "tile-spans-images", "ntiles>1", "n%bn!=0", "y_choff>0", "3x3,shared-halo")),
        case("k64-pool-unstructured", 2, 12, 14, 1, 128, 40, bm, "unstructured", dst="pool", draw="d3",
             tags=("tile-spans-images-pooled", "n<bn", "1x1,padded")),
        case("k64-pool+y2-negzero", 2, 12, 14, 3, 64, 136, bm, "negzero", dst="pool+y2", ld=128, choff=32, y_choff=16, y2_choff=16, draw="d2",
             tags=("x_choff>0", "y2_choff>0", "3x3,padded")),
        case("k64-reorg", 1, 16, 16, 1, 128, 72, bm, "block", (1, ALL), dst="reorg", pad=1, y_choff=32, draw="d3",
             tags=("M%bm==0", "1x1,shared-halo", "y_choff>0")),
        case("k64-single", 1, 6, 6, 3, 64, 128, bm, "single", draw="d3", tags=("M<bm",)),
        case("k64-saturate", 2, 13, 13, 1, 128, 72, bm, "block", (ALL, RANDOM), overflow=True, draw="d3", tags=("M%bm!=0",)),
        # ---- bsparse_kernel<bm, 32, 4>: 32-channel blocks (cin % 64 == 32), K order [channel block][tap][32]
        case("k32-plain-lengths", 2, 13, 13, 3, 96, 440, bm, "block", (0, 1, 2, 3, 4, 5, ALL), pad=1, y_choff=8,
             tags=("M%bm!=0", "tile-spans-images", "ntiles>1", "n%bn!=0", "y_choff>0", "3x3,shared-halo", "bk32")),
        case("k32-pool-unstructured", 2, 12, 14, 1, 96, 40, bm, "unstructured", dst="pool", draw="d3",
             tags=("tile-spans-images-pooled", "n<bn", "1x1,padded")),
        case("k32-pool+y2-negzero", 2, 12, 14, 3, 96, 136, bm, "negzero", dst="pool+y2", ld=160, choff=32, y_choff=16, y2_choff=16,
             tags=("x_choff>0", "y2_choff>0", "3x3,padded", "bk32")),
        case("k32-reorg", 1, 16, 16, 1, 96, 72, bm, "block", (1, ALL), dst="reorg", pad=1, y_choff=32, draw="d3",
             tags=("M%bm==0", "1x1,shared-halo", "y_choff>0")),
        case("k32-single", 1, 6, 6, 3, 96, 128, bm, "single", draw="d3", tags=("M<bm", "bk32")),
        case("k32-saturate", 2, 13, 13, 1, 96, 72, bm, "block", (ALL, RANDOM), overflow=True, draw="d3", tags=("M%bm!=0",)),
    ]


BSPARSE_CASES = _rows(64) + _rows(128) + [
    # the longest list of the network (conv21: 1280 channels, 3x3 -- 180 chunks, three ballot groups of the list kernel)
    case("k64-long-list", 1, 13, 13, 3, 1280, 72, 128, "block", (RANDOM, ALL), draw="s4", wdraw="s4u", tags=("ntiles>1", "n%bn!=0")),
]
LONG_LIST = "k64-long-list"

# one case per instance: run twice on Gaussian data, bit-equal
DETERMINISM_CASES = ("k64-pool+y2-negzero.m64", "k64-plain-lengths.m128", "k32-plain-lengths.m64", "k32-pool+y2-negzero.m128")


def foreign_case(inst):
    """the launch of the foreign-list test on an instance: one tile, 3x3 taps (9 chunks of 64 or 27 of 32)"""
    bm, bk, _ = inst
    return case("foreign-k%d" % bk, 1, 6, 6, 3, 64 if bk == 64 else 96, 64, bm, "unstructured", draw="d3")
