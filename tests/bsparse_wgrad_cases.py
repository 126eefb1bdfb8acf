"""The cases of tests/test_bsparse_wgrad_instances_gpu.py (the list launch of the weight gradient, mcamd_conv_wgrad_bsparse,
DESIGN.md 3zd), the masks they run on, and numpy restatements of the tile lists / tap words and of the split rule.

test_bsparse_wgrad_cases_cpu.py proves without a GPU (through mcamd_conv_wgrad_bsparse_plan, answered by the launch's own plan
function) that the cases reach wgrad9_kernel at 64 and at 32 pixels per step, the one-tap 64 x 64 instance of wgrad_kernel
and the select form of the finish kernel at each of its three lane groupings; the GPU test holds every case to an exact
integer reference (the method of tests/wgrad_cases.py).  Test-side only."""
import collections

import numpy as np
import torch

from modelcompression_amd import ops
from modelcompression_amd import _lib as L

MASK_KINDS = ("random", "one-tap", "tile-cleared", "full", "empty", "holes", "unaligned")

_FIELDS = "name B H W k cin cout pad dy_ld dy_choff mask nsplit grad_scale dbias expect tags"


class Case(collections.namedtuple("Case", _FIELDS)):
    """One launch of mcamd_conv_wgrad_bsparse.  mask: one of MASK_KINDS (make_mask).  nsplit 0: the plan's own split count
    for the kept tiles, else that many.  dy_ld 0: the dy slice is the whole buffer.  expect: (compute kernel, finish kernel)
    as compute_of / finish_of name them for the split count the case runs at.  tags: what the case was written for, each
    re-derived by tags_of()."""
    __slots__ = ()

    def __str__(self):
        return self.name


def case(name, B, H, W, k, cin, cout, mask, expect, pad=0, dy_ld=0, dy_choff=0, nsplit=0, grad_scale=1.0, dbias=True, tags=()):
    return Case(name, B, H, W, k, cin, cout, pad, dy_ld, dy_choff, mask, nsplit, grad_scale, dbias, expect, tuple(tags))


def geom_of(c):
    return ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, c.cin, 0, pad=c.pad)


def pixels_enumerated(c):
    """Products summed into one element of dW (the 9-tap kernel enumerates padded pixels, halo included)."""
    if c.k == 1:
        return c.B * c.H * c.W
    pw = 1 if c.pad else 2
    return c.B * (c.H + pw) * (c.W + pw) + (c.W + 2 if c.pad else 0)


# ---- masks ----------------------------------------------------------------------------------------------------------------
def make_mask(c, gen):
    """fp32 [cout][cin][k][k] of 0 / 1.  Blocks are block_prune's: 64 filters x 64 input channels x one tap."""
    nb = (c.cout // 64, c.cin // 64, c.k * c.k)

    def expand(keep):                 # [ot][ct][tap] -> OIHW
        m = keep.reshape(nb[0], 1, nb[1], 1, nb[2]).expand(nb[0], 64, nb[1], 64, nb[2])
        return m.reshape(c.cout, c.cin, c.k, c.k).float().contiguous()

    if c.mask == "full":
        return torch.ones(c.cout, c.cin, c.k, c.k)
    if c.mask == "empty":
        return torch.zeros(c.cout, c.cin, c.k, c.k)
    keep = torch.rand(nb, generator=gen) < 0.4
    keep[0, 0, 0] = True              # (never empty by accident)
    if c.mask == "random":
        return expand(keep)
    if c.mask == "one-tap":           # the last tile keeps exactly its last tap
        keep[-1, -1] = False
        keep[-1, -1, -1] = True
        return expand(keep)
    if c.mask == "tile-cleared":      # the first tile loses every tap, its neighbours keep some
        keep[0, 0] = False
        keep[-1, -1, 0] = True
        return expand(keep)
    if c.mask == "holes":             # elementwise holes inside kept blocks: whole and partial groups of four channels
        m = expand(keep)
        return m * (torch.rand(m.shape, generator=gen) < 0.7).float()
    assert c.mask == "unaligned", c.mask
    m = torch.zeros(c.cout, c.cin, c.k, c.k)          # a rectangle that straddles the tile borders, and one lone element
    r1 = min(100, c.cout - 4)
    m[40:r1, 30:90] = (torch.rand(r1 - 40, 60, c.k, c.k, generator=gen) < 0.5).float()
    m[c.cout - 1, c.cin - 1, c.k - 1, c.k - 1] = 1.0
    return m


def lists_of(mask):
    """The lists mcamd_wgrad_bsparse_lists builds, restated: (kept tile indices ascending, their words, the word of every
    tile, (kept tiles, kept (tile, tap) pairs)).  Tile (ot, ct) has index ot * (cin / 64) + ct; bit t of its word is set iff
    any mask element of filters [64 ot, 64 ot + 64) x channels [64 ct, 64 ct + 64) x tap t is non-zero."""
    m = np.asarray(mask)
    O, I, k, _ = m.shape
    anyb = (m != 0).reshape(O // 64, 64, I // 64, 64, k * k).any(axis=(1, 3))          # [ot][ct][tap]
    words = (anyb.astype(np.int64) << np.arange(k * k)).sum(-1).reshape(-1).astype(np.int32)
    tiles = np.nonzero(words)[0].astype(np.int32)
    return tiles, words[tiles], words, (int(len(tiles)), int(anyb.sum()))


# ---- the plan, restated ---------------------------------------------------------------------------------------------------
def _pick(tiles, cap, slots):
    best, ns = 1e30, 1
    for c in range(1, cap + 1):
        rounds = float((tiles * c + slots - 1) // slots)
        cost = rounds / c * (1.0 + 0.004 * c)
        if cost < best - 1e-12:
            best, ns = cost, c
    return ns


def nine_kp(c):
    """Pixels per step of wgrad9_kernel: 64 while two double-buffered workgroups of (64 + 64 + 2 S) rows x 128 bytes fit 72 KB."""
    pitch = c.W + (1 if c.pad else 2)
    S = -(-(pitch + 1) // 4) * 4
    return 64 if 2 * (64 + 64 + 2 * S) * 128 <= 72 * 1024 else 32


def split_rule(c, kept_tiles):
    """(nsplit, pix_per_split) of a list launch of `kept_tiles` tiles: the dense plans' cost rule on the kept tile count."""
    tiles = max(kept_tiles, 1)
    if c.k == 3:
        nsteps, u = -(-pixels_enumerated(c) // 32), nine_kp(c) // 32
        cap = max(2048 // tiles, 1)
        if cap > nsteps // 8:                      # at least 8 steps of 32 pixels per split
            cap = nsteps // 8 if nsteps // 8 > 0 else 1
        ns = _pick(tiles, cap, 512)
        sps = -(-(-(-nsteps // ns)) // u) * u
        return -(-nsteps // sps), sps * 32
    M, kp = c.B * c.H * c.W, 64
    cap = min(max(3072 // tiles, 1), max(-(-M // (8 * kp)), 1))      # at least 8 steps of 64 pixels per split
    ns = _pick(tiles, cap, 768)
    pps = -(-(-(-M // ns)) // kp) * kp
    return -(-M // pps), pps


def pix_per_split_of(c, nsplit):
    if c.k == 3:
        nsteps, u = -(-pixels_enumerated(c) // 32), nine_kp(c) // 32
        return -(-(-(-nsteps // nsplit)) // u) * u * 32
    return -(-(-(-(c.B * c.H * c.W) // nsplit)) // 64) * 64


def compute_of(p):
    if p.family == L.WGRAD_NINE:
        return ("wgrad9_kernel", p.kp)
    assert p.family == L.WGRAD_GENERIC, p
    return ("wgrad_kernel", 64, 64, 1, p.kp, p.ns)


def finish_sg(nsplit):
    return 1 if nsplit <= 4 else (8 if nsplit <= 64 else 32)


def nsplit_of(c, kept_tiles):
    return c.nsplit or ops.conv_wgrad_bsparse_plan(geom_of(c), kept_tiles).nsplit


def tags_of(c, nsplit):
    t = set()
    if nsplit == 1:
        t.add("nsplit==1")
    if nsplit > 1 and pixels_enumerated(c) % pix_per_split_of(c, nsplit) != 0:
        t.add("short-last-split")
    if c.dy_choff > 0:
        t.add("dy-slice")
    if c.dbias:
        t.add("dbias")
    if c.pad:
        t.add("shared-halo")
    return t


N64, N32, G1 = ("wgrad9_kernel", 64), ("wgrad9_kernel", 32), ("wgrad_kernel", 64, 64, 1, 64, 3)
VEC = "wgrad_finish_vec_kernel"


def _family(prefix, B, H, W, k, cin, cout, comp, splits):
    """Every mask kind on one shape; the split counts, dy slices and dbias spread over them."""
    out = []
    for i, kind in enumerate(MASK_KINDS):
        ns = splits[i % len(splits)]
        out.append(case("%s-%s" % (prefix, kind), B, H, W, k, cin, cout, kind, (comp, (VEC, k * k, finish_sg(ns or 1))),
                        nsplit=ns, dy_ld=(cout + 64 if i % 2 else 0), dy_choff=(32 if i % 2 else 0),
                        grad_scale=(256.0 if i % 3 == 0 else 1.0), dbias=(i % 3 != 1)))
    return out


WGRAD_BSPARSE_CASES = (
    # 3x3, 64 pixels per step: 2 x 2 tiles; the plan's own split count is 1, 3 splits leave a short last one, 5 reach SG 8
    _family("nine64", 2, 13, 13, 3, 128, 128, N64, (0, 3, 5))
    # 3x3, 32 pixels per step: 1 x 2 tiles
    + _family("nine32", 1, 4, 104, 3, 128, 64, N32, (3, 0, 2))
    # 1x1: one tile is one block
    + _family("one", 2, 13, 13, 1, 128, 128, G1, (0, 2, 5))
    + [
        # the shared-halo form of the operands, and the finish kernel's widest lane grouping (more than 64 slabs)
        case("nine64-shared-halo", 2, 13, 13, 3, 128, 128, "random", (N64, (VEC, 9, 1)), pad=1, nsplit=2, dy_ld=160, dy_choff=16,
             tags=("short-last-split", "dy-slice", "shared-halo", "dbias")),
        # (211 units of 32 padded pixels in 106 splits of one 64-pixel step, the last one 8 pixels; 5408 pixels in 85 splits of
        # one step, the last one 32 pixels)
        case("nine64-106-splits", 8, 27, 27, 3, 64, 64, "holes", (N64, (VEC, 9, 32)), nsplit=106, grad_scale=256.0,
             tags=("short-last-split",)),
        case("one-85-splits", 8, 26, 26, 1, 64, 128, "random", (G1, (VEC, 1, 32)), nsplit=85, tags=("short-last-split",)),
    ])

# what the family cases are there for, by name (tags_of re-derives each)
REQUIRED_TAGS = {"nine64-random": {"nsplit==1"}, "nine64-one-tap": {"short-last-split", "dy-slice"},
                 "nine32-random": {"short-last-split"}, "one-random": {"nsplit==1"}, "one-one-tap": {"short-last-split", "dy-slice"},
                 "nine32-one-tap": {"dy-slice"}, "nine64-full": {"dy-slice"}, "nine64-tile-cleared": {"dbias"}}

# 3x3 geometries whose dense plan is the narrow wgrad9_kernel: the full-list launch at the dense plan's split count must
# equal mcamd_conv_wgrad bit for bit (one per pixels-per-step instance)
DENSE_EQUAL = ("nine64-random", "nine32-random")
