"""The cases of tests/test_sparse_instances_gpu.py: launches of mcamd_conv_fwd_sparse24 (csrc/conv_sparse.hip), their
operands, masks and exact references, the packing restated in Python, and the enumeration of what the launch can choose.

test_sparse_cases_cpu.py proves on the CPU (through mcamd_conv_fwd_sparse24_info, which is answered by the launch's own
mcamd_sparse24_choice()) that SPARSE_CASES reaches every sparse24_kernel instance with every destination form and every
named boundary condition, and that every case's reference meets the conditions of exactness of conv_cases.py;
test_sparse_instances_gpu.py runs each case against that reference.  Test-side only."""
import collections
import ctypes as C
import zlib

import torch

from modelcompression_amd import ops
from modelcompression_amd import _lib as L
import conv_cases as CC
from conv_cases import DRAWS, SLOPE, _draw, reorg, exactness, Operands  # noqa: F401  (shared with the dense cases)

ENV_DEFAULTS = {"MCAMD_SPARSE_WIDE": "1"}
WIDE0 = {"MCAMD_SPARSE_WIDE": "0"}

# sparse24_kernel<BMW, BNP, .., BK, 2> as (bmw, bnp, bk)
I256, I128, I64, I128K32, I64K32 = (256, 128, 64), (128, 128, 64), (64, 128, 64), (128, 128, 32), (64, 128, 32)
INSTANCES = (I256, I128, I64, I128K32, I64K32)
DSTS = CC.DSTS
MASK_KINDS = ("two", "upto2", "none", "bad")

_FIELDS = "name B H W k cin cout pad ld choff y_ld y_choff dst y2_ld y2_choff mask overflow draw wdraw env expect tags"


class Case(collections.namedtuple("Case", _FIELDS)):
    """One launch of mcamd_conv_fwd_sparse24.
    ld / choff: the operand slice (ld 0: the slice is the whole buffer).  y_ld / y_choff: the output slice (y_ld 0: the
    whole buffer); y2_ld / y2_choff: that of the full-resolution copy of dst "pool+y2".
    mask: "two"   exactly 2 of every 4 consecutive input channels at each (filter, tap), non-zero weights;
          "upto2" 0, 1 or 2 of 4, one filter removed, one tap removed in every filter (3x3);
          "none"  no mask, over weights that are 2:4 already and hold zeros at kept positions;
          "bad"   a mask that does NOT conform (1 to 4 of 4): the packer keeps the first two non-zeros in channel order
                  (include/mcamd.h), which first_two() restates for the reference.
    draw / wdraw: conv_cases.DRAWS keys of the activation and the weight values.  overflow: two planted elements beyond
    the fp16 range.  expect: (bmw, bnp, bk), the instance.  tags: the boundary conditions the case was written for, each
    re-derived from the info query by boundary_tags().
    (epi, fwd, n, M, k_tap, ktot, stem, concurrent: what conv_cases.reference / exactness read from a dense case.)"""
    __slots__ = ()
    epi, fwd, stem, concurrent = "fwd-pad", True, 0, False

    def __str__(self):
        return self.name

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
        return 4 * self.cout if self.dst == "reorg" else self.cout

    @property
    def y2_slice(self):
        """(ld, choff) of the full-resolution copy"""
        return (self.y2_ld or ops.round_up(self.cout + 40, 32), self.y2_choff if self.y2_ld else 32)


def case(name, B, H, W, k, cin, cout, expect, mask="two", pad=0, ld=0, choff=0, y_ld=0, y_choff=0, dst="plain", y2_ld=0,
         y2_choff=0, overflow=False, draw="d3", wdraw=None, env=None, tags=()):
    assert dst in DSTS and mask in MASK_KINDS and (dst == "plain" or (H % 2 == 0 and W % 2 == 0))
    assert (y2_ld == 0 and y2_choff == 0) or dst == "pool+y2"
    return Case(name, B, H, W, k, cin, cout, pad, ld, choff, y_ld, y_choff, dst, y2_ld, y2_choff, mask, overflow, draw,
                wdraw or draw, dict(env or {}), tuple(expect), tuple(tags))


def geom_of(c):
    return ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, c.ld or c.k_tap, c.choff, pad=c.pad)


def apply_env(c, setenv):
    for name, default in ENV_DEFAULTS.items():
        setenv(name, c.env.get(name, default))


def info_of(c):
    return ops.conv_fwd_sparse24_info(geom_of(c))


def boundary_tags(c, r):
    """The named boundary conditions this launch meets, from the info query's tile and grid and the case's shape alone."""
    t = set()
    M = c.M
    if M < r.bnp:
        t.add("M<bnp")
    elif M % r.bnp:
        t.add("M%bnp!=0")
    if M % r.bnp == 0:
        t.add("M%bnp==0")
    if c.B > 1 and (c.H * c.W) % r.bnp:          # (pooled order: 4 rows per pooled pixel, the same condition)
        t.add("tile-spans-images" if c.dst == "plain" else "tile-spans-images-pooled")
    if c.cout < r.bmw:
        t.add("cout<bmw")
    if c.cout % r.bmw:
        t.add("cout%bmw!=0")
    if c.cout % 256:
        t.add("cout%256!=0")
    if c.k_tap > c.cin:
        t.add("k-padded")
    if r.bk == 32 and c.k_tap % 64:
        t.add("bk32-by-cin_tap%64")
    if c.k == 1 and c.ktot // r.bk == 1 and r.stages > 1:
        t.add("one-chunk")
    if c.choff > 0 and c.ld > c.choff + c.k_tap:
        t.add("x_choff>0")
    if c.y_choff > 0 and c.y_ld > c.y_choff + c.cdst:
        t.add("y_choff>0")
    if c.dst == "pool+y2" and c.y2_slice[1] > 0 and c.y2_slice[0] > c.y2_slice[1] + c.cout:
        t.add("y2_choff>0")
    t.add("shared-halo" if c.pad else "padded")
    t.add("1x1" if c.k == 1 else "3x3")
    if r.ntiles > 1:
        t.add("ntiles>1")
    if r.mtiles > 8 and r.mtiles % 8:
        t.add("mtiles>8,mtiles%8!=0")
        assert r.grid > r.mtiles * r.ntiles      # blocks that only pad the grid
    if c.env.get("MCAMD_SPARSE_WIDE", "1") == "0" and c.cout >= 256:
        t.add("wide-off")
    return t


# each of these on the 64-filter tile and on a 128- or 256-filter tile
BOUNDARIES_BOTH = ("M<bnp", "M%bnp!=0", "M%bnp==0", "tile-spans-images", "tile-spans-images-pooled", "cout%bmw!=0",
                   "cout%256!=0", "k-padded", "bk32-by-cin_tap%64", "one-chunk", "x_choff>0", "y_choff>0", "y2_choff>0",
                   "padded", "shared-halo", "1x1", "3x3", "ntiles>1", "mtiles>8,mtiles%8!=0")
BOUNDARIES_64 = ("cout<bmw",)                    # (below 128 filters the tile is the 64-filter one)
BOUNDARIES_WIDE = ("wide-off",)                  # (256 filters or more)
PADDED_CINS = (4, 12, 40, 72)                    # multiples of 4 that are no multiple of 32: each in some case


# ---------------------------------------------------------------------------------------------------------------------
# what the launch can choose
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_IMAGES = ((1, 1, 1), (2, 9, 7), (1, 16, 16), (3, 20, 20), (64, 26, 26))


def reachable(setenv):
    """set of (bmw, bnp, bk, stages) over MCAMD_SPARSE_WIDE 0 and 1 x SWEEP_IMAGES x both kernel sizes x every filter and
    input-channel count from 8 to 1344 in steps of 8, by asking the library; the tile counts and the grid of every answer
    are checked against the tile on the way."""
    fn = L.lib().mcamd_conv_fwd_sparse24_info
    g = ops.geom(1, 8, 8, 3, 32, 32, 32)
    out = (C.c_int32 * 7)()
    ref = C.byref(g)
    seen = set()
    for wide in ("0", "1"):
        setenv("MCAMD_SPARSE_WIDE", wide)
        for (B, H, W) in SWEEP_IMAGES:
            g.B, g.H, g.W = B, H, W
            M = B * H * W
            for k in (1, 3):
                g.ksize = k
                for cin in range(8, 1345, 8):
                    g.cin, g.x_ld = cin, ops.round_up(cin, 32)
                    for cout in range(8, 1345, 8):
                        g.cout = cout
                        rc = fn(ref, out)
                        assert rc == 0, (B, H, W, k, cin, cout)
                        bmw, bnp, bk, stages, mtiles, ntiles, grid = out
                        assert mtiles == -(-M // bnp) and ntiles == -(-cout // bmw) and grid == -(-mtiles // 8) * 8 * ntiles
                        assert bk == (64 if g.x_ld % 64 == 0 else 32)
                        seen.add((bmw, bnp, bk, stages))
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# masks, the packer's rule and the packing, restated (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def _groups(t):
    """OIHW -> [cout][cin / 4][4][k][k]: the groups of 4 consecutive input channels"""
    return t.view(t.shape[0], t.shape[1] // 4, 4, t.shape[2], t.shape[3])


def mask_two(gen, cout, cin, k):
    """exactly 2 of 4, the pair drawn among all six"""
    pair = torch.randint(0, 6, (cout, cin // 4, k, k), generator=gen)
    table = torch.zeros(6, 4)
    for i, (a, b) in enumerate(PAIRS):
        table[i, a] = table[i, b] = 1.0
    return table[pair].permute(0, 1, 4, 2, 3).reshape(cout, cin, k, k).contiguous()


def mask_random(gen, cout, cin, k, lo, hi):
    """lo .. hi of 4, at random positions"""
    nkeep = torch.randint(lo, hi + 1, (cout, cin // 4, k, k), generator=gen)
    order = torch.rand(cout, cin // 4, k, k, 4, generator=gen).argsort(-1)
    return (order < nkeep.unsqueeze(-1)).float().permute(0, 1, 4, 2, 3).reshape(cout, cin, k, k).contiguous()


def first_two(v):
    """The packer's documented rule (mcamd_pack_sparse24): of every group of 4 consecutive input channels at one (filter,
    tap) the first two non-zeros of v = w * mask in channel order are kept.  The identity on a conforming v."""
    g = _groups(v)
    nz = g != 0
    keep = nz & (nz.long().cumsum(2) <= 2)
    return torch.where(keep, g, torch.zeros_like(g)).reshape(v.shape)


def group_counts(v):
    """non-zeros per group of 4"""
    return (_groups(v) != 0).long().sum(2)


def packed_k_order(v, c):
    """OIHW [cout][cin][k][k] -> [cout][ktot] in the packed K order [channel block][tap][kb], channels zero-padded to k_tap"""
    cout = v.shape[0]
    p = torch.zeros(cout, c.k_tap, c.ntaps, dtype=v.dtype)
    p[:, :c.cin] = v.reshape(cout, c.cin, c.ntaps)
    return p.view(cout, c.k_tap // c.kb, c.kb, c.ntaps).permute(0, 1, 3, 2).reshape(cout, c.ktot).contiguous()


Packed = collections.namedtuple("Packed", "dense vals p0 p1")


def pack_ref(c, w, mask):
    """pack_sparse24_kernel in plain terms.  dense: (w * mask) in packed K order [cout][ktot] (fp32); vals: the kept fp16
    values [cout][ktot / 2]; p0, p1: the 2-bit offsets of the two slots of every group [cout][ktot / 4].  A group with two
    or more non-zeros keeps the first two; with one at offset o, the slots are (0, 1) if o == 0 else (0, o); with none (0, 1)."""
    v = w if mask is None else w * mask
    dense = packed_k_order(v, c)
    g = dense.view(dense.shape[0], c.ktot // 4, 4)
    nz = (g != 0).long()
    cum = nz.cumsum(-1)
    cnt = cum[..., 3]
    first = (nz * (cum == 1)).argmax(-1)
    second = (nz * (cum == 2)).argmax(-1)
    p0 = torch.where(cnt >= 2, first, torch.zeros_like(first))
    p1 = torch.where(cnt >= 2, second, torch.where((cnt == 1) & (first > 0), first, torch.ones_like(first)))
    vals = torch.stack([g.gather(-1, p0.unsqueeze(-1)).squeeze(-1), g.gather(-1, p1.unsqueeze(-1)).squeeze(-1)], -1)
    return Packed(dense, vals.reshape(dense.shape[0], c.ktot // 2).half(), p0, p1)


def decode_packed(c, vals, idx):
    """The device's packing (flat fp16 values, flat int16 index words) -> (vals [npad][ktot / 2], p0, p1 [npad][ktot / 4],
    dense [npad][ktot]): the index words are read in the stored order [ktot / 32][npad][2]; slot j of group G of a row is
    bits [2 j, 2 j + 2) of the 4-bit field G % 4 of word (G / 4) % 2 of K32 chunk G / 8."""
    npad = ops.round_up(c.cout, 256)
    vals = vals.view(npad, c.ktot // 2).cpu()
    words = (idx.view(c.ktot // 32, npad, 2).cpu().to(torch.int32) & 0xFFFF).permute(1, 0, 2).reshape(npad, c.ktot // 16)
    sh = torch.arange(4, dtype=torch.int32) * 4
    p0 = ((words.unsqueeze(-1) >> sh) & 3).reshape(npad, c.ktot // 4).long()
    p1 = ((words.unsqueeze(-1) >> (sh + 2)) & 3).reshape(npad, c.ktot // 4).long()
    dense = torch.zeros(npad, c.ktot // 4, 4, dtype=torch.float16)
    v = vals.view(npad, c.ktot // 4, 2)
    dense.scatter_(-1, p1.unsqueeze(-1), v[..., 1:2])          # (where p0 == p1 -- never, if the packing is right -- slot 0 wins)
    dense.scatter_(-1, p0.unsqueeze(-1), v[..., 0:1])
    return vals, p0, p1, dense.view(npad, c.ktot)


# ---------------------------------------------------------------------------------------------------------------------
# operands and the exact reference (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
SAT_FILTER = 5
SAT_W, SAT_POS, SAT_NEG = 32.0, 64.0, -256.0      # 64 kept weights: 64 * 32 * 64 * 2 = 262144; 64 * 32 * -256 * 2 / 8 = -131072


def operands(c, gaussian=False, plant=True):
    """conv_cases.Operands: act x [B][cin][H][W]; w OIHW; mask OIHW or None (kind "none"); scale / shift per filter;
    planted [(b, channel, h, w, sign)] of an `overflow` case."""
    gen = torch.Generator().manual_seed(zlib.crc32(c.name.split(".")[0].encode()))
    if gaussian:
        act = torch.randn(c.B, c.cin, c.H, c.W, generator=gen)
        w = torch.randn(c.cout, c.cin, c.k, c.k, generator=gen) * (4.0 / c.ktot) ** 0.5
    else:
        act = _draw(gen, DRAWS[c.draw], (c.B, c.cin, c.H, c.W))
        w = _draw(gen, DRAWS[c.wdraw], (c.cout, c.cin, c.k, c.k))
    if c.mask in ("two", "bad") and not gaussian and not c.wdraw.startswith("s"):
        w[w == 0] = 1.0                            # every kept weight counts (the sparse draws keep their zeros)
    if c.mask == "two":
        mask = mask_two(gen, c.cout, c.cin, c.k)
    elif c.mask == "upto2":
        mask = mask_random(gen, c.cout, c.cin, c.k, 0, 2)
        mask[int(torch.randint(0, c.cout, (1,), generator=gen))] = 0.0
        if c.k == 3:
            mask[:, :, 2, 0] = 0.0
    elif c.mask == "none":
        w = w * mask_two(gen, c.cout, c.cin, c.k)
        mask = None
    else:
        mask = mask_random(gen, c.cout, c.cin, c.k, 1, 4)
    scale = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (c.cout,), generator=gen)]
    shift = torch.randint(-8, 9, (c.cout,), generator=gen).float() * 0.25
    planted = []
    if c.overflow and not gaussian:
        assert c.k == 1 and c.cin == 128 and c.mask == "two" and c.B > 1
        # (every filter sees the planted pixels: scales 1 and 2 and shifts in steps of 64 keep those values fp16 numbers)
        w[SAT_FILTER] = SAT_W
        scale, shift = torch.where(scale < 1.0, scale * 4.0, scale), shift * 256.0
        scale[SAT_FILTER], shift[SAT_FILTER] = 2.0, 0.0
        if plant:
            act[0, :, 1, 2] = SAT_POS
            act[c.B - 1, :, c.H - 1, c.W - 2] = SAT_NEG
            planted = [(0, SAT_FILTER, 1, 2, 1.0), (c.B - 1, SAT_FILTER, c.H - 1, c.W - 2, -1.0)]
    return Operands(act, w, mask, None, scale, shift, planted)


def effective(o):
    """The weights the launch multiplies: the packer's rule applied to w * mask (OIHW, fp32)."""
    return first_two(o.w if o.mask is None else o.w * o.mask)


def reference(c, o):
    """conv_cases.reference (float64 F.conv2d, the inference epilogue, max_pool2d / reorg, the clamp of planted elements)
    of x with the effective weights."""
    return CC.reference(c, o._replace(w=effective(o), mask=None))


_CACHE = {}


def operands_and_reference(c, plant=True):
    """Once per process and case; shared by the tests and never modified."""
    key = (c.name, plant)
    if key not in _CACHE:
        o = operands(c, plant=plant)
        _CACHE[key] = (o, reference(c, o))
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
E = I256
SPARSE_CASES = [
    # ---- sparse24_kernel<256, 128, 64, 64, 64, 2>: 256 filters or more, 64-channel blocks (swz<4> weight rows)
    case("s256-plain", 2, 13, 13, 3, 64, 264, E, "two", pad=1, draw="d2", y_ld=288, y_choff=8,
         tags=("M%bnp!=0", "tile-spans-images", "cout%bmw!=0", "cout%256!=0", "ntiles>1", "shared-halo", "y_choff>0", "3x3")),
    case("s256-pool", 2, 12, 14, 1, 128, 256, E, "upto2", dst="pool", draw="d2", tags=("tile-spans-images-pooled", "1x1", "padded")),
    case("s256-pool+y2", 2, 12, 14, 3, 40, 256, E, "none", dst="pool+y2", ld=128, choff=32, y2_ld=320, y2_choff=16,
         tags=("k-padded", "x_choff>0", "y2_choff>0")),
    case("s256-reorg", 1, 16, 16, 1, 64, 320, E, "bad", dst="reorg", y_ld=1312, y_choff=16,
         tags=("M%bnp==0", "one-chunk", "cout%256!=0", "y_choff>0")),
    case("s256-walk", 3, 20, 20, 1, 64, 512, E, "upto2", tags=("mtiles>8,mtiles%8!=0", "ntiles>1", "one-chunk")),
    case("s256-one-tile", 2, 9, 7, 3, 64, 256, E, "two", draw="d2", tags=("M<bnp",)),
    # the longest chunk loop of the network (conv21: 1280 channels, 3x3 -- 180 chunks), sparse draws
    case("s256-long-k", 2, 13, 13, 3, 1280, 256, E, "two", draw="s4", wdraw="s4u"),
]

E = I128
SPARSE_CASES += [
    # ---- sparse24_kernel<128, 128, 64, 64, 64, 2>: 128 .. 248 filters, or MCAMD_SPARSE_WIDE=0
    case("s128-plain", 2, 13, 13, 3, 128, 136, E, "two", draw="d2", y_ld=160, y_choff=16,
         tags=("cout%bmw!=0", "cout%256!=0", "ntiles>1", "tile-spans-images", "M%bnp!=0", "y_choff>0")),
    case("s128-pool", 2, 12, 14, 3, 64, 128, E, "bad", dst="pool", pad=1, draw="d2", tags=("shared-halo", "tile-spans-images-pooled", "3x3")),
    case("s128-pool+y2", 2, 12, 14, 1, 64, 200, E, "upto2", dst="pool+y2", y2_ld=256, y2_choff=8, tags=("one-chunk", "y2_choff>0", "1x1")),
    case("s128-reorg", 2, 12, 14, 1, 104, 128, E, "none", dst="reorg", ld=192, choff=32, tags=("k-padded", "x_choff>0")),
    case("s128-wide-off-plain", 2, 13, 13, 3, 64, 264, E, "two", env=WIDE0, tags=("wide-off", "ntiles>1", "cout%256!=0")),
    case("s128-wide-off-pool", 3, 20, 20, 1, 64, 256, E, "upto2", dst="pool", env=WIDE0, tags=("wide-off", "mtiles>8,mtiles%8!=0")),
    case("s128-one-tile", 2, 9, 7, 1, 128, 128, E, "none", tags=("M<bnp",)),
    case("s128-whole-tiles", 1, 16, 16, 3, 64, 128, E, "upto2", tags=("M%bnp==0",)),
    case("s128-saturate", 2, 13, 13, 1, 128, 128, E, "two", overflow=True),
]

E = I64
SPARSE_CASES += [
    # ---- sparse24_kernel<64, 128, 32, 64, 64, 2>: below 128 filters; its index region is a quarter (K32 steps x 256 bytes)
    # of the 1024 bytes one DMA instruction fetches
    case("s64-plain", 2, 13, 13, 3, 64, 72, E, "two", pad=1,
         tags=("cout%bmw!=0", "cout%256!=0", "ntiles>1", "shared-halo", "tile-spans-images", "M%bnp!=0")),
    case("s64-pool", 2, 12, 14, 1, 64, 40, E, "upto2", dst="pool", y_ld=64, y_choff=16,
         tags=("cout<bmw", "one-chunk", "tile-spans-images-pooled", "y_choff>0", "1x1")),
    case("s64-pool+y2", 2, 12, 14, 3, 40, 64, E, "bad", dst="pool+y2", ld=128, choff=32, y2_ld=96, y2_choff=16,
         tags=("k-padded", "x_choff>0", "y2_choff>0", "3x3")),
    case("s64-reorg", 1, 16, 16, 1, 128, 24, E, "none", dst="reorg", tags=("M%bnp==0", "cout<bmw", "padded")),
    case("s64-walk", 3, 20, 20, 1, 64, 8, E, "two", tags=("mtiles>8,mtiles%8!=0",)),
    case("s64-one-tile", 2, 9, 7, 3, 64, 64, E, "upto2", tags=("M<bnp",)),
]

E = I128K32
SPARSE_CASES += [
    # ---- sparse24_kernel<128, 128, 64, 64, 32, 2>: 32-channel blocks (the padded channel count is no multiple of 64): the
    # packed K order [channel block][tap][32] with several blocks, unswizzled weight rows
    case("s128k32-plain", 2, 13, 13, 3, 72, 264, E, "two", draw="d2",
         tags=("k-padded", "bk32-by-cin_tap%64", "ntiles>1", "cout%bmw!=0", "cout%256!=0", "tile-spans-images", "M%bnp!=0", "3x3")),
    case("s128k32-pool", 2, 12, 14, 1, 32, 128, E, "upto2", dst="pool", pad=1, tags=("one-chunk", "shared-halo", "tile-spans-images-pooled")),
    case("s128k32-pool+y2", 2, 12, 14, 3, 96, 136, E, "none", dst="pool+y2", draw="d2", y2_ld=192, y2_choff=24, tags=("y2_choff>0",)),
    case("s128k32-reorg", 2, 12, 14, 1, 12, 128, E, "bad", dst="reorg", y_ld=576, y_choff=32, tags=("k-padded", "one-chunk", "y_choff>0")),
    case("s128k32-one-tile", 2, 9, 7, 1, 96, 128, E, "bad", ld=160, choff=32, tags=("M<bnp", "x_choff>0", "1x1")),
    case("s128k32-walk", 3, 20, 20, 3, 32, 128, E, "two", tags=("mtiles>8,mtiles%8!=0", "padded")),
    case("s128k32-whole-tiles", 1, 16, 16, 1, 264, 192, E, "none", draw="d2", tags=("M%bnp==0", "k-padded")),
]

E = I64K32
SPARSE_CASES += [
    # ---- sparse24_kernel<64, 128, 32, 64, 32, 2>
    case("s64k32-plain", 2, 13, 13, 3, 4, 72, E, "two", ld=64, choff=16, y_ld=96, y_choff=8,
         tags=("k-padded", "x_choff>0", "y_choff>0", "ntiles>1", "cout%bmw!=0", "tile-spans-images", "M%bnp!=0", "3x3")),
    case("s64k32-pool", 2, 12, 14, 3, 96, 64, E, "upto2", dst="pool", tags=("bk32-by-cin_tap%64", "tile-spans-images-pooled", "padded")),
    case("s64k32-pool+y2", 2, 12, 14, 1, 32, 48, E, "bad", dst="pool+y2", y2_ld=96, y2_choff=8,
         tags=("cout<bmw", "one-chunk", "y2_choff>0", "1x1")),
    case("s64k32-reorg", 1, 16, 16, 1, 72, 120, E, "none", dst="reorg", pad=1, tags=("M%bnp==0", "shared-halo", "k-padded", "cout%256!=0")),
    case("s64k32-one-tile", 2, 9, 7, 3, 32, 64, E, "two", tags=("M<bnp",)),
    case("s64k32-walk", 3, 20, 20, 1, 96, 16, E, "upto2", dst="pool", tags=("mtiles>8,mtiles%8!=0",)),
]

# one case per instance: run twice on Gaussian data, bit-equal
DETERMINISM_CASES = ("s256-plain", "s128-pool+y2", "s64-pool", "s128k32-reorg", "s64k32-plain")


# ---------------------------------------------------------------------------------------------------------------------
# one-hot filters: which k every index bit-field and every operand lane selects
# ---------------------------------------------------------------------------------------------------------------------
OneHot = collections.namedtuple("OneHot", "k cin image env expect")
# image "1x1": one pixel, channel c holds c + 1; "3x3": nine pixels, channel c of pixel p holds 9 c + p + 1 (3x3 filters only:
# the tap is identified too).  One filter per (channel, tap), in a shuffled order: cout = k * k * cin.
ONEHOT_CASES = [
    OneHot(1, 64, "1x1", {}, I64), OneHot(1, 128, "1x1", {}, I128), OneHot(1, 256, "1x1", {}, I256),
    OneHot(1, 96, "1x1", {}, I64K32), OneHot(1, 264, "1x1", {}, I128K32), OneHot(1, 40, "1x1", {}, I64),
    OneHot(3, 64, "1x1", {}, I256), OneHot(3, 64, "3x3", {}, I256), OneHot(3, 64, "3x3", WIDE0, I128),
    OneHot(3, 96, "1x1", {}, I128K32), OneHot(3, 96, "3x3", {}, I128K32),
    OneHot(3, 72, "3x3", {}, I128K32), OneHot(3, 40, "3x3", {}, I256), OneHot(3, 8, "3x3", {}, I64K32),
]


def onehot_id(h):
    return "k%d-cin%d-%s%s" % (h.k, h.cin, h.image, "-wide-off" if h.env else "")


def onehot_case(h):
    n = 3 if h.image == "3x3" else 1
    return case("onehot-" + onehot_id(h), 1, n, n, h.k, h.cin, h.k * h.k * h.cin, h.expect, env=h.env)


def onehot_operands(h):
    """(x [1][cin][n][n], w OIHW, [(channel, tap, sign)] per filter).  Every value stays below 2048: exact in fp16."""
    c = onehot_case(h)
    gen = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
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
