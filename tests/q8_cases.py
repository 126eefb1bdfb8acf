"""The cases of tests/test_q8_instances_gpu.py: launches of mcamd_conv_fwd_q8 (inference and raw fp32 epilogue),
mcamd_conv_fwd_q8_slim and mcamd_conv_fwd_q8_sparse24 (csrc/conv_q8.hip, csrc/conv_q8_sparse.hip, the byte half of conv_epi.h),
their operands and exact references, and the enumeration of what the launches can choose.

test_q8_cases_cpu.py proves on the CPU (through mcamd_conv_fwd_q8_info, which is answered by the launches' own
mcamd_q8_choice()) that Q8_CASES reaches every kernel instance in both MFMA forms with every destination form, every format
pairing and every named boundary condition and value edge, and that every case's reference meets the conditions of
exactness; test_q8_instances_gpu.py runs each case against that reference.  Test-side only.

Why EQUAL is the right comparison.  With d drawn from a conv_cases.DRAWS set (small integers), activations x = d 2^sa have
exact codes a8 = q(2 x); weights w = d 2^-p_f (p_f per filter) quantise to exact codes w8 = w 2^e_f whatever e_f is; every
product is a small integer times one power of two per filter, so the fp32 sum S is exact in any order (condition 1) and so
is v = leaky(scale_f 2^-(e_f + 1) S + shift_f) with scale_f = 2^(p_f - sa) {1/4, 1/2, 1, 2}, shifts in steps of 1/4 and
slope 1/8: v = leaky(c_f I + shift_f) for an integer I.  A byte destination adds ONE rounding, q(2 v), of that exactly
known value -- float64 and torch's float8_e4m3fn cast give its code; an fp16 destination none (condition 2)."""
import collections
import ctypes as C
import zlib

import torch
import torch.nn.functional as F

from modelcompression_amd import ops
from modelcompression_amd import _lib as L
import conv_cases as CC
from conv_cases import DRAWS, SLOPE, _draw, reorg  # noqa: F401  (shared with the fp16 cases)
import sparse_cases as SC
import q8_ref as R
import q8_slim_ref as S8

ENV = "MCAMD_Q8_MFMA"
FORMS = {"dense": ops.Q8_FORM_INFER, "raw": ops.Q8_FORM_RAW, "slim": ops.Q8_FORM_BORDER, "sparse": ops.Q8_FORM_SPARSE}
KERNELS = ("dense", "raw", "border", "sparse")      # conv_q8_kernel<.., RAW = false / true>, conv_q8_border_kernel, conv_q8_sparse_kernel
# (kernel, f8mfma, bmw): bnp is 128 and the ring has 3 stages everywhere; no 256-filter tile in the default form
INSTANCES = tuple((k, m, b) for k in KERNELS for (m, b) in ((0, 128), (0, 64), (1, 256), (1, 128), (1, 64)))
DSTS = CC.DSTS
FMTS = ("f8", "f16", "f8+f16", "f16+f8")
MASK_KINDS = SC.MASK_KINDS

_FIELDS = ("name fam B H W k cin cout pad ld choff y_ld y_choff dst fmt y2_ld y2_choff mask table stats sa slope special draw "
           "wdraw mfma expect tags")


class Case(collections.namedtuple("Case", _FIELDS)):
    """One launch.  fam: "dense" (mcamd_conv_fwd_q8, inference epilogue), "raw" (.., MCAMD_EPI_RAW_F32), "slim"
    (mcamd_conv_fwd_q8_slim; table: with a border table) or "sparse" (mcamd_conv_fwd_q8_sparse24; mask: a sparse_cases kind).
    ld / choff: the operand slice in bytes (ld 0: the slice is the whole buffer); y_ld / y_choff, y2_ld / y2_choff: the
    output slices.  dst: destination form; fmt: the format of y, or of y and y2 ("f8+f16": y bytes, y2 fp16).  stats (raw):
    with the statistics slab.  sa: activations are d 2^sa.  special: value edges planted in particular filters
    ("zeros", "wsub", "overflow"; operands()).  mfma: MCAMD_Q8_MFMA.  expect: (kernel, f8mfma, bmw), the instance.  tags: the
    boundary conditions and value edges the case was written for, each re-derived by boundary_tags() / value_tags()."""
    __slots__ = ()

    def __str__(self):
        return self.name

    @property
    def M(self):
        return self.B * self.H * self.W

    @property
    def k_tap(self):
        """operand channels per tap the K loop reads"""
        return ops.round_up(self.cin, 64)

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
    def y2_slice(self):
        return (self.y2_ld or ops.round_up(self.cout + 40, 32), self.y2_choff if self.y2_ld else 32)

    @property
    def fmt_y(self):
        return self.fmt.split("+")[0]

    @property
    def fmt_y2(self):
        return self.fmt.split("+")[-1]

    @property
    def kernel(self):
        return {"dense": "dense", "raw": "raw", "sparse": "sparse", "slim": "border" if self.table else "dense"}[self.fam]


def case(name, fam, B, H, W, k, cin, cout, expect, mfma=0, pad=0, ld=0, choff=0, y_ld=0, y_choff=0, dst="plain", fmt="f8", y2_ld=0,
         y2_choff=0, mask="two", table=True, stats=True, sa=-1, slope=SLOPE, special=(), draw="d3", wdraw=None, tags=()):
    assert fam in FORMS and dst in DSTS and (dst == "plain" or (H % 2 == 0 and W % 2 == 0))
    assert (fmt in FMTS and ("+" not in fmt or dst == "pool+y2")) or (fam == "raw" and fmt == "f32" and dst == "plain")
    assert (y2_ld == 0 and y2_choff == 0) or dst == "pool+y2"
    assert mask in MASK_KINDS
    return Case(name, fam, B, H, W, k, cin, cout, pad, ld, choff, y_ld, y_choff, dst, fmt, y2_ld, y2_choff,
                mask if fam == "sparse" else None, bool(table) if fam == "slim" else False, bool(stats) if fam == "raw" else False,
                sa, slope, tuple(special), draw, wdraw or draw, int(mfma), tuple(expect), tuple(tags))


def geom_of(c):
    return ops.geom(c.B, c.H, c.W, c.k, c.cin, c.cout, c.ld or c.k_tap, c.choff, pad=c.pad)


def apply_env(c, setenv):
    setenv(ENV, str(c.mfma))


def info_of(c):
    return ops.conv_fwd_q8_info(geom_of(c), FORMS[c.fam])


def instance_of(c, r):
    return (c.kernel, r.f8mfma, r.bmw)


def border_classes(c):
    return set(S8.class_map(c.H, c.W).flatten().tolist())


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
    if c.B > 1 and (c.H * c.W) % r.bnp:
        t.add("tile-spans-images" if c.dst == "plain" else "tile-spans-images-pooled")
    if c.cout < r.bmw:
        t.add("cout<bmw")
    if c.cout % r.bmw:
        t.add("cout%bmw!=0")
    if c.cout % 256:
        t.add("cout%256!=0")
    if c.k == 1 and c.ktot == 64 and r.stages > 1:
        t.add("one-chunk")
    if c.k == 1 and c.ktot == 128 and r.stages > 2:
        t.add("two-chunks")
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
    if c.fam == "slim":
        if c.cin % 64:
            t.add("cin%64!=0")
        if c.cin < 64:
            t.add("cin<64")
        t.add("table" if c.table else "table-null")
        if c.H == 1:
            t.add("H==1")
        if (c.H, c.W) == (2, 2):
            t.add("2x2")
    if c.fam == "raw":
        t.add("stats-on" if c.stats else "stats-off")
        if M % r.bnp:
            t.add("ragged-M")
        if c.cout % r.bmw:
            t.add("ragged-N")
    if c.fam == "sparse":
        t.add("mask-" + c.mask)
    return t


# each of these on the 64-filter tile and on a wider tile, per family and MFMA form
BOUNDARIES_BOTH = ("M<bnp", "M%bnp!=0", "M%bnp==0", "tile-spans-images", "cout%bmw!=0", "cout%256!=0", "ntiles>1",
                   "mtiles>8,mtiles%8!=0", "1x1", "3x3", "padded", "shared-halo", "x_choff>0", "y_choff>0")
BOUNDARIES_INFERENCE = ("tile-spans-images-pooled", "one-chunk", "two-chunks", "y2_choff>0")     # dense and sparse
BOUNDARIES_RAW = ("stats-on", "stats-off", "ragged-M", "ragged-N")
BOUNDARIES_SLIM = ("cin%64!=0", "cin<64", "table", "tile-spans-images-pooled", "y2_choff>0")
BOUNDARIES_64 = ("cout<bmw",)
ALL_BORDER_CLASSES = {0, 1, 2, 4, 8, 5, 9, 6, 10, 3, 7, 11}      # 3x3 classes of a large image, of H = 1 and of 2x2
VALUE_TAGS = ("tie-even", "sat+", "sat-", "underflow-0", "out-subnormal", "pool-mixed-zeros", "a-subnormal", "w-subnormal", "overflow")


# ---------------------------------------------------------------------------------------------------------------------
# what the launches can choose
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_IMAGES = SC.SWEEP_IMAGES


def reachable(setenv):
    """set of (kernel, f8mfma, bmw) over MCAMD_Q8_MFMA 0 and 1 x the four forms x SWEEP_IMAGES x every filter and input-channel
    count from 8 to 1344 in steps of 8 (those the form accepts), by asking the library; bnp, the stages, the tile counts and
    the grid of every answer are checked against the tile on the way."""
    fn = L.lib().mcamd_conv_fwd_q8_info
    g = ops.geom(1, 8, 8, 3, 64, 64, 64)
    out = (C.c_int32 * 7)()
    ref = C.byref(g)
    seen = set()
    for mfma in ("0", "1"):
        setenv(ENV, mfma)
        for kernel, form in (("dense", ops.Q8_FORM_INFER), ("raw", ops.Q8_FORM_RAW), ("border", ops.Q8_FORM_BORDER), ("sparse", ops.Q8_FORM_SPARSE)):
            for (B, H, W) in SWEEP_IMAGES:
                g.B, g.H, g.W = B, H, W
                M = B * H * W
                for cin in range(8, 1345, 8):
                    if form != ops.Q8_FORM_BORDER and cin % 64:
                        continue
                    g.cin, g.x_ld = cin, ops.round_up(cin, 64)
                    for cout in range(8, 1345, 8):
                        g.cout = cout
                        rc = fn(ref, form, out)
                        assert rc == 0, (kernel, B, H, W, cin, cout)
                        bmw, bnp, f8, stages, mtiles, ntiles, grid = out
                        assert bnp == 128 and stages == 3 and f8 == int(mfma)
                        assert mtiles == -(-M // bnp) and ntiles == -(-cout // bmw) and grid == -(-mtiles // 8) * 8 * ntiles
                        seen.add((kernel, f8, bmw))
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# q(), restated on integers (independent of torch's float8 cast)
# ---------------------------------------------------------------------------------------------------------------------
def q_int(v):
    """float64 values -> (e4m3 codes uint8, tie, lower_odd): clamp to +-448, round to nearest, ties to the even code -- on
    integers: |v| = n * step with step the grid spacing at |v| (2^-9 below 2^-6, else 2^(floor(log2 |v|) - 3)), r = floor(n),
    up if the remainder is above 1/2 or equals it with r odd.  tie: v lies exactly halfway between two codes (and is not
    clamped); lower_odd: the code below it (towards zero) is odd."""
    v = v.double()
    neg = torch.signbit(v)
    a = v.abs().clamp(max=448.0)
    _, x = torch.frexp(a)                                    # a = m 2^x, m in [0.5, 1): floor(log2 a) = x - 1
    e = (x - 1).clamp(min=-6)                                # exponent of the grid: subnormals share 2^-6's
    n = a * torch.pow(2.0, (3 - e).double())                 # in [8, 16) for normals, [0, 8) for subnormals: exact (dyadic)
    r = n.floor()
    rem = n - r
    tie = (rem == 0.5) & (v.abs() <= 448.0)
    lower_odd = (r.long() & 1) == 1
    up = (rem > 0.5) | (tie & lower_odd)
    r = (r + up.double()).long()
    carry = r == 16
    e = torch.where(carry, e + 1, e)
    r = torch.where(carry, torch.full_like(r, 8), r)
    code = torch.where(r >= 8, ((e + 7) << 3) | (r - 8), r)  # (r < 8: subnormal, biased exponent 0)
    code = torch.where(a == 0, torch.zeros_like(code), code)
    return (code | (neg.long() << 7)).to(torch.uint8), tie, lower_odd


def _lowbit_units(vals):
    """fp32 e4m3 values -> (value 2^9 as int64, the largest power of two dividing it -- 0 for a zero)"""
    n = (vals.double() * 512.0).long()
    return n, n.abs() & -n.abs()


# ---------------------------------------------------------------------------------------------------------------------
# operands and the exact reference (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
Operands = collections.namedtuple("Operands", "a8 fill w mask p scale shift border planted")
Reference = collections.namedtuple("Reference", "v v2x y y2 raw s1 s2 w8 w8_eff e")
ZERO_FILTER, SUB_FILTER, WSUB_FILTER, SAT_FILTER = 1, 2, 3, 5
PLANT = 256.0                                         # planted d of an "overflow" case: 128 channels x 256 x c 2 = 65536 > 65504


def operands(c, gaussian=False, plant=True):
    """a8: input codes q(2 x) [B][cin][H][W]; fill: non-zero finite codes for the channels [cin, k_tap) the K loop of a slim
    launch also reads (or None); w OIHW fp32; mask OIHW or None; p: the per-filter exponent of the weights; scale / shift
    per filter (None for the raw form); border [16][cout] or None; planted [(b, channel, h, w, sign)] of an overflow case."""
    gen = torch.Generator().manual_seed(zlib.crc32(c.name.split(".")[0].encode()))
    cout = c.cout
    lo, hi = (1, 3) if c.fam == "slim" else (0, 6)
    p = torch.randint(lo, hi + 1, (cout,), generator=gen)
    p[:hi - lo + 1] = torch.arange(lo, hi + 1)[:cout]                  # every exponent occurs, and inside the first tile
    if cout > 64:
        p[-1], p[-2] = hi, lo                                          # ... and the last tile's differ from filter to filter
    if gaussian:
        a8 = R.q(2.0 * F.leaky_relu(torch.randn(c.B, c.cin, c.H, c.W, generator=gen), 0.1))
        w = torch.randn(cout, c.cin, c.k, c.k, generator=gen) * (2.0 / (c.cin * c.ntaps)) ** 0.5
    else:
        x = _draw(gen, DRAWS[c.draw], (c.B, c.cin, c.H, c.W)) * 2.0 ** c.sa
        w = _draw(gen, DRAWS[c.wdraw], (cout, c.cin, c.k, c.k))
        if c.mask in ("two", "bad") and not c.wdraw.startswith("s"):
            w[w == 0] = 1.0                                            # every kept weight counts (sparse_cases.operands)
        w = w * torch.pow(2.0, -p.float()).view(-1, 1, 1, 1)
    mask = None
    if c.fam == "sparse":
        if c.mask == "two":
            mask = SC.mask_two(gen, cout, c.cin, c.k)
        elif c.mask == "upto2":
            mask = SC.mask_random(gen, cout, c.cin, c.k, 0, 2)
            mask[int(torch.randint(6, cout, (1,), generator=gen))] = 0.0
            if c.k == 3:
                mask[:, :, 2, 0] = 0.0
        elif c.mask == "none":
            w = w * SC.mask_two(gen, cout, c.cin, c.k)
        else:
            mask = SC.mask_random(gen, cout, c.cin, c.k, 1, 4)
    c4 = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (cout,), generator=gen)]
    shift = torch.randint(-8, 9, (cout,), generator=gen).float() * 0.25
    border = None
    if c.fam == "slim" and c.table:
        border = torch.randint(-4, 5, (16, cout), generator=gen).float() * 0.25
    fill = None
    if c.k_tap > c.cin:
        fill = (torch.randint(1, 0x7F, (c.B, c.k_tap - c.cin, c.H, c.W), generator=gen, dtype=torch.int32)
                | (torch.randint(0, 2, (c.B, c.k_tap - c.cin, c.H, c.W), generator=gen, dtype=torch.int32) << 7)).to(torch.uint8)
    planted = []
    if not gaussian:
        if "zeros" in c.special:
            # filter ZERO_FILTER: every |2 v| below half the smallest subnormal -- +0 and -0 only; SUB_FILTER: 2 v = I 2^-11
            # (I > 0) or I 2^-14 (I < 0): zeros of both signs, the tie at 2^-10 and subnormal codes
            c4[ZERO_FILTER], shift[ZERO_FILTER] = 2.0 ** -22, 0.0
            c4[SUB_FILTER], shift[SUB_FILTER] = 2.0 ** -12, 0.0
        if "wsub" in c.special:
            # one full-scale weight beside weights 2^-16 of it: codes 256 and d 2^-8 (subnormal)
            assert c.mfma == 0
            f = WSUB_FILTER
            w[f] = w[f] * 2.0 ** -16
            w[f, 0, c.k // 2, c.k // 2] = 2.0 ** -float(p[f])
            if mask is not None:
                mask[f, 0, c.k // 2, c.k // 2] = 1.0
                mask[f, 1:4, c.k // 2, c.k // 2] = torch.tensor([1.0, 0.0, 0.0])
            c4[f], shift[f] = 1.0, 0.25
        if "overflow" in c.special:
            assert c.k == 1 and c.cin == 128 and c.B > 1 and c.sa == -1 and c.slope == 1.0 and c.fam in ("dense", "sparse")
            # (every filter sees the planted pixels: scales 1 and 2 and shifts in steps of 64 keep those values fp16 numbers)
            f = SAT_FILTER
            w[f] = 2.0 ** -float(p[f])
            if mask is not None and c.mask != "two":
                mask[f] = SC.mask_two(gen, 1, c.cin, c.k)[0]
            kept = 64 if c.fam == "sparse" else 128
            c4, shift = torch.where(c4 < 1.0, c4 * 4.0, c4), shift * 256.0
            c4[f], shift[f] = 2.0 * 128 / kept, 0.0
            if plant:
                x[0, :, 1, 2] = PLANT * 2.0 ** c.sa
                x[c.B - 1, :, c.H - 1, c.W - 2] = -PLANT * 2.0 ** c.sa
                planted = [(0, f, 1, 2, 1.0), (c.B - 1, f, c.H - 1, c.W - 2, -1.0)]
        a8 = R.q(2.0 * x)
        assert torch.equal(R.deq(a8), 2.0 * x), "the activation codes are exact"
    if c.fam == "raw":
        return Operands(a8, fill, w, mask, p, None, None, None, planted)
    if gaussian:
        scale, shift = torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.2
    else:
        scale = c4 * torch.pow(2.0, p.float() - c.sa)
    return Operands(a8, fill, w, mask, p, scale, shift, border, planted)


def quantise(c, o):
    """(w8 codes of w * mask, the codes the launch multiplies, exponents): q8_ref.quantise_weights; for the 2:4 form the packer
    keeps the first two non-zeros of w * mask of every group of 4 (sparse_cases.first_two) -- the exponent stays the whole
    filter's."""
    w8, e = R.quantise_weights(o.w, o.mask)
    if c.fam != "sparse":
        return w8, w8, e
    wm = o.w if o.mask is None else o.w * o.mask
    kept = SC.first_two(wm) != 0
    return w8, torch.where(kept, w8, torch.zeros_like(w8)), e


def reference(c, o, slope=None):
    """The exact result of the launch: float64 F.conv2d on deq(a8), deq(w8), q8_ref.block's / q8_slim_ref.block_border's
    epilogue, then q8_ref.store_bytes / store_fp16 per destination.  v: the epilogue value (float64, full resolution);
    y / y2: what the slices must hold (uint8 codes or fp16 values as fp32); raw form: y fp32 = 2^-(e + 1) S and s1 / s2 =
    its per-channel sum and sum of squares over every 128-pixel slab row [rows][cout] (float64)."""
    w8, w8e, e = quantise(c, o)
    slope = c.slope if slope is None else slope
    if c.fam == "raw":
        Sum = F.conv2d(R.deq(o.a8).double(), R.deq(w8e).double(), None, 1, (c.k - 1) // 2)
        raw = Sum * torch.pow(2.0, -(e.double() + 1.0)).view(1, -1, 1, 1)
        flat = raw.permute(0, 2, 3, 1).reshape(c.M, c.cout)
        rows = -(-c.M // 128)
        padded = torch.zeros(rows * 128, c.cout, dtype=torch.float64)
        padded[:c.M] = flat
        padded = padded.view(rows, 128, c.cout)
        return Reference(None, None, raw, None, raw, padded.sum(1), (padded * padded).sum(1), w8, w8e, e)
    if c.fam == "slim":
        v = S8.block_border(o.a8, w8e, e, o.scale, o.shift, o.border, slope, dtype=torch.float64)
        v64 = _v64(c, o, w8e, e, slope)
    else:
        v = R.block(o.a8, w8e, e, o.scale, o.shift, slope, dtype=torch.float64)
        v64 = _v64(c, o, w8e, e, slope)
    assert torch.equal(v.double(), v64), "the epilogue value is an fp32 number"

    def store(fmt, dst):
        return R.store_bytes(v, dst) if fmt == "f8" else R.store_fp16(v, dst)

    dst = "pool" if c.dst == "pool+y2" else c.dst
    y = store(c.fmt_y, dst)
    y2 = store(c.fmt_y2, "plain") if c.dst == "pool+y2" else None
    return Reference(v64, 2.0 * v64, y, y2, None, None, None, w8, w8e, e)


def _v64(c, o, w8e, e, slope):
    """the same value kept in float64 (the references round it to fp32 on return)"""
    Sum = F.conv2d(R.deq(o.a8).double(), R.deq(w8e).double(), None, 1, (c.k - 1) // 2)
    raw = Sum * torch.pow(2.0, -(e.double() + 1.0)).view(1, -1, 1, 1)
    if o.border is not None:
        raw = raw + S8.border_map(o.border, c.H, c.W)
    v = raw * o.scale.double().view(1, -1, 1, 1) + o.shift.double().view(1, -1, 1, 1)
    return torch.where(v > 0, v, v * slope)


_CACHE = {}


def operands_and_reference(c, plant=True):
    """Once per process and case; shared by the tests and never modified."""
    key = (c.name, plant)
    if key not in _CACHE:
        o = operands(c, plant=plant)
        _CACHE[key] = (o, reference(c, o))
    return _CACHE[key]


def byte_outputs(c, ref):
    """[(name, codes at the destination's resolution)] of the byte destinations"""
    out = []
    if c.fam == "raw":
        return out
    if c.fmt_y == "f8":
        out.append(("y", ref.y))
    if c.dst == "pool+y2" and c.fmt_y2 == "f8":
        out.append(("y2", ref.y2))
    return out


def value_tags(c, o, ref):
    """The value edges that occur in this case's reference (CPU)."""
    t = set()
    a = o.a8 & 0x7F
    if c.sa == -10 and bool(((a >= 1) & (a <= 3)).any()) and bool((a <= 3).all()):
        t.add("a-subnormal")
    wa = ref.w8_eff & 0x7F
    for f in range(c.cout):
        if bool(((wa[f] >= 1) & (wa[f] <= 7)).any()) and bool((R.deq(ref.w8_eff[f]).abs() >= 224).any()):
            t.add("w-subnormal")
    if o.planted:
        t.add("overflow")
    outs = byte_outputs(c, ref)
    if not outs:
        return t
    codes = torch.cat([b.flatten() for _, b in outs])
    if bool((codes == 0x7E).any()):
        t.add("sat+")
    if bool((codes == 0xFE).any()):
        t.add("sat-")
    full = R.q(ref.v2x.float())                              # full-resolution codes
    if bool(((full == 0x00) & (ref.v2x != 0)).any()) and bool(((full == 0x80) & (ref.v2x != 0)).any()):
        t.add("underflow-0")
    mag = codes & 0x7F
    if bool(((mag >= 1) & (mag <= 7)).any()):
        t.add("out-subnormal")
    _, tie, odd = q_int(ref.v2x)
    pos, neg = ref.v2x > 0, ref.v2x < 0
    if all(bool((tie & s & o_).any()) for s in (pos, neg) for o_ in (odd, ~odd)):
        t.add("tie-even")
    if c.dst in ("pool", "pool+y2") and c.fmt_y == "f8":
        win = F.unfold(full.float(), 2, stride=2).view(c.B, c.cout, 4, -1)
        has_p, has_n = (win == 0.0).any(2), (win == 128.0).any(2)
        top_is_zero = R.pool_bytes(full).view(c.B, c.cout, -1) == 0
        if bool((has_p & has_n & top_is_zero).any()):
            t.add("pool-mixed-zeros")
    return t


def exactness(c, o, ref):
    """The conditions under which the kernel output must EQUAL `ref`, as a list of violations (empty: all met).
    1. fp32 sums, on the codes: per filter, max |a8| x (sum over k of |w8|) / (the power of two every product of the filter is
       a multiple of) < 2^24 -- every partial sum in every order is an integer multiple of that unit which fp32 holds.
    2. fp16 outputs are fp16 numbers (the planted elements of an overflow case are +-65504); the raw form's are fp32 numbers.
    3. statistics (raw form): per channel, sum of (y / unit)^2 over ALL pixels < 2^24, unit the power of two every y of the
       channel is a multiple of: every partial sum of y and of y^2 is exact whatever pixels a slab row covers.
    4. under MCAMD_Q8_MFMA=1: per filter, max |product| / (the power of two every product is a multiple of) <= 2^10.  The fp8
       MFMAs keep a product 2^-13 of its group's largest; 2^10 leaves three bits of margin.
    All from the reference's operands, never from kernel output."""
    bad = []
    an, au = _lowbit_units(R.deq(o.a8))
    ua = int(au[au > 0].min()) if bool((au > 0).any()) else 1
    amax = int(an.abs().max())
    wn, wu = _lowbit_units(R.deq(ref.w8_eff))
    worst1 = worst4 = 0.0
    for f in range(c.cout):
        nz = wu[f][wu[f] > 0]
        if nz.numel() == 0:
            continue
        uw = int(nz.min())
        worst1 = max(worst1, amax * float(wn[f].abs().sum()) / (ua * uw))
        worst4 = max(worst4, amax * float(wn[f].abs().max()) / (ua * uw))
    if not worst1 < 2 ** 24:
        bad.append("condition 1: bound %r" % worst1)
    if c.mfma and not worst4 <= 2 ** 10:
        bad.append("condition 4: product range %r" % worst4)
    if c.fam == "raw":
        if not torch.equal(ref.raw.float().double(), ref.raw):
            bad.append("condition 2: the raw values are no fp32 numbers")
        if c.stats:
            n = (ref.raw.permute(1, 0, 2, 3).reshape(c.cout, -1) * 2.0 ** 40).long()     # (y is a multiple of 2^-16 below 2^13: exact)
            for f in range(c.cout):
                low = (n[f].abs() & -n[f].abs())
                if not bool((low > 0).any()):
                    continue
                s = float(((n[f] // int(low[low > 0].min())).double() ** 2).sum())
                if not s < 2 ** 24:
                    bad.append("condition 3: filter %d sum of squares %r units" % (f, s))
                    break
        return bad
    for fmt, t in ((c.fmt_y, ref.y), (c.fmt_y2, ref.y2)):
        if t is None or fmt != "f16":
            continue
        dst = ("pool" if c.dst == "pool+y2" else c.dst) if t is ref.y else "plain"
        exact = ref.v
        if o.planted:
            exact = exact.clamp(-65504.0, 65504.0)
        exact = F.max_pool2d(exact, 2, 2) if dst == "pool" else (reorg(exact, 2) if dst == "reorg" else exact)
        if not torch.equal(t.double(), exact):
            bad.append("condition 2: %d values are no fp16 numbers, max |v| %r" % (int((t.double() != exact).sum()), float(exact.abs().max())))
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
# (suffix, image, k, cin, filters on the 64 / 128 / 256 tile, keywords).  Every row runs on every tile of both MFMA forms.
COUTS = {64: 0, 128: 1, 256: 2}
_INFERENCE_ROWS = [
    ("plain", (2, 13, 13), 3, 64, (72, 136, 264), dict(pad=1, y_choff=8, fmt="f8",
     tags=("M%bnp!=0", "tile-spans-images", "cout%bmw!=0", "cout%256!=0", "ntiles>1", "shared-halo", "y_choff>0", "3x3", "tie-even", "sat+"))),
    ("pool", (2, 12, 14), 1, 128, (40, 128, 256), dict(dst="pool", fmt="f16", draw="d2",
     tags=("tile-spans-images-pooled", "1x1", "padded", "two-chunks", "cout<bmw"))),
    ("pool+y2-f8+f16", (2, 12, 14), 3, 64, (64, 200, 320), dict(dst="pool+y2", fmt="f8+f16", ld=128, choff=32, y2_choff=16, draw="d1",
     tags=("x_choff>0", "y2_choff>0"))),
    ("pool+y2-f16+f8", (1, 16, 16), 1, 64, (48, 128, 256), dict(dst="pool+y2", fmt="f16+f8", draw="d2", tags=("M%bnp==0", "one-chunk"))),
    ("pool+y2-f8", (2, 12, 14), 1, 64, (64, 136, 264), dict(dst="pool+y2", fmt="f8", special=("zeros",), y2_choff=8,
     tags=("pool-mixed-zeros", "underflow-0", "out-subnormal", "y2_choff>0"))),
    ("reorg", (1, 16, 16), 1, 64, (24, 128, 320), dict(dst="reorg", fmt="f8", y_choff=16, sa=-10, tags=("y_choff>0", "a-subnormal"))),
    ("reorg-f16", (2, 12, 14), 1, 128, (8, 192, 256), dict(dst="reorg", fmt="f16", draw="d2", pad=1, tags=("shared-halo",))),
    ("walk", (3, 20, 20), 1, 64, (8, 128, 512), dict(fmt="f16", draw="d2", sa=2, tags=("mtiles>8,mtiles%8!=0",))),
    ("one-tile", (2, 9, 7), 3, 64, (64, 128, 256), dict(fmt="f8", slope=1.0, tags=("M<bnp", "sat+", "sat-"))),
]


def _rows(fam, rows, prefix, masks=None):
    out = []
    i = 0
    for mfma, tiles in ((0, (128, 64)), (1, (256, 128, 64))):
        for T in tiles:
            kern = {"dense": "dense", "raw": "raw", "slim": "border", "sparse": "sparse"}[fam]
            for (suffix, (B, H, W), k, cin, couts, kw) in rows:
                kw = dict(kw)
                cout = couts[COUTS[T]]
                if T == 128 and mfma == 0 and suffix in ("plain", "s-plain", "r-stats"):
                    cout = couts[2]                      # (the default form runs 256 filters or more on the 128-filter tile)
                if kw.get("y_choff"):
                    kw["y_ld"] = ops.round_up(kw["y_choff"] + (4 * cout if kw.get("dst") == "reorg" else cout) + 8, 32)
                if kw.get("y2_choff"):
                    kw["y2_ld"] = ops.round_up(kw["y2_choff"] + cout + 8, 32)
                expect = (kern if kw.get("table", True) else "dense", mfma, T)
                if masks:
                    kw["mask"] = masks[i % len(masks)]
                    kw["tags"] = tuple(kw.get("tags", ())) + ("mask-" + kw["mask"],)
                    i += 1
                if T > 64:
                    kw["tags"] = tuple(t for t in kw.get("tags", ()) if t != "cout<bmw")
                out.append(case("%s%d%s-%s" % (prefix, T, "m" if mfma else "", suffix), fam, B, H, W, k, cin, cout, expect, mfma=mfma, **kw))
    return out


DENSE_CASES = _rows("dense", _INFERENCE_ROWS, "d")
DENSE_CASES += [
    # the longest chunk loop of the network (conv21: 1280 channels, 3x3 -- 180 chunks), sparse draws
    case("d128-long-k", "dense", 2, 13, 13, 3, 1280, 256, ("dense", 0, 128), draw="s4", wdraw="s4u", fmt="f8"),
    case("d256m-long-k", "dense", 2, 13, 13, 3, 1280, 256, ("dense", 1, 256), mfma=1, draw="s4", wdraw="s4u", fmt="f16"),
    # one filter whose small weights quantise to subnormal codes beside a full-scale one (default form: condition 4 excludes it)
    case("d64-wsub", "dense", 2, 9, 7, 1, 64, 72, ("dense", 0, 64), fmt="f8", special=("wsub",), tags=("w-subnormal",)),
    case("d128-wsub", "dense", 2, 9, 7, 1, 64, 136, ("dense", 0, 128), fmt="f8", special=("wsub",), tags=("w-subnormal",)),
    # a planted |v| > 65504: the flag is set on an fp16 destination and +-65504 is stored ...
    case("d128-overflow", "dense", 2, 13, 13, 1, 128, 128, ("dense", 0, 128), fmt="f16", slope=1.0, special=("overflow",), tags=("overflow",)),
    case("d128m-overflow", "dense", 2, 13, 13, 1, 128, 128, ("dense", 1, 128), mfma=1, fmt="f16", slope=1.0, special=("overflow",), tags=("overflow",)),
    # ... and stays 0 when only a byte destination saturates
    case("d128-overflow.bytes", "dense", 2, 13, 13, 1, 128, 128, ("dense", 0, 128), fmt="f8", slope=1.0, special=("overflow",),
         tags=("overflow", "sat+", "sat-")),
]

SPARSE_CASES = _rows("sparse", _INFERENCE_ROWS, "s", masks=MASK_KINDS)
SPARSE_CASES += [
    case("s128-long-k", "sparse", 2, 13, 13, 3, 1280, 256, ("sparse", 0, 128), draw="s4", wdraw="s4u", fmt="f8"),
    case("s256m-long-k", "sparse", 2, 13, 13, 3, 1280, 256, ("sparse", 1, 256), mfma=1, draw="s4", wdraw="s4u", fmt="f16"),
    case("s64-wsub", "sparse", 2, 9, 7, 1, 64, 72, ("sparse", 0, 64), fmt="f8", special=("wsub",), tags=("w-subnormal",)),
    case("s128-overflow", "sparse", 2, 13, 13, 1, 128, 128, ("sparse", 0, 128), fmt="f16", slope=1.0, special=("overflow",), tags=("overflow",)),
]

_SLIM_ROWS = [
    ("s-plain", (2, 13, 13), 3, 72, (72, 136, 264), dict(fmt="f8", y_choff=8,
     tags=("cin%64!=0", "table", "M%bnp!=0", "tile-spans-images", "cout%bmw!=0", "cout%256!=0", "ntiles>1", "3x3", "y_choff>0", "padded"))),
    ("s-pool+y2-f8+f16", (2, 8, 6), 3, 40, (24, 128, 256), dict(dst="pool+y2", fmt="f8+f16", y2_choff=16, draw="d2",
     tags=("cin<64", "M<bnp", "y2_choff>0", "cout<bmw"))),
    ("s-pool+y2-f16+f8", (2, 12, 14), 1, 136, (64, 200, 320), dict(dst="pool+y2", fmt="f16+f8", draw="d2", ld=256, choff=32,
     tags=("tile-spans-images-pooled", "1x1", "x_choff>0"))),
    ("s-pool-2x2", (1, 2, 2), 3, 328, (56, 136, 392), dict(dst="pool", fmt="f16", draw="d1", tags=("2x2", "M<bnp"))),
    ("s-reorg", (1, 16, 16), 3, 40, (8, 128, 256), dict(dst="reorg", fmt="f8", pad=1, tags=("M%bnp==0", "shared-halo", "cin<64"))),
    ("s-h1", (2, 1, 5), 3, 72, (16, 128, 256), dict(fmt="f16", draw="d2", tags=("H==1",))),
    ("s-walk", (3, 20, 20), 1, 8, (8, 136, 264), dict(fmt="f8", slope=1.0, tags=("mtiles>8,mtiles%8!=0", "cin<64"))),
    ("s-null", (2, 9, 11), 3, 72, (72, 200, 264), dict(fmt="f8", table=False, tags=("table-null", "cin%64!=0"))),
    ("s-null-cin128", (1, 16, 16), 1, 128, (64, 128, 256), dict(fmt="f8", table=False, tags=("table-null",))),
]
SLIM_CASES = _rows("slim", _SLIM_ROWS, "b")
SLIM_CASES += [
    case("b128-long-k", "slim", 2, 13, 13, 3, 1280, 256, ("border", 0, 128), draw="s4", wdraw="s4u", fmt="f8"),
]

_RAW_ROWS = [
    ("r-stats", (2, 9, 11), 3, 64, (72, 200, 264), dict(fmt="f32", y_choff=8, tags=("stats-on", "ragged-M", "ragged-N", "y_choff>0", "3x3",
     "tile-spans-images", "M%bnp!=0", "cout%bmw!=0", "cout%256!=0", "ntiles>1", "padded"))),
    ("r-nostats", (1, 16, 16), 1, 64, (64, 128, 256), dict(fmt="f32", stats=False, ld=128, choff=16, tags=("stats-off", "M%bnp==0", "1x1", "x_choff>0"))),
    ("r-walk", (3, 20, 20), 1, 128, (40, 136, 392), dict(fmt="f32", pad=1, sa=-10, tags=("stats-on", "mtiles>8,mtiles%8!=0", "shared-halo", "ragged-N", "cout<bmw"))),
    ("r-one-tile", (2, 9, 7), 3, 64, (64, 128, 256), dict(fmt="f32", tags=("M<bnp", "stats-on"))),
]
RAW_CASES = _rows("raw", _RAW_ROWS, "r")
RAW_CASES += [
    case("r128-long-k", "raw", 2, 13, 13, 3, 1280, 256, ("raw", 0, 128), draw="s4", wdraw="s4u", fmt="f32"),
]

Q8_CASES = DENSE_CASES + RAW_CASES + SLIM_CASES + SPARSE_CASES

# one case per kernel and MFMA form: run twice on Gaussian data, bit-equal
DETERMINISM_CASES = ("d128-plain", "d256m-pool+y2-f8+f16", "r128-r-stats", "r256m-r-stats", "b64-s-plain", "b256m-s-pool+y2-f16+f8",
                     "s128-pool+y2-f16+f8", "s256m-plain")


# ---------------------------------------------------------------------------------------------------------------------
# one-hot filters: which k every operand lane (and, for 2:4, every index bit-field) selects
# ---------------------------------------------------------------------------------------------------------------------
OneHot = collections.namedtuple("OneHot", "fam k cin")
ONEHOT_CASES = [OneHot("dense", 1, 64), OneHot("dense", 1, 128), OneHot("dense", 3, 64), OneHot("dense", 1, 256),
                OneHot("sparse", 1, 64), OneHot("sparse", 1, 128), OneHot("sparse", 3, 64), OneHot("sparse", 1, 256)]


def onehot_id(h):
    return "%s-k%d-cin%d" % (h.fam, h.k, h.cin)


def onehot_case(h, mfma):
    cout = h.k * h.k * h.cin
    bmw = (256 if mfma else 128) if cout >= 256 else (128 if cout >= 128 else 64)
    return case("onehot-%s%s" % (onehot_id(h), "-m" if mfma else ""), h.fam, 2, 3, 3, h.k, h.cin, cout, (h.fam, mfma, bmw), mfma=mfma,
                fmt="f16", slope=1.0, mask="none")


def onehot_operands(h):
    """(a8 [2][cin][3][3], w OIHW, [(channel, tap, sign)] per filter): one filter per (channel, tap) with the weight +-1 there
    (code 0x58 = 256 with e = 8), in a shuffled order.  Image 0 names the channel -- every pixel of channel c holds the code
    0x08 + c % 112 (distinct values within any 64-channel block, all normal), negative for c >= 112 --, image 1 the tap: pixel
    p holds the code 0x10 + p in every channel.  The centre pixel of the output is +-deq(code) / 2 of the selected element."""
    c = onehot_case(h, 0)
    gen = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    ch = torch.arange(h.cin)
    a8 = torch.zeros(2, h.cin, 3, 3, dtype=torch.uint8)
    a8[0] = ((0x08 + ch % 112) | ((ch >= 112).long() << 7)).to(torch.uint8).view(-1, 1, 1)
    a8[1] = (0x10 + torch.arange(9)).to(torch.uint8).view(1, 3, 3)
    order = torch.randperm(c.cout, generator=gen).tolist()
    sign = (torch.randint(0, 2, (c.cout,), generator=gen) * 2 - 1).tolist()
    w = torch.zeros(c.cout, h.cin, h.k, h.k)
    which = []
    for f in range(c.cout):
        chan, tap = divmod(order[f], c.ntaps)
        w[f, chan, tap // h.k, tap % h.k] = float(sign[f])
        which.append((chan, tap, sign[f]))
    return a8, w, which
