"""The cases of tests/test_bn1x1_instances_gpu.py -- bn_conv1x1_kernel<BN, CB> (csrc/bn_conv1x1.hip) behind
mcamd_bn_act_conv1x1_fwd: a PLAIN block's BatchNorm + LeakyReLU fused into the split-operand 1x1 forward that follows it --
with their operands, float64 references, conditions of exactness, and the enumeration of what the launch can choose.

test_bn1x1_cases_cpu.py proves on the CPU (through mcamd_bn_act_conv1x1_info, the launch's own choice function) that the
table reaches every instance and every boundary condition below on both column tiles, and that every reference meets the
conditions; test_bn1x1_instances_gpu.py runs each case against its reference.  Test-side only.

The kernel computes, per pixel m and filter f,
    v = leaky(y[m][c] * scale[c] + shift[c]),  hi = fp16(clamp(v, +-65504)),  lo = fp16(v - hi),
    out[m][f] = sum_c hi w_hi + sum_c lo w_hi + sum_c hi w_lo,   w_hi = fp16(w), w_lo = fp16(w - w_hi)
in fp32 on the fp16 MFMAs, stores hi, and sums out and out^2 per filter into the statistics slab.  The reference restates
that in float64 from y, scale, shift, slope and the fp32 master weights: the planes through act_ref (one fp32 rounding of z,
one of the slope product, one fp16 rounding), the sums as three float64 matrix products over the planes.

Kind "exact": the GEMM is held to EQUALITY
  The lo plane is the rounding residual of the activation, so the planes cannot be drawn independently (split_cases' wrap
  operands); y is built so that the kernel's own conversion yields small-integer planes:
    target v = 1024 d + e / 4, d in {+-1, +-2, +-3}, e in {-1, 0, 1}, and e does not point towards zero where |d| = 1
    (1023.75 is a rounding tie between 1023.5 and 1024).  The fp16 spacing in [1024, 4096) is 1 or 2, so fp16(v) = 1024 d
    with no tie and lo = v - hi = e / 4 exactly.
    z = v (v > 0 or slope 1) or v / slope (slope 0.125: z = 8 v); scale = +-2^j, j in [-2, 2]; shift = s 2^j, s in [-3, 3];
    y = (z - shift) / scale.  z - shift is a multiple of 1/4 below 2^15: 17 bits, so y is an fp32 number, y * scale is exact
    and the sum with the shift is z exactly, fused or not.  z * 0.125 is exact.
    w = a + b 2^-11, a in {0, +-2, +-3}, b in {-1, 0, 1}, b = 0 where a = 0 (split_cases' f8 scheme), through the production
    packer (mcamd_pack_job.split 1): w_hi = a, w_lo = b 2^-11.
  Every product is a multiple of UNIT = 1/4 (hi a: integers; lo a: quarters; hi b 2^-11 = d b / 2).
  One-hot cases (`special`): pixel m has ONE non-zero channel (11 m) % P with v = 1024 d (+ e / 4: "onehot-lo") against
  filters that hold a distinct integer per channel, rotated per filter: a = A[(c + f) % P], A[k] = +-(k + 4), b = +-1.
  out[m][f] is then ONE triple of products that names the channel the value was laid at: the register-piece -> LDS row /
  column map of stage() for every CB and row group.  "onehot-hi" has lo = 0 (a part 1 that reads hi[] doubles the result);
  "onehot-lo" has lo != 0 (a part 0 or 2 that reads lo[] loses 1024 d a).

Kind "value": the edges of the conversion, slope 0.1
  y and the coefficients on act_cases' exact-product grid (y a multiple of 2^-12 below 128, scales with 3 significant bits:
  y * scale is exact, so z is rounded once, fused or not) with act_cases' planted channels 0-9: |v| > 65504 (hi clamps to
  +-65504 and lo holds the rest), an fp16-subnormal v, z = +0 and z = -0, negative scales, both LeakyReLU sides; and scale 0
  in channel 10.  Gaussian weights.  The hi plane is held to EQUALITY; out and the slab to the float64 sums within derived
  bounds, and -- in the GPU test -- to the two-launch route bit for bit.

Conditions of exactness (exactness(), asserted on operands and reference, never on kernel output)
  1. exact: per output, sum |products| / UNIT < 2^24: every partial sum in every order is a multiple of UNIT that fp32 holds.
  2. exact: out is held to equality.  The slab cannot be exact at this unit; it is held to the float64 sums of the exact out
     within gamma_n sum |terms|, gamma_n = n 2^-24 / (1 - n 2^-24), n the channel's pixel count (n - 1 fp32 additions and the
     one rounding of out^2), for s1 over |out| and s2 over out^2 (split_cases' condition 3).
  3. value: every product of two fp16 numbers is exact in fp32, so out differs from the float64 sum by the K - 1 = 3 P - 1
     fp32 additions only: |out - ref| <= bound = gamma_K sum |products|, K = 3 P, per output.  The slab sums the kernel's own
     out: |s1 - sum ref| <= sum bound + gamma_n sum (|ref| + bound), |s2 - sum ref^2| <= sum bound (2 |ref| + bound) + gamma_n
     sum (|ref| + bound)^2.  With bound = 0 this is condition 2.  Derived, not measured."""
import collections
import zlib

import torch

from modelcompression_amd import ops
from modelcompression_amd import _lib as L
import act_cases as A
import act_ref as R

UNIT = 0.25
SLOPES = (0.1, 0.125, 1.0)
INSTANCES = ((64, 1), (64, 2), (128, 1), (128, 2), (128, 3), (128, 4))
SENTINEL_LO = 7.25                      # finite: a launch that wrote the lo plane, or read it, shows
DRAW_D = (-3, -2, -1, 1, 2, 3)
DRAW_A = (-3, -2, 0, 2, 2, 3)
DRAW_B = (-1, 0, 0, 1, 1)
SCALE0_CH = 10                          # value cases: the channel with scale 0 (act_cases plants channels 0-9)

_FIELDS = "name kind B H W P cout slope py_ld py_choff ld choff y_ld y_choff stats special expect tags"


class Case(collections.namedtuple("Case", _FIELDS)):
    """One launch of mcamd_bn_act_conv1x1_fwd.  P: the producer's channels; cout: the consumer's filters.  py_ld / py_choff:
    the producer's fp32 raw output slice; ld / choff: the destination's [hi | lo] slice; y_ld / y_choff: the output slice.
    stats: with a statistics slab.  special: None or a one-hot kind.  expect: (BN, CB).  tags: boundary conditions the case
    was written for, each re-derived by boundary_tags()."""
    __slots__ = ()

    def __str__(self):
        return self.name

    @property
    def M(self):
        return self.B * self.H * self.W


def case(name, kind, B, H, W, P, cout, expect, slope=None, py_extra=0, py_choff=0, x_extra=0, choff=0, y_extra=0, y_choff=0,
         stats=True, special=None, tags=()):
    """py_extra / x_extra / y_extra: channels of the buffer behind the slice"""
    slope = (0.1 if kind == "value" else 0.125) if slope is None else slope
    assert kind in ("exact", "value") and (kind == "value") == (slope == 0.1) and special in (None, "onehot-hi", "onehot-lo")
    return Case(name, kind, B, H, W, P, cout, slope, py_choff + P + py_extra, py_choff, choff + 2 * P + x_extra, choff,
                y_choff + cout + y_extra, y_choff, stats, special, tuple(expect), tuple(tags))


def act_desc_of(c):
    """the activation pass of the pair as a descriptor without pointers"""
    return ops.act_geom(c.B, c.H, c.W, c.P, c.py_ld, c.py_choff, c.slope, L.DST_PLAIN, c.ld, c.choff, planes=2, dst_plane=c.P, dst_pad=0)


def geom_of(c):
    return ops.geom(c.B, c.H, c.W, 1, 3 * c.P, c.cout, c.ld, c.choff, 0, 0, 2 * c.P)


def info_of(c):
    return ops.bn_act_conv1x1_info(act_desc_of(c), geom_of(c))


def slope_tag(s):
    return "slope=%g" % s


def boundary_tags(c, info):
    """The named boundary conditions this launch meets, from the query's answer and the case's shape alone."""
    t = set()
    M = c.M
    if M < 128:
        t.add("M<128")
    elif M == 128:
        t.add("M==128")
    else:
        t.add("M%128==0" if M % 128 == 0 else "M%128!=0")       # several tiles: all full / the last one ragged
    if c.B > 1 and (c.H * c.W) % 128:
        t.add("tile-spans-images")
    t.add("cout==BN" if c.cout == info.bn else "cout<BN")
    if c.py_choff % 8 == 4:
        t.add("py_choff%8==4")
    if c.py_ld > c.P:
        t.add("py_ld>P")
    if c.choff > 0:
        t.add("x_choff>0")
    if c.ld > 2 * c.P:
        t.add("x_ld>2P")
    if c.y_choff > 0:
        t.add("y_choff>0")
    if c.y_ld > c.cout:
        t.add("y_ld>cout")
    t.add("stats-on" if c.stats else "stats-off")
    if info.num_mtiles > info.rows:
        t.add("mtiles>slots")
    t.add(slope_tag(c.slope))
    return t


# every tag the table must carry on each column tile; "mtiles>slots" needs more than 2048 tiles of 128 pixels and stays with
# test_bn_conv1x1_gpu.py::test_persistent_workgroup_takes_two_tiles (PERSISTENT_SHAPE below is that test's shape)
BOUNDARIES = ("M<128", "M==128", "M%128==0", "M%128!=0", "tile-spans-images", "cout==BN", "cout<BN", "py_choff%8==4", "py_ld>P",
              "x_choff>0", "x_ld>2P", "y_choff>0", "y_ld>cout", "stats-on", "stats-off") + tuple(slope_tag(s) for s in SLOPES)


def persistent_case():
    """the shape of test_persistent_workgroup_takes_two_tiles, as a Case (never launched from this table)"""
    P, cout = 128, 64
    cap = info_of(case("probe", "value", 1, 512, 512, P, cout, (64, 2))).rows
    return case("persistent", "value", 1, 512, (128 * cap) // 512 + 1, P, cout, (64, 2))


# ---------------------------------------------------------------------------------------------------------------------
# what the launch can choose
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_IMAGES = ((1, 3, 5), (1, 8, 16), (2, 9, 8), (3, 7, 7), (2, 16, 16), (5, 13, 13))
SWEEP_P = tuple(range(64, 513, 64))
SWEEP_COUT = tuple(range(8, 265, 8))


def reachable():
    """{(BN, CB): an accepted (B, H, W, P, cout)} by asking the library over SWEEP_IMAGES x SWEEP_P x SWEEP_COUT."""
    seen = {}
    for (B, H, W) in SWEEP_IMAGES:
        for P in SWEEP_P:
            for cout in SWEEP_COUT:
                c = case("sweep", "value", B, H, W, P, cout, (0, 0))
                d, g = act_desc_of(c), geom_of(c)
                if not ops.bn_act_conv1x1_ok(d, g):
                    continue
                i = ops.bn_act_conv1x1_info(d, g)
                assert i.cb == P // 64 and i.bn >= cout and i.threads == 4 * i.bn and i.num_mtiles == -(-c.M // 128), (c, i)
                assert i.rows == ops.bn_act_conv1x1_stats_rows(d, g) == ops.stats_rows(g, L.EPI_RAW_F32), (c, i)
                seen.setdefault((i.bn, i.cb), (B, H, W, P, cout))
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# operands and the float64 reference (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
Operands = collections.namedtuple("Operands", "y scale shift slope w d e a b")
"""y [M][P] float64 (fp32 numbers); scale, shift fp32 [P]; w fp32 [cout][P] the master for the production packer.  exact:
d, e [M][P] the intended planes (hi = 1024 d, lo = e / 4), a, b [cout][P] the intended weight parts (w_hi = a, w_lo = b 2^-11)."""
Reference = collections.namedtuple("Reference", "v hi lo w_hi w_lo y absprod s1 s2")
"""float64: v, hi, lo [M][P]; w_hi, w_lo [cout][P]; y [M][cout]; absprod [M][cout] = sum |products|; s1, s2 [cout]"""


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.name.encode()))


def _draw(gen, values, shape):
    t = torch.tensor(values, dtype=torch.float64)
    return t[torch.randint(0, len(values), shape, generator=gen)]


def _exact_y(v, scale, shift, slope):
    z = torch.where(v > 0, v, v / slope)
    return (z - shift.double()) / scale.double()


def _exact_operands(c, gen):
    M, P, n = c.M, c.P, c.cout
    d = _draw(gen, DRAW_D, (M, P))
    e = _draw(gen, (-1, 0, 1), (M, P))
    e = torch.where(d.abs() == 1, e.abs() * d.sign(), e)                  # |v| >= 1024: no rounding tie at 1023.75
    j = torch.randint(-2, 3, (P,), generator=gen).double()
    sign = torch.where(torch.randint(0, 3, (P,), generator=gen) == 0, -1.0, 1.0).double()
    scale = (sign * 2.0 ** j).float()
    shift = (torch.randint(-3, 4, (P,), generator=gen).double() * 2.0 ** j).float()
    a = _draw(gen, DRAW_A, (n, P))
    b = _draw(gen, DRAW_B, (n, P))
    b = torch.where(a != 0, b, torch.zeros_like(b))               # (+0, not -1 * 0 = -0: the packer's w - fp16(w) is +0)
    return Operands(_exact_y(1024 * d + e / 4, scale, shift, c.slope), scale, shift, c.slope, (a + b * 2.0 ** -11).float(), d, e, a, b)


def onehot_channel(m, P):
    return (11 * m) % P


def _onehot_operands(c):
    M, P, n = c.M, c.P, c.cout
    m = torch.arange(M)
    ch = onehot_channel(m, P)
    d = torch.zeros(M, P, dtype=torch.float64)
    e = torch.zeros(M, P, dtype=torch.float64)
    dm = (1 + m % 3).double() * torch.where(m % 2 == 0, 1.0, -1.0).double()
    d[m, ch] = dm
    if c.special == "onehot-lo":
        e[m, ch] = torch.where(m % 5 < 2, -1.0, 1.0).double()
        e = torch.where(d.abs() == 1, e.abs() * d.sign(), e)
    scale, shift = torch.ones(P), torch.zeros(P)
    f, k = torch.arange(n).view(n, 1), torch.arange(P).view(1, P)
    r = (k + f) % P
    a = ((r + 4) * torch.where(r % 2 == 0, 1, -1)).double()
    b = torch.where((k + 2 * f) % 2 == 0, 1.0, -1.0).double().expand(n, P).contiguous()
    return Operands(_exact_y(1024 * d + e / 4, scale, shift, c.slope), scale, shift, c.slope, (a + b * 2.0 ** -11).float(), d, e, a, b)


class _ActView(collections.namedtuple("_ActView", "y32 mode H W")):
    """what act_cases.exactness and act_ref.activation read of a case: an fp32 y, PLAIN, no border"""


_ACT = _ActView(True, A.PLAIN, 1, 1)


def _as_act(o):
    """[M][P] operands as act_cases.Operands (NCHW [M][P][1][1])"""
    return A.Operands(o.y.view(o.y.shape[0], -1, 1, 1), o.scale, o.shift, o.slope, None)


def _value_operands(c, gen):
    M, P, n = c.M, c.P, c.cout
    g = 2.0 ** -12
    y = torch.randint(-int(128 / g) + 1, int(128 / g), (M, P), generator=gen).double() * g
    mant = 1.0 + 0.25 * torch.randint(0, 4, (P,), generator=gen).double()
    sign = torch.where(torch.randint(0, 4, (P,), generator=gen) == 0, -1.0, 1.0).double()
    scale = (sign * mant * 2.0 ** torch.randint(-3, 3, (P,), generator=gen).double()).float()
    shift = (torch.randn(P, generator=gen) * 2).float()
    # act_cases' planted channels: clamps, a subnormal, z = -0 and +0, +-1024; channel 2 reaches -65504 THROUGH the slope
    # (z about -700 000, v about -70 000), so hi clamps on both signs and both LeakyReLU sides
    for ch, (sc, sh) in enumerate(((1.0, 70000.0), (-1.25, 70000.0), (1.0, -700000.0), (1.0, 300.0), (1.5, -300.0),
                                   (0.125, 2.0 ** -15), (-1.5, -0.0), (1.75, 0.0), (1.0, 1024.0), (1.0, -1024.0))):
        scale[ch], shift[ch] = sc, sh
    y[0, 5:8] = 0.0                                   # pixel 0: v = 2^-15 (fp16-subnormal), z = -0, z = +0
    w = torch.randn(n, P, generator=gen) * 0.05
    return Operands(y, scale, shift, c.slope, w.float(), None, None, None, None)


def operands(c):
    gen = _gen(c)
    if c.special:
        return _onehot_operands(c)
    if c.kind == "exact":
        return _exact_operands(c, gen)
    o = _value_operands(c, gen)
    # scale 0 is off act_cases' grid (its exactness() wants 3-bit mantissas): planted after that check, in exactness() below
    return o


def with_scale0(o):
    """the value operands as launched: channel SCALE0_CH has scale 0 (v = leaky(shift) at every pixel)"""
    scale = o.scale.clone()
    scale[SCALE0_CH] = 0.0
    return o._replace(scale=scale)


def launched(c, o):
    return with_scale0(o) if c.kind == "value" else o


def reference(c, o):
    """From y, scale, shift, slope and the master weights alone (never from the intended planes)."""
    o = launched(c, o)
    v = R.activation(_ACT, _as_act(o)).view(o.y.shape)
    hi, lo = R.hi16(v).double(), R.lo16(v).double()
    w_hi = o.w.half().double()
    w_lo = (o.w.double() - w_hi).float().half().double()
    y = hi @ w_hi.t() + lo @ w_hi.t() + hi @ w_lo.t()
    absprod = hi.abs() @ w_hi.abs().t() + lo.abs() @ w_hi.abs().t() + hi.abs() @ w_lo.abs().t()
    return Reference(v, hi, lo, w_hi, w_lo, y, absprod, y.sum(0), (y * y).sum(0))


def gamma(n):
    return n * 2.0 ** -24 / (1.0 - n * 2.0 ** -24)


def y_bound(c, ref):
    """conditions 2 and 3: the allowed |out - ref.y| per output -- zero for the exact kind"""
    if c.kind == "exact":
        return torch.zeros_like(ref.y)
    return gamma(3 * c.P) * ref.absprod


def stats_bounds(c, ref):
    """conditions 2 and 3: (bound on |s1 - sum ref.y|, bound on |s2 - sum ref.y^2|) per channel"""
    b = y_bound(c, ref)
    g = gamma(c.M)
    top = ref.y.abs() + b
    return b.sum(0) + g * top.sum(0), (b * (2 * ref.y.abs() + b)).sum(0) + g * (top * top).sum(0)


def exactness(c, o, ref):
    """Violations of the conditions in the module docstring (empty: all met), from the operands and the reference alone."""
    bad = []
    if not torch.equal(o.y.float().double(), o.y):
        bad.append("y is no fp32 number")
    if not torch.equal(ref.y.float().double(), ref.y) and c.kind == "exact":
        bad.append("the reference is no fp32 number")
    if c.kind == "value":
        try:
            A.exactness(_ACT, _as_act(o))                # the grid conditions, before the scale-0 channel is planted
        except AssertionError as err:
            bad.append("act_cases.exactness: %s" % err)
        lo_ = launched(c, o)
        z = lo_.y * lo_.scale.double() + lo_.shift.double()
        if not torch.equal(z[:, SCALE0_CH], lo_.shift.double()[SCALE0_CH].expand(c.M)):
            bad.append("the scale-0 channel does not evaluate to its shift")
        if not bool(torch.isfinite(ref.lo).all()):
            bad.append("a lo value is not finite")
        return bad
    sc, sh = o.scale.double(), o.shift.double()
    p = o.y * sc
    if not torch.equal(p, R.fl32(p)):
        bad.append("y * scale is not exact in fp32")
    z = p + sh
    bb = z - p
    if not bool((((p - (z - bb)) + (sh - bb)) == 0).all()) or not torch.equal(z, R.fl32(z)):
        bad.append("y * scale + shift is not exact")
    s32 = torch.tensor(o.slope, dtype=torch.float32).double()
    if not torch.equal(z * s32, R.fl32(z * s32)):
        bad.append("the slope product is not exact")
    if not torch.equal(ref.v, 1024 * o.d + o.e / 4):
        bad.append("v is not the target 1024 d + e / 4")
    if not torch.equal(ref.hi, 1024 * o.d) or not torch.equal(ref.lo, o.e / 4):
        bad.append("the reference's planes are not the intended integers")
    if not torch.equal(ref.w_hi, o.a) or not torch.equal(ref.w_lo, o.b * 2.0 ** -11):
        bad.append("fp16(w) != a or fp16(w - a) != b 2^-11")
    worst = float(ref.absprod.max()) / UNIT
    if not worst < 2 ** 24:
        bad.append("condition 1: sum |products| = %r units of 1/4" % worst)
    if not torch.equal(ref.y / UNIT, (ref.y / UNIT).round()):
        bad.append("the reference is no multiple of 1/4")
    return bad


def planted_edges(c, ref):
    """value cases: the conversion edges missing from the reference (empty: all present)"""
    v, hi, lo = ref.v, ref.hi, ref.lo
    miss = []
    if not (bool((hi == 65504).any()) and bool((hi == -65504).any())):
        miss.append("hi clamps on both signs")
    if not bool(((hi.abs() == 65504) & (lo.abs() > 32)).any()):
        miss.append("a clamped hi whose lo holds the rest")
    if not bool(((v != 0) & (v.abs() < 2.0 ** -14)).any()):
        miss.append("an fp16-subnormal v")
    if not (bool(((v == 0) & torch.signbit(v)).any()) and bool(((v == 0) & ~torch.signbit(v)).any())):
        miss.append("z = +0 and z = -0")
    if not (bool((v < 0).double().mean() > 0.2) and bool((v > 0).double().mean() > 0.2)):
        miss.append("both LeakyReLU sides")
    if not bool((v[:, SCALE0_CH] == v[0, SCALE0_CH]).all()):
        miss.append("a scale-0 channel")
    if not float((lo != 0).double().mean()) > 0.5:
        miss.append("a lo plane that is mostly non-zero")
    return miss


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
# every slice inside a larger buffer: the producer's y at a 4-channel offset (the alignment edge of the 16-byte loads)
SLICES = dict(py_extra=8, py_choff=4, x_extra=16, choff=8, y_extra=8, y_choff=4)

CASES = [
    # ---- bn_conv1x1_kernel<64, 1>
    case("e-64x1-m15", "exact", 1, 3, 5, 64, 64, (64, 1), tags=("M<128", "cout==BN", "stats-on", "slope=0.125")),
    case("e-64x1-m128-n56-nostats", "exact", 1, 8, 16, 64, 56, (64, 1), slope=1.0, stats=False,
         tags=("M==128", "cout<BN", "stats-off", "slope=1")),
    case("v-64x1-m147-n48-slices", "value", 3, 7, 7, 64, 48, (64, 1), tags=("M%128!=0", "tile-spans-images", "cout<BN", "py_choff%8==4",
         "py_ld>P", "x_choff>0", "x_ld>2P", "y_choff>0", "y_ld>cout", "slope=0.1"), **SLICES),
    # ---- <64, 2>
    case("e-64x2-m144-n40-slices", "exact", 2, 9, 8, 128, 40, (64, 2), slope=1.0, tags=("M%128!=0", "tile-spans-images", "cout<BN",
         "py_choff%8==4", "py_ld>P", "x_choff>0", "x_ld>2P", "y_choff>0", "y_ld>cout"), **SLICES),
    case("e-64x2-m256", "exact", 2, 8, 16, 128, 64, (64, 2), tags=("M%128==0",)),
    case("v-64x2-m15-nostats", "value", 1, 3, 5, 128, 64, (64, 2), stats=False, tags=("M<128", "stats-off")),
    case("v-64x2-m128-n56", "value", 1, 8, 16, 128, 56, (64, 2), tags=("M==128",), py_choff=4, py_extra=4),
    # ---- <128, 1>
    case("e-128x1-m15", "exact", 1, 3, 5, 64, 128, (128, 1), tags=("M<128", "cout==BN", "slope=0.125")),
    case("v-128x1-m144-slices", "value", 2, 9, 8, 64, 128, (128, 1), tags=("M%128!=0", "tile-spans-images", "py_choff%8==4", "py_ld>P",
         "x_choff>0", "x_ld>2P", "y_choff>0", "y_ld>cout", "slope=0.1"), **SLICES),
    # ---- <128, 2>
    case("e-128x2-m144-n104-slices", "exact", 2, 9, 8, 128, 104, (128, 2), slope=1.0, tags=("M%128!=0", "tile-spans-images", "cout<BN",
         "py_choff%8==4", "py_ld>P", "x_choff>0", "x_ld>2P", "y_choff>0", "y_ld>cout", "slope=1"), **SLICES),
    case("v-128x2-m128-n112", "value", 1, 8, 16, 128, 112, (128, 2), tags=("M==128", "cout<BN")),
    # ---- <128, 3>
    case("e-128x3-m128-n120-nostats", "exact", 1, 8, 16, 192, 120, (128, 3), slope=1.0, stats=False,
         tags=("M==128", "cout<BN", "stats-off")),
    case("v-128x3-m147", "value", 3, 7, 7, 192, 128, (128, 3), stats=False, tags=("M%128!=0", "tile-spans-images", "stats-off")),
    case("e-128x3-m15-slices", "exact", 1, 3, 5, 192, 128, (128, 3), tags=("M<128", "py_choff%8==4", "x_choff>0"), **SLICES),
    # ---- <128, 4>
    case("e-128x4-m256", "exact", 2, 8, 16, 256, 128, (128, 4), tags=("M%128==0", "cout==BN", "stats-on")),
    case("v-128x4-m144-n104-slices", "value", 2, 9, 8, 256, 104, (128, 4), tags=("M%128!=0", "cout<BN", "py_choff%8==4", "y_choff>0"),
         **SLICES),
    case("e-128x4-m147-n120", "exact", 3, 7, 7, 256, 120, (128, 4), slope=1.0, tags=("tile-spans-images", "cout<BN")),
]

# the register-piece -> LDS map of stage(), in every instance: 296 pixels = two full tiles and a ragged one, every channel hit
ONEHOT = [case("onehot-%dx%d-%s" % (bn, cb, kind[7:]), "exact", 1, 8, 37, 64 * cb, bn, (bn, cb), slope=1.0, special=kind)
          for (bn, cb) in INSTANCES for kind in ("onehot-hi", "onehot-lo")]

EXACT = [c for c in CASES if c.kind == "exact"]
VALUE = [c for c in CASES if c.kind == "value"]
assert len({c.name for c in CASES + ONEHOT}) == len(CASES) + len(ONEHOT)
