"""The cases of tests/test_split_instances_gpu.py -- the forward convolutions of the default training precision in their two
operand forms -- with their operands, exact references, conditions of exactness, and the enumeration of what the launches
can choose.

  "wrap"  mcamd_conv_geom.x_wrap: two activation planes [x_hi | x_lo] of P channels against the K-concatenated weights
          [W0 | W1 | W2] of a 3 P channel filter; the third part reads the hi plane again.  igemm_kernel, igemm_pp_kernel and
          small3x3_split_kernel; epilogues MCAMD_EPI_RAW_F32 with statistics ("raw32") and MCAMD_EPI_NCHW_F32 ("nchw").
  "f8"    mcamd_conv_geom.x_f8: the hi plane in fp16 and the e4m3 byte planes [lo8 | x8] against [w_hi | w8 | wlo8]; fp16 chunks
          and then fp8 chunks (v_mfma_scale_f32_32x32x64_f8f6f4) into the same accumulators.  The four F8 instances of
          igemm_pp_kernel, epilogue "raw32" only.

test_split_cases_cpu.py proves on the CPU (through mcamd_conv_route_info, the launches' own route function) that the table
reaches every instance the route rules can name and every boundary condition below, and that every reference meets the
conditions of exactness; test_split_instances_gpu.py runs each case against its reference.  Test-side only.

Operands, and why EQUAL is the right comparison
  wrap  x_hi and x_lo are INDEPENDENT small-integer draws (not a value and its rounding residual), W0, W1, W2 three
        independent integer parts, packed with the plain forward packing of the 3 P channel geometry -- licensed by
        test_split_packing_is_plain_packing_of_concatenation (pack_many(split=True) of w is bit for bit the plain packing of
        cat([w_hi, w_hi, w_lo], 1)).  Reference: float64 conv(x_hi, W0) + conv(x_lo, W1) + conv(x_hi, W2) (+ bias).  A kernel
        that reads the wrong plane for a part is off by an integer; channels of the buffer outside [x_choff, x_choff + 2 P)
        hold NaN, so a third part that does not wrap reads NaN.
        small3x3_split_kernel keeps ONE copy of w_hi in registers for parts 0 and 1 -- the packing contract is
        [w_hi | w_hi | w_lo] -- so its cases tie W1 = W0 (`tie`); the planes and W2 stay independent.
  f8    x_hi small integers; the byte planes are written directly as integer-valued e4m3 codes drawn independently of x_hi
        (the activation pass that produces them in production is checked byte for byte by test_f8_correction_forward).  The
        weights go through the production packer (mcamd_pack_job.split = 2) as w = a + b 2^-11 with a in {0, +-2, +-3}, b in
        {-1, 0, 1} and b = 0 where a = 0 (b 2^-11 alone IS an fp16 number: it would become w_hi).  Then fp16(w) = a, w - a =
        b 2^-11, w8 = a 2^e and wlo8 = b 2^e are exact codes for every exponent e used, and
            y = conv(x_hi, a) + 2^-12 (conv(lo8, a) + conv(x8, b)),
        a multiple of 2^-12 that does not depend on e.  Every case runs at three exponents, one negative.
        One-hot cases (`special`): 1x1, 256 pixels, pixel m has ONE non-zero byte, at position m % 64 of fp8 chunk
        (m / 64) % 4 -- [lo8 0:64, lo8 64:128, x8 0:64, x8 64:128] of P = 128 -- against filters whose byte at position k is
        a distinct code, rotated per filter: "onehot-w8" w = A[(c + f) % 64] (64 distinct signed e4m3 integers up to 64),
        "onehot-wlo8" w = 128 + A[(c + 3 f) % 64] 2^-11.  That pins that A and B of the 64-k instruction are gathered with
        the same k map, and the packer's byte placement.

Conditions of exactness (exactness(), asserted on the operands of every case)
  1. per output, sum of |products| / unit < 2^24 (unit 1 for wrap, 2^-12 for f8), from max|.| x max|.| x K: every partial
     sum in every order is a multiple of the unit that fp32 holds.
  2. wrap: per channel, the sum of y^2 over all pixels < 2^24: every partial sum of y and y^2 is an exact fp32 integer
     whatever pixels a slab row covers; the statistics are held to EQUALITY.
  3. f8: the unit 2^-12 makes 2. unattainable.  y is held to equality; the slab to the float64 sums of that exact y within
     gamma_n sum|terms|, gamma_n = n 2^-24 / (1 - n 2^-24), n the channel's pixel count (n - 1 fp32 additions and the one
     rounding of y^2), per channel, for s1 over |y| and s2 over y^2 (stats_bounds()).  Derived, not measured.
  4. f8: the block-scaled MFMA truncates inside groups of 8 products (include/mcamd.h on MCAMD_Q8_MFMA); q8_cases' MFMA-form
     cases are exact while max |product| / (the power of two every product is a multiple of) <= 2^10.  Here every code and
     every a, b is an integer, so the condition is max(|lo8| |a|, |x8| |b|) <= 2^10 (F8_PRODUCT_RANGE)."""
import collections
import ctypes as C
import zlib

import torch
import torch.nn.functional as F

from modelcompression_amd import ops
from modelcompression_amd import _lib as L
from conv_cases import (DRAWS, _draw, apply_env, ENV_DEFAULTS, IGEMM, PP, KERNEL_NAMES, PP2, PP2_192, PP2_N128,  # noqa: F401
                        PP2_192_N128)

SPLIT = ops.ROUTE_SMALL3X3_SPLIT
UNIT_F8 = 2.0 ** -12
F8_PRODUCT_RANGE = 2 ** 10

# (form, epilogue) -> (mode, statistics slab) of mcamd_conv_route_info.  "f8-nchw" only exists in the sweep of reachable():
# the route function answers for it, the launch refuses it (test_split_refusals).
FORMS = {"wrap-raw32": (L.EPI_RAW_F32, True), "wrap-nchw": (L.EPI_NCHW_F32, False),
         "f8-raw32": (L.EPI_RAW_F32, True), "f8-nchw": (L.EPI_NCHW_F32, False)}
CASE_FORMS = ("wrap-raw32", "wrap-nchw", "f8-raw32")

DRAW_A = (-3, -2, 0, 2, 2, 3)            # hi parts of the f8 weights
DRAW_B = (-1, 0, 0, 1, 1)                # lo parts, in units of 2^-11
WEXPS = (-2, 0, 4)                       # x_f8_wexp of every integer f8 case: a 2^e, b 2^e in [2^-2, 48], all e4m3 normals
WEXPS_ONEHOT = {"onehot-w8": (-2, 0, 2), "onehot-wlo8": (-2, 0, 1)}       # |A| 2^e <= 256, 128 2^e <= 256
# 64 distinct signed integers that are e4m3 numbers (4 significant bits), for the one-hot filters
_POS = list(range(1, 17)) + list(range(18, 33, 2)) + list(range(36, 65, 4))
ONEHOT_TABLE = tuple(v for p in _POS for v in (p, -p))
assert len(set(ONEHOT_TABLE)) == 64

_FIELDS = "name form epi B H W k P n pad ld choff y_ld y_choff draw lodraw wdraw tie special env expect tags"


class Case(collections.namedtuple("Case", _FIELDS)):
    """One launch of mcamd_conv_fwd.  form "wrap" / "f8"; epi "raw32" / "nchw"; P: channels per plane; n: filters.
    ld / choff: the activation slice (ld 0: the buffer is the slice).  y_ld / y_choff: the output slice of "raw32".
    draw / lodraw / wdraw: DRAWS keys of x_hi, of the second plane (x_lo; lo8 and x8) and of the wrap weights.
    tie: W1 = W0 (small3x3_split_kernel).  special: None or a one-hot kind.  expect: (kernel, bm, bn, bk) of the route.
    tags: boundary conditions the case was written for, each re-derived by boundary_tags()."""
    __slots__ = ()

    def __str__(self):
        return self.name

    @property
    def M(self):
        return self.B * self.H * self.W

    @property
    def key(self):
        return "%s-%s" % (self.form, self.epi)

    @property
    def cin(self):
        """input channels of the geometry: the K-concatenated 3 P (wrap), hi plane + byte planes in fp16 units (f8)"""
        return (3 if self.form == "wrap" else 2) * self.P

    @property
    def kb(self):
        return 64 if self.cin % 64 == 0 else 32

    @property
    def ktot(self):
        return self.k * self.k * self.cin

    @property
    def wexps(self):
        if self.form != "f8":
            return (None,)
        return WEXPS_ONEHOT[self.special] if self.special else WEXPS


def case(name, form, epi, B, H, W, k, P, n, expect, pad=0, ld=0, choff=0, y_ld=0, y_choff=0, draw="d2", lodraw="d3", wdraw="d3",
         tie=False, special=None, env=None, tags=()):
    assert "%s-%s" % (form, epi) in CASE_FORMS and (form == "wrap" or (choff == 0 and not tie))
    assert special in (None,) + tuple(WEXPS_ONEHOT) and (special is None or (form == "f8" and k == 1 and P == 128 and B * H * W == 256))
    return Case(name, form, epi, B, H, W, k, P, n, pad, ld, choff, y_ld, y_choff, draw, lodraw, wdraw, tie, special, dict(env or {}),
                tuple(expect), tuple(tags))


def geom_of(c, wexp=0):
    ld = c.ld or 2 * c.P
    if c.form == "wrap":
        return ops.geom(c.B, c.H, c.W, c.k, 3 * c.P, c.n, ld, c.choff, pad=c.pad, x_wrap=2 * c.P)
    return ops.geom(c.B, c.H, c.W, c.k, 2 * c.P, c.n, ld, 0, pad=c.pad, x_f8=c.P, x_f8_wexp=wexp)


def plain_geom_of(c):
    """the 3 P channel geometry whose plain forward packing the wrap cases' weights get"""
    return ops.geom(c.B, c.H, c.W, c.k, 3 * c.P, c.n, 3 * c.P)


def route_of(c):
    mode, stats = FORMS[c.key]
    return ops.conv_route_info(geom_of(c), ops.DIR_FWD, mode, L.DST_PLAIN, stats)


def instance_of(c, r):
    return (c.key, (r.kernel, r.bm, r.bn, r.bk))


def owned_columns(c, r):
    """statistics-slab columns the launch writes: whole column tiles (small3x3_split_kernel: its 64 computed channels)"""
    return 64 if r.kernel == SPLIT else -(-c.n // r.bn) * r.bn


def boundary_tags(c, r):
    """The named boundary conditions this launch meets, from the route query's tile and rows and the case's shape alone."""
    t = set()
    M, n = c.M, c.n
    t.add("1x1" if c.k == 1 else "3x3")
    t.add("kb32" if c.kb == 32 else "kb64")
    if c.pad:
        t.add("shared-halo")
    if c.choff > 0 and (c.ld or 2 * c.P) > c.choff + 2 * c.P:
        t.add("x_choff>0")
    if c.epi == "raw32" and c.y_choff > 0 and c.y_ld > c.y_choff + n:
        t.add("y_choff>0")
    if r.kernel == SPLIT:
        t.add("M%32!=0" if M % 32 else "M%32==0")
        t.add("n=%d" % n)
        return t
    t.add("M%bm!=0" if M % r.bm else "M%bm==0")
    if c.B > 1 and (c.H * c.W) % r.bm:
        t.add("tile-spans-images")
    if c.B > 1 and c.H * c.W < r.bm:
        t.add("HW<bm")
    if n % r.bn:
        t.add("n%bn!=0")
    if n < r.bn:
        t.add("n<bn")
    if c.epi == "nchw" and n % 8:
        t.add("n%8!=0")
    if r.kernel == IGEMM and c.kb == 64 and r.bk == 32:
        t.add("bk32-under-kb64")
    if -(-M // r.bm) > r.rows:
        t.add("persistent-walk")
    if (c.form, r.kernel, c.ktot) in (("wrap", IGEMM, 96), ("wrap", PP, 288)) or (c.form == "f8" and (c.P, c.k) == (128, 1)):
        t.add("shortest-K")                  # wrap: P = 32 (igemm), 3 P k^2 >= 256 (ping-pong); f8: 4 fp16 + 4 fp8 chunks
    if c.ktot // 32 >= 36:
        t.add("long-K")                      # f8, P = 64, k = 3: 18 + 18 chunks
    return t


# Which tags every (form, kernel family) must carry.  What cannot occur:
#   f8 / x_choff>0         the form requires x_choff == 0 (check_geom)
#   f8 / kb32              P % 64 == 0, so the channel block is always 64
#   f8, pp / bk32-under-kb64   the ping-pong kernel has one K chunk size, 32; the tag names igemm_kernel's MCAMD_BK switch
#   n%8!=0                 only the NCHW epilogue takes such n: wrap-nchw, per kernel family (BOUNDARIES_NCHW)
#   small3x3_split_kernel  one shape (P = 32, 3x3, x_choff 0, pad 0): its own list
_COMMON = ("M%bm!=0", "M%bm==0", "tile-spans-images", "HW<bm", "n%bn!=0", "n<bn", "y_choff>0", "shared-halo", "kb64", "1x1", "3x3",
           "persistent-walk", "shortest-K", "long-K")
BOUNDARIES = {("wrap", IGEMM): _COMMON + ("x_choff>0", "kb32", "bk32-under-kb64"),
              ("wrap", PP): _COMMON + ("x_choff>0", "kb32"),
              ("f8", PP): _COMMON,
              ("wrap", SPLIT): ("M%32!=0", "M%32==0", "n=40", "n=64", "y_choff>0")}
BOUNDARIES_NCHW = ("n%8!=0",)


# ---------------------------------------------------------------------------------------------------------------------
# what the route rules can name
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_ENVS = ({}, {"MCAMD_PP": "0"}, {"MCAMD_BK": "32"}, {"MCAMD_SMALL3X3": "0"}, PP2, PP2_192, PP2_N128, PP2_192_N128,
              {"MCAMD_PP": "2", "MCAMD_BK": "32", "MCAMD_SMALL3X3": "0"})
SWEEP_IMAGES = ((1, 8, 8), (2, 9, 7), (2, 13, 13), (1, 16, 16), (3, 13, 13), (4, 26, 26), (1, 64, 64), (1, 70, 61), (2, 48, 48),
                (2, 65, 64), (3, 53, 51), (4, 64, 64), (2, 91, 90), (3, 104, 112), (64, 13, 13), (32, 13, 13), (64, 26, 26),
                (64, 52, 52), (16, 104, 104), (64, 104, 104), (4, 208, 208), (64, 208, 208))
SWEEP_N = (8, 16, 24, 32, 40, 48, 56, 64, 72, 96, 120, 125, 128, 136, 192, 248, 256, 264, 512, 1024, 1056)
SWEEP_P = (32, 64, 96, 128, 160, 256, 512, 1024)


def reachable(setenv):
    """{key of FORMS: set of (kernel, bm, bn, bk)} by asking the library: SWEEP_ENVS x SWEEP_IMAGES x SWEEP_N x SWEEP_P x both
    kernel sizes x both `pad` forms, x_choff 0 and 64 for the wrap form.  "f8-raw32" holds what the launch accepts
    (mcamd_conv_fwd_f8_ok); "f8-nchw" what the route function answers for a combination the launch refuses."""
    g = ops.geom(1, 8, 8, 3, 96, 32, 64, x_wrap=64)
    out = (C.c_int32 * 5)()
    ref = C.byref(g)
    lib = L.lib()
    fn, ok8 = lib.mcamd_conv_route_info, lib.mcamd_conv_fwd_f8_ok
    seen = {key: set() for key in FORMS}
    for env in SWEEP_ENVS:
        for name, default in ENV_DEFAULTS.items():
            setenv(name, env.get(name, default))
        for (B, H, W) in SWEEP_IMAGES:
            g.B, g.H, g.W = B, H, W
            for P in SWEEP_P:
                for form in ("wrap", "f8"):
                    if form == "f8" and P % 64:
                        continue
                    for choff in ((0, 64) if form == "wrap" else (0,)):
                        g.cin = (3 if form == "wrap" else 2) * P
                        g.x_ld, g.x_choff = 2 * P + choff, choff
                        g.x_wrap, g.x_f8, g.x_f8_wexp = (2 * P, 0, 0) if form == "wrap" else (0, P, 0)
                        for n in SWEEP_N:
                            g.cout = n
                            for k in (1, 3):
                                g.ksize = k
                                for pad in (0, 1):
                                    g.pad = pad
                                    for epi in ("raw32", "nchw"):
                                        if epi == "raw32" and n % 8:
                                            continue
                                        mode, stats = FORMS["%s-%s" % (form, epi)]
                                        rc = fn(ref, ops.DIR_FWD, mode, L.DST_PLAIN, 1 if stats else 0, out)
                                        assert rc == 0, (form, epi, B, H, W, P, n, k, pad, choff)
                                        if form == "f8" and epi == "raw32" and not ok8(ref):
                                            assert out[3] != PP
                                            continue
                                        seen["%s-%s" % (form, epi)].add((out[3], out[0], out[1], out[2]))
    for name, default in ENV_DEFAULTS.items():
        setenv(name, default)
    return seen


_REACHABLE = None


def reachable_cached(setenv):
    global _REACHABLE
    if _REACHABLE is None:
        _REACHABLE = reachable(setenv)
    return _REACHABLE


# ---------------------------------------------------------------------------------------------------------------------
# operands and the exact reference (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
Operands = collections.namedtuple("Operands", "x_hi x_lo lo8 x8 w a b bias")
"""wrap: x_hi, x_lo [B][P][H][W]; w [n][3 P][k][k] = [W0 | W1 | W2].  f8: x_hi; lo8, x8 the VALUES of the byte planes; a, b
[n][P][k][k]; w = a + b 2^-11 the fp32 master for the production packer.  bias: "nchw"."""


def _gen(c):
    # (seeded by the name up to its first ".": cases "x.a", "x.b" share operands)
    return torch.Generator().manual_seed(zlib.crc32(c.name.split(".")[0].encode()))


def operands(c):
    gen = _gen(c)
    if c.special:
        return _onehot_operands(c)
    x_hi = _draw(gen, DRAWS[c.draw], (c.B, c.P, c.H, c.W))
    second = _draw(gen, DRAWS[c.lodraw], (c.B, c.P, c.H, c.W))
    if c.form == "wrap":
        w = _draw(gen, DRAWS[c.wdraw], (c.n, 3 * c.P, c.k, c.k))
        if c.tie:
            w[:, c.P:2 * c.P] = w[:, :c.P]
        bias = torch.randint(-40, 41, (c.n,), generator=gen).float() if c.epi == "nchw" else None
        return Operands(x_hi, second, None, None, w, None, None, bias)
    x8 = _draw(gen, DRAWS[c.lodraw], (c.B, c.P, c.H, c.W))
    a = _draw(gen, DRAW_A, (c.n, c.P, c.k, c.k))
    b = _draw(gen, DRAW_B, (c.n, c.P, c.k, c.k))
    b = torch.where(a != 0, b, torch.zeros_like(b))               # (+0, not -1 * 0 = -0: the packer's w - fp16(w) is +0)
    return Operands(x_hi, None, second, x8, a + b * 2.0 ** -11, a, b, None)


def _onehot_operands(c):
    P, n, M = c.P, c.n, c.M
    planes = torch.zeros(M, 2 * P)                               # the pixel's byte string [lo8 | x8]
    m = torch.arange(M)
    planes[m, ((m // 64) % 4) * 64 + m % 64] = (1 + m % 3).float()
    planes = planes.view(c.B, c.H, c.W, 2 * P).permute(0, 3, 1, 2)
    table = torch.tensor(ONEHOT_TABLE, dtype=torch.float32)
    f, ch = torch.arange(n).view(n, 1), torch.arange(P).view(1, P)
    if c.special == "onehot-w8":
        a, b = table[(ch + f) % 64], torch.zeros(n, P)
    else:
        a, b = torch.full((n, P), 128.0), table[(ch + 3 * f) % 64]
    a, b = a.view(n, P, 1, 1).contiguous(), b.view(n, P, 1, 1).contiguous()
    return Operands(torch.zeros(c.B, P, c.H, c.W), None, planes[:, :P].contiguous(), planes[:, P:].contiguous(), a + b * 2.0 ** -11, a, b,
                    None)


def e4m3_codes(v):
    """integer-valued tensor -> its e4m3 bytes (torch.float8_e4m3fn)"""
    return v.to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_values(codes):
    return codes.view(torch.float8_e4m3fn).double()


Reference = collections.namedtuple("Reference", "y s1 s2")
_BIG = {}


def _conv(c, x, w, dt=torch.float64):
    return F.conv2d(x.to(dt), w.to(dt), None, 1, (c.k - 1) // 2).double()


def reference(c, o, dt=None):
    """y [B][n][H][W] float64 (float32 convolutions, exact under condition 1, for the one big case); s1, s2: per-channel sums of
    y and y^2 ("raw32")."""
    big = c.M * c.n * c.ktot > 4e9
    dt = dt or (torch.float32 if big else torch.float64)
    P = c.P
    if c.form == "wrap":
        key = (c.name.split(".")[0], c.B, c.H, c.W, c.k, c.P, c.n, c.draw, c.lodraw, c.wdraw, c.tie)
        if big and key in _BIG:
            y = _BIG[key]                            # the big cases share their operands: one convolution
        else:
            y = _conv(c, o.x_hi, o.w[:, :P], dt) + _conv(c, o.x_lo, o.w[:, P:2 * P], dt) + _conv(c, o.x_hi, o.w[:, 2 * P:], dt)
            if big:
                _BIG.clear()
                _BIG[key] = y
        if c.epi == "nchw":
            y = y + o.bias.double().view(1, -1, 1, 1)
    else:
        y = _conv(c, o.x_hi, o.a, dt) + UNIT_F8 * (_conv(c, o.lo8, o.a, dt) + _conv(c, o.x8, o.b, dt))
    if c.epi == "raw32":
        return Reference(y, y.sum((0, 2, 3)), (y * y).sum((0, 2, 3)))
    return Reference(y, None, None)


def stats_bounds(c, ref):
    """f8, condition 3: (bound on |s1 - sum y|, bound on |s2 - sum y^2|) per channel"""
    n = c.M
    gamma = n * 2.0 ** -24 / (1.0 - n * 2.0 ** -24)
    return gamma * ref.y.abs().sum((0, 2, 3)), gamma * ref.s2


def exactness(c, o, ref):
    """Violations of the conditions in the module docstring (empty: all met), from the operands and the reference alone."""
    bad = []
    mx = lambda t: float(t.abs().max())
    if c.form == "wrap":
        bound = max(mx(o.x_hi), mx(o.x_lo)) * mx(o.w) * c.ktot + (mx(o.bias) if o.bias is not None else 0.0)
        if not bound < 2 ** 24:
            bad.append("condition 1: bound %r" % bound)
        for t in (o.x_hi, o.x_lo, o.w):
            if not torch.equal(t.half().float(), t):
                bad.append("an operand is no fp16 number")
        if ref.s2 is not None and not float(ref.s2.max()) < 2 ** 24:
            bad.append("condition 2: sum of y^2 over all pixels %r" % float(ref.s2.max()))
    else:
        kk = c.k * c.k * c.P
        bound = kk * (mx(o.x_hi) * mx(o.a) / UNIT_F8 + mx(o.lo8) * mx(o.a) + mx(o.x8) * mx(o.b))
        if not bound < 2 ** 24:
            bad.append("condition 1: bound %r units of 2^-12" % bound)
        if not max(mx(o.lo8) * mx(o.a), mx(o.x8) * mx(o.b)) <= F8_PRODUCT_RANGE:
            bad.append("condition 4: product range %r" % max(mx(o.lo8) * mx(o.a), mx(o.x8) * mx(o.b)))
        for t in (o.x_hi, o.a, o.b, o.lo8, o.x8):
            if not torch.equal(t, t.round()):
                bad.append("an operand is no integer")
        if not torch.equal(o.w.half().float(), o.a) or not torch.equal((o.w - o.a) * 2.0 ** 11, o.b):
            bad.append("fp16(w) != a or w - a != b 2^-11")
        for e in c.wexps:
            for t in (o.a * 2.0 ** e, o.b * 2.0 ** e):
                if not torch.equal(e4m3_values(e4m3_codes(t)), t.double()) or float(t.abs().max()) > 448.0:
                    bad.append("a 2^%d or b 2^%d is no e4m3 number" % (e, e))
        for t in (o.lo8, o.x8):
            if not torch.equal(e4m3_values(e4m3_codes(t)), t.double()):
                bad.append("a byte plane does not decode to the intended integers")
        if not torch.equal(ref.y / UNIT_F8, (ref.y / UNIT_F8).round()):
            bad.append("the reference is no multiple of 2^-12")
    if not torch.equal(ref.y.float().double(), ref.y):
        bad.append("the reference is no fp32 number")
    return bad


def count_unequal(got, want):
    """THE comparison of the GPU test: elements of `got` that do not EQUAL `want` (NaN compares unequal)."""
    return int((~(got.double() == want.double())).sum())


def stats_violations(c, got1, got2, ref):
    """The statistics check of the GPU test: float64 sums of the slab rows against the reference -- equal (wrap), within
    stats_bounds (f8).  Returns the number of channels that miss."""
    if c.form == "wrap":
        return count_unequal(got1, ref.s1) + count_unequal(got2, ref.s2)
    b1, b2 = stats_bounds(c, ref)
    return int((~((got1.double() - ref.s1).abs() <= b1)).sum()) + int((~((got2.double() - ref.s2).abs() <= b2)).sum())


# ---- the packed-weight layouts as include/mcamd.h states them (CPU)
def kpos(t, ch, taps, chp):
    """position of (tap t, channel ch) in a packed row of `taps` x `chp` channels: [channel block][tap][channel in block]"""
    kb = 64 if chp % 64 == 0 else 32
    return (ch // kb) * taps * kb + t * kb + ch % kb


def f8_packing(a, b, wexp):
    """mcamd_pack_job.split = 2 of w = a + b 2^-11: [Npad][k*k * 2 P] fp16 units as int16 bit patterns -- per tap [w_hi: P fp16 |
    w8: P e4m3 bytes | wlo8: P bytes], e4m3 element e of the tap's byte string in byte (e & 1) of fp16 unit P + e / 2, the
    units in kpos order over 2 P channels; pad rows zero."""
    n, P, k, _ = a.shape
    kk = k * k
    units = torch.zeros(n, kk, 2 * P, dtype=torch.int16)
    units[:, :, :P] = a.reshape(n, P, kk).permute(0, 2, 1).half().view(torch.int16)
    bytes_ = torch.cat([e4m3_codes(a * 2.0 ** wexp), e4m3_codes(b * 2.0 ** wexp)], 1).reshape(n, 2 * P, kk).permute(0, 2, 1)
    units[:, :, P:] = torch.empty(n, kk, 2 * P, dtype=torch.uint8).copy_(bytes_).view(torch.int16)                     # little endian: element e -> byte e & 1 of unit e / 2
    ch = torch.arange(2 * P)
    rows = torch.zeros(ops.round_up(n, 256), kk * 2 * P, dtype=torch.int16)
    for t in range(kk):
        rows[:n, kpos(t, ch, kk, 2 * P)] = units[:, t]
    return rows


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
W32, WNCHW, F32 = ("wrap", "raw32"), ("wrap", "nchw"), ("f8", "raw32")
PP0 = {"MCAMD_PP": "0"}
BK32 = {"MCAMD_BK": "32"}

E = (IGEMM, 128, 32, 32)
SPLIT_CASES = [
    # ---- igemm_kernel<128, 32, .., 32, 3>
    case("w-i128x32k32-raw32", *W32, 3, 9, 7, 1, 32, 32, E, ld=128, choff=32,
         tags=("M%bm!=0", "tile-spans-images", "HW<bm", "x_choff>0", "shortest-K", "kb32", "1x1")),
    case("w-i128x32k32-raw32-3x3", *W32, 1, 16, 16, 3, 96, 24, E, pad=1, y_ld=40, y_choff=8, draw="d1", lodraw="d1", wdraw="d1",
         tags=("M%bm==0", "n<bn", "y_choff>0", "shared-halo", "long-K", "3x3")),
    case("w-i128x32k32-raw32-bk32-under-kb64", *W32, 2, 13, 13, 3, 64, 32, E, env=BK32, draw="d1", tags=("bk32-under-kb64", "kb64")),
    case("w-i128x32k32-raw32-33-columns-of-tiles", *W32, 3, 53, 51, 1, 32, 1056, E, draw="d1", lodraw="d2", wdraw="d2",
         tags=("persistent-walk",)),
    case("w-i128x32k32-nchw", *WNCHW, 3, 9, 7, 3, 32, 29, E, pad=1, tags=("n%8!=0", "n<bn", "shared-halo")),
]

E = (IGEMM, 128, 32, 64)
SPLIT_CASES += [
    # ---- igemm_kernel<128, 32, .., 64, 2>
    case("w-i128x32k64-raw32", *W32, 3, 13, 13, 3, 64, 96, E, draw="d1", tags=("kb64", "3x3", "tile-spans-images")),
    case("w-i128x32k64-raw32-1x1", *W32, 2, 8, 8, 1, 128, 24, E, ld=320, choff=32, tags=("M%bm==0", "HW<bm", "n<bn", "x_choff>0")),
    case("w-i128x32k64-nchw", *WNCHW, 2, 13, 13, 1, 64, 93, E, tags=("n%8!=0", "n%bn!=0")),
]

E = (IGEMM, 128, 64, 32)
SPLIT_CASES += [
    # ---- igemm_kernel<128, 64, .., 32, 3>
    case("w-i128x64k32-raw32", *W32, 2, 13, 13, 3, 32, 64, E, y_ld=96, y_choff=24, tags=("y_choff>0", "kb32")),
    case("w-i128x64k32-raw32-n120", *W32, 2, 13, 13, 1, 96, 120, E, tags=("n%bn!=0",)),
    case("w-i128x64k32-nchw", *WNCHW, 2, 13, 13, 1, 96, 125, E, tags=("n%8!=0",)),          # the logit layer's filter count
]

E = (IGEMM, 128, 64, 64)
SPLIT_CASES += [
    # ---- igemm_kernel<128, 64, .., 64, 2>: also the few-tile rule at 128 columns
    case("w-i128x64k64-raw32", *W32, 3, 13, 13, 1, 64, 128, E, tags=("1x1", "kb64")),
    case("w-i128x64k64-raw32-n40", *W32, 2, 13, 13, 3, 128, 40, E, pad=1, draw="d1", lodraw="d1", wdraw="d1",
         tags=("n<bn", "shared-halo", "long-K")),
    case("w-i128x64k64-nchw", *WNCHW, 2, 13, 13, 3, 64, 125, E, pad=1, draw="d1", tags=("n%8!=0", "shared-halo")),
]

E = (IGEMM, 128, 128, 32)
SPLIT_CASES += [
    # ---- igemm_kernel<128, 128, .., 32, 3>: 256 tiles of 128 x 128 or more
    case("w-i128x128k32-raw32", *W32, 4, 64, 64, 1, 32, 256, E, draw="d1", lodraw="d1", wdraw="d2", tags=("M%bm==0",)),
    case("w-i128x128k32-raw32-ragged", *W32, 2, 91, 90, 1, 96, 248, E, draw="d1", lodraw="d1", wdraw="d1", tags=("M%bm!=0", "n%bn!=0")),
    case("w-i128x128k32-nchw", *WNCHW, 2, 91, 90, 1, 32, 253, E, draw="d1", tags=("n%8!=0",)),
]

E = (IGEMM, 128, 128, 64)
SPLIT_CASES += [
    # ---- igemm_kernel<128, 128, .., 64, 2>
    case("w-i128x128k64-raw32", *W32, 4, 64, 64, 1, 64, 256, E, ld=192, choff=32, draw="d1", lodraw="d1", wdraw="d1", tags=("x_choff>0",)),
    case("w-i128x128k64-nchw", *WNCHW, 2, 91, 90, 1, 64, 250, E, draw="d1", tags=("n%8!=0",)),
]

E = (IGEMM, 192, 128, 64)
SPLIT_CASES += [
    # ---- igemm_kernel<192, 128, 96, 64, 64, 2>: K >= 2048 and more than 512 tiles of 128 rows -- the one heavy case
    # (the two share their operands and one convolution on the CPU)
    case("w-i192x128k64.raw32", *W32, 2, 65, 64, 3, 128, 1024, E, env=PP0, draw="s4", lodraw="s4", wdraw="s4u", tags=("M%bm!=0", "long-K")),
    case("w-i192x128k64.nchw", *WNCHW, 2, 65, 64, 3, 128, 1024, E, env=PP0, draw="s4", lodraw="s4", wdraw="s4u"),
]

E = (PP, 256, 256, 32)
SPLIT_CASES += [
    # ---- igemm_pp_kernel (MCAMD_PP=2: whenever legal), 256 x 256
    case("w-pp256x256-raw32", *W32, 1, 16, 16, 1, 96, 256, E, env=PP2, tags=("M%bm==0", "shortest-K", "kb32", "1x1")),
    case("w-pp256x256-raw32-3x3", *W32, 2, 13, 13, 3, 32, 136, E, env=PP2, pad=1, y_ld=160, y_choff=8,
         tags=("M%bm!=0", "tile-spans-images", "HW<bm", "n<bn", "y_choff>0", "shared-halo", "3x3")),
    case("w-pp256x256-nchw", *WNCHW, 2, 13, 13, 1, 128, 253, E, env=PP2, tags=("n%8!=0",)),
]

E = (PP, 192, 256, 32)
SPLIT_CASES += [
    # ---- 192 x 256
    case("w-pp192x256-raw32", *W32, 2, 16, 12, 3, 64, 264, E, env=PP2_192, ld=192, choff=32, draw="d1",
         tags=("M%bm==0", "n%bn!=0", "x_choff>0", "kb64", "long-K")),
    case("w-pp192x256-nchw", *WNCHW, 3, 13, 13, 1, 96, 131, E, env=PP2_192, pad=1, tags=("n%8!=0", "n<bn")),
]

E = (PP, 256, 128, 32)
SPLIT_CASES += [
    # ---- 256 x 128
    case("w-pp256x128-raw32", *W32, 3, 13, 13, 1, 128, 136, E, env=PP2_N128, tags=("n%bn!=0", "kb64")),
    case("w-pp256x128-nchw", *WNCHW, 2, 13, 13, 3, 32, 253, E, env=PP2_N128, tags=("n%8!=0",)),
]

E = (PP, 192, 128, 32)
SPLIT_CASES += [
    # ---- 192 x 128
    case("w-pp192x128-raw32", *W32, 2, 13, 13, 3, 96, 128, E, env=PP2_192_N128, pad=1, draw="d1", lodraw="d1", wdraw="d1",
         tags=("shared-halo", "long-K")),
    case("w-pp192x128-raw32-8-columns-of-tiles", *W32, 3, 46, 45, 1, 96, 1024, E, env=PP2_192_N128, draw="d1", lodraw="d1", wdraw="d2",
         tags=("persistent-walk", "M%bm!=0")),
    case("w-pp192x128-nchw", *WNCHW, 2, 13, 13, 1, 128, 135, E, env=PP2_192_N128, tags=("n%8!=0",)),
]

E = (SPLIT, 32, 64, 96)
SPLIT_CASES += [
    # ---- small3x3_split_kernel<4>: P = 32, 3x3, 32 < n <= 64, M >= 4096, x_choff 0, pad 0; W1 = W0 (module docstring)
    case("w-small-split-n64", *W32, 1, 70, 61, 3, 32, 64, E, tie=True, draw="d1", lodraw="d2", wdraw="d2", tags=("M%32!=0", "n=64")),
    case("w-small-split-n40", *W32, 1, 70, 61, 3, 32, 40, E, tie=True, y_ld=48, y_choff=4, draw="d1", lodraw="d2", wdraw="d2",
         tags=("M%32!=0", "n=40", "y_choff>0")),
    case("w-small-split-2-images", *W32, 2, 48, 48, 3, 32, 48, E, tie=True, draw="d1", lodraw="d2", wdraw="d2", tags=("M%32==0",)),
]

E = (PP, 256, 256, 32)
SPLIT_CASES += [
    # ---- igemm_pp_kernel<RAW_F32, BM, BN, 32, F8 = true>, 256 x 256
    case("f8-pp256x256", *F32, 1, 16, 16, 1, 128, 256, E, env=PP2, tags=("M%bm==0", "shortest-K", "1x1")),
    case("f8-pp256x256-3x3", *F32, 2, 13, 13, 3, 64, 136, E, env=PP2, pad=1, y_ld=160, y_choff=8,
         tags=("M%bm!=0", "tile-spans-images", "HW<bm", "n<bn", "y_choff>0", "shared-halo", "long-K", "3x3")),
]

E = (PP, 192, 256, 32)
SPLIT_CASES += [
    case("f8-pp192x256", *F32, 2, 16, 12, 3, 64, 264, E, env=PP2_192, ld=160, tags=("M%bm==0", "n%bn!=0", "long-K")),
    case("f8-pp192x256-1x1", *F32, 3, 13, 13, 1, 256, 128, E, env=PP2_192, pad=1, tags=("n<bn", "HW<bm")),
]

E = (PP, 256, 128, 32)
SPLIT_CASES += [
    case("f8-pp256x128", *F32, 3, 13, 13, 1, 128, 136, E, env=PP2_N128, y_ld=144, y_choff=4, tags=("n%bn!=0", "shortest-K", "y_choff>0")),
    case("f8-pp256x128-3x3", *F32, 1, 16, 16, 3, 64, 128, E, env=PP2_N128, tags=("M%bm==0", "long-K")),
]

E = (PP, 192, 128, 32)
SPLIT_CASES += [
    case("f8-pp192x128", *F32, 2, 13, 13, 3, 128, 128, E, env=PP2_192_N128, draw="d1", tags=("long-K", "tile-spans-images")),
    case("f8-pp192x128-8-columns-of-tiles", *F32, 3, 46, 45, 1, 128, 1024, E, env=PP2_192_N128, draw="d1",
         tags=("persistent-walk", "M%bm!=0", "shortest-K")),
]

# the byte-to-k map of the 64-k instruction and the packer's byte placement, in every F8 tile
for _name, _bm, _bn, _env in (("pp256x256", 256, 256, PP2), ("pp192x256", 192, 256, PP2_192), ("pp256x128", 256, 128, PP2_N128),
                              ("pp192x128", 192, 128, PP2_192_N128)):
    for _kind in ("onehot-w8", "onehot-wlo8"):
        SPLIT_CASES.append(case("f8-%s-%s" % (_name, _kind), *F32, 1, 16, 16, 1, 128, 128, (PP, _bm, _bn, 32), env=_env, special=_kind))


def one_case_per_instance(form, kernels):
    """the cheapest table case of every (form, epilogue, kernel instance) whose kernel is in `kernels`"""
    best = {}
    for c in SPLIT_CASES:
        if c.form == form and c.expect[0] in kernels and not c.special:
            key = (c.key, c.expect)
            if key not in best or c.M * c.n * c.ktot < best[key].M * best[key].n * best[key].ktot:
                best[key] = c
    return [best[key] for key in sorted(best)]
