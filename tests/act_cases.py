"""The case table of the exact bn_act_fwd_kernel tests, and operands whose result does not depend on the kernel's
arithmetic order.

bn_act.hip is compiled with FMA contraction allowed, so `y * scale + shift` must be the same number fused and unfused:
  - y and the border entries are multiples of 2^-12 (fp16 y: of 2^-4) below 128 in magnitude, their sum below 256: at most
    20 significant bits;
  - scales are +-{1, 1.25, 1.5, 1.75} * 2^j, j in [-3, 2]: 3 significant bits, so the product has at most 23 and is EXACT in
    fp32 -- fused or not, the sum with the shift is rounded once;
  - shifts are arbitrary fp32; the slope is 0.1, 0.125 or 1.
`exactness` asserts these conditions, and what follows from them, on the operands themselves (never from kernel output).

Channels 0-7 (and 8, 9 where C >= 16) of every case carry planted coefficients, so that every case whose storage form can show
an edge does: |v| > 65504 (hi clamps, lo is the rest), |2 v| > 448 (codes 0x7E / 0xFE, never a NaN code), an fp16-subnormal v,
z = +0 and z = -0, negative scales, and -- for the strict-maximum copy `pool_act` -- windows whose two largest values round to
one fp16 value with the later one larger, exact fp32 ties, four values of one fp16 value, and all-negative windows.
"""
import collections

import torch

import act_ref as R

PLAIN, POOL, REORG = R.PLAIN, R.POOL, R.REORG
MODE_NAME = {PLAIN: "plain", POOL: "pool", REORG: "reorg"}
SLOPES = (0.1, 0.125, 1.0)
# storage form -> (fp32 y, planes, byte twins)
FORMS = {"h1": (False, 1, False), "h2": (False, 2, False), "h3": (False, 3, False),
         "f1": (True, 1, False), "f2": (True, 2, False), "f3": (True, 3, False), "f4": (True, 4, False), "q8": (True, 1, True)}
FIXED_C, RAGGED_C = (8, 64, 256, 2048), (24, 200, 2056)

Case = collections.namedtuple("Case", "name mode B H W C y32 planes planes2 q8 twin twin2 dst2 y_ld y_choff dst_ld dst_choff "
                                      "dst_plane dst_pad dst2_ld dst2_choff dst2_plane dst2_pad border slope pool_act "
                                      "pool_act_ld pool_act_pad seed big")
Operands = collections.namedtuple("Operands", "y scale shift slope border")   # y: float64 NCHW; scale, shift: fp32; border fp32 [16][C]


def _ld(choff, span, planes, plane, tail):
    need = span if planes == 1 else (2 * plane if planes == 4 else (planes - 1) * plane + span)
    return choff + need + tail


def make(name, mode, C, form, B=2, H=None, W=None, dst2=False, planes2=0, choff=8, gap=8, pad=0, choff2=16, gap2=16, pad2=1,
         tail=8, y_choff=8, y_extra=8, border=False, slope=0.1, pool_act=None, twin=True, twin2=False, seed=0, big=False):
    """gap: dst_plane - span (planes >= 2).  pool_act: None or (pool_act_ld - C, pool_act_pad).  twin / twin2: which of the
    destinations of a "q8" case have a byte twin."""
    y32, planes, q8 = FORMS[form]
    if H is None:
        H, W = (2, 4) if C >= 2048 else ((4, 6) if C >= 200 else (6, 10))
    span = 4 * C if mode == REORG else C
    p2 = (planes2 or planes) if dst2 else planes
    plane = span + gap if planes >= 2 else 0
    plane2 = C + gap2 if (dst2 and p2 >= 2) else 0
    assert planes != 4 or gap >= choff, "form 4: the hi slice and its e4m3 strings must stay inside one plane stride"
    assert not (dst2 and p2 == 4) or gap2 >= choff2
    twin, twin2 = q8 and twin, q8 and dst2 and twin2
    return Case(name, mode, B, H, W, C, y32, planes, p2, twin or twin2, twin, twin2, dst2,
                C + y_choff + y_extra, y_choff, _ld(choff, span, planes, plane, tail), choff, plane, pad,
                _ld(choff2, C, p2, plane2, tail) if dst2 else 0, choff2 if dst2 else 0, plane2, pad2 if dst2 else 0,
                border, slope, pool_act is not None, C + pool_act[0] if pool_act else 0, pool_act[1] if pool_act else 0,
                seed, big)


def _table():
    t = []
    n = 0
    # every instance: mode x FIXED / !FIXED x storage form, channel counts, pads, offsets and slopes rotating
    for mode in (PLAIN, POOL, REORG):
        for form in FORMS:
            for fixed in (True, False):
                Cs = FIXED_C if fixed else RAGGED_C
                C = Cs[n % len(Cs)]
                if C == 2056:
                    shape = dict(B=1, H=2, W=2)
                elif mode == REORG and C >= 2048:
                    shape = dict(B=2, H=2, W=4)
                else:
                    shape = {}
                dst2 = mode != PLAIN and (n // 2 + n) % 2 == 0
                pa = (8 * (n % 3), (n // 2) % 2) if (mode == POOL and not FORMS[form][2] and C >= 16 and C < 2048) else None
                if pa is not None:
                    shape = dict(B=2, H=4, W=6) if C >= 200 else dict(B=2, H=6, W=10)
                t.append(make("%s-%s-c%d" % (MODE_NAME[mode], form, C), mode, C, form, dst2=dst2, choff=8 + 8 * (n % 3),
                              gap=24 + 8 * (n % 2), pad=(n // 2 + n // 16) % 2, choff2=8 + 8 * ((n + 1) % 3), gap2=24, pad2=(n // 4 + n) % 2,
                              border=n % 5 == 0, slope=SLOPES[n % 3], pool_act=pa, twin=True, twin2=dst2, seed=100 + n, **shape))
                n += 1
    # the remaining FIXED / !FIXED channel counts in plain fp32 form, so each occurs in every mode
    for mode in (PLAIN, POOL, REORG):
        for C in FIXED_C + RAGGED_C:
            shape = dict(B=1, H=2, W=2) if C == 2056 else {}
            t.append(make("%s-f2-c%d-all" % (MODE_NAME[mode], C), mode, C, "f2", dst2=mode == POOL, pad=(C // 8) % 2, seed=200 + C + mode,
                          slope=SLOPES[(C // 8 + mode) % 3], **shape))
    # POOL with dst2 in another storage form than dst: the wave-uniform switch of store_act2
    for pl in (2, 3, 4):
        for pl2 in (2, 3, 4):
            t.append(make("pool-f%d-dst2-f%d" % (pl, pl2), POOL, 64, "f%d" % pl, dst2=True, planes2=pl2, pad=pl % 2, pad2=pl2 % 2,
                          pool_act=(8, (pl + pl2) % 2), seed=300 + 10 * pl + pl2, slope=SLOPES[(pl + pl2) % 3]))
    t.append(make("reorg-f4-dst2-f2", REORG, 24, "f4", dst2=True, planes2=2, seed=340))
    t.append(make("pool-h2-dst2-h3", POOL, 64, "h2", dst2=True, planes2=3, pool_act=(0, 1), seed=341))
    t.append(make("pool-h3-dst2-h2", POOL, 24, "h3", dst2=True, planes2=2, pool_act=(16, 0), seed=342))
    # form 4 as the second member of a two-way route: dst_choff = ca, dst_plane = ca + cb
    for mode in (PLAIN, POOL, REORG):
        ca = 64
        t.append(make("%s-f4-route-member" % MODE_NAME[mode], mode, 64 if mode != REORG else 16, "f4", choff=ca, gap=ca,
                      dst2=mode == POOL, choff2=32, gap2=32, pad=1, pad2=0, seed=400 + mode, border=mode == REORG))
    # the border table: all 16 classes need H == 1 and W == 1
    t.append(make("plain-f4-border-h1", PLAIN, 24, "f4", H=1, W=5, border=True, seed=500, slope=0.125))
    t.append(make("plain-h2-border-w1", PLAIN, 64, "h2", H=5, W=1, border=True, pad=1, seed=501))
    t.append(make("plain-q8-border-1x1", PLAIN, 8, "q8", H=1, W=1, border=True, seed=502, slope=1.0))
    t.append(make("plain-f3-border", PLAIN, 200, "f3", H=4, W=6, border=True, seed=503))
    t.append(make("pool-f4-border", POOL, 64, "f4", dst2=True, planes2=3, border=True, pool_act=(8, 1), seed=504))
    t.append(make("reorg-h1-border", REORG, 24, "h1", border=True, pad=1, seed=505))
    # byte twins: dst only, dst2 only, both, and none beside a twin
    for mode in (POOL, REORG):
        for k, (tw, tw2) in enumerate(((True, False), (False, True), (True, True))):
            t.append(make("%s-q8-twins-%d%d" % (MODE_NAME[mode], tw, tw2), mode, 64 if mode == POOL else 24, "q8", dst2=True, twin=tw,
                          twin2=tw2, pad=k % 2, pad2=(k + 1) % 2, seed=600 + 10 * mode + k, slope=SLOPES[k]))
    t.append(make("pool-q8-twin-no-dst2", POOL, 200, "q8", H=4, W=6, seed=640))
    # more than one item per thread: items > 4096 * 256
    t.append(make("plain-f1-c2048-gridstride", PLAIN, 2048, "f1", B=1, H=66, W=64, choff=0, tail=0, y_choff=0, y_extra=0, seed=700,
                  big=True))
    t.append(make("plain-f1-c200-gridstride", PLAIN, 200, "f1", B=2, H=146, W=144, choff=0, tail=0, y_choff=0, y_extra=0, seed=701,
                  big=True))
    names = [c.name for c in t]
    assert len(set(names)) == len(names), [x for x in names if names.count(x) > 1]
    return t


CASES = _table()
SMALL = [c for c in CASES if not c.big]
BIG = [c for c in CASES if c.big]
# cases that run the same operands through the storage forms 1 to 4 (hi must be identical)
SAME_OPERANDS = [make("pool-f%d-same-operands" % pl, POOL, 64, "f%d" % pl, dst2=True, seed=800) for pl in (1, 2, 3, 4)]


def instance(c):
    """(mode, fixed, y32, planes, q8): the bn_act_fwd_kernel<MODE, FIXED, Y32, PL, Q8> instance the case was written for"""
    ch = c.C // 8
    return (c.mode, ch <= 256 and 256 % ch == 0, c.y32, c.planes, c.q8)


def all_instances():
    return {(m, fx) + ((y32, pl, q8)) for m in (PLAIN, POOL, REORG) for fx in (True, False) for (y32, pl, q8) in FORMS.values()}


# ---------------------------------------------------------------------------------------------------------- operands
# planted windows of pool_act (image 0, channels 8 and 9, units of the y grid step g); (ho, wo) -> the four y in scan order
def _windows(g):
    return {(0, 0): (8, [4.0, 1.0, 4.0 + g, 0.5]),            # the two largest round to one fp16 value, the later one larger
            (0, 1): (8, [5.25, 5.25, 1.0, 5.25]),             # exact ties: the first one is the maximum
            (1, 0): (8, [8 + g, 8 + 3 * g, 8 + 2 * g, 8.0]),   # four values of one fp16 value
            (1, 1): (9, [3.0, 3.0 - g, 3.0 + g, 3.0])}        # an all-negative window of one fp16 value


def planted(c):
    return c.pool_act and c.C >= 16 and c.H >= 4 and c.W >= 4


def operands(c):
    gen = torch.Generator().manual_seed(c.seed)
    g = 2.0 ** -12 if c.y32 else 2.0 ** -4
    n = int(128 / g)
    y = torch.randint(-n + 1, n, (c.B, c.C, c.H, c.W), generator=gen).double() * g
    mant = 1.0 + 0.25 * torch.randint(0, 4, (c.C,), generator=gen).double()
    sign = torch.where(torch.randint(0, 4, (c.C,), generator=gen) == 0, -1.0, 1.0).double()
    scale = (sign * mant * 2.0 ** torch.randint(-3, 3, (c.C,), generator=gen).double()).float()
    shift = (torch.randn(c.C, generator=gen) * 2).float()
    border = None
    if c.border:
        border = (torch.randint(-n + 1, n, (16, c.C), generator=gen).double() * g).float()
        border[:, 5:10] = (border[:, 5:10] / (2 * g)).trunc() * g          # the planted channels: |y| stays below 128
    for ch, (sc, sh) in enumerate(((1.0, 70000.0), (-1.25, 70000.0), (1.0, -70000.0), (1.0, 300.0), (1.5, -300.0),
                                   (0.125, 2.0 ** -15), (-1.5, -0.0), (1.75, 0.0), (1.0, 1024.0), (1.0, -1024.0))):
        if ch < c.C and (ch < 8 or c.C >= 16):
            scale[ch], shift[ch] = sc, sh
    cls = R.border_class(c.H, c.W)

    def put(b, ch, h, w, val):                 # so that y + border == val
        y[b, ch, h, w] = val - (float(border[int(cls[h, w]), ch]) if border is not None else 0.0)
    for ch in (5, 6, 7):                       # fp16-subnormal v = 2^-15, z = -0, z = +0
        put(0, ch, 0, 0, 0.0)
    if planted(c):
        for (ho, wo), (ch, vals) in _windows(g).items():
            for k, val in enumerate(vals):
                put(0, ch, 2 * ho + (k >> 1), 2 * wo + (k & 1), val)
    return Operands(y, scale, shift, c.slope, border)


def exactness(c, op):
    """The grid conditions, on the operands alone."""
    g = 2.0 ** -12 if c.y32 else 2.0 ** -4
    y = op.y
    assert bool((y / g == (y / g).round()).all()) and float(y.abs().max()) < 128
    assert torch.equal(y, (y.float() if c.y32 else y.half()).double()), "y is not exact in its storage type"
    ysum = y
    if op.border is not None:
        b = op.border.double()
        assert bool((b * 4096 == (b * 4096).round()).all()) and float(b.abs().max()) < 128
        ysum = y + b[R.border_class(c.H, c.W)].permute(2, 0, 1).unsqueeze(0)
        assert float(ysum.abs().max()) < 256 and torch.equal(ysum, R.fl32(ysum))
    m, e = torch.frexp(op.scale.double().abs())                          # |scale| = m 2^e, m in [0.5, 1)
    assert bool(((m * 8 == (m * 8).round()) & (m * 8 >= 4) & (e - 1 >= -3) & (e - 1 <= 2)).all()), "scale off the grid"
    assert any(op.slope == s for s in SLOPES)
    sc, sh = op.scale.double().view(1, -1, 1, 1), op.shift.double().view(1, -1, 1, 1)
    p = ysum * sc
    assert torch.equal(p, R.fl32(p)), "y * scale is not exact in fp32"
    s = p + sh
    bb = s - p
    assert bool((((p - (s - bb)) + (sh - bb)) == 0).all()), "the float64 sum is not exact"           # two-sum error term
    z = R.fl32(s)
    assert torch.equal((ysum.float() * op.scale.view(1, -1, 1, 1) + op.shift.view(1, -1, 1, 1)).double(), z), "fp32 multiply-then-add"
    s32 = torch.tensor(op.slope, dtype=torch.float32)
    assert torch.equal((z.float() * s32).double(), R.fl32(z * s32.double())), "slope product"
    tiny = 2.0 ** -126
    v = R.activation(c, op)
    assert bool(((v == 0) | (v.abs() >= tiny)).all()), "an fp32-subnormal activation"
    d = v - R.hi16(v).double()
    assert torch.equal(d, R.fl32(d)), "v - hi is not exact in fp32"
    if c.mode == POOL:
        w = R.window(v)
        zero_max = w.amax(0) == 0
        neg0 = ((w == 0) & torch.signbit(w)).any(0)
        pos0 = ((w == 0) & ~torch.signbit(w)).any(0)
        assert not bool((zero_max & neg0 & pos0).any()), "a pooled maximum is a tie between +0 and -0"
    return v
