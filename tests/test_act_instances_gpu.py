"""Every bn_act_fwd_kernel<MODE, FIXED, Y32, PL, Q8> instance mcamd_bn_act_fwd can launch, element by element and with no
tolerance, against the float64 restatement in act_ref.py on the case table of act_cases.py; and bn_coeffs_kernel against a
float64 restatement of nn.BatchNorm2d's statistics (reference src/nets.py:802) to one fp32 ulp.

One launch per case into buffers that hold the sentinel 0x7F7F (an fp16 NaN whose two bytes are the e4m3 NaN code, which no
store produces) everywhere: guard bands, halo pixels, the channels beside the slice, the gaps between planes, the bytes of the
e4m3 strings outside the slice.  The whole buffer must then equal the expected image: every written element bit for bit, every
other one still the sentinel.  The operands make the result independent of the kernel's arithmetic order (act_cases.exactness),
so no comparison here has a tolerance."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops  # noqa: E402
from util import whole  # noqa: E402
import act_cases as A  # noqa: E402
import act_ref as R  # noqa: E402
import q8_ref as Q  # noqa: E402
from test_act_instances_cpu import case_args, query  # noqa: E402


def _sentinel16(buf):
    whole(buf).view(torch.int16).fill_(R.SENT16)
    return buf


def _got16(buf, img, what):
    """device fp16 buffer -> [pixels][ld] bit patterns (int32, cpu); everything outside the image must hold the sentinel"""
    all_ = whole(buf).view(torch.int16).cpu().to(torch.int32) & 0xFFFF
    lo, n = buf.storage_offset(), img.want.numel()
    assert bool((all_[:lo] == R.SENT16).all()) and bool((all_[lo + n:] == R.SENT16).all()), "%s: a store outside the buffer" % what
    return all_[lo:lo + n].view(-1, img.ld)


def run(dev, c, op=None):
    """One launch of the case -> ({destination: [pixels][ld] as stored}, expected images, v)"""
    op = op or A.operands(c)
    A.exactness(c, op)
    want = R.expected(c, op)
    Hd, Wd = (c.H, c.W) if c.mode == A.PLAIN else (c.H // 2, c.W // 2)
    ydt = torch.float32 if c.y32 else torch.float16
    y = torch.full((c.B * c.H * c.W, c.y_ld), float("nan"), dtype=ydt, device=dev)
    y[:, c.y_choff:c.y_choff + c.C] = op.y.permute(0, 2, 3, 1).reshape(-1, c.C).to(ydt).to(dev)
    bufs = {"dst": _sentinel16(ops.alloc_padded(c.B, Hd, Wd, c.dst_ld, dev, pad=c.dst_pad))}
    if c.dst2:
        bufs["dst2"] = _sentinel16(ops.alloc_padded(c.B, c.H, c.W, c.dst2_ld, dev, pad=c.dst2_pad))
    if c.pool_act:
        bufs["pool_act"] = _sentinel16(ops.alloc_padded(c.B, c.H, c.W, c.pool_act_ld, dev, pad=c.pool_act_pad))
    if c.twin:
        bufs["dst_q8"] = ops.alloc_padded_q8(c.B, Hd, Wd, c.dst_ld, dev, pad=c.dst_pad).fill_(R.SENT8)
    if c.twin2:
        bufs["dst2_q8"] = ops.alloc_padded_q8(c.B, c.H, c.W, c.dst2_ld, dev, pad=c.dst2_pad).fill_(R.SENT8)
    a, kw = case_args(c, y.view(-1), op.scale.to(dev), op.shift.to(dev), bufs["dst"], dst2=bufs.get("dst2"),
                      border=op.border.to(dev) if op.border is not None else None, pool_act=bufs.get("pool_act"),
                      dst_q8=bufs.get("dst_q8"), dst2_q8=bufs.get("dst2_q8"))
    ops.bn_act_fwd(*a, **kw)
    torch.cuda.synchronize()
    got = {}
    for name, buf in bufs.items():
        if name.endswith("q8"):
            assert buf.numel() == want[name].want.numel()
            got[name] = buf.cpu().to(torch.int32).view(-1, want[name].ld)
        else:
            got[name] = _got16(buf, want[name], "%s %s" % (c.name, name))
    return got, want, R.activation(c, op)


def check(c, got, want):
    q = query(c)
    assert (q.mode, q.fixed, q.y32, q.planes, q.q8) == A.instance(c), (c.name, q)
    for name in got:
        bad = R.first_mismatch(want[name], got[name])
        assert bad is None, "%s, %s, %s: %s" % (c.name, q, name, bad)


def relations(c, got, want, v):
    """what must hold between the outputs of one launch"""
    span = 4 * c.C if c.mode == A.REORG else c.C
    dst = want["dst"]
    hi = R.interior(dst, got["dst"], c.dst_choff, span)
    if c.planes == 3:
        assert torch.equal(R.interior(dst, got["dst"], c.dst_choff + 2 * c.dst_plane, span), hi), "third plane != first"
    if c.dst2 and c.planes2 == 3:
        d2 = want["dst2"]
        assert torch.equal(R.interior(d2, got["dst2"], c.dst2_choff + 2 * c.dst2_plane, c.C),
                           R.interior(d2, got["dst2"], c.dst2_choff, c.C)), "dst2: third plane != first"
    if c.mode == A.POOL and c.dst2 and c.planes == c.planes2 and c.twin == c.twin2:
        hi2 = R.interior(want["dst2"], got["dst2"], c.dst2_choff, c.C)
        as_f = lambda b: ((b ^ 0x8000) - 0x8000).to(torch.int16).contiguous().view(torch.float16).float()   # noqa: E731
        assert torch.equal(as_f(hi), F.max_pool2d(as_f(hi2), 2, 2)), "dst != the pool of dst2's hi plane"
        if c.twin:
            b1 = R.interior(want["dst_q8"], got["dst_q8"], c.dst_choff, c.C).to(torch.uint8)
            b2 = R.interior(want["dst2_q8"], got["dst2_q8"], c.dst2_choff, c.C).to(torch.uint8)
            assert torch.equal(b1, Q.pool_bytes(b2)), "pooled bytes != pool_bytes of the full-resolution twin"
    for name in ("dst_q8", "dst2_q8"):
        if name in got:
            inner = got[name][want[name].region == R.TWIN]
            assert not bool(((inner & 0x7F) == 0x7F).any()), "a NaN code in %s" % name
    if c.pool_act:
        pa = R.interior(want["pool_act"], got["pool_act"], 0, c.C)
        plain = R.bits16(R.hi16(v))
        w = R.window(plain)
        top = R.bits16(R.hi16(R.window(v).amax(0)))
        untied = ((w == top).sum(0) == 1)                                    # windows whose maximum is one fp16 value alone
        touched = (R.window(pa) != w).any(0)
        assert not bool((touched & untied).any()), "pool_act: an untied window was changed"
        moved = 0
        for (ho, wo), (ch, _) in A._windows(1.0).items():
            moved += int((R.window(pa)[:, 0, ch, ho, wo] != w[:, 0, ch, ho, wo]).sum())
        assert moved == 9, "pool_act: %d of the 9 planted neighbours were moved" % moved
        assert want["moved"] >= 9


@pytest.mark.parametrize("c", A.SMALL, ids=[c.name for c in A.SMALL])
def test_act_instance_exact(dev, c):
    got, want, v = run(dev, c)
    check(c, got, want)
    relations(c, got, want, v)


@pytest.mark.parametrize("c", A.BIG, ids=[c.name for c in A.BIG])
def test_act_grid_stride_exact(dev, c):
    """items > 4096 * 256: some threads take a second item of the grid-stride loop; the whole tensor is compared."""
    q = query(c)
    assert q.items > q.grid * 256
    got, want, _ = run(dev, c)
    check(c, got, want)


def test_hi_plane_is_the_same_in_every_form(dev):
    """forms 1 to 4 on the same operands: the hi plane of dst and of dst2 does not depend on what is stored beside it"""
    his = []
    for c in A.SAME_OPERANDS:
        got, want, v = run(dev, c)
        check(c, got, want)
        his.append((R.interior(want["dst"], got["dst"], c.dst_choff, c.C), R.interior(want["dst2"], got["dst2"], c.dst2_choff, c.C)))
    for h, h2 in his[1:]:
        assert torch.equal(h, his[0][0]) and torch.equal(h2, his[0][1])


# ------------------------------------------------------------------------------------------------ bn_coeffs_kernel
MOMENTUM, EPS = 0.1, 1e-5
ROWS, CS = (1, 127, 128, 129, 300), (8, 125, 200, 1024)
# (rows, C, training, permuted, ones_channel, count per row)
COEFF_CASES = [(r, c_, True, (i + j) % 2 == 1, (c_ - 2) if (i + j) % 3 == 0 else -1, 16) for i, r in enumerate(ROWS) for j, c_ in enumerate(CS)]
COEFF_CASES += [(0, c_, False, j % 2 == 0, 5 if j % 2 else -1, 16) for j, c_ in enumerate(CS)]
COEFF_CASES += [(1, 8, True, True, -1, 1), (1, 200, True, False, 7, 1)]               # count == 1: no unbiased correction


def within_one_ulp(got, want64):
    w = want64.float()
    inf = torch.full_like(w, float("inf"))
    return (got == w) | (got == torch.nextafter(w, inf)) | (got == torch.nextafter(w, -inf))


@functools.lru_cache(maxsize=None)
def coeff_operands(rows, C_, count_per_row):
    gen = torch.Generator().manual_seed(1000 * rows + C_ + count_per_row)
    ld = C_ + 8
    stats = None
    if rows:
        stats = torch.full((rows, 2, ld), float("nan"))
        n = count_per_row
        stats[:, 0, :C_] = torch.randint(-10 * n, 10 * n + 1, (rows, C_), generator=gen).float()
        if n == 1:
            stats[:, 1, :C_] = stats[:, 0, :C_] ** 2                     # one element per channel: variance 0
        else:
            stats[:, 1, :C_] = torch.randint(120 * n, 400 * n, (rows, C_), generator=gen).float()
            stats[:, 0, 3], stats[:, 1, 3] = float(n), 0.0               # s2 / count - mean^2 = -1: must clamp to 0
    gamma, beta = torch.randn(C_, generator=gen), torch.randn(C_, generator=gen)
    gamma[1] = 0.0
    rmean, rvar = torch.randn(C_, generator=gen), torch.rand(C_, generator=gen) + 0.5
    perm = torch.randperm(C_, generator=gen).to(torch.int32)
    return stats, gamma, beta, rmean, rvar, perm


@pytest.mark.parametrize("case", COEFF_CASES, ids=["-".join(str(int(v)) for v in k) for k in COEFF_CASES])
def test_bn_coeffs_one_ulp(dev, case):
    """scale, shift, mean, invstd and the running statistics within ONE fp32 ulp of the float64 value rounded to fp32.  The bar
    is derived, not measured: the kernel computes in double from exactly summed (integer-valued) slab entries, and two correctly
    rounded double evaluations of one expression can lie on the two sides of at most one fp32 rounding boundary.  Outputs are
    in physical channel order, parameters and running statistics in the module's order (`perm`); vectors start as NaN and must
    stay NaN beyond C; the NaN in the slab columns >= C must never be read."""
    rows, C_, training, permuted, ones, cpr = case
    stats, gamma, beta, rmean, rvar, perm = coeff_operands(rows, C_, cpr)
    count = max(rows, 1) * cpr
    perm = perm if permuted else None
    d = lambda t: t.to(dev).clone()                                           # noqa: E731
    out = {k: torch.full((C_ + 16,), float("nan"), device=dev) for k in ("scale", "shift", "mean", "invstd")}
    rm, rv = d(rmean), d(rvar)
    ops.bn_coeffs(d(stats) if training else None, C_, count, d(gamma), d(beta), rm, rv, training, out["scale"], out["shift"],
                  out["mean"], out["invstd"], momentum=MOMENTUM, eps=EPS, perm=d(perm) if permuted else None, ones_channel=ones)
    torch.cuda.synchronize()
    out = {k: t.cpu() for k, t in out.items()}
    for k, t in out.items():
        assert bool(torch.isnan(t[C_:]).all()), "%s written beyond C" % k
        assert not bool(torch.isnan(t[:C_]).any()), "%s: a NaN (from the slab's columns >= C?)" % k
    # float64 restatement
    pc = perm.long() if permuted else torch.arange(C_)
    g64, b64, rm64, rv64 = (t.double()[pc] for t in (gamma, beta, rmean, rvar))          # physical order
    m, e = (float(torch.tensor(x, dtype=torch.float32)) for x in (MOMENTUM, EPS))
    if training:
        s = stats.double()[:, :, :C_].sum(0)                                  # exact: integers
        mean = s[0] / count
        var = (s[1] / count - mean * mean).clamp(min=0.0)
        assert float(s[1][3] / count - mean[3] * mean[3]) < 0 or cpr == 1
        unbiased = var * count / (count - 1.0) if count > 1 else var
        new_rm, new_rv = (1.0 - m) * rm64 + m * mean, (1.0 - m) * rv64 + m * unbiased
        for name, got, want in (("running_mean", rm.cpu(), new_rm), ("running_var", rv.cpu(), new_rv)):
            ok = within_one_ulp(got[pc], want)
            assert bool(ok.all()), "%s: %d channels off by more than one ulp" % (name, int((~ok).sum()))
    else:
        mean, var = rm64, rv64
        assert torch.equal(rm.cpu(), rmean) and torch.equal(rv.cpu(), rvar), "eval mode changed the running statistics"
    invstd = 1.0 / torch.sqrt(var + e)
    scale = g64 * invstd
    keep = torch.ones(C_, dtype=torch.bool)
    if ones >= 0:
        keep[ones] = False
        assert float(out["scale"][ones]) == 0.0 and float(out["shift"][ones]) == 1.0, "ones_channel"
    for name, want in (("scale", scale), ("mean", mean), ("invstd", invstd)):
        ok = within_one_ulp(out[name][:C_], want) | (~keep if name == "scale" else torch.zeros_like(keep))
        assert bool(ok.all()), "%s: %d channels off by more than one ulp, first %d" % (name, int((~ok).sum()), int((~ok).nonzero()[0]))
    # shift = beta - mean * scale with the scale AS STORED (include/mcamd.h): the stored scale has just been checked
    shift = b64 - mean * out["scale"][:C_].double()
    ok = within_one_ulp(out["shift"][:C_], shift) | ~keep
    assert bool(ok.all()), "shift: %d channels off by more than one ulp, first %d" % (int((~ok).sum()), int((~ok).nonzero()[0]))
