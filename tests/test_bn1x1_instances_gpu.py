"""Every bn_conv1x1_kernel<BN, CB> instance behind mcamd_bn_act_conv1x1_fwd (csrc/bn_conv1x1.hip) against a float64
reference that is not a kernel.

tests/bn1x1_cases.py holds the cases, their operands, the float64 restatement and the conditions under which the kernel's
output must EQUAL it (kind "exact") or stay within a derived fp32-summation bound of it (kind "value": Gaussian operands
with the conversion's edges planted); test_bn1x1_cases_cpu.py proves without a GPU that the table reaches all six instances
in both kinds and every boundary condition on both column tiles, and that every reference meets the conditions.

Every buffer starts as sentinels: the producer's y holds NaN outside its slice; the destination holds NaN in the hi plane's
interior (every element must be overwritten), a finite sentinel in the lo plane, zeros in the halo of the slice and NaN in
every other channel and pixel; the output and the whole statistics slab start as NaN.  After the launch the hi plane and the
output are compared with the reference bit for bit and value for value (a NaN counts as different), and everything else must
still hold what it held.  The only tolerances are bn1x1_cases.y_bound / stats_bounds, derived from the operands.

test_bn_conv1x1_gpu.py keeps the bit-equality with the two launches at its own shapes and the persistent-slot walk
("mtiles>slots": test_persistent_workgroup_takes_two_tiles); the value cases repeat that equality at every instance."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops, _lib as L  # noqa: E402
import bn1x1_cases as BC  # noqa: E402
import act_ref as R  # noqa: E402
from util import NAN, whole  # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(c):
    """operands and reference of a case, computed once and shared (never modified)"""
    if c.name not in _REF:
        o = BC.operands(c)
        _REF[c.name] = (o, BC.reference(c, o))
    return _REF[c.name]


def _check_instance(c):
    i = BC.info_of(c)
    assert (i.bn, i.cb) == c.expect, (c.name, i)
    assert set(c.tags) <= BC.boundary_tags(c, i), (c.name, i)
    return i


class Buffers:
    """The device buffers of one case, sentinel-filled, and the arguments of both routes."""

    def __init__(self, dev, c, o):
        self.c, self.dev = c, dev
        o = BC.launched(c, o)
        M, P = c.M, c.P
        self.py = torch.full((M, c.py_ld), NAN, device=dev)
        self.py[:, c.py_choff:c.py_choff + P] = o.y.float().to(dev)
        self.scale, self.shift = o.scale.to(dev), o.shift.to(dev)
        w = o.w.view(c.cout, P, 1, 1).to(dev).contiguous()
        self.g = BC.geom_of(c)
        self.wp = torch.zeros(ops.packed_elems(self.g)[0], dtype=torch.float16, device=dev)
        table = ops.pack_table([dict(w=w, dst_fwd=self.wp, cout=c.cout, cin=P, ksize=1, split=1)], dev)
        ops.pack_many(*table)
        self._keep = (w, table)

    def dst(self):
        """the destination: NaN in every channel and pixel, but zeros in the halo of the slice and the finite sentinel in the lo
        plane; the guard bands around the buffer keep their zeros (the two-launch route's forward may read them)"""
        c = self.c
        buf = ops.alloc_padded(c.B, c.H, c.W, c.ld, self.dev)
        v = ops.padded_view(buf, c.B, c.H, c.W, c.ld)
        v.fill_(NAN)
        v[..., c.choff:c.choff + 2 * c.P] = 0
        v[:, 1:-1, 1:-1, c.choff:c.choff + c.P] = NAN
        v[:, 1:-1, 1:-1, c.choff + c.P:c.choff + 2 * c.P] = BC.SENTINEL_LO
        return buf

    def outputs(self, rows):
        c = self.c
        y = torch.full((c.M, c.y_ld), NAN, device=self.dev)
        slab = torch.full((rows, 2, ops.round_up(c.cout, 256)), NAN, device=self.dev) if c.stats else None
        return y, slab

    def act_args(self, dst):
        c = self.c
        return ((c.B, c.H, c.W, c.P, self.py, c.py_ld, c.py_choff, self.scale, self.shift, c.slope, L.DST_PLAIN, dst, c.ld, c.choff),
                dict(planes=2, dst_plane=c.P, dst_pad=0))

    def fused(self, rows):
        dst = self.dst()
        before = whole(dst).clone()
        y, slab = self.outputs(rows)
        a, kw = self.act_args(dst)
        ops.bn_act_conv1x1_fwd(a, kw, self.g, self.wp, y, self.c.y_ld, self.c.y_choff, slab)
        torch.cuda.synchronize()
        return dst, before, y, slab

    def two_launches(self):
        """bn_act_fwd + conv_fwd_raw32 on the same values.  bn_act_fwd takes y slices in steps of 8 channels only, the fused
        launch in steps of 4: where the case's slice is off that grid, the activation pass reads a whole-buffer copy of it."""
        c = self.c
        dst = self.dst()
        a, kw = self.act_args(dst)
        if c.py_ld % 8 or c.py_choff % 8:
            own = self.py[:, c.py_choff:c.py_choff + c.P].contiguous()
            a = a[:4] + (own, c.P, 0) + a[7:]
        ops.bn_act_fwd(*a, **kw)
        y, slab = self.outputs(ops.stats_rows(self.g, L.EPI_RAW_F32))
        ops.conv_fwd_raw32(self.g, dst, self.wp, y, self.c.y_ld, self.c.y_choff, slab)
        torch.cuda.synchronize()
        return dst, y, slab


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _hi_plane(c, dst):
    """[M][P] fp16 (cpu): the interior of the hi plane"""
    v = ops.padded_view(dst, c.B, c.H, c.W, c.ld)
    return v[:, 1:-1, 1:-1, c.choff:c.choff + c.P].reshape(c.M, c.P).cpu()


def _assert_equal(c, i, what, got, want, block, block_name):
    """got [M][n] as stored; want float64 [M][n].  EQUAL value for value, and bit for bit where the reference is +-0; a NaN
    (an unwritten sentinel) is different."""
    g = got.double()
    bad = ~(g == want) | ((want == 0) & (torch.signbit(g) != torch.signbit(want)))
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    m, ch = idx[0].tolist()
    diff = (g - want)[bad]
    diff = diff[~torch.isnan(diff)]
    raise AssertionError("%s, bn_conv1x1_kernel<%d, %d>: %d of %d elements of %s differ from the reference; first (pixel, channel) (%d, %d) "
                         "[M tile %d, row %d of the tile; %s %d]: got %r want %r; difference min %r max %r, %d NaN among them; M tiles "
                         "touched %s, %ss touched %s"
                         % (c.name, i.bn, i.cb, int(bad.sum()), bad.numel(), what, m, ch, m // 128, m % 128, block_name, ch // block,
                            float(g[m, ch]), float(want[m, ch]), float(diff.min()) if diff.numel() else NAN,
                            float(diff.max()) if diff.numel() else NAN, int(bad.sum()) - diff.numel(),
                            sorted(set((idx[:, 0] // 128).tolist()))[:16], block_name, sorted(set((idx[:, 1] // block).tolist()))[:16]))


def _assert_untouched(c, i, dst, before, y):
    """Everything but the hi plane's interior and the output slice holds what it held: the lo plane its sentinel, the halo
    its zeros, every other channel and pixel its NaN, the guard bands their zeros."""
    after = whole(dst).clone()
    lo = dst.storage_offset()
    n = c.B * (c.H + 2) * (c.W + 2) * c.ld
    for t in (after, before):
        t[lo:lo + n].view(c.B, c.H + 2, c.W + 2, c.ld)[:, 1:-1, 1:-1, c.choff:c.choff + c.P] = 0
    bad = (_bits(after) != _bits(before)).nonzero().flatten()
    if bad.numel():
        e = int(bad[0]) - lo
        pix, ch = divmod(e, c.ld)
        where = "a guard band" if not 0 <= e < n else (
            "the lo plane" if c.choff + c.P <= ch < c.choff + 2 * c.P else ("the hi plane's halo" if c.choff <= ch < c.choff + c.P else
                                                                              "a channel outside the slice"))
        raise AssertionError("%s, bn_conv1x1_kernel<%d, %d>: %d elements of the destination outside the hi plane's interior were written; "
                             "first at padded pixel %d channel %d (%s): 0x%04x -> 0x%04x"
                             % (c.name, i.bn, i.cb, bad.numel(), pix, ch, where, int(_bits(before)[bad[0]]) & 0xFFFF,
                                int(_bits(after)[bad[0]]) & 0xFFFF))
    rest = torch.cat([y[:, :c.y_choff].reshape(-1), y[:, c.y_choff + c.cout:].reshape(-1)])
    assert bool(torch.isnan(rest).all()), "%s: %d elements of y outside the output slice were written" % (c.name, int((~torch.isnan(rest)).sum()))


def _check_slab(c, i, slab, ref):
    """-> (largest |s1 - ref| / bound, largest |s2 - ref| / bound) over the channels"""
    n = c.cout
    slab = slab.cpu()
    assert slab.shape[0] == i.rows
    assert not bool(torch.isnan(slab[:, :, :n]).any()), "%s: slab rows with NaN: %s" % (
        c.name, torch.isnan(slab[:, :, :n]).any(2).any(1).nonzero().flatten().tolist()[:16])
    # columns of the tile beyond the filters: the packing's zero rows, so zero sums; further columns belong to nobody
    assert bool((slab[:, :, n:i.bn] == 0).all()), "%s: slab columns [%d, %d) must hold the zero sums of the pad filters" % (c.name, n, i.bn)
    assert bool(torch.isnan(slab[:, :, i.bn:]).all()), "%s: slab columns >= %d were written" % (c.name, i.bn)
    s = slab.double().sum(0)[:, :n]
    b1, b2 = BC.stats_bounds(c, ref)
    e1, e2 = (s[0] - ref.s1).abs(), (s[1] - ref.s2).abs()
    k1, k2 = int((e1 - b1).argmax()), int((e2 - b2).argmax())
    r1, r2 = float((e1 / b1).max()), float((e2 / b2).max())
    print("%s: slab: largest |sum y - ref| %.6g (bound %.6g), largest |sum y^2 - ref| %.6g (bound %.6g); largest error / bound %.3g, %.3g"
          % (c.name, float(e1.max()), float(b1[int(e1.argmax())]), float(e2.max()), float(b2[int(e2.argmax())]), r1, r2))
    assert bool((e1 <= b1).all()) and bool((e2 <= b2).all()), (
        "%s, bn_conv1x1_kernel<%d, %d>: statistics miss; sum y: channel %d got %r want %r (allowed %r); sum y^2: channel %d got %r want %r "
        "(allowed %r)" % (c.name, i.bn, i.cb, k1, float(s[0][k1]), float(ref.s1[k1]), float(b1[k1]), k2, float(s[1][k2]), float(ref.s2[k2]),
                          float(b2[k2])))
    return r1, r2


def _run(dev, c):
    """One fused launch of a case into sentinel-filled buffers; the checks both kinds share.  -> (buffers, info, reference,
    hi plane, y slice, slab)"""
    i = _check_instance(c)
    o, ref = _ref(c)
    assert BC.exactness(c, o, ref) == [], c.name           # the conditions of exactness, on this case's own reference
    bufs = Buffers(dev, c, o)
    dst, before, y, slab = bufs.fused(i.rows)
    hi = _hi_plane(c, dst)
    _assert_equal(c, i, "the hi plane", hi, R.hi16(ref.v).double(), 64, "64-channel K block")
    assert torch.equal(R.bits16(hi), R.bits16(R.hi16(ref.v))), "%s: the hi plane differs in a sign of zero or a NaN payload" % c.name
    y = y.cpu()
    _assert_untouched(c, i, dst, before, y)
    return bufs, i, ref, hi, y[:, c.y_choff:c.y_choff + c.cout], slab


@pytest.mark.parametrize("c", BC.EXACT, ids=str)
def test_bn1x1_instance_exact(dev, c):
    """Small-integer planes out of the kernel's own conversion: the hi plane and y EQUAL the float64 reference."""
    bufs, i, ref, hi, y, slab = _run(dev, c)
    _assert_equal(c, i, "y", y, ref.y, 32, "32-filter wave column")
    if c.stats:
        _check_slab(c, i, slab, ref)


@pytest.mark.parametrize("c", BC.VALUE, ids=str)
def test_bn1x1_instance_value(dev, c):
    """Gaussian operands with the conversion's edges planted, slope 0.1: the hi plane EQUALS the float64 restatement; y and the
    slab are bit-equal to the two launches the kernel replaces and within the derived bounds of the float64 sums."""
    bufs, i, ref, hi, y, slab = _run(dev, c)
    dst2, y2, slab2 = bufs.two_launches()
    assert torch.equal(R.bits16(_hi_plane(c, dst2)), R.bits16(hi)), "%s: hi plane against bn_act_fwd" % c.name
    y2 = y2.cpu()[:, c.y_choff:c.y_choff + c.cout]
    assert torch.equal(_bits(y), _bits(y2)), "%s: y against the two launches: %d outputs differ" % (c.name, int((_bits(y) != _bits(y2)).sum()))
    bound = BC.y_bound(c, ref)
    err = (y.double() - ref.y).abs()
    k = int((err / bound).argmax())
    print("%s: y: largest |y - ref| %.6g (bound there %.6g); largest error / bound %.3g"
          % (c.name, float(err.max()), float(bound.reshape(-1)[int(err.argmax())]), float((err / bound).max())))
    if not bool((err <= bound).all()):                       # (a NaN misses)
        m, f = divmod(k, c.cout)
        raise AssertionError("%s, bn_conv1x1_kernel<%d, %d>: %d of %d outputs miss the float64 sum by more than gamma_K sum|products|; worst "
                             "(pixel, filter) (%d, %d) [M tile %d, 32-filter wave column %d]: got %r want %r, allowed %r"
                             % (c.name, i.bn, i.cb, int((~(err <= bound)).sum()), err.numel(), m, f, m // 128, f // 32, float(y[m, f]),
                                float(ref.y[m, f]), float(bound[m, f])))
    if c.stats:
        assert torch.equal(_bits(slab[:, :, :c.cout]), _bits(slab2[:, :, :c.cout])), "%s: the slab against the two launches" % c.name
        _check_slab(c, i, slab, ref)


@pytest.mark.parametrize("c", BC.ONEHOT, ids=str)
def test_bn1x1_onehot(dev, c):
    """One non-zero channel per pixel against filters with a distinct integer per channel, rotated per filter: every output is
    one triple of products that names the channel the kernel laid the value at, and the plane each part read."""
    bufs, i, ref, hi, y, slab = _run(dev, c)
    if bool((y.double() == ref.y).all()):
        return
    # where the value landed instead: the channel k whose filter entries explain the first wrong row
    bad = (~(y.double() == ref.y)).any(1).nonzero().flatten()
    m = int(bad[0])
    ch = int(BC.onehot_channel(m, c.P))
    h, l = float(ref.hi[m, ch]), float(ref.lo[m, ch])
    rows = {"hi w_hi + lo w_hi + hi w_lo": h * (ref.w_hi + ref.w_lo) + l * ref.w_hi,
            "hi w_hi + HI w_hi + hi w_lo (part 1 reads hi[])": 2 * h * ref.w_hi + h * ref.w_lo,
            "LO w_hi + lo w_hi + hi w_lo (part 0 reads lo[])": 2 * l * ref.w_hi + h * ref.w_lo,
            "hi w_hi + lo w_hi + LO w_lo (part 2 reads lo[])": (h + l) * ref.w_hi + l * ref.w_lo}
    found = ["%s at channel %d" % (name, k) for name, t in rows.items() for k in range(c.P) if bool((t[:, k] == y[m].double()).all())]
    _assert_equal(c, i, "y (pixel %d holds its value at channel %d [K block %d, piece %d]; the row the kernel wrote is what %s gives)"
                  % (m, ch, ch // 64, ch % 64 // 8, found or "no single channel"), y, ref.y, 32, "32-filter wave column")


@pytest.mark.parametrize("name", ["v-64x1-m147-n48-slices", "v-128x4-m144-n104-slices"])
def test_bn1x1_is_deterministic(dev, name):
    """Two launches of one case per column tile into fresh buffers: hi plane, y and slab bit-equal."""
    c = next(c for c in BC.VALUE if c.name == name)
    i = _check_instance(c)
    o, _ = _ref(c)
    bufs = Buffers(dev, c, o)
    a, b = bufs.fused(i.rows), bufs.fused(i.rows)
    assert torch.equal(_bits(whole(a[0])), _bits(whole(b[0]))), "%s: the destinations differ" % name
    assert torch.equal(_bits(a[2]), _bits(b[2])), "%s: y differs" % name
    assert torch.equal(_bits(a[3]), _bits(b[3])), "%s: the slabs differ" % name
