"""csrc/conv_stem_block.hip per element and per channel against the float64 reference of stem_block_ref.py, on the
inputs of stem_block_cases.py: every pooled output element, the batch statistics of every channel, all 864 entries of dW
and the 32 of dgamma and dbeta, pool ties, every store slice, and one shape on which every kernel makes several passes.

Tolerances, in units of EPS32 * scale (`scale`: the value's own formula with every difference of like quantities replaced
by the sum of their magnitudes).  Measured yardsticks -- the float32 restatements on the CPU against the reference over
all inputs, printed by test_stem_block_cpu.py: forward 2.14, statistics 4.42, backward 0.148 units.  K = 4 x that, rounded
up to a power of two: K_FWD = 16, K_STATS = 32, K_BWD = 1 (stem_block_cases.py); the factor 4 is for the MFMA's internal
order and contraction.  On top of K units every value gets the rounding of the format it is stored in: half an fp16 ulp at
max(|ref|, |got|) for the pooled output (2^-22 |m| for hi + lo of the split storage), half a float32 ulp for the float32
results (an ulp of var + eps for the variance, which is read from the stored invstd).  The forward reference uses the
device's own scale / shift, the backward reference the device's saved mean / invstd / scale / shift (teacher forcing):
those are the kernels' inputs.  Pooled pixels with |z_win| or the gap to the runner-up inside (0, 1e-4) get G = 0 on both
sides -- at most 1e-3 of a case's; exact ties stay in.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops  # noqa: E402
from util import to_padded, padded_to_nchw, nchw_to_raw  # noqa: E402
import stem_block_ref as R  # noqa: E402
import stem_block_cases as SC  # noqa: E402

EPS32 = R.EPS32
SLICES = [(32, 0), (64, 32), (40, 8), (104, 72)]          # (dst_ld, dst_choff)


def first_beyond(got, ref, tol, what):
    """Every element of |got - ref| within tol; reports how many are not, and the first of them."""
    bad = torch.nonzero((got - ref).abs() > tol)
    worst = float(((got - ref).abs() / tol.clamp_min(1e-300)).max()) if tol.numel() else 0.0
    assert len(bad) == 0, "%s: %d of %d elements beyond the bound (largest %.2f x), the first at %s: %r against %r (bound %.3g)" % (
        what, len(bad), got.numel(), worst, bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]),
        float(tol[tuple(bad[0])]))
    return worst


def units(got, ref, scale):
    live = scale > 0
    return float(((got - ref).abs()[live] / (EPS32 * scale[live])).max()) if live.any() else 0.0


class Device:
    """The device side of a case: the padded NHWC4 image, the packed weights and the coefficient vectors."""

    def __init__(self, dev, c):
        self.dev, self.c, self.n = dev, c, c.w.shape[0]
        self.xb, _ = to_padded(c.x.to(dev))
        g = ops.geom(c.B, c.H, c.W, 3, 3, self.n, 4, 0, stem=1)
        self.mask = c.mask.to(dev).contiguous() if c.mask is not None else None
        self.wp, _ = ops.pack_weights(g, c.w.to(dev).contiguous(), self.mask)
        self.gamma, self.beta = c.gamma.to(dev), c.beta.to(dev)
        self.scale, self.shift, self.mean, self.invstd = (torch.full((self.n,), float("nan"), device=dev) for _ in range(4))
        self.ws = torch.empty(ops.stem_block_workspace_bytes(), dtype=torch.uint8, device=dev)
        self.rm, self.rv = c.rm0.to(dev), c.rv0.to(dev)

    def eval_coeffs(self):
        ops.bn_coeffs(None, self.n, 1, self.gamma, self.beta, self.rm, self.rv, False, self.scale, self.shift)

    def fwd(self, training, dst, ld, choff, planes=1, momentum=0.1, **kw):
        c = self.c
        ops.stem_block_fwd(c.B, c.H, c.W, self.xb, self.wp, self.gamma, self.beta, self.rm, self.rv, training, self.scale,
                           self.shift, self.mean, self.invstd, SC.SLOPE, dst, ld, choff, self.ws if training else None,
                           momentum=momentum, eps=SC.EPS, cout=self.n, planes=planes, **kw)

    def coeffs(self):
        return self.scale.cpu().double(), self.shift.cpu().double()

    def bwd(self, G, ld, choff, grad_scale):
        """dW, dgamma, dbeta for the gradient G [B, 32, H/2, W/2] (fp16 values) handed over as G * grad_scale."""
        c = self.c
        gb = nchw_to_raw(G * grad_scale, ld, choff)
        dw = torch.full((32, 3, 3, 3), float("nan"), device=self.dev)
        dgamma, dbeta = torch.full((32,), float("nan"), device=self.dev), torch.full((32,), float("nan"), device=self.dev)
        ops.stem_block_bwd(c.B, c.H, c.W, self.xb, self.wp, self.gamma, self.scale, self.shift, self.mean, self.invstd, SC.SLOPE,
                           gb, ld, choff, dw, dgamma, dbeta, self.ws, mask=self.mask, grad_scale=grad_scale)
        return dw.cpu(), dgamma.cpu(), dbeta.cpu()


def sentinel_dst(dev, B, H2, W2, ld):
    """A padded buffer whose every element, halo included, holds a finite pattern; (buffer, its [B][H2+2][W2+2][ld] view, a
    copy of the view's bits)."""
    dst = ops.alloc_padded(B, H2, W2, ld, dev)
    v = ops.padded_view(dst, B, H2, W2, ld)
    idx = torch.arange(v.numel(), device=dev)
    v.copy_((((idx * 37) % 509).float() * 0.25 - 63.0).half().view(v.shape))
    return dst, v, v.view(torch.int16).clone()


def check_untouched(dst, v, before, choff, span, what):
    """Bit for bit outside the slice's interior: other channels keep the sentinel, the halo is not written, and neither is
    anything behind the buffer's last pixel."""
    written = torch.zeros(v.shape, dtype=torch.bool, device=v.device)
    written[:, 1:-1, 1:-1, choff:choff + span] = True
    assert torch.equal(v.view(torch.int16)[~written], before[~written]), what
    assert not dst[v.numel():].any(), what
    assert bool((v.view(torch.int16)[written] != before[written]).any()), what      # (and the slice itself was written)


def check_pooled(got_hi, fw, K, what, got_lo=None):
    """The pooled output against the reference per element; got_lo: hi + lo of the split storage against the unrounded m."""
    got_hi = got_hi.double()
    hi = first_beyond(got_hi, fw.m, K * EPS32 * fw.scale + R.half_ulp16(torch.maximum(fw.m.abs(), got_hi.abs())), what)
    if got_lo is None:
        return hi
    return first_beyond(got_hi + got_lo.double(), fw.m, K * EPS32 * fw.scale + SC.LO_TERM * fw.m.abs(), what + " (hi + lo)")


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward per element

@pytest.mark.parametrize("masked", [False, True], ids=["dense", "masked"])
@pytest.mark.parametrize("B, H, W", SC.SHAPES)
def test_forward_per_element_every_slice(dev, B, H, W, masked):
    """Train-mode and eval-mode forward into every destination slice: every pooled element within K_FWD units and half an
    fp16 ulp of the reference on the device's own scale / shift; everything outside the slice's interior bit for bit as it
    was.  The three shapes' chains stay within the yardstick's 128 steps (asserted through the plan query)."""
    c = SC.make(B, H, W, masked)
    p = SC.pre(SC.make, B, H, W, masked)
    d = Device(dev, c)
    assert all(l.passes >= 1 and l.per_wave <= 128 for l in ops.stem_block_plan_info(B, H, W))
    H2, W2 = H // 2, W // 2
    for training in (True, False):
        fw = None
        for ld, choff in SLICES:
            dst, v, before = sentinel_dst(dev, B, H2, W2, ld)
            if not training:
                d.eval_coeffs()
            d.fwd(training, dst, ld, choff)
            what = "%dx%dx%d %s %s slice (%d, %d)" % (B, H, W, "masked" if masked else "dense", "train" if training else "eval", ld, choff)
            check_untouched(dst, v, before, choff, 32, what)
            if fw is None:
                fw = R.forward(p, *d.coeffs(), SC.SLOPE)
            worst = check_pooled(padded_to_nchw(dst, B, H2, W2, ld, 32, choff), fw, SC.K_FWD, what)
        print("%s: the last slice's largest error %.2f x its bound" % (what, worst))


@pytest.mark.parametrize("cout", [8, 16, 24])
def test_forward_slim_filters_per_element(dev, cout):
    """Eval-mode forward with fewer than 32 filters: the kept channels per element, channels cout..31 exactly zero."""
    B, H, W = 3, 6, 64
    c = SC.make(B, H, W, False, cout)
    d = Device(dev, c)
    d.eval_coeffs()
    ld, choff = 64, 32
    dst, v, before = sentinel_dst(dev, B, H // 2, W // 2, ld)
    d.fwd(False, dst, ld, choff)
    check_untouched(dst, v, before, choff, 32, "cout %d" % cout)
    fw = R.forward(SC.pre(SC.make, B, H, W, False, cout), *d.coeffs(), SC.SLOPE)
    got = padded_to_nchw(dst, B, H // 2, W // 2, ld, 32, choff)
    check_pooled(got[:, :cout], fw, SC.K_FWD, "cout %d" % cout)
    assert not got[:, cout:].any() and not torch.signbit(got[:, cout:]).any()


def split_device(dev, c):
    """hi / lo images and weights of the split-operand block, and its coefficients from the statistics pass."""
    hi, lo = ops.alloc_padded(c.B, c.H, c.W, 4, dev), ops.alloc_padded(c.B, c.H, c.W, 4, dev)
    ops.nchw_to_nhwc4_split(c.x.to(dev).contiguous(), hi, lo)
    d = Device(dev, c)
    wp_lo = torch.zeros_like(d.wp)
    d.wp.zero_()
    ops.pack_stem_split(c.w.to(dev).contiguous(), d.mask, d.wp, wp_lo)
    rows = ops.stem_block_stats_rows(c.B, c.H, c.W)
    assert rows == ops.stem_block_plan_info(c.B, c.H, c.W).stats.grid
    stats = torch.full((rows, 2, 32), float("nan"), device=dev)
    ops.stem_block_stats(c.B, c.H, c.W, hi, d.wp, stats, x_lo=lo, wp_lo=wp_lo)
    ops.bn_coeffs(stats, 32, c.B * c.H * c.W, d.gamma, d.beta, d.rm, d.rv, True, d.scale, d.shift, d.mean, d.invstd,
                  momentum=0.1, eps=SC.EPS)
    d.xb = hi
    return d, lo, wp_lo


@pytest.mark.parametrize("operands", ["plain", "split"])
@pytest.mark.parametrize("planes", [1, 2, 3])
def test_forward_planes_per_element(dev, planes, operands):
    """hi | lo | hi storage of the pooled output on plain and on split operands: the hi plane as every fp16 output, hi + lo
    against the unrounded m within K units + 2^-22 |m|, the third plane equal to the first.  Split operands go against the
    reference on the UNROUNDED fp32 image and weights with K_SPLIT = 16 units (the block's 2e-6 claim per element)."""
    B, H, W = SC.SHAPES[2]
    c = SC.make(B, H, W, True)
    span = 32 * planes
    ld, choff = span + 16, 8
    dst, v, before = sentinel_dst(dev, B, H // 2, W // 2, ld)
    if operands == "plain":
        d, K = Device(dev, c), SC.K_FWD
        d.fwd(True, dst, ld, choff, planes=planes)
        p = SC.pre(SC.make, B, H, W, True)
    else:
        (d, lo, wp_lo), K = split_device(dev, c), SC.K_SPLIT
        d.fwd(False, dst, ld, choff, planes=planes, x_lo=lo, wp_lo=wp_lo)
        p = R.pre(*SC.split_operands(c))
    what = "planes %d, %s operands" % (planes, operands)
    check_untouched(dst, v, before, choff, span, what)
    fw = R.forward(p, *d.coeffs(), SC.SLOPE)
    get = lambda k: padded_to_nchw(dst, B, H // 2, W // 2, ld, 32, choff + 32 * k)
    worst = check_pooled(get(0), fw, K, what, get(1) if planes >= 2 else None)
    print("%s: largest error %.2f x its bound" % (what, worst))
    if planes == 3:
        assert torch.equal(get(2), get(0))


# ---------------------------------------------------------------------------------------------------------------------
# 3. statistics per channel

def check_stats(mean, invstd, st, what, more_mean=0.0, more_var=0.0):
    """mean and var (read from the stored invstd) per channel: K_STATS units and the rounding of the stored float32."""
    mean, invstd = mean.cpu().double(), invstd.cpu().double()
    var = 1.0 / (invstd * invstd) - R.f32(SC.EPS)
    um = first_beyond(mean, st.mean, SC.K_STATS * EPS32 * st.scale_mean + 0.5 * EPS32 * st.mean.abs() + more_mean, what + " mean")
    uv = first_beyond(var, st.var, SC.K_STATS * EPS32 * st.scale_var + EPS32 * (st.var + R.f32(SC.EPS)) + more_var, what + " var")
    print("%s: mean %.2f units, var %.2f units (K = %g)" % (what, units(mean, st.mean, st.scale_mean), units(var, st.var, st.scale_var), SC.K_STATS))
    return um, uv


def coefficient_error(d, c, st):
    """E_c = |scale error| max|y_c| + |shift error| against 2^-12 |gamma_c|: by how much a pre-activation can move."""
    sc, sh = R.coeffs(st, c.gamma.double(), c.beta.double())
    got_sc, got_sh = d.coeffs()
    return ((got_sc - sc).abs() * st.ymax + (got_sh - sh).abs()) / (2.0 ** -12 * c.gamma.double().abs())


@pytest.mark.parametrize("route", ["gram", "split"])
@pytest.mark.parametrize("image", ["a", "b", "c"])
def test_statistics_per_channel(dev, image, route):
    """Batch statistics of a blob, an edge, a pruned, a tiny and a huge filter on a uniform, a low-contrast and a nearly
    constant image: the Gram route (mean, invstd, running statistics for momentum 0.1, 0 and 1) and the statistics pass on
    split operands followed by bn_coeffs (against the unrounded operands).  On "a" and "b" the coefficient error must not
    move a pre-activation by 2^-12 |gamma|; "c" is the stated conditioning limit: its E_c and kappa are printed."""
    c = SC.make_stats(image)
    B, H, W = SC.STATS_SHAPE
    M = float(B * H * W)
    if route == "gram":
        st = SC.stats(SC.make_stats, image)
        for momentum in (0.1, 0.0, 1.0):
            d = Device(dev, c)
            d.fwd(True, None, 0, 0, momentum=momentum)
            check_stats(d.mean, d.invstd, st, "image %s gram momentum %g" % (image, momentum))
            rm, rv, rm_s, rv_s = R.running(st, c.rm0.double(), c.rv0.double(), momentum)
            mo = R.f32(momentum)
            if momentum == 0.0:
                assert torch.equal(d.rm.cpu(), c.rm0) and torch.equal(d.rv.cpu(), c.rv0)
            if momentum == 1.0:
                assert torch.equal(d.rm, d.mean)
            first_beyond(d.rm.cpu().double(), rm, SC.K_STATS * EPS32 * mo * st.scale_mean + 0.5 * EPS32 * rm.abs(), "running mean")
            first_beyond(d.rv.cpu().double(), rv, SC.K_STATS * EPS32 * mo * st.scale_var * M / (M - 1) + 0.5 * EPS32 * rv.abs(), "running var")
    else:
        # the pass's own arithmetic: against float64 of the three products it accumulates, on the hi / lo operands it reads
        weff = c.w * c.mask
        st = R.stats_of(*R.split_product(c.x, weff), SC.EPS)
        d, _, _ = split_device(dev, c)
        check_stats(d.mean, d.invstd, st, "image %s split" % image)
        # ... and against the UNROUNDED operands.  hi + lo represents an operand v to 2^-23 |v| while lo is a normal fp16
        # number; below |v| = 2^-3 lo is subnormal and its rounding an ABSOLUTE 2^-25.  The relative parts and the dropped
        # x_lo w_lo (2^-22) are 2 units, inside K; the absolute part moves a y by at most D = 2^-25 (sum_k |v_k| + sum_k |w_k|),
        # so a mean by at most D and a variance by at most 2 std D + D^2.
        x, w = SC.split_operands(c)
        full = R.stats(x, w, SC.EPS)
        D = 2.0 ** -25 * (27.0 + w.abs().sum((1, 2, 3)))                   # image values are at most 1
        check_stats(d.mean, d.invstd, full, "image %s split, unrounded operands" % image, D, 2.0 * full.var.sqrt() * D + D * D)
        rm, rv, _, _ = R.running(st, c.rm0.double(), c.rv0.double(), 0.1)
        mo = R.f32(0.1)
        first_beyond(d.rm.cpu().double(), rm, SC.K_STATS * EPS32 * mo * st.scale_mean + 0.5 * EPS32 * rm.abs(), "running mean")
        first_beyond(d.rv.cpu().double(), rv, SC.K_STATS * EPS32 * mo * st.scale_var * M / (M - 1) + 0.5 * EPS32 * rv.abs(), "running var")
    E = coefficient_error(d, c, st)
    n = int(E.argmax())
    print("image %s %s: largest E_c %.3g x the 2^-12 |gamma| bar = %.3g at channel %d (kappa %.3g); blob E_c %.3g, kappa %.3g"
          % (image, route, float(E[n]), float(E[n]) * 2.0 ** -12 * abs(float(c.gamma[n])), n, float(st.kappa[n]),
             float(E[SC.BLOB]) * 2.0 ** -12 * abs(float(c.gamma[SC.BLOB])), float(st.kappa[SC.BLOB])))
    if image != "c":
        assert float(E.max()) <= 1.0, "channel %d: E_c is %.3g x the bar" % (n, float(E[n]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. backward per element, ties

def check_backward(d, p, st, fw, G, grad_scale, g_ld, g_choff, what):
    """dW, dgamma, dbeta per element against the reference teacher-forced on the device's saved vectors."""
    c = d.c
    sc, sh = d.coeffs()
    mask = c.mask.double() if c.mask is not None else None
    ref = R.backward(p, c.gamma.double(), d.mean.cpu().double(), d.invstd.cpu().double(), sc, sh, SC.SLOPE, G * grad_scale, st, mask=mask)
    dw, dgamma, dbeta = (t.double() for t in d.bwd(G, g_ld, g_choff, grad_scale))
    out = []
    for name, got, want, scale in (("dW", dw, ref.dw, ref.scale_dw), ("dgamma", dgamma, ref.dgamma, ref.scale_dgamma),
                                   ("dbeta", dbeta, ref.dbeta, ref.scale_dbeta)):
        want, scale = want / grad_scale, scale / grad_scale
        assert torch.isfinite(got).all()
        out.append(units(got, want, scale))
        first_beyond(got, want, SC.K_BWD * EPS32 * scale + 0.5 * EPS32 * want.abs(), "%s %s" % (what, name))
    if mask is not None:
        assert not dw[mask == 0].any() and float(dgamma[5]) == 0.0 and not dw[5].any()
    print("%s grad_scale %g: dW %.3f dgamma %.3f dbeta %.3f units (K = %g)" % (what, grad_scale, out[0], out[1], out[2], SC.K_BWD))
    return out


def excluded_gradient(c, fw):
    """G with the pooled pixels near a discontinuity zeroed, at most 1e-3 of them."""
    ex = R.excluded(fw, SC.TAU)
    share = float(ex.double().mean())
    assert share <= SC.MAX_EXCLUDED, share
    return torch.where(ex, torch.zeros(()), c.G), share


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "masked"])
@pytest.mark.parametrize("B, H, W", SC.SHAPES)
def test_backward_per_element(dev, B, H, W, masked):
    """All 864 entries of dW and the 32 of dgamma and dbeta within K_BWD units, for grad_scale 1 and 8; masked entries of
    dW and a pruned filter's dgamma exactly zero."""
    c = SC.make(B, H, W, masked)
    p, st = SC.pre(SC.make, B, H, W, masked), SC.stats(SC.make, B, H, W, masked)
    d = Device(dev, c)
    d.fwd(True, None, 0, 0)
    fw = R.forward(p, *d.coeffs(), SC.SLOPE)
    G, share = excluded_gradient(c, fw)
    what = "%dx%dx%d %s (excluded %.1e)" % (B, H, W, "masked" if masked else "dense", share)
    check_backward(d, p, st, fw, G, 1.0, 32, 0, what)
    check_backward(d, p, st, fw, G, SC.GRAD_SCALE, 64, 32, what)


@pytest.mark.parametrize("kind", ["rows", "cols", "bands"])
def test_ties_go_to_the_first_maximum(dev, kind):
    """Exact arithmetic on both sides (stem_block_cases.make_ties): at least a quarter of the windows tie, the tied
    positions' v differ, so dW tells which position received the gradient (test_stem_block_cpu.py: the last maximum
    instead of the first moves T by more than 1000 K units): the first maximum in (row, column) order."""
    c = SC.make_ties(kind)
    B, H, W = SC.TIES_SHAPE
    p, st = SC.pre(SC.make_ties, kind), SC.stats(SC.make_ties, kind)
    d = Device(dev, c)
    dst, v, before = sentinel_dst(dev, B, H // 2, W // 2, 32)
    d.fwd(True, dst, 32, 0)
    fw = R.forward(p, *d.coeffs(), SC.SLOPE)
    check_pooled(padded_to_nchw(dst, B, H // 2, W // 2, 32, 32, 0), fw, SC.K_FWD, "ties %s" % kind)
    assert float((fw.gap == 0).double().mean()) >= 0.25 and not ((fw.gap > 0) & (fw.gap < SC.TAU)).any()
    G, share = excluded_gradient(c, fw)
    check_backward(d, p, st, fw, G, 1.0, 32, 0, "ties %s (excluded %.1e)" % (kind, share))


# ---------------------------------------------------------------------------------------------------------------------
# 2. several passes of every persistent kernel

@pytest.fixture(scope="module")
def multipass(dev):
    """B = 5470, H = 6, W = 64: 32820 units, 65640 Gram steps, every image with content of its own.  The float64 convolution
    is computed once; the train-mode forward runs twice here and its outputs are kept."""
    B, H, W = SC.MULTIPASS
    c = SC.make_multipass()
    p, st = SC.pre(SC.make_multipass), SC.stats(SC.make_multipass)
    d = Device(dev, c)
    runs = []
    for _ in range(2):
        d.rm, d.rv = c.rm0.to(dev), c.rv0.to(dev)
        dst = ops.alloc_padded(B, H // 2, W // 2, 32, dev)
        d.fwd(True, dst, 32, 0)
        runs.append((dst, [t.clone() for t in (d.scale, d.shift, d.mean, d.invstd, d.rm, d.rv)]))
    fw = R.forward(p, *d.coeffs(), SC.SLOPE)
    return dict(c=c, p=p, st=st, d=d, runs=runs, fw=fw)


def test_multipass_every_kernel_makes_several_passes(multipass):
    plan = ops.stem_block_plan_info(*SC.MULTIPASS)
    print(plan)
    assert all(l.passes >= 2 for l in plan), plan
    assert all(l.per_wave <= 128 for l in plan), plan            # within the yardstick's chains


def test_multipass_forward_and_statistics(multipass):
    """The plain forward pass (2 passes) per element, the Gram pass (5 passes) per channel; two calls bit-identical."""
    B, H, W = SC.MULTIPASS
    (dst0, v0), (dst1, v1) = multipass["runs"]
    assert torch.equal(dst0, dst1) and all(torch.equal(a, b) for a, b in zip(v0, v1))
    worst = check_pooled(padded_to_nchw(dst0, B, H // 2, W // 2, 32, 32, 0), multipass["fw"], SC.K_FWD, "multi-pass forward")
    print("multi-pass forward: largest error %.2f x its bound" % worst)
    d = multipass["d"]
    check_stats(d.mean, d.invstd, multipass["st"], "multi-pass gram")


def test_multipass_statistics_pass(dev, multipass):
    """mcamd_stem_block_stats on plain operands (5 passes) followed by bn_coeffs, per channel; two calls bit-identical."""
    B, H, W = SC.MULTIPASS
    c, d = multipass["c"], multipass["d"]
    rows = ops.stem_block_plan_info(B, H, W).stats.grid
    slabs = []
    for _ in range(2):
        stats = torch.full((rows, 2, 32), float("nan"), device=dev)
        ops.stem_block_stats(B, H, W, d.xb, d.wp, stats)
        slabs.append(stats)
    assert torch.equal(slabs[0], slabs[1]) and torch.isfinite(slabs[0]).all()
    vec = [torch.empty(32, device=dev) for _ in range(4)]
    ops.bn_coeffs(slabs[0], 32, B * H * W, d.gamma, d.beta, c.rm0.to(dev), c.rv0.to(dev), True, vec[0], vec[1], vec[2], vec[3],
                  momentum=0.1, eps=SC.EPS)
    check_stats(vec[2], vec[3], multipass["st"], "multi-pass statistics pass")


def test_multipass_forward_two_planes(dev, multipass):
    """The planes = 2 forward pass (3 passes) on the same scale / shift: hi as the plain pass wrote it, hi + lo per element."""
    B, H, W = SC.MULTIPASS
    d = multipass["d"]
    outs = []
    for _ in range(2):
        dst = ops.alloc_padded(B, H // 2, W // 2, 64, dev)
        d.fwd(False, dst, 64, 0, planes=2)
        outs.append(dst)
    assert torch.equal(outs[0], outs[1])
    hi, lo = (padded_to_nchw(outs[0], B, H // 2, W // 2, 64, 32, k) for k in (0, 32))
    assert torch.equal(hi, padded_to_nchw(multipass["runs"][0][0], B, H // 2, W // 2, 32, 32, 0))
    worst = check_pooled(hi, multipass["fw"], SC.K_FWD, "multi-pass planes = 2", lo)
    print("multi-pass planes = 2: largest error of hi + lo %.2f x its bound" % worst)


def test_multipass_backward(dev, multipass):
    """The backward pass (17 passes) per element; two calls bit-identical."""
    c, d, fw = multipass["c"], multipass["d"], multipass["fw"]
    G, share = excluded_gradient(c, fw)
    first = d.bwd(G, 32, 0, 1.0)
    again = d.bwd(G, 32, 0, 1.0)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    check_backward(d, multipass["p"], multipass["st"], fw, G, 1.0, 32, 0, "multi-pass (excluded %.1e)" % share)
