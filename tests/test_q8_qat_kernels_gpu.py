"""Kernels of fp8 quantisation-aware training, each against the restatement in q8_qat_ref.py / q8_ref.py:
the raw fp32 epilogue of mcamd_conv_fwd_q8 with its statistics slab, the byte destinations of mcamd_bn_act_fwd,
mcamd_fakequant_q8 and the training form of the cast pass.

Shapes (B, H, W, cin, cout, k, pad form, input channel offset) are the smallest that reach every way the kernels can go
wrong: a ragged M over two pixel tiles with a ragged second filter tile, the 64-filter tile in the shared-halo form, a 1x1
with four chunks, one chunk (the ring's prologue only), and eleven pixel tiles that take the 256-filter tile under the fp8
MFMA."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops, _lib as L  # noqa: E402
from util import rel_l2  # noqa: E402
import q8_ref as R  # noqa: E402
import q8_qat_ref as Q  # noqa: E402
from test_q8_kernels_gpu import bytes_to_padded  # noqa: E402

SHAPES = [(2, 9, 11, 64, 200, 3, 0, 32), (3, 10, 14, 64, 72, 3, 1, 0), (2, 12, 12, 256, 136, 1, 0, 64),
          (1, 13, 13, 64, 48, 1, 0, 16), (2, 26, 26, 256, 512, 3, 1, 32)]
IDS = ["-".join(str(v) for v in c) for c in SHAPES]
TOL = 1e-3          # the project's kernel tolerance (fp8-MFMA form)


def operands(case, seed):
    """Generated as test_q8_kernels_gpu.run_case does; masks on odd seeds."""
    B, H, W, cin, cout, k, pad, choff = case
    gen = torch.Generator().manual_seed(seed)
    a8 = R.q(2.0 * F.leaky_relu(torch.randn(B, cin, H, W, generator=gen), 0.1))
    w = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    mask = (torch.rand(cout, cin, k, k, generator=gen) < 0.5).float() if seed % 2 else None
    return a8, w, mask


def run_raw(dev, case, seed):
    """-> (y NCHW cpu fp32, slab cpu, float64 reference y, a8, w8, e) of one raw launch, everything else checked here."""
    B, H, W, cin, cout, k, pad, choff = case
    a8, w, mask = operands(case, seed)
    ld = ops.round_up(choff + cin, 32)
    xb = bytes_to_padded(a8, ld, choff, pad, dev)
    g = ops.geom(B, H, W, k, cin, cout, ld, choff, 0, pad)
    assert ops.conv_fwd_q8_ok(g)
    wq, wexp = ops.pack_q8(g, w.to(dev).contiguous(), mask.to(dev).contiguous() if mask is not None else None)
    w8, e = R.quantise_weights(w, mask)
    assert torch.equal(wexp[:cout].cpu(), e), "exponents"
    rows = ops.conv_fwd_q8_stats_rows(g)
    assert rows == (B * H * W + 127) // 128
    yld, yoff = ops.round_up(cout + 12, 8), 8
    sld = ops.round_up(cout, 256)
    outs = []
    for _ in range(2):
        y = torch.full((B * H * W, yld), float("nan"), device=dev)
        slab = torch.full((rows, 2, sld), float("nan"), device=dev)
        ops.conv_fwd_q8_raw(g, xb, wq, wexp, y, yld, yoff, stats=slab)
        torch.cuda.synchronize()
        outs.append((y.cpu(), slab.cpu()))
    (y, slab), (y_b, slab_b) = outs
    assert bool(torch.isnan(y[:, :yoff]).all()) and bool(torch.isnan(y[:, yoff + cout:]).all()), "channels outside the slice"
    y = y[:, yoff:yoff + cout]
    assert not bool(torch.isnan(y).any()), "a y element was not written"
    assert not bool(torch.isnan(slab[:, :, :cout]).any()), "a slab row was not written"
    assert torch.equal(y, y_b[:, yoff:yoff + cout]) and torch.equal(slab[:, :, :cout], slab_b[:, :, :cout]), "two launches differ"
    with pytest.raises(L.McamdError):       # the slab row count must equal the query
        ops.conv_fwd_q8_raw(g, xb, wq, wexp, torch.empty(B * H * W, yld, device=dev), yld, yoff,
                            stats=torch.empty(rows + 1, 2, sld, device=dev))
    y = y.view(B, H, W, cout).permute(0, 3, 1, 2).contiguous()
    return y, slab[:, :, :cout], Q.raw(a8, w8, e), a8, w8, e


def check_stats(y, slab):
    """Per channel: the rows summed in float64 against float64 sums of the kernel's own y."""
    yd = y.double()
    s1, s2 = slab[:, 0].double().sum(0), slab[:, 1].double().sum(0)
    r1, r2 = yd.sum((0, 2, 3)), (yd * yd).sum((0, 2, 3))
    b1, b2 = 1e-5 * yd.abs().sum((0, 2, 3)), 1e-5 * r2
    print("stats: worst sum error / bar %.3g, sum of squares %.3g" % (float(((s1 - r1).abs() / b1).max()),
                                                                     float(((s2 - r2).abs() / b2).max())))
    assert bool(((s1 - r1).abs() <= b1).all()), "sums"
    assert bool(((s2 - r2).abs() <= b2).all()), "sums of squares"


@pytest.mark.parametrize("case", SHAPES, ids=IDS)
def test_raw_epilogue(dev, case):
    """fp32 y against the float64 convolution of the same codes: rel-L2 <= max(1e-6, 4 x the error of the CPU's own float32
    F.conv2d on the same dequantised operands); the statistics slab; bit-equal repeats."""
    seed = sum(case[:6])
    y, slab, y_ref, a8, w8, e = run_raw(dev, case, seed)
    k = case[5]
    y32 = F.conv2d(Q.x_q(a8), Q.w_q(w8, e), None, 1, (k - 1) // 2)
    cpu_err, err = rel_l2(y32, y_ref), rel_l2(y, y_ref)
    print("raw y rel-L2 %.3g (CPU float32 conv2d: %.3g)" % (err, cpu_err))
    assert err <= max(1e-6, 4 * cpu_err)
    check_stats(y, slab)


@pytest.mark.parametrize("case", SHAPES[-2:], ids=IDS[-2:])
def test_raw_epilogue_fp8_mfma(dev, setenv, case):
    """MCAMD_Q8_MFMA=1: the same epilogue behind the block-scaled fp8 MFMA (the 256-filter tile on the last shape), to the
    project's kernel tolerance."""
    setenv("MCAMD_Q8_MFMA", "1")
    y, slab, y_ref, _, _, _ = run_raw(dev, case, sum(case[:6]) + 1)
    err = rel_l2(y, y_ref)
    print("raw y rel-L2 %.3g (fp8 MFMA)" % err)
    assert err <= TOL
    check_stats(y, slab)


# (B, H, W, C, mode, dst2?, dst pad, dst2 pad, dst choff, byte twins of (dst, dst2))
ACT = [(2, 9, 11, 64, "plain", False, 0, 0, 0, (True, False)), (2, 9, 11, 200, "plain", False, 1, 0, 8, (True, False)),
       (3, 10, 14, 64, "pool", False, 1, 0, 8, (True, False)), (3, 10, 14, 200, "pool", False, 0, 0, 0, (True, False)),
       (2, 12, 12, 64, "pool", True, 0, 1, 8, (True, True)), (2, 12, 12, 200, "pool", True, 1, 0, 0, (True, True)),
       (2, 12, 12, 64, "pool", True, 1, 1, 8, (True, False)), (2, 12, 12, 64, "pool", True, 0, 0, 0, (False, True)),
       (2, 12, 12, 64, "reorg", False, 0, 0, 8, (True, False)), (2, 26, 26, 200, "reorg", False, 1, 0, 0, (True, False))]


def _interior(buf, f8, B, H, W, ld, pad):
    v = ops.padded_view_q8(buf, B, H, W, ld, pad) if f8 else ops.padded_view(buf, B, H, W, ld, pad)
    return v


def _check_dst(h16, b8, B, H, W, ld, choff, C, pad, v64, dst, twin, what):
    """One destination: bytes against store_bytes of the float64 evaluation (cap, adjacent codes), fp16 = deq(byte) / 2 bit
    for bit (or fp16(v) without a twin), halo and out-of-slice elements zero."""
    vh = _interior(h16, False, B, H, W, ld, pad)
    halo_ok = lambda v: bool((v[:, 0] == 0).all() and (v[:, -1] == 0).all() and (v[:, :, 0] == 0).all() and (v[:, :, -1] == 0).all())
    assert halo_ok(vh), what + ": fp16 halo"
    assert bool((vh[..., :choff] == 0).all() and (vh[..., choff + C:] == 0).all()), what + ": fp16 outside the slice"
    got16 = vh[:, 1:-1, 1:-1, choff:choff + C].permute(0, 3, 1, 2).float().cpu()
    if not twin:
        assert rel_l2(got16, R.store_fp16(v64, dst)) < TOL, what + ": fp16(v)"
        return None
    vb = _interior(b8, True, B, H, W, ld, pad)
    assert halo_ok(vb), what + ": byte halo"
    assert bool((vb[..., :choff] == 0).all() and (vb[..., choff + C:] == 0).all()), what + ": bytes outside the slice"
    got8 = vb[:, 1:-1, 1:-1, choff:choff + C].permute(0, 3, 1, 2).contiguous().cpu()
    share, adjacent = R.byte_mismatch(got8, R.store_bytes(v64, dst))
    print("%s: byte mismatch share %.3g (adjacent: %s)" % (what, share, adjacent))
    assert adjacent and share <= R.MISMATCH_CAP, what
    assert torch.equal(got16, R.deq(got8) / 2.0), what + ": fp16 twin is not deq(byte) / 2"
    return got8


@pytest.mark.parametrize("case", ACT, ids=["-".join(str(v) for v in c[:9]) + "-" + "".join("b" if t else "h" for t in c[9]) for c in ACT])
def test_act_pass_byte_destinations(dev, case):
    B, H, W, C, dst, dual, pad, pad2, choff, (tw, tw2) = case
    gen = torch.Generator().manual_seed(B + H + W + C + len(dst) + pad + 2 * pad2)
    yld, yoff = ops.round_up(C + 8, 8), 8
    y = torch.randn(B, C, H, W, generator=gen)
    scale, shift = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.2
    y[0, 0, 0, 0], scale[0], shift[0] = 400.0, 1.0, 0.0        # 2 v beyond the format's range: saturates at 448
    yb = torch.zeros(B * H * W, yld, device=dev)
    yb[:, yoff:yoff + C] = y.permute(0, 2, 3, 1).reshape(-1, C).to(dev)
    mode = {"plain": L.DST_PLAIN, "pool": L.DST_POOL, "reorg": L.DST_REORG}[dst]
    Ho, Wo = (H, W) if dst == "plain" else (H // 2, W // 2)
    cdst = 4 * C if dst == "reorg" else C
    ld, ld2, choff2 = ops.round_up(choff + cdst + 8, 32), ops.round_up(C + 40, 32), 16
    h16 = ops.alloc_padded(B, Ho, Wo, ld, dev, pad=pad)
    b8 = ops.alloc_padded_q8(B, Ho, Wo, ld, dev, pad=pad) if tw else None
    h16_2 = ops.alloc_padded(B, H, W, ld2, dev, pad=pad2) if dual else None
    b8_2 = ops.alloc_padded_q8(B, H, W, ld2, dev, pad=pad2) if (dual and tw2) else None
    ops.bn_act_fwd(B, H, W, C, yb.view(-1), yld, yoff, scale.to(dev), shift.to(dev), 0.1, mode, h16, ld, choff, h16_2,
                   ld2 if dual else 0, choff2 if dual else 0, dst_pad=pad, dst2_pad=pad2 if dual else 0, dst_q8=b8, dst2_q8=b8_2)
    torch.cuda.synchronize()
    v64 = Q.act(y, scale, shift, R.SLOPE, torch.float64)
    got8 = _check_dst(h16, b8, B, Ho, Wo, ld, choff, cdst, pad, v64, dst, tw, "dst")
    if tw and (dst == "plain"):
        assert int(got8[0, 0, 0, 0]) == 0x7E, "saturation at 448"
    if dual:
        got8_2 = _check_dst(h16_2, b8_2, B, H, W, ld2, choff2, C, pad2, v64, "plain", tw2, "dst2")
        if tw and tw2:
            assert torch.equal(got8, R.pool_bytes(got8_2)), "pooled bytes != pool_bytes of the full-resolution copy"


def test_act_pass_byte_destination_needs_fp32_y(dev):
    B, H, W, C = 1, 4, 4, 64
    y = torch.zeros(B * H * W * C, dtype=torch.float16, device=dev)
    one = torch.ones(C, device=dev)
    with pytest.raises(L.McamdError):
        ops.bn_act_fwd(B, H, W, C, y, C, 0, one, one, 0.1, L.DST_PLAIN, ops.alloc_padded(B, H, W, C, dev), C, 0,
                       dst_q8=ops.alloc_padded_q8(B, H, W, C, dev))


@pytest.mark.parametrize("shape,masked", [((72, 64, 3, 3), True), ((136, 256, 1, 1), False), ((16, 128, 1, 1), True)])
def test_fakequant_q8_equals_restatement(dev, shape, masked):
    gen = torch.Generator().manual_seed(sum(shape))
    cout, cin, k, _ = shape
    w = torch.randn(shape, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    mask = (torch.rand(shape, generator=gen) < 0.5).float() if masked else None
    w[1] = 0.0                                                  # an all-zero filter
    w[2] *= 1e-4                                                # a small one: a large exponent
    if masked:
        mask[3] = 0.0                                           # a filter masked entirely
    g = ops.geom(1, 8, 8, k, cin, cout, cin)
    wd, md = w.to(dev).contiguous(), (mask.to(dev).contiguous() if masked else None)
    _, wexp = ops.pack_q8(g, wd, md)
    got = ops.fakequant_q8(g, wd, md, wexp).cpu()
    assert torch.equal(got, Q.fakequant(w, mask))


def test_cast_q8_train_equals_restatement(dev):
    """The training form of the fp16 -> fp8 edge: the codes of mcamd_cast_q8, and the fp16 slice overwritten with
    deq(code) / 2; nothing outside the slice changes in either buffer."""
    gen = torch.Generator().manual_seed(2)
    P, sld, dld, C = 300, 96, 64, 40
    src = (torch.randn(P, sld, generator=gen) * 3).half()
    src[0, 8] = 300.0
    sd = src.to(dev).clone()
    dst = torch.zeros(P * dld, dtype=torch.uint8, device=dev)
    ops.cast_q8(sd.view(-1), P, sld, 8, C, dst, dld, 16, write_back=True)
    codes, back = Q.cast_train(src[:, 8:8 + C])
    got = dst.view(P, dld).cpu()
    assert torch.equal(got[:, 16:16 + C], codes)
    assert bool((got[:, :16] == 0).all()) and bool((got[:, 16 + C:] == 0).all())
    after = sd.cpu()
    assert torch.equal(after[:, 8:8 + C].float(), back)
    assert torch.equal(after[:, :8], src[:, :8]) and torch.equal(after[:, 8 + C:], src[:, 8 + C:])
    plain = torch.zeros_like(dst)
    ops.cast_q8(src.to(dev).view(-1), P, sld, 8, C, plain, dld, 16)
    assert torch.equal(plain, dst), "the codes are those of the inference cast"
