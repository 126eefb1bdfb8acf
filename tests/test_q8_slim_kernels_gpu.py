"""The fp8 block of slim_export models (mcamd_pack_q8_slim / mcamd_conv_fwd_q8_slim, csrc/conv_q8.hip + conv_epi.h; DESIGN.md
3m), teacher-forced per block against the float64 restatement in q8_slim_ref.py: an input channel count that is a multiple
of 8 only on zero-padded weight rows, and the border table added by pixel class in the epilogue.

Inputs follow test_q8_kernels_gpu.run_case's law; the table is built the way slim.py builds it, from cin / 2 removed
channels (q8_slim_ref.make_case).  Every case runs with a byte and with an fp16 destination; halo bytes and out-of-slice
channels of the destinations are asserted untouched.  The shapes are the smallest that reach each way to go wrong:

  (2, 13, 13,  72,  40, 3, plain)   one full + one ragged K block; all nine classes of a 3x3 conv
  (2,  8,  6,  40,  24, 3, pool+y2) cin < 64; windows that mix classes; both LDS tiles (mixed destination formats)
  (1,  2,  2, 328, 136, 3, pool)    every pixel a corner: four classes in one window; six K blocks; two 64-filter tiles
  (2,  6, 10,  40,   8, 3, reorg)   conv21's form: 8 filters, reorg
  (1, 26, 26, 136,  72, 1, plain)   1x1: more than one pixel tile (676 pixels)
  (2,  1,  5,  72,  16, 3, plain)   H = 1: classes with top and bottom set
  (2, 12, 10, 200, 264, 3, plain)   a slice at x_choff 64 of a wider buffer whose other bytes are another tensor's codes;
                                    two filter tiles (the 256 x 128 tile under MCAMD_Q8_MFMA=1)
  (2,  9, 11,  72, 200, 3, plain)   ragged cin without a table (NULL)
  the first one in the shared-halo `pad` form

The default form of the kernel is held to q8_ref.MISMATCH_CAP, the fp8-MFMA form (MCAMD_Q8_MFMA=1) to q8_ref.FP8_MFMA_CAP;
every differing byte must be the adjacent code; fp16 destinations to 1e-3 rel-L2.  Bit-equality with the dense fp8 entry
points, with no tolerance, shows that the pad columns are zero and nothing else changed."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops, _lib as L  # noqa: E402
import q8_ref as R  # noqa: E402
import q8_slim_ref as S  # noqa: E402
from test_q8_kernels_gpu import bytes_to_padded, read_dst, check_dst  # noqa: E402

# (B, H, W, cin, cout, k, dst, y2, pad, choff, x_ld (0: the smallest), table)
CASES = [(2, 13, 13, 72, 40, 3, "plain", False, 0, 0, 0, True),
         (2, 8, 6, 40, 24, 3, "pool", True, 0, 0, 0, True),
         (1, 2, 2, 328, 136, 3, "pool", False, 0, 0, 0, True),
         (2, 6, 10, 40, 8, 3, "reorg", False, 0, 0, 0, True),
         (1, 26, 26, 136, 72, 1, "plain", False, 0, 0, 0, True),
         (2, 1, 5, 72, 16, 3, "plain", False, 0, 0, 0, True),
         (2, 12, 10, 200, 264, 3, "plain", False, 0, 64, 384, True),
         (2, 9, 11, 72, 200, 3, "plain", False, 0, 0, 0, False),
         (2, 13, 13, 72, 40, 3, "plain", False, 1, 0, 0, True)]


def finite_codes(shape, gen):
    """Random e4m3 codes that are neither a zero nor a NaN: what another tensor's bytes can look like."""
    b = torch.randint(1, 0x7F, shape, generator=gen, dtype=torch.int32)          # magnitude 0x01 .. 0x7e
    return (b | (torch.randint(0, 2, shape, generator=gen, dtype=torch.int32) << 7)).to(torch.uint8)


def padded_input(a8, ld, choff, pad, dev, gen=None):
    """The padded byte buffer of a case; with `gen`, every interior byte outside the slice holds a non-zero finite code
    (the halo stays 0x00, as in a buffer that several tensors share)."""
    B, C, H, W = a8.shape
    if gen is None:
        return bytes_to_padded(a8, ld, choff, pad, dev)
    full = finite_codes((B, ld, H, W), gen)
    full[:, choff:choff + C] = a8
    return bytes_to_padded(full, ld, 0, pad, dev)


def run_case(dev, case, seed, y_f8, y2_f8=False, cap=R.MISMATCH_CAP):
    B, H, W, cin, cout, k, dst, dual, pad, choff, ld, table = case
    a8, w, mask, scale, shift, border = S.make_case(B, H, W, cin, cout, k, seed, table)
    cin_pad = ops.round_up(cin, 64)
    ld = ld or ops.round_up(choff + cin_pad, 16)
    # every interior byte outside the slice -- the channels [cin, cin_pad) the K loop also reads among them -- holds a
    # non-zero finite code, as where another concat member lives there (0x00, a never-written pad byte, is the easy case)
    xb = padded_input(a8, ld, choff, pad, dev, torch.Generator().manual_seed(seed + 1))
    g = ops.geom(B, H, W, k, cin, cout, ld, choff, 0, pad)
    assert ops.conv_fwd_q8_slim_ok(g) and (cin % 64 == 0 or not ops.conv_fwd_q8_ok(g))
    wq, wexp = ops.pack_q8_slim(g, w.to(dev).contiguous(), mask.to(dev).contiguous() if mask is not None else None)
    w8, e = R.quantise_weights(w, mask)
    assert torch.equal(wexp[:cout].cpu(), e), "exponents"
    mode = {"plain": L.DST_PLAIN, "pool": L.DST_POOL, "reorg": L.DST_REORG}[dst]
    Ho, Wo = (H, W) if dst == "plain" else (H // 2, W // 2)
    cdst = 4 * cout if dst == "reorg" else cout
    off = 8
    dld = ops.round_up(off + cdst + 8, 32)
    y2ld = ops.round_up(cout + 40, 32)
    y = ops.alloc_padded_q8(B, Ho, Wo, dld, dev) if y_f8 else ops.alloc_padded(B, Ho, Wo, dld, dev)
    y2 = None
    if dual:
        y2 = ops.alloc_padded_q8(B, H, W, y2ld, dev) if y2_f8 else ops.alloc_padded(B, H, W, y2ld, dev)
    ops.conv_fwd_q8_slim(g, xb, wq, wexp, y, dld, off, scale.to(dev), shift.to(dev), 0.1, dst_mode=mode, y2=y2,
                         y2_ld=y2ld if dual else 0, y2_choff=32 if dual else 0, y_f8=y_f8, y2_f8=y2_f8,
                         border=border.to(dev) if border is not None else None)
    torch.cuda.synchronize()
    got, halo, outside = read_dst(y, y_f8, B, Ho, Wo, dld, cdst, off)
    assert halo, "halo of y"
    assert outside, "out-of-slice channels of y"
    v_ref = S.block_border(a8, w8, e, scale, shift, border, R.SLOPE)
    over = []
    check_dst(got, v_ref, y_f8, dst, "y", over, cap)
    if dual:
        got2, halo2, outside2 = read_dst(y2, y2_f8, B, H, W, y2ld, cout, 32)
        assert halo2 and outside2, "halo / out-of-slice channels of y2"
        check_dst(got2, v_ref, y2_f8, "plain", "y2", over, cap)
        if y_f8 == y2_f8:
            assert torch.equal(got, R.pool_bytes(got2) if y_f8 else torch.nn.functional.max_pool2d(got2, 2, 2)), "pooled y2 != y"
    assert not over, "; ".join(over)


def case_id(c):
    return "%d-%d-%d-c%d-n%d-k%d-%s%s%s%s%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], "-y2" if c[7] else "", "-pad" if c[8] else "",
                                                "-off%d" % c[9] if c[9] else "", "" if c[11] else "-notable")


# every case with a byte and with an fp16 destination; the one with a full-resolution copy also with one of each
CASES_FMT = [(c, f) for c in CASES for f in (["f8", "f16", "f8+f16", "f16+f8"] if c[7] else ["f8", "f16"])]


@pytest.mark.parametrize("case,fmt", CASES_FMT, ids=[case_id(c) + "-" + f for c, f in CASES_FMT])
def test_q8_slim_block(dev, case, fmt):
    fy, fy2 = (fmt.split("+") + [fmt])[:2]
    run_case(dev, case, seed=sum(case[:6]) + len(fmt), y_f8=fy == "f8", y2_f8=fy2 == "f8")


SWITCH = [(CASES[0], "f8"), (CASES[1], "f8"), (CASES[1], "f16+f8"), (CASES[4], "f8"), (CASES[6], "f8"), (CASES[6], "f16")]


@pytest.mark.parametrize("case,fmt", SWITCH, ids=[case_id(c) + "-" + f for c, f in SWITCH])
def test_q8_slim_block_fp8_mfma(dev, setenv, case, fmt):
    """MCAMD_Q8_MFMA=1, the block-scaled fp8 MFMA (the 256 x 128 tile on the 264-filter case): the same plumbing, every
    differing byte the adjacent code, the share of differing bytes inside q8_ref.FP8_MFMA_CAP, fp16 destinations to TOL."""
    setenv("MCAMD_Q8_MFMA", "1")
    fy, fy2 = (fmt.split("+") + [fmt])[:2]
    run_case(dev, case, seed=sum(case[:6]) + len(fmt), y_f8=fy == "f8", y2_f8=fy2 == "f8", cap=R.FP8_MFMA_CAP)


def _dense_and_slim(dev, B, H, W, cin_slim, cin_dense, cout, k, ld, seed, fill):
    """The same buffer and weights through mcamd_conv_fwd_q8 (cin_dense channels, the weight zero-extended) and through
    mcamd_conv_fwd_q8_slim (cin_slim channels, no table): (bytes, exponents) of each."""
    gen = torch.Generator().manual_seed(seed)
    a8 = R.q(2.0 * torch.nn.functional.leaky_relu(torch.randn(B, cin_slim, H, W, generator=gen), 0.1))
    w = torch.randn(cout, cin_slim, k, k, generator=gen) * (2.0 / (cin_slim * k * k)) ** 0.5
    mask = (torch.rand(cout, cin_slim, k, k, generator=gen) < 0.5).float()
    scale, shift = torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.2
    xb = padded_input(a8, ld, 0, 0, dev, gen if fill else None)
    if fill:
        v = xb.view(B, H + 2, W + 2, ld)[:, 1:-1, 1:-1, cin_slim:]
        assert bool((v != 0).all()) and bool(((v & 0x7F) != 0x7F).all()), "non-zero finite codes behind the slice"
    wz, mz = torch.zeros(cout, cin_dense, k, k), torch.zeros(cout, cin_dense, k, k)
    wz[:, :cin_slim], mz[:, :cin_slim] = w, mask
    out = []
    for slim in (False, True):
        g = ops.geom(B, H, W, k, cin_slim if slim else cin_dense, cout, ld)
        if slim:
            wq, wexp = ops.pack_q8_slim(g, w.to(dev).contiguous(), mask.to(dev).contiguous())
        else:
            wq, wexp = ops.pack_q8(g, wz.to(dev).contiguous(), mz.to(dev).contiguous())
        dld = ops.round_up(cout, 32)
        y = ops.alloc_padded_q8(B, H, W, dld, dev)
        fn = ops.conv_fwd_q8_slim if slim else ops.conv_fwd_q8
        fn(g, xb, wq, wexp, y, dld, 0, scale.to(dev), shift.to(dev), 0.1, y_f8=True)
        torch.cuda.synchronize()
        out.append((y.cpu(), wexp.cpu(), wq.cpu()))
    return out


def test_q8_slim_equals_dense_entry_points_at_cin_128(dev):
    """(a) cin 128, no table: output bytes, exponents and packed weights equal mcamd_conv_fwd_q8 / mcamd_pack_q8 on the same
    operands, bit for bit."""
    (yd, ed, wd), (ys, es, ws) = _dense_and_slim(dev, 2, 9, 11, 128, 128, 72, 3, 128, seed=21, fill=False)
    assert torch.equal(es, ed) and torch.equal(ws, wd) and torch.equal(ys, yd)
    assert bool((yd != 0).any())


@pytest.mark.parametrize("mfma", ["0", "1"])
def test_q8_slim_pad_columns_are_zero(dev, setenv, mfma):
    """(b) cin 72 in an ld = 128 buffer whose channels 72..127 hold random non-zero finite codes: output bytes and exponents
    equal mcamd_conv_fwd_q8 with cin 128 on that same buffer and the weight tensor zero-extended to 128 channels -- in
    both MFMA forms (a zero weight byte times a finite code is an exact 0 in either)."""
    setenv("MCAMD_Q8_MFMA", mfma)
    (yd, ed, wd), (ys, es, ws) = _dense_and_slim(dev, 2, 9, 11, 72, 128, 72, 3, 128, seed=22, fill=True)
    assert torch.equal(es, ed), "exponents"
    assert torch.equal(ys, yd), "output bytes"
    assert bool((yd != 0).any())


@pytest.mark.parametrize("k,cin,cout", [(3, 72, 24), (1, 136, 264), (3, 40, 8)])
def test_pack_q8_slim_layout(dev, k, cin, cout):
    """(c) pack_q8_slim's rows equal pack_q8 of the zero-extended weight, byte for byte (pad rows up to Npad included), and
    the kernel's K order [channel block of 64][tap][64] with 0x00 in the pad columns."""
    gen = torch.Generator().manual_seed(5 + cin)
    cp = ops.round_up(cin, 64)
    w = torch.randn(cout, cin, k, k, generator=gen) * 0.05
    mask = (torch.rand(cout, cin, k, k, generator=gen) < 0.7).float()
    wz, mz = torch.zeros(cout, cp, k, k), torch.zeros(cout, cp, k, k)
    wz[:, :cin], mz[:, :cin] = w, mask
    wq = torch.full((ops.q8_slim_elems(ops.geom(1, 4, 4, k, cin, cout, cp))[0],), 0xAB, dtype=torch.uint8, device=dev)
    wq, wexp = ops.pack_q8_slim(ops.geom(1, 4, 4, k, cin, cout, cp), w.to(dev).contiguous(), mask.to(dev).contiguous(), out_w=wq)
    wqd, wexpd = ops.pack_q8(ops.geom(1, 4, 4, k, cp, cout, cp), wz.to(dev).contiguous(), mz.to(dev).contiguous())
    assert wq.numel() == wqd.numel() and torch.equal(wq, wqd) and torch.equal(wexp, wexpd)
    w8, e = R.quantise_weights(w, mask)
    npad = ops.round_up(cout, 256)
    packed = wq.view(npad, cp // 64, k * k, 64).cpu()
    w8z = torch.zeros(cout, cp, k, k, dtype=torch.uint8)
    w8z[:, :cin] = w8
    assert torch.equal(packed[:cout], w8z.view(cout, cp // 64, 64, k * k).permute(0, 1, 3, 2))
    assert bool((packed[cout:] == 0).all()) and bool((wexp[cout:] == 0).all()) and torch.equal(wexp[:cout].cpu(), e)


def test_q8_slim_rejects_bad_arguments(dev):
    g = ops.geom(1, 4, 4, 3, 72, 40, 128)
    w = torch.randn(40, 72, 3, 3, device=dev)
    wq, wexp = ops.pack_q8_slim(g, w)
    xb = ops.alloc_padded_q8(1, 4, 4, 128, dev)
    y = ops.alloc_padded_q8(1, 4, 4, 64, dev)
    tab = torch.zeros(16, 40, device=dev)
    with pytest.raises(L.McamdError):       # a table narrower than cout
        ops.conv_fwd_q8_slim(g, xb, wq, wexp, y, 64, 0, None, None, 0.1, y_f8=True, border=tab, border_ld=32)
    with pytest.raises(L.McamdError):       # the pad crosses x_ld
        ops.conv_fwd_q8_slim(ops.geom(1, 4, 4, 3, 72, 40, 96), xb, wq, wexp, y, 64, 0, None, None, 0.1, y_f8=True)
    with pytest.raises(L.McamdError):       # the dense entry point still wants cin % 64 == 0
        ops.conv_fwd_q8(g, xb, wq, wexp, y, 64, 0, None, None, 0.1, y_f8=True)
