"""2:4 fp8 packer + block (mcamd_pack_q8_sparse24 / mcamd_conv_fwd_q8_sparse24, csrc/conv_q8_sparse.hip) through the C ABI,
teacher-forced per block against the float64 restatement in q8_ref.py -- a 2:4 mask is just a mask there -- with the
packing decoded on the host from the layout include/mcamd.h states (q8_sparse_ref.py).

Mask kinds, cycled over the cases by seed: 0 exactly 2 of 4; 1 at most 2 (groups with 1 or 0 kept, one filter and one tap
masked whole); 2 no mask, weights that are themselves 2:4.  The default form (fp16 sparse MFMAs on converted bytes) is held
to the byte cap q8_ref.MISMATCH_CAP; the fp8 sparse MFMA (MCAMD_Q8_MFMA=1) to the cap that follows from the width the
probe measured (q8_sparse_ref.FP8_SPARSE_MFMA_CAP), with adjacency and the fp16 tolerance."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops, _lib as L  # noqa: E402
from util import padded_to_nchw  # noqa: E402
import q8_ref as R  # noqa: E402
import q8_sparse_ref as S  # noqa: E402
from test_q8_kernels_gpu import bytes_to_padded, read_dst, check_dst, RAGGED, YOLO, SWITCH_RAGGED  # noqa: E402

YOLO_IDS = ["%d-%d-%d-k%d-%s%s" % (c[0], c[1], c[2], c[3], c[4], "-y2" if c[5] else "") for c in YOLO]


def pack(dev, g, w, mask):
    wq, idx, wexp = ops.pack_q8_sparse24(g, w.to(dev).contiguous(), mask.to(dev).contiguous() if mask is not None else None)
    return wq, idx, wexp


def run_case(dev, B, H, W, cin, cout, k, dst, dual, pad, choff, seed, y_f8, y2_f8=False, ref_images=None, cap=R.MISMATCH_CAP):
    gen = torch.Generator().manual_seed(seed)
    a8 = R.q(2.0 * F.leaky_relu(torch.randn(B, cin, H, W, generator=gen), 0.1))     # codes, subnormal ones included
    w = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    w, mask = S.make_mask(seed % 3, w, gen)
    scale, shift = torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.2
    ld = ops.round_up(choff + cin, 32)
    xb = bytes_to_padded(a8, ld, choff, pad, dev)
    g = ops.geom(B, H, W, k, cin, cout, ld, choff, 0, pad)
    assert ops.conv_fwd_q8_sparse24_ok(g)
    wq, idx, wexp = pack(dev, g, w, mask)
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
    ops.conv_fwd_q8_sparse24(g, xb, wq, idx, wexp, y, dld, off, scale.to(dev), shift.to(dev), 0.1, dst_mode=mode, y2=y2,
                             y2_ld=y2ld if dual else 0, y2_choff=32 if dual else 0, y_f8=y_f8, y2_f8=y2_f8)
    torch.cuda.synchronize()
    got, halo, outside = read_dst(y, y_f8, B, Ho, Wo, dld, cdst, off)
    assert halo, "halo of y"
    assert outside, "out-of-slice channels of y"
    imgs = list(range(B)) if ref_images is None else ref_images
    v_ref = R.block(a8[imgs], w8, e, scale, shift, R.SLOPE)
    over = []
    check_dst(got[imgs], v_ref, y_f8, dst, "y", over, cap)
    if dual:
        got2, halo2, outside2 = read_dst(y2, y2_f8, B, H, W, y2ld, cout, 32)
        assert halo2 and outside2, "halo / out-of-slice channels of y2"
        check_dst(got2[imgs], v_ref, y2_f8, "plain", "y2", over, cap)
        if y_f8 == y2_f8:
            assert torch.equal(got, R.pool_bytes(got2) if y_f8 else F.max_pool2d(got2, 2, 2)), "pooled y2 != y"
    assert not over, "; ".join(over)


# ----------------------------------------------------------------------------- packer
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("shape", [(64, 48, 1), (128, 264, 3), (1280, 72, 3)])
def test_pack_q8_sparse24_decodes_to_the_dense_codes(dev, shape, kind):
    cin, cout, k = shape
    gen = torch.Generator().manual_seed(cin + cout + kind)
    w, mask = S.make_mask(kind, torch.randn(cout, cin, k, k, generator=gen) * 0.05, gen)
    g = ops.geom(1, 4, 4, k, cin, cout, cin)
    wq, idx, wexp = pack(dev, g, w, mask)
    npad, ktot = ops.round_up(cout, 256), cin * k * k
    assert (wq.numel(), idx.numel(), wexp.numel()) == ops.q8_sparse24_elems(g) == (npad * ktot // 2, npad * ktot // 32, npad)
    w8, e = R.quantise_weights(w, mask)
    assert torch.equal(wexp[:cout].cpu(), e), "exponents"
    kept, words = wq.view(npad, ktot // 2).cpu(), idx.view(ktot // 64, npad, 2).cpu()
    dense = S.decompress(kept, words)
    assert torch.equal(R.deq(dense[:cout]), R.deq(S.dense_rows(w8))), "decoded packing != dense codes"
    assert bool((kept[cout:] == 0).all()) and bool((wexp[cout:] == 0).all()), "pad rows"
    # the offsets of every group are distinct and ascending, pad rows included
    off = ((words.to(torch.int64) & 0xFFFFFFFF).unsqueeze(-1) >> (2 * torch.arange(16))) & 3
    assert bool((off[..., 0::2] < off[..., 1::2]).all())
    # ... and they are the ones of the kept rule (zero-valued fill entries included)
    wm = w * mask if mask is not None else w
    want_kept, want_words = S.compress(w8, S.keep_positions(wm))
    assert torch.equal(words[:, :cout].to(torch.int64) & 0xFFFFFFFF, want_words)
    assert torch.equal(R.deq(kept[:cout]), R.deq(want_kept))


def test_pack_q8_sparse24_non_conforming_mask_keeps_the_first_two(dev):
    cin, cout, k = 128, 16, 3
    gen = torch.Generator().manual_seed(21)
    w = torch.randn(cout, cin, k, k, generator=gen) * 0.05
    mask = (torch.rand(cout, cin, k, k, generator=gen) < 0.7).float()      # groups with 3 and 4 non-zeros
    g = ops.geom(1, 4, 4, k, cin, cout, cin)
    wq, idx, wexp = pack(dev, g, w, mask)
    w8, e = R.quantise_weights(w, mask)                      # the exponent is the whole filter's
    assert torch.equal(wexp[:cout].cpu(), e)
    keep = S.keep_positions(w * mask)
    first_two = torch.zeros(cout, cin * k * k // 4, 4, dtype=torch.uint8).scatter_(
        2, keep, S.dense_rows(w8).view(cout, -1, 4).gather(2, keep)).view(cout, -1)
    assert not torch.equal(R.deq(first_two), R.deq(S.dense_rows(w8))), "the mask does not conform"
    dense = S.decompress(wq.view(256, -1).cpu(), idx.view(-1, 256, 2).cpu())
    assert torch.equal(R.deq(dense[:cout]), R.deq(first_two))


# ----------------------------------------------------------------------------- index bit order and k permutation
@pytest.mark.parametrize("mfma", ["0", "1"])
def test_q8_sparse_index_one_hot(dev, setenv, mfma):
    """A 1x1 block on a one-hot input (activation 0.5 = byte value 1.0 in channel c of pixel c), scale 1, shift 0, slope 1,
    fp16 destination returns 0.5 * w8[f, c] * 2^-e_f exactly at kept positions and exactly 0 at pruned ones: a single
    product per sum is exact in either instruction."""
    setenv("MCAMD_Q8_MFMA", mfma)
    cin, cout, H, W = 64, 8, 8, 8
    gen = torch.Generator().manual_seed(11)
    w = torch.randn(cout, cin, 1, 1, generator=gen) * 0.1
    mask = S.mask_24(cout, cin, 1, gen)
    mask[5, 32:] = 0.0
    mask[6] = 0.0
    mask[7, :, 0, 0] = torch.tensor([0.0, 0.0, 1.0, 1.0]).repeat(16)      # both kept at the high offsets
    a = torch.zeros(1, cin, H, W)
    a.view(1, cin, H * W)[0, torch.arange(cin), torch.arange(cin)] = 0.5
    a8 = R.q(2.0 * a)
    g = ops.geom(1, H, W, 1, cin, cout, cin)
    xb = bytes_to_padded(a8, cin, 0, 0, dev)
    wq, idx, wexp = pack(dev, g, w, mask)
    y = ops.alloc_padded(1, H, W, 32, dev)
    ops.conv_fwd_q8_sparse24(g, xb, wq, idx, wexp, y, 32, 0, torch.ones(cout, device=dev), torch.zeros(cout, device=dev), 1.0)
    got = padded_to_nchw(y, 1, H, W, 32, cout).view(cout, H * W)[:, :cin]
    w8, e = R.quantise_weights(w, mask)
    assert torch.equal(wexp[:cout].cpu(), e)
    want = (0.5 * R.deq(w8).view(cout, cin).double() * torch.pow(2.0, -e.double()).view(-1, 1)).float()
    assert torch.equal(want.half().float(), want), "fp16 holds the expected values"
    assert bool((want[mask.view(cout, cin) == 0] == 0).all()) and int((want != 0).sum()) > 100
    assert torch.equal(got, want)


# ----------------------------------------------------------------------------- blocks, default form
RAGGED_FMT = [(c, f) for c in RAGGED for f in (["f8", "f16", "f8+f16", "f16+f8"] if c[7] else ["f8", "f16"])]


@pytest.mark.parametrize("case,fmt", RAGGED_FMT)
def test_q8_sparse_ragged(dev, case, fmt):
    fy, fy2 = (fmt.split("+") + [fmt])[:2]
    run_case(dev, *case, seed=sum(case[:6]) + len(fmt), y_f8=fy == "f8", y2_f8=fy2 == "f8")


@pytest.mark.parametrize("case", YOLO, ids=YOLO_IDS)
def test_q8_sparse_yolov2_shapes(dev, case):
    H, cin, cout, k, dst, dual = case
    run_case(dev, 1, H, H, cin, cout, k, dst, dual, 0, 0, seed=H + cin + cout + 1, y_f8=True, y2_f8=True)


def test_q8_sparse_large_addresses(dev):
    """B = 64 at 104 x 104 (byte offsets of the last image beyond 2^25 pixels x channels): the float64 reference on the
    first and the last image."""
    run_case(dev, 64, 104, 104, 64, 128, 3, "pool", False, 0, 0, seed=7, y_f8=True, ref_images=[0, 63])


# ----------------------------------------------------------------------------- MCAMD_Q8_MFMA=1
@pytest.mark.parametrize("case", YOLO, ids=YOLO_IDS)
def test_q8_sparse_fp8_mfma_switch_yolov2_shapes(dev, setenv, case):
    """The fp8 sparse MFMA on every YOLOv2 shape at B=1 with byte destinations: the same plumbing, every differing byte the
    adjacent code, the share of differing bytes (printed) inside the cap of that instruction."""
    setenv("MCAMD_Q8_MFMA", "1")
    H, cin, cout, k, dst, dual = case
    run_case(dev, 1, H, H, cin, cout, k, dst, dual, 0, 0, seed=H + cin + cout + 1, y_f8=True, y2_f8=True,
             cap=S.FP8_SPARSE_MFMA_CAP)


@pytest.mark.parametrize("case,fmt", SWITCH_RAGGED)
def test_q8_sparse_fp8_mfma_switch(dev, setenv, case, fmt):
    """... and on ragged geometries (256-channel tile with a ragged last tile, both LDS tiles, REORG, the shared-halo form),
    fp16 destinations to TOL."""
    setenv("MCAMD_Q8_MFMA", "1")
    fy, fy2 = (fmt.split("+") + [fmt])[:2]
    run_case(dev, *case, seed=sum(case[:6]) + len(fmt), y_f8=fy == "f8", y2_f8=fy2 == "f8", cap=S.FP8_SPARSE_MFMA_CAP)
