"""Block pruning and the block-sparse forward, kernel by kernel (csrc/prune.hip: mcamd_block_scores / mcamd_block_mask;
csrc/conv_bsparse.hip: mcamd_bsparse_lists / mcamd_conv_fwd_bsparse) against the numpy restatement bsparse_ref.py and the
dense kernels.  (These are the Gaussian checks on the network's shapes; test_bsparse_instances_gpu.py holds every
bsparse_kernel instance and the list kernel to an exact reference, in both `pad` forms.)"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import bsparse_ref as R  # noqa: E402
from modelcompression_amd import ops, _lib as L  # noqa: E402
from modelcompression_amd.pruning.weightPruning.layers import MaskedConv2d  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import block_prune  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2, to_padded, padded_to_nchw, halo_is_zero, q16  # noqa: E402

TOL = 1e-3

# (cout, cin, k): 32-channel blocks with a ragged last filter block of 8; 64-channel blocks, 1x1; the 3-channel first layer
# (no block form); eight filter blocks x four channel blocks x nine taps
SHAPES = [(136, 96, 3), (64, 128, 1), (32, 3, 3), (512, 256, 3)]


def weights(cout, cin, k, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5


def old_mask(shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) > 0.4).float()


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] % 32 == 0])
def test_block_scores_and_mask(dev, shape):
    cout, cin, k = shape
    w = weights(cout, cin, k, 11 + cout)
    for old in (None, old_mask(w.shape, 12 + cout)):
        got = ops.block_scores(w.to(dev).contiguous(), None if old is None else old.to(dev).contiguous()).cpu().numpy()
        ref = R.block_scores(w.numpy(), None if old is None else old.numpy())
        assert got.dtype == np.float64 and got.shape == ref.shape
        assert np.array_equal(got, ref), "scores differ from the documented summation order by up to %.3e (relative)" % (
            np.abs(got - ref).max() / ref.max())
        keep = (torch.rand(ref.shape[0], generator=torch.Generator().manual_seed(13)) > 0.5).to(torch.int32)
        m = ops.block_mask(keep.to(dev), tuple(w.shape), None if old is None else old.to(dev).contiguous())
        assert torch.equal(m.cpu(), torch.from_numpy(R.block_mask(keep.numpy(), tuple(w.shape), None if old is None else old.numpy())))


class Stack(nn.Module):
    """The four test shapes as the parameters of one model (block_prune only walks parameters and masks)."""

    def __init__(self, seed):
        super().__init__()
        self.convs = nn.ModuleList([MaskedConv2d(cin, cout, k, 1, (k - 1) // 2, bias=False) for cout, cin, k in SHAPES])
        self.bn = nn.BatchNorm2d(8)          # 1-D parameters: not pruned
        with torch.no_grad():
            for i, (c, (cout, cin, k)) in enumerate(zip(self.convs, SHAPES)):
                c.weight.copy_(weights(cout, cin, k, seed + i))


# (percentages whose virtual index (n - 1) perc / 100 is no integer for the 371 blocks of the stack, nor for its layers' 81,
# 2 and 288: the threshold then lies between two scores)
@pytest.mark.parametrize("perc,per_layer,with_old", [(45.0, False, False), (75.0, False, True), (57.0, True, False),
                                                     (100.0, False, False)])
def test_block_prune_matches_reference(dev, perc, per_layer, with_old):
    m = Stack(seed=21)
    ws = [c.weight.detach().clone().numpy() for c in m.convs]
    olds = None
    if with_old:
        olds = [old_mask(w.shape, 31 + i).numpy() for i, w in enumerate(ws)]
        olds[1] = None                       # a layer without a mask beside masked ones
    # the reference's thresholds must not sit on a score: a last-bit difference could not flip a block then
    scores = [R.block_scores(w, None if olds is None else olds[i]) for i, w in enumerate(ws) if w.shape[1] % 32 == 0]
    groups = scores if per_layer else [np.concatenate(scores)]
    for sc in groups:
        thr = R.threshold(sc, perc)
        if perc < 100.0:                     # (at 100 % the threshold IS the largest score: strict <, exact by construction)
            assert np.abs(sc - thr).min() > 1e-9 * thr, "pick another seed: the threshold is within 1e-9 of a score"
    m.to(dev)
    if with_old:
        for c, o in zip(m.convs, olds):
            if o is not None:
                c.set_mask(torch.from_numpy(o))
        ws = [c.weight.detach().cpu().numpy() for c in m.convs]      # (set_mask zeroed the masked weights)
    masks = block_prune(m, perc, per_layer=per_layer)
    ref = R.block_prune(ws, perc, olds, per_layer)
    assert len(masks) == len(SHAPES)
    for got, want, shape in zip(masks, ref, SHAPES):
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (shape[0], shape[1], shape[2], shape[2])
        assert torch.equal(got.cpu(), torch.from_numpy(want)), shape
    assert bool((masks[2] == (1 if olds is None else torch.from_numpy(olds[2]).to(dev))).all())      # ineligible: untouched
    if perc == 100.0:                        # every layer keeps exactly its best block (no ties in random data)
        for got, shape in zip(masks, SHAPES):
            if shape[1] % 32 == 0:
                idx = R.block_index(shape[0], shape[1], shape[2] * shape[2]).reshape(-1)
                alive = np.bincount(idx, weights=got.cpu().numpy().reshape(-1).astype(np.float64))
                assert int((alive > 0).sum()) == 1


def lists_case(dev, cout, cin, k, mask, seed):
    w = weights(cout, cin, k, seed) + 0.5 * torch.sign(weights(cout, cin, k, seed))      # no value rounds to zero in fp16
    g = ops.geom(1, 4, 4, k, cin, cout, cin)
    wp, _ = ops.pack_weights(g, w.to(dev).contiguous(), mask.to(dev).contiguous(), True, False)
    kb = R.block_kb(cin)
    packed = R.pack_fwd(w.numpy(), mask.numpy())
    assert np.array_equal(wp.cpu().numpy().reshape(packed.shape), packed)      # (by value: -0 == +0)
    count, lst = ops.bsparse_lists(g, wp)
    rc, rl = R.chunk_lists(packed, cout, kb)
    assert count.dtype == torch.int32 and lst.dtype == torch.int32 and tuple(lst.shape) == rl.shape
    assert torch.equal(count.cpu(), torch.from_numpy(rc)), (count.cpu().tolist(), rc.tolist())
    assert torch.equal(lst.cpu(), torch.from_numpy(rl))
    return rc


@pytest.mark.parametrize("shape", [(136, 96, 3), (512, 256, 3), (72, 1280, 3)])
def test_bsparse_lists(dev, shape):
    """Empty tiles, full tiles, one kept chunk per tile, a random block mask, an unstructured mask (full lists); the ragged
    last tile (136 and 72 filters) and more than 64 chunks per tile (1280 channels: 180, three ballot groups)."""
    cout, cin, k = shape
    nfb, ncb, kb = R.block_dims(cout, cin, k * k)
    nchunks = ncb * k * k
    gen = torch.Generator().manual_seed(41)
    keep = np.zeros((nfb, nchunks), np.int32)
    keep[1::3] = 1                                               # tile 0 empty, tile 1 full, ...
    for t in range(2, nfb, 3):
        keep[t] = 0
        keep[t, (37 * t + 5) % nchunks] = 1                      # ... tile 2 one chunk
    keep[nfb - 1] = 0
    keep[nfb - 1, nchunks - 1] = 1                               # the ragged last tile keeps the last chunk only
    rc = lists_case(dev, cout, cin, k, torch.from_numpy(R.block_mask(keep.reshape(-1), (cout, cin, k, k))), 42)
    assert rc[0] == 0 and rc[-1] == 1 and (nfb < 3 or rc[1] == nchunks)
    rnd = (torch.rand(nfb * nchunks, generator=gen) > 0.6).to(torch.int32).numpy()
    lists_case(dev, cout, cin, k, torch.from_numpy(R.block_mask(rnd, (cout, cin, k, k))), 43)
    rc = lists_case(dev, cout, cin, k, (torch.rand(cout, cin, k, k, generator=gen) > 0.8).float(), 44)      # unstructured, 80 % zeros
    assert (rc == nchunks).all()


# (B, H, W, cin, cout, k, dst, y2, pad, choff)
FWD = [(2, 9, 11, 96, 200, 3, "plain", False, 0, 32), (3, 10, 14, 64, 72, 3, "pool", False, 1, 0),
       (2, 12, 12, 256, 136, 1, "reorg", False, 0, 64), (2, 26, 26, 256, 512, 3, "pool", True, 1, 32),
       (2, 20, 20, 96, 64, 3, "pool", True, 0, 0), (2, 13, 13, 1280, 1024, 3, "plain", False, 1, 0),
       (1, 13, 13, 1024, 512, 1, "plain", False, 0, 0)]
FORCED = (0, 1, 2, 3, 4, None)      # per-tile chunk counts every case covers (None = all chunks): the ring's edge cases


def forced_mask(cout, cin, k, rnd, gen):
    """Random block mask (about half the chunks kept) whose tile t keeps exactly FORCED[(rnd * ntiles + t) % 6] chunks for
    the first six (round, tile) pairs; -> (mask, counts)."""
    nfb, ncb, kb = R.block_dims(cout, cin, k * k)
    nchunks = ncb * k * k
    keep = (torch.rand(nfb, nchunks, generator=gen) > 0.5).to(torch.int32).numpy()
    for t in range(nfb):
        j = rnd * nfb + t
        if j < len(FORCED):
            want = nchunks if FORCED[j] is None else min(FORCED[j], nchunks)
            keep[t] = 0
            keep[t, torch.randperm(nchunks, generator=gen)[:want].numpy()] = 1
    return torch.from_numpy(R.block_mask(keep.reshape(-1), (cout, cin, k, k))), keep.sum(1)


@pytest.mark.parametrize("bm", [128, 64])
@pytest.mark.parametrize("case", FWD, ids=["-".join(str(v) for v in c) for c in FWD])
def test_bsparse_forward(dev, setenv, case, bm):
    """(a) the launch on the lists equals the launch on full lists bit for bit, over the whole padded buffers; (b) the
    full-list launch equals the split-K pair with one slice bit for bit where that entry accepts the case (pad == 0: cases
    1, 3, 5 and 7), else the dense conv_fwd_padded within TOL (the pad == 1 cases 2, 4 and 6: mcamd_conv_fwd_splitk has
    no shared-halo form); (c) float64 conv2d of the fp16-rounded masked operands with the same epilogue, rel-L2 < 1e-3;
    (d) halo and out-of-slice channels zero, pooled == max_pool2d(y2).  Both M tiles (MCAMD_BSPARSE_BM)."""
    B, H, W, cin, cout, k, dst, dual, pad, choff = case
    setenv("MCAMD_BSPARSE_BM", str(bm))          # both M tiles of the kernel (128 rows is the default)
    gen = torch.Generator().manual_seed(sum(case[:6]))
    x = torch.randn(B, cin, H, W, generator=gen)
    w = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    scale, shift = torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.2
    ld = ops.round_up(choff + ops.round_up(cin, 32), 32)
    xb, _ = to_padded(x.to(dev), ld=ld, choff=choff, pad=pad)
    g = ops.geom(B, H, W, k, cin, cout, ld, choff, 0, pad)
    assert ops.conv_fwd_bsparse_ok(g)
    mode = {"plain": L.DST_PLAIN, "pool": L.DST_POOL, "reorg": L.DST_REORG}[dst]
    Ho, Wo = (H, W) if dst == "plain" else (H // 2, W // 2)
    cdst = 4 * cout if dst == "reorg" else cout
    off = 8
    dld = ops.round_up(off + cdst + 8, 32)
    y2ld = ops.round_up(cout + 40, 32)
    sc, sh = scale.to(dev), shift.to(dev)
    ntiles = (cout + 63) // 64
    nchunks = ops.bsparse_elems(g)[1] // ntiles
    seen = set()
    for rnd in range((len(FORCED) + ntiles - 1) // ntiles):
        mask, counts = forced_mask(cout, cin, k, rnd, gen)
        wd, md = w.to(dev).contiguous(), mask.to(dev).contiguous()
        wp, _ = ops.pack_weights(g, wd, md, True, False)
        count, lst = ops.bsparse_lists(g, wp)
        assert count.cpu().tolist() == counts.tolist()
        seen.update(counts.tolist())
        outs = {}
        for name in ("lists", "all", "dense"):
            y = ops.alloc_padded(B, Ho, Wo, dld, dev)
            y2 = ops.alloc_padded(B, H, W, y2ld, dev) if dual else None
            kw = dict(dst_mode=mode, y2=y2, y2_ld=y2ld if dual else 0, y2_choff=32 if dual else 0)
            if name == "lists":
                ops.conv_fwd_bsparse(g, xb, wp, count, lst, y, dld, off, sc, sh, 0.1, **kw)
            elif name == "all":
                ops.conv_fwd_bsparse(g, xb, wp, count, lst, y, dld, off, sc, sh, 0.1, all_chunks=True, **kw)
            elif pad == 0:
                ops.conv_fwd_splitk(g, xb, wp, y, dld, off, sc, sh, 0.1, slices=1, **kw)
            else:
                ops.conv_fwd_padded(g, xb, wp, y, dld, off, sc, sh, 0.1, **kw)
            outs[name] = (y, y2)
        y, y2 = outs["lists"]
        assert torch.equal(y, outs["all"][0]), "(a) lists vs all chunks, round %d" % rnd
        assert not dual or torch.equal(y2, outs["all"][1]), "(a) y2"
        got = padded_to_nchw(y, B, Ho, Wo, dld, cdst, off)
        if pad == 0:
            assert torch.equal(outs["all"][0], outs["dense"][0]), "(b) all chunks vs split-K with one slice"
            assert not dual or torch.equal(outs["all"][1], outs["dense"][1]), "(b) y2"
        else:
            e = rel_l2(got, padded_to_nchw(outs["dense"][0], B, Ho, Wo, dld, cdst, off))
            print("round %d: block-sparse vs conv_fwd_padded rel-L2 %.2e" % (rnd, e))
            assert e < TOL, "(b) vs conv_fwd_padded"
        act = F.leaky_relu(F.conv2d(q16(x).double(), q16(w * mask).double(), None, 1, (k - 1) // 2)
                           * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1), 0.1)
        ref = act if dst == "plain" else (F.max_pool2d(act, 2, 2) if dst == "pool" else O.reorg(act, 2))
        e = rel_l2(got, ref)
        print("round %d: counts %s, vs float64 rel-L2 %.2e" % (rnd, counts.tolist(), e))
        assert e < TOL, "(c) vs float64"
        assert halo_is_zero(y, B, Ho, Wo, dld), "(d) halo"
        v = ops.padded_view(y, B, Ho, Wo, dld)
        assert float(v[..., :off].abs().sum()) == 0 and float(v[..., off + cdst:].abs().sum()) == 0, "(d) out-of-slice channels"
        if dual:
            got2 = padded_to_nchw(y2, B, H, W, y2ld, cout, 32)
            assert rel_l2(got2, act) < TOL
            assert halo_is_zero(y2, B, H, W, y2ld)
            v2 = ops.padded_view(y2, B, H, W, y2ld)
            assert float(v2[..., :32].abs().sum()) == 0 and float(v2[..., 32 + cout:].abs().sum()) == 0
            assert torch.equal(got, F.max_pool2d(got2, 2, 2)), "(d) pooled == max_pool2d(y2)"
    assert {min(c, nchunks) for c in (0, 1, 2, 3, 4)} | {nchunks} <= seen


def test_bsparse_clamps_foreign_lists(dev):
    """A count above nchunks and indices outside [0, nchunks) are clamped into range: the launch stays inside its operands
    and computes what the clamped list says."""
    B, H, W, cin, cout, k = 1, 6, 6, 64, 64, 3
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, cin, H, W, generator=gen)
    w = weights(cout, cin, k, 6)
    xb, ld = to_padded(x.to(dev))
    g = ops.geom(B, H, W, k, cin, cout, ld)
    wp, _ = ops.pack_weights(g, w.to(dev).contiguous(), None, True, False)
    outs = []
    for cnt, lst in ((10 ** 6, [0, 1, 2, 3, 4, 5, 6, 7, 8 + 10 ** 6]), (9, list(range(9)))):
        y = ops.alloc_padded(B, H, W, 64, dev)
        ops.conv_fwd_bsparse(g, xb, wp, torch.tensor([cnt], dtype=torch.int32, device=dev),
                             torch.tensor([lst], dtype=torch.int32, device=dev), y, 64)
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
