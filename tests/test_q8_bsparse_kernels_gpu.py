"""The block-sparse fp8 forward, kernel by kernel (csrc/conv_q8_bsparse.hip: mcamd_q8_bsparse_lists /
mcamd_conv_fwd_q8_bsparse) against the numpy restatement q8_bsparse_ref.py, the dense fp8 entry and the
float64 restatement q8_ref.py, in both MFMA forms (MCAMD_Q8_MFMA)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import bsparse_ref as BR  # noqa: E402
import q8_bsparse_ref as R  # noqa: E402
import q8_ref as Q  # noqa: E402
import test_q8_kernels_gpu as K  # noqa: E402  (its buffers, read-back and caps: the ones mcamd_conv_fwd_q8 is held to)
from modelcompression_amd import ops, _lib as L  # noqa: E402


def weights(cout, cin, k, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5


def lists_case(dev, cout, cin, k, w, mask):
    """Device packing == the CPU packing byte for byte; device lists == the restatement on those bytes.  -> counts"""
    g = ops.geom(1, 4, 4, k, cin, cout, cin)
    wq, wexp = ops.pack_q8(g, w.to(dev).contiguous(), mask.to(dev).contiguous())
    w8, e = Q.quantise_weights(w, mask)
    packed = R.pack_bytes(w8.numpy())
    assert np.array_equal(wq.cpu().numpy().reshape(packed.shape), packed)
    count, lst = ops.q8_bsparse_lists(g, wq)
    rc, rl = R.chunk_lists(packed, cout)
    assert count.dtype == torch.int32 and lst.dtype == torch.int32 and tuple(lst.shape) == rl.shape
    assert torch.equal(count.cpu(), torch.from_numpy(rc)), (count.cpu().tolist(), rc.tolist())
    assert torch.equal(lst.cpu(), torch.from_numpy(rl))
    return rc


@pytest.mark.parametrize("shape", [(136, 128, 3), (512, 256, 3), (72, 1280, 3)])
def test_q8_bsparse_lists(dev, shape):
    """Empty tiles, full tiles, one kept chunk per tile, a random block mask, an unstructured mask (full lists), and kept
    weights that round to the zero byte (byte lists shorter than the mask's); the ragged last tile (136 and 72 filters) and
    more than 64 chunks per tile (1280 channels: 180, three ballot groups)."""
    cout, cin, k = shape
    nfb, ncb, kb = BR.block_dims(cout, cin, k * k)
    nchunks = ncb * k * k
    assert kb == 64
    gen = torch.Generator().manual_seed(41)
    w = weights(cout, cin, k, 42)
    w = w + 0.5 * torch.sign(w)                                  # no kept value rounds to the zero byte
    keep = np.zeros((nfb, nchunks), np.int32)
    keep[1::3] = 1                                               # tile 0 empty, tile 1 full, ...
    for t in range(2, nfb, 3):
        keep[t] = 0
        keep[t, (37 * t + 5) % nchunks] = 1                      # ... tile 2 one chunk
    keep[nfb - 1] = 0
    keep[nfb - 1, nchunks - 1] = 1                               # the ragged last tile keeps the last chunk only
    rc = lists_case(dev, cout, cin, k, w, torch.from_numpy(BR.block_mask(keep.reshape(-1), (cout, cin, k, k))))
    assert rc.tolist() == keep.sum(1).tolist() and rc[0] == 0 and rc[-1] == 1 and (nfb < 3 or rc[1] == nchunks)
    rnd = (torch.rand(nfb * nchunks, generator=gen) > 0.6).to(torch.int32).numpy()
    mask = torch.from_numpy(BR.block_mask(rnd, (cout, cin, k, k)))
    rc = lists_case(dev, cout, cin, k, w, mask)
    assert rc.tolist() == rnd.reshape(nfb, nchunks).sum(1).tolist()
    rc = lists_case(dev, cout, cin, k, w, (torch.rand(cout, cin, k, k, generator=gen) > 0.8).float())      # unstructured, 80 % zeros
    assert (rc == nchunks).all()
    # kept weights that round to the zero byte: every third kept chunk of the random block mask shrunk by 2^-20 in tiles that
    # keep another one (q8_bsparse_cpu: below half the smallest subnormal once the filter's largest weight sits in (224, 448])
    w2, want = w.clone(), rnd.reshape(nfb, nchunks).copy()
    for t in range(nfb):
        qs = np.nonzero(want[t])[0]
        for q in qs[1::3]:
            cb, tap = q // (k * k), q % (k * k)
            w2[64 * t:64 * t + 64, 64 * cb:64 * cb + 64, tap // k, tap % k] *= 2.0 ** -20
            want[t, q] = 0
    rc2 = lists_case(dev, cout, cin, k, w2, mask)
    assert rc2.tolist() == want.sum(1).tolist() and int(rc2.sum()) < int(rnd.sum()), "byte lists and mask lists differ"


# (B, H, W, cin, cout, k, dst, y2, choff): ragged filter and pixel tiles (+ an input channel offset); 4 chunks against the
# 3-stage ring; POOL with the full-resolution copy; one tile of 180 chunks
FWD = [(2, 9, 11, 128, 200, 3, "plain", False, 32), (2, 12, 12, 256, 136, 1, "reorg", False, 0),
       (2, 10, 14, 64, 72, 3, "pool", True, 0), (1, 13, 13, 1280, 64, 3, "plain", False, 0)]
FWD_FMT = [(c, f) for c in FWD for f in (["f8+f16", "f16+f8", "f8+f8", "f16+f16"] if c[7] else ["f8", "f16"])]
FORCED = (0, 1, 2, 3, 4, None)      # per-tile chunk counts every case covers (None = all chunks): the ring's edge cases


def forced_mask(cout, cin, k, rnd, gen):
    """Random block mask (about half the chunks kept) whose tile t keeps exactly FORCED[(rnd * ntiles + t) % 6] chunks for
    the first six (round, tile) pairs; -> (mask, counts)."""
    nfb, ncb, kb = BR.block_dims(cout, cin, k * k)
    nchunks = ncb * k * k
    keep = (torch.rand(nfb, nchunks, generator=gen) > 0.5).to(torch.int32).numpy()
    for t in range(nfb):
        j = rnd * nfb + t
        if j < len(FORCED):
            want = nchunks if FORCED[j] is None else min(FORCED[j], nchunks)
            keep[t] = 0
            keep[t, torch.randperm(nchunks, generator=gen)[:want].numpy()] = 1
    return torch.from_numpy(BR.block_mask(keep.reshape(-1), (cout, cin, k, k))), keep.sum(1)


@pytest.mark.parametrize("mfma", [0, 1], ids=["f16mfma", "f8mfma"])
@pytest.mark.parametrize("case,fmt", FWD_FMT, ids=["-".join(str(v) for v in c) + "-" + f for c, f in FWD_FMT])
def test_q8_bsparse_forward(dev, setenv, case, fmt, mfma):
    """(a) the launch on the lists equals the launch on full lists bit for bit, over the whole padded buffers; (b) the
    full-list launch equals mcamd_conv_fwd_q8 on the same operands bit for bit; (c) the float64 restatement q8_ref.block on
    the codes: byte destinations inside the cap test_q8_kernels_gpu.py holds mcamd_conv_fwd_q8 to in this MFMA form (every
    differing byte the adjacent code), fp16 destinations to its TOL; (d) halo and out-of-slice bytes zero, pooled == the pool
    of y2 on the order-preserving key where both destinations have one format."""
    B, H, W, cin, cout, k, dst, dual, choff = case
    setenv("MCAMD_Q8_MFMA", str(mfma))
    cap = Q.FP8_MFMA_CAP if mfma else Q.MISMATCH_CAP
    fy, fy2 = (fmt.split("+") + [fmt])[:2]
    y_f8, y2_f8 = fy == "f8", fy2 == "f8"
    gen = torch.Generator().manual_seed(sum(case[:6]) + len(fmt))
    a8 = Q.q(2.0 * F.leaky_relu(torch.randn(B, cin, H, W, generator=gen), 0.1))     # codes, subnormal ones included
    w = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    scale, shift = torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.2
    ld = ops.round_up(choff + cin, 32)
    xb = K.bytes_to_padded(a8, ld, choff, 0, dev)
    g = ops.geom(B, H, W, k, cin, cout, ld, choff, 0, 0)
    assert ops.conv_fwd_q8_bsparse_ok(g) and ops.conv_fwd_q8_bsparse_info(g).f8mfma == mfma
    mode = {"plain": L.DST_PLAIN, "pool": L.DST_POOL, "reorg": L.DST_REORG}[dst]
    Ho, Wo = (H, W) if dst == "plain" else (H // 2, W // 2)
    cdst = 4 * cout if dst == "reorg" else cout
    off = 8
    dld = ops.round_up(off + cdst + 8, 32)
    y2ld = ops.round_up(cout + 40, 32)
    sc, sh = scale.to(dev), shift.to(dev)
    ntiles = (cout + 63) // 64
    nchunks = ops.q8_bsparse_elems(g)[1] // ntiles
    seen, over = set(), []
    for rnd in range((len(FORCED) + ntiles - 1) // ntiles):
        mask, counts = forced_mask(cout, cin, k, rnd, gen)
        wq, wexp = ops.pack_q8(g, w.to(dev).contiguous(), mask.to(dev).contiguous())
        w8, e = Q.quantise_weights(w, mask)
        assert torch.equal(wexp[:cout].cpu(), e), "exponents"
        count, lst = ops.q8_bsparse_lists(g, wq)
        assert count.cpu().tolist() == counts.tolist()
        seen.update(counts.tolist())
        outs = {}
        for name in ("lists", "all", "dense"):
            y = ops.alloc_padded_q8(B, Ho, Wo, dld, dev) if y_f8 else ops.alloc_padded(B, Ho, Wo, dld, dev)
            y2 = None
            if dual:
                y2 = ops.alloc_padded_q8(B, H, W, y2ld, dev) if y2_f8 else ops.alloc_padded(B, H, W, y2ld, dev)
            kw = dict(dst_mode=mode, y2=y2, y2_ld=y2ld if dual else 0, y2_choff=32 if dual else 0, y_f8=y_f8, y2_f8=y2_f8)
            if name == "lists":
                ops.conv_fwd_q8_bsparse(g, xb, wq, wexp, count, lst, y, dld, off, sc, sh, 0.1, **kw)
            elif name == "all":
                ops.conv_fwd_q8_bsparse(g, xb, wq, wexp, count, lst, y, dld, off, sc, sh, 0.1, all_chunks=True, **kw)
            else:
                ops.conv_fwd_q8(g, xb, wq, wexp, y, dld, off, sc, sh, 0.1, **kw)
            outs[name] = (y, y2)
        torch.cuda.synchronize()
        y, y2 = outs["lists"]
        for what, a, b in (("(a) lists vs all chunks", "lists", "all"), ("(b) all chunks vs conv_fwd_q8", "all", "dense")):
            for i, buf in enumerate(("y", "y2")[:2 if dual else 1]):
                ta, tb = outs[a][i], outs[b][i]
                same = torch.equal(ta, tb)
                print("round %d %s %s: equal %s%s" % (rnd, what, buf, same, "" if same else
                                                      ", %d of %d elements differ" % (int((ta != tb).sum()), ta.numel())))
                assert same, "%s, %s, round %d (counts %s)" % (what, buf, rnd, counts.tolist())
        got, halo, outside = K.read_dst(y, y_f8, B, Ho, Wo, dld, cdst, off)
        assert halo, "(d) halo of y"
        assert outside, "(d) out-of-slice channels of y"
        v_ref = Q.block(a8, w8, e, scale, shift, Q.SLOPE)
        print("round %d: counts %s" % (rnd, counts.tolist()))
        K.check_dst(got, v_ref, y_f8, dst, "(c) y", over, cap)
        if dual:
            got2, halo2, outside2 = K.read_dst(y2, y2_f8, B, H, W, y2ld, cout, 32)
            assert halo2 and outside2, "(d) halo / out-of-slice channels of y2"
            K.check_dst(got2, v_ref, y2_f8, "plain", "(c) y2", over, cap)
            if y_f8 == y2_f8:
                assert torch.equal(got, Q.pool_bytes(got2) if y_f8 else F.max_pool2d(got2, 2, 2)), "(d) pooled y2 != y"
    assert {min(c, nchunks) for c in (0, 1, 2, 3, 4)} | {nchunks} <= seen
    assert not over, "; ".join(over)
