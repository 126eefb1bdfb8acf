"""The weight-sharing kernels (csrc/wshare.hip) against the numpy restatement of include/mcamd.h
(wshare_ref.py): every layer set once alone and once as one multi-segment table, every library call under
torch.cuda.set_sync_debug_mode("error").

Dyadic inputs (multiples of 2^-12): every float64 sum is exact in any order, so codebooks and codes are the reference's bit
for bit.  Gaussian inputs: codes and counts are exact given the centroids; two float64 summation orders of a cluster's n
members differ by at most n 2^-52 sum|w|, which bounds the sums and, with one fp32 rounding, the centroids."""
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import _lib, ops  # noqa: E402
import wshare_ref as R  # noqa: E402

SHAPES = [(3, 7, 3, 3), (16, 64, 1, 1), (_lib.WS_SLAB + 1, 1, 1, 1), (125, 64, 1, 1), (256, 128, 3, 3)]
BITS = [1, 4, 8]
MASKS = ["none", "random80", "zeros", "few", "last"]


@contextlib.contextmanager
def no_sync():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def numel(shape):
    return int(np.prod(shape))


@functools.lru_cache(maxsize=None)
def weights(shape, dist, seed=0):
    rng = np.random.default_rng(1000 * seed + numel(shape))
    if dist == "dyadic":
        w = rng.integers(-2048, 2049, numel(shape)).astype(np.float32) / np.float32(4096.0)
    else:
        w = (rng.normal(size=numel(shape)) * 0.05).astype(np.float32)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def mask(shape, kind, K):
    n = numel(shape)
    rng = np.random.default_rng(7 + n)
    if kind == "none":
        return None
    m = np.zeros(n, dtype=np.float32)
    if kind == "random80":
        m[rng.random(n) > 0.8] = 1.0
    elif kind == "few":
        m[rng.choice(n, max(1, min(n, K) // 2), replace=False)] = 1.0
    elif kind == "last":
        m[-1] = 1.0
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def ref_kmeans(shape, dist, kind, K, iters):
    trace = []
    c, codes = R.kmeans(weights(shape, dist), mask(shape, kind, K), K, iters, trace)
    return c, codes, trace


def table(dev, layers, K, codes=None, codebook=None):
    """layers: [(w numpy, mask numpy or None)] -> (ops.WsTable, items); built outside the no-sync region (uploads)."""
    items = []
    for s, (w, m) in enumerate(layers):
        items.append(dict(w=torch.from_numpy(np.array(w)).to(dev), mask=None if m is None else torch.from_numpy(np.array(m)).to(dev),
                          codes=(torch.from_numpy(np.array(codes[s])).to(dev) if codes is not None
                                 else torch.full((w.size,), 0xA5, dtype=torch.uint8, device=dev)), K=K))
    cb = None if codebook is None else torch.from_numpy(np.concatenate(codebook).astype(np.float32)).to(dev)
    return ops.WsTable(items, codebook=cb), items


def layer_sets(shapes):
    """every shape alone, then all of them as one table"""
    return [[s] for s in shapes] + [list(shapes)]


def books(t):
    cb = t.codebook.cpu().numpy()
    return [cb[o:o + int(it["K"])] for o, it in zip(t.offsets, t.items)]


# ----------------------------------------------------------------------------- dyadic: bit for bit
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("bits", BITS)
def test_dyadic_kmeans_is_the_reference_bit_for_bit(dev, bits, kind):
    K = 1 << bits
    for shapes in layer_sets(SHAPES):
        for iters in (1, 3, 6):
            t, items = table(dev, [(weights(s, "dyadic"), mask(s, kind, K)) for s in shapes], K)
            with no_sync():
                t.init()
                for _ in range(iters):
                    t.iterate()
                t.assign()
            for s, it, cb in zip(shapes, items, books(t)):
                want_c, want_codes, _ = ref_kmeans(s, "dyadic", kind, K, iters)
                assert cb.tobytes() == want_c.tobytes(), (s, iters, cb, want_c)
                got = it["codes"].cpu().numpy()
                keep = R.keep_of(got.size, mask(s, kind, K))
                assert np.array_equal(got[keep], want_codes[keep]) and (got[~keep] == 0).all(), (s, iters)


def test_linear_initialisation_alone(dev):
    for kind in ("none", "random80", "zeros"):
        t, _ = table(dev, [(weights(s, "gauss"), mask(s, kind, 256)) for s in SHAPES], 256)
        with no_sync():
            t.init()
        for s, cb in zip(SHAPES, books(t)):
            assert cb.tobytes() == R.init(weights(s, "gauss"), mask(s, kind, 256), 256).tobytes(), (s, kind)


# ----------------------------------------------------------------------------- gaussian: one round at a time
def check_round(s, kind, K, c_in, got_codes, got_sums, got_counts, got_c):
    w, m = weights(s, "gauss"), mask(s, kind, K)
    keep = R.keep_of(w.size, m)
    codes = R.assign(c_in, w)
    assert np.array_equal(got_codes[keep], codes[keep]) and (got_codes[~keep] == 0).all(), (s, kind)
    sums, counts, sabs = R.sums_counts(w, codes, keep, K)
    assert np.array_equal(got_counts, counts), (s, kind)
    slack = counts * 2.0 ** -52 * sabs
    assert (np.abs(got_sums - sums) <= slack).all(), (s, kind, np.abs(got_sums - sums).max())
    c_ref = R.update(c_in, w, codes, keep)
    bound = R.ulp32(c_ref) + slack / np.maximum(counts, 1)
    empty = counts == 0
    assert (np.abs(got_c.astype(np.float64) - c_ref.astype(np.float64)) <= bound).all(), (s, kind)
    assert got_c[empty].tobytes() == c_in[empty].tobytes()                  # an empty cluster keeps its centroid, exactly


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("bits", BITS)
def test_gaussian_rounds_given_the_reference_centroids(dev, bits, kind):
    K = 1 << bits
    for shapes in layer_sets(SHAPES):
        for r in (0, 2):                          # the linear codebook, and the reference's after two rounds
            c_in = [ref_kmeans(s, "gauss", kind, K, 3)[2][r] for s in shapes]
            t, items = table(dev, [(weights(s, "gauss"), mask(s, kind, K)) for s in shapes], K, codebook=c_in)
            with no_sync():
                t.iterate()
            sums, counts = t.sums.cpu().numpy(), t.counts.cpu().numpy()
            for s, it, o, cb, c0 in zip(shapes, items, t.offsets, books(t), c_in):
                check_round(s, kind, K, c0, it["codes"].cpu().numpy(), sums[o:o + K], counts[o:o + K], cb)
            # assign alone gives the same codes against the same centroids
            t2, items2 = table(dev, [(weights(s, "gauss"), mask(s, kind, K)) for s in shapes], K, codebook=c_in)
            with no_sync():
                t2.assign()
            for s, a, b in zip(shapes, items, items2):
                keep = torch.from_numpy(R.keep_of(numel(s), mask(s, kind, K))).to(dev)
                assert torch.equal(a["codes"][keep], b["codes"][keep])
            assert torch.equal(t2.codebook, torch.from_numpy(np.concatenate(c_in)).to(dev))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gaussian_kmeans_end_to_end(dev, seed):
    """(4097 weights, K = 16, 6 rounds, sigma 0.05): asserted first, on the CPU, that in the reference run no weight comes
    within 4 fp32 ulps of a midpoint at any round, so a centroid that differs in its last bit cannot move a code."""
    n, K, iters = _lib.WS_SLAB + 1, 16, 6
    w = (np.random.default_rng(seed).normal(size=n) * 0.05).astype(np.float32)
    trace = []
    want_c, want_codes = R.kmeans(w, None, K, iters, trace)
    assert R.min_midpoint_gap_ulps(w, None, trace) >= 4.0
    t, items = table(dev, [(w, None)], K)
    with no_sync():
        t.init()
        for _ in range(iters):
            t.iterate()
        t.assign()
    assert np.array_equal(items[0]["codes"].cpu().numpy(), want_codes)
    keep = np.ones(n, dtype=bool)
    _, counts, sabs = R.sums_counts(w, R.assign(trace[-2], w), keep, K)
    bound = R.ulp32(want_c) + counts * 2.0 ** -52 * sabs / np.maximum(counts, 1)
    assert (np.abs(books(t)[0].astype(np.float64) - want_c.astype(np.float64)) <= bound).all()


# ----------------------------------------------------------------------------- project / expand
def random_codes(shape, K):
    rng = np.random.default_rng(99 + numel(shape))
    used = max(1, (3 * K) // 4)                    # the upper quarter of the codebook has no member
    return rng.integers(0, used, numel(shape)).astype(np.uint8)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("bits", BITS)
def test_project(dev, bits, kind):
    K = 1 << bits
    for shapes in layer_sets(SHAPES):
        layers, codes, c_in = [], [], []
        for s in shapes:
            w, m = np.array(weights(s, "gauss")), mask(s, kind, K)
            if m is not None:
                w[m == 0] = 7.25                  # garbage where the layer is pruned: never read into a mean, never written
            layers.append((w, m))
            codes.append(random_codes(s, K))
            c_in.append(np.linspace(-1, 1, K).astype(np.float32))
        runs = []
        for _ in range(2):                        # two fresh runs
            t, items = table(dev, layers, K, codes=codes, codebook=c_in)
            with no_sync():
                t.project()
            first = [it["w"].clone() for it in items], t.codebook.clone()
            with no_sync():
                t.project()                       # the layer is tied now: the identity, bit for bit
            assert all(torch.equal(a.view(torch.int32), it["w"].view(torch.int32)) for a, it in zip(first[0], items))
            assert torch.equal(first[1].view(torch.int32), t.codebook.view(torch.int32))
            runs.append(([a.cpu().numpy() for a in first[0]], first[1].cpu().numpy(), t.counts.cpu().numpy()))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][0], runs[1][0])) and runs[0][1].tobytes() == runs[1][1].tobytes()
        got_w, got_cb, got_counts = runs[0]
        for s, (w, m), cd, c0, o, gw in zip(shapes, layers, codes, c_in, t.offsets, got_w):
            keep = R.keep_of(w.size, m)
            sums, counts, sabs = R.sums_counts(w, cd, keep, K)
            _, c_ref = R.project(w, m, cd, c0)
            cb = got_cb[o:o + K]
            assert np.array_equal(got_counts[o:o + K], counts)
            bound = R.ulp32(c_ref) + counts * 2.0 ** -52 * sabs / np.maximum(counts, 1)
            assert (np.abs(cb.astype(np.float64) - c_ref.astype(np.float64)) <= bound).all(), (s, kind)
            assert cb[counts == 0].tobytes() == c0[counts == 0].tobytes()
            assert gw[keep].tobytes() == cb[cd[keep]].tobytes()              # every member holds its cluster's entry
            assert (gw[~keep] == np.float32(7.25)).all()


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("bits", BITS)
def test_expand(dev, bits, kind):
    K = 1 << bits
    for shapes in layer_sets(SHAPES):
        layers = [(np.full(numel(s), 7.25, dtype=np.float32), mask(s, kind, K)) for s in shapes]
        codes = [np.random.default_rng(5 + numel(s)).integers(0, K, numel(s)).astype(np.uint8) for s in shapes]
        c_in = [np.random.default_rng(6 + numel(s)).normal(size=K).astype(np.float32) for s in shapes]
        c_in[0][0] = -0.0
        t, items = table(dev, layers, K, codes=codes, codebook=c_in)
        with no_sync():
            t.expand()
        for (w, m), cd, c0, it in zip(layers, codes, c_in, items):
            assert it["w"].cpu().numpy().tobytes() == R.expand(c0, cd, m).tobytes()


def test_mixed_bits_in_one_table(dev):
    """Segments of different K share the arrays: offsets are the running sums of K."""
    Ks = [2, 256, 16, 4, 256]
    items = []
    for s, K in zip(SHAPES, Ks):
        m = mask(s, "random80", K)
        items.append(dict(w=torch.from_numpy(np.array(weights(s, "dyadic"))).to(dev), mask=torch.from_numpy(np.array(m)).to(dev),
                          codes=torch.zeros(numel(s), dtype=torch.uint8, device=dev), K=K))
    t = ops.WsTable(items)
    assert t.offsets == [0, 2, 258, 274, 278] and t.cb == 534
    with no_sync():
        t.init()
        for _ in range(3):
            t.iterate()
        t.assign()
    for s, K, it, cb in zip(SHAPES, Ks, items, books(t)):
        want_c, want_codes, _ = ref_kmeans(s, "dyadic", "random80", K, 3)
        keep = R.keep_of(numel(s), mask(s, "random80", K))
        assert cb.tobytes() == want_c.tobytes() and np.array_equal(it["codes"].cpu().numpy()[keep], want_codes[keep])
