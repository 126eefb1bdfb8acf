"""Weight sharing as include/mcamd.h pins it, restated in numpy from the header alone (no package import).

Per layer, over the KEPT weights (mask != 0, or all), K = 2^bits:
  range    lo, hi = min / max of the kept fp32 weights; no kept weight: a codebook of zeros
  init     c[k] = fp32(lo + ((hi - lo) * k) / (K - 1)) in float64, in that order
  assign   code = #{j in 0..K-2 : mid[j] < w}, mid[j] = (double(c[j]) + double(c[j+1])) / 2
  update   c[k] = fp32(float64 sum of the members / count); an empty cluster keeps its centroid
  kmeans   init, `iters` rounds of assign + update, one last assign
  project  codes fixed: update, then w = c[code] on kept weights; the others are not written
  expand   w = c[code] on kept weights, +0 elsewhere
The float64 sums here run in index order from 0.0; the device adds slab by slab (MCAMD_WS_SLAB), which is another order of
the same terms: exact on dyadic inputs, within n 2^-52 sum|w| otherwise.
"""
import numpy as np

SLAB = 4096


def keep_of(n, mask):
    return np.ones(n, dtype=bool) if mask is None else (np.asarray(mask).reshape(-1) != 0)


def init(w, mask, K):
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    kept = w[keep_of(w.size, mask)]
    if kept.size == 0:
        return np.zeros(K, dtype=np.float32)
    lo, hi = float(kept.min()), float(kept.max())
    return np.array([np.float32(lo + ((hi - lo) * float(k)) / float(K - 1)) for k in range(K)], dtype=np.float32)


def midpoints(c):
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    return (c[:-1] + c[1:]) / 2.0


def assign(c, w):
    """Codes of EVERY entry of w (the caller zeroes those of weights that are not kept)."""
    mid = midpoints(c)
    w = np.asarray(w, dtype=np.float32).reshape(-1).astype(np.float64)
    return (mid[None, :] < w[:, None]).sum(axis=1).astype(np.uint8) if w.size * mid.size <= 1 << 22 else \
        np.searchsorted(mid, w, side="left").astype(np.uint8)


def sums_counts(w, codes, keep, K):
    """(float64 sums in index order from 0.0, int64 counts, float64 sums of |w|) per cluster over the kept weights."""
    w = np.asarray(w, dtype=np.float32).reshape(-1).astype(np.float64)[keep]
    codes = np.asarray(codes).reshape(-1)[keep].astype(np.int64)
    return (np.bincount(codes, weights=w, minlength=K), np.bincount(codes, minlength=K).astype(np.int64),
            np.bincount(codes, weights=np.abs(w), minlength=K))


def update(c, w, codes, keep):
    c = np.asarray(c, dtype=np.float32).copy()
    s, n, _ = sums_counts(w, codes, keep, c.size)
    for k in range(c.size):
        if n[k] > 0:
            c[k] = np.float32(s[k] / float(n[k]))
    return c


def kmeans(w, mask, K, iters, trace=None):
    """(codebook fp32 [K], codes uint8 [n] with 0 where not kept).  trace: a list that receives the codebook every assign
    of the run used (iters + 1 entries), for the tests' distance-to-midpoint precondition."""
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    keep = keep_of(w.size, mask)
    c = init(w, mask, K)
    for _ in range(iters):
        if trace is not None:
            trace.append(c.copy())
        codes = assign(c, w)
        c = update(c, w, codes, keep)
    if trace is not None:
        trace.append(c.copy())
    codes = assign(c, w)
    codes[~keep] = 0
    return c, codes


def project(w, mask, codes, c):
    """(projected weights, updated codebook); neither input is changed."""
    w = np.asarray(w, dtype=np.float32).reshape(-1).copy()
    keep = keep_of(w.size, mask)
    c = update(c, w, codes, keep)
    w[keep] = c[np.asarray(codes).reshape(-1)[keep]]
    return w, c


def expand(c, codes, mask):
    codes = np.asarray(codes).reshape(-1)
    w = np.asarray(c, dtype=np.float32)[codes]
    return np.where(keep_of(codes.size, mask), w, np.float32(0.0)).astype(np.float32)


def ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def min_midpoint_gap_ulps(w, mask, trace):
    """The smallest |w - mid| over the kept weights and every codebook of `trace`, in fp32 ulps of w."""
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    kept = w[keep_of(w.size, mask)]
    best = np.inf
    for c in trace:
        mid = midpoints(c)
        j = np.clip(np.searchsorted(mid, kept.astype(np.float64)), 0, mid.size - 1)
        d = np.minimum(np.abs(kept - mid[j]), np.abs(kept - mid[np.maximum(j - 1, 0)]))
        best = min(best, float((d / np.maximum(ulp32(kept), np.finfo(np.float32).tiny)).min())) if kept.size else best
    return best
