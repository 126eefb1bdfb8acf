"""A numpy restatement of the Taylor-importance contract (include/mcamd.h), test-side only: one step of a conv
segment and of a gate segment in the documented arithmetic and summation order, and the three mask rules of taylor_prune.
Block geometry and the block mask come from bsparse_ref (the contract is mcamd_block_scores')."""
import numpy as np

import bsparse_ref as B


def wave_sum(x):
    """float64 [..., n] -> [...]: lane l adds elements l, l + 64, ... in ascending order starting from 0.0; the 64 lane sums are
    combined by s[l] = s[l] + s[l ^ d] for d = 32, 16, 8, 4, 2, 1."""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    lanes = np.zeros(x.shape[:-1] + (64,), np.float64)
    for first in range(0, n, 64):
        part = x[..., first:first + 64]
        lanes[..., :part.shape[-1]] = lanes[..., :part.shape[-1]] + part
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., idx ^ d]
    return lanes[..., 0]


def products(w, g):
    """p = g * w rounded to float32, as [cout][cin][khw]."""
    w = np.asarray(w, np.float32)
    cout = w.shape[0]
    cin = w.shape[1] if w.ndim > 1 else 1
    p = np.asarray(g, np.float32).reshape(w.shape) * w
    assert p.dtype == np.float32
    return p.reshape(cout, cin, -1)


def weight_term(w, g):
    """float32, the weight's shape: p * p rounded to float32 (the caller adds it to acc_w in float32)."""
    p = products(w, g)
    t = p * p
    assert t.dtype == np.float32
    return t.reshape(np.asarray(w).shape)


def block_sums(w, g):
    """float64 [nfb * ncb * khw]: S_b."""
    p = products(w, g)
    cout, cin, khw = p.shape
    nfb, ncb, kb = B.block_dims(cout, cin, khw)
    out = np.zeros((nfb, ncb, khw), np.float64)
    for fb in range(nfb):
        rows = min(B.FILTERS, cout - B.FILTERS * fb)
        for cb in range(ncb):
            blk = p[B.FILTERS * fb:B.FILTERS * fb + rows, kb * cb:kb * cb + kb, :].astype(np.float64)     # [r][c][tap]
            out[fb, cb] = wave_sum(blk.transpose(2, 0, 1).reshape(khw, rows * kb))                        # e = r * kb + c
    return out.reshape(-1)


def filter_sums(w, g, bias=None, gbias=None):
    """float64 [cout]: S_f, elements in memory order, the bias product (float32) added last."""
    p = products(w, g)
    S = wave_sum(p.reshape(p.shape[0], -1).astype(np.float64))
    if bias is not None:
        pb = np.asarray(gbias, np.float32) * np.asarray(bias, np.float32)
        assert pb.dtype == np.float32
        S = S + pb.astype(np.float64)
    return S


def gate_sums(gamma, dgamma, beta, dbeta):
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return f(gamma) * f(dgamma) + f(beta) * f(dbeta)


def conv_step(w, g, bias=None, gbias=None, acc_w=None, acc_b=None, acc_f=None):
    """One step in place on the accumulators given (numpy arrays: acc_w float32, acc_b / acc_f float64)."""
    if acc_w is not None:
        assert acc_w.dtype == np.float32
        acc_w += weight_term(w, g)
    if acc_b is not None:
        S = block_sums(w, g)
        acc_b += S * S
    if acc_f is not None:
        S = filter_sums(w, g, bias, gbias)
        acc_f += S * S


def gate_step(gamma, dgamma, beta, dbeta, acc_f):
    t = gate_sums(gamma, dgamma, beta, dbeta)
    acc_f += t * t


# ----------------------------------------------------------------------------- masks
def weight_masks(scores, perc, per_layer=False):
    """float32 percentile of all scores (numpy's own, on a float32 array); mask = score > threshold."""
    scores = [np.asarray(s, np.float32) for s in scores]
    if per_layer:
        return [(s > np.percentile(s.reshape(-1), perc)).astype(np.float32) for s in scores]
    thr = np.percentile(np.concatenate([s.reshape(-1) for s in scores]), perc)
    assert thr.dtype == np.float32
    return [(s > thr).astype(np.float32) for s in scores]


def block_masks(shapes, acc_b, steps, perc, old_masks=None, per_layer=False):
    """shapes: every prunable parameter's; acc_b: one float64 array per parameter (None where ineligible)."""
    old_masks = old_masks or [None] * len(shapes)
    elig = [len(s) == 4 and B.block_kb(s[1]) is not None for s in shapes]
    scores = [np.asarray(a, np.float64) / np.float64(steps) for a, e in zip(acc_b, elig) if e]
    keeps = iter(B.keep_flags(scores, perc, per_layer) if scores else ())
    out = []
    for s, m, e in zip(shapes, old_masks, elig):
        if e:
            out.append(B.block_mask(next(keeps), s, m))
        else:
            out.append(np.ones(s, np.float32) if m is None else np.asarray(m, np.float32).copy())
    return out


def filter_masks(shapes, acc_f, steps, perc, per_layer=False):
    """4-D parameters only: normalise per layer by sqrt(sum s^2) (unless 0), float64 percentile over all, zero what is strictly
    below, keep every layer's best filter (the first of equal maxima)."""
    normed = []
    for a in acc_f:
        s = np.asarray(a, np.float64) / np.float64(steps)
        norm = np.sqrt(np.square(s).sum())
        normed.append(s / norm if norm != 0 else s)
    glob = None if per_layer else np.percentile(np.concatenate(normed), perc)
    out = []
    for shape, s in zip(shapes, normed):
        thr = np.percentile(s, perc) if per_layer else glob
        keep = np.ones(s.shape[0], np.float32)
        keep[s < thr] = 0
        best = 0
        for i in range(s.shape[0]):
            if s[i] > s[best]:
                best = i
        keep[best] = 1
        out.append(np.broadcast_to(keep.reshape(-1, *([1] * (len(shape) - 1))), shape).copy())
    return out
