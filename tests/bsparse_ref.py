"""A numpy restatement of the block-pruning contract (include/mcamd.h), test-side only: block geometry, the
block scores in the kernel's documented summation order, the threshold / keep rule of block_prune, the mask, and the chunk
lists of a packed forward weight matrix."""
import numpy as np

FILTERS = 64      # filters per block = the N tile of the block-sparse forward


def block_kb(cin):
    """Channels per block (the channel block of the packed K axis), or None when the tensor has no block form."""
    if cin % 32 != 0:
        return None
    return 64 if cin % 64 == 0 else 32


def block_dims(cout, cin, khw):
    """(filter blocks, channel blocks, kb) of an OIHW tensor, or None when it is ineligible."""
    kb = block_kb(cin)
    if kb is None:
        return None
    return (cout + FILTERS - 1) // FILTERS, cin // kb, kb


def block_index(cout, cin, khw):
    """int64 [cout][cin][khw]: the block index (fb * ncb + cb) * khw + tap of every element."""
    nfb, ncb, kb = block_dims(cout, cin, khw)
    o = np.arange(cout)[:, None, None] // FILTERS
    c = np.arange(cin)[None, :, None] // kb
    t = np.arange(khw)[None, None, :]
    return (o * ncb + c) * khw + t


def block_scores(w, old_mask=None):
    """float64 [nfb * ncb * khw]: mean over the block of (double)(w * old_mask)^2, the product in float32, summed as the
    kernel sums: elements numbered e = r * kb + c, lane l adds e = l, l + 64, ... in ascending order, then the lane sums are
    combined by s[l] = s[l] + s[l ^ d] for d = 32, 16, 8, 4, 2, 1."""
    cout, cin = w.shape[:2]
    w = np.asarray(w, np.float32).reshape(cout, cin, -1)
    khw = w.shape[2]
    v = w if old_mask is None else w * np.asarray(old_mask, np.float32).reshape(w.shape)     # float32 product
    nfb, ncb, kb = block_dims(cout, cin, khw)
    out = np.zeros((nfb, ncb, khw), np.float64)
    for fb in range(nfb):
        rows = min(FILTERS, cout - FILTERS * fb)
        n = rows * kb
        blk = v[FILTERS * fb:FILTERS * fb + rows].reshape(rows, ncb, kb, khw).astype(np.float64)
        sq = (blk * blk).transpose(1, 3, 0, 2).reshape(ncb, khw, n)          # [cb][tap][e = r * kb + c]
        steps = (n + 63) // 64
        pad = np.zeros((ncb, khw, steps * 64), np.float64)                   # (+0.0 behind the last element changes no sum)
        pad[..., :n] = sq
        pad = pad.reshape(ncb, khw, steps, 64)
        lanes = np.zeros((ncb, khw, 64), np.float64)
        for k in range(steps):
            lanes = lanes + pad[:, :, k, :]
        idx = np.arange(64)
        for d in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[..., idx ^ d]
        out[fb] = lanes[..., 0] / np.float64(n)
    return out.reshape(-1)


def threshold(values, perc):
    return np.percentile(np.asarray(values, np.float64), perc)


def keep_flags(scores, perc, per_layer=False):
    """One int32 keep vector per layer.  A block is zeroed when its score is strictly below the threshold (the percentile
    over all layers' scores, or over the layer's own); the highest-scoring block of every layer survives, ties to the
    lowest block index."""
    glob = None if per_layer else threshold(np.concatenate(list(scores)), perc)
    keeps = []
    for s in scores:
        thr = threshold(s, perc) if per_layer else glob
        keep = np.ones(s.shape[0], np.int32)
        keep[s < thr] = 0
        best = 0
        for i in range(s.shape[0]):
            if s[i] > s[best]:
                best = i
        keep[best] = 1
        keeps.append(keep)
    return keeps


def block_mask(keep, shape, old_mask=None):
    cout, cin = shape[:2]
    khw = int(np.prod(shape[2:]))
    m = np.asarray(keep)[block_index(cout, cin, khw)].astype(np.float32).reshape(shape)
    return m if old_mask is None else m * np.asarray(old_mask, np.float32)


def block_prune(weights, perc, old_masks=None, per_layer=False):
    """Masks for a list of float32 tensors (None entries of old_masks = no mask): eligible ones (4-D, cin % 32 == 0) get
    old_mask * keep, the others their old mask or ones."""
    old_masks = old_masks or [None] * len(weights)
    elig = [w.ndim == 4 and block_kb(w.shape[1]) is not None for w in weights]
    scores = [block_scores(w, m) for w, m, e in zip(weights, old_masks, elig) if e]
    keeps = iter(keep_flags(scores, perc, per_layer) if scores else ())
    out = []
    for w, m, e in zip(weights, old_masks, elig):
        if e:
            out.append(block_mask(next(keeps), w.shape, m))
        else:
            out.append(np.ones(w.shape, np.float32) if m is None else np.asarray(m, np.float32).copy())
    return out


def pack_fwd(w, mask=None):
    """fp16 [round_up(cout, 256)][khw * cin] forward packing of an OIHW tensor with cin % 32 == 0 (include/mcamd.h):
    column kpos(t, c) = (c / kb) * khw * kb + t * kb + c % kb."""
    cout, cin = w.shape[:2]
    v = np.asarray(w, np.float32).reshape(cout, cin, -1)
    if mask is not None:
        v = v * np.asarray(mask, np.float32).reshape(v.shape)
    khw, kb = v.shape[2], block_kb(cin)
    p = v.reshape(cout, cin // kb, kb, khw).transpose(0, 1, 3, 2).reshape(cout, khw * cin).astype(np.float16)
    out = np.zeros(((cout + 255) // 256 * 256, khw * cin), np.float16)
    out[:cout] = p
    return out


def chunk_lists(packed, cout, kb):
    """(count int32[ntiles], list int32[ntiles][nchunks]) of a packed fp16 matrix: per tile of 64 rows the chunks q with
    any non-zero value (by value: -0 is zero) in columns [q kb, q kb + kb), ascending; entries behind the count are 0."""
    ntiles, nchunks = (cout + FILTERS - 1) // FILTERS, packed.shape[1] // kb
    count = np.zeros(ntiles, np.int32)
    lst = np.zeros((ntiles, nchunks), np.int32)
    for nt in range(ntiles):
        rows = packed[FILTERS * nt:FILTERS * nt + FILTERS].reshape(-1, nchunks, kb)
        nz = (rows != 0).any(axis=(0, 2))
        q = np.nonzero(nz)[0]
        count[nt] = q.shape[0]
        lst[nt, :q.shape[0]] = q
    return count, lst
