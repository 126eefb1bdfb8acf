"""Weight sharing: trained quantisation by k-means (an addition beyond the reference; DESIGN.md 3u, include/mcamd.h).

The stage of Deep Compression (Han, Mao and Dally) between pruning and the file: each conv layer's kept weights are
clustered into 2^bits shared values, the shared values are fine-tuned instead of the individual weights, and the file
stores a codebook plus a narrow index per kept weight.

    kmeans_share(model, bits=4, iters=ITERS, layers=None) -> codebooks
    model.set_codebooks(codebooks)            # ties the weights: weight = codebook[codes] on kept positions
    model.project_codebooks()                 # behind every optimizer.step(): each cluster back to its mean
    are_codebooks_consistent(model) -> bool   # every tied layer holds at most K distinct kept values
    model.save_compressed(path, "shared")     # compress.py

A tied model is ordinary fp32 master weights that take at most 2^bits distinct values per layer, so every engine,
precision and sparse mode runs it as it is.  A model on the GPU is clustered and projected by csrc/wshare.hip (all layers
through one table, nothing read back); a model on the CPU takes the numpy path below, the same arithmetic
(include/mcamd.h pins it; tests/wshare_ref.py restates it).
"""
import numpy as np
import torch

from . import _lib as L
from ._lib import McamdError

# The API default of `iters`.  Chosen from the numpy path on the seeded YOLOv2-VOC weights: from the linear
# initialisation Lloyd's rounds converge slowly on bell-shaped weights -- at 4 bits the relative within-cluster squared error
# is 3.7e-2 at the start, 2.3e-2 after 8 rounds, 1.7e-2 after 16 and 1.2e-2 after 32, still falling 1.4 % per round; at 8
# bits it moves by 0.1 % in all.  A round of the whole model costs about 0.5 ms (4 bits) to 4 ms (8 bits) on the device, so
# 32 rounds are cheap there and keep the numpy path of a 50 M-weight model under a minute.
ITERS = 32


# ----------------------------------------------------------------------------- the arithmetic, in numpy
def np_init(kept, K):
    """The linear initialisation over the kept fp32 weights (a flat array)."""
    if kept.size == 0:
        return np.zeros(K, dtype=np.float32)
    lo, hi = np.float64(kept.min()), np.float64(kept.max())
    k = np.arange(K, dtype=np.float64)
    return (lo + ((hi - lo) * k) / np.float64(K - 1)).astype(np.float32)


def np_assign(c, w):
    mid = (c[:-1].astype(np.float64) + c[1:].astype(np.float64)) / np.float64(2.0)
    return np.searchsorted(mid, w.astype(np.float64), side="left").astype(np.uint8)


def np_update(c, kept, codes):
    """(new codebook, float64 sums, int64 counts): members summed in index order; an empty cluster keeps its centroid."""
    K = c.size
    sums = np.bincount(codes, weights=kept.astype(np.float64), minlength=K)
    counts = np.bincount(codes, minlength=K).astype(np.int64)
    new = c.copy()
    nz = counts > 0
    new[nz] = (sums[nz] / counts[nz].astype(np.float64)).astype(c.dtype)      # fp32 (a float64 codebook stays float64)
    return new, sums, counts


def np_kmeans(w, mask, K, iters):
    """(codebook fp32 [K], codes uint8 [n], 0 where not kept) of a flat fp32 array and its flat mask (or None)."""
    keep = np.ones(w.size, dtype=bool) if mask is None else (mask != 0)
    kept = w[keep]
    c = np_init(kept, K)
    for _ in range(iters):
        c, _, _ = np_update(c, kept, np_assign(c, kept))
    codes = np.zeros(w.size, dtype=np.uint8)
    codes[keep] = np_assign(c, kept)
    return c, codes


def np_project(w, mask, codes, c):
    """In place on the flat arrays `w` and `c`: every cluster's kept members, and its codebook entry, become fp32(mean)."""
    keep = np.ones(w.size, dtype=bool) if mask is None else (mask != 0)
    kc = codes[keep]
    new, _, counts = np_update(c, w[keep], kc)
    c[:] = new
    w[keep] = c[kc]            # (an empty cluster has no member to write)


# ----------------------------------------------------------------------------- the model's layers
def _blocks(model):
    """[(conv number, MaskedConv2d)] in set_masks order; the refusals of compress.py, by name."""
    out = []
    for ind, block in enumerate(model.blocks[1:]):
        if block["type"] == "connected":
            raise McamdError("weight sharing clusters convolutional blocks only: a [connected] block is not supported")
        if block["type"] != "convolutional":
            continue
        conv = model.models[ind][0]
        if getattr(conv, "border_bias", None) is not None:
            raise McamdError("weight sharing does not support slim_export models (conv%d has a border table)" % (len(out) + 1))
        out.append((len(out) + 1, conv))
    return out


def _bits_of(bits, numbers):
    per = {}
    for i in numbers:
        b = bits.get(i) if isinstance(bits, dict) else bits
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 1 <= int(b) <= 8:
            raise McamdError("bits must be an int in 1..8, or a dict of them by conv number (conv%d: %r)" % (i, b))
        per[i] = int(b)
    return per


def _mask_of(conv):
    return conv.mask if getattr(conv, "mask_flag", False) else None


def tied_layers(model):
    """[(conv number, MaskedConv2d)] of the layers set_codebooks tied."""
    return [(i, conv) for i, conv in _blocks(model) if getattr(conv, "share_flag", False)]


def kmeans_share(model, bits=4, iters=ITERS, layers=None):
    """Cluster every chosen conv layer's kept weights into 2^bits shared values (include/mcamd.h: linear initialisation,
    `iters` Lloyd rounds, one last assignment).  Returns one entry per conv block in set_masks order: (codebook fp32 [K],
    codes uint8 of the weight's shape, 0 where the weight is not kept), or None for a layer not in `layers` (conv
    numbers; default: all).  `bits`: an int, or a dict of them by conv number.  The model is not changed: hand the result
    to model.set_codebooks."""
    convs = _blocks(model)
    if not convs:
        raise McamdError("the model has no convolutional block to share")
    numbers = [i for i, _ in convs]
    chosen = numbers if layers is None else [int(i) for i in layers]
    bad = sorted(set(chosen) - set(numbers))
    if bad:
        raise McamdError("layers names conv numbers the model does not have: %r" % bad)
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
        raise McamdError("iters must be a non-negative int (got %r)" % (iters,))
    per = _bits_of(bits, chosen)
    picked = [(i, conv) for i, conv in convs if i in per]
    out = {}
    if picked and all(conv.weight.is_cuda for _, conv in picked):
        from . import ops
        items = []
        for i, conv in picked:
            w, m = conv.weight.data, _mask_of(conv)
            if w.dtype != torch.float32:
                raise McamdError("weight sharing clusters fp32 master weights")
            items.append(dict(w=w.contiguous(), mask=m.contiguous().float() if m is not None else None,
                              codes=torch.empty(w.shape, dtype=torch.uint8, device=w.device), K=1 << per[i]))
        table = ops.WsTable(items)
        table.init()
        for _ in range(int(iters)):
            table.iterate()
        table.assign()
        for s, (i, _) in enumerate(picked):
            out[i] = (table.layer_codebook(s).clone(), items[s]["codes"])
    else:
        for i, conv in picked:
            w, m = conv.weight.data.detach().cpu().float(), _mask_of(conv)
            c, codes = np_kmeans(w.numpy().reshape(-1), None if m is None else m.detach().cpu().float().numpy().reshape(-1),
                                 1 << per[i], int(iters))
            out[i] = (torch.from_numpy(c).to(conv.weight.device), torch.from_numpy(codes).view(w.shape).to(conv.weight.device))
    return [out.get(i) for i in numbers]


# ----------------------------------------------------------------------------- Darknet.set_codebooks / project_codebooks
def expand(codebook, codes, mask):
    """codebook[codes] on kept positions, +0 elsewhere (torch, either device)."""
    w = codebook[codes.long()]
    return w if mask is None else torch.where(mask != 0, w, torch.zeros_like(w))


def set_codebooks(model, codebooks, expand_weights=True):
    convs = _blocks(model)
    if len(codebooks) != len(convs):
        raise McamdError("set_codebooks: %d entries for %d convolutional blocks" % (len(codebooks), len(convs)))
    for (i, conv), entry in zip(convs, codebooks):
        if entry is None:
            continue
        codebook, codes = entry
        K = codebook.numel()
        if codebook.dim() != 1 or K < 2 or K > 256 or K & (K - 1):
            raise McamdError("set_codebooks: conv%d: a codebook holds 2^bits entries, bits in 1..8 (got %d)" % (i, K))
        if tuple(codes.shape) != tuple(conv.weight.shape) or codes.dtype != torch.uint8:
            raise McamdError("set_codebooks: conv%d: codes must be a uint8 tensor of the weight's shape" % i)
        dev = conv.weight.device
        conv.register_buffer("codebook", codebook.detach().to(device=dev, dtype=torch.float32).contiguous().clone())
        conv.register_buffer("codes", codes.detach().to(dev).contiguous().clone())
        if expand_weights:
            conv.weight.data = expand(conv.codebook, conv.codes, _mask_of(conv)).to(conv.weight.dtype)
        conv.share_flag = True
    model._ws_table = None
    model._mark_weights_replaced()


def _device_table(model, tied):
    """The cached ops.WsTable over the tied layers.  The layers' `codebook` buffers are made views of one flat array, so one
    library call updates them all; the table is rebuilt when any tensor it names has moved (model.to, load_state_dict)."""
    from . import ops
    key = tuple((conv.weight.data_ptr(), None if _mask_of(conv) is None else conv.mask.data_ptr(), conv.codes.data_ptr(),
                 conv.codebook.data_ptr(), conv.codebook.numel()) for _, conv in tied)
    cached = getattr(model, "_ws_table", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    flat = torch.cat([conv.codebook.reshape(-1) for _, conv in tied])
    items = []
    for i, conv in tied:
        w, m = conv.weight.data, _mask_of(conv)
        if w.dtype != torch.float32 or not w.is_contiguous() or (m is not None and (m.dtype != torch.float32 or not m.is_contiguous())):
            raise McamdError("project_codebooks: conv%d: weights and masks must be contiguous fp32 tensors" % i)
        items.append(dict(w=w, mask=m, codes=conv.codes, K=conv.codebook.numel()))
    table = ops.WsTable(items, codebook=flat)
    for s, (_, conv) in enumerate(tied):
        conv._buffers["codebook"] = table.layer_codebook(s)
    key = tuple(k[:3] + (conv.codebook.data_ptr(), k[4]) for k, (_, conv) in zip(key, tied))
    model._ws_table = (key, table)
    return table


def project_codebooks(model):
    tied = tied_layers(model)
    if not tied:
        return
    if all(conv.weight.is_cuda for _, conv in tied):
        _device_table(model, tied).project()
        # The kernel wrote through raw pointers.  Bumping the version counters is what an in-place torch write would have
        # done: EVERY engine of the model compares them before its next forward and re-packs.  (Darknet._mark_weights_replaced()
        # reaches every engine too, and has each read its per-layer fp8 exponents on the host again.)  A "mixed" engine does
        # not re-read them on a version-only change; none is needed here: a mean never exceeds its largest member, so no
        # layer's largest |w| grows.
        for _, conv in tied:
            torch.autograd.graph.increment_version(conv.weight)
    else:
        for _, conv in tied:
            w = conv.weight.data.detach().cpu().float().contiguous()
            m, c = _mask_of(conv), conv.codebook.detach().cpu().clone()
            np_project(w.numpy().reshape(-1), None if m is None else m.detach().cpu().float().numpy().reshape(-1),
                       conv.codes.detach().cpu().numpy().reshape(-1), c.numpy())
            conv.weight.data.copy_(w)
            conv.codebook.copy_(c)
        model._mark_weights_replaced()


def are_codebooks_consistent(model):
    """True when every tied layer holds at most K distinct kept values (one host read per layer: an epoch-end check)."""
    for _, conv in tied_layers(model):
        w, m = conv.weight.data, _mask_of(conv)
        kept = w.reshape(-1) if m is None else w[m != 0]
        if torch.unique(kept).numel() > conv.codebook.numel():
            return False
    return True
