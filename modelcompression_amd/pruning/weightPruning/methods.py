"""Mirror of the reference's src/pruning/weightPruning/methods.py: weight_prune,
quick_filter_prune, prune_one_filter, filter_prune -- same signatures, masks bit-identical.

The 50.6 M-element scans run in HIP (mcamd_kth_magnitude, mcamd_magnitude_mask,
mcamd_filter_scores); the host only does the scalar percentile bookkeeping of
`np.percentile` (float32 virtual index for weight_prune, float64 interpolation over the
10 461 filter scores for quick_filter_prune).  Parameters must live on the GPU.
"""
import math

import numpy as np
import torch

from ... import ops
from ..._lib import McamdError
from .utils import prune_rate, arg_nonzero_min
from ...share import kmeans_share  # noqa: F401  (the stage behind pruning: weight sharing, share.py)
from ...importance import taylor_prune  # noqa: F401  (ranking by first-order Taylor importance, importance.py)
from ...sparsify import GroupLasso  # noqa: F401  (block and filter sparsity learned while training, sparsify.py)


def _virtual_index(n, perc, ftype):
    """np.percentile's index arithmetic for a `ftype` array (numpy 2.x): q = perc/100 in
    ftype, v = ftype(n-1) * q, k = floor(v), gamma = v - k (reference call sites
    methods.py:18 and :55)."""
    q = ftype(perc) / ftype(100)
    v = ftype(n - 1) * q
    k = int(math.floor(float(v)))
    return k, ftype(v - ftype(k)), bool(v >= ftype(n - 1))


def _lerp(a, b, t):
    ft = type(a)
    d = ft(b - a)
    if t >= ft(0.5):
        return ft(b - ft(d * ft(ft(1) - t)))
    return ft(a + ft(d * t))


def _prunable(model):
    ps = [p for p in model.parameters() if p.dim() != 1]
    for p in ps:
        if not p.is_cuda:
            raise McamdError("pruning needs the model on the GPU (model.cuda()); there is no CPU path")
    return ps


def weight_prune(model, pruning_perc):
    '''
    Prune pruning_perc% weights globally (not layer-wise)
    arXiv: 1606.09274                                     (reference methods.py:9-26)
    '''
    ps = _prunable(model)
    ws = [p.data.contiguous() for p in ps]
    n = sum(w.numel() for w in ws)
    k, gamma, above = _virtual_index(n, pruning_perc, np.float32)
    if above:
        k = n - 1
    pair = ops.kth_magnitude(ws, k).cpu().numpy()          # s[k], s[k+1]
    threshold = np.float32(pair[1]) if above else _lerp(np.float32(pair[0]), np.float32(pair[1]), gamma)
    thr = torch.tensor([float(threshold)], dtype=torch.float32, device=ws[0].device)
    return [ops.magnitude_mask(w, thr) for w in ws]


def nm_prune(model, n=2, m=4):
    '''
    N:M structured magnitude pruning -- an addition beyond the reference (which has only weight_prune and the filter
    methods).  Same calling convention as weight_prune: one mask per `p.dim() != 1` parameter in model.parameters()
    order, applied by the caller with model.set_masks(masks).  For a conv weight [O, I, kh, kw] with I % m == 0, every
    group of m consecutive input channels at a fixed (o, tap) keeps its n entries of largest |w * old_mask| (ties: the
    lower channel), old_mask being the layer's current mask (kept entries keep its value: composes with weight_prune)
    or all ones; other parameters (conv1: 3 input channels) get their old mask unchanged, or all ones.  The 2:4 pattern
    is what v_smfmac runs at twice the dense rate (Darknet.sparse = "2:4").  Only n=2, m=4.
    '''
    if (n, m) != (2, 4):
        raise McamdError("nm_prune supports the 2:4 pattern only (got %s:%s)" % (n, m))
    ps = _prunable(model)
    owner = {}
    for mod in model.modules():
        if getattr(mod, "mask_flag", False) and hasattr(mod, "weight"):
            owner[id(mod.weight)] = mod.mask
    masks = []
    for p in ps:
        old = owner.get(id(p))
        old = old.contiguous() if old is not None and old.shape == p.shape else None
        if p.dim() == 4 and p.shape[1] % m == 0:
            masks.append(ops.nm_mask(p.data.contiguous(), old, n, m))
        else:
            masks.append(old.clone() if old is not None else torch.ones_like(p.data))
    return masks


def _layer_scores(p):
    return ops.filter_scores(p.data.contiguous())


def _percentile_f64(values, perc):
    """np.percentile(values, perc) for a float64 vector (method 'linear')."""
    n = values.shape[0]
    k, gamma, above = _virtual_index(n, perc, np.float64)
    s = np.sort(values)
    if above:
        return np.float64(s[-1])
    return _lerp(np.float64(s[k]), np.float64(s[k + 1]), gamma)


def _block_keep(scores, pruning_perc, per_layer=False):
    """Keep flags (int32, one array per layer) from the layers' float64 block scores: a block goes when its score is
    strictly below the `pruning_perc` percentile of all scores (of its own layer's with per_layer); the highest-scoring
    block of every layer stays whatever the threshold, ties to the lowest block index."""
    allv = np.concatenate([np.zeros(0, np.float64)] + list(scores))
    if not per_layer and allv.shape[0]:
        threshold = _percentile_f64(allv, pruning_perc)
    keeps = []
    for s in scores:
        if per_layer:
            threshold = _percentile_f64(s, pruning_perc)
        keep = (~(s < threshold)).astype(np.int32)
        keep[int(np.argmax(s))] = 1           # (argmax: the first of equal maxima)
        keeps.append(keep)
    return keeps


def block_prune(model, pruning_perc, per_layer=False):
    '''
    Block magnitude pruning (Narang et al. 2017, arXiv:1711.02782; Mao et al. 2017, arXiv:1705.08922) -- an addition
    beyond the reference.  Same calling convention as weight_prune / nm_prune: one mask per `p.dim() != 1` parameter in
    model.parameters() order, applied by the caller with model.set_masks(masks).  For a conv weight [O, I, kh, kw] with
    I % 32 == 0 a block is filters [64 f, min(64 f + 64, O)) x input channels [kb c, kb c + kb) at one tap, kb = 64 when
    I % 64 == 0 else 32: one K chunk of one 64-filter tile of the forward kernels, so Darknet.sparse = "block" skips it.
    A block's score is the float64 mean of (w * old_mask)^2 (mcamd_block_scores: fixed summation order), old_mask being
    the layer's current mask or all ones; blocks scoring strictly below the pruning_perc percentile of all eligible blocks
    of the model (per_layer=True: of their own layer) are zeroed, except that every layer keeps its highest-scoring block
    (ties: the lowest block index).  mask = old_mask * keep, so the method composes with weight_prune / nm_prune.  Other
    parameters (conv1: 3 input channels) get their old mask unchanged, or all ones.
    '''
    ps = _prunable(model)
    owner = {}
    for mod in model.modules():
        if getattr(mod, "mask_flag", False) and hasattr(mod, "weight"):
            owner[id(mod.weight)] = mod.mask
    olds, elig = [], []
    for p in ps:
        old = owner.get(id(p))
        olds.append(old.contiguous() if old is not None and old.shape == p.shape else None)
        elig.append(p.dim() == 4 and p.shape[1] % 32 == 0)
    scores = [ops.block_scores(p.data.contiguous(), old) for p, old, e in zip(ps, olds, elig) if e]
    keeps = iter(())
    if scores:
        # one device->host read of all scores (12 367 for YOLOv2-VOC), one host->device write of the keep flags
        sizes = [s.numel() for s in scores]
        host = np.split(torch.cat(scores).cpu().numpy(), np.cumsum(sizes)[:-1])
        keep_all = torch.from_numpy(np.concatenate(_block_keep(host, pruning_perc, per_layer))).to(ps[0].device)
        keeps = iter(torch.split(keep_all, sizes))
    masks = []
    for p, old, e in zip(ps, olds, elig):
        if e:
            masks.append(ops.block_mask(next(keeps).contiguous(), tuple(p.shape), old))
        else:
            masks.append(old.clone() if old is not None else torch.ones_like(p.data))
    return masks


def quick_filter_prune(model, pruning_perc):
    '''
    Prune pruning_perc% filters globally                   (reference methods.py:28-78)
    '''
    convs = [p for p in model.parameters() if p.dim() == 4]
    for p in convs:
        if not p.is_cuda:
            raise McamdError("pruning needs the model on the GPU (model.cuda()); there is no CPU path")
    scores = [_layer_scores(p) for p in convs]
    # one device->host read of all 10 461 scores, one host->device write of the keep flags (the reference moves every
    # weight tensor to the host twice, methods.py:37-72)
    values32 = torch.cat(scores).cpu().numpy()
    values = np.concatenate([np.zeros(0, np.float64), values32.astype(np.float64)])
    threshold = _percentile_f64(values, pruning_perc)
    keep_all = torch.from_numpy((~(values < threshold)).astype(np.int32)).to(convs[0].device)
    masks, off = [], 0
    for p in convs:
        masks.append(ops.filter_mask(keep_all[off:off + p.shape[0]], tuple(p.shape)))
        off += p.shape[0]
    return masks


def prune_one_filter(model, masks):
    '''
    Pruning one least ``important'' feature map by the scaled l2norm of
    kernel weights.  arXiv:1611.06440                      (reference methods.py:81-125)
    '''
    NO_MASKS = False
    if not masks:
        masks = []
        NO_MASKS = True
    values = []
    for p in model.parameters():
        if p.dim() == 4:
            if not p.is_cuda:
                raise McamdError("pruning needs the model on the GPU (model.cuda()); there is no CPU path")
            if NO_MASKS:
                masks.append(torch.ones_like(p.data))
            # scaled mean-square normalised by the layer's L2 norm; no /max step in this variant
            v = _scores_without_max(p)
            min_value, min_ind = arg_nonzero_min(list(v))
            values.append([min_value, min_ind])
    assert len(masks) == len(values), "something wrong here"
    values = np.array(values)
    to_prune_layer_ind = np.argmin(values[:, 0])
    to_prune_filter_ind = int(values[to_prune_layer_ind, 1])
    masks[to_prune_layer_ind][to_prune_filter_ind] = 0.
    print('Prune filter #{} in layer #{}'.format(to_prune_filter_ind, to_prune_layer_ind))
    return masks


def _scores_without_max(p):
    """mean square / L2 norm of the layer (methods.py:104-109), fp32 in numpy's order.
    The per-filter mean squares come from the HIP kernel; the O(cout) normalisation is
    finished on the host with the same pairwise sum numpy uses."""
    ms = ops.filter_mean_square(p.data.contiguous()).cpu().numpy()
    norm = np.sqrt(np.square(ms).sum())
    return ms / norm


def filter_prune(model, pruning_perc):
    '''
    Prune filters one by one until reach pruning_perc      (reference methods.py:128-142)
    (not iterative pruning)

    Note: on a Darknet the reference's loop never terminates -- its prune_one_filter builds
    numpy masks, MaskedConv2d.set_mask's register_buffer rejects them and Darknet.set_masks
    swallows the error (nets.py:1059-1060), so prune_rate never moves.  Here the masks are
    tensors, set_masks applies them, and the loop ends as the docstring intends.
    '''
    masks = []
    current_pruning_perc = 0.
    while current_pruning_perc < pruning_perc:
        masks = prune_one_filter(model, masks)
        model.set_masks(masks)
        current_pruning_perc = prune_rate(model, verbose=False)
        print('{:.2f} pruned'.format(current_pruning_perc))
    return masks
