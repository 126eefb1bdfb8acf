"""First-order Taylor importance for pruning (an addition beyond the reference; DESIGN.md 3zb, include/mcamd.h).

Every other pruner of the package ranks by magnitude.  Here the importance of a group S of parameters is the squared change
of the loss a first-order expansion predicts for removing it, (sum over S of g w)^2, averaged over mini-batches (Molchanov
et al. 2019, arXiv:1906.10771):

    imp = TaylorImportance(model)                       # accumulators allocated once
    for batch in some batches:
        loss(model(x)).backward()
        imp.accumulate()                                # ONE launch for all layers; no optimizer.step() needed
    masks = taylor_prune(model, 60, imp, "filter")      # "weight" | "block" | "filter": ordinary masks
    model.set_masks(masks)

A group is one weight, one block of block_prune (64 filters x kb channels x one tap) or one filter.  A filter that is followed
by BatchNorm on batch statistics is scored through the BatchNorm gate, (gamma dgamma + beta dbeta)^2: the loss does not
change when such a filter is rescaled, so the sum of g w over its own weights is zero up to rounding (Euler's theorem).  A
conv without BatchNorm (the last one) is scored by its weights plus its bias.

A model on the GPU is accumulated by csrc/taylor.hip; CPU tensors take the torch restatement below, the same arithmetic
operation by operation (include/mcamd.h pins it; tests/taylor_ref.py restates it in numpy).
"""
import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from ._lib import McamdError

BLOCK_FILTERS = 64
GRANULARITIES = ("weight", "block", "filter")


def _block_kb(cin):
    return 64 if cin % 64 == 0 else 32


def _nblocks(cout, cin, khw):
    return ((cout + BLOCK_FILTERS - 1) // BLOCK_FILTERS) * (cin // _block_kb(cin)) * khw


# ----------------------------------------------------------------------------- the arithmetic, in torch (CPU tensors)
_LANES = torch.arange(64)


def _lane_sum(x):
    """x float64 [..., n] -> [...]: lane l adds elements l, l + 64, ... in ascending order starting from 0.0, then the lane sums
    are combined by s[l] += s[l ^ d], d = 32 ... 1 (a +0.0 behind the last element changes no sum)."""
    n = x.shape[-1]
    steps = (n + 63) // 64
    pad = torch.zeros(x.shape[:-1] + (steps * 64,), dtype=torch.float64)
    pad[..., :n] = x
    pad = pad.view(x.shape[:-1] + (steps, 64))
    s = torch.zeros(x.shape[:-1] + (64,), dtype=torch.float64)
    for j in range(steps):
        s = s + pad[..., j, :]
    for d in (32, 16, 8, 4, 2, 1):
        s = s + s[..., _LANES ^ d]
    return s[..., 0]


def torch_conv_step(w, g, bias=None, gbias=None, acc_w=None, acc_b=None, acc_f=None):
    """One step of a conv segment on CPU tensors, in place on the accumulators that are given."""
    cout = w.shape[0]
    cin = w.shape[1] if w.dim() > 1 else 1
    p = (g.detach().float() * w.detach().float()).reshape(cout, cin, -1)          # fp32 product
    khw = p.shape[2]
    if acc_w is not None:
        acc_w.add_((p * p).view(acc_w.shape))
    if acc_b is not None:
        kb = _block_kb(cin)
        nfb, ncb = (cout + BLOCK_FILTERS - 1) // BLOCK_FILTERS, cin // kb
        S = torch.zeros(nfb, ncb, khw, dtype=torch.float64)
        for fb in range(nfb):
            rows = min(BLOCK_FILTERS, cout - BLOCK_FILTERS * fb)
            blk = p[BLOCK_FILTERS * fb:BLOCK_FILTERS * fb + rows].double().view(rows, ncb, kb, khw)
            S[fb] = _lane_sum(blk.permute(1, 3, 0, 2).reshape(ncb, khw, rows * kb))          # [cb][tap][e = r kb + c]
        acc_b.add_((S * S).view(-1))
    if acc_f is not None:
        S = _lane_sum(p.double().reshape(cout, cin * khw))
        if bias is not None:
            S = S + (gbias.detach().float() * bias.detach().float()).double()
        acc_f.add_(S * S)


def torch_gate_step(gamma, dgamma, beta, dbeta, acc_f):
    t = gamma.detach().double() * dgamma.detach().double() + beta.detach().double() * dbeta.detach().double()
    acc_f.add_(t * t)


# ----------------------------------------------------------------------------- the accumulators of a model
class TaylorImportance:
    """The Taylor-importance accumulators of `model`, one set per `p.dim() != 1` parameter in model.parameters() order:

      weight   fp32, the parameter's shape          sum over steps of (g w)^2            (203 MB for YOLOv2-VOC)
      block    float64 [blocks], cin % 32 == 0 only  sum over steps of (sum over the block of g w)^2, block_prune's blocks
      filter   float64 [cout], 4-D parameters        sum over steps of the filter's term: through the BatchNorm gate when a
                                                     BatchNorm follows the conv inside its Sequential, else weights + bias

    accumulate() adds one step's term: call it after backward() and before optimizer.step() (which changes w).  On the GPU
    it is one launch over a table built once (rebuilt when a tensor it names has moved), with no allocation and no host
    synchronisation."""

    def __init__(self, model, weight=True, block=True, filter=True):
        self.model = model
        self.params = [p for p in model.parameters() if p.dim() != 1]
        if not self.params:
            raise McamdError("TaylorImportance: the model has no parameter to score")
        dev = self.params[0].device
        conv_of, bn_of = {}, {}
        for m in model.modules():
            if isinstance(m, nn.Conv2d):
                conv_of[id(m.weight)] = m
            if isinstance(m, nn.Sequential):
                kids = list(m.children())
                for a, b in zip(kids, kids[1:]):
                    if isinstance(a, nn.Conv2d) and isinstance(b, nn.BatchNorm2d):
                        bn_of[id(a.weight)] = b
        self.layers = []
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev:
                raise McamdError("TaylorImportance scores fp32 parameters on one device")
            cout, cin = p.shape[0], p.shape[1]
            khw = p.numel() // (cout * cin)
            conv, bn = conv_of.get(id(p)), bn_of.get(id(p))
            if bn is not None and (bn.weight is None or bn.bias is None):
                bn = None                                   # no affine gate to score through
            lay = dict(p=p, conv=conv, bn=bn, acc_w=None, acc_b=None, acc_f=None)
            if weight:
                lay["acc_w"] = torch.zeros_like(p.data, memory_format=torch.contiguous_format)
            if block and p.dim() == 4 and cin % 32 == 0:
                lay["acc_b"] = torch.zeros(_nblocks(cout, cin, khw), dtype=torch.float64, device=dev)
            if filter and p.dim() == 4:
                lay["acc_f"] = torch.zeros(cout, dtype=torch.float64, device=dev)
            self.layers.append(lay)
        self._steps = torch.zeros(1, dtype=torch.int32, device=dev)
        self._table, self._key = None, None
        self.tables_built = 0
        if not any(a is not None for lay in self.layers for a in (lay["acc_w"], lay["acc_b"], lay["acc_f"])):
            raise McamdError("TaylorImportance: nothing to accumulate (weight, block and filter are all off)")

    # ---- the segments
    @staticmethod
    def _grad(t, what):
        if t.grad is None:
            raise McamdError("TaylorImportance.accumulate: %s has no gradient; call it after backward()" % what)
        return t.grad

    def _segments(self):
        """[dict] in table order: per parameter its conv segment (when it has an output), then its gate segment."""
        segs = []
        for i, lay in enumerate(self.layers):
            p, conv, bn = lay["p"], lay["conv"], lay["bn"]
            own_f = lay["acc_f"] if bn is None else None
            if lay["acc_w"] is not None or lay["acc_b"] is not None or own_f is not None:
                s = dict(w=p.data, g=self._grad(p, "parameter %d" % i), acc_w=lay["acc_w"], acc_b=lay["acc_b"], acc_f=own_f)
                if own_f is not None and conv is not None and conv.bias is not None:
                    s["bias"], s["gbias"] = conv.bias.data, self._grad(conv.bias, "the bias of parameter %d" % i)
                segs.append(s)
            if bn is not None and lay["acc_f"] is not None:
                segs.append(dict(gate=True, w=bn.weight.data, g=self._grad(bn.weight, "a BatchNorm weight"), bias=bn.bias.data,
                                 gbias=self._grad(bn.bias, "a BatchNorm bias"), acc_f=lay["acc_f"]))
        return segs

    def accumulate(self, skip=None):
        """Add this step's term to every accumulator and 1 to the step count; nothing at all when `skip` (a one-element fp32
        tensor on the model's device, e.g. train.StepGuard.found) is non-zero."""
        segs = self._segments()
        if not self._steps.is_cuda:
            if skip is not None and float(skip.reshape(-1)[0]) != 0.0:
                return
            for s in segs:
                if s.get("gate"):
                    torch_gate_step(s["w"], s["g"], s["bias"], s["gbias"], s["acc_f"])
                else:
                    torch_conv_step(s["w"], s["g"], s.get("bias"), s.get("gbias"), s["acc_w"], s["acc_b"], s["acc_f"])
            self._steps += 1
            return
        from . import ops
        key = tuple(t.data_ptr() for s in segs for t in (s["w"], s["g"], s.get("bias"), s.get("gbias")) if t is not None)
        if self._table is None or key != self._key:
            for s in segs:
                for name in ("w", "g", "bias", "gbias"):
                    t = s.get(name)
                    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                        raise McamdError("TaylorImportance.accumulate: weights and gradients must be contiguous fp32 tensors")
            self._table, self._key = ops.TaylorTable(segs, self._steps), key
            self.tables_built += 1
        self._table.accumulate(skip)

    # ---- reading
    def steps(self):
        """Steps accumulated so far (one host read of the device counter)."""
        return int(self._steps.item())

    def reset(self):
        self._steps.zero_()
        for lay in self.layers:
            for name in ("acc_w", "acc_b", "acc_f"):
                if lay[name] is not None:
                    lay[name].zero_()

    def weight_scores(self):
        return [lay["acc_w"] for lay in self.layers]

    def block_scores(self):
        return [lay["acc_b"] for lay in self.layers]

    def filter_scores(self):
        return [lay["acc_f"] for lay in self.layers]

    def all_reduce(self):
        """Under torch.distributed with more than one rank: every accumulator and the step count become their sums over
        the ranks (each rank scored its own shard of the batches)."""
        if not (dist.is_initialized() and dist.get_world_size() > 1):
            return
        for lay in self.layers:
            for name in ("acc_w", "acc_b", "acc_f"):
                if lay[name] is not None:
                    dist.all_reduce(lay[name])
        dist.all_reduce(self._steps)


# ----------------------------------------------------------------------------- masks
def _old_masks(model, ps):
    owner = {}
    for mod in model.modules():
        if getattr(mod, "mask_flag", False) and hasattr(mod, "weight"):
            owner[id(mod.weight)] = mod.mask
    olds = []
    for p in ps:
        old = owner.get(id(p))
        olds.append(old.contiguous() if old is not None and old.shape == p.shape else None)
    return olds


def _kth_pair(tensors, k):
    """(s[k], s[min(k + 1, n - 1)]) of the ascending |score| over all tensors, as float32 numpy scalars."""
    if tensors[0].is_cuda:
        from . import ops
        return ops.kth_magnitude(tensors, k).cpu().numpy()
    s = torch.sort(torch.cat([t.reshape(-1).abs() for t in tensors])).values
    return s[[k, min(k + 1, s.numel() - 1)]].numpy()


def _weight_masks(scores, perc):
    from .pruning.weightPruning.methods import _virtual_index, _lerp
    n = sum(s.numel() for s in scores)
    k, gamma, above = _virtual_index(n, perc, np.float32)
    if above:
        k = n - 1
    pair = _kth_pair(scores, k)
    threshold = np.float32(pair[1]) if above else _lerp(np.float32(pair[0]), np.float32(pair[1]), gamma)
    if scores[0].is_cuda:
        from . import ops
        thr = torch.tensor([float(threshold)], dtype=torch.float32, device=scores[0].device)
        return [ops.magnitude_mask(s, thr) for s in scores]
    return [(s.abs() > float(threshold)).to(torch.float32) for s in scores]


def _block_mask(keep, shape, old):
    """old (ones when None) with the blocks whose keep flag is 0 zeroed; keep: int32 tensor on the parameter's device."""
    if keep.is_cuda:
        from . import ops
        return ops.block_mask(keep.contiguous(), tuple(shape), old)
    cout, cin = shape[0], shape[1]
    khw = int(np.prod(shape[2:]))
    kb = _block_kb(cin)
    o = torch.arange(cout).view(-1, 1, 1) // BLOCK_FILTERS
    c = torch.arange(cin).view(1, -1, 1) // kb
    t = torch.arange(khw).view(1, 1, -1)
    flags = keep[((o * (cin // kb) + c) * khw + t).reshape(-1)].view(tuple(shape)) != 0
    base = old.to(torch.float32) if old is not None else torch.ones(tuple(shape), dtype=torch.float32)
    return torch.where(flags, base, torch.zeros_like(base))


def _filter_mask(keep, shape):
    if keep.is_cuda:
        from . import ops
        return ops.filter_mask(keep.contiguous(), tuple(shape))
    return (keep != 0).to(torch.float32).view(-1, *([1] * (len(shape) - 1))).expand(tuple(shape)).contiguous()


def filter_keep(scores, pruning_perc, per_layer=False):
    """Keep flags (int32, one array per layer) from the layers' float64 filter scores: each layer's scores are divided by
    the layer's sqrt(sum s^2) (a layer whose sum is 0 stays as it is), a filter goes when its normalised score is strictly
    below the `pruning_perc` percentile of all of them (of its own layer's with per_layer); the highest-scoring filter of
    every layer stays whatever the threshold, ties to the lowest index."""
    from .pruning.weightPruning.methods import _percentile_f64
    normed = []
    for s in scores:
        s = np.asarray(s, np.float64)
        norm = np.sqrt(np.square(s).sum())
        normed.append(s / norm if norm != 0 else s.copy())
    allv = np.concatenate([np.zeros(0, np.float64)] + normed)
    if not per_layer and allv.shape[0]:
        threshold = _percentile_f64(allv, pruning_perc)
    keeps = []
    for s in normed:
        if per_layer:
            threshold = _percentile_f64(s, pruning_perc)
        keep = (~(s < threshold)).astype(np.int32)
        keep[int(np.argmax(s))] = 1           # (argmax: the first of equal maxima)
        keeps.append(keep)
    return keeps


def taylor_prune(model, pruning_perc, importance, granularity, per_layer=False):
    '''
    Taylor-importance pruning (Molchanov et al. 2019, arXiv:1906.10771) -- an addition beyond the reference.  Same calling
    convention as weight_prune / block_prune: one mask per `p.dim() != 1` parameter in model.parameters() order, applied by
    the caller with model.set_masks(masks).  `importance` is the TaylorImportance of this model after at least one
    accumulate(); scores are accumulator / steps.

      "weight"  weight_prune's arithmetic on the weight scores in place of the weights: the float32 percentile of all scores
                (per_layer: of the layer's own), mask = score > threshold, so ties are pruned and a weight that is already
                masked (w = 0, score 0) stays pruned.
      "block"   block_prune's rule on the block scores: the RAW group importance, not divided by the block's size (a ragged
                block has fewer terms and is not compensated); mask = old_mask * keep, every layer keeps its best block;
                parameters without a block form (conv1: 3 input channels) keep their old mask, or all ones.
      "filter"  each 4-D parameter's filter scores divided by the layer's L2 norm, the float64 percentile over all of them,
                filters strictly below it are zeroed, every layer keeps its best filter (filter_keep); the masks are
                ops.filter_mask's, what quick_filter_prune hands to filter compaction and slim_export.
    '''
    if granularity not in GRANULARITIES:
        raise McamdError("taylor_prune: granularity must be one of %r (got %r)" % (GRANULARITIES, granularity))
    if not isinstance(importance, TaylorImportance):
        raise McamdError("taylor_prune: importance must be a TaylorImportance")
    ps = [p for p in model.parameters() if p.dim() != 1]
    if len(ps) != len(importance.params) or any(a is not b for a, b in zip(ps, importance.params)):
        raise McamdError("taylor_prune: the importance was accumulated on another model")
    steps = importance.steps()
    if steps == 0:
        raise McamdError("taylor_prune: no step has been accumulated (TaylorImportance.accumulate after backward())")
    dev = ps[0].device
    olds = _old_masks(model, ps)
    if granularity == "weight":
        scores = importance.weight_scores()
        if any(s is None for s in scores):
            raise McamdError('taylor_prune: "weight" needs TaylorImportance(weight=True)')
        # (the accumulators themselves: dividing 50 M scores by `steps` would change no order worth a 203 MB temporary)
        if per_layer:
            return [_weight_masks([s], pruning_perc)[0] for s in scores]
        return _weight_masks(scores, pruning_perc)
    if granularity == "block":
        elig = [p.dim() == 4 and p.shape[1] % 32 == 0 for p in ps]
        accs = [a for a, e in zip(importance.block_scores(), elig) if e]
        if any(a is None for a in accs):
            raise McamdError('taylor_prune: "block" needs TaylorImportance(block=True)')
        from .pruning.weightPruning.methods import _block_keep
        keeps = iter(())
        if accs:
            sizes = [a.numel() for a in accs]
            host = np.split(torch.cat(accs).cpu().numpy() / np.float64(steps), np.cumsum(sizes)[:-1])
            keep_all = torch.from_numpy(np.concatenate(_block_keep(host, pruning_perc, per_layer))).to(dev)
            keeps = iter(torch.split(keep_all, sizes))
        masks = []
        for p, old, e in zip(ps, olds, elig):
            if e:
                masks.append(_block_mask(next(keeps), tuple(p.shape), old))
            else:
                masks.append(old.clone() if old is not None else torch.ones_like(p.data))
        return masks
    four = [p.dim() == 4 for p in ps]
    accs = [a for a, f in zip(importance.filter_scores(), four) if f]
    if any(a is None for a in accs):
        raise McamdError('taylor_prune: "filter" needs TaylorImportance(filter=True)')
    keeps = iter(())
    if accs:
        sizes = [a.numel() for a in accs]
        host = np.split(torch.cat(accs).cpu().numpy() / np.float64(steps), np.cumsum(sizes)[:-1])
        keep_all = torch.from_numpy(np.concatenate(filter_keep(host, pruning_perc, per_layer))).to(dev)
        keeps = iter(torch.split(keep_all, sizes))
    masks = []
    for p, old, f in zip(ps, olds, four):
        if f:
            masks.append(_filter_mask(next(keeps), tuple(p.shape)))
        else:
            masks.append(old.clone() if old is not None else torch.ones_like(p.data))
    return masks
