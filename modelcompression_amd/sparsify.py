"""Structured sparsity learned while training: proximal group lasso (an addition beyond the reference; DESIGN.md 3ze,
include/mcamd.h).

Every pruner of the package ranks a finished network once and cuts it.  Here a group-lasso penalty is applied as a proximal
step behind the optimizer (Wen et al. 2016, arXiv:1608.03665, for weight groups; Liu et al. 2017, arXiv:1708.06519, for
BatchNorm gates), so the groups the loss does not need shrink to exactly zero over the steps and the cut that follows removes
only what is already zero:

    gl = GroupLasso(model, lam=1e-2, granularity="block")     # or "filter"
    for batch in batches:
        loss(model(x)).backward()
        optimizer.step()
        gl.step(optimizer.param_groups[0]["lr"])              # ONE launch for all layers
    model.set_masks(gl.masks())                               # ordinary masks: every engine, .mcz payload and sparse_train

  "block"   the groups are block_prune's blocks (64 filters x kb channels x one tap) of every 4-D parameter with
            cin % 32 == 0, the last conv included: w_g <- w_g * max(0, 1 - lr lam sqrt(n_g) / ||w_g||), the proximal operator
            of lam * sqrt(n_g) * ||w_g|| at step lr.
  "filter"  the group is the gamma of the BatchNorm that follows a conv inside its Sequential (TaylorImportance's rule):
            gamma <- sign(gamma) max(0, |gamma| - lr lam).  A conv followed by BatchNorm is scale-free in its own filter
            norms, which is why the gate is the group; the last conv has no gate and is left alone.

A model on the GPU is stepped by csrc/group_prox.hip; CPU tensors take the torch restatement below, the same arithmetic
operation by operation (include/mcamd.h pins it; tests/gprox_ref.py restates it in numpy).
"""
import math

import torch
import torch.nn as nn

from ._lib import McamdError
from .importance import BLOCK_FILTERS, _block_kb, _block_mask, _filter_mask, _lane_sum, _nblocks, _old_masks

GRANULARITIES = ("block", "filter")


def check_config(lam, granularity, who="GroupLasso"):
    """The refusals GroupLasso and train() share; returns lam as a float."""
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not math.isfinite(lam) or lam < 0:
        raise McamdError("%s: lam must be a finite number >= 0 (got %r)" % (who, lam))
    if granularity not in GRANULARITIES:
        raise McamdError("%s: granularity must be one of %r (got %r)" % (who, GRANULARITIES, granularity))
    return float(lam)


# ----------------------------------------------------------------------------- the arithmetic, in torch (CPU tensors)
def torch_block_prox(w, tau2, nz=None):
    """One proximal step of a BLOCK segment in place on the CPU fp32 tensor `w` ([cout][cin]...); nz: int32 [blocks] or None."""
    cout, cin = w.shape[0], w.shape[1]
    khw = w.numel() // (cout * cin)
    kb = _block_kb(cin)
    nfb, ncb = (cout + BLOCK_FILTERS - 1) // BLOCK_FILTERS, cin // kb
    flat = w.view(cout, cin, khw)
    flags = nz.view(nfb, ncb, khw) if nz is not None else None
    for fb in range(nfb):
        rows = min(BLOCK_FILTERS, cout - BLOCK_FILTERS * fb)
        blk = flat[BLOCK_FILTERS * fb:BLOCK_FILTERS * fb + rows].double().view(rows, ncb, kb, khw)
        n2 = _lane_sum((blk * blk).permute(1, 3, 0, 2).reshape(ncb, khw, rows * kb))      # [cb][tap], e = r kb + c
        thr2 = torch.full_like(n2, float(tau2) * float(rows * kb))
        zero = n2 <= thr2
        s = 1.0 - torch.sqrt(thr2 / n2)
        new = (blk * s.view(1, ncb, 1, khw)).float()
        new = torch.where(zero.view(1, ncb, 1, khw), torch.zeros((), dtype=torch.float32), new)
        flat[BLOCK_FILTERS * fb:BLOCK_FILTERS * fb + rows] = new.view(rows, cin, khw)
        if flags is not None:
            flags[fb] = (~zero).to(torch.int32)


def torch_gate_prox(gamma, tau, nz=None):
    """One proximal step of a GATE segment in place on the CPU fp32 tensor `gamma`; tau is rounded to fp32 first."""
    a = gamma.abs() - torch.tensor(float(tau), dtype=torch.float32)
    zero = a <= 0
    new = torch.where(a > 0, torch.copysign(a, gamma), torch.where(zero, torch.zeros((), dtype=torch.float32), gamma))
    gamma.copy_(new)
    if nz is not None:
        nz.copy_((~zero).to(torch.int32))


# ----------------------------------------------------------------------------- the groups of a model
class GroupLasso:
    """The proximal group-lasso step of `model` (module docstring).

    step(lr, skip=None) shrinks every group at tau = lr * lam: call it behind optimizer.step().  On the GPU it is one launch
    over a table built once (rebuilt when a tensor it names has moved, e.g. behind set_masks), with no allocation and no host
    synchronisation; `skip` (a one-element fp32 tensor on the model's device, e.g. train.StepGuard.found) non-zero leaves
    every weight, gamma and flag as it was, decided on the device.  The flags (int32, one per group: 0 = the group is zero)
    are those of the last step that ran, all ones before the first."""

    def __init__(self, model, lam, granularity="block"):
        self.lam = check_config(lam, granularity)
        self.granularity = granularity
        self.model = model
        allp = list(model.parameters())
        self.params = [p for p in allp if p.dim() != 1]
        if not self.params:
            raise McamdError("GroupLasso: the model has no parameter to group")
        dev = allp[0].device
        if any(p.dtype != torch.float32 or p.device != dev for p in allp):
            raise McamdError("GroupLasso: the model's parameters must be fp32 tensors on one device")
        if any(getattr(m, "share_flag", False) for m in model.modules()):
            raise McamdError("GroupLasso: the model's layers are tied by set_codebooks; the projection onto the codebooks and "
                             "the proximal step would undo each other")
        bn_of = {}
        for m in model.modules():
            if isinstance(m, nn.Sequential):
                kids = list(m.children())
                for a, b in zip(kids, kids[1:]):
                    if isinstance(a, nn.Conv2d) and isinstance(b, nn.BatchNorm2d) and b.weight is not None:
                        bn_of[id(a.weight)] = b
        # per p.dim() != 1 parameter: the tensor the step writes (the weight or its gate's gamma) and its group count, or None
        self.targets, counts = [], []
        for p in self.params:
            t = None
            if granularity == "block" and p.dim() == 4 and p.shape[1] % 32 == 0:
                t = p
                counts.append(_nblocks(p.shape[0], p.shape[1], p.numel() // (p.shape[0] * p.shape[1])))
            elif granularity == "filter" and p.dim() == 4 and id(p) in bn_of:
                t = bn_of[id(p)].weight
                counts.append(t.numel())
            self.targets.append(t)
        if not counts:
            raise McamdError("GroupLasso: the model has no %s group" % granularity)
        self._flat = torch.ones(sum(counts), dtype=torch.int32, device=dev)
        views = iter(torch.split(self._flat, counts))
        self.flags = [next(views) if t is not None else None for t in self.targets]
        self._table, self._key = None, None
        self.tables_built = 0

    def step(self, lr, skip=None):
        tau = float(lr) * self.lam
        if not math.isfinite(tau) or tau < 0:
            raise McamdError("GroupLasso.step: lr * lam must be a finite number >= 0 (got %r)" % (tau,))
        written = [(t, f) for t, f in zip(self.targets, self.flags) if t is not None]
        gate = self.granularity == "filter"
        if not self._flat.is_cuda:
            if skip is not None and float(skip.reshape(-1)[0]) != 0.0:
                return
            for t, f in written:
                w = t.data
                if not w.is_contiguous():
                    raise McamdError("GroupLasso.step: weights must be contiguous fp32 tensors")
                if gate:
                    torch_gate_prox(w, tau, f)
                else:
                    torch_block_prox(w, tau * tau, f)
            if hasattr(self.model, "_mark_weights_replaced"):
                self.model._mark_weights_replaced()
            return
        from . import ops
        key = tuple(t.data_ptr() for t, _ in written)
        if self._table is None or key != self._key:
            self._table = ops.GroupProxTable([dict(w=t.data, nz=f, gate=gate) for t, f in written])
            self._key = key
            self.tables_built += 1
        self._table.step(tau, skip)
        # The kernel wrote through raw pointers.  Bumping the version counters is what an in-place torch write would have done:
        # every engine of the model compares them before its next forward and re-packs (share.project_codebooks).  A "mixed"
        # engine does not re-read its per-layer exponents on a version-only change; none is needed here: every weight is
        # multiplied by a scale in [0, 1] and every |gamma| decreases, so no layer's largest |w| grows.
        for t, _ in written:
            torch.autograd.graph.increment_version(t)

    # ---- reading
    def nonzero_flags(self):
        """One int32 tensor per p.dim() != 1 parameter in model.parameters() order (None for a parameter without groups):
        block flags in mcamd_block_scores' block order, or one flag per filter."""
        return list(self.flags)

    def zero_fraction(self):
        """The fraction of groups that are zero (one host read)."""
        return float((self._flat == 0).sum().item()) / self._flat.numel()

    def masks(self):
        """One mask per p.dim() != 1 parameter in model.parameters() order, the calling convention of every pruner here.
        "block": old_mask x the block flags (ops.block_mask).  "filter": ops.filter_mask of keep = (gamma != 0), what
        quick_filter_prune hands to filter compaction and slim_export.  Parameters without groups keep their old mask, or all
        ones."""
        olds = _old_masks(self.model, self.params)
        out = []
        for p, t, f, old in zip(self.params, self.targets, self.flags, olds):
            if t is None:
                out.append(old.clone() if old is not None else torch.ones_like(p.data))
            elif self.granularity == "block":
                out.append(_block_mask(f, tuple(p.shape), old))
            else:
                out.append(_filter_mask((t.data != 0).to(torch.int32), tuple(p.shape)))
        return out
