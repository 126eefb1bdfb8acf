"""Low-rank layers (an addition beyond the reference; DESIGN.md 3zf, include/mcamd.h).

A k x k convolution Cin -> Cout is split into a k x k convolution Cin -> r and a 1 x 1 convolution r -> Cout (Jaderberg et
al. 2014; Zhang et al. 2015; Denton et al. 2014): the weight, viewed as [Cout, Cin k k], is replaced by its best rank-r
approximation V U.

    lowrank_factor(model, rank=None, energy=None, layers=None) -> factors
    model.set_factors(factors)          # ties the weights: weight = V @ U; registers factor_u / factor_v
    model.lowrank = True                # eval, precision "fp16": fresh factored blocks run csrc/conv_lowrank.hip

A factored model is ordinary fp32 master weights of rank r, so every engine, precision, sparse mode and file format runs
it as it is; only the fp16 inference engine multiplies the factors themselves.  Factors are FRESH while the weight still is
the product set_factors wrote: any later write (optimizer.step, load_weights, set_masks, invalidate_packed) makes them
stale, and a stale block runs dense on its current weights.

    fs = FactorSGD(model, momentum, weight_decay); ...; optimizer.step(); fs.step(lr)    # retraining in factored form

keeps them fresh through training: the dense gradient goes onto the factors, they take the SGD step and W = V U is written
back (csrc/lowrank_train.hip).
"""
import torch

from ._lib import McamdError
from .share import _blocks

MAX_RANK = 256      # the kernel's largest intermediate tile (csrc/conv_lowrank.hip)


def _inner_bn(model):
    """[(conv number, MaskedConv2d, factorisable)] in set_masks order: inner blocks with BatchNorm are factorisable."""
    convs = _blocks(model)
    bn = [int(b.get("batch_normalize", 0)) != 0 for b in model.blocks[1:] if b["type"] == "convolutional"]
    return [(i, conv, 0 < n < len(convs) - 1 and bn[n]) for n, (i, conv) in enumerate(convs)]


def lowrank_factor(model, rank=None, energy=None, layers=None):
    """One (U [r, Cin, k, k], V [Cout, r]) fp32 pair or None per conv block, in set_masks order, from a float64 SVD of each
    inner BatchNorm block's weight viewed as [Cout, Cin k k]: U = sqrt(S_r) Vh_r, V = Uo_r sqrt(S_r).  `rank`: an int, or a
    dict of them by conv number; otherwise `energy`: the smallest multiple of 32 whose kept squared singular values reach
    that fraction of their total.  None where the rank would exceed 256, where r (Cin k k + Cout) >= Cin k k Cout (nothing
    saved), for a block not in `layers` (conv numbers; default: all) and for the first and the last block.  The model is not
    changed: hand the result to model.set_factors."""
    if (rank is None) == (energy is None):
        raise McamdError("lowrank_factor takes exactly one of rank and energy")
    if energy is not None and not 0.0 < float(energy) <= 1.0:
        raise McamdError("energy must be a fraction in (0, 1] (got %r)" % (energy,))
    blocks = _inner_bn(model)
    numbers = [i for i, _, _ in blocks]
    chosen = set(numbers if layers is None else [int(i) for i in layers])
    if chosen - set(numbers):
        raise McamdError("layers names conv numbers the model does not have: %r" % sorted(chosen - set(numbers)))
    out = []
    for i, conv, ok in blocks:
        r = rank.get(i) if isinstance(rank, dict) else rank
        if not ok or i not in chosen or (rank is not None and r is None):
            out.append(None)
            continue
        w = conv.weight.data
        cout, K = w.shape[0], w[0].numel()
        uo, s, vh = torch.linalg.svd(w.detach().reshape(cout, K).double(), full_matrices=False)
        if rank is None:
            e = torch.cumsum(s * s, 0)
            need = int((e < float(energy) * e[-1] * (1.0 - 1e-12)).sum().item()) + 1     # singular values that reach it
            r = (need + 31) // 32 * 32
        elif isinstance(r, bool) or not isinstance(r, int) or r < 1:
            raise McamdError("rank must be a positive int, or a dict of them by conv number (conv%d: %r)" % (i, r))
        if r > MAX_RANK or r > s.numel() or r * (K + cout) >= K * cout:
            out.append(None)
            continue
        root = s[:r].sqrt()
        u = (root[:, None] * vh[:r]).float().reshape((r,) + tuple(w.shape[1:])).contiguous()
        v = (uo[:, :r] * root[None, :]).float().contiguous()
        out.append((u, v))
    return out


def stamp(model, conv):
    """Remember the state the factors of `conv` describe: the parameter's version counter (in-place writes such as
    optimizer.step) and the model's replaced-weights count (load_weights, set_masks, invalidate_packed).  No device read."""
    conv._factor_stamp = (conv.weight._version, model._weights_serial)


def is_fresh(model, conv):
    return (getattr(conv, "factor_u", None) is not None
            and getattr(conv, "_factor_stamp", None) == (conv.weight._version, model._weights_serial))


def set_factors(model, factors):
    convs = _blocks(model)
    if len(factors) != len(convs):
        raise McamdError("set_factors: %d entries for %d convolutional blocks" % (len(factors), len(convs)))
    if all(f is None for f in factors):          # remove: the weights stay what they are
        for _, conv in convs:
            for name in ("factor_u", "factor_v"):
                if name in conv._buffers:
                    del conv._buffers[name]
            conv._factor_stamp = None
        model._mark_weights_replaced()
        return
    for (i, conv), entry in zip(convs, factors):
        if entry is None:
            continue
        if getattr(conv, "mask_flag", False) or getattr(conv, "share_flag", False):
            raise McamdError("set_factors: conv%d carries a %s: a factored block has neither a mask nor a codebook"
                             % (i, "mask" if getattr(conv, "mask_flag", False) else "codebook"))
        u, v = entry
        cout, r = conv.weight.shape[0], u.shape[0]
        if u.dim() != 4 or tuple(u.shape[1:]) != tuple(conv.weight.shape[1:]) or tuple(v.shape) != (cout, r):
            raise McamdError("set_factors: conv%d: factors must be U [r, Cin, k, k] and V [Cout, r] (got %s, %s)"
                             % (i, tuple(u.shape), tuple(v.shape)))
    model._mark_weights_replaced()
    for (i, conv), entry in zip(convs, factors):
        if entry is None:
            continue
        dev = conv.weight.device
        conv.register_buffer("factor_u", entry[0].detach().to(device=dev, dtype=torch.float32).contiguous().clone())
        conv.register_buffer("factor_v", entry[1].detach().to(device=dev, dtype=torch.float32).contiguous().clone())
        r = conv.factor_u.shape[0]
        conv.weight.data = (conv.factor_v @ conv.factor_u.reshape(r, -1)).reshape(conv.weight.shape).to(conv.weight.dtype)
        stamp(model, conv)


def fresh_blocks(model):
    """[(conv number, MaskedConv2d)] whose factors still describe the weight."""
    return [(i, conv) for i, conv in _blocks(model) if is_fresh(model, conv)]


# ----------------------------------------------------------------------------- retraining in factored form
class FactorSGD:
    """Momentum SGD on the factors of `model`'s fresh factored blocks (include/mcamd.h).

        fs = FactorSGD(model, momentum=0.9, weight_decay=0.0)
        loss.backward(); optimizer.step(); fs.step(lr)

    The training step stays the dense one on W = V U.  step() reads the dense weight.grad the backward left, takes it onto the
    factors (gU = V^T G + wd U, gV = G U^T + wd V, both from the old factors), steps them as torch's SGD would (M = mom M + g,
    x = x - lr M; the momentum buffers live here, not in the state_dict) and writes W = V U over whatever the dense optimizer
    wrote: this object owns the weights of its blocks.  On the GPU that is one library call over all blocks -- three launches,
    no allocation, no host synchronisation, bit-reproducible -- on a table built once and rebuilt when a tensor it names has
    moved (weight.grad included).  Afterwards the weights' version counters are bumped and the blocks are stamped fresh, so
    model.lowrank = True runs the trained factors.
    `skip` (a one-element fp32 tensor on the model's device) non-zero leaves factors, momentum and weights as they were,
    decided on the device.  It MUST be the flag the optimizer itself honours (train.StepGuard.found): then the dense step
    left W alone as well, W = V U still holds and the stamp stays valid.
    CPU tensors take a torch fp32 restatement of the same formulas; its sums run in another order, so it is not bit-equal
    to the device."""

    def __init__(self, model, momentum=0.9, weight_decay=0.0):
        self.model, self.momentum, self.weight_decay = model, float(momentum), float(weight_decay)
        self.blocks = fresh_blocks(model)
        if not self.blocks:
            raise McamdError("FactorSGD: the model has no fresh factored block (lowrank_factor, then set_factors)")
        from . import _lib
        for i, conv in self.blocks:
            cout, r = conv.factor_v.shape
            if conv.weight.dtype != torch.float32:
                raise McamdError("FactorSGD: conv%d: the weight must be fp32" % i)
            info = _lib.LrsgdInfo()       # (the CPU restatement keeps the kernel's shapes: one rule for both)
            if _lib.lib().mcamd_lowrank_sgd_info(cout, conv.weight[0].numel(), r, _lib.C.byref(info)) != 0:
                raise McamdError("FactorSGD: conv%d: %s" % (i, _lib.lib().mcamd_last_error().decode()))
        self.mu = [torch.zeros_like(conv.factor_u) for _, conv in self.blocks]
        self.mv = [torch.zeros_like(conv.factor_v) for _, conv in self.blocks]
        self._table, self._key = None, None
        self.tables_built = 0

    def step(self, lr, skip=None):
        lr = float(lr)
        for i, conv in self.blocks:
            if conv.weight.grad is None:
                raise McamdError("FactorSGD.step: conv%d has no weight.grad: call it behind backward() and optimizer.step()" % i)
        if not self.blocks[0][1].weight.is_cuda:
            if skip is not None and float(skip.reshape(-1)[0]) != 0.0:
                return
            mom, wd = self.momentum, self.weight_decay
            for (_, conv), mu, mv in zip(self.blocks, self.mu, self.mv):
                u4, v = conv.factor_u, conv.factor_v
                u, g = u4.reshape(u4.shape[0], -1), conv.weight.grad.reshape(v.shape[0], -1).float()
                gu, gv = v.t() @ g + wd * u, g @ u.t() + wd * v
                mu.mul_(mom).add_(gu.reshape(mu.shape))
                mv.mul_(mom).add_(gv)
                u4.sub_(lr * mu)
                v.sub_(lr * mv)
                with torch.no_grad():
                    conv.weight.copy_((v @ u4.reshape(u4.shape[0], -1)).reshape(conv.weight.shape))
                stamp(self.model, conv)
            return
        from . import ops
        tensors = [(conv.weight.grad, conv.factor_u, conv.factor_v, mu, mv, conv.weight.data)
                   for (_, conv), mu, mv in zip(self.blocks, self.mu, self.mv)]
        key = tuple(t.data_ptr() for ts in tensors for t in ts)
        if self._table is None or key != self._key:
            self._table = ops.LowRankSgdTable([dict(zip(("g", "u", "v", "mu", "mv", "w"), ts)) for ts in tensors])
            self._key = key
            self.tables_built += 1
        self._table.step(lr, self.momentum, self.weight_decay, skip)
        # The kernel wrote through raw pointers.  Bumping the version counters is what an in-place torch write would have done:
        # every engine of the model compares them before its next forward and re-packs (share.project_codebooks); the stamp
        # behind it says the factors describe the weight again.
        for _, conv in self.blocks:
            torch.autograd.graph.increment_version(conv.weight)
            stamp(self.model, conv)
