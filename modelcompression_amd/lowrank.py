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
