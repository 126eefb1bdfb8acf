"""Fused MI355X execution plan for a Darknet/YOLOv2 block list.

`Darknet.forward` (reference src/nets.py:720-774) walks the cfg blocks and calls one torch
module per block.  Here the same block list is compiled once per batch size into a static
launch plan over libmcamd.so:

  forward, per [convolutional] block
      mcamd_conv_fwd      implicit-GEMM MFMA conv -> raw fp16 output + BN partial sums
      mcamd_bn_coeffs     batch (train) or running (eval) statistics -> scale/shift
      mcamd_bn_act_fwd    BN + LeakyReLU, fused with the following [maxpool] / [reorg],
                          written straight into the consumer's padded NHWC buffer
                          ([route] concat = channel slices of one buffer, no copy)
      the last, linear block writes fp32 NCHW logits (+bias) from the conv epilogue
  backward, reverse order
      mcamd_bn_act_bwd    pool/reorg/route + LeakyReLU + BN backward -> dY (padded NHWC)
      mcamd_conv_wgrad    dW * mask (fp32 OIHW, straight into the flat gradient buffer)
      mcamd_conv_dgrad    gradient wrt the block input

Activations live in HBM as padded NHWC fp16 for the whole step; weights are re-packed
(fp32 master * mask -> fp16) once per optimizer step.  All buffers are allocated once per
batch size; a B=64 training step holds ~7 GB of the 288 GB.
"""
import contextlib
import math
import os
import time

import torch

from . import ops
from . import _lib as L
from ._lib import McamdError


class _T:
    """Where a block output lives: channel slice [choff, choff+C) of a padded NHWC buffer.  `ps`: plane stride of
    the buffer when it holds split (hi | lo | hi) activations (precision "fp16x3"): the slice repeats at
    choff + ps and choff + 2 * ps."""
    __slots__ = ("buf", "ld", "choff", "C", "H", "W", "ps", "ps0")

    def __init__(self, buf, ld, choff, C, H, W, ps=0):
        self.buf, self.ld, self.choff, self.C, self.H, self.W, self.ps = buf, ld, choff, C, H, W, ps
        self.ps0 = ps          # (a folded producer's planes move closer together: Engine._plan_folds)


_LAYER_FIELDS = dict(
    # geometry: the block, its place in the plan, the shapes of its launches
    index=0, li=0, conv=None, bn=None, slope=1.0, src=0, tin=None, cin=0, cout=0, cout_p=0, H=0, W=0, k=0, M=0, stem=0, pad=0,
    level=1, mode=0, out_id=None, out2_id=None, out_t=None, out2_t=None, is_last=False, train_ok=True, border=None,
    border_map=None, geom=None, geom_f=None, p_lo=0, p_hi=0,
    # buffers: packed weights (forward / dgrad), raw output + statistics, BatchNorm coefficients, gradients
    wp=None, wd=None, y=None, stats=None, scale=None, shift=None, mean=None, invstd=None, dy=None, gin=None, act_full=None,
    # compaction / fold (_update_compaction, _plan_folds)
    keep=None, perm=None, perm32=None, in_perm=None, g_rows=None, g_cols=None, n_act=0, geom_act=None, gather=False,
    fold=None, fold_cin=0, fold_aug=0, fold_consumers=None, ones_idx=-1, skip_dead=False, bn_width=0, waug=None, dwaug=None,
    # first-block variants, and the fp8 correction form of a split-operand block
    fused_stem=False, fused_stem_eval=False, stem_shadow=False, stem_split=False, stem_f32=False, stem_ws=None, weff=None,
    sh_img=None, sh_img_lo=None, sh_geom=None, sh_wp=None, sh_wp_lo=None, sh_coef=None,
    f8=False, f8_wexp=ops.F8_WEXP_DEFAULT, f8_wexp_eff=ops.F8_WEXP_DEFAULT,
    # inference form (Engine._choose_forms, _FORMS) and what belongs to one: split-K slices (forms "splitk" and "q8_splitk"),
    # 2:4 values + index words, block-sparse chunk lists
    form="dense", sk_slices=1, wsp=None, widx=None, bs_count=None, bs_list=None,
    # the training form of the block-sparse kernel (form "bsparse_train"): its statistics slab (one row per pixel tile), the
    # chunk lists over the dgrad packing, whether the dgrad launch takes it too, and full lists (Engine.bsparse_train_full_lists)
    bs_stats=None, bs_dcount=None, bs_dlist=None, bs_dgrad=False, bs_full=None,
    # ... and its weight gradient on tile lists (Darknet.sparse_train = "block-wgrad"): the lists built from the
    # mask when the policy ran with their two counters as host integers (kept tiles, kept (tile, tap) pairs), whether the
    # launch takes them, its split count and workspace bytes, and full lists at that split count
    bw_tiles=None, bw_words=None, bw_dev_counts=None, bw_counts=None, bw_on=False, bw_nsplit=0, bw_bytes=0, bw_full=None,
    # fp8: launch geometry on the byte buffer, byte destinations, private input copy, packed operands; "fp8-qat" training:
    # the fp32 raw output + statistics that stand in for the fp16 ones, and the values the weight bytes stand for
    geom_q8=None, q8_y=False, q8_y2=False, xq=None, _xq=None, _xq_key=None, wq=None, wqs=None, widx8=None, wexp=None,
    w4c=None, w4g=None, wexp4=None,
    y_f16=None, stats_f16=None, y_f32=None, stats_q8=None, w_q=None)


class _Layer:
    """One [convolutional] block of the plan.  Every field it can carry is declared above with its default: a misspelt one
    raises instead of reading as "off"."""
    __slots__ = tuple(_LAYER_FIELDS)

    def __init__(self):
        for name, default in _LAYER_FIELDS.items():
            setattr(self, name, default)
        self.fold_consumers = []

    # exactly one inference form per block; the flags of the single forms are read-only views of it
    sp_on = property(lambda self: self.form == "sparse24")
    bs_on = property(lambda self: self.form == "bsparse")
    sk_on = property(lambda self: self.form == "splitk")
    q8_on = property(lambda self: self.form in ("q8", "q8_slim", "q8_sparse24", "q8_splitk", "q8_w4", "q8_bsparse"))
    q8s_on = property(lambda self: self.form == "q8_sparse24")
    q8_slim = property(lambda self: self.form == "q8_slim")


def _momentum(bn):
    """BatchNorm momentum as the coefficient kernels take it (None reads as torch's default, 0.1)."""
    return bn.momentum if bn.momentum is not None else 0.1


def _resolve_routes(blocks):
    """Per models-index: (type, [source tensor ids]); tensor id -1 is the network input."""
    ops_ = []
    for ind, b in enumerate(blocks[1:]):
        t = b["type"]
        if t in ("convolutional", "maxpool", "reorg"):
            ops_.append((t, [ind - 1]))
        elif t == "route":
            ls = [int(i) if int(i) > 0 else int(i) + ind for i in b["layers"].split(",")]
            ops_.append((t, ls))
        elif t in ("region", "cost"):
            ops_.append((t, []))
        else:
            raise NotImplementedError("block type %r is outside the YOLOv2 conv hot path" % t)
    return ops_


# Relative error one conv block adds to the logits when both of its MFMA operands are plain fp16 (weights and
# stored activation rounded to 11 bits: 2 x 2.07e-4 rms in quadrature; tools/error_budget.py measures 1.1-3.2e-4 per
# block of YOLOv2-VOC, 1.26e-3 root-sum-square over the 23 blocks = the 1.3e-3 the all-fp16 forward shows).
PLAIN_BLOCK_ERR = 2.9e-4
# "mixed" precision keeps plain fp16 operands on the costliest blocks while their root-sum-square stays below this
# (north_star: region-layer logits within 1e-3 of the reference; measured on YOLOv2-VOC: 5.2e-4 at B=1)
MIXED_BUDGET = 5.5e-4
# TRAINING mode is different: with batch statistics a random-init BatchNorm / LeakyReLU network AMPLIFIES a perturbation on
# its way to the logits -- plain fp16 operands on block l alone cost 3.0e-4 (conv23), 3.7e-4 (conv19), 1.0e-3 (conv14),
# 4.8e-3 (conv6), 1.9e-2 (conv1) on YOLOv2-VOC (tools/error_budget.py --train; the oracle with every stored tensor
# rounded to fp16 sits at 3.7e-2 at every batch size and seed).  So the blocks that may stay plain are the LAST ones, the
# first block must be split too, and a block's term grows by TRAIN_GAIN per conv block that follows it (measured
# 1.05 ... 1.15 over the last ten blocks).  With this budget conv19 / 20 / 22 stay plain: 6.0e-4 predicted, 5.7-6.0e-4
# measured over four seeds (tools/f8_seeds.py).
# The fp8 correction form of the split blocks (Engine.f8) leaves ~4 % of a block's plain-operand term (two e4m3 roundings
# per correction product), amplified like it: measured per block conv3 3.9e-4, conv5 1.9e-4, conv6 2.0e-4, conv8 1.0e-4,
# the ten blocks behind 1.4e-4 together; 5.0e-4 in all -> 7.3-7.7e-4 over the four seeds, 7.8e-4 at B=16 / seed 0.
# (Leaving conv3 on fp16 lo planes: 6.7e-4 for +0.13 ms per B=64 step; conv3 and conv5: 6.5e-4 for +0.25 ms.  The fp8
# form stays on everywhere: the step meets 12.0 ms with it and the bar is 1e-3.)
MIXED_BUDGET_TRAIN = 7.0e-4
TRAIN_GAIN = 1.1
# Darknet.sparse = "block": a masked block leaves the dense fp16 launch for the block-sparse kernel (csrc/conv_bsparse.hip)
# when the kept fraction of its (64-filter tile, K chunk) pairs is at most this -- the default of Darknet.sparse_max_kept.
# Measured (tools/bsparse_bench.py, profiles/bsparse_bench.json): the largest kept fraction at which the kernel
# is at least 10 % faster than the dense launch on every layer of conv9 .. conv22 at B = 128 (worst layer 1.15x at 0.375;
# at 0.5 conv9 / 11 / 13 gain 4-9 % only, and from 0.625 up the 3x3 layers lose).
BSPARSE_MAX_KEPT = 0.375
# Darknet.precision = "fp8-block": a masked fp8 block leaves the dense fp8 launch for the block-sparse fp8 kernel
# (csrc/conv_q8_bsparse.hip) when the kept fraction of its (64-filter tile, 64-byte K chunk) pairs is at most
# this -- the default of Darknet.fp8_block_max_kept.  Measured by the rule of DESIGN.md 3t against the same commit's "fp8"
# engine (tools/bsparse_bench.py --precision fp8, profiles/q8_bsparse_bench.json and q8_bsparse_bench_mfma.json):
# the largest kept fraction at which the kernel is at least 10 % faster than the fp8 launch on every layer of conv9 .. conv22
# at B = 128 is 0.375 in both MFMA forms (worst layer 1.16x on converted bytes, 1.15x on the fp8 MFMA; at 0.5 conv15 / conv22
# gain 5-7 % only, and from 0.625 up the fp8-MFMA form loses on the 13x13 3x3 layers).
Q8_BSPARSE_MAX_KEPT = 0.375
# Darknet.sparse_train = "block": a masked block of the fp16 TRAINING step leaves the dense forward and dgrad launches for the
# raw-epilogue form of the block-sparse kernel when its kept-chunk fraction is at most this -- the default of
# Darknet.sparse_train_max_kept.  The rule of DESIGN.md 3t on tools/bsparse_train_bench.py (profiles/bsparse_train_bench.json):
# the largest measured kept fraction at which BOTH the forward and the dgrad launch of every layer of conv9 .. conv22 are at
# least 10 % faster than the dense training launches they replace (0.0 would mean: no level passes).  Measured at B = 64: 0.375
# (worst launch 1.11x, conv21's dgrad; at 0.5 conv9's dgrad loses 3 %).  The rule looks at the launches it replaces: the two list
# launches per chosen block and step (0.9 ms per step in all) are not in it -- the whole step only gains below kept 0.3.
BSPARSE_TRAIN_MAX_KEPT = 0.375
# Darknet.sparse_train = "block-wgrad": a block that trains on the block-sparse kernel also sends its weight gradient through
# the list launch (mcamd_conv_wgrad_bsparse) when the kept fraction of its (64 x 64 tile, tap) pairs is at most
# this -- the default of Darknet.sparse_train_wgrad_max_kept.  The rule of DESIGN.md 3t on tools/bsparse_train_bench.py
# (profiles/bsparse_train_wgrad_bench.json): the largest measured kept level at which the list launch of EVERY chosen layer of
# conv9 .. conv22 is at least 10 % faster than the dense weight-gradient launch it replaces; 0.0: no level passes.
# Measured at B = 64: 0.1 (worst layer 1.15x, conv18; at 0.25 the 13x13 3x3 layers lose 2-18 %: a 9-tap tile stages its whole
# window for however few taps it keeps, and nearly every tile keeps some).  Whole step at kept 0.1: dense 9.15, "block" 7.89,
# "block-wgrad" 7.13 ms.  A block_prune level of 90 % leaves layers at 0.100 .. 0.125: a caller who wants them all sets 0.125.
BSPARSE_TRAIN_WGRAD_MAX_KEPT = 0.1


class _Dense:
    """One inference form of a block (`_Layer.form`, chosen by Engine._choose_forms): what it allocates, how it packs and
    what it launches.  This one is the dense fp16 launch off the packed weights every block has; a form with packed
    operands of its own names them once.  `ops` functions are named, not bound, and looked up when they are called."""
    fwd = "conv_fwd_padded"              # ops: the forward with the fused inference epilogue
    geom = "geom_act"                    # layer field of its geometry
    bufs = (("wp", torch.float16),)      # (layer field, dtype) of its weight operands, in the order elems / packer / fwd take them
    elems = packer = None                # ops: their sizes, and the pass that fills them from the fp32 master * mask (None:
                                         # `wp` is the pack table's)

    def alloc(self, eng, lays):
        """Buffers of the blocks that took this form (behind every choice): kept where the size already matches."""
        for lay in lays if self.elems else ():
            for (name, dtype), n in zip(self.bufs, getattr(ops, self.elems)(getattr(lay, self.geom))):
                if getattr(lay, name) is None or getattr(lay, name).numel() != n:
                    setattr(lay, name, torch.zeros(n, dtype=dtype, device=eng.device))

    def pack(self, eng, lay, w, mask):
        """This form's operands (every re-pack, in front of the pack table's launch)."""
        if self.packer:
            getattr(ops, self.packer)(getattr(lay, self.geom), w, mask, *(getattr(lay, name) for name, _ in self.bufs))

    def repacked(self, eng, lay):
        """... and what it derives from the packed weights (every re-pack, behind that launch)."""

    def operands(self, eng, lay, xin):
        """(geometry, input, weights...) of the fused launch and its extra keywords."""
        return (getattr(lay, self.geom), xin, *(getattr(lay, name) for name, _ in self.bufs)), {}

    def raw(self, eng, lay, xin, training):
        """The launch of a block that does not take the fused path: raw fp16 output (+ batch statistics in training)."""
        eng._timed('fwd', lay, ops.conv_fwd_raw, lay.geom_act, xin, lay.wp, lay.y, lay.cout, 0, lay.stats if training else None)


class _SplitK(_Dense):
    """Few pixels: K cut into slices over the whole chip (Darknet.splitk, csrc/conv_splitk.hip)."""
    fwd = "conv_fwd_splitk"

    def alloc(self, eng, lays):
        # one workspace of the largest requirement: the layers run one after another on the launch stream
        need = max(ops.conv_fwd_splitk_info(lay.geom_act, *eng._splitk_form(lay)).workspace_bytes for lay in lays)
        if eng._splitk_ws is None or eng._splitk_ws.numel() * 4 < need:
            eng._splitk_ws = torch.empty(need // 4, dtype=torch.float32, device=eng.device)

    def operands(self, eng, lay, xin):
        return _Dense.operands(self, eng, lay, xin)[0], dict(slices=lay.sk_slices, workspace=eng._splitk_ws)

    def raw(self, eng, lay, xin, training):
        if training:
            return _Dense.raw(self, eng, lay, xin, training)
        eng._timed('fwd', lay, ops.conv_fwd_raw_splitk, lay.geom_act, xin, lay.wp, lay.y, lay.cout, 0,
                   slices=lay.sk_slices, workspace=eng._splitk_ws)


class _Sparse24(_Dense):
    """2:4 weights on the sparse MFMA (Darknet.sparse = "2:4", csrc/conv_sparse.hip): kept values + index words."""
    fwd, elems, packer = "conv_fwd_sparse24", "sparse24_elems", "pack_sparse24"
    bufs = (("wsp", torch.float16), ("widx", torch.int16))


class _BSparse(_Dense):
    """The non-zero K chunks of each 64-filter tile only (Darknet.sparse = "block", csrc/conv_bsparse.hip).  Two phases:
    `policy` reads the masked weights in front of the filter compaction (the blocks it picks are exempt from it),
    `repacked` rebuilds the chunk lists of the blocks that kept the form from the weights the launch reads."""
    fwd = "conv_fwd_bsparse"
    bufs = (("wp", torch.float16), ("bs_count", torch.int32), ("bs_list", torch.int32))

    def policy(self, eng, max_kept):
        """Taken in front of every re-pack (masks, weights, the mode or Darknet.sparse_max_kept changed): every candidate's
        chunk lists from its packed weights in their own filter and channel order (mcamd_bsparse_lists on a temporary
        packing), ONE host read of all counts, and a candidate is chosen when its kept-chunk fraction, sum(count) /
        (tiles x chunks), is at most `max_kept`.  Returns (the chosen layer indices, conv number -> kept fraction of every
        candidate): pack() keeps the chosen blocks out of the filter compaction, whose physical channel order would scatter
        the zero blocks over the K chunks."""
        def masked(lay):
            m = lay.conv.mask if lay.conv.mask_flag else None
            return m is not None and m.is_cuda and m.dtype == torch.float32 and m.shape == lay.conv.weight.shape
        cand = [lay for lay in eng.layers if masked(lay) and not eng.q8 and eng._eligible(lay, compacted=False)
                and ops.conv_fwd_bsparse_ok(lay.geom)]
        sums = []
        for lay in cand:
            wp, _ = ops.pack_weights(lay.geom, lay.conv.weight.data, lay.conv.mask.contiguous(), want_dgrad=False)
            sums.append(ops.bsparse_lists(lay.geom, wp)[0].sum())
        chosen, kept = [], {}
        for lay, s_ in zip(cand, torch.stack(sums).cpu().tolist() if cand else []):
            kept[lay.li + 1] = s_ / float(ops.bsparse_elems(lay.geom)[1])       # conv number (conv1 = the first block)
            if kept[lay.li + 1] <= max_kept:
                chosen.append(lay.li)
        return frozenset(chosen), kept

    def alloc(self, eng, lays):
        for lay in lays:
            nc, nl = ops.bsparse_elems(lay.geom_act)
            if lay.bs_count is None or lay.bs_count.numel() != nc or lay.bs_list.numel() != nl:
                lay.bs_count = torch.zeros(nc, dtype=torch.int32, device=eng.device)
                lay.bs_list = torch.zeros(nc, nl // nc, dtype=torch.int32, device=eng.device)

    def repacked(self, eng, lay):
        ops.bsparse_lists(lay.geom_act, lay.wp, lay.bs_count, lay.bs_list)


class _BSparseTrain(_BSparse):
    """The training form (Darknet.sparse_train = "block"): the same kernel with the raw fp16 epilogue, for the
    forward launch (statistics slab of one row per pixel tile) and -- on chunk lists built from the dgrad packing, whose K
    order is the forward's over cout_p -- for the dgrad launch.  Both lists are rebuilt behind every re-pack."""
    fwd = None                           # (no fused inference launch: an eval pass chooses its forms by Darknet.sparse)

    def policy(self, eng, max_kept, wgrad=False):
        """_BSparse.policy for the training step: the candidates are the masked inner blocks the training launches accept
        (Engine._bst_eligible); planned once while the masks are static (pack caches the answer by the mask keys).
        `wgrad` ("block-wgrad"): the tile lists of the weight gradient's list launch are built here too, from the MASK of
        every candidate whose geometry mcamd_conv_wgrad_bsparse_ok accepts, and their two counters come back in the same
        host read: a step never builds them, and never reads anything back (Engine._choose_bst_wgrad decides from them)."""
        def masked(lay):
            m = lay.conv.mask if lay.conv.mask_flag else None
            return m is not None and m.is_cuda and m.dtype == torch.float32 and m.shape == lay.conv.weight.shape
        cand = [lay for lay in eng.layers if masked(lay) and eng._bst_eligible(lay, compacted=False)]
        sums = []
        for lay in cand:
            wp, _ = ops.pack_weights(lay.geom, lay.conv.weight.data, lay.conv.mask.contiguous(), want_dgrad=False)
            sums.append(ops.bsparse_lists(lay.geom, wp)[0].sum())
        for lay in eng.layers:
            lay.bw_counts, lay.bw_full = None, None
        wcand = [lay for lay in cand if wgrad and ops.conv_wgrad_bsparse_ok(lay.geom)]
        for lay in wcand:
            nt, nw = ops.wgrad_bsparse_elems(lay.geom)
            if lay.bw_tiles is None or lay.bw_tiles.numel() != nt:
                lay.bw_tiles = torch.zeros(nt, dtype=torch.int32, device=eng.device)
                lay.bw_words = torch.zeros(nw, dtype=torch.int32, device=eng.device)
                lay.bw_dev_counts = torch.zeros(2, dtype=torch.int32, device=eng.device)
            ops.wgrad_bsparse_lists(lay.geom, lay.conv.mask.contiguous(), lay.bw_tiles, lay.bw_words, lay.bw_dev_counts)
        host = (torch.cat([torch.stack(sums)] + [lay.bw_dev_counts.long() for lay in wcand]).cpu().tolist() if cand else [])
        chosen, kept = [], {}
        for lay, s_ in zip(cand, host):
            kept[lay.li + 1] = s_ / float(ops.bsparse_elems(lay.geom)[1])       # conv number (conv1 = the first block)
            if kept[lay.li + 1] <= max_kept:
                chosen.append(lay.li)
        for i, lay in enumerate(wcand):
            lay.bw_counts = tuple(host[len(cand) + 2 * i:len(cand) + 2 * i + 2])
        return frozenset(chosen), kept

    def alloc(self, eng, lays):
        _BSparse.alloc(self, eng, lays)
        dev = eng.device
        for lay in lays:
            rows = ops.bsparse_raw_stats_rows(lay.geom_act)
            if lay.bs_stats is None or lay.bs_stats.shape[0] != rows:
                lay.bs_stats = torch.zeros(rows, 2, ops.round_up(lay.cout, 256), dtype=torch.float32, device=dev)
            # a block on the one-launch 1x1 backward keeps that backward: only its forward is chosen
            lay.bs_dgrad = (lay.gin is not None and lay.wd is not None and not eng._bwd1x1_route(lay)
                            and ops.conv_bsparse_train_ok(lay.geom_act, True))
            nc, nl = ops.bsparse_elems_dgrad(lay.geom_act) if lay.bs_dgrad else (0, 0)
            if lay.bs_dgrad and (lay.bs_dcount is None or lay.bs_dcount.numel() != nc or lay.bs_dlist.numel() != nl):
                lay.bs_dcount = torch.zeros(nc, dtype=torch.int32, device=dev)
                lay.bs_dlist = torch.zeros(nc, nl // nc, dtype=torch.int32, device=dev)
            lay.bs_full = None               # (Engine.bsparse_train_full_lists: built when a launch asks for them)

    def repacked(self, eng, lay):
        eng._timed('lists', lay, ops.bsparse_lists, lay.geom_act, lay.wp, lay.bs_count, lay.bs_list)
        if lay.bs_dgrad:
            eng._timed('lists', lay, ops.bsparse_lists_dgrad, lay.geom_act, lay.wd, lay.bs_dcount, lay.bs_dlist)

    def full(self, eng, lay):
        """(count, list, dgrad count, dgrad list) naming every chunk: the test switch Engine.bsparse_train_full_lists"""
        if lay.bs_full is None:
            full = ops.bsparse_full_lists(*ops.bsparse_elems(lay.geom_act), eng.device)
            lay.bs_full = full + (ops.bsparse_full_lists(*ops.bsparse_elems_dgrad(lay.geom_act), eng.device) if lay.bs_dgrad
                                  else (None, None))
        return lay.bs_full

    def raw(self, eng, lay, xin, training):
        if not training:
            return _Dense.raw(self, eng, lay, xin, training)
        count, lst = self.full(eng, lay)[:2] if eng.bsparse_train_full_lists else (lay.bs_count, lay.bs_list)
        eng._timed('fwd', lay, ops.conv_fwd_bsparse_raw, lay.geom_act, xin, lay.wp, count, lst, lay.y, lay.cout, 0, stats=lay.bs_stats)

    def dgrad(self, eng, lay, concurrent):
        """The dgrad launch of a chosen block (Engine._backward_body): no producer sums -- its producer's BatchNorm backward
        runs its own pass 0."""
        count, lst = self.full(eng, lay)[2:] if eng.bsparse_train_full_lists else (lay.bs_dcount, lay.bs_dlist)
        eng._timed('dgrad', lay, ops.conv_dgrad_bsparse, lay.geom_act, lay.dy, lay.cout_p, 0, lay.wd, count, lst, lay.gin,
                   lay.tin.ld, lay.tin.choff, overflow=eng.overflow, concurrent=concurrent)

    def wgrad(self, eng, lay, gw, mask, D, dbias, ws):
        """The weight gradient of a block on the list launch (lay.bw_on, Engine._choose_bst_wgrad): the lists and the host
        integers the policy left; under Engine.bsparse_train_full_lists every tile with every tap at the SAME split count."""
        tiles, words, n = lay.bw_tiles, lay.bw_words, lay.bw_counts[0]
        if eng.bsparse_train_full_lists:
            if lay.bw_full is None:
                lay.bw_full = ops.wgrad_bsparse_full_lists(lay.geom, eng.device)
            (tiles, words), n = lay.bw_full, lay.bw_full[0].numel()
        eng._timed('wgrad', lay, ops.conv_wgrad_bsparse, lay.geom, eng.bufs[lay.tin.buf], lay.dy, lay.cout_p, 0, gw, mask, tiles,
                   words, n, lay.bw_nsplit, D, dbias, ws)


class _Q8(_Dense):
    """e4m3 activations x e4m3 weights (Darknet.precision = "fp8", csrc/conv_q8.hip): bytes + one exponent per filter,
    computed on the device."""
    fwd, elems, packer, geom = "conv_fwd_q8", "q8_elems", "pack_q8", "geom_q8"
    bufs = (("wq", torch.uint8), ("wexp", torch.int32))

    def pack(self, eng, lay, w, mask):
        _Dense.pack(self, eng, lay, w, mask)
        if eng._qat_train(lay):     # the values those bytes stand for, fp32 OIHW: the dgrad packing's source
            ops.fakequant_q8(lay.geom_act, w, mask, lay.wexp, lay.w_q)

    def qat_raw(self, eng, lay, x8):
        """The training-mode launch of a quantisation-aware training block (Engine._qat_forward): fp32 raw output + statistics."""
        eng._timed('fwd', lay, ops.conv_fwd_q8_raw, lay.geom_act, x8, lay.wq, lay.wexp, lay.y, lay.cout, 0, lay.stats)

    def operands(self, eng, lay, xin):
        x8 = eng.qbufs.get(lay.tin.buf)
        if lay.xq is not None:      # the fp16 -> fp8 edge: cast pass over the padded input slice into a private byte copy
            ti, x8 = lay.tin, lay.xq
            eng._timed('cast', lay, ops.cast_q8, xin, eng.B * (ti.H + 2) * (ti.W + 2), ti.ld, ti.choff, lay.cin,
                       x8, lay.geom_q8.x_ld, ti.choff)
        return _Dense.operands(self, eng, lay, x8)[0], dict(y_f8=lay.q8_y, y2_f8=lay.q8_y2)


class _Q8Slim(_Q8):
    """A slim model's fp8 block: rows of round_up(cin, 64) channels with zero bytes behind the real ones, border table in
    the epilogue."""
    fwd, elems, packer = "conv_fwd_q8_slim", "q8_slim_elems", "pack_q8_slim"

    def operands(self, eng, lay, xin):
        args, kw = _Q8.operands(self, eng, lay, xin)
        return args, dict(kw, border=lay.border, border_ld=lay.cout)


class _Q8Sparse24(_Q8):
    """2:4-compressed e4m3 weights with their index words on the sparse MFMA ("fp8-2:4", csrc/conv_q8_sparse.hip)."""
    fwd, elems, packer = "conv_fwd_q8_sparse24", "q8_sparse24_elems", "pack_q8_sparse24"
    bufs = (("wqs", torch.uint8), ("widx8", torch.int32), ("wexp", torch.int32))


class _Q8SplitK(_Q8):
    """An fp8 block of few pixels: the byte K loop cut into slices over the whole chip ("fp8-splitk", csrc/conv_q8_splitk.hip).
    The operands are _Q8's; the workspace is the engine's one split-K workspace."""
    fwd = "conv_fwd_q8_splitk"

    def alloc(self, eng, lays):
        _Q8.alloc(self, eng, lays)
        need = max(ops.conv_fwd_q8_splitk_info(lay.geom_q8, lay.mode, lay.sk_slices).workspace_bytes for lay in lays)
        if eng._splitk_ws is None or eng._splitk_ws.numel() * 4 < need:
            eng._splitk_ws = torch.empty(need // 4, dtype=torch.float32, device=eng.device)

    def operands(self, eng, lay, xin):
        args, kw = _Q8.operands(self, eng, lay, xin)
        return args, dict(kw, slices=lay.sk_slices, workspace=eng._splitk_ws)


class _Q8BSparse(_Q8):
    """The non-zero 64-byte K chunks of each 64-filter tile only ("fp8-block", csrc/conv_q8_bsparse.hip): _Q8's
    bytes and exponents plus the chunk lists.  Two phases, as _BSparse: `policy` reads the packed bytes of the masked weights
    in front of the filter compaction (the blocks it picks are exempt from it), `repacked` rebuilds the lists of the blocks
    that took the form from the bytes the launch reads."""
    fwd = "conv_fwd_q8_bsparse"
    bufs = (("wq", torch.uint8), ("wexp", torch.int32), ("bs_count", torch.int32), ("bs_list", torch.int32))

    def policy(self, eng, max_kept):
        """Taken in front of every re-pack of an "fp8-block" engine: the candidates are the masked blocks _choose_q8 would give
        form "q8" if their filters stayed uncompacted; each one's chunk lists from a temporary mcamd_pack_q8 in the layer's
        own order (mcamd_q8_bsparse_lists), ONE host read of all counts, and a candidate is chosen when its kept-chunk
        fraction is at most `max_kept` (0.0 chooses nothing).  Returns (the chosen layer indices, conv number -> kept
        fraction of every candidate)."""
        def masked(lay):
            m = lay.conv.mask if lay.conv.mask_flag else None
            return m is not None and m.is_cuda and m.dtype == torch.float32 and m.shape == lay.conv.weight.shape
        cand = [lay for lay in eng.layers if masked(lay) and not lay.pad and lay.cin % 64 == 0 and lay.border is None
                and eng._eligible(lay, compacted=False) and ops.conv_fwd_q8_bsparse_ok(lay.geom)]
        sums = []
        for lay in cand:
            wq, _ = ops.pack_q8(lay.geom, lay.conv.weight.data, lay.conv.mask.contiguous())
            sums.append(ops.q8_bsparse_lists(lay.geom, wq)[0].sum())
        chosen, kept = [], {}
        for lay, s_ in zip(cand, torch.stack(sums).cpu().tolist() if cand else []):
            kept[lay.li + 1] = s_ / float(ops.q8_bsparse_elems(lay.geom)[1])    # conv number (conv1 = the first block)
            if max_kept > 0.0 and kept[lay.li + 1] <= max_kept:
                chosen.append(lay.li)
        return frozenset(chosen), kept

    def alloc(self, eng, lays):
        for lay in lays:
            for (name, dtype), n in zip(self.bufs[:2], ops.q8_elems(lay.geom_q8)):
                if getattr(lay, name) is None or getattr(lay, name).numel() != n:
                    setattr(lay, name, torch.zeros(n, dtype=dtype, device=eng.device))
            nc, nl = ops.q8_bsparse_elems(lay.geom_q8)
            if lay.bs_count is None or lay.bs_count.numel() != nc or lay.bs_list.numel() != nl:
                lay.bs_count = torch.zeros(nc, dtype=torch.int32, device=eng.device)
                lay.bs_list = torch.zeros(nc, nl // nc, dtype=torch.int32, device=eng.device)

    def pack(self, eng, lay, w, mask):
        ops.pack_q8(lay.geom_q8, w, mask, lay.wq, lay.wexp)

    def repacked(self, eng, lay):
        ops.q8_bsparse_lists(lay.geom_q8, lay.wq, lay.bs_count, lay.bs_list)


class _Q8W4(_Q8):
    """An fp8 block on 4-bit weights ("fp8-w4", csrc/conv_q8_w4.hip): e2m1 nibble codes, one shift byte per group
    of 32 input channels and one exponent per filter -- 4.25 bits per weight, expanded to e4m3 bytes in the kernel's registers.
    No weight bytes (`wq`) are held.  Under "fp8-w4-qat"  the training-mode forward runs on the same operands,
    re-quantised every step, and `w_q` -- the values the codes stand for -- is decoded from them for the dgrad packing."""
    fwd, elems, packer = "conv_fwd_q8_w4", "q8_w4_elems", "pack_q8_w4"
    bufs = (("w4c", torch.uint8), ("w4g", torch.uint8), ("wexp4", torch.int32))

    def pack(self, eng, lay, w, mask):
        _Dense.pack(self, eng, lay, w, mask)
        if eng._qat_train(lay):
            ops.fakequant_q8_w4(lay.geom_act, lay.w4c, lay.w4g, lay.wexp4, lay.w_q)

    def qat_raw(self, eng, lay, x8):
        eng._timed('fwd', lay, ops.conv_fwd_q8_w4_raw, lay.geom_act, x8, lay.w4c, lay.w4g, lay.wexp4, lay.y, lay.cout, 0, lay.stats)


_FORMS = {"dense": _Dense(), "splitk": _SplitK(), "sparse24": _Sparse24(), "bsparse": _BSparse(), "bsparse_train": _BSparseTrain(), "q8": _Q8(),
          "q8_slim": _Q8Slim(), "q8_sparse24": _Q8Sparse24(), "q8_splitk": _Q8SplitK(), "q8_w4": _Q8W4(), "q8_bsparse": _Q8BSparse()}


def _probe_side_stream(device, tries=8):
    """(stream, concurrent): see Engine._get_side_stream.
    The decision is taken from DEVICE timestamps (the candidate's kernel ended before the launch stream's burst did), not
    from a host-side query, and the ranks of one node take turns (an advisory file lock): eight processes starting at
    once on a busy host cannot turn each other's probe into a false "not concurrent" (VERDICT r03 item 5)."""
    lock = None
    try:
        import fcntl
        import tempfile
        lock = open(os.path.join(tempfile.gettempdir(), "mcamd_side_probe.lock"), "w")
        fcntl.flock(lock, fcntl.LOCK_EX)
    except Exception:
        lock = None                    # no lock file: probe anyway
    try:
        main = torch.cuda.current_stream(device)
        big = torch.empty(64 << 20, dtype=torch.float32, device=device)       # 256 MB: ~0.05 ms per pass
        tiny = torch.zeros(64, dtype=torch.float32, device=device)
        first = None
        for _ in range(tries):
            cand = torch.cuda.Stream(device)
            first = first or cand
            torch.cuda.synchronize(device)
            busy, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(80):        # ~3 ms of work queued on the launch stream
                big.fill_(1.0)
            busy.record(main)
            with torch.cuda.stream(cand):
                tiny.add_(1.0)
                done.record(cand)
            torch.cuda.synchronize(device)
            # concurrent: the candidate's kernel was done BEFORE the launch stream finished its burst (a stream that shares
            # the launch stream's hardware queue runs it behind the burst: a negative time)
            concurrent = done.elapsed_time(busy) > 0.0
            if concurrent:
                return cand, True
        return first, False
    finally:
        if lock is not None:
            try:
                import fcntl
                fcntl.flock(lock, fcntl.LOCK_UN)
                lock.close()
            except Exception:
                pass


class Engine:
    def __init__(self, model, B, H, W, device, grad_scale=256.0, precision="fp16", for_training=False, train_layout=False):
        """`precision`: "fp16" -- fp16 MFMA operands everywhere (the throughput mode); "fp16x3" -- every conv block
        multiplies split operands (x_hi*w_hi + x_lo*w_hi + x_hi*w_lo, fp32 accumulate: three fp16 MFMA products per
        multiply, ~2^-21 operand precision), activations are stored as hi | lo pairs and the raw conv output as fp32;
        "mixed" -- split operands except on the costliest blocks that the 1e-3 logit budget can afford to leave
        plain (MIXED_BUDGET; `for_training`: the budget of the training-mode forward, MIXED_BUDGET_TRAIN, under which the
        first block is split as well).  The backward pass uses plain fp16 operands in every mode.
        "fp8" -- inference only: the "fp16" engine with every eligible block on e4m3 activations and weights
        (csrc/conv_q8.hip, `fp8_layers`, _choose_q8); a training-mode forward raises.
        "fp8-2:4" -- the "fp8" engine with every fp8 block whose mask conforms to 2:4 on the sparse fp8 kernel
        (csrc/conv_q8_sparse.hip, `fp8_sparse_layers`); every other block runs what "fp8" runs.
        "fp8-splitk" -- the "fp8" engine for low batches: every block of form "q8" whose launch the split-K
        policy gives two slices or more runs the fp8 split-K pair (csrc/conv_q8_splitk.hip, `fp8_splitk_layers`); every other
        block, and every batch the policy does not split, runs exactly what "fp8" runs.  Differs from "fp8" by the order of
        the fp32 sums only.
        "fp8-qat" -- fp8 quantisation-aware training: in training mode every block of `fp8_layers` runs its
        forward in the "fp8" arithmetic on batch statistics (mcamd_conv_fwd_q8 with the fp32 raw epilogue, byte + dequantised
        fp16 destinations) and a straight-through backward on the fp16 kernels; every other block trains as in "fp16".  An
        inference-mode forward is the "fp8" engine's, bit for bit.
        "fp8-w4" -- the "fp8" engine on 4-bit weights, inference only: every block "fp8" runs in form "q8" holds
        its weights as e2m1 codes with a shift per group of 32 input channels (csrc/conv_q8_w4.hip, `fp8_w4_layers`) and
        computes what the fp8 block computes on the e4m3 bytes those codes stand for; the slim blocks and every other block
        run what "fp8" runs.
        "fp8-w4-qat" -- 4-bit quantisation-aware training: "fp8-qat" with the weights of every fp8 block in the
        4-bit format -- in training mode every block of `fp8_layers` (`fp8_w4_layers` is the same list) re-quantises its weights
        to codes, shifts and exponents every step and runs its forward on them (mcamd_conv_fwd_q8_w4_raw); the backward is
        "fp8-qat"'s on the values the codes stand for.  An inference-mode forward is the "fp8-w4" engine's, bit for bit.
        "fp8-block" -- the "fp8" engine for block-pruned models, inference only: every masked block "fp8" would
        run in form "q8" with its filters uncompacted, and whose kept fraction of (64-filter tile, 64-byte K chunk) pairs is at
        most Darknet.fp8_block_max_kept, keeps its filters out of the compaction and runs the block-sparse fp8 kernel on the
        chunks that hold a non-zero weight byte (csrc/conv_q8_bsparse.hip, `fp8_block_layers`, `fp8_block_kept`); every
        other block runs what "fp8" runs, and with nothing chosen it is the "fp8" engine bit for bit."""
        if precision not in ("fp16", "fp16x3", "mixed", "fp8", "fp8-2:4", "fp8-splitk", "fp8-qat", "fp8-w4", "fp8-w4-qat",
                             "fp8-block"):
            raise McamdError("precision must be 'fp16', 'fp16x3', 'mixed', 'fp8', 'fp8-2:4', 'fp8-splitk', 'fp8-qat', 'fp8-w4', "
                             "'fp8-w4-qat' or 'fp8-block' (got %r)" % (precision,))
        self.model, self.B, self.device = model, B, device
        self.precision = precision
        self.for_training = bool(for_training)
        self.train_layout = bool(train_layout)     # built by a model in training mode: forward(training=True) only
        self.precise = precision not in ("fp16", "fp8", "fp8-2:4", "fp8-splitk", "fp8-qat", "fp8-w4", "fp8-w4-qat", "fp8-block")
        # fp8 quantised inference (Darknet.precision = "fp8"): conv numbers of the blocks that run mcamd_conv_fwd_q8, chosen
        # when the masks change (_choose_q8); `qbufs`: buffer id -> the BYTE buffer of an activation tensor stored as e4m3
        self.q8 = precision in ("fp8", "fp8-2:4", "fp8-splitk", "fp8-qat", "fp8-w4", "fp8-w4-qat", "fp8-block")
        self.qat = precision in ("fp8-qat", "fp8-w4-qat")   # ... and their training-mode forward / straight-through backward
        self.fp8_layers = []
        # "fp8-2:4": the subset of fp8_layers whose masks conform to 2:4 and that run mcamd_conv_fwd_q8_sparse24
        self.q8_sparse = precision == "fp8-2:4"
        self.fp8_sparse_layers = []
        # "fp8-splitk": the subset of fp8_layers the split-K policy gives two slices or more and that run
        # mcamd_conv_fwd_q8_splitk (they share `_splitk_ws` below)
        self.q8_splitk = precision == "fp8-splitk"
        self.fp8_splitk_layers = []
        # "fp8-w4" / "fp8-w4-qat": the subset of fp8_layers that run on 4-bit weights (every block of form "q8": all of them in
        # a training engine, which has no slim blocks)
        self.q8_w4 = precision in ("fp8-w4", "fp8-w4-qat")
        self.fp8_w4_layers = []
        # "fp8-block": the subset of fp8_layers the block policy chose and that run mcamd_conv_fwd_q8_bsparse, and the kept-chunk
        # fraction of every candidate (conv number -> fraction); chosen when the masks, the weights or
        # Darknet.fp8_block_max_kept change (_Q8BSparse.policy; the chosen blocks share `_bs_exempt` with sparse = "block")
        self.q8_bsparse = precision == "fp8-block"
        self.fp8_block_layers = []
        self.fp8_block_kept = {}
        self.qbufs = {}
        self._qld = {}                         # buffer id -> bytes per pixel of its byte buffer (_choose_q8)
        self.grad_scale = float(grad_scale)
        self.serial = 0
        self._packed_sig = None
        self._weights_seen = None     # Darknet._weights_serial at the last pack (None: never packed)
        self.events = None            # list of (tag, layer, start, end) HIP events while profiling
        self.event_pool = None        # ... and reusable timing events a caller may hand in for them (_timed)
        # weight-gradient kernels on a second HIP stream beside the dgrad / BN-backward chain (they fill each other's
        # tails: +3.5 % images/s at B=64); MCAMD_OVERLAP_WGRAD=0 serialises everything on the launch stream (per-kernel
        # timing passes do that, bench.py)
        self.overlap_wgrad = os.environ.get("MCAMD_OVERLAP_WGRAD", "1") == "1"
        # every switch is read here, once per engine -- never inside a step
        self.wgrad_chunk = 1          # blocks per hand-over of weight gradients to the second stream (1-3 measured equal, 4+ slower)
        # launch plans (csrc/plan.hip): the layer walk of forward / backward is RECORDED once and replayed with one library
        # call per segment instead of one ctypes call per kernel launch (MCAMD_PLAN=0: the per-launch path; it is also what
        # a per-kernel timing pass uses).  Plans hold raw pointers: `_plan_epoch` counts re-plannings of the channel layout,
        # `_ptr_sig()` follows the tensors torch owns.
        self.use_plan = os.environ.get("MCAMD_PLAN", "1") == "1"
        self._fwd_plans, self._bwd_plan, self._plan_epoch = {}, None, 0
        self._logits = self._gout = self._flat = None
        self._pack_on_side = False
        # 2:4 sparse inference (Darknet.sparse = "2:4", plain-fp16 eval engines only): conv indices of the blocks that run
        # mcamd_conv_fwd_sparse24, chosen when the masks or the mode change (_choose_forms); empty = every block dense
        self.sparse_layers = []
        # block-sparse inference (Darknet.sparse = "block", plain-fp16 eval engines only): conv numbers of the blocks that run
        # mcamd_conv_fwd_bsparse, chosen when the masks, the weights or Darknet.sparse_max_kept change (_choose_forms)
        self.bsparse_layers = []
        self.bsparse_kept = {}           # conv number -> kept-chunk fraction of every candidate block
        self._bs_exempt = frozenset()    # layer indices the policy chose: their filters are not compacted (_BSparse.policy)
        # block-sparse TRAINING (Darknet.sparse_train = "block", plain-fp16 training passes only): conv numbers of
        # the blocks whose forward runs mcamd_conv_fwd_bsparse_raw, of those whose dgrad runs mcamd_conv_dgrad_bsparse too, and
        # the kept-chunk fraction of every candidate; planned once while the masks are static (`_bst_policy` caches the
        # policy's answer by mask keys and bound).  `bsparse_train_full_lists` (tests): the same kernels on full lists.
        self.bsparse_train_layers = []
        self.bsparse_train_dgrad_layers = []
        self.bsparse_train_kept = {}
        self._bst_policy = None
        self._bst_full = False
        # ... "block-wgrad" (DESIGN.md 3zd): conv numbers of the chosen blocks whose weight gradient runs the list launch
        # mcamd_conv_wgrad_bsparse, and the kept (tile, tap) fraction of every candidate (_choose_bst_wgrad)
        self.bsparse_train_wgrad_layers = []
        self.bsparse_train_wgrad_kept = {}
        self._bst_wgrad_key = None
        # split-K low-batch inference (Darknet.splitk, plain-fp16 eval engines only): conv numbers of the blocks that run
        # mcamd_conv_fwd_splitk, chosen when the flag or the masks change (_choose_forms); one workspace for all of them
        self.splitk_layers = []
        self._splitk_ws = None
        # what every block's form was last chosen for (pack): mask keys, block-sparse choice, sparse mode, sparse_max_kept,
        # split-K flag
        self._form_key = (None, None, None, None, None)
        self._training, self._fold_key = None, None
        self.fold_dead = os.environ.get("MCAMD_FOLD_DEAD", "1") == "1"
        # "mixed": the two correction products of the split-operand forward from e4m3 copies on the block-scaled fp8 MFMAs
        # (csrc/conv_igemm_pp.hip, F8).  "fp16x3" keeps all three products on fp16 operands: it is the tests' tight reference.
        self.f8 = precision == "mixed" and os.environ.get("MCAMD_F8", "1") == "1"
        self.bn_narrow_on = True      # BatchNorm / activation passes of a folded producer on its kept channels only
        self.bwd_from_act = True      # split-operand engines: BatchNorm backward of PLAIN blocks from the stored activation
        self.pool_act_on = True       # ... and of MaxPool blocks from a full-resolution copy (off with filter compaction)
        # ... and the sums of a PLAIN block's BatchNorm backward in the epilogue of the dgrad launch that stores its G
        # (mcamd_conv_dgrad_sums; MCAMD_DGRAD_BN_SUMS=0: the two-pass mcamd_bn_act_bwd everywhere)
        self.dgrad_bn_sums = os.environ.get("MCAMD_DGRAD_BN_SUMS", "1") == "1"
        # ... and a PLAIN block's BatchNorm + LeakyReLU inside the forward launch of the split-operand 1x1 block behind it
        # (mcamd_bn_act_conv1x1_fwd, _fused_1x1; MCAMD_FUSE_BN_1X1=0: activation pass + forward launch).  The counter says how
        # many such launches the layer walk has issued (recorded ones count once, when the plan is recorded).
        self.fuse_bn_1x1 = os.environ.get("MCAMD_FUSE_BN_1X1", "1") == "1"
        self.fused_1x1_launches = 0
        self._fused_1x1_cache = {}
        # ... and the whole backward of a narrow dense 1x1 block -- dgrad, its producer's BatchNorm sums, wgrad -- in one launch
        # on the launch stream (mcamd_conv_bwd1x1, _bwd1x1_route; MCAMD_BWD1X1=0: a dgrad launch + a wgrad launch on the
        # second stream).  One workspace for the blocks' weight-gradient splits, allocated once: plans hold its address.
        self.bwd1x1 = os.environ.get("MCAMD_BWD1X1", "1") == "1"
        self._bwd1x1_cache = {}
        self._bwd1x1_ws = None
        self._dgrad_sums_cache = {}
        self._side_stream = None
        self._side_concurrent = True
        self._side_ws = None
        # set by the backward kernels when a scaled gradient (grad_scale x dY / dX) had to be clamped to +-65504
        self.overflow = torch.zeros(1, dtype=torch.int32, device=device)
        self._build_plan(H, W)

    # ------------------------------------------------------------------ plan
    def _build_plan(self, H0, W0):
        model, B, dev = self.model, self.B, self.device
        blocks = model.blocks
        bops = _resolve_routes(blocks)
        n = len(bops)

        def alias(t):                      # single-layer routes are aliases
            while t >= 0 and bops[t][0] == "route" and len(bops[t][1]) == 1:
                t = bops[t][1][0]
            return t

        srcs = [[alias(s) for s in o[1]] for o in bops]
        consumers = {}
        for ind, (t, _) in enumerate(bops):
            if t == "route" and len(srcs[ind]) == 1:
                continue
            for s in srcs[ind]:
                consumers.setdefault(s, []).append(ind)

        # shapes of every tensor id
        shape = {-1: (int(blocks[0]["channels"]), H0, W0)}
        for ind, (t, _) in enumerate(bops):
            if t == "convolutional":
                c, h, w = shape[srcs[ind][0]]
                assert int(blocks[ind + 1]["stride"]) == 1, "only stride-1 convolutions (YOLOv2)"
                shape[ind] = (int(blocks[ind + 1]["filters"]), h, w)
            elif t == "maxpool":
                c, h, w = shape[srcs[ind][0]]
                if int(blocks[ind + 1]["size"]) != 2 or int(blocks[ind + 1]["stride"]) != 2:
                    raise NotImplementedError("only maxpool size=2 stride=2 is on the YOLOv2 path")
                shape[ind] = (c, h // 2, w // 2)
            elif t == "reorg":
                c, h, w = shape[srcs[ind][0]]
                assert int(blocks[ind + 1]["stride"]) == 2
                shape[ind] = (4 * c, h // 2, w // 2)
            elif t == "route":
                if len(srcs[ind]) == 1:
                    shape[ind] = shape[srcs[ind][0]]
                else:
                    (c1, h, w), (c2, h2, w2) = shape[srcs[ind][0]], shape[srcs[ind][1]]
                    assert (h, w) == (h2, w2)
                    shape[ind] = (c1 + c2, h, w)

        self._bops, self._srcs, self._shape = bops, srcs, shape
        # fusion: what each conv's activation kernel produces
        conv_inds = [i for i, (t, _) in enumerate(bops) if t == "convolutional"]
        fused = {}
        for ci in conv_inds:
            cons = consumers.get(ci, [])
            pools = [c for c in cons if bops[c][0] == "maxpool"]
            reorgs = [c for c in cons if bops[c][0] == "reorg"]
            if len(pools) == 1 and len(cons) == 1:
                fused[ci] = (L.DST_POOL, pools[0], None)
            elif len(pools) == 1 and not reorgs:
                fused[ci] = (L.DST_POOL, pools[0], ci)          # pooled + full-resolution copy (route source)
            elif len(reorgs) == 1 and len(cons) == 1:
                fused[ci] = (L.DST_REORG, reorgs[0], None)
            elif not pools and not reorgs:
                fused[ci] = (L.DST_PLAIN, ci, None)
            else:
                raise NotImplementedError("unsupported consumer pattern after conv block %d" % ci)
        for ind, (t, _) in enumerate(bops):
            if t in ("maxpool", "reorg") and not any(f[1] == ind for f in fused.values()):
                raise NotImplementedError("stand-alone %s block %d (not directly after a conv)" % (t, ind))

        # placement: concat members share one buffer
        place = {}
        self.bufs = []

        # Small images (W <= 26: the 26x26 and 13x13 tensors of YOLOv2) live in the SHARED-HALO form (include/mcamd.h): the
        # 9-tap weight gradient enumerates (H + 1)(W + 1) instead of (H + 2)(W + 2) padded pixels per image (13x13: -13 % of
        # its MFMA work, conv19's launch -19 %); every other kernel only sees a different row pitch.  Training engines only
        # (inference engines keep the padded form); since round 4 also the split-operand ones, whose backward pass is the same.
        self.shared_halo_maxw = 0
        if self.train_layout:
            self.shared_halo_maxw = 26

        def pad_for(w):
            return 1 if (w <= self.shared_halo_maxw and w >= 4) else 0

        def new_buf(Bn, h, w, ld):
            self.bufs.append(ops.alloc_padded(Bn, h, w, ld, dev, pad=pad_for(w)))
            return len(self.bufs) - 1
        self._pad_for = pad_for

        # Split activation storage of the precise modes: hi | lo planes, the consumer's third K part (x_hi * w_lo) wraps back
        # onto the hi plane (mcamd_conv_geom.x_wrap) -- when every tensor's channel count is a multiple of 32 (K blocks must
        # not straddle the wrap); otherwise (physically slim models) three planes hi | lo | hi.  The network input always has
        # three (9 channels).
        planes = 1
        if self.precise:
            chans = [shape[t][0] for ci in conv_inds for t in fused[ci][1:] if t is not None and consumers.get(t)]
            chans += [shape[srcs[i][0]][0] + shape[srcs[i][1]][0] for i, (t, _) in enumerate(bops) if t == "route" and len(srcs[i]) == 2]
            planes = 2 if all(c % 32 == 0 for c in chans) else 3
        self.act_planes = planes

        for ind, (t, _) in enumerate(bops):
            if t == "route" and len(srcs[ind]) == 2:
                a, b = srcs[ind]
                (ca, h, w), (cb, _, _) = shape[a], shape[b]
                assert ca % 8 == 0 and a not in place and b not in place
                ld = ops.round_up((ca + cb) * planes, 32)
                ps = ca + cb if self.precise else 0
                bid = new_buf(B, h, w, ld)
                place[a] = _T(bid, ld, 0, ca, h, w, ps)
                place[b] = _T(bid, ld, ca, cb, h, w, ps)
                place[ind] = _T(bid, ld, 0, ca + cb, h, w, ps)
        cin0 = shape[-1][0]
        first_k = int(blocks[conv_inds[0] + 1]["size"])
        # NHWC4 image = plain fp16 operands on the first block.  The split-operand modes give the image three planes --
        # except "mixed" when the first block runs as one fused unit (section 3e of DESIGN.md): its image and weights stay
        # plain fp16 (logits 5.2e-4 -> 5.4e-4, tools/error_budget.py), its pooled output is written unrounded as hi | lo | hi
        c0 = conv_inds[0]
        stem_block_ok = (cin0 == 3 and first_k == 3 and int(blocks[c0 + 1]["filters"]) == 32
                         and int(blocks[c0 + 1]["batch_normalize"]) and fused[c0][0] == L.DST_POOL and fused[c0][2] is None
                         and W0 % 32 == 0 and H0 % 2 == 0)
        # (not in training: there the first block's operand rounding alone costs 1.9e-2 on the logits, MIXED_BUDGET_TRAIN)
        self.stem = (cin0 == 3 and first_k == 3) and (not self.precise or (self.precision == "mixed" and stem_block_ok
                                                                          and not self.for_training))
        # "mixed" in training: the first block is the fused unit on SPLIT operands in the forward pass (two passes over the
        # hi / lo NHWC4 images, section 3e of DESIGN.md), and its BACKWARD pass is the fused first block's on plain fp16
        # operands, as every backward in every mode: that one recomputes the block from the NHWC4 hi image, so neither the
        # block's raw output nor its dY ever exists.  Its Gram context and self-consistent coefficients come from the
        # statistics half of the plain block (mcamd_stem_block_fwd with dst = NULL).
        self.stem_shadow = bool(self.precise and self.for_training and not self.stem and stem_block_ok)
        ld0 = 4 if self.stem else ops.round_up(cin0 * (3 if self.precise else 1), 32)
        place[-1] = _T(new_buf(B, H0, W0, ld0), ld0, 0, cin0, H0, W0, cin0 if (self.precise and not self.stem) else 0)
        materialized = set()
        for ci in conv_inds:
            mode, out_id, out2_id = fused[ci]
            for tid in (out_id, out2_id):
                if tid is None:
                    continue
                materialized.add(tid)
                if tid not in place and consumers.get(tid):
                    c, h, w = shape[tid]
                    ld = ops.round_up(c * planes, 32)
                    place[tid] = _T(new_buf(B, h, w, ld), ld, 0, c, h, w, c if self.precise else 0)

        # layers
        self.layers = []
        by_src = {}
        bn_names = []
        for li, ci in enumerate(conv_inds):
            blk = blocks[ci + 1]
            seq = model.models[ci]
            lay = _Layer()
            lay.index, lay.li = ci, li
            lay.conv = seq[0]
            lay.bn = seq[1] if int(blk["batch_normalize"]) else None
            lay.slope = 0.1 if blk["activation"] == "leaky" else 1.0
            if blk["activation"] not in ("leaky", "linear"):
                raise NotImplementedError("activation %r" % blk["activation"])
            src = srcs[ci][0]
            lay.src = src
            tin = place[src]
            lay.tin = tin
            lay.cin, lay.H, lay.W = shape[src]
            lay.cout = shape[ci][0]
            lay.k = int(blk["size"])
            pad = int((lay.k - 1) / 2) if int(blk["pad"]) else 0
            if pad != (lay.k - 1) // 2 or lay.k not in (1, 3):
                raise NotImplementedError("conv block %d: only 'same' 1x1/3x3 convolutions" % ci)
            lay.stem = 1 if (li == 0 and self.stem) else 0
            lay.pad = 0 if lay.stem else pad_for(lay.W)        # form of this block's padded operands (input and dY)
            lay.geom = ops.geom(B, lay.H, lay.W, lay.k, lay.cin, lay.cout, tin.ld, tin.choff, lay.stem, lay.pad)
            lay.level = 1     # operand terms of the forward product: 1 plain, 3 = x_hi*w_hi + x_lo*w_hi + x_hi*w_lo
            lay.M = B * lay.H * lay.W
            lay.mode, lay.out_id, lay.out2_id = fused[ci]
            lay.is_last = lay.bn is None
            if lay.is_last:
                if lay.slope != 1.0 or consumers.get(ci):
                    raise NotImplementedError("a conv block without batch_normalize must be the final linear block")
            else:
                if lay.cout % 8:
                    raise NotImplementedError("BN channel count %d (needs a multiple of 8)" % lay.cout)
            # the BN backward kernels keep one channel group per thread: 8 * (power of two) channels
            lay.train_ok = lay.is_last or (lay.cout // 8 <= 256 and 256 % (lay.cout // 8) == 0)
            # slim models (slim.py): constant contribution of physically removed input channels, by border class
            lay.border = getattr(lay.conv, "border_bias", None)
            if lay.border is not None:
                lay.border = lay.border.detach().to(device=dev, dtype=torch.float32).contiguous()
                if tuple(lay.border.shape) != (16, lay.cout):
                    raise McamdError("conv block %d: border_bias must be [16, %d]" % (ci, lay.cout))
                if lay.is_last:      # the fp32 NCHW epilogue has no table: added to the logits as a [1,C,H,W] map
                    hh = torch.arange(lay.H, device=dev)
                    ww = torch.arange(lay.W, device=dev)
                    cls = ((hh == 0).long() + 2 * (hh == lay.H - 1).long())[:, None] + \
                          (4 * (ww == 0).long() + 8 * (ww == lay.W - 1).long())[None, :]
                    lay.border_map = lay.border[cls.reshape(-1)].t().reshape(1, lay.cout, lay.H, lay.W).contiguous()
            by_src.setdefault(src, []).append(lay)
            self.layers.append(lay)
        for s, ls in by_src.items():
            if len(ls) > 1:
                raise NotImplementedError("tensor %d feeds %d conv blocks; one consumer conv per tensor is supported" % (s, len(ls)))
        # which conv block produces a tensor id (its pooled / reorged / plain output and the full-resolution copy)
        self.producer_of = {}
        for lay in self.layers:
            if not lay.is_last:
                self.producer_of[lay.out_id] = lay
                if lay.out2_id is not None:
                    self.producer_of[lay.out2_id] = lay
        # a concat tensor's members are consumed through the concat's consumer
        self.consumer_of = {}
        for lay in self.layers:
            self.consumer_of[lay.src] = lay
            if lay.src >= 0 and bops[lay.src][0] == "route" and len(srcs[lay.src]) == 2:
                for m in srcs[lay.src]:
                    self.consumer_of[m] = lay

        if self.precise:
            # split operands need the input tensor's three planes side by side: a channel slice of a wider buffer
            # (no such consumer on the YOLOv2 path) stays plain
            can = [lay for lay in self.layers if lay.tin.choff == 0 and lay.tin.C == lay.tin.ps and not lay.stem]
            plain = set()
            by_cost = sorted(can, key=lambda l: (-l.M * l.cout * l.cin * l.k * l.k, -l.li))
            if self.precision == "mixed" and self.for_training:
                # training: a block's term is amplified by the blocks behind it; costliest first while the
                # root-sum-square of the plain blocks' terms stays inside the budget
                nl = len(self.layers)
                term = lambda l: PLAIN_BLOCK_ERR * TRAIN_GAIN ** (nl - 1 - l.li)
                used = sum(term(l) ** 2 for l in self.layers if l not in can)       # blocks that cannot be split
                for l in by_cost:
                    if used + term(l) ** 2 > MIXED_BUDGET_TRAIN ** 2:
                        break
                    used += term(l) ** 2
                    plain.add(l.li)
            elif self.precision == "mixed":
                budget = int((MIXED_BUDGET / PLAIN_BLOCK_ERR) ** 2)        # blocks that may keep plain operands
                # (the fused first block is outside this count: only its image and weights are plain operands, its
                # output stays unrounded -- 5.21e-4 -> 5.39e-4 / 4.33e-4 -> 5.01e-4 on two seeds, tools/error_budget.py)
                unsplittable = len(self.layers) - len(can) - (1 if self.stem else 0)
                plain = set(l.li for l in by_cost[:max(0, budget - unsplittable)])
            for lay in can:
                if lay.li not in plain:
                    lay.level = 3
        f32 = dict(dtype=torch.float32, device=dev)
        wbytes = 0

        def li_is_first(l):
            return l.li == 0
        for lay in self.layers:
            g = lay.geom
            # forward geometry: the K-concatenated problem [x_hi | x_lo | x_hi] x [w_hi | w_hi | w_lo] (the packed buffer is
            # sized for it), or its fp8-correction form where the layer's kernel has one (_set_geom_f)
            wrap = 2 * lay.tin.ps if (self.act_planes == 2 and lay.li > 0) else 0      # (the network input keeps three planes)
            lay.geom_f = g if lay.level == 1 else ops.geom(B, lay.H, lay.W, lay.k, lay.level * lay.cin, lay.cout,
                                                           lay.tin.ld, 0, 0, lay.pad, wrap)
            nf, _ = ops.packed_elems(lay.geom_f)
            if self.precise:
                lay.n_act, lay.geom_act = lay.cout, g
                self._set_geom_f(lay)
            _, nd = ops.packed_elems(g)
            # zero-initialised: the one-launch packer writes real entries only (pad rows / channels stay zero)
            lay.wp = torch.zeros(nf, dtype=ops.HALF, device=dev)
            lay.wd = torch.zeros(nd, dtype=ops.HALF, device=dev) if (nd and lay.li > 0) else None
            wbytes = max(wbytes, ops.wgrad_workspace_bytes(g))
            lay.cout_p = ops.round_up(lay.cout, 32)
            # the first block as one unit (conv1 + BN + LeakyReLU + maxpool, csrc/conv_stem_block.hip): neither its raw
            # output (709 MB at B=64) nor the gradient wrt it is ever stored
            lay.fused_stem = bool(lay.stem and lay.bn is not None and lay.mode == L.DST_POOL and lay.out2_id is None
                                  and lay.cout == 32 and lay.W % 32 == 0 and lay.H % 2 == 0 and lay.border is None)
            # physically slim models keep 8 / 16 / 24 filters here: the inference-mode forward takes the same kernel
            lay.fused_stem_eval = bool(lay.stem and lay.bn is not None and lay.mode == L.DST_POOL and lay.out2_id is None
                                       and lay.cout in (8, 16, 24) and lay.W % 32 == 0 and lay.H % 2 == 0 and lay.border is None)
            lay.stem_shadow = bool(li_is_first(lay) and self.stem_shadow and lay.bn is not None and lay.mode == L.DST_POOL
                                   and lay.out2_id is None and lay.cout == 32 and lay.border is None)
            # ... and (round 4) its FORWARD pass is the fused first block too, on SPLIT operands: a statistics pass over the
            # hi / lo NHWC4 images that writes nothing but per-channel sums, then conv + BatchNorm + LeakyReLU + MaxPool
            # recomputed and written once as the pooled hi | lo planes (csrc/conv_stem_block.hip, SPLIT).  Replaces the fp32
            # first convolution's 1.4 GB raw output, its BatchNorm pass and the scratch forward of the plain block:
            # 1.16 -> 0.41 ms per B=64 step (13.85 -> 12.98 ms, A/B on one box).
            lay.stem_split = lay.stem_shadow      # (one property since round 4: forward on split operands, backward the plain block's)
            if lay.stem_shadow:
                lay.sh_img = ops.alloc_padded(B, lay.H, lay.W, 4, dev)                    # NHWC4 fp16 image
                lay.sh_geom = ops.geom(B, lay.H, lay.W, 3, 3, lay.cout, 4, 0, 1)
                lay.sh_wp = torch.zeros(ops.packed_elems(lay.sh_geom)[0], dtype=ops.HALF, device=dev)
                lay.sh_img_lo = ops.alloc_padded(B, lay.H, lay.W, 4, dev)                 # fp16(x - fp16(x))
                lay.sh_wp_lo = torch.zeros_like(lay.sh_wp)
                lay.sh_coef = [torch.empty(lay.cout, **f32) for _ in range(4)]             # scale, shift, mean, invstd
                lay.stem_ws = torch.empty(ops.stem_block_workspace_bytes(), dtype=torch.uint8, device=dev)
            lay.dy = None if (lay.fused_stem or lay.stem_shadow) else ops.alloc_padded(B, lay.H, lay.W, lay.cout_p, dev, pad=lay.pad)
            if lay.li > 0:
                lay.gin = torch.empty(lay.M * lay.tin.ld, dtype=ops.HALF, device=dev)
            lay.n_act, lay.geom_act = lay.cout, lay.geom
            if not lay.is_last:
                if lay.fused_stem:
                    lay.stem_ws = torch.empty(ops.stem_block_workspace_bytes(), dtype=torch.uint8, device=dev)
                else:
                    # The first convolution of the split-operand modes: fp32 on the vector ALUs straight from the fp32 image
                    # (csrc/conv_stem_f32.hip) instead of hi | lo | hi image planes through the generic MFMA kernel
                    # (layout 0.38 + conv 0.86 ms per B=64 step -> 0.4 ms, and exact fp32 products).
                    lay.stem_f32 = bool(self.precise and li_is_first(lay) and lay.cin == 3 and lay.k == 3 and lay.cout == 32
                                        and lay.bn is not None and not lay.stem_split)
                    # zero-initialised: with filter compaction the convolution writes the kept channels only
                    # (the split-operand fused first block never stores its raw output)
                    lay.y = None if lay.stem_split else torch.zeros(lay.M * lay.cout, dtype=torch.float32 if self.precise else ops.HALF,
                                                                    device=dev)
                    # Split-operand TRAINING engines keep y as fp32; the backward pass of a MaxPool block reads a full-resolution
                    # fp16 copy of the block's ACTIVATION instead (mcamd_act_bwd_desc.act, as the PLAIN blocks read their stored
                    # activation), which the activation pass writes beside the pooled output with the pooled element as the
                    # window's strict maximum (mcamd_act_desc.pool_act): +2 bytes per element once, -2 bytes per element in
                    # each of the two backward passes (dense B=64 step 11.69 -> 11.56 ms, A/B on one box).  NOT with filter
                    # compaction (self.pool_act_on, _update_compaction): there the weight-gradient stream is the longer one of
                    # the backward pass, the bytes saved on the launch stream buy nothing and the forward's extra write is paid
                    # (filter40: 8.29 -> 8.37 ms with it, same box)
                    if (self.bwd_from_act and self.precise and self.train_layout and lay.y is not None and lay.mode == L.DST_POOL
                            and lay.border is None and lay.slope > 0.0):
                        lay.act_full = ops.alloc_padded(B, lay.H, lay.W, ops.round_up(lay.cout, 8), dev, pad=pad_for(lay.W))
                    if lay.stem_split:
                        lay.stats = torch.zeros(ops.stem_block_stats_rows(B, lay.H, lay.W), 2, ops.round_up(lay.cout, 256), **f32)
                    elif lay.stem_f32:
                        lay.stats = torch.zeros(ops.stem_conv_f32_stats_rows(), 2, ops.round_up(lay.cout, 256), **f32)
                        lay.weff = torch.empty(lay.cout * 27, **f32)
                    else:
                        lay.stats = torch.zeros(ops.stats_rows(lay.geom_f, L.EPI_RAW_F32 if self.precise else L.EPI_RAW_F16), 2,
                                                ops.round_up(lay.cout, 256), **f32)
                lay.scale, lay.shift, lay.mean, lay.invstd = (torch.empty(lay.cout, **f32) for _ in range(4))
                lay.out_t = place.get(lay.out_id)
                lay.out2_t = place.get(lay.out2_id) if lay.out2_id is not None else None
                if lay.out_t is None:
                    raise NotImplementedError("conv block %d output is never consumed" % lay.index)
        self.wgrad_ws = torch.empty(max(wbytes, 16), dtype=torch.uint8, device=dev)
        self._pack_key, self._pack_table, self._pack_keep = None, None, []
        # filter compaction + dead-input folding; since round 4 also in the split-operand engines (two-plane storage)
        self.compact = os.environ.get("MCAMD_COMPACT", "1") == "1" and (not self.precise or self.act_planes == 2)
        self.fuse_eval = os.environ.get("MCAMD_FUSE_EVAL", "1") == "1"
        self.compact_gran = 0         # granularity of a compacted filter count: 0 = 64, or 8 below 128 filters
        maxc = max(l.cout for l in self.layers)
        self.bwd_ws = torch.empty(ops.bn_act_bwd_workspace_bytes(maxc), dtype=torch.uint8, device=dev)
        self.params = list(model.parameters())
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += p.numel()
        self.total_params = off
        # slice of the flat gradient each conv block owns (its conv + BN parameters are adjacent in
        # model.parameters(), nets.py:798-815): [p_lo, p_hi) tile [0, total) in layer order
        offs = {id(p): (o, p.numel()) for p, o in zip(self.params, self.offsets)}
        for lay in self.layers:
            own = [lay.conv.weight] + ([lay.conv.bias] if lay.conv.bias is not None else [])
            if lay.bn is not None:
                own += [lay.bn.weight, lay.bn.bias]
            lay.p_lo = min(offs[id(p)][0] for p in own)
            lay.p_hi = max(offs[id(p)][0] + offs[id(p)][1] for p in own)
        edge = 0
        for lay in self.layers:
            if lay.p_lo != edge:
                raise NotImplementedError("parameters outside the conv blocks (offset %d)" % edge)
            edge = lay.p_hi
        if edge != off:
            raise NotImplementedError("parameters outside the conv blocks (tail)")
        self.out_shape = (B, self.layers[-1].cout, self.layers[-1].H, self.layers[-1].W)

    # ------------------------------------------------------------------ second stream
    _SIDE_STREAMS = {}      # device index -> (stream, concurrent?)  one per process: every engine of a device shares it

    def _get_side_stream(self):
        """The second HIP stream (weight gradients, fold + re-pack) -- one that really runs BESIDE the launch stream.
        HIP multiplexes its streams onto a few hardware queues (4 by default) in creation order, and a stream that lands
        on the launch stream's queue is silently serialised behind it: with a process group alive (RCCL creates streams
        of its own first) exactly that happened -- rocprofv3 showed every kernel of both streams on one queue id and the
        step went from 9.7 to 10.7 ms (profiles/r02c_*).  So candidates are probed: a few milliseconds of work are queued
        on the launch stream, one tiny kernel on the candidate; the candidate is concurrent if its kernel is done while
        the launch stream is still busy.  The first concurrent candidate of up to eight is kept for the process."""
        key = self.device.index if self.device.index is not None else torch.cuda.current_device()
        if self._side_stream is None:
            hit = Engine._SIDE_STREAMS.get(key)
            if hit is None:
                hit = _probe_side_stream(self.device)
                Engine._SIDE_STREAMS[key] = hit
            self._side_stream = hit[0]
            self._side_concurrent = hit[1] is not False      # (None = not probed: assumed concurrent)
        return self._side_stream

    # ------------------------------------------------------------------ per-kernel timing
    def _timed(self, tag, lay, fn, *args, **kw):
        """Run one library call; when profiling, bracket it with HIP events on the launch stream."""
        if self.events is None:
            return fn(*args, **kw)
        # (events come from a pool the caller may hand in -- `self.event_pool`, a list of reusable timing events -- so that a
        # long instrumented pass does not keep hundreds of profiling signals alive; the host-side seconds of the three
        # parts [record, call, record] are kept next to the pair: a GPU-side gap with a long host part is a HOST stall)
        pool = self.event_pool
        if pool:
            e0, e1 = pool.pop(), pool.pop()
        else:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        t1 = time.perf_counter()
        r = fn(*args, **kw)
        t2 = time.perf_counter()
        e1.record()
        t3 = time.perf_counter()
        self.events.append((tag, lay, e0, e1, (t1 - t0, t2 - t1, t3 - t2)))
        return r

    def conv_flops(self, lay):
        """Algorithmic FLOPs of one forward conv launch (2 * M * Cout * Cin * k*k, unpadded); with filter
        compaction Cout is the number of filters the launch actually computes."""
        return 2.0 * lay.M * lay.n_act * (lay.fold_aug if lay.fold is not None else lay.cin) * lay.k * lay.k

    # ------------------------------------------------------------------ weights
    def _signature(self):
        sig = []
        for lay in self.layers:
            w = lay.conv.weight
            m = lay.conv.mask if lay.conv.mask_flag else None
            bnv = None
            if lay.fold is not None and self._training is False:
                # eval: the folded constants beta - running_mean * gamma / sqrt(running_var + eps) are baked into the
                # augmented weights -- an in-place change of the producer's BatchNorm tensors (dp.sync_buffers,
                # running_mean.copy_, load_state_dict) must trigger a re-pack
                bn = lay.fold.bn
                bnv = tuple(t._version for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
            sig.append((w.data_ptr(), w._version, None if m is None else (m.data_ptr(), m._version), bnv))
        return tuple(sig)

    def pack(self, force=False, training=True, sparse=None, splitk=False, max_kept=None, wgrad_max_kept=None):
        """fp32 master * mask -> fp16 kernel layouts (replaces layers.py:59's per-forward multiply).
        `sparse`, `splitk`, `max_kept`: the inference options forward() validated (Darknet.sparse / splitk /
        sparse_max_kept; off in training mode); every block's form is chosen again when they or the masks change.
        `wgrad_max_kept` (sparse = "block-train" only; None: off): Darknet.sparse_train = "block-wgrad"."""
        if any(lay.fold is not None for lay in self.layers) and training != self._training:
            force = True          # the folded constants differ between batch and running statistics
        self._training = training
        sig = self._signature()
        # "the model says its weights were replaced" is per engine: Darknet._weights_dirty is cleared by the first engine
        # that packs, Darknet._weights_serial counts every time it was raised -- an eval engine must re-pack after
        # invalidate_packed() although the training engine packed first, and an engine's first pack (a second training
        # engine after grad_scale was halved) must not keep the static default exponents
        serial = self.model._weights_serial
        dirty = self.model._weights_dirty or serial != self._weights_seen
        if not force and sig == self._packed_sig and (sparse, max_kept, splitk) == self._form_key[2:] and not dirty:
            return
        if dirty or (self.f8 and self.serial % 1000 == 999):      # (and every 1 000th forward: slow drift)
            self._refresh_f8_wexp()
        mkeys = tuple(None if not lay.conv.mask_flag else (lay.conv.mask.data_ptr(), lay.conv.mask._version)
                      for lay in self.layers)
        # (Darknet.sparse = "block": the blocks the policy chose keep their dense filter layout, so the compaction plan
        # depends on that choice too; it is the empty set in every other mode)
        exempt = frozenset()
        if sparse == "block":
            exempt, self.bsparse_kept = _FORMS["bsparse"].policy(self, max_kept)
        elif sparse == "block-train":       # (Darknet.sparse_train; re-packed every step: one host read per set of masks)
            pkey = (mkeys, max_kept) + ((True,) if wgrad_max_kept is not None else ())
            if self._bst_policy is None or self._bst_policy[0] != pkey:
                self._bst_policy = (pkey,) + _FORMS["bsparse_train"].policy(self, max_kept, wgrad=wgrad_max_kept is not None)
            exempt, self.bsparse_train_kept = self._bst_policy[1:]
        elif self.q8_bsparse and max_kept is not None:
            exempt, self.fp8_block_kept = _FORMS["q8_bsparse"].policy(self, max_kept)
        key = (mkeys, exempt, sparse, max_kept, splitk)
        if key != self._form_key:          # masks are static during retraining: planned once
            self._choose_forms(key)
        # (the list weight gradient follows the forms: chosen again when they, the masks -- part of the form key -- or its
        # bound change, from the counters the policy read; None in every mode but "block-wgrad")
        wkey = (key, wgrad_max_kept) if sparse == "block-train" and wgrad_max_kept is not None else None
        if wkey != self._bst_wgrad_key:
            self._choose_bst_wgrad(None if wkey is None else wgrad_max_kept)
            self._bst_wgrad_key = wkey
        # geom_act / g_rows / g_cols: physical channel order (kept filters first, permuted inputs); identity = None.
        # Split-operand engines: forward = fp16 of [w_hi | w_hi | w_lo] along the input channels (w_hi = fp16(w * mask),
        # w_lo = fp16(w * mask - w_hi)), matching the [x_hi | x_lo | x_hi] activation planes, written by the one-launch
        # packer itself (mcamd_pack_job.split); dgrad = the plain fp16 packing (the backward pass multiplies plain operands)
        # (the forms are chosen in front of the job table: it names the fp8 blocks' w_q)
        tkey = tuple((s_[0], None if s_[2] is None else s_[2][0]) for s_ in sig)
        if tkey != self._pack_key:          # weight / mask storage moved, or the compaction changed: new job table
            jobs, self._pack_keep = [], []
            for lay in self.layers:
                w = lay.conv.weight.data
                if w.dtype != torch.float32 or not w.is_contiguous():
                    raise McamdError("conv weights must be contiguous fp32 (master copy)")
                mask = lay.conv.mask if lay.conv.mask_flag else None
                if mask is not None and not mask.is_contiguous():
                    raise McamdError("conv masks must be contiguous")
                if lay.stem:
                    continue
                self._pack_keep += [w, mask]
                split = 2 if lay.f8 else (1 if lay.level == 3 else 0)      # mcamd_pack_job.split
                if lay.fold is not None:     # augmented weights (kept inputs + the folded ones-channel), rebuilt per step
                    jobs.append(dict(w=lay.waug, mask=None, rows=None, cols=None, cout=lay.n_act, cin=lay.fold_aug,
                                     ksize=lay.k, dst_fwd=lay.wp, dst_dgrad=lay.wd, split=split, f8_wexp=lay.f8_wexp_eff))
                    continue
                if self._qat_train(lay):     # straight-through backward: the dgrad operand is fp16(w_q) (no mask: it is in w_q)
                    jobs.append(dict(w=lay.w_q, mask=None, rows=None, cols=None, cout=lay.cout, cin=lay.cin, ksize=lay.k,
                                     dst_fwd=None, dst_dgrad=lay.wd, split=0))
                    continue
                jobs.append(dict(w=w, mask=mask, rows=lay.g_rows, cols=lay.g_cols, cout=lay.n_act, cin=lay.cin, ksize=lay.k,
                                 dst_fwd=lay.wp, dst_dgrad=lay.wd, split=split, f8_wexp=lay.f8_wexp_eff))
            self._pack_table = ops.pack_table(jobs, self.device) if jobs else None
            self._pack_key = tkey
        for lay in self.layers:
            mask = lay.conv.mask.contiguous() if lay.conv.mask_flag else None
            if lay.form != "dense":
                _FORMS[lay.form].pack(self, lay, lay.conv.weight.data, mask)
            if lay.stem:
                ops.pack_weights(lay.geom_act, lay.conv.weight.data, mask, True, False, lay.wp, None, rows=lay.g_rows)
            if lay.stem_split:          # hi and lo stem packings of the split-operand fused first block
                ops.pack_stem_split(lay.conv.weight.data, mask, lay.sh_wp, lay.sh_wp_lo)
        # The layers behind the first block are not needed until that block's forward is done: with folded layers
        # (filter masks) their fold + re-pack runs on the second stream under the first block's Gram / forward kernels and
        # forward() makes the launch stream wait for it in front of the second block (self._pack_event): 7.17 -> 7.10 ms
        # per filter-pruned step.  Dense: the lone re-pack launch gains nothing from it (9.69 vs 9.73 ms), so it stays on
        # the launch stream.
        self._pack_on_side = False
        side = None
        if (training and self.overlap_wgrad and self.events is None and self.layers[0].fused_stem
                and any(lay.fold is not None for lay in self.layers)):
            main = torch.cuda.current_stream(self.device)
            side = self._get_side_stream()
            side.wait_stream(main)            # the optimizer step that produced these weights
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            folds = [lay for lay in self.layers if lay.fold is not None]
            if folds and self._training:
                # training: the folded constants are leaky(beta) of the producers' own parameter tensors -> one launch for
                # all layers through a cached job table (the table holds pointers: rebuilt when a tensor moved)
                fkey = tuple((lay.conv.weight.data_ptr(), lay.fold.bn.bias.data_ptr(),
                              lay.conv.mask.data_ptr() if lay.conv.mask_flag else 0) for lay in folds)
                if fkey != self._fold_key:
                    self._fold_table = ops.fold_table([dict(w=lay.conv.weight.data, mask=lay.conv.mask if lay.conv.mask_flag else None,
                                                            rows=lay.g_rows, cols=lay.g_cols, beta=lay.fold.bn.bias.data,
                                                            slope=lay.fold.slope, n=lay.n_act, cin_k=lay.fold_cin, waug=lay.waug)
                                                       for lay in folds], self.device)
                    self._fold_key = fkey
                ops.fold_many(*self._fold_table)
            else:
                for lay in folds:       # eval: the constants come from the running statistics (a temporary per forward)
                    mask = lay.conv.mask if lay.conv.mask_flag else None
                    ops.fold_weights(lay.conv.weight.data, mask, lay.g_rows, lay.g_cols, self._fold_constants(lay.fold, False),
                                     lay.fold.slope, lay.n_act, lay.fold_cin, lay.waug)
            if self._pack_table is not None:
                ops.pack_many(*self._pack_table)
            if side is not None:
                self._pack_on_side = True      # forward() makes the launch stream wait for the second one before block 2
            # what a form derives from the packed weights (the chunk lists): on the stream the re-pack ran on, behind it.
            # Only blocks behind the first one take such a form, so the wait in front of block 2 orders their launches
            # behind these as it orders them behind the re-pack.
            for lay in self.layers:
                if lay.form != "dense":       # (_inner: lay.li > 0)
                    _FORMS[lay.form].repacked(self, lay)
        self._packed_sig = sig
        self._weights_seen = serial
        self.model._weights_dirty = False

    # ------------------------------------------------------------------ inference forms
    def _fused_eval(self, lay, border_ok=False, compacted=True):
        """Does this block take the fused inference path (BN + LeakyReLU [+ pool / reorg] in the conv epilogue)?
        `border_ok`: also with a border table (slim models) -- the fp8 epilogue adds it (_choose_q8), the fp16 ones do not.
        `compacted=False`: whatever the filter compaction made of it (_eligible)."""
        return (self.fuse_eval and not self.precise and not lay.is_last and (lay.perm is None or not compacted)
                and (border_ok or lay.border is None)
                and (lay.out2_t is None or lay.mode == L.DST_POOL)
                and (lay.mode == L.DST_PLAIN or (lay.H % 2 == 0 and lay.W % 2 == 0)))

    def _inner(self, lay):
        """Neither the first block (nor a stem in any form) nor the last one."""
        return lay.li > 0 and not lay.stem and not lay.is_last

    def _eligible(self, lay, border_ok=False, compacted=True):
        """Can this block leave the dense launch?  It is neither the first nor the last block, takes the fused inference
        path, and its filters are not compacted, its inputs neither permuted nor folded.
        `border_ok`: a border table is acceptable (slim fp8).  `compacted=False`: the compaction state is ignored -- for the
        block-sparse policy, which runs in front of the compaction and exempts the blocks it picks from it."""
        return (self._inner(lay) and self._fused_eval(lay, border_ok, compacted)
                and (not compacted or (lay.fold is None and lay.g_cols is None)))

    def _bst_eligible(self, lay, compacted=True):
        """Can this block train on the block-sparse kernel (form "bsparse_train")?  An inner block of the plain-fp16 engine
        with a BatchNorm and a raw fp16 output whose geometry mcamd_conv_bsparse_train_ok accepts; `compacted` (behind the
        compaction plan): and no fold, gather or perm, on itself or forced on it by its producer."""
        ok = (self.precision == "fp16" and self._inner(lay) and lay.bn is not None and lay.y is not None
              and lay.y.dtype == torch.float16 and lay.geom is not None and ops.conv_bsparse_train_ok(lay.geom))
        if ok and compacted:
            ok = (lay.fold is None and not lay.gather and lay.perm is None and lay.in_perm is None and lay.geom_act is lay.geom
                  and not lay.fold_consumers and not lay.skip_dead)
        return ok

    bsparse_train_full_lists = property(lambda self: self._bst_full)

    @bsparse_train_full_lists.setter
    def bsparse_train_full_lists(self, on):
        if bool(on) != self._bst_full:
            self._bst_full = bool(on)
            self._plan_epoch += 1            # recorded plans hold the lists' addresses

    def _choose_bst_wgrad(self, bound):
        """Which blocks send their weight gradient through the list launch (Darknet.sparse_train = "block-wgrad", DESIGN.md
        3zd), behind _choose_forms and from the counters _BSparseTrain.policy read: no launch and no host read here.  A block
        is chosen when it took form "bsparse_train", has no gather, perm or fold, is not on the one-launch 1x1 backward, its
        geometry has a list launch and its kept (tile, tap) fraction is at most `bound`.  The split count of each plan and the
        split-K workspaces (this stream's and the second one's) are settled here.  bound None: nothing is chosen."""
        self._plan_epoch += 1
        chosen, kept, wbytes = [], {}, 0
        for lay in self.layers:
            lay.bw_on = False
            if bound is None or lay.bw_counts is None:
                continue
            ntiles, npairs = lay.bw_counts
            kept[lay.li + 1] = npairs / float(ops.wgrad_bsparse_elems(lay.geom)[0] * lay.k * lay.k)
            if (lay.form == "bsparse_train" and not lay.gather and lay.perm is None and lay.fold is None
                    and not self._bwd1x1_route(lay) and kept[lay.li + 1] <= bound):
                plan = ops.conv_wgrad_bsparse_plan(lay.geom, ntiles)
                lay.bw_on, lay.bw_nsplit, lay.bw_bytes = True, plan.nsplit, plan.bytes
                wbytes = max(wbytes, plan.bytes)
                chosen.append(lay.li + 1)
        if wbytes > self.wgrad_ws.numel():
            self.wgrad_ws = torch.empty(wbytes, dtype=torch.uint8, device=self.device)
        if self._side_ws is not None and self._side_ws.numel() < self.wgrad_ws.numel():
            self._side_ws = torch.empty(self.wgrad_ws.numel(), dtype=torch.uint8, device=self.device)
            self._side_ws.record_stream(self._get_side_stream())
        if self._training:
            self.bsparse_train_wgrad_layers, self.bsparse_train_wgrad_kept = chosen, kept

    def _conforming(self, cand):
        """The blocks of `cand` whose mask keeps at most 2 of every 4 consecutive input channels at each (filter, tap):
        checked on the device, one pass per candidate and ONE host read for all."""
        if not cand:
            return []
        counts = torch.zeros(len(cand), dtype=torch.int32, device=self.device)
        for i, lay in enumerate(cand):
            ops.nm_violations(lay.conv.mask.contiguous(), counts[i:i + 1])
        return [lay for lay, bad in zip(cand, counts.cpu().tolist()) if not bad]

    def _choose_forms(self, key):
        """Every block's inference form (`_Layer.form`, exactly one of _FORMS), chosen when `key` changes: the mask keys,
        the block-sparse policy's choice, Darknet.sparse, sparse_max_kept and Darknet.splitk (pack).  In this order:
          1. (pack) the block-sparse policy (sparse = "block", or _Q8BSparse.policy under "fp8-block": there a chosen block that
             _choose_q8 then gives form "q8" takes "q8_bsparse") has read the masked weights; the blocks it chose are exempt from
          2. filter compaction and folding, planned again when the masks or that choice changed;
          3. then fp8 (every eligible block of an fp8 engine; under "fp8-splitk" behind it: every block of form "q8" -- not the
             slim ones -- whose launch the split-K policy gives two slices or more, mcamd_conv_fwd_q8_splitk_info; under
             "fp8-w4" every block of form "q8" takes the 4-bit form "q8_w4"), 2:4
             (sparse = "2:4": every eligible block whose mask conforms and whose geometry mcamd_conv_fwd_sparse24_ok accepts)
             or block-sparse (sparse = "block": the chosen blocks that
             are still eligible -- one whose producer was compacted after all, so that its input channels are permuted, stays
             dense), which depend on perm / g_cols / fold -- and all of it in front of the pack job table, which names w_q of
             an fp8-qat training block;
          4. split-K last: it only takes blocks that are still dense -- sparse and block-sparse blocks are never split --
             and does when the library's policy gives the block's eval-mode launch two slices or more
             (mcamd_conv_fwd_splitk_info).
        Every other block stays dense.  The `*_layers` lists are the conv numbers (conv1 = the first block) per form."""
        mkeys, exempt, sparse, max_kept, splitk = key
        self._plan_epoch += 1             # recorded plans name each block's launch and hold its operands' addresses
        if (mkeys, exempt) != self._form_key[:2]:
            self._bs_exempt = exempt
            self._update_compaction()
            self._pack_key = None
            for lay in self.layers:          # the packed shapes may have shrunk: stale entries must not survive
                lay.wp.zero_()
                if lay.wd is not None:
                    lay.wd.zero_()
        for lay in self.layers:
            lay.form, lay.sk_slices = "dense", 1
            lay.q8_y, lay.q8_y2, lay.xq, lay.geom_q8 = False, False, None, lay.geom_act
            if lay.y_f16 is not None:        # (an fp8-qat training block: back to its fp16 raw output and statistics)
                lay.y, lay.stats = lay.y_f16, lay.stats_f16
        if sparse != "block":
            self.bsparse_kept = {}
        if self.q8:
            self._choose_q8()
            self._pack_key = None
            if self.q8_splitk:
                for lay in self.layers:
                    if lay.form != "q8" or lay.geom_q8.pad:
                        continue
                    info = ops.conv_fwd_q8_splitk_info(lay.geom_q8, lay.mode)
                    if info.slices >= 2:
                        lay.form, lay.sk_slices = "q8_splitk", info.slices
            if self.q8_bsparse:          # (a chosen block whose input was permuted or folded after all did not get form "q8")
                for lay in self.layers:
                    if lay.li in exempt and lay.form == "q8" and ops.conv_fwd_q8_bsparse_ok(lay.geom_q8):
                        lay.form = "q8_bsparse"
            if self.q8_w4:               # (the slim blocks keep their form, as under "fp8-splitk")
                for lay in self.layers:
                    if lay.form == "q8" and ops.conv_fwd_q8_w4_ok(lay.geom_q8):
                        lay.form = "q8_w4"
        elif sparse == "2:4":
            for lay in self._conforming([lay for lay in self.layers
                                         if self._eligible(lay) and lay.conv.mask_flag and lay.cin % 4 == 0
                                         and lay.conv.mask.shape == lay.conv.weight.shape
                                         and ops.conv_fwd_sparse24_ok(lay.geom_act)]):
                lay.form = "sparse24"
        elif sparse == "block":
            for lay in self.layers:
                if lay.li in exempt and self._eligible(lay):
                    lay.form = "bsparse"
        elif sparse == "block-train":
            for lay in self.layers:          # (a chosen block whose producer was compacted after all stays dense)
                if lay.li in exempt and self._bst_eligible(lay):
                    lay.form = "bsparse_train"
        if splitk:
            for lay in self.layers:
                launch = self._splitk_form(lay)
                if launch is None or lay.geom_act.pad:
                    continue
                info = ops.conv_fwd_splitk_info(lay.geom_act, launch[0], launch[1])
                if info.slices >= 2:
                    lay.form, lay.sk_slices = "splitk", info.slices
        by_form = {}
        for lay in self.layers:
            by_form.setdefault(lay.form, []).append(lay)
        for name, lays in by_form.items():
            _FORMS[name].alloc(self, lays)
        nums = lambda *names: [lay.li + 1 for lay in self.layers if lay.form in names]
        self.sparse_layers, self.bsparse_layers, self.splitk_layers = nums("sparse24"), nums("bsparse"), nums("splitk")
        self.fp8_layers = nums("q8", "q8_slim", "q8_sparse24", "q8_splitk", "q8_w4", "q8_bsparse")
        self.fp8_block_layers = nums("q8_bsparse")
        if self._training:                   # (what the last training-mode choice was; an eval pass in between keeps it)
            self.bsparse_train_layers = nums("bsparse_train")
            self.bsparse_train_dgrad_layers = [lay.li + 1 for lay in self.layers if lay.form == "bsparse_train" and lay.bs_dgrad]
            if sparse != "block-train":
                self.bsparse_train_kept = {}
        self.fp8_sparse_layers, self.fp8_splitk_layers, self.fp8_w4_layers = nums("q8_sparse24"), nums("q8_splitk"), nums("q8_w4")
        self._form_key = key

    def _splitk_form(self, lay):
        """(epilogue mode, dst_mode) of the eval-mode launch of a block the split-K pair can stand in for, or None: the fused
        inference launch (ops.conv_fwd_padded) or the raw one without statistics (ops.conv_fwd_raw: blocks with a border
        table, a permutation or folding -- how slim_export models run in fp16)."""
        if not self._inner(lay) or lay.form not in ("dense", "splitk") or self.precise or self.q8:
            return None
        return (L.EPI_PAD_F16, lay.mode) if self._fused_eval(lay) else (L.EPI_RAW_F16, L.DST_PLAIN)

    # ------------------------------------------------------------------ fp8 quantised inference
    def _choose_q8(self):
        """Which blocks of an fp8 engine run an fp8 forward, and which tensors are held as bytes (step 3 of _choose_forms): a
        block does when it is eligible (_eligible), has a multiple of 64 input channels and no border table, and
        mcamd_conv_fwd_q8_ok accepts its geometry.  Every other block runs what the "fp16"
        engine runs.  An activation buffer holds e4m3 bytes when EVERY block that reads it (a concat member can have a
        reader of its own beside the concat's) and every block that writes into it are fp8 blocks: one format per tensor.
        Otherwise the buffer stays fp16 and an fp8 block that reads it takes a private byte copy that a cast pass
        (mcamd_cast_q8) writes in front of it.
        Precision "fp8-2:4": an fp8 block whose mask is present with the weight's shape and keeps at most 2 of every 4
        consecutive input channels at each (filter, tap) (_conforming) runs
        the sparse fp8 kernel (`fp8_sparse_layers`); formats and buffers do not depend on that.
        Slim models (a model some conv of which carries a border table; not under "fp8-qat"): a block with a
        border table and / or an input channel count that is
        no multiple of 64 becomes an fp8 block on mcamd_conv_fwd_q8_slim when it meets the other conditions above,
        mcamd_conv_fwd_q8_slim_ok accepts it and round_up(cin, 64) <= 2 cin; it always runs the dense fp8 kernel.  Its K
        loop reads round_up(cin, 64) bytes per pixel and tap, so a byte buffer's leading dimension (`_qld`, the private
        copies' too) is raised until that span lies inside it for every fp8 reader; the bytes behind a tensor's channels are
        allocated 0x00 and never written."""
        dev = self.device
        # "fp8-qat" training engines keep their small images in the shared-halo form (both kernels read it); the set of
        # blocks is the inference engine's: the same predicate on everything that does not depend on the layout
        qat_train = self.qat and self.train_layout
        # the slim form is for slim_export models (some conv carries a border table): every other model keeps the set it
        # had -- conv2 of the dense YOLOv2 (32 input channels, no table) stays an fp16 block
        slim_model = not self.qat and any(lay.border is not None for lay in self.layers)
        for lay in self.layers:
            if lay.pad and not qat_train:
                continue
            if lay.cin % 64 == 0 and self._eligible(lay) and ops.conv_fwd_q8_ok(lay.geom_act):
                lay.form = "q8"
            elif (slim_model and (lay.border is not None or lay.cin % 64 != 0) and self._eligible(lay, border_ok=True)
                  and ops.round_up(lay.cin, 64) <= 2 * lay.cin and ops.conv_fwd_q8_slim_ok(self._q8_geom(lay))):
                lay.form = "q8_slim"
        if self.q8_sparse:
            for lay in self._conforming([lay for lay in self.layers
                                         if lay.form == "q8" and lay.conv.mask_flag
                                         and lay.conv.mask.shape == lay.conv.weight.shape
                                         and ops.conv_fwd_q8_sparse24_ok(lay.geom_act)]):
                lay.form = "q8_sparse24"
        writers = {}                      # buffer id -> the blocks that write into it
        for lay in self.layers:
            if not lay.is_last:
                for t in (lay.out_t, lay.out2_t):
                    if t is not None:
                        writers.setdefault(t.buf, []).append(lay)
        readers = {}                      # buffer id -> the blocks that read it (a concat member may have a reader of its own)
        for lay in self.layers:
            readers.setdefault(lay.tin.buf, []).append(lay)
        live = set()
        for lay in self.layers:
            if not lay.q8_on:
                continue
            t = lay.tin
            ws = writers.get(t.buf, [])
            shared = bool(ws) and all(w.q8_on for w in ws) and all(r.q8_on for r in readers[t.buf])
            # bytes per pixel of the buffer this block reads: wide enough for every fp8 reader's K loop (t.ld unless a
            # reader's round_up(cin, 64) channels reach past it)
            qld = max(self._q8_ld(r) for r in readers[t.buf]) if shared else self._q8_ld(lay)
            if qld != t.ld or lay.q8_slim:
                lay.geom_q8 = self._q8_geom(lay, qld)
            if shared:
                live.add(t.buf)
                if t.buf not in self.qbufs or self._qld.get(t.buf) != qld:
                    self.qbufs[t.buf] = ops.alloc_padded_q8(self.B, t.H, t.W, qld, dev, pad=self._pad_for(t.W))
                    self._qld[t.buf] = qld
            else:
                if qat_train and readers[t.buf] != [lay]:
                    # the training cast writes the dequantised values back over the fp16 slice, which is safe only when
                    # this block is the buffer's one reader (forward and weight gradient)
                    raise NotImplementedError("fp8-qat: conv%d reads an fp16 tensor that another block reads too"
                                              % (lay.li + 1))
                key = (self.B, t.H, t.W, qld)
                if lay._xq_key != key:
                    lay._xq, lay._xq_key = ops.alloc_padded_q8(self.B, t.H, t.W, qld, dev, pad=self._pad_for(t.W)), key
                lay.xq = lay._xq
            if qat_train:
                # fp32 raw output + its statistics slab (the fp16 ones come back when the block leaves the set), and w_q
                if lay.y_f16 is None:
                    lay.y_f16, lay.stats_f16 = lay.y, lay.stats
                    lay.y_f32 = torch.zeros(lay.M * lay.cout, dtype=torch.float32, device=dev)
                    lay.stats_q8 = torch.zeros(ops.conv_fwd_q8_stats_rows(lay.geom_act), 2, ops.round_up(lay.cout, 256),
                                               dtype=torch.float32, device=dev)
                    lay.w_q = torch.zeros_like(lay.conv.weight.data)
                lay.y, lay.stats = lay.y_f32, lay.stats_q8
        for b in [b for b in self.qbufs if b not in live]:
            del self.qbufs[b]
            self._qld.pop(b, None)
        for lay in self.layers:
            if lay.q8_on:
                lay.q8_y = lay.out_t.buf in self.qbufs
                lay.q8_y2 = lay.out2_t is not None and lay.out2_t.buf in self.qbufs

    def _q8_ld(self, lay):
        """Bytes per pixel a byte buffer needs for this block to read its input from it: the fp16 buffer's leading dimension,
        or more when the round_up(cin, 64) channels of the block's K loop (slim models) reach past it."""
        return max(lay.tin.ld, ops.round_up(lay.tin.choff + ops.round_up(lay.cin, 64), 16))

    def _q8_geom(self, lay, ld=None):
        """Geometry of this block's fp8 launch on a byte buffer of `ld` bytes per pixel (default: _q8_ld)."""
        return ops.geom(self.B, lay.H, lay.W, lay.k, lay.cin, lay.cout, ld if ld is not None else self._q8_ld(lay),
                        lay.tin.choff, 0, lay.pad)

    def _q8_tld(self, t, f8):
        """Leading dimension of tensor `t` in the buffer a launch addresses: the byte buffer's (`f8`) or the fp16 one's."""
        return self._qld[t.buf] if f8 else t.ld

    def _qat_train(self, lay):
        """Does this block train in the fp8 arithmetic (a block of fp8_layers in an "fp8-qat" / "fp8-w4-qat" training engine)?"""
        return self.qat and self.train_layout and lay.q8_on

    def qat_block_io(self, conv_number):
        """Debug accessor of an "fp8-qat" training engine: what fp8 block `conv_number` read and wrote in the last training
        step, from the engine's own buffers, as CPU tensors (NCHW) -- `x8` input codes and `x16` the fp16 values beside them;
        `y` the fp32 raw output; batch `scale` / `shift` / `mean` / `invstd`; `out8` (`out2_8`) output codes where the
        destination is held as bytes, else None, and `out16` (`out2_16`) the fp16 buffer of the same tensor; `dst`;
        `dy` the gradient wrt y times grad_scale (after a backward); `w_q` the weights the dgrad operand was packed from,
        `wexp` their exponents; `gin` the gradient wrt the block's input slice times grad_scale.  A 4-bit block ("fp8-w4-qat")
        adds `codes` [cout][ktot / 2] and `gshift` [ktot / 64][cout][2], the packed operands of its forward (`wexp` = e4_f)."""
        lay = self.layers[conv_number - 1]
        if not self._qat_train(lay):
            raise McamdError("conv%d is not an fp8 block of an fp8-qat training engine (fp8_layers = %r)"
                             % (conv_number, self.fp8_layers))
        B, interior = self.B, self._interior
        t, t2, ti = lay.out_t, lay.out2_t, lay.tin
        cdst = 4 * lay.cout if lay.mode == L.DST_REORG else lay.cout
        out = dict(x8=interior(lay.xq if lay.xq is not None else self.qbufs[ti.buf], True, ti, lay.cin, lay.geom_q8.x_ld),
                   x16=interior(self.bufs[ti.buf], False, ti, lay.cin),
                   y=lay.y.view(B, lay.H, lay.W, lay.cout).permute(0, 3, 1, 2).contiguous().cpu(),
                   scale=lay.scale.cpu(), shift=lay.shift.cpu(), mean=lay.mean.cpu(), invstd=lay.invstd.cpu(), slope=lay.slope,
                   out8=interior(self.qbufs[t.buf], True, t, cdst) if lay.q8_y else None,
                   out16=interior(self.bufs[t.buf], False, t, cdst), out2_8=None, out2_16=None,
                   dst={L.DST_PLAIN: "plain", L.DST_POOL: "pool", L.DST_REORG: "reorg"}[lay.mode],
                   dy=ops.padded_view(lay.dy, B, lay.H, lay.W, lay.cout_p, lay.pad)[:, 1:-1, 1:-1, :lay.cout]
                   .permute(0, 3, 1, 2).contiguous().float().cpu(),
                   w_q=lay.w_q.cpu(), wexp=(lay.wexp4 if lay.form == "q8_w4" else lay.wexp)[:lay.cout].cpu(),
                   gin=lay.gin.view(B, lay.H, lay.W, ti.ld)[..., ti.choff:ti.choff + lay.cin].permute(0, 3, 1, 2)
                   .contiguous().float().cpu())
        if lay.form == "q8_w4":
            ktot, npad = lay.cin * lay.k * lay.k, ops.round_up(lay.cout, 256)
            out["codes"] = lay.w4c.view(npad, ktot // 2)[:lay.cout].cpu()
            out["gshift"] = lay.w4g.view(ktot // 64, npad, 2)[:, :lay.cout].contiguous().cpu()
        if t2 is not None:
            out["out2_8"] = interior(self.qbufs[t2.buf], True, t2, lay.cout) if lay.q8_y2 else None
            out["out2_16"] = interior(self.bufs[t2.buf], False, t2, lay.cout)
        return out

    def _interior(self, buf, f8, t, C, ld=None):
        """The C channels of tensor `t` in `buf` -- its byte buffer of `ld` bytes per pixel (`f8`; default: the engine's
        buffer of that tensor) or its fp16 one -- without the halo, as a CPU NCHW tensor: codes (uint8) or fp32 values."""
        pad = self._pad_for(t.W)
        if f8:
            v = ops.padded_view_q8(buf, self.B, t.H, t.W, ld or self._qld[t.buf], pad)
        else:
            v = ops.padded_view(buf, self.B, t.H, t.W, t.ld, pad)
        v = v[:, 1:-1, 1:-1, t.choff:t.choff + C].permute(0, 3, 1, 2).contiguous().cpu()
        return v if f8 else v.float()

    def q8_block_io(self, conv_number):
        """Debug accessor: what fp8 block `conv_number` read and wrote in the last forward, from the engine's own buffers,
        as CPU NCHW tensors -- `x8` e4m3 codes of the input; `y` (and `y2`, the full-resolution copy, or None) as codes
        (uint8) where `y_f8` (`y2_f8`) else fp16 values; `dst` "plain" / "pool" / "reorg"; the epilogue's `scale`, `shift`,
        `slope`."""
        lay = self.layers[conv_number - 1]
        if not lay.q8_on:
            raise McamdError("conv%d is not an fp8 block (fp8_layers = %r)" % (conv_number, self.fp8_layers))
        read = self._interior
        t, t2, ti = lay.out_t, lay.out2_t, lay.tin
        cdst = 4 * lay.cout if lay.mode == L.DST_REORG else lay.cout
        out = dict(x8=read(lay.xq if lay.xq is not None else self.qbufs[ti.buf], True, ti, lay.cin, lay.geom_q8.x_ld),
                   y=read(self.qbufs[t.buf] if lay.q8_y else self.bufs[t.buf], lay.q8_y, t, cdst), y_f8=lay.q8_y,
                   y2=None, y2_f8=lay.q8_y2, dst={L.DST_PLAIN: "plain", L.DST_POOL: "pool", L.DST_REORG: "reorg"}[lay.mode],
                   scale=lay.scale.cpu(), shift=lay.shift.cpu(), slope=lay.slope)
        if t2 is not None:
            out["y2"] = read(self.qbufs[t2.buf] if lay.q8_y2 else self.bufs[t2.buf], lay.q8_y2, t2, lay.cout)
        return out

    # ------------------------------------------------------------------ filter compaction
    def _set_geom_f(self, lay):
        """Forward geometry of a layer in a split-operand engine, over the filters it computes and the input channels it
        reads (all of them, or kept + ones of a folded producer): the K-concatenated problem [x_hi | x_lo | x_hi] x
        [w_hi | w_hi | w_lo] on the two planes `tin.ps` apart (x_wrap), or the plain geometry for a block left on plain
        operands (it reads the hi plane, like every backward launch)."""
        if not self.precise:
            return
        cin_eff = lay.fold_aug if lay.fold is not None else lay.cin
        if lay.level == 1:
            lay.geom_f = lay.geom_act
            return
        wrap = 2 * lay.tin.ps if (self.act_planes == 2 and lay.li > 0) else 0      # (the network input keeps three planes)
        lay.geom_f = ops.geom(self.B, lay.H, lay.W, lay.k, lay.level * cin_eff, lay.n_act, lay.tin.ld, 0, 0, lay.pad, wrap)
        # fp8 correction terms (mcamd_conv_geom.x_f8, "mixed" only): x_hi w_hi on the fp16 MFMAs, x_lo w_hi + x_hi w_lo from
        # e4m3 copies on the block-scaled fp8 MFMAs -- where the layer's forward takes the ping-pong kernel and its input is
        # written by an ordinary block's activation pass (which then stores hi | [lo8 | x8], _planes_for)
        lay.f8 = False
        prod = self.producer_of.get(lay.src)
        if (self.f8 and wrap and prod is not None and not lay.stem and not prod.stem
                and lay.bn is not None and cin_eff % 64 == 0 and lay.tin.ps == cin_eff and lay.tin.choff == 0):
            # (a folding consumer's augmented weights carry the folded constants of up to cout dead channels in one column:
            # 16x of headroom above the layer's own largest weight)
            lay.f8_wexp_eff = lay.f8_wexp - (4 if lay.fold is not None else 0)
            g8 = ops.geom(self.B, lay.H, lay.W, lay.k, 2 * cin_eff, lay.n_act, lay.tin.ld, 0, 0, lay.pad, 0, x_f8=cin_eff,
                          x_f8_wexp=lay.f8_wexp_eff)
            if ops.conv_fwd_f8_ok(g8):
                lay.f8, lay.geom_f = True, g8

    def _refresh_f8_wexp(self):
        """Per-layer exponent of the e4m3 weight bytes (mcamd_conv_geom.x_f8_wexp): the layer's largest |w| lands at
        112-224 of e4m3's 448.  BatchNorm makes a layer's weight scale arbitrary and the bytes have 17 binades, so a static
        exponent served initialisation-sized weights only (x 300: 5e-3 on the train logits).  One host read,
        taken when the model says its weights were replaced (load_state_dict / load_weights / invalidate_packed, and the
        first pack) -- not per step: SGD moves a layer's largest weight by far less than the 2x of headroom."""
        cands = [lay for lay in self.layers if lay.level == 3 and lay.bn is not None and not lay.stem]
        if not (self.f8 and cands):
            return
        amax = torch.stack([lay.conv.weight.data.abs().max() for lay in cands]).tolist()
        changed = False
        for lay, a in zip(cands, amax):
            e = ops.F8_WEXP_DEFAULT
            if a > 0.0 and math.isfinite(a):
                e = max(-20, min(36, int(math.floor(math.log2(224.0 / a)))))
            if e != lay.f8_wexp:
                lay.f8_wexp, changed = e, True
        if changed:
            for lay in self.layers:
                self._set_geom_f(lay)
            self._pack_key = None
            self._plan_epoch += 1         # the forward geometries changed: recorded plans are stale

    def _planes_for(self, tid):
        """Storage form of activation tensor `tid` in a split-operand engine (mcamd_act_desc.planes): 4 = hi | e4m3
        corrections when its consumer multiplies fp8 correction terms, else hi | lo (or hi | lo | hi)."""
        c = self.consumer_of.get(tid)
        return 4 if (c is not None and c.f8) else self.act_planes

    def _update_compaction(self):
        """Sparse-masked path: skip the filters a filter mask removed (north_star: "a sparse-masked wgrad
        path that skips zeroed filters"; the reference multiplies by the mask and computes them anyway,
        layers.py:59-64).

        A filter whose mask row is all zero has zero effective weights, so its raw conv output is exactly 0,
        its weight gradient is 0 and it contributes nothing to the input gradient.  Per BN conv block the
        engine therefore orders that block's output channels PHYSICALLY as [kept filters..., removed
        filters...] and runs forward, dgrad and wgrad with cout = the kept count (rounded up to 8): the
        removed channels of y / dY are never written and stay zero, BatchNorm then yields their constant
        leaky(beta) exactly as in the dense computation.  Everything downstream that indexes channels by
        position follows the permutation: the consumer's weights are gathered to the physical input order
        before packing, its weight gradient is scattered back, and the BN parameter vectors are addressed
        through `chan_perm`.  Pool / reorg / route keep or compose permutations.  Called when a mask
        object changes (one host sync for the kept counts)."""
        dev = self.device
        # (every recorded plan is stale, buffers / maps / geometries below change: _choose_forms, the one caller, has bumped
        # _plan_epoch)
        tperm = {-1: None}               # tensor id -> LongTensor physical position -> original channel (None = identity)
        by_ci = {lay.index: lay for lay in self.layers}
        wbytes = 16
        for ind, (t, _) in enumerate(self._bops):
            src = self._srcs[ind]
            if t == "convolutional":
                lay = by_ci[ind]
                mask = lay.conv.mask if lay.conv.mask_flag else None
                if mask is not None and (not mask.is_cuda or mask.dtype != torch.float32 or tuple(mask.shape) != tuple(lay.conv.weight.shape)):
                    raise McamdError("conv block %d: mask must be a CUDA fp32 tensor shaped like the weight" % ind)
                perm, n_act, keep = None, lay.cout, None
                if mask is not None:
                    alive = mask.reshape(lay.cout, -1).amax(1) != 0
                    keep = alive.float()
                    # (the 3-channel first layer keeps all its filters: its streaming kernels -- stem_fwd / wgrad_stem --
                    # exist for 32 and 64 filters only, and a ragged count falls back to the generic kernels:
                    # measured 0.22 -> 0.33 ms forward, 0.19 -> 0.32 ms weight gradient at 40 % pruning)
                    # (... nor does the first block of a split-operand engine: its fused / fp32 kernels want all 32 filters)
                    # (... nor does a block that runs the block-sparse kernel: it skips the dead filters' tiles itself)
                    if (self.compact and lay.bn is not None and not lay.stem and not (self.precise and lay.li == 0)
                            and lay.li not in self._bs_exempt):
                        # kept count rounded up so the kernels keep their tile shapes: whole 64-filter tiles
                        # (the 9-tap wgrad and the 128-wide igemm tiles) where the layer has them
                        gran = self.compact_gran or (64 if lay.cout >= 128 else 8)
                        n8 = min(lay.cout, ops.round_up(max(int(alive.sum()), 1), gran))
                        if n8 < lay.cout:
                            perm = torch.cat((torch.nonzero(alive).flatten(), torch.nonzero(~alive).flatten()))
                            n_act = n8
                in_perm = tperm[src[0]]
                lay.perm, lay.n_act, lay.in_perm = perm, n_act, in_perm
                lay.perm32 = perm.to(torch.int32).contiguous() if perm is not None else None
                lay.keep = None if keep is None else (keep[perm].contiguous() if perm is not None else keep)
                lay.geom_act = lay.geom if perm is None else ops.geom(self.B, lay.H, lay.W, lay.k, lay.cin, n_act,
                                                                      lay.tin.ld, lay.tin.choff, lay.stem, lay.pad)
                lay.gather = perm is not None or in_perm is not None
                lay.g_rows = perm[:n_act].to(torch.int32).contiguous() if perm is not None else None
                lay.g_cols = in_perm.to(torch.int32).contiguous() if in_perm is not None else None
                self._set_geom_f(lay)
                if lay.bn is not None and not lay.fused_stem and lay.y is not None and not lay.stem_f32:
                    rows = ops.stats_rows(lay.geom_f, L.EPI_RAW_F32) if self.precise else ops.stats_rows(lay.geom_act)
                    if lay.stats.shape[0] != rows:
                        lay.stats = torch.zeros(rows, 2, lay.stats.shape[2], dtype=torch.float32, device=dev)
                    else:
                        lay.stats.zero_()
                    lay.y.zero_()
                wbytes = max(wbytes, ops.wgrad_workspace_bytes(lay.geom_act))
                tperm[ind] = perm
            elif t == "maxpool":
                tperm[ind] = tperm[src[0]]
            elif t == "reorg":
                p = tperm[src[0]]
                C = self._shape[src[0]][0]
                tperm[ind] = None if p is None else torch.cat([p + q * C for q in range(4)])
            elif t == "route" and len(src) == 2:
                pa, pb = tperm[src[0]], tperm[src[1]]
                ca, cb = self._shape[src[0]][0], self._shape[src[1]][0]
                if pa is None and pb is None:
                    tperm[ind] = None
                else:
                    pa = pa if pa is not None else torch.arange(ca, device=dev)
                    pb = pb if pb is not None else torch.arange(cb, device=dev)
                    tperm[ind] = torch.cat((pa, pb + ca))
            elif t == "route":
                tperm[ind] = tperm[src[0]]
            else:
                tperm[ind] = None
        wbytes = max(wbytes, self._plan_folds())
        self.pool_act_on = not any(lay.perm is not None for lay in self.layers)
        if wbytes > self.wgrad_ws.numel():
            self.wgrad_ws = torch.empty(wbytes, dtype=torch.uint8, device=dev)

    def _plan_folds(self):
        """Dead INPUT channels (csrc/fold.hip).  A compacted producer whose every consumer reads its tensor directly (not
        through a concat or reorg) turns its first dead physical channel into a channel of ones (mcamd_bn_coeffs_ex) and
        each consumer runs forward / dgrad / wgrad on  kept + 1  input channels with augmented weights: the dead
        channels' constants leaky(beta) are folded into the filter of the ones-channel, exactly, borders included.
        Returns the weight-gradient workspace bytes the new geometries need."""
        dev = self.device
        for lay in self.layers:
            lay.fold, lay.ones_idx, lay.skip_dead, lay.fold_consumers, lay.bn_width = None, -1, False, [], 0
            lay.waug = lay.dwaug = None
            self._fold_key = None
            if lay.gin is not None:
                lay.gin.zero_()       # a folding consumer's dgrad leaves the dead channels of G untouched: they must be finite
            for t in (lay.tin, lay.out_t, lay.out2_t):
                if t is not None and t.ps != t.ps0:      # planes of a formerly folded producer: back to the full width
                    t.ps = t.ps0
                    v = ops.padded_view(self.bufs[t.buf], self.B, t.H, t.W, t.ld)[:, 1:-1, 1:-1]
                    v[..., t.choff:t.choff + 2 * t.C] = 0
        if not (self.compact and self.fold_dead):
            for lay in self.layers:
                self._set_geom_f(lay)
            return 16
        wbytes = 16
        for prod in self.layers:
            if prod.perm is None or prod.is_last or prod.mode == L.DST_REORG or prod.n_act >= prod.cout:
                continue
            outs = [t for t in (prod.out_id, prod.out2_id) if t is not None and t in self.consumer_of]
            cons = [self.consumer_of[t] for t in outs]
            if not cons or any(c.src != t or c.stem or c.tin.choff != 0 for c, t in zip(cons, outs)):
                continue              # a concat member / reorg source: its consumer reads every channel
            # the augmented channel count keeps the kernels' fast shapes (whole 64-channel K blocks for wide inputs), and
            # folding must remove at least a quarter of the input channels to pay for its ragged tiles (measured on
            # conv19 of the 40 % model, 840 of 1024 channels: dgrad 0.188 -> 0.294 ms)
            aug = ops.round_up(prod.n_act + 1, 64 if prod.cout >= 256 else (32 if self.precise else 8))
            # BatchNorm / activation passes of a folded producer on fewer channels (their kernels keep one 8-channel group per
            # thread: 8 x a power of two channels).  EXACT: the kept count itself is such a number -- the pass covers the kept
            # channels and the ones-channel behind them is written once, here.  WIDENED (round 4): otherwise the next such
            # number that holds kept + ones -- the pass then writes the ones-channel itself (scale 0 / shift 1) and, behind it,
            # dead channels as the constants they are, which meet zero columns of the augmented weights.  0 = full width.
            ch = prod.n_act // 8
            exact = prod.n_act % 8 == 0 and ch >= 1 and (ch & (ch - 1)) == 0 and ch <= 256
            width = prod.n_act if exact else 0
            if not exact:
                w2 = 8
                while w2 < prod.n_act + 1:
                    w2 *= 2
                if w2 < prod.cout and w2 <= 2048:
                    width = w2
            if not self.bn_narrow_on:
                width = 0
            if self.precise:
                # Split-operand engines store a tensor as hi | lo planes; a folding consumer's K-concatenated geometry wants
                # them `aug` channels apart (x_wrap = 2 aug), so the producer's activation pass writes `aug`-spaced planes --
                # which only works when it is a narrowed pass that fits under the plane pitch (a full-width pass would run over
                # its own lo plane).  Producers without one stay compacted but unfolded.
                if not width:
                    continue
                aug = max(aug, width)
            elif width and aug > width and not exact:
                width = 0                 # (the consumer would read channels the narrowed pass does not write)
            if aug > 0.75 * prod.cout:
                continue
            prod.ones_idx, prod.skip_dead = prod.n_act, True
            prod.fold_consumers = sorted(cons, key=lambda c: -c.li)      # backward order: the first one initialises dbeta
            prod.bn_width = width
            if width:
                for t in (prod.out_t, prod.out2_t):
                    if t is not None:
                        v = ops.padded_view(self.bufs[t.buf], self.B, t.H, t.W, t.ld)[:, 1:-1, 1:-1]
                        if self.precise:                 # both planes: aug apart from now on, zero but for the ones-channel
                            t.ps = aug
                            v[..., t.choff:t.choff + 2 * t.C] = 0
                        elif exact:
                            v[..., t.choff + prod.n_act + 1:t.choff + prod.cout] = 0
                        if exact:
                            v[..., t.choff + prod.n_act] = 1
                prod.dy.zero_()
            for c in cons:
                c.fold = prod
                c.fold_cin = prod.n_act
                c.fold_aug = min(aug, ops.round_up(prod.cout, 8))      # padding columns: zero weights
                c.geom_act = ops.geom(self.B, c.H, c.W, c.k, c.fold_aug, c.n_act, c.tin.ld, c.tin.choff, 0, c.pad)
                c.gather = True
                c.waug = torch.zeros(c.n_act, c.fold_aug, c.k, c.k, dtype=torch.float32, device=dev)
                c.dwaug = torch.zeros_like(c.waug)
                wbytes = max(wbytes, ops.wgrad_workspace_bytes(c.geom_act))
        for lay in self.layers:          # (plane strides may have moved under any layer: every forward geometry again)
            self._set_geom_f(lay)
            if lay.bn is not None and not lay.fused_stem and lay.y is not None and not lay.stem_f32:
                rows = ops.stats_rows(lay.geom_f, L.EPI_RAW_F32) if self.precise else ops.stats_rows(lay.geom_act)
                if lay.stats.shape[0] != rows:
                    lay.stats = torch.zeros(rows, 2, lay.stats.shape[2], dtype=torch.float32, device=dev)
        for prod in self.layers:         # a ones-channel written once (exact narrowed pass) in front of an fp8-correction
            if prod.ones_idx < 0 or not prod.bn_width or prod.bn_width != prod.n_act:     # consumer: its x8 byte = e4m3(1 * 2)
                continue
            for tid, t in ((prod.out_id, prod.out_t), (prod.out2_id, prod.out2_t)):
                if t is not None and self._planes_for(tid) == 4:
                    v8 = ops.padded_view(self.bufs[t.buf].view(torch.uint8), self.B, t.H, t.W, 2 * t.ld,
                                         pad=ops.pad_of(self.bufs[t.buf]))[:, 1:-1, 1:-1]
                    v8[..., 2 * t.choff + 3 * t.ps + prod.n_act] = 0x40
        return wbytes

    def _fold_constants(self, prod, training):
        """Pre-activation value of the producer's dead channels in the module's channel order: y = 0 there, so
        z = shift = beta in training (batch mean 0) and beta - running_mean * gamma / sqrt(running_var + eps) in eval."""
        bn = prod.bn
        if training:
            return bn.bias.data
        return bn.bias.data - bn.running_mean * bn.weight.data / torch.sqrt(bn.running_var + bn.eps)

    # ------------------------------------------------------------------ launch plans
    def _ptr_sig(self):
        """Everything a recorded plan holds BY VALUE that torch may change under it: addresses of parameters, masks and
        BatchNorm buffers, of the engine's own persistent flat-gradient / logit-gradient buffers, and the BatchNorm momentum /
        eps the coefficient kernels were recorded with."""
        sig = [p.data_ptr() for p in self.params]
        sig.append(self._flat.data_ptr() if self._flat is not None else 0)
        sig.append(self._gout.data_ptr() if self._gout is not None else 0)
        for lay in self.layers:
            if lay.bn is not None:
                sig.append(lay.bn.running_mean.data_ptr())
                sig.append(lay.bn.running_var.data_ptr())
                sig.append((lay.bn.momentum, lay.bn.eps))
            if lay.conv.mask_flag:
                sig.append(lay.conv.mask.data_ptr())
        return tuple(sig)

    # ------------------------------------------------------------------ forward
    def forward(self, x, training):
        B = self.B
        if tuple(x.shape) != (B, self.layers[0].cin, self.layers[0].H, self.layers[0].W):
            raise McamdError("engine built for input %s, got %s" % ((B, self.layers[0].cin, self.layers[0].H, self.layers[0].W), tuple(x.shape)))
        if bool(training) != self.train_layout and self.shared_halo_maxw:
            raise McamdError("this engine was planned for %s (activation layout); build one for the other mode"
                             % ("training" if self.train_layout else "inference"))
        if training:
            for lay in self.layers:
                if lay.border is not None:
                    raise McamdError("slim models (border_bias tables) are inference-only: call model.eval()")
                if not lay.train_ok:
                    raise McamdError("conv block %d: training needs a BN channel count of 8 * (power of two), got %d"
                                     % (lay.index, lay.cout))
        if training and self.q8 and not self.qat:
            raise McamdError("precision %r is inference only (there is no fp8 training path): call model.eval() or "
                             "pick another precision for training" % (self.precision,))
        mode = None if training else getattr(self.model, "sparse", None)
        st = getattr(self.model, "sparse_train", None) if training else None
        if st not in (None, "block", "block-wgrad"):
            raise McamdError("sparse_train must be None, 'block' or 'block-wgrad' (got %r)" % (st,))
        if st is not None and self.precision != "fp16":
            raise McamdError("sparse_train=%r trains in the plain-fp16 engine only (model.precision = 'fp16'), not precision=%r"
                             % (st, self.precision))
        if mode is not None and (self.precise or self.q8):
            raise McamdError("sparse=%r runs in the plain-fp16 inference engine only (model.precision = 'fp16'), not %r%s"
                             % (mode, self.precision, "; 2:4 masks on the fp8 engine: model.precision = 'fp8-2:4' with "
                                "model.sparse = None" if self.q8 and mode == "2:4" else
                                "; block masks on the fp8 engine: model.precision = 'fp8-block' with model.sparse = None"
                                if self.q8 and mode == "block" else ""))
        splitk = bool(getattr(self.model, "splitk", False)) and not training
        if splitk and (self.precise or self.q8):
            raise McamdError("splitk=True runs in the plain-fp16 inference engine only (model.precision = 'fp16'), not %r%s"
                             % (self.precision, "; split-K on the fp8 engine: model.precision = 'fp8-splitk' with "
                                "model.splitk = False" if self.q8 else ""))
        if mode not in (None, "2:4", "block"):
            raise McamdError("sparse must be None, '2:4' or 'block' (got %r)" % (mode,))
        max_kept = float(getattr(self.model, "sparse_max_kept", BSPARSE_MAX_KEPT)) if mode == "block" else None
        if self.q8_bsparse and not training:
            max_kept = float(getattr(self.model, "fp8_block_max_kept", Q8_BSPARSE_MAX_KEPT))
        wgrad_max = None
        if st is not None and float(getattr(self.model, "sparse_train_max_kept", BSPARSE_TRAIN_MAX_KEPT)) > 0.0:
            # (a bound of 0.0 chooses nothing: the sparse_train = None engine, bit for bit)
            mode, max_kept = "block-train", float(getattr(self.model, "sparse_train_max_kept", BSPARSE_TRAIN_MAX_KEPT))
            if st == "block-wgrad" and float(getattr(self.model, "sparse_train_wgrad_max_kept", BSPARSE_TRAIN_WGRAD_MAX_KEPT)) > 0.0:
                # (again 0.0 chooses nothing: sparse_train = "block", bit for bit, and no list is built)
                wgrad_max = float(getattr(self.model, "sparse_train_wgrad_max_kept", BSPARSE_TRAIN_WGRAD_MAX_KEPT))
        self.pack(force=bool(training), training=training, sparse=mode, splitk=splitk, max_kept=max_kept, wgrad_max_kept=wgrad_max)
        self.serial += 1
        tin = self.layers[0].tin
        xs = x.detach().contiguous().float()
        if self.precise and not self.stem:
            l0 = self.layers[0]
            if l0.stem_split:
                ops.nchw_to_nhwc4_split(xs, l0.sh_img, l0.sh_img_lo)      # hi and lo NHWC4 images in one pass
            elif l0.stem_f32:
                # the first convolution in fp32 from the image itself (outside the recorded plan: the image pointer is
                # the caller's); the hi plane of the image is still needed where the generic weight gradient reads it
                if training:
                    ops.nchw_to_padded_split(xs, self.bufs[tin.buf], tin.ld, tin.choff, tin.ps)
                mask0 = l0.conv.mask if l0.conv.mask_flag else None
                self._timed('fwd', l0, ops.stem_conv_f32, xs, l0.conv.weight.data, mask0, l0.weff, l0.y, l0.cout,
                            l0.stats if training else None)
            else:
                # the image too is an MFMA operand: hi | lo | hi planes
                # (written by the layout kernel itself: round 2 built the planes with torch.cat, three 3 x B x H x W fp32
                # temporaries per forward -- 0.8 GB at B=128 through the caching allocator)
                ops.nchw_to_padded_split(xs, self.bufs[tin.buf], tin.ld, tin.choff, tin.ps)
        else:
            ops.nchw_to_padded(xs, self.bufs[tin.buf], tin.ld, tin.choff)
        if self._logits is None:
            self._logits = torch.empty(self.out_shape, dtype=torch.float32, device=self.device)
        main = torch.cuda.current_stream(self.device)
        side = self._get_side_stream() if self._pack_on_side else None
        if self.use_plan and self.events is None:
            # one library call replays the recorded layer walk (csrc/plan.hip); recorded again when a pointer moved
            key = (bool(training), main.cuda_stream, side.cuda_stream if side is not None else 0, self._plan_epoch,
                   self._ptr_sig())
            plan = self._fwd_plans.get(bool(training))
            if plan is None or plan.key != key:
                plan = ops.Plan([main] + ([side] if side is not None else []))
                with plan:
                    self._forward_body(training, main, side)
                plan.key = key
                self._fwd_plans[bool(training)] = plan
            plan.run()
        else:
            self._forward_body(training, main, side)
        last = self.layers[-1]
        out = self._logits + last.border_map if last.border_map is not None else self._logits.clone()
        if training:
            bns = [lay.bn.num_batches_tracked for lay in self.layers if lay.bn is not None]
            if bns:
                torch._foreach_add_(bns, 1)
        return out

    def _forward_body(self, training, main, side):
        """The layer walk of the forward pass: library calls only (every one of them recordable)."""
        B = self.B
        out = self._logits
        fused_done = set()      # blocks whose forward launch ran inside their producer's (_fused_1x1)
        for lay in self.layers:
            xin = self.bufs[lay.tin.buf]
            if lay.li == 1 and side is not None:
                ops.stream_wait(main, side)     # the fold + re-pack of the layers behind the first block ran on the second stream
            if lay.is_last:
                bias = lay.conv.bias.data if lay.conv.bias is not None else None
                self._timed('fwd', lay, ops.conv_fwd_nchw, lay.geom_f if self.precise else lay.geom_act, xin, lay.wp, out, bias)
                continue
            bn = lay.bn
            if lay.fused_stem or (lay.fused_stem_eval and not training and lay.out_t.ld - lay.out_t.choff >= 32):
                # conv1 + BatchNorm + LeakyReLU + maxpool in one pass over the image (batch statistics from the Gram
                # matrix of the image windows in training mode, running statistics otherwise)
                if not training:
                    ops.bn_coeffs(None, lay.cout, lay.M, bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, False,
                                  lay.scale, lay.shift, lay.mean, lay.invstd, eps=bn.eps)
                t = lay.out_t
                self._timed('fwd', lay, ops.stem_block_fwd, B, lay.H, lay.W, xin, lay.wp, bn.weight.data, bn.bias.data,
                            bn.running_mean, bn.running_var, training, lay.scale, lay.shift, lay.mean, lay.invstd, lay.slope,
                            self.bufs[t.buf], t.ld, t.choff, lay.stem_ws if lay.fused_stem else None,
                            momentum=_momentum(bn), eps=bn.eps, cout=lay.cout,
                            planes=self.act_planes)
                continue
            if training and lay.stem_split:
                # statistics half of the plain-operand block (dst None): Gram context + self-consistent coefficients for the
                # backward pass (no running-statistics update: the split pass below owns them)
                c = lay.sh_coef
                ops.stem_block_fwd(B, lay.H, lay.W, lay.sh_img, lay.sh_wp, bn.weight.data, bn.bias.data, None, None, True,
                                   c[0], c[1], c[2], c[3], lay.slope, None, 0, 0, lay.stem_ws,
                                   momentum=0.0, eps=bn.eps, cout=lay.cout, planes=1)
                self._timed('fwd', lay, self._stem_split_forward, lay)
                continue
            if self.precise:
                # unrounded fp32 raw output (+ batch statistics from the fp32 values), then BN + LeakyReLU
                # (+ pool / reorg / route) written as hi | lo | hi planes
                if not lay.stem_f32 and lay.li not in fused_done:   # (the fp32 first convolution ran in forward(), from the caller's image)
                    self._timed('fwd', lay, ops.conv_fwd_raw32, lay.geom_f, xin, lay.wp, lay.y, lay.cout, 0,
                                lay.stats if training else None)
                ops.bn_coeffs(lay.stats if training else None, lay.cout, lay.M, bn.weight.data, bn.bias.data,
                              bn.running_mean, bn.running_var, training, lay.scale, lay.shift, lay.mean, lay.invstd,
                              momentum=_momentum(bn), eps=bn.eps, perm=lay.perm32, ones_channel=lay.ones_idx)
                t, t2 = lay.out_t, lay.out2_t
                cons = self._fused_1x1(lay)
                if cons is not None:
                    # the activation goes straight into the 1x1 forward behind this block: only its hi plane is stored
                    self._timed('fwd', cons, ops.bn_act_conv1x1_fwd, *self._fused_1x1_act(lay), cons.geom_f, cons.wp, cons.y,
                                cons.cout, 0, cons.stats if training else None)
                    fused_done.add(cons.li)
                    self.fused_1x1_launches += 1
                    continue
                af = lay.act_full if (training and self.pool_act_on) else None
                dst2, dst2_pad = self._dst2(t2)
                ops.bn_act_fwd(B, lay.H, lay.W, lay.bn_width or lay.cout, lay.y, lay.cout, 0, lay.scale, lay.shift,
                               lay.slope, lay.mode, self.bufs[t.buf], t.ld, t.choff, *dst2, border=lay.border,
                               planes=self._planes_for(lay.out_id), dst_plane=t.ps, dst2_plane=t2.ps if t2 is not None else 0,
                               dst_pad=self._pad_for(t.W), dst2_pad=dst2_pad,
                               planes2=self._planes_for(lay.out2_id) if t2 is not None else 0,
                               pool_act=af, pool_act_ld=ops.round_up(lay.cout, 8) if af is not None else 0,
                               pool_act_pad=self._pad_for(lay.W) if af is not None else 0)
                continue
            if not training and (self._fused_eval(lay) or lay.q8_on):
                # inference: BN (running statistics) + LeakyReLU -- and the MaxPool / Reorg that follows the block -- in the
                # conv epilogue, written straight into the consumer's padded buffer: the raw output is never stored (one
                # fp16 rounding per layer, no second pass)
                ops.bn_coeffs(None, lay.cout, lay.M, bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, False,
                              lay.scale, lay.shift, lay.mean, lay.invstd, eps=bn.eps)
                t = lay.out_t
                # destination form of the epilogue: plain / pool (+ the full-resolution copy y2) / reorg, each as bytes where
                # the engine holds the tensor as e4m3 (fp8 forms only) and as fp16 elsewhere
                y, y_ld = (self.qbufs if lay.q8_y else self.bufs)[t.buf], self._q8_tld(t, lay.q8_y)
                (y2, y2_ld, y2_choff), _ = self._dst2(lay.out2_t, lay.q8_y2)
                form = _FORMS[lay.form]
                args, kw = form.operands(self, lay, xin)
                self._timed('fwd', lay, getattr(ops, form.fwd), *args, y, y_ld, t.choff, lay.scale, lay.shift, lay.slope,
                            dst_mode=lay.mode, y2=y2, y2_ld=y2_ld, y2_choff=y2_choff, **kw)
                continue
            if training and self._qat_train(lay):
                self._qat_forward(lay, xin)
                continue
            _FORMS[lay.form].raw(self, lay, xin, training)
            stats = lay.bs_stats if lay.form == "bsparse_train" else lay.stats      # (one row per pixel tile of that kernel)
            ops.bn_coeffs(stats if training else None, lay.cout, lay.M, bn.weight.data, bn.bias.data,
                          bn.running_mean, bn.running_var, training, lay.scale, lay.shift, lay.mean, lay.invstd,
                          momentum=_momentum(bn), eps=bn.eps, perm=lay.perm32, ones_channel=lay.ones_idx)
            t = lay.out_t
            dst2, dst2_pad = self._dst2(lay.out2_t)
            ops.bn_act_fwd(B, lay.H, lay.W, lay.bn_width or lay.cout, lay.y, lay.cout, 0, lay.scale, lay.shift,
                           lay.slope, lay.mode, self.bufs[t.buf], t.ld, t.choff, *dst2, border=lay.border,
                           dst_pad=self._pad_for(t.W), dst2_pad=dst2_pad)

    def _dst2(self, t2, f8=False):
        """The second destination of a block (the full-resolution copy beside a pooled output): ((buffer, leading dimension,
        channel offset), pad form), all None / 0 where the block has none.  `f8`: the tensor's byte buffer."""
        if t2 is None:
            return (None, 0, 0), 0
        return ((self.qbufs if f8 else self.bufs)[t2.buf], self._q8_tld(t2, f8), t2.choff), self._pad_for(t2.W)

    def _fused_1x1_act(self, lay):
        """(positional, keyword) arguments of the activation pass of the PLAIN block `lay` in hi | lo storage, as
        ops.bn_act_fwd takes them."""
        t = lay.out_t
        return ((self.B, lay.H, lay.W, lay.cout, lay.y, lay.cout, 0, lay.scale, lay.shift, lay.slope, lay.mode,
                 self.bufs[t.buf], t.ld, t.choff),
                dict(planes=self._planes_for(lay.out_id), dst_plane=t.ps, dst_pad=self._pad_for(t.W)))

    def _fused_1x1(self, lay):
        """The block whose forward launch takes the BatchNorm + LeakyReLU of block `lay` (ops.bn_act_conv1x1_fwd), or None.
        `lay` must be a PLAIN block of a split-operand engine with one destination and none of keep / perm / fold /
        fold_consumers / a narrowed BatchNorm pass / a border table; its one consumer a BatchNorm 1x1 block on three fp16
        operand terms (level 3, no fp8 correction form) that runs its dense geometry (no fold / gather / in_perm) on exactly
        the producer's channel slice; and the library must have a kernel for the pair (mcamd_bn_act_conv1x1_ok)."""
        if not (self.fuse_bn_1x1 and self.precise):
            return None
        key = (lay.li, self._plan_epoch)
        hit = self._fused_1x1_cache.get(key, False)
        if hit is not False:
            return hit
        res = None
        cons = self.consumer_of.get(lay.out_id)
        t = lay.out_t
        if (cons is not None and t is not None and lay.mode == L.DST_PLAIN and lay.out2_id is None and lay.out2_t is None
                and not lay.stem and not lay.fused_stem and not lay.stem_split and not lay.stem_f32
                and lay.keep is None and lay.perm is None and lay.fold is None and not lay.fold_consumers and not lay.bn_width
                and not lay.skip_dead and lay.ones_idx < 0 and lay.border is None
                and lay.y is not None and lay.y.dtype == torch.float32
                and cons.bn is not None and not cons.is_last and cons.k == 1 and cons.level == 3 and not cons.f8
                and cons.fold is None and not cons.gather and cons.in_perm is None and cons.geom_act is cons.geom
                and cons.src == lay.out_id
                and cons.tin.buf == t.buf and cons.tin.ld == t.ld and cons.tin.choff == t.choff and cons.cin == lay.cout
                and cons.y is not None and cons.y.dtype == torch.float32):
            args, kw = self._fused_1x1_act(lay)
            d = ops.act_geom(self.B, lay.H, lay.W, lay.cout, lay.cout, 0, lay.slope, lay.mode, t.ld, t.choff, **kw)
            if ops.bn_act_conv1x1_ok(d, cons.geom_f):
                res = cons
        self._fused_1x1_cache = {k: v for k, v in self._fused_1x1_cache.items() if k[1] == self._plan_epoch}
        self._fused_1x1_cache[key] = res
        return res

    def _qat_forward(self, lay, xin):
        """Training-mode forward of an fp8 block ("fp8-qat"; "fp8-w4-qat", 3x): the fp8 convolution's fp32 raw
        output and its batch statistics, coefficients, then BatchNorm + LeakyReLU (+ pool / reorg / route) written as e4m3 codes into the
        tensors the engine holds as bytes -- with the dequantised values in their fp16 buffers, which the backward pass
        reads -- and as fp16 elsewhere."""
        B, bn = self.B, lay.bn
        x8 = self.qbufs.get(lay.tin.buf)
        if lay.xq is not None:          # the fp16 -> fp8 edge: codes of the padded input slice, dequantised values written back
            ti, x8 = lay.tin, lay.xq
            self._timed('cast', lay, ops.cast_q8, xin, ops.padded_pixels(B, ti.H, ti.W, self._pad_for(ti.W)), ti.ld, ti.choff,
                        lay.cin, x8, ti.ld, ti.choff, write_back=True)
        _FORMS[lay.form].qat_raw(self, lay, x8)     # (the raw forward of the block's form: fp8 bytes, or 4-bit codes)
        ops.bn_coeffs(lay.stats, lay.cout, lay.M, bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, True,
                      lay.scale, lay.shift, lay.mean, lay.invstd, momentum=_momentum(bn), eps=bn.eps)
        t, t2 = lay.out_t, lay.out2_t
        dst2, dst2_pad = self._dst2(t2)
        ops.bn_act_fwd(B, lay.H, lay.W, lay.cout, lay.y, lay.cout, 0, lay.scale, lay.shift, lay.slope, lay.mode,
                       self.bufs[t.buf], t.ld, t.choff, *dst2, dst_pad=self._pad_for(t.W), dst2_pad=dst2_pad,
                       dst_q8=self.qbufs[t.buf] if lay.q8_y else None,
                       dst2_q8=self.qbufs[t2.buf] if (t2 is not None and lay.q8_y2) else None)

    def _stem_split_forward(self, lay):
        """The first block of the "mixed" training precision: batch statistics of the split-operand conv output (nothing
        stored), coefficients, then conv + BatchNorm + LeakyReLU + MaxPool recomputed into the consumer's hi | lo planes."""
        bn, t = lay.bn, lay.out_t
        ops.stem_block_stats(self.B, lay.H, lay.W, lay.sh_img, lay.sh_wp, lay.stats, x_lo=lay.sh_img_lo, wp_lo=lay.sh_wp_lo)
        ops.bn_coeffs(lay.stats, lay.cout, lay.M, bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, True,
                      lay.scale, lay.shift, lay.mean, lay.invstd, momentum=_momentum(bn), eps=bn.eps)
        ops.stem_block_fwd(self.B, lay.H, lay.W, lay.sh_img, lay.sh_wp, bn.weight.data, bn.bias.data, None, None, False,
                           lay.scale, lay.shift, lay.mean, lay.invstd, lay.slope, self.bufs[t.buf], t.ld, t.choff, None,
                           eps=bn.eps, cout=lay.cout, planes=self.act_planes, x_lo=lay.sh_img_lo, wp_lo=lay.sh_wp_lo)

    # ------------------------------------------------------------------ backward
    def _bwd1x1_route(self, lay):
        """Does block `lay` run its backward as ONE launch (ops.conv_bwd1x1)?  The library has an instance for its dense
        geometry (ops.conv_bwd1x1_ok) and the block runs that geometry: no fold, no gather, no in_perm -- the conditions
        _dgrad_sums puts on the consumer."""
        if not self.bwd1x1 or lay.li == 0 or lay.gin is None or lay.fused_stem or lay.stem_shadow:
            return False
        key = (lay.li, self._plan_epoch)
        hit = self._bwd1x1_cache.get(key)
        if hit is None:
            hit = (lay.fold is None and not lay.gather and lay.in_perm is None and lay.geom_act is lay.geom
                   and ops.conv_bwd1x1_ok(lay.geom)[0])
            self._bwd1x1_cache = {k: v for k, v in self._bwd1x1_cache.items() if k[1] == self._plan_epoch}
            self._bwd1x1_cache[key] = hit
        if hit and self._bwd1x1_ws is None:
            need = max(ops.conv_bwd1x1_workspace_bytes(l.geom) for l in self.layers if l.geom is not None)
            self._bwd1x1_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return hit

    def _dgrad_sums(self, lay, concurrent, fused=False):
        """(descriptor, slab, producer) when the dgrad launch of block `lay` can take the BatchNorm-backward sums of the
        block that produced its input (ops.dgrad_sums), else None.  The producer must be a PLAIN block of a split-operand
        engine read from its stored activation (bwd_from_act), with this block as its only consumer and none of keep / perm /
        fold / skip_dead / a narrowed BatchNorm pass; this block must run its dense geometry (no gather / fold of its own),
        and the kernel its dgrad gets must have the sums-taking form (ops.dgrad_sums_rows > 0).
        `fused`: the launch is the block's one-launch backward (_bwd1x1_route), whose slab has ops.conv_bwd1x1_sums_rows rows."""
        if not (self.dgrad_bn_sums and self.bwd_from_act and self.precise) or lay.gin is None:
            return None
        key = (lay.li, "fused" if fused else bool(concurrent), self._plan_epoch)
        hit = self._dgrad_sums_cache.get(key, False)
        if hit is not False:
            return hit
        res = None
        if lay.fold is None and not lay.gather and lay.in_perm is None and lay.geom_act is lay.geom:
            for prod in self.layers:
                if prod.is_last or prod.fused_stem or prod.stem_shadow or prod.bn is None or prod.out_t is None:
                    continue
                if self.consumer_of.get(prod.out_id) is not lay or prod.mode != L.DST_PLAIN or prod.slope <= 0.0:
                    continue
                if prod.out2_id is not None and prod.out2_id in self.consumer_of:
                    continue              # a second consumer: its G arrives in two tensors
                if (prod.keep is not None or prod.perm is not None or prod.fold is not None or prod.skip_dead or prod.fold_consumers
                        or prod.bn_width or prod.border is not None or prod.cout % 8 != 0):
                    continue
                t = prod.out_t
                ch_lo = t.choff - lay.tin.choff
                if t.buf != lay.tin.buf or t.ld != lay.tin.ld or ch_lo < 0 or ch_lo % 8 != 0 or ch_lo + prod.cout > lay.geom.cin:
                    continue
                rows = ops.conv_bwd1x1_sums_rows(lay.geom) if fused else ops.dgrad_sums_rows(lay.geom_act, concurrent)
                if rows <= 0:
                    continue
                slab = torch.empty(rows, 2, prod.cout, dtype=torch.float32, device=self.device)
                y = prod.y if (prod.y is not None and prod.y.dtype == torch.float32) else None
                desc = ops.dgrad_sums(slab, self.bufs[t.buf], t.ld, t.choff, self._pad_for(t.W), prod.scale, prod.shift, prod.mean,
                                      prod.invstd, prod.slope, prod.cout, ch_lo=ch_lo, y=y, y_ld=prod.cout, y_choff=0)
                res = (desc, slab, prod)
                break
        self._dgrad_sums_cache = {k: v for k, v in self._dgrad_sums_cache.items() if k[2] == self._plan_epoch}
        self._dgrad_sums_cache[key] = res
        return res

    def bn_act_bwd_layer(self, lay, g, g_ld, g_choff, g2, g2_ld, g2_choff, dy, dgamma, dbeta, grad_scale, sums=None):
        """pool / reorg / route + LeakyReLU + BatchNorm backward of one block: G (gradient wrt the block's output, at the
        consumer's channel slice) -> dY (padded NHWC), dgamma, dbeta.  One place for the launch arguments (narrowed to the
        kept channels for a folded producer); tests re-issue it with a substitute G.
        `sums`: the slab the dgrad launch that wrote G left the block's sums in (_dgrad_sums) -- only the backward walk,
        which has just issued that launch, passes it."""
        cb = lay.bn_width or lay.cout
        act = {}
        if self.bwd_from_act and self.precise and lay.mode == L.DST_PLAIN and g2 is None:
            # split-operand engines save y as fp32: a PLAIN block's two backward passes read the stored activation (the hi
            # plane in the consumer's input buffer, 2 bytes) instead and invert LeakyReLU (mcamd_act_bwd_desc.act)
            t = lay.out_t
            act = dict(act=self.bufs[t.buf], act_ld=t.ld, act_choff=t.choff, act_pad=self._pad_for(t.W))
        elif self.bwd_from_act and self.precise and self.train_layout and lay.mode == L.DST_POOL and lay.slope > 0.0:
            # ... and a MaxPool block's read the full-resolution fp16 copy of its activation (mcamd_act_desc.pool_act)
            if self.pool_act_on and lay.act_full is not None:
                act = dict(act=lay.act_full, act_ld=ops.round_up(lay.cout, 8), act_choff=0, act_pad=self._pad_for(lay.W))
            if g2 is None and lay.y is not None:
                # ... and the pass that forms the sums needs the pooled element only: the hi plane of the consumer's
                # input buffer, a quarter of the copy (mcamd_act_bwd_desc.pool_out) -- also where there is no copy (filter
                # compaction): 4 bytes per window instead of the 18 of four fp32 y values and G
                t = lay.out_t
                act.update(pool_out=self.bufs[t.buf], pool_out_ld=t.ld, pool_out_choff=t.choff,
                           pool_out_pad=self._pad_for(t.W))
        if sums is not None:
            act["sums"] = sums
        ops.bn_act_bwd(self.B, lay.H, lay.W, cb, lay.y, lay.cout, 0, lay.scale, lay.shift, lay.mean,
                       lay.invstd, lay.slope, lay.mode, g, g_ld, g_choff, dy, lay.cout_p, 0,
                       dgamma, dbeta, grad_scale, g2, g2_ld, g2_choff,
                       self.bwd_ws, None if lay.keep is None else lay.keep[:cb], None if lay.perm32 is None else lay.perm32[:cb],
                       overflow=self.overflow, skip_dead_from=lay.n_act if lay.skip_dead else 0, dy_pad=lay.pad, **act)

    def backward(self, grad_out, on_ready=None):
        """grad wrt the returned logits -> one flat fp32 gradient buffer; returns per-parameter views.
        `on_ready(flat, lo, hi)` -- or `on_ready(flat, lo, hi, fence)` when the callable has `takes_fence = True`:
        `fence()` returns the stream context in which that slice is visible, to be entered only when a collective is
        really launched -- is called as soon as every kernel writing flat[lo:hi] is enqueued
        (layers finish last-to-first, so the slices walk down from the tail): dp.GradReducer
        starts its all-reduce buckets there.
        The flat buffer is PERSISTENT (one per engine, the recorded plan holds its address): the views returned here --
        what p.grad becomes -- are overwritten by the next backward() of this engine."""
        S = self.grad_scale
        # data parallel: every PARAMETER gradient leaves the kernels already divided by the world size (it rides on the
        # 1 / grad_scale factor their finish passes apply anyway), so the summed all-reduce result is the average and no
        # separate 202 MB division pass follows it (dp.attach sets model._grad_div)
        D = S * float(getattr(self.model, "_grad_div", 1.0))
        if self._flat is None:
            # every element is written by the kernels (wgrad finish / dgamma / dbeta / dbias): no memset needed
            self._flat = torch.empty(self.total_params, dtype=torch.float32, device=self.device)
            self._gout = torch.empty(self.out_shape, dtype=torch.float32, device=self.device)
            self._sizes = [p.numel() for p in self.params]
        flat = self._flat
        # fresh view objects per call (autograd's AccumulateGrad adopts a gradient only when nobody else holds it): one
        # split + a reshape for the 4-d tensors
        views = [v if p.dim() == 1 else v.view(p.shape) for v, p in zip(flat.split_with_sizes(self._sizes), self.params)]
        gmap = {id(p): v for p, v in zip(self.params, views)}
        self._gout.copy_(grad_out.detach())      # the plan reads the logit gradient from a fixed address
        main = torch.cuda.current_stream(self.device)
        side = None
        if self.overlap_wgrad and self.events is None:    # per-kernel timing: one stream, no overlapping launches
            side = self._get_side_stream()
            # the side stream's split-K slabs must not alias the main stream's: with filter compaction the gather
            # layers run their weight gradient on the main stream while a side-stream one may still be in flight
            if self._side_ws is None or self._side_ws.numel() < self.wgrad_ws.numel():
                self._side_ws = torch.empty(self.wgrad_ws.numel(), dtype=torch.uint8, device=self.device)
                self._side_ws.record_stream(side)
                self._plan_epoch += 1

        def fence():
            """Stream context in which a collective over final slices may be enqueued: this block's slice is written from
            both streams (dgamma / dbeta and the gather layers' dW on the main one, dW on the side one), so the side stream
            first waits for everything the main stream has issued so far.  Called by the reducer only when it really
            launches a bucket (six times per dense step); entering it for every block cost 0.55 ms per step in the one-rank
            RCCL rehearsal (10.51 -> 9.96 ms)."""
            ev2 = torch.cuda.Event()
            ev2.record(main)
            side.wait_event(ev2)
            return torch.cuda.stream(side)

        def on_side():
            """The same context WITHOUT a new event: enough for every block whose weight gradient was handed to the second
            stream, because that hand-over already made the second stream wait for an event recorded on the launch stream
            BEHIND the block's BatchNorm backward -- the only launch-stream kernels that write into the block's slice
            (dgamma / dbeta; everything else, dW, dbias, the unfolded columns and dbeta of folded producers, is written by
            the second stream itself).  Saves the six event records per step the bucket launches put into the launch
            stream's queue."""
            return torch.cuda.stream(side)

        def ready(lay):
            if on_ready is None:
                return
            if side is None:
                on_ready(flat, lay.p_lo, lay.p_hi)
            elif getattr(on_ready, "takes_fence", False):
                # (the fused first block writes its whole slice on the launch stream: it needs the real fence; so does a
                # block whose weight gradient comes out of its one-launch backward, _bwd1x1_route)
                on_ready(flat, lay.p_lo, lay.p_hi,
                         fence if (lay.fused_stem or lay.stem_shadow or self._bwd1x1_route(lay)) else on_side)
            else:
                with fence():
                    on_ready(flat, lay.p_lo, lay.p_hi)

        if self.use_plan and self.events is None:
            key = (main.cuda_stream, side.cuda_stream if side is not None else 0, D, self._plan_epoch, self._ptr_sig())
            plan = self._bwd_plan
            if plan is None or plan.key != key:
                plan = ops.Plan([main] + ([side] if side is not None else []))
                seg_lays = [[]]

                def close_segment(lay):      # the block's slice of the flat buffer is final once this segment is enqueued
                    seg_lays[-1].append(lay)
                    plan.mark()
                    seg_lays.append([])
                with plan:
                    self._backward_body(gmap, main, side, S, D, close_segment)
                plan.key, plan.seg_lays = key, seg_lays
                self._bwd_plan = plan
            if on_ready is None:
                plan.run()
            else:
                for si in range(plan.segments):
                    plan.run(si, si + 1)
                    for lay in plan.seg_lays[si]:
                        ready(lay)
        else:
            self._backward_body(gmap, main, side, S, D, ready)
        return flat, views

    def _backward_body(self, gmap, main, side, S, D, ready):
        """The layer walk of the backward pass: library calls only (recordable); `ready(lay)` after the last launch that
        writes block `lay`'s slice of the flat gradient."""
        # Weight gradients go to the second stream in groups of `chunk` blocks (self.wgrad_chunk, 1 = each block
        # at once).  Every hand-over is an event record in the launch stream's queue plus a cross-queue wait; grouping 2-3
        # blocks per hand-over measured the same (9.63 / 9.64 / 9.64 ms per dense step), 4 and 6 slower (9.71 / 9.75: the
        # late start costs more overlap than the saved events).  dY and the block inputs stay in place until the next
        # forward, so a late start is safe.
        pending, chunk = [], self.wgrad_chunk
        sums_of = {}      # block -> slab its consumer's dgrad launch (issued earlier in this walk) left its sums in

        def flush():
            if not pending:
                return
            ops.stream_wait(side, main)           # dY of these blocks is complete on the launch stream
            with torch.cuda.stream(side):
                for fn, _ in pending:
                    fn(self._side_ws)
            for _, l in pending:
                ready(l)
            pending.clear()

        for lay in reversed(self.layers):
            if lay.stem_shadow:
                flush()
                # the first block's backward pass = the fused first block's, from the NHWC4 image, the plain-operand
                # coefficients of its own forward call and G
                cons = self.consumer_of[lay.out_id]
                mask = lay.conv.mask.contiguous() if lay.conv.mask_flag else None
                c = lay.sh_coef
                self._timed('wgrad', lay, ops.stem_block_bwd, self.B, lay.H, lay.W, lay.sh_img, lay.sh_wp,
                            lay.bn.weight.data, c[0], c[1], c[2], c[3], lay.slope, cons.gin, cons.tin.ld,
                            lay.out_t.choff, gmap[id(lay.conv.weight)], gmap[id(lay.bn.weight)], gmap[id(lay.bn.bias)],
                            lay.stem_ws, mask=mask, grad_scale=D)
                ready(lay)
                continue
            if lay.fused_stem:
                flush()
                # the whole backward of the first block in one pass over the image and G (conv_stem_block.hip)
                cons = self.consumer_of[lay.out_id]
                mask = lay.conv.mask.contiguous() if lay.conv.mask_flag else None
                self._timed('wgrad', lay, ops.stem_block_bwd, self.B, lay.H, lay.W, self.bufs[lay.tin.buf], lay.wp,
                            lay.bn.weight.data, lay.scale, lay.shift, lay.mean, lay.invstd, lay.slope, cons.gin, cons.tin.ld,
                            lay.out_t.choff, gmap[id(lay.conv.weight)], gmap[id(lay.bn.weight)], gmap[id(lay.bn.bias)],
                            lay.stem_ws, mask=mask, grad_scale=D)
                ready(lay)
                continue
            if lay.is_last:
                ops.nchw_to_padded(self._gout, lay.dy, lay.cout_p, 0, S, overflow=self.overflow, pad=lay.pad)
            else:
                cons = self.consumer_of[lay.out_id]
                t = lay.out_t
                g2 = g2_ld = g2_choff = None
                if lay.out2_id is not None and lay.out2_id in self.consumer_of:
                    c2, t2 = self.consumer_of[lay.out2_id], lay.out2_t
                    g2, g2_ld, g2_choff = c2.gin, c2.tin.ld, t2.choff
                self.bn_act_bwd_layer(lay, cons.gin, cons.tin.ld, t.choff, g2, g2_ld or 0, g2_choff or 0, lay.dy,
                                      gmap[id(lay.bn.weight)], gmap[id(lay.bn.bias)], D, sums=sums_of.pop(lay.li, None))
            mask = lay.conv.mask.contiguous() if lay.conv.mask_flag else None
            dbias = gmap[id(lay.conv.bias)] if lay.conv.bias is not None else None
            if self._bwd1x1_route(lay):
                # a narrow dense 1x1 block: G, the sums of the PLAIN block that produced its input and dW from ONE pass over
                # dY and the input, on the launch stream (timed under 'dgrad': the block has no 'wgrad' launch)
                flush()
                ds = self._dgrad_sums(lay, False, fused=True)
                if ds is not None:
                    sums_of[ds[2].li] = ds[1]
                self._timed('dgrad', lay, ops.conv_bwd1x1, lay.geom, self.bufs[lay.tin.buf], lay.dy, lay.cout_p, 0, lay.wd,
                            lay.gin, lay.tin.ld, lay.tin.choff, gmap[id(lay.conv.weight)], mask=mask, grad_scale=D, dbias=dbias,
                            workspace=self._bwd1x1_ws, overflow=self.overflow, sums=ds[0] if ds is not None else None)
                ready(lay)
                continue
            def wgrad_of(ws, lay=lay, mask=mask, dbias=dbias):
                """This block's weight gradient (nothing in the backward chain depends on it)."""
                if lay.fold is not None:
                    # kept input channels + the ones-channel: dense augmented gradient, then back to OIHW (the folded
                    # column expands to the dead inputs) and to dbeta of the producer's dead channels (csrc/fold.hip)
                    gw, prod = gmap[id(lay.conv.weight)], lay.fold
                    if lay.perm is not None:
                        ops.memset_zero(gw)
                    self._timed('wgrad', lay, ops.conv_wgrad, lay.geom_act, self.bufs[lay.tin.buf], lay.dy, lay.cout_p, 0,
                                lay.dwaug, None, D, dbias, ws)
                    ops.unfold_wgrad(lay.conv.weight.data, mask, lay.g_rows, lay.g_cols, prod.bn.bias.data, prod.slope, lay.n_act,
                                     lay.fold_cin, lay.dwaug, gw, gmap[id(prod.bn.bias)], gmap[id(prod.bn.weight)],
                                     accumulate=prod.fold_consumers[0] is not lay)
                elif lay.gather:
                    # kept filters only, in physical channel order; the finish kernel scatters to OIHW order.  Rows of
                    # removed filters are zero (as `grad * mask` makes them in the reference): zeroed here, not computed
                    gw = gmap[id(lay.conv.weight)]
                    if lay.perm is not None:
                        ops.memset_zero(gw)
                    self._timed('wgrad', lay, ops.conv_wgrad, lay.geom_act, self.bufs[lay.tin.buf], lay.dy, lay.cout_p, 0,
                                gw, mask, D, dbias, ws, rows=lay.g_rows, cols=lay.g_cols)
                elif lay.bw_on:
                    # the tiles and taps the block mask keeps only (Darknet.sparse_train = "block-wgrad")
                    _FORMS["bsparse_train"].wgrad(self, lay, gmap[id(lay.conv.weight)], mask, D, dbias, ws)
                else:
                    self._timed('wgrad', lay, ops.conv_wgrad, lay.geom, self.bufs[lay.tin.buf], lay.dy, lay.cout_p, 0,
                                gmap[id(lay.conv.weight)], mask, D, dbias, ws)

            if side is None:
                wgrad_of(self.wgrad_ws)
                ready(lay)
            else:
                # dY of this block is complete on the main stream: the weight gradient runs beside the dgrad /
                # BatchNorm-backward chain on the second stream (own split-K workspace) and fills its tails
                pending.append((wgrad_of, lay))
                if len(pending) >= chunk or lay.li <= 1:
                    flush()
            if lay.li > 0:
                # gradient wrt this block's input slice, written into gin at the slice's channel offset
                # (concurrent: the weight gradients run beside this launch and take the CUs it leaves idle, so the library
                # picks the tile with the least CU-time.  Not in the per-kernel timing mode, where every launch has the GPU
                # to itself: the layer table then shows the tile that is fastest alone -- three launches differ)
                # (... and where the input comes from a PLAIN block, the launch takes that block's BatchNorm-backward sums
                # from the tile it stores: _dgrad_sums)
                conc = side is not None and self._side_concurrent
                if lay.form == "bsparse_train" and lay.bs_dgrad:
                    _FORMS[lay.form].dgrad(self, lay, conc)
                    continue
                ds = self._dgrad_sums(lay, conc)
                if ds is not None:
                    sums_of[ds[2].li] = ds[1]
                self._timed('dgrad', lay, ops.conv_dgrad_raw, lay.geom_act, lay.dy, lay.cout_p, 0, lay.wd, lay.gin, lay.tin.ld,
                            lay.tin.choff, overflow=self.overflow, concurrent=conc, sums=ds[0] if ds is not None else None)
        if side is not None:
            flush()
            ops.stream_wait(main, side)
