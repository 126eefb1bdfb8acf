"""Model API of the reference's src/nets.py for the YOLOv2 path, MI355X-native underneath.

Kept surface (reference file:line): parse_cfg nets.py:39-73, print_cfg 75-190, the weight
(de)serialisers 194-279, MaxPoolStride1/Reorg/GlobalAvgPool2d/EmptyModule 640-688,
Darknet 692-1061 (blocks, models, loss, width/height, anchors..., header, seen, forward,
print_network, create_network, load_weights, save_weights, set_masks), getYOLOv2 1069-1074.
`state_dict()` keys and `parameters()` order are identical to the reference's, so its
checkpoints and mask lists interchange.

What differs: `Darknet.forward` does not call one torch module per block.  The block list is
compiled into a fused HIP launch plan (engine.py) that runs on the GPU only; a CPU tensor
raises instead of falling back to a PyTorch path.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import McamdError
from .pruning.weightPruning.layers import MaskedConv2d
from .pruning.weightPruning.methods import quick_filter_prune, weight_prune  # noqa: F401 (reference re-exports)
from .pruning.weightPruning.utils import prune_rate, are_masks_consistent  # noqa: F401
from .region_loss import RegionLoss, build_targets  # noqa: F401

USE_GPU = torch.cuda.is_available()


# ----------------------------------------------------------------------------- cfg
def parse_cfg(cfgfile, verbose=0):
    """Darknet .cfg -> list of dict blocks (nets.py:39-73).  A line is only rstrip()ped before
    the blank/'#' test; '[name]' opens a block; [convolutional] gets the int default
    batch_normalize=0; every other line must split on '=' into exactly two parts; the key
    'type' is stored as '_type'; values are stripped strings."""
    blocks = []
    block = None
    with open(cfgfile, 'r') as fp:
        for raw in fp:
            line = raw.rstrip()
            if line == '' or line[0] == '#':
                continue
            if line[0] == '[':
                if block:
                    if verbose:
                        print('')
                        print(' - block : ', block)
                    blocks.append(block)
                block = dict()
                block['type'] = line.lstrip('[').rstrip(']')
                if block['type'] == 'convolutional':
                    block['batch_normalize'] = 0
            else:
                key, value = line.split('=')
                key = key.strip()
                if key == 'type':
                    key = '_type'
                block[key] = value.strip()
    if block:
        blocks.append(block)
    return blocks


def cfg_shapes(blocks):
    """(input w, h, channels, output w, h, channels) of every non-[net] block of a parsed cfg, by the rules of the layer
    table (nets.py:75-190): the one place that walks a cfg's geometry (print_cfg, train's teacher check)."""
    prev_w = prev_h = prev_f = 0
    shapes = []
    for block in blocks:
        t = block['type']
        if t == 'net':
            prev_w, prev_h, prev_f = int(block['width']), int(block['height']), int(block['channels'])
            continue
        ind = len(shapes)
        w, h, f = prev_w, prev_h, prev_f
        if t == 'convolutional':
            f, k, s = int(block['filters']), int(block['size']), int(block['stride'])
            pad = (k - 1) // 2 if int(block['pad']) else 0
            w, h = (prev_w + 2 * pad - k) // s + 1, (prev_h + 2 * pad - k) // s + 1
        elif t == 'maxpool':
            s = int(block['stride'])
            w, h = prev_w // s, prev_h // s
        elif t == 'reorg':
            s = int(block['stride'])
            f, w, h = s * s * prev_f, prev_w // s, prev_h // s
        elif t == 'route':
            layers = [int(i) if int(i) > 0 else int(i) + ind for i in block['layers'].split(',')]
            prev_w, prev_h = w, h = shapes[layers[0]][3], shapes[layers[0]][4]
            prev_f = f = sum(shapes[l][5] for l in layers)
        shapes.append((prev_w, prev_h, prev_f, w, h, f))
        prev_w, prev_h, prev_f = w, h, f
    return shapes


def print_cfg(blocks):
    """Layer table like nets.py:75-190 (index, type, filters, size, input -> output)."""
    print('layer     filters    size              input                output')
    shapes = cfg_shapes(blocks)
    ind = -1
    for block in blocks:
        t = block['type']
        if t == 'net':
            continue
        ind += 1
        prev_w, prev_h, prev_f, w, h, f = shapes[ind]
        if t == 'convolutional':
            k, s = int(block['size']), int(block['stride'])
            print('%5d %-6s %4d  %d x %d / %d   %3d x %3d x%4d   ->   %3d x %3d x%4d' % (
                ind, 'conv', f, k, k, s, prev_w, prev_h, prev_f, w, h, f))
        elif t == 'maxpool':
            k, s = int(block['size']), int(block['stride'])
            print('%5d %-6s       %d x %d / %d   %3d x %3d x%4d   ->   %3d x %3d x%4d' % (
                ind, 'max', k, k, s, prev_w, prev_h, prev_f, w, h, prev_f))
        elif t == 'reorg':
            s = int(block['stride'])
            print('%5d %-6s              / %d   %3d x %3d x%4d   ->   %3d x %3d x%4d' % (
                ind, 'reorg', s, prev_w, prev_h, prev_f, w, h, f))
        elif t == 'route':
            layers = [int(i) if int(i) > 0 else int(i) + ind for i in block['layers'].split(',')]
            print('%5d %-6s %s' % (ind, 'route', ' '.join(str(l) for l in layers)))
        elif t == 'region':
            print('%5d %-6s' % (ind, 'detection'))
        else:
            print('unknown type %s' % t)


# ----------------------------------------------------------------------------- weight files
def convert2cpu(gpu_matrix):
    return torch.FloatTensor(gpu_matrix.size()).copy_(gpu_matrix)


def load_param(file, param):
    """nets.py:256-259: the next param.numel() float32 values of the open file."""
    buf = np.fromfile(file, dtype=np.float32, count=param.numel())
    if buf.size != param.numel():
        raise EOFError("weights file ended inside a %s parameter" % (tuple(param.shape),))
    param.data.copy_(torch.from_numpy(buf.reshape(tuple(param.shape))))


def load_conv(file, conv_model):
    load_param(file, conv_model.bias)
    load_param(file, conv_model.weight)


def load_conv_bn(file, conv_model, bn_model):
    """nets.py:270-276 order: bn.bias, bn.weight, running_mean, running_var, conv.weight."""
    load_param(file, bn_model.bias)
    load_param(file, bn_model.weight)
    load_param(file, bn_model.running_mean)
    load_param(file, bn_model.running_var)
    load_param(file, conv_model.weight)


def load_fc(file, fc_model):
    load_param(file, fc_model.bias)
    load_param(file, fc_model.weight)


def _tofile(t, fp):
    t.detach().cpu().numpy().astype(np.float32, copy=False).tofile(fp)


def save_conv(fp, conv_model):
    _tofile(conv_model.bias.data, fp)
    _tofile(conv_model.weight.data, fp)


def save_conv_bn(fp, conv_model, bn_model):
    _tofile(bn_model.bias.data, fp)
    _tofile(bn_model.weight.data, fp)
    _tofile(bn_model.running_mean, fp)
    _tofile(bn_model.running_var, fp)
    _tofile(conv_model.weight.data, fp)


def save_fc(fp, fc_model):
    _tofile(fc_model.bias.data, fp)
    _tofile(fc_model.weight.data, fp)


# ----------------------------------------------------------------------------- glue modules
class MaxPoolStride1(nn.Module):
    def forward(self, x):
        return F.max_pool2d(F.pad(x, (0, 1, 0, 1), mode='replicate'), 2, stride=1)


class Reorg(nn.Module):
    """nets.py:648-667 (marvis ordering): out channel = (hs*stride + ws)*C + c.  Inside a
    Darknet the reorg is fused into the producing conv's activation kernel; this module keeps
    the class for API parity and for use on its own."""

    def __init__(self, stride=2):
        super(Reorg, self).__init__()
        self.stride = stride

    def forward(self, x):
        s = self.stride
        assert x.dim() == 4
        B, C, H, W = x.shape
        assert H % s == 0 and W % s == 0
        x = x.view(B, C, H // s, s, W // s, s).transpose(3, 4).contiguous()
        x = x.view(B, C, (H // s) * (W // s), s * s).transpose(2, 3).contiguous()
        x = x.view(B, C, s * s, H // s, W // s).transpose(1, 2).contiguous()
        return x.view(B, s * s * C, H // s, W // s)


class GlobalAvgPool2d(nn.Module):
    def forward(self, x):
        N, C, H, W = x.shape
        return F.avg_pool2d(x, (H, W)).view(N, C)


class EmptyModule(nn.Module):
    def forward(self, x):
        return x


# ----------------------------------------------------------------------------- autograd bridge
class _DarknetFn(torch.autograd.Function):
    """logits = engine.forward(x); backward hands every parameter its gradient as a view of one
    flat fp32 buffer (bucket-free all-reduce for data parallel training).

    The 134 parameters are NOT inputs of this node: one `anchor` tensor is, so that autograd calls backward() at all, and
    backward() stores the gradients itself -- `p.grad = view` (or `p.grad += view` when a gradient is already there: the
    accumulation semantics of loss.backward()).  134 AccumulateGrad nodes and a 134-tensor argument tuple per step cost
    0.7 ms of host time (tools/host_profile.py), a third of a step's enqueue time.  What this gives up: tensor hooks on
    the parameters and torch.autograd.grad(loss, params) -- neither is used on the reference's path (train.py:224-235)."""

    @staticmethod
    def forward(ctx, model, engine, training, x, anchor):
        out = engine.forward(x, training)
        ctx.model, ctx.engine, ctx.serial, ctx.training = model, engine, engine.serial, training
        return out

    @staticmethod
    def backward(ctx, gout):
        eng = ctx.engine
        if ctx.needs_input_grad[3]:
            raise McamdError("gradient wrt the input image is not provided (the first conv has no dgrad)")
        if not ctx.training:
            raise McamdError("backward through an eval-mode forward is not supported; call model.train()")
        if eng.serial != ctx.serial:
            raise McamdError("backward() must follow the forward() it belongs to (activations are kept in place)")
        # gradients already present (no zero_grad() since the last backward) are accumulated into, as autograd would; they
        # may alias the engine's persistent flat buffer, so they are saved first (rare path)
        prev = [(i, p.grad.clone()) for i, p in enumerate(eng.params) if p.grad is not None]
        flat, views = eng.backward(gout, on_ready=ctx.model._grad_ready_hook)
        ctx.model._last_flat_grad = flat
        hook = ctx.model._grad_hook
        if hook is not None:
            hook(flat)
        for i, g in prev:
            views[i].add_(g)
        for p, v in zip(eng.params, views):
            if p.requires_grad:
                p.grad = v
        return None, None, None, None, None


# ----------------------------------------------------------------------------- Darknet
class Darknet(nn.Module):
    def __init__(self, cfgfile, verbose=0):
        super(Darknet, self).__init__()
        self.blocks = parse_cfg(cfgfile)
        self.models = self.create_network(self.blocks)  # merge conv, bn, leaky
        self.loss = self.models[len(self.models) - 1]

        self.width = int(self.blocks[0]['width'])
        self.height = int(self.blocks[0]['height'])

        if self.blocks[(len(self.blocks) - 1)]['type'] == 'region':
            self.anchors = self.loss.anchors
            self.num_anchors = self.loss.num_anchors
            self.anchor_step = self.loss.anchor_step
            self.num_classes = self.loss.num_classes
            if verbose:
                print('  -- [Darknet] anchors %s num_anchors %s anchor_step %s num_classes %s' % (
                    self.anchors, self.num_anchors, self.anchor_step, self.num_classes))

        self.header = torch.IntTensor([0, 0, 0, 0])
        self.seen = 0
        # engine state (not part of the reference surface)
        self._engines = {}
        self._weights_dirty = True      # raised by _mark_weights_replaced(), cleared by the first engine that packs
        self._weights_serial = 0        # ... and how often it was raised: what every further engine goes by
        self._ws_table = None           # project_codebooks: the cached table over the tied layers (share.py)
        self._grad_hook = None          # callable(flat_grad) run at the end of backward (data parallel)
        self._grad_ready_hook = None    # callable(flat_grad, lo, hi[, fence]): that slice is final (overlapped all-reduce; Engine.backward)
        self._last_flat_grad = None
        self._anchor = None             # the one differentiable input of the autograd node (see _DarknetFn)
        self.grad_scale = 256.0         # fp16 gradient scaling inside the engine, undone in fp32
        # Operand precision of the forward convolutions (engine.py): "fp16" (plain operands: the throughput opt-in),
        # "fp16x3" (split hi/lo operands on every block, three fp16 MFMA products per multiply), "mixed" (split except on
        # the costliest blocks the 1e-3 logit budget leaves plain -- in eval AND in training, where the budget is tighter:
        # engine.MIXED_BUDGET_TRAIN), or "auto" = "mixed" in BOTH modes (round 4) -- so that the drop-in reproduces the
        # reference's fp32 region-layer logits within 1e-3 (north_star) by default, as the reference itself computes in
        # fp32 end to end (layers.py:59-64, train.py:224-235).  Training in plain fp16 does NOT meet 1e-3 end to end on
        # a random-init network (3.2e-2 at B=64; the fp32 oracle with fp16-rounded storage: 3.7e-2) and is 1.35x faster:
        # `model.precision = "fp16"` / MCAMD_PRECISION=fp16 selects it explicitly (bench.py reports both).
        # "fp8" (an addition beyond the reference, eval only): post-training quantised inference -- the "fp16" engine with every
        # eligible block (engine.Engine.fp8_layers: conv3-conv22 of YOLOv2-VOC) on e4m3 activations and weights, fp32
        # accumulation, no calibration data (csrc/conv_q8.hip; MCAMD_Q8_MFMA picks the MFMA form).  A training-mode
        # forward raises.  "fp8-2:4": the "fp8" engine with every fp8 block whose mask conforms to 2:4 (nm_prune) on the sparse
        # fp8 MFMA kernel (engine.Engine.fp8_sparse_layers, csrc/conv_q8_sparse.hip); `sparse` stays None with it.
        # "fp8-splitk" (eval only): the "fp8" engine for one image at a time -- every fp8 block whose launch would leave most CUs
        # idle runs as a split-K pair on the same byte operands (engine.Engine.fp8_splitk_layers, csrc/conv_q8_splitk.hip,
        # DESIGN.md 3v); batches the policy does not split run exactly what "fp8" runs; `splitk` stays False with it.
        # "fp8-qat" (an addition beyond the reference): fp8 quantisation-aware training -- in training mode the blocks of
        # engine.Engine.fp8_layers run their forward in the "fp8" arithmetic on batch statistics and a straight-through backward
        # on the fp16 kernels, every other block trains as in "fp16"; in eval mode it is the "fp8" engine, bit for bit
        # (DESIGN.md 3l).  The fine-tuning step between pruning / retraining and deployment under "fp8" or "fp8-2:4".
        # "fp8-w4" (eval only, an opt-in): the "fp8" engine with the weights of every dense fp8 block held as 4-bit e2m1 codes
        # + one shift per group of 32 input channels, 4.25 bits per weight resident, expanded to e4m3 bytes in the kernel's
        # registers (engine.Engine.fp8_w4_layers, csrc/conv_q8_w4.hip); `sparse` and `splitk` stay off with it.
        # "fp8-w4-qat" (an addition beyond the reference): 4-bit quantisation-aware training -- "fp8-qat" with the weights of every
        # fp8 block re-quantised to the "fp8-w4" format every step: the training-mode forward multiplies the codes the block would
        # be deployed with, the backward is straight-through on the values they stand for; in eval mode it is the "fp8-w4" engine,
        # bit for bit.  The fine-tuning step in front of deployment under "fp8-w4"; `sparse` and `splitk` stay off.
        # "fp8-block" (eval only, an addition beyond the reference): the "fp8" engine for block-pruned models -- every masked fp8
        # block whose kept fraction of (64-filter tile, 64-byte K chunk) pairs is at most `fp8_block_max_kept` keeps its filters
        # out of the compaction and multiplies only the chunks that hold a non-zero weight byte
        # (engine.Engine.fp8_block_layers / fp8_block_kept, csrc/conv_q8_bsparse.hip); with nothing chosen it is
        # the "fp8" engine bit for bit.  What block_prune + "fp8-qat" fine-tuning deploy to; `sparse` and `splitk` stay off.
        self.precision = os.environ.get("MCAMD_PRECISION", "auto")
        from .engine import Q8_BSPARSE_MAX_KEPT
        self.fp8_block_max_kept = Q8_BSPARSE_MAX_KEPT    # the policy constant of "fp8-block" (engine.py)
        # 2:4 structured-sparse inference (an addition beyond the reference): "2:4" runs every eligible block whose mask
        # keeps at most 2 of every 4 consecutive input channels (pruning.weightPruning.methods.nm_prune) on the sparse MFMA
        # (engine.Engine.sparse_layers).  "block" runs every eligible masked block on the block-sparse kernel
        # (csrc/conv_bsparse.hip): per 64-filter tile it multiplies only the K chunks of the packed weights that
        # hold a non-zero value -- what pruning.weightPruning.methods.block_prune zeroes is skipped, bit-identically to
        # multiplying it -- provided the layer's kept-chunk fraction is at most `sparse_max_kept`
        # (engine.Engine.bsparse_layers).  Eval with precision "fp16" only -- other eval precisions raise; training ignores it.
        self.sparse = None
        from .engine import BSPARSE_MAX_KEPT
        self.sparse_max_kept = BSPARSE_MAX_KEPT      # the measured policy constant (engine.py)
        # Block-sparse TRAINING (an addition beyond the reference): "block" runs the forward and the dgrad launch
        # of every masked inner block whose kept-chunk fraction is at most `sparse_train_max_kept` on the raw-epilogue form of
        # the block-sparse kernel (engine.Engine.bsparse_train_layers / bsparse_train_dgrad_layers / bsparse_train_kept): the
        # zero blocks of block_prune / taylor_prune(granularity="block") masks are skipped, bit-identically to multiplying
        # them.  The weight gradient stays dense.  Training-mode passes with precision "fp16" only -- any other training
        # precision raises; eval ignores it (`sparse` is the eval switch, and training keeps ignoring that one).  A bound of
        # 0.0, or a model without masks, is the engine of sparse_train = None bit for bit.
        # "block-wgrad"  does everything "block" does and also sends the weight gradient of the chosen blocks
        # that are neither compacted nor on the one-launch 1x1 backward through the list launch mcamd_conv_wgrad_bsparse when
        # the kept fraction of their (64 x 64 tile, tap) pairs is at most `sparse_train_wgrad_max_kept`
        # (engine.Engine.bsparse_train_wgrad_layers / bsparse_train_wgrad_kept): masked tiles and taps are never computed and
        # their gradient is exactly 0.  The lists come from the masks when the masks change, never per step.  A bound of 0.0
        # is "block" bit for bit.
        self.sparse_train = None
        from .engine import BSPARSE_TRAIN_MAX_KEPT, BSPARSE_TRAIN_WGRAD_MAX_KEPT
        self.sparse_train_max_kept = BSPARSE_TRAIN_MAX_KEPT      # the measured policy constant (engine.py)
        self.sparse_train_wgrad_max_kept = BSPARSE_TRAIN_WGRAD_MAX_KEPT      # ... and the weight gradient's
        # Low-batch inference (an addition beyond the reference): True runs every block whose forward launch would leave most
        # CUs idle -- the 13x13 and 26x26 layers at B = 1 -- as a split-K pair (csrc/conv_splitk.hip, DESIGN.md 3p,
        # engine.Engine.splitk_layers); batches the policy does not split run exactly what they run without it.  Eval with
        # precision "fp16" only -- other eval precisions raise; training ignores it.  MCAMD_SPLITK=1 sets the default.
        self.splitk = os.environ.get("MCAMD_SPLITK", "0") == "1"

    # ---- engine plumbing
    def _mark_weights_replaced(self):
        """The weights (or masks) were replaced behind the engines' backs: every engine re-packs, and reads what it derives
        from the weights on the host again, before its next forward.  `_weights_dirty` is the flag the first engine that
        packs clears; `_weights_serial` counts the calls, and each engine compares it with the count it last packed at
        (Engine.pack) -- a model has up to three engines, and the flag alone reaches only the first of them."""
        self._weights_dirty = True
        self._weights_serial += 1

    def _apply(self, fn, *args, **kwargs):
        self._engines = {}
        self._mark_weights_replaced()
        self._ws_table = None
        return super(Darknet, self)._apply(fn, *args, **kwargs)

    def grad_overflowed(self, reset=True):
        """True when a backward pass since the last call had to clamp a scaled gradient (grad_scale x dY / dX) to the
        fp16 range: the engine saturates instead of producing inf, so the step's gradients are finite but wrong.
        One host sync.  train.py skips such a step and halves `grad_scale` (all ranks together)."""
        hit = False
        for eng in self._engines.values():
            if int(eng.overflow.item()):
                hit = True
                if reset:
                    eng.overflow.zero_()
        return hit

    def invalidate_packed(self):
        """Call after modifying weights through `.data` outside optimizer.step / set_masks / load_weights."""
        self._mark_weights_replaced()

    def load_state_dict(self, *args, **kwargs):
        self._mark_weights_replaced()
        return super(Darknet, self).load_state_dict(*args, **kwargs)

    def _engine_for(self, x):
        from .engine import Engine
        prec = self.precision
        if prec == "auto":
            prec = "mixed"
        # "mixed" has two budgets: the training-mode forward amplifies operand rounding of the early blocks (engine.py)
        for_training = bool(self.training and prec == "mixed")
        # training and inference engines differ in their activation layout (the small images of a training engine are in the
        # shared-halo form, engine.py), so each mode has its own
        key = (tuple(x.shape), x.device.index, float(self.grad_scale), prec, for_training, bool(self.training))
        eng = self._engines.get(key)
        if eng is None:
            if len(self._engines) >= 3:
                self._engines.pop(next(iter(self._engines)))
            eng = Engine(self, x.shape[0], x.shape[2], x.shape[3], x.device, self.grad_scale, prec, for_training,
                         train_layout=bool(self.training))
            self._engines[key] = eng
        return eng

    def forward(self, x):
        """nets.py:720-774: returns the last conv block's output (the [region] block is skipped;
        the caller applies the loss).  NCHW fp32 in, NCHW fp32 out."""
        if not x.is_cuda:
            raise McamdError("Darknet.forward needs a CUDA (MI355X) tensor: modelcompression_amd has no CPU path "
                             "(the CPU restatement lives in oracle/ and is test infrastructure)")
        eng = self._engine_for(x)
        if self._anchor is None or self._anchor.device != x.device:
            self._anchor = torch.zeros(1, device=x.device, requires_grad=True)
        if not torch.is_grad_enabled():
            return eng.forward(x, self.training)
        return _DarknetFn.apply(self, eng, self.training, x, self._anchor)

    def detect(self, images, conf_thresh=0.25, nms_thresh=0.45):
        """Eval forward plus the fused post-processing (nets2_utils.detections_device): device tensors
        (rows [B, N, 8], probs [B, N, C], nkept [B]) with no host synchronisation, in every eval precision."""
        from .nets2_utils import detections_device
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                out = self(images)
            return detections_device(out, conf_thresh, nms_thresh, self.num_classes, self.anchors, self.num_anchors)
        finally:
            self.train(was_training)

    def print_network(self):
        print_cfg(self.blocks)

    def create_network(self, blocks):
        """nets.py:779-895: one module per non-[net] block, so that `models[i]` pairs with `blocks[i + 1]` and
        `state_dict()` keys read `models.{i}.conv{id}.weight`.  Table-driven over the block types the engine runs
        (convolutional, maxpool, reorg, route, region, cost); the reference's other branches (avgpool, softmax,
        shortcut, connected: Darknet classifier / residual blocks that no YOLOv2 cfg of this project uses and the
        engine has no kernels for) raise instead of building modules that could never execute."""
        models = nn.ModuleList()
        widths = []                     # output channels of every module built so far
        state = {"prev": 3, "conv_id": 0}

        def conv(block):
            state["conv_id"] += 1
            cid, k, filters = state["conv_id"], int(block['size']), int(block['filters'])
            pad = int((k - 1) / 2) if int(block['pad']) else 0          # 1x1 convs get pad 0 despite pad=1 (nets.py:796)
            bn = int(block['batch_normalize'])
            seq = nn.Sequential()
            seq.add_module('conv%d' % cid, MaskedConv2d(state["prev"], filters, k, int(block['stride']), pad, bias=not bn))
            if bn:
                seq.add_module('bn%d' % cid, nn.BatchNorm2d(filters))
            act = {'leaky': lambda: nn.LeakyReLU(0.1, inplace=True), 'relu': lambda: nn.ReLU(inplace=True)}.get(block['activation'])
            if act is not None:
                seq.add_module('%s%d' % (block['activation'], cid), act())
            state["prev"] = filters
            return seq, filters

        def maxpool(block):
            stride = int(block['stride'])
            return (nn.MaxPool2d(int(block['size']), stride) if stride > 1 else MaxPoolStride1()), state["prev"]

        def reorg(block):
            stride = int(block['stride'])
            state["prev"] = stride * stride * state["prev"]
            return Reorg(stride), state["prev"]

        def route(block):
            ind = len(models)
            src = [int(i) if int(i) > 0 else int(i) + ind for i in block['layers'].split(',')]
            if len(src) == 2:
                assert src[0] == ind - 1                                # nets.py:855
            if len(src) in (1, 2):
                state["prev"] = sum(widths[i] for i in src)
            return EmptyModule(), state["prev"]

        def region(block):
            loss = RegionLoss()
            loss.anchors = [float(i) for i in block['anchors'].split(',')]
            loss.num_classes = int(block['classes'])
            loss.num_anchors = int(block['num'])
            loss.anchor_step = len(loss.anchors) / loss.num_anchors
            for key in ('object_scale', 'noobject_scale', 'class_scale', 'coord_scale'):
                setattr(loss, key, float(block[key]))
            return loss, state["prev"]

        def cost(block):
            kinds = {'sse': nn.MSELoss, 'L1': nn.L1Loss, 'smooth': nn.SmoothL1Loss}
            return kinds[block['_type']](reduction='mean'), 1

        builders = {'convolutional': conv, 'maxpool': maxpool, 'reorg': reorg, 'route': route, 'region': region, 'cost': cost}
        for block in blocks:
            t = block['type']
            if t == 'net':
                state["prev"] = int(block['channels'])
                continue
            if t not in builders:
                raise NotImplementedError("cfg block [%s] is outside the YOLOv2 path this package executes "
                                          "(supported: %s)" % (t, ', '.join(sorted(builders))))
            module, width = builders[t](block)
            models.append(module)
            widths.append(width)
        return models

    def load_weights(self, weightfile):
        """nets.py:897-948: 3 x int32 major/minor/revision, `seen` as int64 when
        major*10+minor >= 2 (both < 1000) else int32, then the conv blocks in order.
        A file that begins with the magic of a compressed model file (compress.py) goes to load_compressed:
        a Darknet file cannot begin with it, its first int32 is a small version number."""
        from . import compress
        if compress.is_compressed(weightfile):
            compress.load_compressed(self, weightfile)
            return
        with open(weightfile, mode='rb') as f:
            major = int(np.fromfile(f, dtype=np.int32, count=1)[0])
            minor = int(np.fromfile(f, dtype=np.int32, count=1)[0])
            revision = int(np.fromfile(f, dtype=np.int32, count=1)[0])
            if major * 10 + minor >= 2 and major < 1000 and minor < 1000:
                seen = int(np.fromfile(f, dtype=np.int64, count=1)[0])
            else:
                seen = int(np.fromfile(f, dtype=np.int32, count=1)[0])
            # like the reference, the header values are read and dropped here (nets.py:899-905):
            # only load_weights_old() keeps `header` / `seen`.
            del revision, seen
            ind = -2
            for block in self.blocks:
                if ind >= len(self.models):
                    break
                ind = ind + 1
                if block['type'] == 'net':
                    continue
                elif block['type'] == 'convolutional':
                    model = self.models[ind]
                    if int(block['batch_normalize']):
                        load_conv_bn(f, model[0], model[1])
                    else:
                        load_conv(f, model[0])
                elif block['type'] == 'connected':
                    model = self.models[ind]
                    load_fc(f, model[0] if block['activation'] != 'linear' else model)
        self._mark_weights_replaced()

    def load_weights_old(self, weightfile):
        """nets.py:950-1005: 4 x int32 header (kept in self.header, seen = header[3]), then floats."""
        with open(weightfile, 'rb') as f:
            header = np.fromfile(f, count=4, dtype=np.int32)
            self.header = torch.from_numpy(header)
            self.seen = self.header[3]
            ind = -2
            for block in self.blocks:
                ind = ind + 1
                if block['type'] == 'convolutional':
                    model = self.models[ind]
                    if int(block['batch_normalize']):
                        load_conv_bn(f, model[0], model[1])
                    else:
                        load_conv(f, model[0])
                elif block['type'] == 'connected':
                    model = self.models[ind]
                    load_fc(f, model[0] if block['activation'] != 'linear' else model)
        self._mark_weights_replaced()

    def save_weights(self, outfile, cutoff=0):
        """nets.py:1007-1051: header int32 [major, minor, revision, seen] (so a saved file always
        re-loads through the int32-`seen` branch when the header is the default [0,0,0,*])."""
        if cutoff <= 0:
            cutoff = len(self.blocks) - 1
        with open(outfile, 'wb') as fp:
            self.header[3] = int(self.seen)
            self.header.numpy().tofile(fp)
            ind = -1
            for blockId in range(1, cutoff + 1):
                ind = ind + 1
                block = self.blocks[blockId]
                if block['type'] == 'convolutional':
                    model = self.models[ind]
                    if int(block['batch_normalize']):
                        save_conv_bn(fp, model[0], model[1])
                    else:
                        save_conv(fp, model[0])
                elif block['type'] == 'connected':
                    model = self.models[ind]
                    save_fc(fp, model[0] if block['activation'] != 'linear' else model)

    def save_compressed(self, outfile, payload="fp16", layers=None, entropy=None):
        """Write a compressed model file (an addition beyond the reference; compress.save_compressed).
        payload "shared": codebooks + narrow codes of the layers set_codebooks tied; payload "w4": the 4-bit
        codes, group shifts and filter exponents the "fp8-w4" engine consumes.  entropy "huffman": the coded
        container, which load_weights and load_compressed read like the plain one."""
        from . import compress
        compress.save_compressed(self, outfile, payload, layers, entropy)

    def load_compressed(self, weightfile, set_masks=True):
        """Read a compressed model file; returns the kept-bit masks (compress.load_compressed).  A "shared" file also
        sets the codebooks."""
        from . import compress
        return compress.load_compressed(self, weightfile, set_masks)

    def set_codebooks(self, codebooks):
        """Tie the weights (an addition beyond the reference; share.py): `codebooks` is what
        share.kmeans_share returns, one (codebook, codes) or None per conv block in set_masks order.  Registers the buffers
        `codebook` and `codes` on each MaskedConv2d named -- only here, like set_mask: an untied model's state_dict is
        unchanged --, sets its weights to codebook[codes] on kept positions and raises its share_flag."""
        from . import share
        share.set_codebooks(self, codebooks)

    def project_codebooks(self):
        """Put every cluster of every tied layer back on its mean (share.py): call it behind optimizer.step().  On the GPU one
        library call over all tied layers with no host synchronisation; every engine re-packs before its next forward."""
        from . import share
        share.project_codebooks(self)

    def set_masks(self, masks):
        """nets.py:1053-1061: hand masks[count] to every MaskedConv2d in module order.  Like the
        reference, failures are swallowed (a too-short list leaves the remaining layers unmasked)."""
        count = 0
        for m in self.modules():
            try:
                if m[0].name == 'MaskedConv2d':
                    m[0].set_mask(masks[count])
                    count += 1
            except Exception:
                pass
        self._mark_weights_replaced()


def debug_weights(model):
    for name, param in model.named_parameters():
        if param.requires_grad and param.grad is not None:
            print('  -- [DEBUG] : ', name, '\t  - \t', round(param.grad.data.sum().item(), 3), '   [', param.shape, ']')


def getYOLOv2(cfgfile, weightfile):
    """nets.py:1069-1074."""
    model = Darknet(cfgfile)
    model.load_weights(weightfile)
    if USE_GPU:
        model.cuda()
    return model
