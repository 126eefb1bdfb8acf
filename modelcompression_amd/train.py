"""Retrain entry point: mirror of the reference's src/train.py (YOLOv2Train.train, 67-290).

Same signature and the same sequence -- build Darknet from the cfg, load .weights, SGD with
lr 1e-5 / momentum / weight_decay = decay*BATCH_SIZE (train.py:144-147), optional pruning +
set_masks (167-174), epochs of forward / RegionLoss / zero_grad / backward / step (214-235),
per-epoch prune_rate + are_masks_consistent and a checkpoint every 5th epoch when pruning
(247-252) -- with the model running on the HIP engine.  Differences, all additive:
  * launched under torch.distributed (one process per GPU) it shards each batch across the
    ranks and averages gradients with one flat all-reduce per step (RCCL over xGMI);
  * masks are computed on rank 0 and broadcast;
  * `torch.autograd.detect_anomaly()` / pdb of the reference are not entered (a non-finite loss
    raises instead);
  * when the image list is missing, a seeded synthetic detection set of the same shapes is
    used so the entry point can be exercised without VOC on disk;
  * MAX_EPOCHS can be given to stop early (the reference hard-codes 135);
  * AUGMENT=True trains on the reference's train=True augmentation (dataloader.py:68-75): data.VOCAugment (or
    data.SyntheticAugment without a list) decodes and draws parameters, augment.DeviceAugmenter does the pixels in
    one HIP launch pair per batch on the training stream.  Off by default.
  * RESIDENT=True decodes the train list once into device memory (data.ResidentImages; every rank keeps the whole
    set) and trains from it with no loader workers: data.ResidentAugment with AUGMENT, data.ResidentList without;
    with EVAL the evaluation pictures are made resident once, for every epoch's predict.  Off by default.
  * TEACHER adds knowledge distillation to the retraining (distill.py): True = a frozen copy of the model as loaded, taken
    before pruning (the common case: `pruning_perc=80, TEACHER=True`), a path = a Darknet of MODEL_CFG with those weights,
    or a Darknet of the caller's (its own cfg and eval `precision`; that object itself is used: it is moved to the
    device, put in eval mode and frozen with requires_grad_(False), in place).  Anything else, False included, raises.
    The teacher stays in eval mode without masks,
    optimizer entry or gradient hook; every step runs its forward under no_grad in front of the student's and adds
    DISTILL(output, teacher_output) -- a distill.DistillLoss, by default DistillLoss.from_model(model) -- to the region
    loss.  Off by default: the same launches and results as without the keywords.
  * SHARE=4 (bits), or a dict of share.kmeans_share keywords, adds weight sharing to the retraining (share.py, DESIGN.md
    3u): behind pruning and set_masks every conv layer's kept weights are clustered into 2^bits shared values
    (kmeans_share + Darknet.set_codebooks), and Darknet.project_codebooks() behind every optimizer.step() puts each
    cluster back on its mean -- SGD on the shared values with the mean member gradient.  Each epoch prints whether every
    tied layer still holds at most 2^bits distinct kept values.  Given by keyword only (the positional parameters of train()
    stay as they were: a wrapper takes the keyword off), or set as the attribute YOLOv2Train.SHARE, which the keyword
    overrides.  Off by default: the same launches and results as without it.
  * YOLOv2Train.SAVE_COMPRESSED = "fp32" / "fp16" / "w4" / "fp8" / "shared" (an attribute, set on the class or on the object before
    train() is called: the signature of train() stays the reference's plus the keywords above) writes a compressed model
    file of that payload (compress.py) beside every .weights file saved, with the extension .mcz.
    MODEL_WEIGHT and a TEACHER path may name such a file: Darknet.load_weights recognises it, and train() resumes at the
    epoch the file's `seen` stands for (a .weights file drops `seen`, as in the reference).  None by default: the same
    files as before.  YOLOv2Train.SAVE_COMPRESSED_ENTROPY = "huffman" (an attribute too) makes that file a Huffman-coded one
    (DESIGN.md 3z), which load_weights reads the same way; None by default.
  * pruning_method = "taylor-weight" / "taylor-block" / "taylor-filter" ranks by first-order Taylor importance instead of
    magnitude (importance.py): before pruning, YOLOv2Train.TAYLOR_STEPS batches of the training loader go
    through forward, loss (with the distillation term when there is a TEACHER) and backward in training mode, WITHOUT an
    optimizer step; importance.TaylorImportance.accumulate adds each step's scores in one launch, skipped on the device
    when StepGuard flags the step.  The BatchNorm running statistics are put back afterwards.  With several ranks each
    scores its own shard and the accumulators are all-reduced.  Every other method value behaves as before.
  * YOLOv2Train.SPARSE_TRAIN = "block" (an attribute; None by default: train() is what it was) sets Darknet.sparse_train on the
    model behind set_masks: with pruning_method "block" or "taylor-block" and the training precision "fp16", the forward and
    dgrad launches of the retraining steps skip the zeroed blocks of every layer whose kept fraction is at most the model's
    default bound (engine.BSPARSE_TRAIN_MAX_KEPT).  SPARSE_TRAIN = "block-wgrad" also runs their weight
    gradient on the tiles and taps the masks keep (engine.BSPARSE_TRAIN_WGRAD_MAX_KEPT).
  * YOLOv2Train.GROUP_LASSO = {"lam": float, "granularity": "block" | "filter"} (an attribute; None by default: train()
    issues the launches it issued before and nothing more) learns structured sparsity while training (sparsify.py, DESIGN.md
    3ze): a sparsify.GroupLasso is built behind set_masks, and its proximal step -- one launch over all layers, at the
    optimizer's learning rate, skipped on the device when StepGuard flags the step -- runs behind every optimizer.step().
    "block" shrinks block_prune's blocks of the conv weights, "filter" the BatchNorm gammas.  Each epoch logs the fraction of
    zero groups; before every checkpoint and at the end model.set_masks(gl.masks()) turns the zero groups into ordinary
    masks, so the .weights / .mcz files and the later engines see them as any pruner's.  Data-parallel ranks hold identical
    weights after the all-reduced step and the proximal step is a deterministic function of the weights: nothing travels.
    SHARE together with GROUP_LASSO raises (the projection and the proximal step would undo each other).  The object is kept
    as YOLOv2Train.group_lasso.
"""
import os

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC for RCCL: read when HIP initialises (dp.init_from_env)

import functools  # noqa: E402
import time  # noqa: E402

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.optim as optim  # noqa: E402

from . import dp  # noqa: E402
from .augment import DeviceAugmenter, collate_fn  # noqa: E402
from .distill import DistillLoss  # noqa: E402
from .data import (VOCList, SyntheticDetection, VOCAugment, SyntheticAugment, ResidentImages, ResidentAugment,  # noqa: E402
                   ResidentList, label_path_for, read_boxes)
from .nets import Darknet, cfg_shapes, parse_cfg  # noqa: E402
from .pruning.weightPruning.methods import block_prune, quick_filter_prune, weight_prune  # noqa: E402
from .pruning.weightPruning.utils import prune_rate, are_masks_consistent  # noqa: E402
from .share import kmeans_share, are_codebooks_consistent, _bits_of  # noqa: E402
from .importance import TaylorImportance, taylor_prune  # noqa: E402
from .sparsify import GroupLasso, check_config as _group_lasso_config  # noqa: E402

TAYLOR_METHODS = {"taylor-weight": "weight", "taylor-block": "block", "taylor-filter": "filter"}


def logging(message):
    print('%s %s' % (time.strftime("%Y-%m-%d %H:%M:%S", time.localtime()), message))


def file_lines(thefilepath):
    with open(thefilepath, 'rb') as f:
        return sum(buf.count(b'\n') for buf in iter(lambda: f.read(1 << 20), b''))


def _logit_grid(model):
    """(width, height) of the grid a Darknet maps its cfg's input size to, from the cfg alone (no forward)."""
    return cfg_shapes(model.blocks)[-1][3:5]


class StepGuard:
    """The overflow / non-finite policy of a training step WITHOUT a host synchronisation in the step.

    The engine keeps gradients as fp16 x grad_scale and saturates at +-65504 (a device flag per engine records it;
    RegionLoss's exp terms can push |dL/dlogit| x 256 beyond that), and a non-finite loss must not reach the weights.
    Round 2 read both on the host every step (`isfinite(loss)`, `grad_overflowed().item()`, an `isfinite` scan of the
    202 MB gradient buffer and two collectives).  Here:
      * `decide(loss)` (after backward) folds the engines' flags and `~isfinite(loss)` into ONE device scalar, takes the
        maximum over the ranks (one 4-byte all-reduce on the stream, so every rank takes the same branch) and hands it
        to the fused SGD kernel as `found_inf`: a flagged step's update is skipped ON THE DEVICE;
      * the host reads that scalar one step LATE (pinned copy + event recorded here, consumed by the next call, when
        the following step is already enqueued): engine overflow -> grad_scale halved for the steps after it, overflow
        of the fp16 all-reduce transport (dp.GradReducer.overflow) -> its fp16_scale halved, non-finite loss ->
        FloatingPointError (the reference enters pdb on a NaN loss, train.py:226-231).
    (The gradient buffer needs no scan of its own: every fp16-writing backward kernel clamps and flags, the fp32
    finish passes only scale finite values, so a finite loss gives finite gradients.)"""

    def __init__(self, model, optimizer, dev, log=None):
        self.model, self.opt, self.dev, self.log = model, optimizer, dev, log
        self.flags = torch.zeros(3, dtype=torch.float32, device=dev)   # [engine overflow, non-finite loss, transport overflow]
        self.found = torch.zeros(1, dtype=torch.float32, device=dev)
        optimizer.found_inf = self.found          # torch's fused SGD skips the whole update when this is EXACTLY 1.0
        # momentum buffers exist (zero) from the start: a skipped FIRST step would otherwise leave them uninitialised
        # (torch creates them with empty_like on the first call); zero buffers give the same first update, buf = grad
        for group in optimizer.param_groups:
            if group.get("momentum", 0):
                for p in group["params"]:
                    optimizer.state[p].setdefault("momentum_buffer", torch.zeros_like(p))
        self._host = torch.zeros(3, dtype=torch.float32)
        if dev.type == "cuda":
            self._host = self._host.pin_memory()
        self._event, self._pending = None, False
        self.skipped = 0
        # scales the pending step RAN with: its flag is read one step late, when the next step -- enqueued with the same
        # scales -- has usually overflowed too; a flag only halves a scale that is still the one its step used, so one
        # overflow event costs one halving, not two.  `clean` counts steps since the last skip: after
        # GROWTH_INTERVAL of them a halved scale doubles again (up to where it started), as torch.amp.GradScaler does --
        # otherwise a long run only ever loses gradient bits.
        self._pending_scales = (None, None)
        self._scale0 = float(getattr(model, "grad_scale", 1.0))
        self._tscale0 = None
        self.clean = 0
        self._collective = dist.is_initialized() and (dist.get_world_size() > 1 or dp.rehearsal())

    def consume(self):
        """Act on the flag of the step BEFORE the one just enqueued (no-op when there is none)."""
        if not self._pending:
            return 0
        if self._event is not None:
            self._event.synchronize()             # that step is long done unless the host runs a whole step ahead
        over, bad, tover = (bool(v) for v in self._host.tolist())
        self._pending = False
        if bad:
            raise FloatingPointError("non-finite training loss")
        ran_gs, ran_ts = self._pending_scales
        red = getattr(self.model, "_grad_reducer", None)
        if over or tover:
            self.skipped += 1
            self.clean = 0
        else:
            self.clean += 1
        if over and (ran_gs is None or ran_gs == self.model.grad_scale):
            self.model.grad_scale = max(1.0, self.model.grad_scale / 2.0)
            if self.log:
                self.log('gradient overflow in fp16 storage: step skipped, grad_scale -> %g' % self.model.grad_scale)
        if tover and (ran_ts is None or ran_ts == red.fp16_scale):
            red.fp16_scale = max(1.0 / 65536.0, red.fp16_scale / 2.0)
            if self.log:
                self.log('gradient overflow in the fp16 all-reduce transport: step skipped, fp16_scale -> %g' % red.fp16_scale)
        if self.clean >= self.GROWTH_INTERVAL:
            self.clean = 0
            if self.model.grad_scale < self._scale0:
                self.model.grad_scale = min(self._scale0, self.model.grad_scale * 2.0)
                if self.log:
                    self.log('%d clean steps: grad_scale -> %g' % (self.GROWTH_INTERVAL, self.model.grad_scale))
            if red is not None and self._tscale0 is not None and red.fp16_scale < self._tscale0:
                red.fp16_scale = min(self._tscale0, red.fp16_scale * 2.0)
        return int(over) + 2 * int(bad) + 4 * int(tover)

    GROWTH_INTERVAL = 2000

    def decide(self, loss):
        """Call between backward() and optimizer.step()."""
        red = getattr(self.model, "_grad_reducer", None)
        # the scales the step that just ran its backward USED (consume() below may change them for the next one)
        ran = (float(getattr(self.model, "grad_scale", 1.0)), red.fp16_scale if red is not None else None)
        if red is not None and self._tscale0 is None:
            self._tscale0 = red.fp16_scale
        self.consume()
        self._pending_scales = ran
        flags = [eng.overflow for eng in getattr(self.model, "_engines", {}).values()]
        tflag = red.overflow if red is not None else None
        if (self.dev.type == "cuda" and len(flags) <= 8 and loss.dtype == torch.float32 and loss.numel() == 1
                and all(f.is_cuda and f.dtype == torch.int32 for f in flags + ([tflag] if tflag is not None else []))):
            # one launch (mcamd_step_flags) instead of the dozen torch micro-kernels below: 9.42 -> 9.3x ms per real step
            from . import ops
            ops.step_flags(flags, loss.detach().reshape(1), tflag, self.flags, None if self._collective else self.found)
            if self._collective:
                dist.all_reduce(self.flags, op=dist.ReduceOp.MAX)
                ops.step_flags([], None, None, self.flags, self.found)
            self._host.copy_(self.flags, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record()
            self._pending = True
            return
        zero = torch.zeros((), dtype=torch.float32, device=self.dev)
        over = torch.stack([f.reshape(()) for f in flags]).sum().clamp(max=1).to(torch.float32) if flags else zero
        bad = (~torch.isfinite(loss.detach())).to(torch.float32).reshape(())
        tover = tflag.reshape(()).clamp(max=1).to(torch.float32) if tflag is not None else zero
        self.flags.copy_(torch.stack((over, bad, tover)))
        for f in flags + ([tflag] if tflag is not None else []):
            f.zero_()
        if self._collective:
            dist.all_reduce(self.flags, op=dist.ReduceOp.MAX)
        self.found.copy_(self.flags.amax().clamp(max=1).reshape(1))      # exactly 1.0: the fused SGD tests `== 1`
        self._host.copy_(self.flags, non_blocking=True)
        if self.dev.type == "cuda":
            self._event = torch.cuda.Event()
            self._event.record()
        self._pending = True

    def finish(self):
        """End of an epoch / run: the last step's flag."""
        return self.consume()


def _share_keyword(train):
    """train(..., SHARE=...): the keyword is taken off here and handed to the call as an attribute.  The parameter list of
    train() itself stays the reference's plus the earlier keywords, positions included (callers pass it positionally up to
    RESIDENT, and its end is pinned by tests/test_distill_cpu.py), so SHARE can only be given by keyword."""
    @functools.wraps(train)
    def with_share(self, *args, SHARE=None, **kwargs):
        self._share_arg = SHARE
        try:
            return train(self, *args, **kwargs)
        finally:
            self._share_arg = None
    return with_share


class YOLOv2Train():
    # "fp32" / "fp16" / "fp8": train() writes a compressed model file of that payload (compress.py) beside every .weights file
    # it saves.  An attribute, like PASCALVOCEval.fused, not a keyword: train() keeps its signature.
    SAVE_COMPRESSED = None
    # None / "huffman": the entropy keyword of that save_compressed call ("huffman": a coded "MCZH" file)
    SAVE_COMPRESSED_ENTROPY = None
    # bits, or a dict of share.kmeans_share keywords: the default of train()'s SHARE keyword (module docstring)
    SHARE = None
    _share_arg = None
    # batches scored before pruning by pruning_method = "taylor-*" (an attribute: train() keeps its signature)
    TAYLOR_STEPS = 16
    # None / "block": Darknet.sparse_train of the model train() builds, set behind set_masks (an attribute too).  "block" skips
    # the zero blocks of pruning_method "block" / "taylor-block" masks in the forward and dgrad launches of the fp16 training
    # step; it needs the training precision "fp16" (MCAMD_PRECISION) and, for blocks to be chosen, a bound
    # Darknet.sparse_train_max_kept above the layers' kept fractions.  "block-wgrad"  also skips them in the
    # weight gradient of the layers below Darknet.sparse_train_wgrad_max_kept.
    SPARSE_TRAIN = None
    # None, or {"lam": float, "granularity": "block" | "filter"}: a proximal group-lasso step (sparsify.GroupLasso, DESIGN.md
    # 3ze) behind every optimizer.step(); the learned zero groups become masks before every file is saved (an attribute too)
    GROUP_LASSO = None

    def __init__(self):
        self.model = ''
        self.optimizer = ''
        self.trainlist = ''
        self.testlist = ''
        self.init_width = ''
        self.init_height = ''
        self.batch_size = ''
        self.teacher = None       # train(TEACHER=...): the frozen Darknet and the distill.DistillLoss of the last call
        self.distill = None
        self.group_lasso = None   # GROUP_LASSO: the sparsify.GroupLasso of the last call

    @_share_keyword
    def train(self, PASCAL_DIR, PASCAL_TRAIN, PASCAL_VALID, TRAIN_LOGDIR, VAL_LOGDIR, VAL_OUTPUTDIR_PKL, VAL_PREFIX,
              MODEL_CFG, MODEL_WEIGHT,
              BATCH_SIZE, SAVE_INTERNAL,
              LOGGER='', DEBUG_EPOCHS=-1, verbose=0, pruning_perc=0., pruning_method="weight",
              MAX_EPOCHS=135, SYNTHETIC_SAMPLES=256, EVAL=False, AUGMENT=False, RESIDENT=False, TEACHER=None,
              DISTILL=None):
        SHARE = self.SHARE if self._share_arg is None else self._share_arg
        SAVE_COMPRESSED = self.SAVE_COMPRESSED
        if SAVE_COMPRESSED not in (None, "fp32", "fp16", "w4", "fp8", "shared"):
            raise ValueError('train: SAVE_COMPRESSED must be None, "fp32", "fp16", "w4", "fp8" or "shared", got %r' % (SAVE_COMPRESSED,))
        if self.SAVE_COMPRESSED_ENTROPY not in (None, "huffman"):
            raise ValueError('train: SAVE_COMPRESSED_ENTROPY must be None or "huffman", got %r' % (self.SAVE_COMPRESSED_ENTROPY,))
        if SHARE is not None and not isinstance(SHARE, dict):
            SHARE = dict(bits=SHARE)
        if SHARE is not None and not isinstance(SHARE.get("bits", 4), dict):
            _bits_of(SHARE.get("bits", 4), [1])       # a bad width is refused here, before the model is built
        GROUP_LASSO = self.GROUP_LASSO
        if GROUP_LASSO is not None:
            if not isinstance(GROUP_LASSO, dict) or set(GROUP_LASSO) != {"lam", "granularity"}:
                raise ValueError('train: GROUP_LASSO must be None or a dict {"lam": float, "granularity": "block" | "filter"}, '
                                 'got %r' % (GROUP_LASSO,))
            _group_lasso_config(GROUP_LASSO["lam"], GROUP_LASSO["granularity"], who="train: GROUP_LASSO")
            if SHARE is not None:
                raise ValueError("train: SHARE and GROUP_LASSO cannot be combined: the projection onto the codebooks and the "
                                 "proximal step would undo each other")
        if DISTILL is not None and TEACHER is None:
            raise ValueError("train: DISTILL needs a TEACHER (True, a .weights path or a Darknet)")
        rank, world = dp.init_from_env()
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)

        # Step 1 - model
        net_options = parse_cfg(MODEL_CFG)[0]
        self.model = Darknet(MODEL_CFG)
        if MODEL_WEIGHT and os.path.exists(MODEL_WEIGHT):
            self.model.load_weights(MODEL_WEIGHT)
        else:
            from .synthetic import init_synthetic
            init_synthetic(self.model, seed=0)
            logging('weights file %r not found: seeded synthetic initialisation' % (MODEL_WEIGHT,))
        self.model = self.model.to(dev)
        dp.broadcast_parameters(self.model, src=0)
        self.teacher, self.distill = self._make_teacher(TEACHER, DISTILL, MODEL_CFG, dev)

        # Step 2 - dataset
        self.trainlist, self.testlist = PASCAL_TRAIN, PASCAL_VALID
        self.init_width, self.init_height = self.model.width, self.model.height
        shape = (self.init_width, self.init_height)
        resident = None
        if PASCAL_TRAIN and os.path.exists(PASCAL_TRAIN):
            nsamples = file_lines(self.trainlist)
            dataset = VOCAugment(self.trainlist, shape=shape) if AUGMENT else VOCList(self.trainlist, shape=shape, train=True)
            if RESIDENT:
                t0 = time.time()
                resident = ResidentImages(dataset.lines, dev)
                labels = [label_path_for(p) for p in dataset.lines]
                dataset = (ResidentAugment(resident, [read_boxes(lp) for lp in labels], shape) if AUGMENT
                           else ResidentList(resident, labels, shape))
        else:
            nsamples = SYNTHETIC_SAMPLES
            dataset = SyntheticAugment(nsamples, shape=shape) if AUGMENT else SyntheticDetection(nsamples, shape=shape)
            logging('train list %r not found: synthetic detection set of %d samples' % (PASCAL_TRAIN, nsamples))
            if RESIDENT:
                # the uint8 sources of SyntheticAugment either way (SyntheticDetection's float pictures have no uint8 form)
                t0 = time.time()
                items = [SyntheticAugment(nsamples, shape=shape)[i] for i in range(nsamples)]
                resident = ResidentImages.from_sources([src for src, _, _ in items], dev)
                if AUGMENT:
                    dataset = ResidentAugment(resident, [boxes for _, boxes, _ in items], shape)
                else:
                    targets = torch.zeros(nsamples, 250)
                    for i, (_, boxes, _) in enumerate(items):
                        targets[i, :boxes.size] = torch.from_numpy(boxes.astype('float32').reshape(-1))
                    dataset = ResidentList(resident, targets, shape)
        if resident is not None and rank == 0:
            logging('%d pictures resident on %s: %d bytes, built in %.2f s' % (len(resident), dev, resident.nbytes,
                                                                               time.time() - t0))
        if TRAIN_LOGDIR and rank == 0 and not os.path.exists(TRAIN_LOGDIR):
            os.makedirs(TRAIN_LOGDIR, exist_ok=True)

        # Step 3 - training parameters (train.py:113-147)
        self.batch_size = BATCH_SIZE
        momentum = float(net_options['momentum'])
        decay = float(net_options['decay'])
        region_loss = self.model.loss
        region_loss.seen = self.model.seen
        init_epoch = int(self.model.seen / nsamples)
        LR = 0.00001
        optimizer = optim.SGD(self.model.parameters(), lr=LR, momentum=momentum, dampening=0,
                              weight_decay=decay * self.batch_size, fused=True)   # same rule (train.py:144-147), one kernel
        self.optimizer = optimizer
        reducer = None

        masks = None
        if pruning_perc > 0:
            if pruning_method in TAYLOR_METHODS:
                masks = self._taylor_masks(TAYLOR_METHODS[pruning_method], pruning_perc, dataset, resident, shape, AUGMENT,
                                           init_epoch, rank, world, dev, region_loss, optimizer)
            elif pruning_method == "filter":
                masks = quick_filter_prune(self.model, pruning_perc)
            elif pruning_method == "block":
                masks = block_prune(self.model, pruning_perc)
            else:
                masks = weight_prune(self.model, pruning_perc)
            dp.broadcast_masks(masks, src=0)
            self.model.set_masks(masks)
        if self.SPARSE_TRAIN is not None:      # (the engine checks the value and the training precision: "fp16" only)
            self.model.sparse_train = self.SPARSE_TRAIN
        if world > 1:
            # static weight masks: only the kept gradient entries travel (dp.py); filter masks keep the dense transport
            reducer = dp.attach(self.model, masks=masks if (masks is not None and pruning_method not in ("filter", "taylor-filter")) else None)
        if SHARE is not None:
            # every rank clusters the same broadcast weights under the same masks: the codebooks agree, nothing travels
            self.model.set_codebooks(kmeans_share(self.model, **SHARE))
        self.group_lasso = gl = None
        if GROUP_LASSO is not None:
            gl = self.group_lasso = GroupLasso(self.model, GROUP_LASSO["lam"], GROUP_LASSO["granularity"])
        if masks is not None:
            p_rate = prune_rate(self.model, rank == 0)
            if rank == 0:
                print(' %s=pruned: %s' % (pruning_method, p_rate))

        per_rank = max(1, self.batch_size // world)
        sampler = torch.utils.data.distributed.DistributedSampler(dataset, world, rank, shuffle=True) if world > 1 else None
        augmenter = DeviceAugmenter(shape, dev, resident) if AUGMENT or resident is not None else None
        loader = torch.utils.data.DataLoader(dataset, batch_size=per_rank, shuffle=(sampler is None), sampler=sampler,
                                             num_workers=4 if isinstance(dataset, (VOCList, VOCAugment, SyntheticAugment)) else 0,
                                             pin_memory=True, drop_last=True,
                                             collate_fn=dataset.collate if resident is not None
                                             else collate_fn(shape) if AUGMENT else None)
        eval_resident = None
        if RESIDENT and EVAL and rank == 0 and PASCAL_VALID and os.path.exists(PASCAL_VALID):
            eval_resident = ResidentImages(VOCList(PASCAL_VALID, shape=shape, train=False).lines, dev)
        guard = StepGuard(self.model, optimizer, dev, log=logging if rank == 0 else None)
        epoch = init_epoch
        for epoch in range(init_epoch, min(MAX_EPOCHS, 135)):
            if sampler is not None:
                sampler.set_epoch(epoch)
            if AUGMENT:
                dataset.set_epoch(epoch)       # before the loader's workers take their copy of the dataset
            if rank == 0:
                print(' ---------------------------- EPOCH : ', epoch, ' (LR : ', LR, ') ---------------------------------- ')
            self.model.train()
            # the loss is accumulated on the device and read once per epoch; the skip policy lives in StepGuard
            train_loss_total, t0, steps_here = torch.zeros((), dtype=torch.float32, device=dev), time.time(), 0
            skipped_before = guard.skipped
            distill_loss_total = torch.zeros((), dtype=torch.float32, device=dev) if self.teacher is not None else None
            for batch_idx, batch in enumerate(loader):
                if DEBUG_EPOCHS > -1 and batch_idx > DEBUG_EPOCHS:
                    break
                data, target = augmenter(batch) if augmenter is not None else batch
                data = data.to(dev, non_blocking=True)
                target = target.float().to(dev, non_blocking=True)
                if self.teacher is not None:
                    with torch.no_grad():
                        t_out = self.teacher(data)
                output = self.model(data)
                region_loss.seen = region_loss.seen + data.size(0) * world
                train_loss = region_loss(output, target)
                if self.teacher is not None:
                    distill_loss = self.distill(output, t_out)
                    train_loss = train_loss + distill_loss
                    distill_loss_total += distill_loss.detach()
                train_loss_total += train_loss.detach()
                optimizer.zero_grad()
                train_loss.backward()
                # no host synchronisation here: a saturated / non-finite step is skipped on the device, by all ranks
                # together, and the host learns of it one step late (StepGuard)
                guard.decide(train_loss)
                optimizer.step()
                if gl is not None:
                    # the proximal step of the penalty, at the step size SGD just used; a step StepGuard skipped leaves the
                    # weights exactly as they were, decided on the device
                    gl.step(optimizer.param_groups[0]["lr"], skip=guard.found)
                if SHARE is not None:
                    # By linearity, SGD on the shared values with the mean member gradient (momentum and weight decay
                    # included).  A step StepGuard skipped left the weights tied: the projection is then the identity.
                    self.model.project_codebooks()
                steps_here += 1
                if verbose and rank == 0:
                    print(' - loss : ', float(train_loss.detach()))
            guard.finish()
            torch.cuda.synchronize()
            seen_here = (steps_here - (guard.skipped - skipped_before)) * per_rank * world
            train_loss_total = float(train_loss_total)
            if rank == 0:
                logging('training with %f samples/s, mean loss %.4f%s' % (
                    seen_here / max(time.time() - t0, 1e-9), train_loss_total / max(len(loader), 1),
                    '' if distill_loss_total is None else
                    ', of it distillation %.4f' % (float(distill_loss_total) / max(len(loader), 1))))
            if gl is not None and rank == 0:
                logging('group lasso (%s, lam %g): %.4f of the groups are zero' % (gl.granularity, gl.lam, gl.zero_fraction()))
            dp.sync_buffers(self.model)     # BatchNorm running statistics are rank-local: average before checkpoint / eval
            if gl is not None and pruning_perc > 0 and (epoch + 1) % 5 == 0 and TRAIN_LOGDIR:
                # a checkpoint follows: the zero groups become ordinary masks first, on every rank alike
                masks = gl.masks()
                self.model.set_masks(masks)
            if pruning_perc > 0 and rank == 0:
                print(' pruned: %s' % prune_rate(self.model, False))
                print(' pruned weights consistent after retraining: %s ' % are_masks_consistent(self.model, masks))
                if SHARE is not None:
                    print(' shared weights consistent after retraining: %s ' % are_codebooks_consistent(self.model))
                if (epoch + 1) % 5 == 0 and TRAIN_LOGDIR:
                    name = '%s/%s-pruned-%s-retrained_%06d.weights' % (TRAIN_LOGDIR, pruning_method, pruning_perc, epoch + 1)
                    logging('save weights to %s' % name)
                    self.model.save_weights(name)
                    self._save_compressed(name, SAVE_COMPRESSED)
            if LOGGER != '' and rank == 0:
                LOGGER.save_value('Total Loss', 'Train Loss', epoch + 1, train_loss_total / max(len(loader), 1))
            self.model.seen = (epoch + 1) * nsamples
            if EVAL and rank == 0:
                from .predict import PASCALVOCEval
                PASCALVOCEval(self.model, MODEL_CFG, MODEL_WEIGHT, region_loss, PASCAL_DIR, PASCAL_VALID, VAL_LOGDIR,
                              VAL_PREFIX, VAL_OUTPUTDIR_PKL, LOGGER, epoch).predict(BATCH_SIZE, RESIDENT=eval_resident)
        if gl is not None:
            # the learned structure as ordinary masks: what the .weights / .mcz files and the later engines see
            masks = gl.masks()
            self.model.set_masks(masks)
        if TRAIN_LOGDIR and rank == 0:
            name = '%s/%s-pruned-%s-retrained-final_%06d.weights' % (TRAIN_LOGDIR, pruning_method, pruning_perc, epoch + 1)
            logging('save weights to %s' % name)
            self.model.save_weights(name)
            self._save_compressed(name, SAVE_COMPRESSED)
        return self.model

    def _taylor_masks(self, granularity, pruning_perc, dataset, resident, shape, AUGMENT, epoch, rank, world, dev, region_loss,
                      optimizer):
        """pruning_method = "taylor-*": score TAYLOR_STEPS batches (no optimizer step), then taylor_prune.  The loader is
        built the way the training loop builds its own; the model's buffers (BatchNorm running statistics) are restored."""
        nsteps = int(self.TAYLOR_STEPS)
        if nsteps < 1:
            raise ValueError("train: TAYLOR_STEPS must be at least 1, got %r" % (self.TAYLOR_STEPS,))
        per_rank = max(1, self.batch_size // world)
        sampler = torch.utils.data.distributed.DistributedSampler(dataset, world, rank, shuffle=True) if world > 1 else None
        if sampler is not None:
            sampler.set_epoch(epoch)
        if AUGMENT:
            dataset.set_epoch(epoch)
        augmenter = DeviceAugmenter(shape, dev, resident) if AUGMENT or resident is not None else None
        loader = torch.utils.data.DataLoader(dataset, batch_size=per_rank, shuffle=(sampler is None), sampler=sampler,
                                             num_workers=4 if isinstance(dataset, (VOCList, VOCAugment, SyntheticAugment)) else 0,
                                             pin_memory=True, drop_last=True,
                                             collate_fn=dataset.collate if resident is not None
                                             else collate_fn(shape) if AUGMENT else None)
        if len(loader) == 0:
            raise ValueError("train: the training set holds no full batch to score")
        imp = TaylorImportance(self.model, weight=granularity == "weight", block=granularity == "block",
                               filter=granularity == "filter")
        saved = [(b, b.detach().clone()) for b in self.model.buffers()]
        guard = StepGuard(self.model, optimizer, dev, log=logging if rank == 0 else None)
        self.model.train()
        done, t0 = 0, time.time()
        while done < nsteps:
            for batch in loader:
                data, target = augmenter(batch) if augmenter is not None else batch
                data = data.to(dev, non_blocking=True)
                target = target.float().to(dev, non_blocking=True)
                if self.teacher is not None:
                    with torch.no_grad():
                        t_out = self.teacher(data)
                output = self.model(data)
                loss = region_loss(output, target)
                if self.teacher is not None:
                    loss = loss + self.distill(output, t_out)
                optimizer.zero_grad()
                loss.backward()
                guard.decide(loss)
                imp.accumulate(skip=guard.found)          # a flagged step adds nothing, on the device
                done += 1
                if done == nsteps:
                    break
        guard.finish()
        optimizer.zero_grad()
        with torch.no_grad():
            for b, v in saved:
                b.copy_(v)
        imp.all_reduce()
        scored = imp.steps()
        masks = taylor_prune(self.model, pruning_perc, imp, granularity)
        if rank == 0:
            logging('taylor-%s: %d of %d scoring steps accumulated (over all ranks) in %.2f s' % (
                granularity, scored, nsteps * world, time.time() - t0))
        return masks

    def _save_compressed(self, weights_name, payload):
        """YOLOv2Train.SAVE_COMPRESSED = payload: the compressed model file (compress.py) beside a .weights file just saved."""
        if payload is None:
            return
        name = os.path.splitext(weights_name)[0] + '.mcz'
        logging('save compressed weights (%s) to %s' % (payload, name))
        self.model.save_compressed(name, payload, entropy=self.SAVE_COMPRESSED_ENTROPY)

    def _make_teacher(self, TEACHER, DISTILL, MODEL_CFG, dev):
        """(teacher, loss) of the TEACHER / DISTILL keywords, (None, None) without a teacher.  Called after the model is
        loaded and broadcast and BEFORE pruning: TEACHER=True freezes the weights the student starts from."""
        if TEACHER is None:
            return None, None
        if isinstance(TEACHER, Darknet):
            teacher = TEACHER.to(dev)
        else:
            # a fresh Darknet, not copy.deepcopy: a Darknet carries engines with device pointers
            teacher = Darknet(MODEL_CFG)
            if TEACHER is True:
                teacher.load_state_dict(self.model.state_dict())
            elif isinstance(TEACHER, (str, os.PathLike)) and os.path.exists(TEACHER):
                teacher.load_weights(os.fspath(TEACHER))
            else:
                raise ValueError("train: TEACHER must be True, an existing .weights file or a Darknet, got %r" % (TEACHER,))
            teacher = teacher.to(dev)
        teacher.eval()
        teacher.requires_grad_(False)
        distill = DistillLoss.from_model(self.model) if DISTILL is None else DISTILL
        if not isinstance(distill, DistillLoss):
            raise ValueError("train: DISTILL must be a distill.DistillLoss, got %r" % (DISTILL,))
        head = (self.model.num_anchors, self.model.num_classes)
        if (teacher.num_anchors, teacher.num_classes) != head or (distill.num_anchors, distill.num_classes) != head:
            raise ValueError("train: the student's region layer has %d anchors x %d classes, the teacher's %d x %d, the "
                             "distillation loss %d x %d" % (head + (teacher.num_anchors, teacher.num_classes,
                                                                    distill.num_anchors, distill.num_classes)))
        shapes = [_logit_grid(m) for m in (self.model, teacher)]
        if shapes[0] != shapes[1] or (self.model.width, self.model.height) != (teacher.width, teacher.height):
            raise ValueError("train: the student maps %dx%d pictures to a %dx%d grid, the teacher %dx%d to %dx%d"
                             % (self.model.width, self.model.height, shapes[0][0], shapes[0][1],
                                teacher.width, teacher.height, shapes[1][0], shapes[1][1]))
        return teacher, distill.to(dev)

    def adjust_learning_rate(self, optimizer, batch, learning_rate, steps, scales, batch_size):
        """train.py:277-290 (never called by the reference's loop either)."""
        lr = learning_rate
        for i in range(len(steps)):
            scale = scales[i] if i < len(scales) else 1
            if batch >= steps[i]:
                lr = lr * scale
                if batch == steps[i]:
                    break
            else:
                break
        for param_group in optimizer.param_groups:
            param_group['lr'] = lr / batch_size
        return lr
