"""Taylor-importance pruning through the model API on the device (importance.py; tests/golden/mini.cfg, B = 4
at 64x64): the accumulators of real training steps against the numpy restatement applied to clones of (w, grad), the three
mask rules against the restatement's, the masks on the engines that consume them, a warm accumulate() without allocation or
host synchronisation, and train(pruning_method="taylor-*")."""
import contextlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bsparse_ref as B  # noqa: E402
import taylor_ref as R  # noqa: E402
from modelcompression_amd import nets  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.importance import TaylorImportance, taylor_prune, GRANULARITIES  # noqa: E402
from modelcompression_amd.pruning.weightPruning.utils import are_masks_consistent  # noqa: E402
from modelcompression_amd.synthetic import init_synthetic  # noqa: E402
from modelcompression_amd.train import YOLOv2Train  # noqa: E402
from util import rel_l2  # noqa: E402

MINI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini.cfg")


@contextlib.contextmanager
def no_sync():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def batch(dev, seed):
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(seed)).to(dev)
    target = torch.zeros(4, 250, device=dev)
    target[:, :5] = torch.tensor([3.0, 0.5, 0.5, 0.3, 0.4], device=dev)
    target[1, 5:10] = torch.tensor([7.0, 0.25, 0.7, 0.2, 0.2], device=dev)
    return x, target


def backward(model, x, target):
    model.zero_grad()
    model.loss(model(x), target).backward()


def blocks_of(model):
    """[(conv, bn or None)] in parameter order."""
    out = []
    for seq in model.models:
        if isinstance(seq, torch.nn.Sequential) and getattr(seq[0], "name", "") == "MaskedConv2d":
            out.append((seq[0], seq[1] if len(seq) > 1 and isinstance(seq[1], torch.nn.BatchNorm2d) else None))
    return out


def same_bits(got, want):
    want = torch.from_numpy(want)
    bits = torch.int32 if want.dtype == torch.float32 else torch.int64
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu().view(bits), want.view(bits))


@pytest.fixture(scope="module")
def scored(dev):
    """(model, importance, restatement accumulators) after three real forward/backward steps, computed once."""
    model = init_synthetic(nets.Darknet(MINI), seed=0).to(dev)
    model.train()
    imp = TaylorImportance(model)
    layers = blocks_of(model)
    assert len(layers) == len(imp.params) == 7 and all(c.weight is p for (c, _), p in zip(layers, imp.params))
    ref = []
    for conv, _ in layers:
        cout, cin, kh, kw = conv.weight.shape
        dims = B.block_dims(cout, cin, kh * kw)
        ref.append(dict(acc_w=np.zeros((cout, cin, kh, kw), np.float32),
                        acc_b=None if dims is None else np.zeros(dims[0] * dims[1] * kh * kw), acc_f=np.zeros(cout)))
    n = lambda t: t.detach().cpu().numpy().copy()
    for step in range(3):
        backward(model, *batch(dev, 40 + step))
        imp.accumulate()
        for (conv, bn), a in zip(layers, ref):
            w, g = n(conv.weight), n(conv.weight.grad)
            if bn is None:
                R.conv_step(w, g, n(conv.bias), n(conv.bias.grad), a["acc_w"], a["acc_b"], a["acc_f"])
            else:
                R.conv_step(w, g, acc_w=a["acc_w"], acc_b=a["acc_b"])
                R.gate_step(n(bn.weight), n(bn.weight.grad), n(bn.bias), n(bn.bias.grad), a["acc_f"])
    return model, imp, ref


def test_accumulators_equal_the_restatement_on_real_gradients(scored):
    model, imp, ref = scored
    assert imp.steps() == 3 and imp.tables_built == 1
    assert [a is None for a in imp.block_scores()] == [r["acc_b"] is None for r in ref] == [True] + [False] * 6
    for name, got in (("acc_w", imp.weight_scores()), ("acc_b", imp.block_scores()), ("acc_f", imp.filter_scores())):
        for i, (t, r) in enumerate(zip(got, ref)):
            if r[name] is not None:
                assert same_bits(t, r[name]), "conv%d %s" % (i + 1, name)
                assert float(t.sum()) > 0
    zeros = sum(int((t == 0).sum()) for t in imp.weight_scores()) / sum(t.numel() for t in imp.weight_scores())
    print("weight scores exactly 0 after 3 steps: %.4f %%" % (100 * zeros))


@pytest.mark.parametrize("per_layer", [False, True])
@pytest.mark.parametrize("granularity", GRANULARITIES)
def test_masks_equal_the_restatements(scored, granularity, per_layer):
    model, imp, ref = scored
    shapes = [tuple(p.shape) for p in imp.params]
    masks = taylor_prune(model, 50, imp, granularity, per_layer=per_layer)
    if granularity == "weight":
        want = R.weight_masks([r["acc_w"] for r in ref], 50, per_layer)
    elif granularity == "block":
        want = R.block_masks(shapes, [r["acc_b"] for r in ref], 3, 50, per_layer=per_layer)
    else:
        want = R.filter_masks(shapes, [r["acc_f"] for r in ref], 3, 50, per_layer)
    assert len(masks) == len(want) == 7
    for i, (m, r) in enumerate(zip(masks, want)):
        assert m.is_cuda and m.dtype == torch.float32 and torch.equal(m.cpu(), torch.from_numpy(r)), "conv%d" % (i + 1)
    pruned = sum(float((m == 0).sum()) for m in masks) / sum(m.numel() for m in masks)
    assert 0.05 < pruned < 0.95


def fresh_with_masks(dev, granularity, perc=50):
    model = init_synthetic(nets.Darknet(MINI), seed=0).to(dev)
    model.train()
    imp = TaylorImportance(model, weight=granularity == "weight", block=granularity == "block", filter=granularity == "filter")
    for step in range(2):
        backward(model, *batch(dev, 50 + step))
        imp.accumulate()
    masks = taylor_prune(model, perc, imp, granularity)
    model.set_masks(masks)
    return model, masks


def test_filter_masks_survive_a_training_step(dev):
    model, masks = fresh_with_masks(dev, "filter")
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4, fused=True)
    x, target = batch(dev, 60)
    loss = model.loss(model(x), target)
    opt.zero_grad()
    loss.backward()
    opt.step()
    assert torch.isfinite(loss) and are_masks_consistent(model, masks)
    for m in masks:
        flat = m.reshape(m.shape[0], -1)
        assert bool((flat.min(1).values == flat.max(1).values).all()) and float(flat.max()) == 1
    assert any(float(m.min()) == 0 for m in masks)


def test_block_masks_run_on_the_block_sparse_forward(dev):
    model, masks = fresh_with_masks(dev, "block", perc=60)
    model.eval()
    model.precision = "fp16"
    model.sparse_max_kept = 1.0
    x, _ = batch(dev, 61)
    with torch.no_grad():
        model.sparse = None
        dense = model(x).clone()
        model.sparse = "block"
        sparse = model(x).clone()
    eng = [e for k, e in model._engines.items() if k[0] == tuple(x.shape) and not e.train_layout][0]
    assert eng.bsparse_layers, "no layer took the block-sparse kernel"
    e = rel_l2(sparse, dense)
    print("block-sparse vs dense fp16 engine on taylor-block masks: rel-L2 %.2e, layers %s" % (e, eng.bsparse_layers))
    assert e < 1e-3                              # the bound tests/test_bsparse_model_gpu.py holds the same pair to


def test_a_warm_accumulate_allocates_nothing_and_does_not_synchronise(dev):
    model = init_synthetic(nets.Darknet(MINI), seed=0).to(dev)
    model.train()
    imp = TaylorImportance(model)
    x, target = batch(dev, 70)
    found = torch.zeros(1, device=dev)
    backward(model, x, target)
    imp.accumulate(skip=found)                   # builds the table
    backward(model, x, target)                   # the gradients are views of one persistent buffer: the pointers stay
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(dev)
    with no_sync():
        imp.accumulate(skip=found)
        imp.accumulate()
    torch.cuda.synchronize()
    after = torch.cuda.memory_stats(dev)
    assert imp.tables_built == 1 and imp.steps() == 3
    for key in ("num_alloc_retries", "segment.all.allocated", "allocation.all.allocated"):
        assert after[key] == before[key], key
    # a gradient that moved: the table is rebuilt, the step still counts
    for p in model.parameters():
        p.grad = p.grad.clone()
    imp.accumulate()
    assert imp.tables_built == 2 and imp.steps() == 4
    model.zero_grad()
    with pytest.raises(McamdError, match="after backward"):
        imp.accumulate()


def structure_ok(method, conv):
    m = conv.mask
    O_, I = m.shape[:2]
    if method == "taylor-filter":
        flat = m.reshape(O_, -1)
        return bool((flat.min(1).values == flat.max(1).values).all())
    if method == "taylor-block":
        if I % 32 != 0:
            return bool((m == 1).all())
        kb = 64 if I % 64 == 0 else 32
        for f in range(0, O_, 64):
            mk = m[f:f + 64].reshape(min(64, O_ - f), I // kb, kb, -1)
            per = mk.sum((0, 2))
            if not bool(((per == 0) | (per == mk.shape[0] * kb)).all()):
                return False
        return True
    return bool(((m == 0) | (m == 1)).all())


@pytest.mark.parametrize("method", ["taylor-weight", "taylor-block", "taylor-filter"])
def test_train_taylor_methods(dev, tmp_path, method):
    """train(pruning_method="taylor-*"): the masks have the granularity's structure, about half is pruned, and what was
    masked is still zero after the epoch."""
    t = YOLOv2Train()
    t.TAYLOR_STEPS = 2
    m = t.train('', '', '', str(tmp_path / "log"), '', '', 'p_', MINI, '', 4, 10, DEBUG_EPOCHS=0, MAX_EPOCHS=1,
                SYNTHETIC_SAMPLES=8, pruning_perc=50, pruning_method=method)
    assert YOLOv2Train.TAYLOR_STEPS == 16
    convs = [mod for mod in m.modules() if getattr(mod, "mask_flag", False)]
    masks = [c.mask for c in convs]
    assert len(masks) == len([p for p in m.parameters() if p.dim() == 4]) == 7
    assert are_masks_consistent(m, masks)
    assert all(structure_ok(method, c) for c in convs), "not a %s mask" % method
    zero = sum(float((k == 0).sum()) for k in masks) / sum(k.numel() for k in masks)
    print("%s: %.1f %% of the weights masked" % (method, 100 * zero))
    assert 0.05 < zero < 0.95
    if method == "taylor-weight":
        assert abs(zero - 0.5) < 0.01
    for c in convs:
        assert float((c.weight.detach().abs() * (1 - c.mask)).sum()) == 0.0
    for p in m.parameters():
        assert torch.isfinite(p).all()
