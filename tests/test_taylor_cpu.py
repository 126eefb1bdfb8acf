"""Taylor-importance pruning without a device (importance.py, csrc/taylor.hip's C surface): the symbols, the
refusals of mcamd_taylor_accum, the numpy restatement on cases worked out by hand, the package's torch path against the
restatement, taylor_prune on hand-made accumulators, and the all-reduce over gloo."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import modelcompression_amd
from modelcompression_amd import _lib, importance, ops
from modelcompression_amd._lib import McamdError
from modelcompression_amd.importance import TaylorImportance, taylor_prune
from modelcompression_amd.pruning.weightPruning import methods
from modelcompression_amd.pruning.weightPruning.layers import MaskedConv2d
import bsparse_ref as B
import taylor_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcamd_taylor_seg_workgroups", "mcamd_taylor_accum")


# ----------------------------------------------------------------------------- the C surface
def test_symbols_are_declared_bound_exported_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mcamd_taylor_\w+)\(", hdr))
    assert declared == set(NAMES) == set(k for k in _lib.SIGNATURES if k.startswith("mcamd_taylor_"))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r" T (mcamd_taylor_\w+)", out)) == set(NAMES)
    lib = _lib.lib()
    assert all(hasattr(lib, name) for name in NAMES)
    body = re.search(r"typedef struct mcamd_taylor_seg \{(.*?)\} mcamd_taylor_seg;", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.TaylorSeg._fields_] and C.sizeof(_lib.TaylorSeg) == 80
    for name, value in (("MCAMD_TAYLOR_CONV", _lib.TAYLOR_CONV), ("MCAMD_TAYLOR_GATE", _lib.TAYLOR_GATE)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
    assert len(_lib.SIGNATURES["mcamd_taylor_accum"][1]) == 6
    src = open(os.path.join(ROOT, "modelcompression_amd", "build.py")).read()
    assert re.search(r'"taylor.hip": \["-ffp-contract=off"\]', src)
    assert callable(ops.TaylorTable) and callable(ops.TaylorTable.accumulate)
    assert modelcompression_amd.taylor_prune is methods.taylor_prune is importance.taylor_prune
    assert modelcompression_amd.TaylorImportance is TaylorImportance


def test_train_takes_the_new_method_values_without_a_new_parameter():
    from modelcompression_amd import train
    assert train.YOLOv2Train.TAYLOR_STEPS == 16
    assert train.TAYLOR_METHODS == {"taylor-weight": "weight", "taylor-block": "block", "taylor-filter": "filter"}
    names = list(inspect.signature(train.YOLOv2Train.train).parameters)
    assert not any("taylor" in n.lower() for n in names)


def seg(**kw):
    s = _lib.TaylorSeg()
    s.w, s.g, s.acc_w, s.acc_b, s.acc_f = 4096, 8192, 12288, 16384, None
    s.kind, s.cout, s.cin, s.khw, s.wg0 = _lib.TAYLOR_CONV, 70, 64, 9, 0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


GATE = dict(kind=_lib.TAYLOR_GATE, cin=1, khw=1, bias=20480, gbias=24576, acc_w=None, acc_b=None, acc_f=28672)


@pytest.mark.parametrize("bad,text", [
    (dict(w=None), "null tensor"),
    (dict(g=None), "null tensor"),
    (dict(w=4098), "4-byte aligned"),
    (dict(acc_w=12290), "4-byte aligned"),
    (dict(acc_b=16388), "8-byte aligned"),
    (dict(acc_f=16388), "8-byte aligned"),
    (dict(cin=48), "block scores need cin % 32 == 0 (cin 48)"),
    (dict(cin=3), "block scores need cin % 32 == 0 (cin 3)"),
    (dict(cout=0), "bad shape"),
    (dict(kind=2), "unknown kind 2"),
    (dict(bias=20480), "a bias and its gradient go together"),
    (dict(acc_w=None, acc_b=None), "no output"),
    (dict(wg0=1), "wg0 1 is not the running sum 0"),
    (dict(GATE, bias=None), "a gate needs beta, dbeta and acc_f"),
    (dict(GATE, acc_f=None), "a gate needs beta, dbeta and acc_f"),
    (dict(GATE, acc_w=12288), "filter scores only"),
    (dict(GATE, cin=2), "filter scores only"),
])
def test_accum_refuses_bad_tables(bad, text):
    """Every argument error is refused before a launch (the pointers are never dereferenced: this runs without a device)."""
    lib = _lib.lib()
    arr = (_lib.TaylorSeg * 1)(seg(**bad))
    assert lib.mcamd_taylor_accum(arr, 4096, 1, None, 4096, None) == -1
    err = lib.mcamd_last_error().decode()
    assert text in err and err.startswith("taylor_accum:"), err


def test_accum_refuses_bad_arguments_and_inconsistent_offsets():
    lib = _lib.lib()
    err = lambda: lib.mcamd_last_error().decode()
    one = (_lib.TaylorSeg * 1)(seg())
    assert lib.mcamd_taylor_accum(None, 4096, 1, None, 4096, None) == -1 and "null argument" in err()
    assert lib.mcamd_taylor_accum(one, None, 1, None, 4096, None) == -1 and "null argument" in err()
    assert lib.mcamd_taylor_accum(one, 4096, 1, None, None, None) == -1 and "null argument" in err()
    assert lib.mcamd_taylor_accum(one, 4096, 0, None, 4096, None) == -1 and "null argument" in err()
    assert lib.mcamd_taylor_accum(one, 4096, 1, 4098, 4096, None) == -1 and "misaligned" in err()
    assert lib.mcamd_taylor_accum(one, 4096, 1, None, 4098, None) == -1 and "misaligned" in err()
    # (70, 64, 9) with block scores: 2 filter blocks x 1 channel block; a gate of 300 channels: 2 workgroups
    assert lib.mcamd_taylor_seg_workgroups(C.byref(seg())) == 2
    assert lib.mcamd_taylor_seg_workgroups(C.byref(seg(acc_f=16384))) == 2 + 18
    assert lib.mcamd_taylor_seg_workgroups(C.byref(seg(acc_b=None))) == (70 * 64 * 9 + 2047) // 2048
    assert lib.mcamd_taylor_seg_workgroups(C.byref(seg(cout=300, **GATE))) == 2
    assert lib.mcamd_taylor_seg_workgroups(C.byref(seg(cin=3))) == 0
    two = (_lib.TaylorSeg * 2)(seg(), seg(cout=300, wg0=3, **GATE))
    assert lib.mcamd_taylor_accum(two, 4096, 2, None, 4096, None) == -1 and "segment 1: wg0 3 is not the running sum 2" in err()


def test_accum_is_recorded_while_a_plan_records():
    """Launch-type: a valid table is appended to the plan being recorded instead of launched (pure host work)."""
    lib = _lib.lib()
    streams = (C.c_void_p * 1)(None)
    assert lib.mcamd_plan_begin(streams, 1) == 0
    try:
        one = (_lib.TaylorSeg * 1)(seg())
        assert lib.mcamd_taylor_accum(one, 4096, 1, None, 4096, None) == 0
        bad = (_lib.TaylorSeg * 1)(seg(wg0=1))
        assert lib.mcamd_taylor_accum(bad, 4096, 1, None, 4096, None) == -1          # the checks come first
    finally:
        plan = lib.mcamd_plan_end()
    assert plan and lib.mcamd_plan_launches(plan) == 1
    lib.mcamd_plan_destroy(plan)


def test_wrapper_has_no_cpu_path():
    w = torch.zeros(2, 3, 1)
    with pytest.raises(McamdError, match="no CPU path"):
        ops.TaylorTable([dict(w=w, g=w.clone(), acc_w=w.clone())], torch.zeros(1, dtype=torch.int32))


# ----------------------------------------------------------------------------- the restatement, by hand
def test_restatement_single_nonzero_block():
    """(128, 128, 9): blocks of 64 x 64.  g w = 0.5 on block (fb 1, cb 0, tap 4) alone: S = 64 * 64 * 0.5 exactly."""
    w = np.zeros((128, 128, 3, 3), np.float32)
    g = np.ones_like(w)
    w[64:128, 0:64, 1, 1] = 0.5
    S = R.block_sums(w, g).reshape(2, 2, 9)
    want = np.zeros((2, 2, 9))
    want[1, 0, 4] = 2048.0
    assert np.array_equal(S, want)
    acc_b, acc_w = np.full(36, 1.0), np.zeros(w.shape, np.float32)
    R.conv_step(w, g, acc_w=acc_w, acc_b=acc_b)
    assert np.array_equal(acc_b.reshape(2, 2, 9), 1.0 + want * want)
    assert np.array_equal(acc_w, (w * w).astype(np.float32))
    # opposite signs cancel inside a block although every weight score is positive: the group score is not their sum
    g[64:96, 0:64, 1, 1] = -1.0
    assert R.block_sums(w, g).reshape(2, 2, 9)[1, 0, 4] == 0.0 and R.weight_term(w, g)[64:128, 0:64, 1, 1].min() == 0.25


def test_restatement_ragged_last_filter_block_and_order():
    """(70, 32, 1): kb 32, the second filter block holds 6 rows = 192 elements, 3 per lane."""
    rng = np.random.default_rng(1)
    w = rng.standard_normal((70, 32, 1, 1)).astype(np.float32)
    g = rng.standard_normal((70, 32, 1, 1)).astype(np.float32)
    p = (g * w).reshape(70, 32).astype(np.float64)
    S = R.block_sums(w, g)
    assert S.shape == (2,)
    e = p[64:70].reshape(-1)                      # e = r * 32 + c
    lanes = [(e[l] + e[l + 64]) + e[l + 128] for l in range(64)]
    for d in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l ^ d] for l in range(64)]
    assert S[1] == lanes[0]
    # a filter sum of the same tensor: memory order over 32 elements, lanes 32..63 hold 0.0
    F = R.filter_sums(w, g, bias=np.full(70, 3.0, np.float32), gbias=np.full(70, 0.5, np.float32))
    lanes = list(p[5]) + [0.0] * 32
    for d in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l ^ d] for l in range(64)]
    assert F[5] == lanes[0] + 1.5


def test_restatement_cin3_takes_weight_scores_only():
    w = np.arange(2 * 3 * 9, dtype=np.float32).reshape(2, 3, 3, 3) / 8
    g = np.full_like(w, 0.25)
    assert B.block_dims(2, 3, 9) is None
    acc_w = np.ones(w.shape, np.float32)
    R.conv_step(w, g, acc_w=acc_w)
    assert np.array_equal(acc_w, 1 + (w / 4) ** 2)
    t = R.gate_sums([2.0, -1.0], [0.5, 3.0], [1.0, 3.0], [-1.0, 1.0])
    assert np.array_equal(t, [0.0, 0.0])          # gamma dgamma + beta dbeta cancels exactly
    acc_f = np.zeros(2)
    R.gate_step([2.0, 1.0], [0.5, 3.0], [1.0, 0.0], [1.0, 1.0], acc_f)
    assert np.array_equal(acc_f, [4.0, 9.0])


# ----------------------------------------------------------------------------- the torch path
def block(cin, cout, k, bn=True, masked=False):
    conv = (MaskedConv2d if masked else nn.Conv2d)(cin, cout, k, padding=k // 2, bias=not bn)
    return nn.Sequential(conv, nn.BatchNorm2d(cout), nn.LeakyReLU(0.1)) if bn else nn.Sequential(conv)


def make_model(seed=0, masked=False):
    """(70, 3, 9) ineligible; (70, 64... kb 64 ragged); (64, 96, 1) kb 32; the last conv without BatchNorm, with a bias."""
    torch.manual_seed(seed)
    model = nn.Sequential(block(3, 64, 3, masked=masked), block(64, 70, 3, masked=masked), block(70, 96, 1, masked=masked),
                          block(96, 64, 1, masked=masked), block(64, 5, 1, bn=False, masked=masked))
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.5, 0.5)
    return model


def set_grads(model, seed):
    gen = torch.Generator().manual_seed(seed)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=gen)


def ref_step(model, acc):
    """One restatement step on acc = [dict(acc_w, acc_b, acc_f)] per prunable parameter."""
    for seq, a in zip(model, acc):
        conv = seq[0]
        bn = seq[1] if len(seq) > 1 else None
        w, g = conv.weight.detach().numpy(), conv.weight.grad.numpy()
        if bn is None:
            R.conv_step(w, g, conv.bias.detach().numpy(), conv.bias.grad.numpy(), a["acc_w"], a["acc_b"], a["acc_f"])
        else:
            R.conv_step(w, g, acc_w=a["acc_w"], acc_b=a["acc_b"])
            R.gate_step(bn.weight.detach().numpy(), bn.weight.grad.numpy(), bn.bias.detach().numpy(), bn.bias.grad.numpy(), a["acc_f"])


def ref_acc(model):
    acc = []
    for seq in model:
        w = seq[0].weight
        dims = B.block_dims(w.shape[0], w.shape[1], w.shape[2] * w.shape[3])
        acc.append(dict(acc_w=np.zeros(tuple(w.shape), np.float32),
                        acc_b=None if dims is None else np.zeros(dims[0] * dims[1] * w.shape[2] * w.shape[3]),
                        acc_f=np.zeros(w.shape[0])))
    return acc


def assert_same(imp, acc):
    for got, name in ((imp.weight_scores(), "acc_w"), (imp.block_scores(), "acc_b"), (imp.filter_scores(), "acc_f")):
        for t, a in zip(got, acc):
            assert (t is None) == (a[name] is None), name
            if t is not None:
                want = torch.from_numpy(a[name])
                assert t.dtype == want.dtype and t.shape == want.shape
                bits = torch.int32 if t.dtype == torch.float32 else torch.int64
                assert torch.equal(t.view(bits), want.view(bits)), name


def test_torch_path_equals_the_restatement_exactly():
    model = make_model()
    imp = TaylorImportance(model)
    assert [p.shape[1] for p in imp.params] == [3, 64, 70, 96, 64]
    assert [a is not None for a in imp.block_scores()] == [False, True, False, True, True]
    acc = ref_acc(model)
    acc[2]["acc_b"] = None                          # cin 70: no block form
    with pytest.raises(McamdError, match="after backward"):
        imp.accumulate()
    for step in range(3):
        set_grads(model, 10 + step)
        imp.accumulate()
        ref_step(model, acc)
        assert_same(imp, acc)
    assert imp.steps() == 3
    set_grads(model, 99)
    imp.accumulate(skip=torch.ones(1))              # a flagged step: nothing moves
    assert imp.steps() == 3
    assert_same(imp, acc)
    imp.accumulate(skip=torch.zeros(1))
    assert imp.steps() == 4
    imp.reset()
    assert imp.steps() == 0 and all(float(t.abs().sum()) == 0 for t in imp.weight_scores())


def test_outputs_that_are_off_are_not_allocated():
    model = make_model()
    imp = TaylorImportance(model, weight=False, block=False)
    assert all(t is None for t in imp.weight_scores() + imp.block_scores()) and all(t is not None for t in imp.filter_scores())
    set_grads(model, 1)
    imp.accumulate()
    acc = ref_acc(model)
    ref_step(model, acc)
    for t, a in zip(imp.filter_scores(), acc):
        assert torch.equal(t, torch.from_numpy(a["acc_f"]))
    with pytest.raises(McamdError, match="weight=True"):
        taylor_prune(model, 50, imp, "weight")
    with pytest.raises(McamdError, match="all off"):
        TaylorImportance(model, weight=False, block=False, filter=False)


# ----------------------------------------------------------------------------- taylor_prune on hand-made accumulators
def fill(imp, name, arrays, steps=1):
    for lay, a in zip(imp.layers, arrays):
        if a is not None:
            lay[name].copy_(torch.as_tensor(np.asarray(a)).view(lay[name].shape))
    imp._steps.fill_(steps)


def two_layer(masked=False):
    torch.manual_seed(0)
    return nn.Sequential(block(32, 70, 1, masked=masked), block(70, 4, 1, bn=False, masked=masked))


def test_steps_zero_raises_and_arguments_are_checked():
    model = two_layer()
    imp = TaylorImportance(model)
    for gran in importance.GRANULARITIES:
        with pytest.raises(McamdError, match="no step has been accumulated"):
            taylor_prune(model, 50, imp, gran)
    imp._steps.fill_(1)
    with pytest.raises(McamdError, match="granularity"):
        taylor_prune(model, 50, imp, "channel")
    with pytest.raises(McamdError, match="another model"):
        taylor_prune(two_layer(), 50, imp, "weight")


def test_weight_a_large_weight_with_zero_gradient_goes_and_ties_are_pruned():
    model = two_layer()
    w0, w1 = model[0][0].weight.data, model[1][0].weight.data
    w0.fill_(0.01), w1.fill_(0.01)
    w0[0, 0, 0, 0] = 100.0                          # the largest weight of the model; its gradient is zero
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    model[0][0].weight.grad[0, 0, 0, 0] = 0.0
    model[1][0].weight.grad[:, :35] = 4.0           # half of the second layer carries 16x the score of the rest
    imp = TaylorImportance(model)
    imp.accumulate()
    masks = taylor_prune(model, 50, imp, "weight")
    assert [tuple(m.shape) for m in masks] == [tuple(w0.shape), tuple(w1.shape)] and all(m.dtype == torch.float32 for m in masks)
    assert masks[0][0, 0, 0, 0] == 0                # weight_prune would keep it: |w| = 100
    by_magnitude = (torch.cat([w0.reshape(-1), w1.reshape(-1)]).abs() > 0.01)
    assert bool(by_magnitude[0]) and int(by_magnitude.sum()) == 1
    # every score but 140 equals the threshold: strict >, so the tie is pruned, all of it
    assert float(masks[0].sum()) == 0 and torch.equal(masks[1], (model[1][0].weight.grad == 4.0).float())
    ref = R.weight_masks([t.numpy() for t in imp.weight_scores()], 50)
    assert all(torch.equal(m, torch.from_numpy(r)) for m, r in zip(masks, ref))
    per = taylor_prune(model, 50, imp, "weight", per_layer=True)
    ref = R.weight_masks([t.numpy() for t in imp.weight_scores()], 50, per_layer=True)
    assert all(torch.equal(m, torch.from_numpy(r)) for m, r in zip(per, ref))


@pytest.mark.parametrize("perc", [10, 37.5, 80])
def test_weight_matches_numpy_percentile_on_random_scores(perc):
    model = make_model()
    imp = TaylorImportance(model, block=False, filter=False)
    rng = np.random.default_rng(5)
    fill(imp, "acc_w", [rng.random(tuple(p.shape), dtype=np.float32) ** 4 for p in imp.params], steps=3)
    masks = taylor_prune(model, perc, imp, "weight")
    ref = R.weight_masks([t.numpy() for t in imp.weight_scores()], perc)
    assert all(torch.equal(m, torch.from_numpy(r)) for m, r in zip(masks, ref))
    kept = sum(float(m.sum()) for m in masks) / sum(m.numel() for m in masks)
    assert abs(kept - (1 - perc / 100)) < 1e-3


def test_weight_old_masks_compose():
    model = two_layer(masked=True)
    old = torch.ones_like(model[0][0].weight.data)
    old[:35] = 0
    model[0][0].set_mask(old)                       # zeroes those weights: their scores are 0 whatever the gradient
    model[1][0].set_mask(torch.ones_like(model[1][0].weight.data))
    set_grads(model, 3)
    imp = TaylorImportance(model)
    imp.accumulate()
    assert float(imp.weight_scores()[0][:35].abs().sum()) == 0
    for perc in (5, 60):
        masks = taylor_prune(model, perc, imp, "weight")
        assert float(masks[0][:35].sum()) == 0 and float(masks[0][35:].sum()) > 0


def test_block_every_layer_keeps_its_best_block_and_old_masks_compose():
    torch.manual_seed(0)
    model = nn.Sequential(block(3, 64, 3, masked=True), block(64, 130, 3, masked=True), block(130, 32, 1, masked=True),
                          block(32, 70, 1, bn=False, masked=True))
    old = (torch.rand(130, 64, 3, 3) > 0.3).float()
    model[1][0].set_mask(old)
    imp = TaylorImportance(model)
    shapes = [tuple(p.shape) for p in imp.params]
    assert [a is not None for a in imp.block_scores()] == [False, True, False, True]
    rng = np.random.default_rng(2)
    big = rng.random(3 * 1 * 9) + 10.0              # every block of this layer outranks ...
    small = rng.random(2 * 1 * 1) * 1e-3            # ... both blocks of this one
    small[1] = small[0]                             # a tie for the best: the lower index stays
    fill(imp, "acc_b", [None, big, None, small], steps=4)
    masks = taylor_prune(model, 60, imp, "block")
    ref = R.block_masks(shapes, [None, big, None, small], 4, 60, [None, old.numpy(), None, None])
    assert all(torch.equal(m, torch.from_numpy(r)) for m, r in zip(masks, ref))
    assert torch.equal(masks[0], torch.ones(shapes[0])) and torch.equal(masks[2], torch.ones(shapes[2]))    # no block form
    assert float(masks[3][:64].min()) == 1 and float(masks[3][64:].max()) == 0
    assert bool(((masks[1] == 0) | (old == 1)).all()) and 0 < float(masks[1].sum()) < float(old.sum())
    per = taylor_prune(model, 60, imp, "block", per_layer=True)
    ref = R.block_masks(shapes, [None, big, None, small], 4, 60, [None, old.numpy(), None, None], per_layer=True)
    assert all(torch.equal(m, torch.from_numpy(r)) for m, r in zip(per, ref))


def test_filter_scores_come_from_the_gate_and_every_layer_keeps_its_best_filter():
    model = make_model()
    imp = TaylorImportance(model, weight=False, block=False)
    shapes = [tuple(p.shape) for p in imp.params]
    rng = np.random.default_rng(3)
    acc = [rng.random(s[0]) for s in shapes]
    acc[2] = np.zeros(96)                           # a layer whose scores are all 0: not normalised, keeps filter 0 only
    acc[3][7] = acc[3][20] = acc[3].max() + 1.0     # a tie for the best
    acc[4] = acc[4] * 1e-9                          # normalisation: a layer is ranked inside itself, not by its scale
    fill(imp, "acc_f", acc, steps=2)
    masks = taylor_prune(model, 50, imp, "filter")
    ref = R.filter_masks(shapes, acc, 2, 50)
    assert all(torch.equal(m, torch.from_numpy(r)) for m, r in zip(masks, ref))
    assert float(masks[2].sum()) == shapes[2][1] * shapes[2][2] * shapes[2][3] and float(masks[2][0].min()) == 1
    assert float(masks[3][7].min()) == 1
    assert 0 < float(masks[4].sum())
    for m in masks:                                 # whole filters
        flat = m.reshape(m.shape[0], -1)
        assert bool((flat.min(1).values == flat.max(1).values).all())
    masks = taylor_prune(model, 100, imp, "filter")         # the threshold is the largest score of all
    ref = R.filter_masks(shapes, acc, 2, 100)
    assert all(torch.equal(m, torch.from_numpy(r)) for m, r in zip(masks, ref))
    kept = [m.reshape(m.shape[0], -1)[:, 0] for m in masks]
    assert all(1 <= int(k.sum()) <= 2 for k in kept) and sum(int(k.sum()) for k in kept) <= 6
    assert kept[3][7] == 1 and kept[2][0] == 1      # the first of equal maxima stays
    per = taylor_prune(model, 50, imp, "filter", per_layer=True)
    ref = R.filter_masks(shapes, acc, 2, 50, per_layer=True)
    assert all(torch.equal(m, torch.from_numpy(r)) for m, r in zip(per, ref))


def test_a_filter_under_batchnorm_is_scored_by_the_gate_not_by_its_weights():
    """Euler's theorem on a real graph: with BatchNorm on batch statistics sum(g w) over a filter vanishes, the gate does not.
    (BatchNorm's eps leaves the filter's own sum at a relative size of eps / var: the weights are made large.)"""
    torch.manual_seed(0)
    model = nn.Sequential(block(3, 8, 3), block(8, 4, 1, bn=False)).double()
    model[0][0].weight.data.mul_(1e4)
    x = torch.randn(6, 3, 8, 8, dtype=torch.float64)
    model.train()
    model(x).square().sum().backward()
    conv, bn = model[0][0], model[0][1]
    own = (conv.weight.grad * conv.weight.detach()).reshape(8, -1).sum(1)
    gate = bn.weight.grad * bn.weight.detach() + bn.bias.grad * bn.bias.detach()
    assert float(own.abs().max()) < 1e-9 * float(gate.abs().max())


# ----------------------------------------------------------------------------- data parallel
def _gloo_worker(rank, world, port, tmp):
    import torch.distributed as dist
    from modelcompression_amd import dp
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    assert dp.init_from_env("gloo") == (rank, world)
    model = make_model()
    imp = TaylorImportance(model)
    for step in range(1 + rank):                    # rank 0 scores one step, rank 1 two
        set_grads(model, 100 * rank + step)
        imp.accumulate()
    imp.all_reduce()
    assert imp.steps() == 3
    masks = {g: dp.broadcast_masks(taylor_prune(model, 50, imp, g), src=0) for g in importance.GRANULARITIES}
    torch.save(dict(acc=[imp.weight_scores(), imp.block_scores(), imp.filter_scores()], masks=masks),
               os.path.join(tmp, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_gloo_world2(tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = (torch.load(tmp_path / ("rank%d.pt" % r)) for r in (0, 1))
    # what each rank had on its own, summed (a two-term sum: no order to pin)
    want = []
    for rank in (0, 1):
        model = make_model()
        imp = TaylorImportance(model)
        for step in range(1 + rank):
            set_grads(model, 100 * rank + step)
            imp.accumulate()
        want.append([imp.weight_scores(), imp.block_scores(), imp.filter_scores()])
    for kind in range(3):
        for x, y, u, v in zip(a["acc"][kind], b["acc"][kind], want[0][kind], want[1][kind]):
            assert (x is None) == (u is None)
            if x is not None:
                assert torch.equal(x, y) and torch.equal(x, u + v)
    for g in importance.GRANULARITIES:
        assert all(torch.equal(x, y) for x, y in zip(a["masks"][g], b["masks"][g]))
        assert any(float(x.min()) == 0 for x in a["masks"][g])
