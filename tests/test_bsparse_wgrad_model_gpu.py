"""Darknet.sparse_train = "block-wgrad" (DESIGN.md 3zd): the fp16 training step of a block_prune-masked YOLOv2-VOC with the
weight gradient of the chosen blocks on the list launch mcamd_conv_wgrad_bsparse -- which blocks take it, bit identity of
the skipping, exact zeros and finite gradients, accuracy against the fp32 masked-dense oracle next to the dense fp16
engine's, lists rebuilt when the masks change, the bound 0.0, and allocations of a warm step."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402
import bsparse_wgrad_cases as BC  # noqa: E402
from test_bsparse_train_model_gpu import pruned, batch, engine_of, step, running, restore, assert_same  # noqa: E402


def wpruned(dev, wgrad_max_kept=1.0, sparse_train="block-wgrad", **kw):
    """pruned() with the weight gradient's bound set explicitly: the test does not hang on the measured default."""
    blocks, state, m, masks = pruned(dev, sparse_train=sparse_train, **kw)
    m.sparse_train_wgrad_max_kept = wgrad_max_kept
    return blocks, state, m, masks


@pytest.fixture(scope="module")
def first(dev):
    """One step of a fresh "block-wgrad" model, shared by the tests that only read it."""
    blocks, state, m, masks = wpruned(dev)
    x, gout = batch(dev)
    init = running(m)
    s = step(m, x, gout, dev)
    return dict(blocks=blocks, state=state, m=m, masks=masks, x=x, gout=gout, init=init, s=s)


def test_which_blocks_take_the_list_launch(dev, first):
    eng = engine_of(first["m"])
    kept = dict(eng.bsparse_train_wgrad_kept)
    print("kept (tile, tap) fractions: %s" % " ".join("%d:%.3f" % kv for kv in sorted(kept.items())))
    print("weight gradient on the list launch: %s" % eng.bsparse_train_wgrad_layers)
    assert eng.bsparse_train_wgrad_layers
    want = [lay.li + 1 for lay in eng.layers
            if lay.form == "bsparse_train" and not lay.gather and lay.perm is None and lay.fold is None
            and not eng._bwd1x1_route(lay) and ops.conv_wgrad_bsparse_ok(lay.geom)]
    assert eng.bsparse_train_wgrad_layers == want
    assert set(want) <= set(eng.bsparse_train_layers) and set(want) <= set(kept)
    assert all(0.0 < v <= 1.0 for v in kept.values())
    # the lists on the layers are what the masks say, and the host integers are the device counters
    for lay in eng.layers:
        if lay.bw_on:
            tiles, words, allw, counts = BC.lists_of(lay.conv.mask.cpu().numpy())
            assert lay.bw_counts == counts and lay.bw_dev_counts.cpu().tolist() == list(counts), lay.li + 1
            assert lay.bw_tiles.cpu().tolist()[:counts[0]] == tiles.tolist(), lay.li + 1
            assert lay.bw_words.cpu().tolist()[:counts[0]] == words.tolist(), lay.li + 1
            assert lay.bw_nsplit == ops.conv_wgrad_bsparse_plan(lay.geom, counts[0]).nsplit
            assert kept[lay.li + 1] == counts[1] / float(len(allw) * lay.k * lay.k)


def test_skipping_is_bit_identical(dev, first):
    """One step on the lists equals the same step on full lists (at the short lists' split counts): logits, every gradient,
    the running statistics."""
    m, eng = first["m"], engine_of(first["m"])
    chosen = list(eng.bsparse_train_wgrad_layers)
    restore(m, first["init"])
    eng.bsparse_train_full_lists = True
    try:
        b = step(m, first["x"], first["gout"], dev)
    finally:
        eng.bsparse_train_full_lists = False
    restore(m, first["init"])
    assert engine_of(m) is eng and eng.bsparse_train_wgrad_layers == chosen
    assert_same(first["s"], b, "lists vs full lists")


def test_masked_gradients_are_zero_and_all_finite(dev, first):
    grads = first["s"][1]
    convs = [(n, c) for n, c in first["m"].named_modules() if getattr(c, "mask_flag", False)]
    zeros = 0
    for n, c in convs:
        g = grads[n + ".weight"]
        assert bool((g[c.mask == 0] == 0).all()), n
        zeros += int((c.mask == 0).sum())
    assert zeros > 0
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())


def test_accuracy_against_the_fp32_oracle(dev, first):
    """Per tensor against the fp32 masked-dense CPU oracle, next to the dense fp16 engine's error against the same oracle:
    the bound of test_bsparse_train_model_gpu.py (the same fp16 operands, fp32 accumulation, another summation order:
    at most 1.25 x the dense error)."""
    blocks, x, gout, s = first["blocks"], first["x"], first["gout"], first["s"]
    st = {k: v.clone() for k, v in first["state"].items()}
    for k in O.param_keys(blocks):
        st[k].requires_grad_(True)
    ref = O.forward(blocks, st, x, training=True, masks=[k.cpu() for k in first["masks"]])
    ref.backward(gout)
    _, _, md, _ = pruned(dev, sparse_train=None)
    d = step(md, x, gout, dev)
    es, ed = rel_l2(s[0].cpu(), ref.detach()), rel_l2(d[0].cpu(), ref.detach())
    print("logits vs fp32 oracle: block-wgrad %.3e, dense fp16 %.3e" % (es, ed))
    bad = []
    for k in O.param_keys(blocks):
        a, b_ = rel_l2(s[1][k].cpu(), st[k].grad), rel_l2(d[1][k].cpu(), st[k].grad)
        print("  grad %-16s block-wgrad %.3e dense %.3e ratio %.3f" % (k, a, b_, a / max(b_, 1e-30)))
        if not a <= 1.25 * b_:
            bad.append(k)
    assert es <= 1.25 * ed
    assert not bad, bad


def test_lists_are_rebuilt_when_the_masks_change(dev):
    """set_masks with other masks on a live engine: the next step equals a fresh engine's step with those masks."""
    x, gout = batch(dev)
    _, _, m, masks = wpruned(dev)
    init = running(m)
    step(m, x, gout, dev)
    eng = engine_of(m)
    before = {lay.li: lay.bw_words.cpu().tolist() for lay in eng.layers if lay.bw_on}
    w0 = {n: p.detach().clone() for n, p in m.named_parameters()}
    # the same masks moved by one block of 64 filters: other tiles and taps, and the blocks they newly keep hold zero weights
    # (a kept weight that is zero still has a gradient: the lists must come from the masks)
    masks2 = [torch.roll(k, 64, dims=0).contiguous() for k in masks]
    m.set_masks(masks2)
    restore(m, init)
    a = step(m, x, gout, dev)
    assert engine_of(m) is eng, "the live engine must have taken the new masks"
    after = {lay.li: lay.bw_words.cpu().tolist() for lay in eng.layers if lay.bw_on}
    assert after and after.keys() == before.keys() and sum(after[k] != before[k] for k in after) >= len(after) // 2
    for lay in eng.layers:
        if lay.bw_on:
            assert lay.bw_counts == BC.lists_of(lay.conv.mask.cpu().numpy())[3], lay.li + 1
    # a fresh model with the same weights and masks
    _, _, m2, _ = wpruned(dev)
    with torch.no_grad():
        for n, p in m2.named_parameters():
            p.copy_(w0[n])
    m2.set_masks([k.clone() for k in masks2])
    restore(m2, init)
    b = step(m2, x, gout, dev)
    assert engine_of(m2).bsparse_train_wgrad_layers == eng.bsparse_train_wgrad_layers
    assert_same(a, b, "live engine after set_masks vs fresh engine")


def test_bound_zero_is_block(dev, first):
    x, gout = first["x"], first["gout"]
    _, _, m0, _ = wpruned(dev, wgrad_max_kept=0.0)
    a = step(m0, x, gout, dev)
    assert engine_of(m0).bsparse_train_wgrad_layers == [] and engine_of(m0).bsparse_train_layers
    assert all(lay.bw_tiles is None for lay in engine_of(m0).layers), "no list is built"
    _, _, m1, _ = pruned(dev, sparse_train="block")
    b = step(m1, x, gout, dev)
    assert engine_of(m1).bsparse_train_wgrad_layers == []
    assert_same(a, b, "wgrad bound 0.0 vs 'block'")


def test_a_warm_step_allocates_nothing(dev, first):
    m = first["m"]
    eng = engine_of(m)
    assert eng.use_plan and eng.bsparse_train_wgrad_layers
    xd, gd = first["x"].to(dev), first["gout"].to(dev)
    for _ in range(2):
        m(xd).backward(gd)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(dev)
    m(xd).backward(gd)
    torch.cuda.synchronize()
    after = torch.cuda.memory_stats(dev)
    assert after["num_alloc_retries"] == before["num_alloc_retries"]
    assert after["segment.all.allocated"] == before["segment.all.allocated"]
    restore(m, first["init"])
