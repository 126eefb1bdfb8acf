"""Darknet.precision = "fp8-block": block-pruned YOLOv2-VOC on the block-sparse fp8 kernel (csrc/conv_q8_bsparse.hip,
Engine._choose_forms) -- bit equality with the "fp8" engine where both run the same blocks, the layers a global
block_prune empties (which "fp8" loses to the filter compaction), the error level against the CPU restatement, the policy
bound, refusals and read-outs, the switch from an "fp8-qat" fine-tune, compressed-file round trips, no allocation in a warm forward and model.detect."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, engine as E, nets2_utils as U, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import block_prune  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402
import q8_ref as R  # noqa: E402

EXPECTED = list(range(3, 23))      # conv3 ... conv22: every candidate of YOLOv2-VOC


def pruned(dev, seed, per_layer, max_kept=None):
    """Seeded YOLOv2-VOC, block_prune(75), masks set, eval.  Seed 1 with per_layer=True leaves no filter without a kept
    block (bsparse_ref.block_prune says so on the CPU); the global threshold empties conv19 / 20 / 22 down to one block."""
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(blocks, seed=seed))
    m.to(dev)
    masks = block_prune(m, 75.0, per_layer=per_layer)
    m.set_masks(masks)
    m.eval()
    if max_kept is not None:
        m.fp8_block_max_kept = max_kept
    return blocks, m, masks


def engine_for(m, x, prec="fp8-block"):
    return [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and k[3] == prec and not e.train_layout][0]


def run(m, x, prec):
    m.precision = prec
    with torch.no_grad():
        return m(x).clone()


def mask_fractions(masks):
    """conv number -> kept fraction of the (64-filter tile, 64-channel block, tap) blocks, from the masks alone."""
    out = {}
    for i, mk in enumerate(masks):
        co, ci = mk.shape[:2]
        if ci % 64 != 0 or i + 1 not in EXPECTED:
            continue
        t = -(-co // 64)
        full = np.zeros((t * 64, ci, mk.shape[2] * mk.shape[3]), np.float32)
        full[:co] = mk.cpu().numpy().reshape(co, ci, -1)
        out[i + 1] = float(full.reshape(t, 64, ci // 64, 64, -1).max(axis=(1, 3)).astype(np.float64).mean())
    return out


@pytest.mark.parametrize("mfma", [0, 1], ids=["f16mfma", "f8mfma"])
def test_equals_fp8_where_both_run_the_same_blocks(dev, setenv, mfma):
    """block_prune(75, per_layer=True), seed 1: no filter dies, so "fp8" compacts nothing and runs conv3 .. conv22; under
    fp8_block_max_kept = 1.0 every one of them runs the block-sparse kernel and the logits are the same bits."""
    setenv("MCAMD_Q8_MFMA", str(mfma))
    _, m, masks = pruned(dev, 1, True, max_kept=1.0)
    assert all(bool((mk.reshape(mk.shape[0], -1).amax(1) != 0).all()) for mk in masks), "a filter died: pick another seed"
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(5)).to(dev)
    q = run(m, x, "fp8")
    b = run(m, x, "fp8-block")
    dense, block = engine_for(m, x, "fp8"), engine_for(m, x)
    assert dense.fp8_layers == block.fp8_layers == EXPECTED
    assert block.fp8_block_layers == EXPECTED and dense.fp8_block_layers == []
    same = torch.equal(b, q)
    print("MCAMD_Q8_MFMA=%d: fp8-block equals fp8: %s%s" % (mfma, same, "" if same else " (%d of %d logits differ, rel-L2 %.3g)"
                                                          % (int((b != q).sum()), b.numel(), rel_l2(b.cpu(), q.cpu()))))
    assert same
    assert torch.equal(run(m, x, "fp8"), q) and torch.equal(run(m, x, "fp8-block"), b), "switching back and forth"


_REFS = {}


def emptied(dev):
    """The globally pruned model and its CPU references at B = 1, computed once."""
    if not _REFS:
        blocks, m, masks = pruned(dev, 0, False)
        x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(6))
        state = {k: v.cpu() for k, v in m.state_dict().items()}
        cm = [k.cpu() for k in masks]
        with torch.no_grad():
            ref32 = O.forward(blocks, state, x, training=False, masks=cm)
            ref8 = R.forward(blocks, state, x, EXPECTED, masks=cm)
        _REFS.update(m=m, masks=masks, x=x, ref32=ref32, ref8=ref8)
    return _REFS


@pytest.mark.parametrize("mfma", [0, 1], ids=["f16mfma", "f8mfma"])
def test_emptied_layers_run_the_kernel(dev, setenv, mfma):
    """block_prune(75) over the whole model leaves conv19 / 20 / 22 one block each: "fp8" compacts their filters and loses them
    (and the blocks behind them) to the fp16 path; "fp8-block" with the default bound keeps them on the fp8 engine, on the
    block-sparse kernel.  e_engine <= 1.10 e_ref against the fp32 oracle, as test_q8_model_gpu.py holds "fp8" to."""
    setenv("MCAMD_Q8_MFMA", str(mfma))
    r = emptied(dev)
    m, x = r["m"], r["x"].to(dev)
    m.fp8_block_max_kept = E.Q8_BSPARSE_MAX_KEPT
    run(m, x, "fp8")
    lost = [c for c in EXPECTED if c not in engine_for(m, x, "fp8").fp8_layers]
    got = run(m, x, "fp8-block").cpu()
    eng = engine_for(m, x)
    print("fp8 loses %s; fp8-block runs %s on the kernel; kept %s"
          % (lost, eng.fp8_block_layers, " ".join("%d:%.4f" % kv for kv in sorted(eng.fp8_block_kept.items()))))
    assert {19, 20, 22} <= set(lost) and {19, 20, 22} <= set(eng.fp8_block_layers) and eng.fp8_layers == EXPECTED
    assert all(eng.fp8_block_kept[c] <= E.Q8_BSPARSE_MAX_KEPT for c in eng.fp8_block_layers)
    assert all(eng.fp8_block_kept[c] > E.Q8_BSPARSE_MAX_KEPT for c in EXPECTED if c not in eng.fp8_block_layers)
    e_engine, e_ref = rel_l2(got, r["ref32"]), rel_l2(r["ref8"], r["ref32"])
    print("MCAMD_Q8_MFMA=%d: engine %.4f, q8_ref %.4f against the fp32 oracle (ratio %.3f)" % (mfma, e_engine, e_ref, e_engine / e_ref))
    assert e_engine <= 1.10 * e_ref


def test_refusals_and_read_outs(dev):
    r = emptied(dev)
    m, masks, x = r["m"], r["masks"], r["x"].to(dev)
    q = run(m, x, "fp8")
    m.fp8_block_max_kept = 0.0
    z = run(m, x, "fp8-block")
    eng = engine_for(m, x)
    assert eng.fp8_block_layers == [] and eng.fp8_layers == engine_for(m, x, "fp8").fp8_layers
    assert torch.equal(z, q), "fp8_block_max_kept = 0.0 is not the fp8 engine bit for bit"
    # the read-out: every candidate's kept fraction, from the bytes -- here what the masks say (no kept block of a random-init
    # layer rounds to zero bytes as a whole)
    want = mask_fractions(masks)
    assert sorted(eng.fp8_block_kept) == EXPECTED == sorted(want)
    assert all(abs(eng.fp8_block_kept[c] - want[c]) < 1e-12 for c in EXPECTED), (eng.fp8_block_kept, want)
    m.fp8_block_max_kept = 1.0
    run(m, x, "fp8-block")
    assert eng.fp8_block_layers == EXPECTED
    m.fp8_block_max_kept = E.Q8_BSPARSE_MAX_KEPT
    # training-mode forward: as under "fp8"
    m.train()
    with pytest.raises(McamdError, match="inference only"):
        m(x)
    m.eval()
    # sparse = "block" belongs to the fp16 engine: both fp8 precisions refuse it and name the way out
    m.sparse = "block"
    try:
        for prec in ("fp8-block", "fp8"):
            m.precision = prec
            with torch.no_grad(), pytest.raises(McamdError) as ei:
                m(x)
            assert "'fp8-block'" in str(ei.value) and "model.sparse = None" in str(ei.value), str(ei.value)
    finally:
        m.sparse = None


def test_after_fp8_qat_steps_under_block_masks(dev):
    """The line prune -> "fp8-qat" fine-tune -> "fp8-block" on tests/golden/q8_qat.cfg: block_prune(50, per_layer=True) (no filter
    dies at seed 0), two SGD steps under "fp8-qat", then the eval forward under "fp8-block" with every candidate on the kernel
    is the eval forward under "fp8-qat" -- the "fp8" engine -- bit for bit."""
    cfg = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "q8_qat.cfg")
    m = nets.Darknet(cfg)
    m.load_state_dict(O.init_state(O.parse_cfg(cfg), seed=0))
    m.to(dev)
    masks = block_prune(m, 50.0, per_layer=True)
    m.set_masks(masks)
    assert all(bool((mk.reshape(mk.shape[0], -1).amax(1) != 0).all()) for mk in masks), "a filter died: pick another seed"
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(dev)
    m.precision = "fp8-qat"
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9)
    for _ in range(2):
        loss = (m(x).float() ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    m.eval()
    m.fp8_block_max_kept = 1.0
    q = run(m, x, "fp8-qat")
    b = run(m, x, "fp8-block")
    eng = engine_for(m, x)
    assert eng.fp8_layers == engine_for(m, x, "fp8-qat").fp8_layers == list(range(3, 11))
    assert eng.fp8_block_layers == list(range(3, 11)) and all(0.0 < v <= 0.75 for v in eng.fp8_block_kept.values()), eng.fp8_block_kept
    assert bool(torch.isfinite(b).all()) and torch.equal(b, q)


@pytest.mark.parametrize("entropy", [None, "huffman"], ids=["plain", "huffman"])
def test_fp8_file_round_trip(dev, tmp_path, entropy):
    """The "fp8" payload is the operand set: the same bytes and exponents, so the same lists and the same logits."""
    r = emptied(dev)
    m, x = r["m"], r["x"].to(dev)
    m.fp8_block_max_kept = E.Q8_BSPARSE_MAX_KEPT
    want = run(m, x, "fp8-block")
    eng = engine_for(m, x)
    path = str(tmp_path / "block.mcz")
    m.save_compressed(path, "fp8", layers=eng.fp8_layers, entropy=entropy)
    back = nets.Darknet(YOLOV2_VOC_CFG)
    back.to(dev)
    back.load_weights(path)
    back.eval()
    got = run(back, x, "fp8-block")
    e2 = engine_for(back, x)
    assert e2.fp8_layers == eng.fp8_layers and e2.fp8_block_layers == eng.fp8_block_layers and e2.fp8_block_kept == eng.fp8_block_kept
    assert torch.equal(got, want)


def test_warm_forward_allocates_nothing_and_detect(dev):
    r = emptied(dev)
    m = r["m"]
    m.fp8_block_max_kept = E.Q8_BSPARSE_MAX_KEPT
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(9)).to(dev)
    m.precision = "fp8-block"
    with torch.no_grad():
        m(x)
        m(x)
        torch.cuda.synchronize()
        before, stats0 = torch.cuda.memory_allocated(dev), torch.cuda.memory_stats(dev)
        m(x)
        torch.cuda.synchronize()
        after, stats1 = torch.cuda.memory_allocated(dev), torch.cuda.memory_stats(dev)
        logits = m(x)
    assert engine_for(m, x).fp8_block_layers
    assert after == before
    assert stats1["num_alloc_retries"] == stats0["num_alloc_retries"]
    assert stats1["segment.all.allocated"] == stats0["segment.all.allocated"]
    # (threshold 0: a random-init model keeps boxes; rows at or beyond nkept[b] are unspecified)
    got = m.detect(x, 0.0, 0.45)
    want = U.detections_device(logits, 0.0, 0.45, m.num_classes, m.anchors, m.num_anchors)
    assert len(got) == len(want) == 3 and torch.equal(got[2], want[2]) and int(got[2].min()) > 0
    for b, n in enumerate(got[2].cpu().tolist()):
        assert torch.equal(got[0][b, :n], want[0][b, :n]) and torch.equal(got[1][b, :n], want[1][b, :n])
