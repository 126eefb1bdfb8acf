"""Darknet.splitk = True: the low-batch mode of the plain-fp16 inference engine on a synthetic-init YOLOv2-VOC at 416x416 --
which blocks split at B = 1, accuracy against the fp32 oracle next to the unsplit engine's, plan replay, a batch the policy
leaves alone, a slim_export model (raw path), the 2:4 engine beside it, the precision / mode rules and model.detect."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, slim, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import nm_prune, quick_filter_prune  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402


def engine_for(m, x):
    """The plain-fp16 inference engine of this input shape (other precisions' engines of the same model live beside it)."""
    return [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and not e.train_layout and e.precision == "fp16"][0]


@functools.lru_cache(maxsize=None)
def dense(dev):
    """The model in eval / fp16, one image, the fp32 oracle's logits and today's engine's."""
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(blocks, seed=0))
    m.to(dev).eval()
    m.precision = "fp16"
    x1 = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref1 = O.forward(blocks, {k: v.cpu() for k, v in m.state_dict().items()}, x1, training=False)
        m.splitk = False
        off = m(x1.to(dev)).clone()
    return m, x1.to(dev), ref1, off


def test_splitk_b1_layers_accuracy_and_plan_replay(dev):
    m, x, ref1, off = dense(dev)
    try:
        with torch.no_grad():
            m.splitk = True
            on = m(x).clone()
            eng = engine_for(m, x)
            assert set(eng.splitk_layers) >= {14, 16, 18, 19, 20, 22}, eng.splitk_layers
            assert 1 not in eng.splitk_layers and 23 not in eng.splitk_layers
            assert bool(torch.isfinite(on).all())
            e_on, e_off = rel_l2(on.cpu(), ref1), rel_l2(off.cpu(), ref1)
            print("B=1 logits vs fp32 oracle: splitk %.3e, unsplit %.3e; split layers %s" % (e_on, e_off, eng.splitk_layers))
            assert e_on <= 1.1 * e_off
            assert torch.equal(m(x), on), "the replayed plan differs from the recorded forward"
            m.splitk = False
            assert torch.equal(m(x), off) and engine_for(m, x).splitk_layers == []
            m.splitk = True
            assert torch.equal(m(x), on)
    finally:
        m.splitk = False


def test_splitk_leaves_a_large_batch_alone(dev):
    m, _, _, _ = dense(dev)
    x = torch.rand(32, 3, 416, 416, generator=torch.Generator().manual_seed(5)).to(dev)
    try:
        with torch.no_grad():
            m.splitk = False
            off = m(x).clone()
            m.splitk = True
            on = m(x)
            assert engine_for(m, x).splitk_layers == []
            assert torch.equal(on, off)
    finally:
        m.splitk = False


def test_splitk_slim_model(dev, tmp_path):
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(blocks, seed=0))
    m.to(dev)
    masks = quick_filter_prune(m, 60.0)
    m.set_masks(masks)
    m.eval()
    s = slim.slim_export(m, str(tmp_path / "slim.cfg"))
    s.precision = "fp16"
    x1 = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref1 = O.forward(blocks, {k: v.cpu() for k, v in m.state_dict().items()}, x1, training=False,
                         masks=[k.cpu() for k in masks])
        off = s(x1.to(dev)).clone()
        s.splitk = True
        on = s(x1.to(dev)).clone()
        eng = engine_for(s, x1)
        split = [lay for lay in eng.layers if lay.sk_on]
        assert split, "no block of the slim model splits"
        assert any(not eng._fused_eval(lay) for lay in split), "no split block on the raw path"
        e_on, e_off = rel_l2(on.cpu(), ref1), rel_l2(off.cpu(), ref1)
        print("slim60 B=1 vs masked-dense fp32 oracle: splitk %.3e, unsplit %.3e; split layers %s (raw path: %s)"
              % (e_on, e_off, eng.splitk_layers, [lay.li + 1 for lay in split if not eng._fused_eval(lay)]))
        assert bool(torch.isfinite(on).all()) and e_on <= 1.1 * e_off
        assert torch.equal(s(x1.to(dev)), on)


def test_splitk_beside_sparse24(dev):
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(blocks, seed=0))
    m.to(dev)
    m.set_masks(nm_prune(m))
    m.eval()
    m.precision = "fp16"
    m.sparse, m.splitk = "2:4", True
    x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        out = m(x)
    eng = engine_for(m, x)
    assert eng.sparse_layers and set(eng.sparse_layers) & set(eng.splitk_layers) == set()
    assert bool(torch.isfinite(out).all())


def test_splitk_precision_and_mode_rules(dev):
    m, x, _, _ = dense(dev)
    try:
        m.splitk = True
        for prec in ("mixed", "fp8"):
            m.precision = prec
            with torch.no_grad(), pytest.raises(McamdError, match="splitk"):
                m(x)
        m.precision = "fp16"
        # a training-mode forward ignores the flag
        xt = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(6)).to(dev)
        outs = []
        for flag in (False, True):
            m.splitk = flag
            m.load_state_dict(O.init_state(O.parse_cfg(YOLOV2_VOC_CFG), seed=0))      # (the same running statistics)
            m.train()
            with torch.no_grad():
                outs.append(m(xt).clone())
        assert torch.equal(outs[0], outs[1])
    finally:
        m.splitk = False
        m.precision = "fp16"
        m.load_state_dict(O.init_state(O.parse_cfg(YOLOV2_VOC_CFG), seed=0))
        m.eval()


def test_splitk_detect_shapes(dev):
    m, x, _, _ = dense(dev)
    try:
        m.splitk = False
        base = m.detect(x)
        m.splitk = True
        got = m.detect(x)
        assert engine_for(m, x).splitk_layers
        assert [(t.shape, t.dtype) for t in got] == [(t.shape, t.dtype) for t in base]
    finally:
        m.splitk = False
