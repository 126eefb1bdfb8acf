"""lowrank.FactorSGD on the device (csrc/lowrank_train.hip): a training step of YOLOv2-VOC at 2 x 160 x 160 with
seven factored blocks leaves the factors fresh and the weights their product, the eval engine then runs the TRAINED factors,
a skipped step writes nothing, and train() with YOLOv2Train.LOWRANK ends with fresh factors."""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, lowrank, lowrank_factor, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd.train import YOLOv2Train  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402

RANKS = {9: 64, 10: 64, 11: 64, 12: 64, 13: 64, 15: 64, 21: 32}
MINI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini.cfg")
LR = 1e-3


def state(fs):
    return [t.detach().clone() for _, c in fs.blocks for t in (c.weight, c.factor_u, c.factor_v)] + \
           [t.clone() for t in fs.mu + fs.mv]


@functools.lru_cache(maxsize=None)
def stepped(dev):
    """(model, FactorSGD, input, factors before the step) behind one forward, backward, optimizer.step(), fs.step(LR)"""
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(O.parse_cfg(YOLOV2_VOC_CFG), seed=0))
    m.to(dev).train()
    m.precision = "fp16"
    m.set_factors(lowrank_factor(m, rank=RANKS))
    opt = torch.optim.SGD(m.parameters(), lr=LR, momentum=0.9, weight_decay=5e-4, fused=True)
    fs = lowrank.FactorSGD(m, momentum=0.9, weight_decay=5e-4)
    before = [(c.factor_u.clone(), c.factor_v.clone()) for _, c in fs.blocks]
    x = torch.rand(2, 3, 160, 160, generator=torch.Generator().manual_seed(3)).to(dev)
    m(x).float().pow(2).mean().backward()
    opt.step()
    fs.step(LR)
    return m, fs, x, before


def test_a_step_leaves_fresh_factors_and_their_product(dev):
    m, fs, _, before = stepped(dev)
    assert [i for i, _ in fs.blocks] == sorted(RANKS)
    for (i, c), (u0, v0) in zip(fs.blocks, before):
        assert lowrank.is_fresh(m, c), i
        r = c.factor_u.shape[0]
        u, v = c.factor_u.double().reshape(r, -1), c.factor_v.double()
        bound = (r + 2) * 2.0 ** -24 * (v.abs() @ u.abs())
        assert bool(((c.weight.detach().double().reshape(v.shape[0], -1) - v @ u).abs() <= bound).all()), i
        assert not torch.equal(c.factor_u, u0) and not torch.equal(c.factor_v, v0), i


def test_the_eval_engine_runs_the_trained_factors(dev):
    m, fs, x, _ = stepped(dev)
    m.eval()
    m.lowrank_max_cost, m.lowrank_min_tiles = 1.0, 1
    try:
        with torch.no_grad():
            m.lowrank = True
            on = m(x).clone()
            eng = [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and not e.train_layout][0]
            assert eng.lowrank_layers and eng.lowrank_stale == []
            m.lowrank = False
            off = m(x).clone()
    finally:
        m.lowrank = False
        m.train()
    ref = O.forward(O.parse_cfg(YOLOV2_VOC_CFG), {k: v.cpu() for k, v in m.state_dict().items() if "factor" not in k}, x.cpu(),
                    training=False)
    e_on, e_off = rel_l2(on.cpu(), ref), rel_l2(off.cpu(), ref)
    print("rel-L2 against the fp32 forward on the product weights: trained factors %.3e, dense fp16 %.3e" % (e_on, e_off))
    assert e_on <= 2 * e_off


def test_a_skipped_step_writes_nothing(dev):
    m, fs, _, _ = stepped(dev)
    before = state(fs)
    fs.step(LR, skip=torch.ones(1, device=dev))
    assert all(torch.equal(a, b) for a, b in zip(before, state(fs))) and fs.tables_built == 1
    assert all(lowrank.is_fresh(m, c) for _, c in fs.blocks)


def test_train_with_lowrank_ends_with_fresh_factors(dev):
    t = YOLOv2Train()
    t.LOWRANK = {"rank": 32}
    torch.manual_seed(0)
    m = t.train('', '', '', '', '', '', 'p_', MINI, '', 2, 10, MAX_EPOCHS=1, SYNTHETIC_SAMPLES=4)       # two steps at B = 2
    assert YOLOv2Train.LOWRANK is None and len(t.factor_sgd.blocks) >= 2
    for i, c in t.factor_sgd.blocks:
        assert lowrank.is_fresh(m, c) and c.factor_u.shape[0] == 32, i
        assert float(t.factor_sgd.mu[0].abs().max()) > 0
