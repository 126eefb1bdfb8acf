"""Factor SGD without a device (lowrank.FactorSGD, csrc/lowrank_train.hip's C surface): the symbols, the torch
restatement against the float64 closed form, and the refusals of FactorSGD and of YOLOv2Train.LOWRANK."""
import os
import re

import pytest
import torch

from modelcompression_amd import _lib, lowrank, lowrank_factor, nets, ops
from modelcompression_amd._lib import McamdError
from modelcompression_amd.synthetic import init_synthetic
from modelcompression_amd.train import YOLOv2Train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "golden", "mini.cfg")
NAMES = ("mcamd_lowrank_sgd_ok", "mcamd_lowrank_sgd_info", "mcamd_lowrank_sgd")


def factored(rank=32):
    m = init_synthetic(nets.Darknet(MINI), seed=0)
    m.set_factors(lowrank_factor(m, rank=rank))
    return m


def test_the_names_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, hdr) and n in _lib.SIGNATURES and hasattr(_lib.lib(), n)
    assert "typedef struct mcamd_lrsgd_seg" in hdr and callable(ops.LowRankSgdTable.step)
    info = ops.lowrank_sgd_info(1024, 4608, 128)
    assert info.slice == int(re.search(r"#define MCAMD_LRSGD_SLICE (\d+)", hdr).group(1))
    assert info.slices == -(-4608 // info.slice) and info.workspace_bytes == info.slices * 1024 * 128 * 4
    assert _lib.lib().mcamd_lowrank_sgd_ok(96, 288, 96) == 1 and _lib.lib().mcamd_lowrank_sgd_ok(96, 288, 48) == 0


def test_cpu_step_is_the_closed_form_and_stays_fresh():
    m = factored()
    fs = lowrank.FactorSGD(m, momentum=0.9, weight_decay=5e-4)
    assert len(fs.blocks) >= 2
    gen = torch.Generator().manual_seed(1)
    for _, c in fs.blocks:
        c.weight.grad = torch.randn(c.weight.shape, generator=gen)
    lr, old = 1e-2, [(c.factor_u.double().clone(), c.factor_v.double().clone()) for _, c in fs.blocks]
    fs.step(lr)
    for (i, c), (u4, v) in zip(fs.blocks, old):
        u, g = u4.reshape(u4.shape[0], -1), c.weight.grad.double().reshape(v.shape[0], -1)
        un, vn = u - lr * (v.t() @ g + 5e-4 * u), v - lr * (g @ u.t() + 5e-4 * v)        # zero buffers: M = g
        n = max(g.shape)
        for got, ref, mag in ((c.factor_u.double().reshape(un.shape), un, u.abs() + lr * (v.abs().t() @ g.abs())),
                              (c.factor_v.double(), vn, v.abs() + lr * (g.abs() @ u.abs().t()))):
            assert bool(((got - ref).abs() <= (n + 4) * 2.0 ** -24 * mag).all()), i
        assert lowrank.is_fresh(m, c)
        w = (c.factor_v @ c.factor_u.reshape(u.shape)).reshape(c.weight.shape)
        assert torch.equal(c.weight.detach(), w)


def test_factor_sgd_refusals():
    with pytest.raises(McamdError, match="no fresh factored block"):
        lowrank.FactorSGD(init_synthetic(nets.Darknet(MINI), seed=0))
    with pytest.raises(McamdError, match=r"conv\d+: lowrank_sgd: rank r must be a multiple of 32"):
        lowrank.FactorSGD(factored(rank=16))


@pytest.mark.parametrize("attr,kwargs,word", [(None, dict(pruning_perc=10.), "pruning_perc"), ("SHARE", {}, "SHARE"),
                                              ("GROUP_LASSO", {}, "GROUP_LASSO")])
def test_train_refuses_lowrank_with_masks_or_codebooks(attr, kwargs, word):
    t = YOLOv2Train()
    t.LOWRANK = {"rank": 32}
    if attr is not None:
        setattr(t, attr, 4 if attr == "SHARE" else {"lam": 1.0, "granularity": "block"})
    with pytest.raises(ValueError, match="LOWRANK and %s" % word):
        t.train('', '', '', '', '', '', 'p_', MINI, '', 2, 10, MAX_EPOCHS=1, SYNTHETIC_SAMPLES=2, **kwargs)
    t.LOWRANK = {"rank": 32, "energy": 0.5}
    with pytest.raises(ValueError, match="LOWRANK must be None or a dict"):
        t.train('', '', '', '', '', '', 'p_', MINI, '', 2, 10, MAX_EPOCHS=1, SYNTHETIC_SAMPLES=2)
