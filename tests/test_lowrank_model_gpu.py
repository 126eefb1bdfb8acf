"""Darknet.lowrank: factored blocks of YOLOv2-VOC on the fused two-GEMM kernel (csrc/conv_lowrank.hip) -- the
factors tie the weights, which blocks leave the dense launch, the error level, the off settings, staleness and the rules.
Seven blocks are factored: plain destinations, conv13's pool + full-resolution copy and conv21's reorg."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, lowrank_factor, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402

RANKS = {9: 64, 10: 64, 11: 64, 12: 64, 13: 64, 15: 64, 21: 32}


def fresh_model(dev, factored=True):
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(blocks, seed=0))
    m.to(dev).eval()
    m.precision = "fp16"
    if factored:
        m.set_factors(lowrank_factor(m, rank=RANKS))
        m.lowrank_max_cost, m.lowrank_min_tiles = 1.0, 1
    return m


@functools.lru_cache(maxsize=None)
def shared(dev):
    """(factored model, input, logits with lowrank off, logits with it on)"""
    m = fresh_model(dev)
    x = torch.rand(2, 3, 160, 160, generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        off = m(x).clone()
        m.lowrank = True
        on = m(x).clone()
    return m, x, off, on


def engine_for(m, x):
    return [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and not e.train_layout][0]


def convs(m):
    return [blk[0] for blk, b in zip(m.models, m.blocks[1:]) if b["type"] == "convolutional"]


def test_factors_tie_the_weights(dev):
    plain, m = fresh_model(dev, factored=False), shared(dev)[0]
    assert not any("factor" in k for k in plain.state_dict())
    for n, (a, b) in enumerate(zip(convs(plain), convs(m)), 1):
        if n in RANKS:
            r = b.factor_u.shape[0]
            assert r == RANKS[n] and torch.equal(b.weight.data, (b.factor_v @ b.factor_u.reshape(r, -1)).reshape(b.weight.shape))
        else:
            assert torch.equal(a.weight.data, b.weight.data) and getattr(b, "factor_u", None) is None
    masked = fresh_model(dev, factored=False)
    masked.set_masks([torch.ones_like(c.weight) for c in convs(masked)])
    with pytest.raises(McamdError, match="conv9"):
        masked.set_factors(lowrank_factor(masked, rank={9: 64}))


def test_chosen_blocks_error_level_and_off_settings(dev):
    m, x, off, on = shared(dev)
    eng = engine_for(m, x)
    assert eng.lowrank_layers == sorted(RANKS) and eng.lowrank_ranks == RANKS and eng.lowrank_stale == []
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    ref = O.forward(blocks, {k: v.cpu() for k, v in m.state_dict().items() if "factor" not in k}, x.cpu(), training=False)
    e_on, e_off = rel_l2(on.cpu(), ref), rel_l2(off.cpu(), ref)
    print("rel-L2 against the fp32 forward: lowrank %.3e, dense fp16 %.3e" % (e_on, e_off))
    assert e_on <= 2 * e_off
    never = fresh_model(dev, factored=False)
    for a, b in zip(convs(never), convs(m)):
        a.weight.data.copy_(b.weight.data)
    never.invalidate_packed()
    with torch.no_grad():
        base = never(x)
        assert torch.equal(off, base)
        m.lowrank_max_cost = 0.0
        assert torch.equal(m(x), base) and engine_for(m, x).lowrank_layers == []
        m.lowrank_max_cost = 1.0
        assert torch.equal(m(x), on) and engine_for(m, x).lowrank_layers == sorted(RANKS)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats(dev)
        m(x)
        torch.cuda.synchronize()
        after = torch.cuda.memory_stats(dev)
    assert after["segment.all.allocated"] == before["segment.all.allocated"] and after["num_alloc_retries"] == before["num_alloc_retries"]


def test_staleness_and_rules(dev):
    m = fresh_model(dev)
    x = shared(dev)[1]
    m.lowrank = True
    with torch.no_grad():
        m(x)
        convs(m)[9].weight.mul_(1.01)            # conv10, in place: its factors no longer describe it
        stale = m(x).clone()
        eng = engine_for(m, x)
        assert eng.lowrank_stale == [10] and eng.lowrank_layers == sorted(set(RANKS) - {10})
        for c in convs(m):                       # every factored block stale: the dense engine on the current weights
            c.weight.mul_(1.0)
        allstale = m(x).clone()
        assert eng.lowrank_layers == [] and eng.lowrank_stale == sorted(RANKS)
        m.lowrank = False
        assert torch.equal(m(x), allstale) and not torch.equal(stale, allstale)
    m.lowrank = True
    for kw, words in ((dict(precision="fp8"), ("lowrank", "fp8")), (dict(splitk=True), ("lowrank", "splitk")),
                      (dict(sparse="block"), ("lowrank", "sparse"))):
        old = {k: getattr(m, k) for k in kw}
        for k, v in kw.items():
            setattr(m, k, v)
        with pytest.raises(McamdError) as err, torch.no_grad():
            m(x)
        assert all(w in str(err.value) for w in words)
        for k, v in old.items():
            setattr(m, k, v)
    m.train()                                    # training ignores the switch
    m(x)
    assert [e for e in m._engines.values() if e.train_layout][0].lowrank_layers == []


def test_decision_rule_at_its_boundaries(dev):
    """r (K + Cout) <= max_cost K Cout and mtiles >= min_tiles, each at its boundary: conv9 (10 x 10 at this input, 4 tiles) is
    chosen at lowrank_min_tiles = 4 and left dense at 5; conv13 is chosen at its own ratio times (1 + 1e-6) and left dense at
    (1 - 1e-6) -- every other block follows the same inequality -- and the blocks a rule leaves dense run the dense launch:
    the logits equal those of a model that carries the same weights and factors for the chosen blocks only."""
    from modelcompression_amd import ops
    m, x, off, on = shared(dev)
    cs = convs(m)
    K = {n: cs[n - 1].weight[0].numel() for n in RANKS}
    cout = {n: cs[n - 1].weight.shape[0] for n in RANKS}
    ratio = {n: RANKS[n] * (K[n] + cout[n]) / (K[n] * cout[n]) for n in RANKS}

    def mtiles(n):
        lay = [lay for lay in engine_for(m, x).layers if lay.li + 1 == n][0]
        return ops.conv_fwd_lowrank_info(lay.geom_act, RANKS[n]).mtiles

    def run(max_cost, min_tiles):
        m.lowrank_max_cost, m.lowrank_min_tiles = max_cost, min_tiles
        with torch.no_grad():
            y = m(x).clone()
        return y, engine_for(m, x).lowrank_layers

    def only(chosen):
        """the logits of a model with m's weights whose factors cover `chosen` alone, every one of them forced on"""
        p = fresh_model(dev, factored=False)
        for a, b in zip(convs(p), cs):
            a.weight.data.copy_(b.weight.data)
        p.set_factors([(b.factor_u, b.factor_v) if n in chosen else None for n, b in enumerate(cs, 1)])
        assert all(torch.equal(a.weight.data, b.weight.data) for a, b in zip(convs(p), cs))
        p.lowrank, p.lowrank_max_cost, p.lowrank_min_tiles = True, 1.0, 1
        with torch.no_grad():
            y = p(x).clone()
        assert engine_for(p, x).lowrank_layers == sorted(chosen)
        return y

    try:
        tiles = {n: mtiles(n) for n in RANKS}
        assert tiles[9] == 2 * 10 * 10 // 64 + 1 and tiles[15] < tiles[9]
        y, chosen = run(1.0, tiles[9])
        assert 9 in chosen and chosen == [n for n in sorted(RANKS) if tiles[n] >= tiles[9]] and chosen != sorted(RANKS)
        assert torch.equal(y, only(chosen))
        y, chosen = run(1.0, tiles[9] + 1)
        assert 9 not in chosen and chosen == [n for n in sorted(RANKS) if tiles[n] >= tiles[9] + 1]
        assert chosen or torch.equal(y, off)
        for sign, inside in ((1.0, True), (-1.0, False)):
            cost = ratio[13] * (1.0 + sign * 1e-6)
            y, chosen = run(cost, 1)
            assert (13 in chosen) == inside
            assert chosen == [n for n in sorted(RANKS) if RANKS[n] * (K[n] + cout[n]) <= cost * K[n] * cout[n]]
            if inside:
                assert 0 < len(chosen) < len(RANKS) and torch.equal(y, only(chosen))
            else:
                assert not any(abs(ratio[n] - ratio[13]) < 1e-9 for n in chosen)
                assert chosen or torch.equal(y, off)
    finally:
        m.lowrank_max_cost, m.lowrank_min_tiles = 1.0, 1
    with torch.no_grad():
        assert torch.equal(m(x), on)
