"""mcamd_lowrank_sgd (csrc/lowrank_train.hip) through ops.LowRankSgdTable against a float64 restatement of
the header's formulas, stage by stage and element by element.  The bound is derived, not measured: a length-n fp32 dot
product in any order errs by at most (n + 2) 2^-24 (|A| |B|)[i, j]; the two fused multiply-adds behind it add one rounding
each of a value no larger than the sum of their terms' magnitudes."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402

EPS = 2.0 ** -24
LR, MOM, WD = np.float32(1e-2), np.float32(0.9), np.float32(5e-4)
NAMES = ("u", "v", "mu", "mv", "w")


def cases():
    S = ops.lowrank_sgd_info(64, 64, 32).slice
    cin = -(-(2 * S + 32) // (9 * 32)) * 32                # the smallest Cin % 32 == 0 whose 9 Cin reaches 2 S + 32
    return [(96, 32, 3, 32), (128, 64, 3, 256), (64, 64, 1, 96), (64, cin, 3, 64)]


def operands(case, dev, seed):
    cout, cin, k, r = case
    g = torch.Generator().manual_seed(seed)
    shapes = dict(g=(cout, cin, k, k), u=(r, cin, k, k), v=(cout, r), w=(cout, cin, k, k))
    it = {n: torch.randn(s, generator=g).to(dev) for n, s in shapes.items()}
    it["mu"], it["mv"] = torch.zeros_like(it["u"]), torch.zeros_like(it["v"])
    return it


def snap(items):
    return [{n: t.detach().cpu().clone() for n, t in it.items()} for it in items]


@functools.lru_cache(maxsize=None)
def grouped(dev):
    """All four blocks in ONE table, two steps: the states before, between and after."""
    items = [operands(c, dev, 10 + i) for i, c in enumerate(cases())]
    table = ops.LowRankSgdTable(items)
    states = [snap(items)]
    for _ in range(2):
        table.step(LR, MOM, WD)
        states.append(snap(items))
    return states


def check_step(old, new, what):
    """`new` against the header's formulas applied to `old`."""
    d = {n: t.double().reshape(t.shape[0], -1) for n, t in old.items()}
    k = {n: t.double().reshape(t.shape[0], -1) for n, t in new.items()}
    cout, K = d["g"].shape
    lr, mom, wd = float(LR), float(MOM), float(WD)
    for m, x, prod, mag, n in (("mu", "u", d["v"].t() @ d["g"], d["v"].abs().t() @ d["g"].abs(), cout),
                               ("mv", "v", d["g"] @ d["u"].t(), d["g"].abs() @ d["u"].abs().t(), K)):
        ref = mom * d[m] + prod + wd * d[x]
        bound = (n + 2) * EPS * mag + 2 * EPS * (mag + (wd * d[x]).abs() + (mom * d[m]).abs())
        excess = ((k[m] - ref).abs() - bound).max().item()
        print("%s %s: largest |error| - bound %.3e" % (what, m, excess))
        assert excess <= 0, (what, m)
        once = torch.addcmul(d[x], k[m], torch.tensor(-lr, dtype=torch.float64)).float()      # fmaf(-lr, M, old): one rounding
        assert torch.equal(new[x].reshape(once.shape), once), (what, x)
    r = d["u"].shape[0]
    excess = ((k["w"] - k["v"] @ k["u"]).abs() - (r + 2) * EPS * (k["v"].abs() @ k["u"].abs())).max().item()
    print("%s w: largest |error| - bound %.3e" % (what, excess))
    assert excess <= 0, (what, "w")


@pytest.mark.parametrize("ci", range(4))
def test_one_block_alone(dev, ci):
    it = operands(cases()[ci], dev, 10 + ci)
    old = snap([it])[0]
    ops.LowRankSgdTable([it]).step(LR, MOM, WD)
    new = snap([it])[0]
    check_step(old, new, "alone %r" % (cases()[ci],))
    # the grouped tile map computes what the block's own table computes, bit for bit
    assert all(torch.equal(new[n], grouped(dev)[1][ci][n]) for n in NAMES)


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("ci", range(4))
def test_grouped_table_and_second_step(dev, ci, step):
    states = grouped(dev)
    assert step == 1 or float(states[1][ci]["mu"].abs().max()) > 0          # momentum comes in non-zero
    check_step(states[step - 1][ci], states[step][ci], "grouped step %d %r" % (step, cases()[ci]))


def test_skip_writes_nothing_and_runs_are_bit_equal(dev):
    runs = []
    for _ in range(2):
        items = [operands(c, dev, 10 + i) for i, c in enumerate(cases())]
        table, before = ops.LowRankSgdTable(items), snap(items)
        table.step(LR, MOM, WD, skip=torch.ones(1, device=dev))
        assert all(torch.equal(a[n], b[n]) for a, b in zip(before, snap(items)) for n in NAMES)
        table.step(LR, MOM, WD, skip=torch.zeros(1, device=dev))
        runs.append(snap(items))
    assert all(torch.equal(a[n], b[n]) for a, b in zip(*runs) for n in NAMES)
    assert all(torch.equal(a[n], b[n]) for a, b in zip(runs[0], grouped(dev)[1]) for n in NAMES)


@pytest.mark.parametrize("case,word", [((64, 64, 1, 48), "rank r"), ((320, 64, 1, 288), "rank r"), ((40, 64, 1, 32), "Cout")])
def test_refusals_by_name(dev, case, word):
    with pytest.raises(McamdError, match=word):
        ops.LowRankSgdTable([operands(case, dev, 0)])
