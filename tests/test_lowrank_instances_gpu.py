"""All four lowrank_kernel<R> instances mcamd_conv_fwd_lowrank can launch (csrc/conv_lowrank.hip, the fused two-GEMM forward
behind Darknet.lowrank), against an EXACT reference, with the method of test_splitk_instances_gpu.py.

The operands hold small integers; while max|x| max|U| Ktot and max|H| max|V| r stay below 2^24 every partial sum of either
GEMM in any order is a number fp32 holds, the intermediate is rounded (and saturated) to fp16 the way the reference rounds
it, and the epilogue (scales 1/4 .. 2, shifts in steps of 1/4, slope 1/8) is exact up to the final rounding to fp16, which
the float64 reference performs on the exact value.  The result must EQUAL the reference: a K chunk of either phase that is
lost, doubled or decoded to the wrong (block, tap, sub-chunk), an H column the hand-over lays into the wrong chunk or piece,
a ring item of phase 2 read before it landed or a wrong row of a pooled tile that spans two images is off by at least one
unit (test_lowrank_cases_cpu.py proves that every chunk of either phase is visible in every tile).  There is no tolerance in
this file.

tests/lowrank_cases.py holds the cases; test_lowrank_cases_cpu.py proves without a GPU that they reach every instance with
its padded and its unpadded rank, both kernel sizes, both K orders (32 and 64 channels per block), every destination form and
every boundary condition.  Channels outside the operand slice hold NaN, the slice beyond the real channels and the halo hold
zero; every output starts as NaN everywhere, halo and guard bands included, and must stay so outside the interior of its
slice.
MEASURED (MI355X): 0 of 1 199 960 elements differ over the 62 compared outputs of all launches of this file (28 cases and their
re-runs in test_saturation and test_no_history, 18 one-hot batches); every flag as expected."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lowrank_cases as LR  # noqa: E402
from test_lowrank_kernels_gpu import launch  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_equal(c, what, got, want):
    """got, want fp16 [B][n][h][w]: the bit patterns must be the reference's (NaN, an unwritten or polluted element,
    compares unequal)."""
    assert got.dtype == want.dtype == torch.float16 and got.shape == want.shape, (c.name, what, got.dtype, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    print("%s %s: %d of %d elements differ" % (c.name, what, int(bad.sum()), bad.numel()))
    if not bool(bad.any()):
        return
    first = tuple(bad.nonzero()[0].tolist())
    raise AssertionError("%s (lowrank_kernel<%d>, rank %d, %d x %d tiles): %d of %d elements of %s differ from the exact result; "
                         "first (image, channel, y, x) %s, got %r want %r; %d sentinels among them"
                         % ((c.name,) + c.expect[:1] + (c.r,) + c.expect[1:3] + (int(bad.sum()), bad.numel(), what, list(first),
                            float(got[first]), float(want[first]), int((torch.isnan(got) & bad).sum()))))


def _run(dev, c, overflow=True):
    """One launch of a case of the table: info as expected, y (and y2) equal to the reference, sentinels kept; the flag"""
    assert LR.expect_of(LR.info_of(c)) == c.expect, c.name
    want = LR.reference_of(c.name)[0]
    outs, flag = launch(dev, LR.operands(c.name), overflow=overflow)
    assert len(outs) == len(want)
    for what, (got, rest), w in zip(("y", "y2"), outs, want):
        _assert_equal(c, what, got, w)
        assert bool(torch.isnan(rest).all()), "%s: %d elements of %s outside the slice were written" % (c.name, int((~torch.isnan(rest)).sum()), what)
    return flag


@pytest.mark.parametrize("c", LR.LOWRANK_CASES, ids=str)
def test_instance_exact(dev, c):
    flag = _run(dev, c)
    assert flag == int(LR.reference_of(c.name)[2]), "the overflow flag must be set exactly when an intermediate or an output was clamped"


@pytest.mark.parametrize("h", LR.ONEHOT_CASES, ids=LR.onehot_id)
def test_onehot(dev, h):
    """Every filter of U keeps ONE weight at its own (channel, tap) and between them the filters select every k of the packed
    order that holds a real channel; every activation value is distinct; V is the identity.  The output of filter f at the
    centre pixel must be the value at f's (channel, tap): which k each operand lane of phase 1 selects and where the
    hand-over puts each H column, with no sum in the way."""
    x, u, which, batches = LR.onehot_operands(h)
    for b in batches:
        (got, rest), = launch(dev, b)[0]
        n = min(256, len(which) - b.f0)
        want = [9 * chan + (tap if h.k == 3 else 4) + 1 for chan, tap in which[b.f0:b.f0 + n]] + [0] * (b.r - n)
        bad = [(b.f0 + f, which[b.f0 + f] if f < n else None, float(got[0, f, 1, 1]), want[f]) for f in range(b.r)
               if not float(got[0, f, 1, 1]) == want[f]]
        assert not bad, "%s: %d of %d filters select the wrong k; first (filter, (channel, tap), got, want): %s" % (b.name, len(bad), b.r, bad[:8])
        _assert_equal(b.case, "y", got, LR.reference(b)[0])
        assert bool(torch.isnan(rest).all())


def test_saturation(dev):
    """The three planted cases and their twins with the flag cleared before each launch: set by a clamped H alone, by a
    clamped output alone and by both; 0 for every twin; and a launch without a flag simply runs, with the same clamped result."""
    planted = [c for c in LR.LOWRANK_CASES if c.plant and not c.twin]
    assert sorted(c.plant for c in planted) == ["both", "h", "y"]
    for c in planted:
        assert LR.reference_of(c.name)[2] and _run(dev, c) == 1, "%s: a value was clamped to +-65504: the overflow flag must be set" % c.name
        assert _run(dev, LR.BY_NAME[c.name + ".twin"]) == 0, "%s: nothing was clamped: the overflow flag must stay 0" % c.name
    assert _run(dev, planted[0], overflow=False) is None


def test_no_history(dev):
    """The H tile and the ring are not cleared between launches: after a rank-256 launch with H in the thousands a rank-32
    and a rank-160 launch (kc2 = 1 and 5 of their instances' 2 and 6 chunks) must still equal the reference, which is what a
    process's first launch of the same case gives (test_instance_exact)."""
    big = LR.BY_NAME[LR.NO_HISTORY[0]]
    for name in LR.NO_HISTORY[1:]:
        assert _run(dev, big) == 0
        assert _run(dev, LR.BY_NAME[name]) == 0


@pytest.mark.parametrize("name", LR.DETERMINISM_CASES)
def test_deterministic(dev, name):
    """Gaussian operands (sums that DO depend on the order) and two launches into fresh buffers: bit-equal, no sentinel left
    inside a slice and none lost outside."""
    o = LR.gaussian(LR.BY_NAME[name])
    a, b = launch(dev, o)[0], launch(dev, o)[0]
    for (ga, ra), (gb, _) in zip(a, b):
        assert not bool(torch.isnan(ga).any()) and torch.equal(_bits(ga), _bits(gb)) and bool(torch.isnan(ra).all())
