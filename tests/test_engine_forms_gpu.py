"""An engine's state does not depend on the order in which options and masks were applied (Engine._choose_forms): one model is
driven through a sequence of states on the SAME engine object, and at each state a freshly constructed model with the same
weights, masks and options does one forward -- the per-form layer lists, the recorded plan's launch count and the logits (bit
for bit) must agree, and the lists must equal what the engine's rules give for tests/golden/q8_qat.cfg at 64x64, B = 2.

Host-only facts for these shapes (mcamd_conv_fwd_*_ok, mcamd_conv_fwd_splitk_info): every non-dense fp16 form accepts
conv2 .. conv10, the fp8 forms conv3 .. conv10; the split-K policy gives conv8 two slices and conv10 three and splits nothing
else -- also not conv5 with 64 of its 128 filters compacted away nor conv6 behind it with the dead inputs folded."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import nm_prune, weight_prune  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402

CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "q8_qat.cfg")
FORMS = ("dense", "splitk", "sparse24", "bsparse", "q8", "q8_slim", "q8_sparse24")
LISTS = ("sparse_layers", "bsparse_layers", "splitk_layers", "fp8_layers", "fp8_sparse_layers")
NM = [2, 3, 4, 5, 6, 7, 9]          # conv numbers that get a 2:4 mask; conv8 and conv10 a magnitude mask that does not conform
ALL = list(range(2, 11))


def convs_of(m):
    return [mod[0] for mod in m.models if isinstance(mod, torch.nn.Sequential) and hasattr(mod[0], "mask_flag")]


def model(dev, prec):
    m = nets.Darknet(CFG)
    m.load_state_dict(O.init_state(O.parse_cfg(CFG), seed=0))
    m.to(dev).eval()
    m.precision = prec
    return m


def image(dev):
    return torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(11)).to(dev)


def masks_24(m, conforming=NM):
    """One mask per conv: 2:4 (nm_prune) on `conforming`, a 60 % magnitude mask elsewhere in conv2 .. conv10, ones on the
    first and the last block."""
    nm, mag = nm_prune(m), weight_prune(m, 60.0)
    out = [torch.ones_like(k) for k in nm]
    for n in ALL:
        out[n - 1] = (nm if n in conforming else mag)[n - 1].clone()
    return out


def with_dead_filters(masks, conv, keep):
    """The same masks with all but the first `keep` filters of block `conv` removed."""
    out = [k.clone() for k in masks]
    out[conv - 1][keep:] = 0
    return out


def fresh_like(hist, dev):
    """A newly constructed model with the weights, statistics, masks and options `hist` has now."""
    m = nets.Darknet(CFG)
    m.load_state_dict({k: v for k, v in hist.state_dict().items() if not k.endswith(".mask")})
    m.to(dev).eval()
    if any(c.mask_flag for c in convs_of(hist)):
        assert all(c.mask_flag for c in convs_of(hist))
        m.set_masks([c.mask.clone() for c in convs_of(hist)])
    m.precision, m.sparse, m.sparse_max_kept, m.splitk = hist.precision, hist.sparse, hist.sparse_max_kept, hist.splitk
    return m


def eval_engine(m):
    return [e for e in m._engines.values() if not e.train_layout][0]


def compare(hist, dev, x, what, expect=None):
    """One forward of `hist` and of a fresh copy: same lists (= `expect` where given), same launch count, same bits."""
    with torch.no_grad():
        out = hist(x).clone()
        new = fresh_like(hist, dev)
        ref = new(x)
    eng, eng2 = eval_engine(hist), eval_engine(new)
    print(what, {k: getattr(eng, k) for k in LISTS})
    for k in LISTS:
        assert getattr(eng, k) == getattr(eng2, k), (what, k, getattr(eng, k), getattr(eng2, k))
        if expect is not None:
            assert getattr(eng, k) == expect.get(k, []), (what, k, getattr(eng, k))
    assert sorted(eng.bsparse_kept) == sorted(eng2.bsparse_kept), what
    for lay, lay2 in zip(eng.layers, eng2.layers):
        assert lay.form in FORMS and lay.form == lay2.form, (what, lay.li + 1, lay.form, lay2.form)
        assert [lay.sp_on, lay.bs_on, lay.sk_on, lay.q8_on].count(True) == (lay.form != "dense"), (what, lay.li + 1)
        assert (lay.sk_slices, lay.q8_y, lay.q8_y2, lay.xq is None) == (lay2.sk_slices, lay2.q8_y, lay2.q8_y2, lay2.xq is None), \
            (what, lay.li + 1)
    assert eng._fwd_plans[False].launches == eng2._fwd_plans[False].launches, what
    assert torch.equal(out, ref), what + ": logits differ from a fresh engine's"
    return eng


def test_fp16_forms_do_not_depend_on_history(dev):
    m, x = model(dev, "fp16"), image(dev)
    base = masks_24(m)
    m.set_masks(base)

    def state(what, sparse, splitk, expect, max_kept=None):
        m.sparse, m.splitk = sparse, splitk
        if max_kept is not None:
            m.sparse_max_kept = max_kept
        return compare(m, dev, x, what, expect)
    first = state("1 dense", None, False, {})
    state("2 2:4", "2:4", False, dict(sparse_layers=NM))
    eng = state("3 2:4 + splitk", "2:4", True, dict(sparse_layers=NM, splitk_layers=[8, 10]))
    assert eng is first, "the sequence must run on one engine object"
    assert len({lay.form for lay in eng.layers}) == 3          # dense (first / last), sparse24, splitk in one forward
    assert [eng.layers[n - 1].sk_slices for n in (8, 10)] == [2, 3]
    # every masked block is a candidate and max_kept = 1 takes them all: nothing is left for split-K
    state("4 block + splitk", "block", True, dict(bsparse_layers=ALL), max_kept=1.0)
    state("5 splitk", None, True, dict(splitk_layers=[8, 10]))
    # 64 of conv5's 128 filters removed: conv5 is compacted (its POOL epilogue goes) and conv6 reads folded inputs -- both
    # leave the 2:4 form, and the split-K policy takes neither
    m.sparse = "2:4"
    m.set_masks(with_dead_filters(base, 5, 64))
    eng = state("6 2:4 + splitk, filter mask", "2:4", True, dict(sparse_layers=[2, 3, 4, 7, 9], splitk_layers=[8, 10]))
    assert eng.layers[4].perm is not None and (eng.layers[5].fold is eng.layers[4] or eng.layers[5].g_cols is not None)
    # the block-sparse policy runs in front of the compaction and exempts what it takes: conv5 keeps its dense layout
    eng = state("7 block + splitk, filter mask", "block", True, dict(bsparse_layers=ALL))
    assert eng.layers[4].perm is None and eng.layers[5].fold is None
    eng = state("8 dense, filter mask", None, False, {})
    assert eng is first and eng.layers[4].perm is not None


@pytest.mark.parametrize("prec", ["fp8", "fp8-2:4"])
def test_fp8_forms_do_not_depend_on_history(dev, prec):
    m, x = model(dev, prec), image(dev)
    sp = prec == "fp8-2:4"
    fp8 = list(range(3, 11))
    first = compare(m, dev, x, prec + " 1 no masks", dict(fp8_layers=fp8))
    conforming = [3, 4, 6, 7, 9]
    base = masks_24(m, conforming)
    m.set_masks(base)
    compare(m, dev, x, prec + " 2 2:4 masks", dict(fp8_layers=fp8, fp8_sparse_layers=conforming if sp else []))
    # conv7 compacted: it and its two readers (conv8 behind the pool, conv9 behind the routed copy) run fp16 launches
    m.set_masks(with_dead_filters(base, 7, 64))
    eng = compare(m, dev, x, prec + " 3 filter mask", dict(fp8_layers=[3, 4, 5, 6, 10], fp8_sparse_layers=[3, 4, 6] if sp else []))
    assert eng.layers[6].perm is not None
    for c in convs_of(m):
        c.mask_flag = False
    eng = compare(m, dev, x, prec + " 4 masks off", dict(fp8_layers=fp8))
    assert eng is first


def test_fp8_qat_eval_after_a_training_step(dev):
    m, x = model(dev, "fp8-qat"), image(dev)
    m.train()
    out = m(x)
    m.zero_grad()
    out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(12)).to(dev))
    train = [e for e in m._engines.values() if e.train_layout][0]
    assert train.fp8_layers == list(range(3, 11)) and train.fp8_sparse_layers == []
    m.eval()
    compare(m, dev, x, "fp8-qat eval", dict(fp8_layers=list(range(3, 11))))


def test_forbidden_combinations_raise(dev):
    x = image(dev)
    m = model(dev, "fp16")
    with torch.no_grad():
        ref = m(x).clone()
        m.sparse = "3:4"
        with pytest.raises(McamdError, match=r"sparse must be None, '2:4' or 'block' \(got '3:4'\)"):
            m(x)
        m.sparse = None
        assert torch.equal(m(x), ref)          # the refused call left the engine as it was
        m.precision, m.sparse, m.splitk = "fp8", "2:4", False
        with pytest.raises(McamdError, match="sparse='2:4' runs in the plain-fp16 inference engine only"):
            m(x)
        m.sparse, m.splitk = None, True
        with pytest.raises(McamdError, match="splitk=True runs in the plain-fp16 inference engine only"):
            m(x)
    m.precision, m.sparse, m.splitk = "fp8", None, False
    m.train()
    with pytest.raises(McamdError, match="precision 'fp8' is inference only"):
        m(x)
