"""Darknet.precision = "fp8": post-training e4m3 inference of YOLOv2-VOC (csrc/conv_q8.hip, Engine._choose_q8) -- which
blocks are quantised, every block recomputed exactly from the input the engine gave it, the end-to-end error LEVEL against
the CPU restatement (two correct 8-bit engines differ from each other at the level of their own quantisation noise, so
outputs are never compared directly), re-packing, the precision rules and no allocation in a warm forward."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import os  # noqa: E402

from modelcompression_amd import nets, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import weight_prune, quick_filter_prune  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402
import q8_ref as R  # noqa: E402

TOL = 1e-3
EXPECTED = list(range(3, 23))      # conv3 ... conv22


TWO_READERS_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "q8_two_readers.cfg")


def model(dev, seed=0, cfg=YOLOV2_VOC_CFG):
    blocks = O.parse_cfg(cfg)
    m = nets.Darknet(cfg)
    m.load_state_dict(O.init_state(blocks, seed=seed))
    m.to(dev)
    m.eval()
    return blocks, m


def engine_for(m, x, prec="fp8"):
    return [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and k[3] == prec and not e.train_layout][0]


def check_blocks(m, eng, convs, over, cap=R.MISMATCH_CAP):
    """Recompute fp8 blocks from the codes the engine fed them (its own buffers after a forward), in float64.  A differing
    byte that is not the adjacent code, or an fp16 destination off by more than TOL, fails at once (a wrong offset, a stale
    exponent, a mask that was not applied); blocks above the byte-mismatch cap are collected in `over` and asserted by the
    caller at its end, so that every stage of a test is still recomputed."""
    layers = [mod[0] for mod in m.models if isinstance(mod, torch.nn.Sequential) and hasattr(mod[0], "mask_flag")]
    worst = 0.0
    for c in convs:
        io = eng.q8_block_io(c)
        conv = layers[c - 1]
        mask = conv.mask.cpu() if conv.mask_flag else None
        w8, e = R.quantise_weights(conv.weight.data.cpu(), mask)
        v = R.block(io["x8"], w8, e, io["scale"], io["shift"], R.SLOPE if io["slope"] != 1.0 else 1.0)
        for name, got, f8, dst in (("y", io["y"], io["y_f8"], io["dst"]), ("y2", io["y2"], io["y2_f8"], "plain")):
            if got is None:
                continue
            if f8:
                share, adjacent = R.byte_mismatch(got, R.store_bytes(v, dst))
                worst = max(worst, share)
                assert adjacent, "conv%d %s: a differing byte is not the adjacent e4m3 code" % (c, name)
                if share > cap:
                    over.append("conv%d %s: share of differing bytes %.3g" % (c, name, share))
            else:
                err = rel_l2(got, R.store_fp16(v, dst))
                assert err < TOL, "conv%d %s: fp16 rel-L2 %.3g" % (c, name, err)
    return worst


def test_fp8_layers_and_engine_separation(dev):
    _, m = model(dev)
    for B in (1, 128):
        x = torch.rand(B, 3, 416, 416, generator=torch.Generator().manual_seed(4)).to(dev)
        with torch.no_grad():
            m.precision = "fp16"
            d = m(x)
            m.precision = "fp8"
            q1 = m(x)
            assert engine_for(m, x).fp8_layers == EXPECTED
            q2 = m(x)
            m.precision = "fp16"
            d2 = m(x)
        assert torch.equal(d, d2), "the fp16 engine is unaffected"
        assert torch.equal(q1, q2), "fp8 run to run"
        assert q1.shape == d.shape and bool(torch.isfinite(q1).all())
        print("B=%d: fp8 vs fp16 engine rel-L2 %.3g" % (B, rel_l2(q1.cpu(), d.cpu())))
    # conv22 writes fp16 for conv23; every other fp8 block writes bytes; conv3 reads the cast copy of conv2's output
    eng = engine_for(m, x)
    by = {lay.li + 1: lay for lay in eng.layers}
    assert not by[22].q8_y and all(by[c].q8_y for c in range(3, 22))
    assert by[13].q8_y2 and by[3].xq is not None and all(by[c].xq is None for c in range(4, 23))


def test_fp8_blocks_exact_inside_the_engine(dev):
    _, m = model(dev, seed=1)
    m.precision = "fp8"
    x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(5)).to(dev)
    with torch.no_grad():
        m(x)
    eng = engine_for(m, x)
    over = []
    worst = check_blocks(m, eng, eng.fp8_layers, over)
    print("worst byte mismatch share over conv3-conv22: %.3g" % worst)
    assert not over, "; ".join(over)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("pruned", [False, True], ids=["dense", "weight80"])
def test_fp8_error_level(dev, seed, pruned):
    """e_engine <= 1.10 e_ref against the fp32 oracle (two correct implementations were within 1.3 % of each other;
    a plumbing error costs tens of per cent)."""
    blocks, m = model(dev, seed=seed)
    masks = None
    if pruned:
        masks = weight_prune(m, 80.0)
        m.set_masks(masks)
    m.precision = "fp8"
    x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(6 + seed))
    state = {k: v.cpu() for k, v in m.state_dict().items()}
    cm = [k.cpu() for k in masks] if masks is not None else None
    with torch.no_grad():
        got = m(x.to(dev)).cpu()
        layers = engine_for(m, x).fp8_layers
        ref32 = O.forward(blocks, state, x, training=False, masks=cm)
        ref8 = R.forward(blocks, state, x, layers, masks=cm)
    assert layers == EXPECTED
    e_engine, e_ref = rel_l2(got, ref32), rel_l2(ref8, ref32)
    print("seed %d %s: engine %.4f, q8_ref %.4f against the fp32 oracle (ratio %.3f)"
          % (seed, "weight80" if pruned else "dense", e_engine, e_ref, e_engine / e_ref))
    assert e_engine <= 1.10 * e_ref


def test_fp8_mfma_switch_model(dev, setenv):
    """MCAMD_Q8_MFMA=1 inside the engine: the same blocks, every block recomputed from the engine's own buffers inside
    q8_ref.FP8_MFMA_CAP (adjacent codes only), and the same error level as the restatement."""
    setenv("MCAMD_Q8_MFMA", "1")
    blocks, m = model(dev, seed=1)
    m.precision = "fp8"
    x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(5))
    state = {k: v.cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        got = m(x.to(dev)).cpu()
        eng = engine_for(m, x)
        assert eng.fp8_layers == EXPECTED
        over = []
        worst = check_blocks(m, eng, eng.fp8_layers, over, cap=R.FP8_MFMA_CAP)
        ref32 = O.forward(blocks, state, x, training=False)
        ref8 = R.forward(blocks, state, x, eng.fp8_layers)
    e_engine, e_ref = rel_l2(got, ref32), rel_l2(ref8, ref32)
    print("fp8 MFMA: worst byte mismatch share over conv3-conv22 %.3g; engine %.4f, q8_ref %.4f (ratio %.3f)"
          % (worst, e_engine, e_ref, e_engine / e_ref))
    assert not over, "; ".join(over)
    assert e_engine <= 1.10 * e_ref


def test_fp8_one_format_per_tensor_with_two_readers(dev):
    """A concat buffer with two readers: conv4 reads the member conv3 on its own (64 channels: an fp8 block), conv5 the
    concatenation conv4 | conv3 (96 channels: not one).  The buffer must stay fp16 -- both writers are fp8 blocks, but one
    reader is not -- and conv4 reads a cast copy; every fp8 block is recomputed from the engine's own buffers and the error
    level is the restatement's (conv5 reading a buffer nobody writes costs tens of per cent)."""
    blocks, m = model(dev, seed=2, cfg=TWO_READERS_CFG)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(13))
    state = {k: v.cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        m.precision = "fp16"
        d = m(x.to(dev)).cpu()
        m.precision = "fp8"
        got = m(x.to(dev)).cpu()
        eng = engine_for(m, x)
        assert eng.fp8_layers == [3, 4, 6]
        by = {lay.li + 1: lay for lay in eng.layers}
        assert not by[3].q8_y and not by[4].q8_y and by[4].xq is not None and not eng.qbufs
        over = []
        check_blocks(m, eng, eng.fp8_layers, over)
        ref32 = O.forward(blocks, state, x, training=False)
        ref8 = R.forward(blocks, state, x, eng.fp8_layers)
    e_engine, e_ref = rel_l2(got, ref32), rel_l2(ref8, ref32)
    print("two readers: engine %.4f, q8_ref %.4f against the fp32 oracle; fp8 vs fp16 engine %.4f" % (e_engine, e_ref, rel_l2(got, d)))
    assert not over, "; ".join(over)
    assert e_engine <= 1.10 * e_ref


def test_fp8_non_square_input(dev):
    _, m = model(dev)
    x = torch.rand(4, 3, 352, 480, generator=torch.Generator().manual_seed(7)).to(dev)
    with torch.no_grad():
        m.precision = "fp16"
        d = m(x)
        m.precision = "fp8"
        q1, q2 = m(x), m(x)
    assert q1.shape == d.shape == (4, 125, 11, 15) and bool(torch.isfinite(q1).all()) and torch.equal(q1, q2)
    assert engine_for(m, x).fp8_layers == EXPECTED
    print("(4, 352, 480): fp8 vs fp16 engine rel-L2 %.3g" % rel_l2(q1.cpu(), d.cpu()))


def test_fp8_follows_replaced_weights(dev):
    blocks, m = model(dev, seed=0)
    m.precision = "fp8"
    x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(8)).to(dev)
    with torch.no_grad():
        m(x)
        eng = engine_for(m, x)
        m.load_state_dict(O.init_state(blocks, seed=3))      # another seed: the filters' largest weights move
        m(x)
        over = []
        check_blocks(m, eng, [3, 9, 13, 21, 22], over)
        layers = [mod[0] for mod in m.models if isinstance(mod, torch.nn.Sequential) and hasattr(mod[0], "mask_flag")]
        layers[4].weight.data.mul_(1.0 / 32)  # conv5 and conv21 through .data
        layers[20].weight.data[3].mul_(100.0)
        m.invalidate_packed()
        m(x)
        check_blocks(m, eng, [5, 21, 22], over)
        # and a mask, applied before the exponent is taken (random per weight: no filter is masked whole, which would
        # hand the block to filter compaction)
        gen = torch.Generator().manual_seed(12)
        masks = [(torch.rand(k.shape, generator=gen) < 0.5).float().to(dev) for k in weight_prune(m, 80.0)]
        m.set_masks(masks)
        m(x)
        assert eng.fp8_layers == EXPECTED
        check_blocks(m, eng, [4, 14, 21], over)
    assert not over, "; ".join(over)


def test_fp8_is_inference_only_and_allocates_nothing_warm(dev):
    _, m = model(dev)
    m.precision = "fp8"
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(9)).to(dev)
    m.train()
    with pytest.raises(McamdError):
        m(x)
    m.eval()
    m.sparse = "2:4"
    with torch.no_grad(), pytest.raises(McamdError):
        m(x)
    m.sparse = None
    with torch.no_grad():
        m(x)
        m(x)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats(dev)
        m(x)
        torch.cuda.synchronize()
        after = torch.cuda.memory_stats(dev)
    assert after["num_alloc_retries"] == before["num_alloc_retries"]
    assert after["segment.all.allocated"] == before["segment.all.allocated"]


def test_fp8_leaves_compacted_blocks_fp16(dev):
    """Filter compaction and folding are out of scope: a filter40 model still runs, with fewer fp8 blocks (or none)."""
    _, m = model(dev)
    m.set_masks(quick_filter_prune(m, 40.0))
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(10)).to(dev)
    with torch.no_grad():
        m.precision = "fp16"
        d = m(x)
        m.precision = "fp8"
        q = m(x)
    layers = engine_for(m, x).fp8_layers
    print("filter40: fp8_layers %r, fp8 vs fp16 rel-L2 %.3g" % (layers, rel_l2(q.cpu(), d.cpu())))
    assert len(layers) < len(EXPECTED) and set(layers) <= set(EXPECTED)
    assert bool(torch.isfinite(q).all()) and rel_l2(q.cpu(), d.cpu()) < 0.5
