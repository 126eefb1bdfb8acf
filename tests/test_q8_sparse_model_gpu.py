"""Darknet.precision = "fp8-2:4": the fp8 engine with the nm_prune masks on the sparse fp8 kernel (csrc/conv_q8_sparse.hip,
Engine._choose_q8) -- which blocks go sparse, every block recomputed from the input the engine gave it, the end-to-end
error LEVEL against the CPU restatement (q8_ref.forward with the 2:4 masks: a 2:4 mask is just a mask), the per-block
fallback to the dense fp8 kernel, engine separation, the precision rules and no allocation in a warm forward."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import nm_prune  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402
import q8_ref as R  # noqa: E402
import q8_sparse_ref as S  # noqa: E402
from test_q8_model_gpu import check_blocks, engine_for, EXPECTED  # noqa: E402

PREC = "fp8-2:4"


def pruned(dev, seed=0, masked=True):
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(blocks, seed=seed))
    m.to(dev)
    masks = None
    if masked:
        masks = nm_prune(m)
        m.set_masks(masks)
    m.eval()
    return blocks, m, masks


def test_fp8_sparse_layers_and_blocks_inside_the_engine(dev):
    _, m, _ = pruned(dev, seed=1)
    m.precision = PREC
    x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(5)).to(dev)
    with torch.no_grad():
        q1 = m(x)
        eng = engine_for(m, x, PREC)
        assert eng.fp8_layers == EXPECTED and eng.fp8_sparse_layers == EXPECTED
        over = []
        worst = check_blocks(m, eng, eng.fp8_layers, over)
        q2 = m(x)
    print("worst byte mismatch share over conv3-conv22: %.3g" % worst)
    assert torch.equal(q1, q2), "run to run"
    assert not over, "; ".join(over)


def error_level(dev, seed, cap=R.MISMATCH_CAP):
    blocks, m, masks = pruned(dev, seed=seed)
    m.precision = PREC
    x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(6 + seed))
    state = {k: v.cpu() for k, v in m.state_dict().items()}
    cm = [k.cpu() for k in masks]
    with torch.no_grad():
        got = m(x.to(dev)).cpu()
        eng = engine_for(m, x, PREC)
        assert eng.fp8_layers == EXPECTED and eng.fp8_sparse_layers == EXPECTED
        over = []
        worst = check_blocks(m, eng, eng.fp8_layers, over, cap=cap)
        ref32 = O.forward(blocks, state, x, training=False, masks=cm)
        ref8 = R.forward(blocks, state, x, eng.fp8_layers, masks=cm)
    e_engine, e_ref = rel_l2(got, ref32), rel_l2(ref8, ref32)
    print("seed %d 2:4: worst byte mismatch share %.3g; engine %.4f, q8_ref %.4f against the fp32 masked oracle (ratio %.3f)"
          % (seed, worst, e_engine, e_ref, e_engine / e_ref))
    assert not over, "; ".join(over)
    assert e_engine <= 1.10 * e_ref


@pytest.mark.parametrize("seed", [0, 1])
def test_fp8_sparse_error_level(dev, seed):
    error_level(dev, seed)


def test_fp8_sparse_fp8_mfma_switch_model(dev, setenv):
    """MCAMD_Q8_MFMA=1 inside the engine: the same blocks, every block inside that instruction's cap (adjacent codes only),
    the same error level as the restatement."""
    setenv("MCAMD_Q8_MFMA", "1")
    error_level(dev, 1, cap=S.FP8_SPARSE_MFMA_CAP)


def test_fp8_sparse_per_block_fallback(dev):
    _, m, masks = pruned(dev, seed=0)
    m.precision = PREC
    x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(8)).to(dev)
    rest = [c for c in EXPECTED if c != 9]
    with torch.no_grad():
        q1 = m(x)
        eng = engine_for(m, x, PREC)
        assert eng.fp8_sparse_layers == EXPECTED
        conv9 = [mod[0] for mod in m.models if isinstance(mod, torch.nn.Sequential) and hasattr(mod[0], "mask_flag")][8]
        w9 = conv9.weight.data.clone()          # (set_mask zeroes the pruned weights for good, as the reference does)
        gen = torch.Generator().manual_seed(12)
        other = [k.clone() for k in masks]
        other[8] = (torch.rand(masks[8].shape, generator=gen) < 0.5).float().to(dev)      # conv9: 50 %, not 2:4
        m.set_masks(other)
        m(x)
        assert eng.fp8_layers == EXPECTED and eng.fp8_sparse_layers == rest
        over = []
        check_blocks(m, eng, eng.fp8_layers, over)
        conv9.weight.data.copy_(w9)
        m.set_masks(masks)
        q3 = m(x)
        assert eng.fp8_layers == EXPECTED and eng.fp8_sparse_layers == EXPECTED
        check_blocks(m, eng, [8, 9, 10], over)
    assert torch.equal(q1, q3), "the 2:4 mask restored"
    assert not over, "; ".join(over)


def test_fp8_sparse_without_masks_is_the_fp8_engine(dev):
    _, m, _ = pruned(dev, masked=False)
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        m.precision = "fp8"
        q = m(x)
        m.precision = PREC
        s = m(x)
    eng = engine_for(m, x, PREC)
    assert eng.fp8_layers == EXPECTED and eng.fp8_sparse_layers == []
    assert torch.equal(q, s)


def test_fp8_sparse_engine_separation(dev):
    _, m, _ = pruned(dev)
    for B, H, W in ((1, 416, 416), (128, 416, 416), (4, 352, 480)):
        x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(4)).to(dev)
        first = {}
        with torch.no_grad():
            for prec in ("fp16", "fp8", PREC, "fp8", "fp16", PREC):
                m.precision = prec
                out = m(x)
                assert torch.equal(first.setdefault(prec, out), out), "%s at B=%d changed after a switch" % (prec, B)
        eng = engine_for(m, x, PREC)
        assert eng.fp8_layers == EXPECTED and eng.fp8_sparse_layers == EXPECTED
        dense = engine_for(m, x, "fp8")
        assert dense.fp8_layers == EXPECTED and dense.fp8_sparse_layers == []
        assert first[PREC].shape == first["fp16"].shape and bool(torch.isfinite(first[PREC]).all())
        print("B=%d %dx%d: fp8-2:4 vs fp8 engine rel-L2 %.3g, vs fp16 %.3g"
              % (B, H, W, rel_l2(first[PREC].cpu(), first["fp8"].cpu()), rel_l2(first[PREC].cpu(), first["fp16"].cpu())))


def test_fp8_sparse_rules_and_allocates_nothing_warm(dev):
    _, m, _ = pruned(dev)
    m.precision = PREC
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(9)).to(dev)
    m.train()
    with pytest.raises(McamdError):
        m(x)
    m.eval()
    m.sparse = "2:4"
    with torch.no_grad(), pytest.raises(McamdError):
        m(x)
    m.precision = "fp8"
    with torch.no_grad(), pytest.raises(McamdError, match="fp8-2:4"):
        m(x)
    m.sparse = None
    m.precision = PREC
    with torch.no_grad():
        m(x)
        m(x)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats(dev)
        m(x)
        torch.cuda.synchronize()
        after = torch.cuda.memory_stats(dev)
    assert engine_for(m, x, PREC).fp8_sparse_layers == EXPECTED
    assert after["num_alloc_retries"] == before["num_alloc_retries"]
    assert after["segment.all.allocated"] == before["segment.all.allocated"]
