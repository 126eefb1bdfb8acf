"""Darknet.precision = "fp8-w4": the fp8 engine of YOLOv2-VOC on 4-bit weights (csrc/conv_q8_w4.hip, engine._Q8W4, DESIGN.md
3w) -- which blocks take the form and what they hold, every w4 block recomputed from the codes the engine fed it (w4_ref +
q8_ref.block, float64), equality with the "fp8" engine of a model whose weights ARE the dequantised 4-bit values, the
end-to-end error level against the fp32 oracle beside the CPU restatement's, the precision's rules, switching between
precisions, no allocation in a warm forward and model.detect."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, ops, slim, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd import engine as E  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import quick_filter_prune  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402
import q8_ref as R  # noqa: E402
import w4_ref as W  # noqa: E402

TOL = 1e-3
EXPECTED = list(range(3, 23))      # conv3 ... conv22


def model(dev, seed=1):
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(blocks, seed=seed))
    m.to(dev)
    m.eval()
    return blocks, m


def engine_for(m, x, prec="fp8-w4"):
    return [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and k[3] == prec and not e.train_layout][0]


def convs_of(m):
    return [mod[0] for mod in m.models if isinstance(mod, torch.nn.Sequential) and hasattr(mod[0], "mask_flag")]


@pytest.fixture(scope="module")
def quantised(dev):
    """The seed-1 network, its 4-bit quantisation on the CPU (once; shared and left unchanged): per conv number of EXPECTED the
    bytes the codes stand for, the exponents e4 and the dequantised fp32 weights; the input and the fp32 oracle's logits."""
    blocks, m = model(dev)
    q = {}
    for c in EXPECTED:
        codes, g, e4, values, b = W.quantise(convs_of(m)[c - 1].weight.data.cpu())
        q[c] = (b, e4, W.dequantised(values, e4))
    x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(5))
    state = {k: v.cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref32 = O.forward(blocks, state, x, training=False)
    return blocks, m, q, x, state, ref32


def dequantised_model(dev, q):
    """Model B: the same network with the weights of the w4 blocks replaced by the values their codes stand for."""
    _, b = model(dev)
    for c, (_, _, wd) in q.items():
        convs_of(b)[c - 1].weight.data.copy_(wd.to(dev))
    b.invalidate_packed()
    b.eval()
    return b


def check_blocks(eng, q, convs, over, cap):
    """test_q8_model_gpu.check_blocks for w4 blocks: recomputed in float64 from the codes the engine fed them and w4_ref's bytes
    and exponents.  A differing byte that is not the adjacent code, or an fp16 destination off by more than TOL, fails at
    once; blocks above the cap are collected in `over`."""
    worst = 0.0
    for c in convs:
        io = eng.q8_block_io(c)
        b, e4, _ = q[c]
        v = R.block(io["x8"], b, e4, io["scale"], io["shift"], R.SLOPE if io["slope"] != 1.0 else 1.0)
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


def weight_operand_bytes(eng, convs):
    """resident bytes of the weight operands the forward of these blocks reads"""
    total = 0
    for lay in eng.layers:
        if lay.li + 1 in convs:
            total += sum(getattr(lay, name).numel() * getattr(lay, name).element_size() for name, _ in E._FORMS[lay.form].bufs)
    return total


def test_w4_layers_forms_and_buffers(dev, quantised):
    blocks, m, q, x, state, ref32 = quantised
    with torch.no_grad():
        m.precision = "fp8"
        m(x.to(dev))
        m.precision = "fp8-w4"
        m(x.to(dev))
    e8, e4 = engine_for(m, x, "fp8"), engine_for(m, x)
    assert e4.fp8_w4_layers == e4.fp8_layers == EXPECTED and e8.fp8_layers == EXPECTED
    assert e8.fp8_w4_layers == [] and e4.fp8_sparse_layers == [] and e4.fp8_splitk_layers == []
    for lay in e4.layers:
        assert lay.form in E._FORMS and [lay.sp_on, lay.bs_on, lay.sk_on, lay.q8_on].count(True) <= 1
        if lay.li + 1 in EXPECTED:
            assert lay.form == "q8_w4" and lay.wq is None and lay.wqs is None and lay.wexp is None, "no byte operand is held"
            nc, ng, ne = ops.q8_w4_elems(lay.geom_q8)
            assert (lay.w4c.numel(), lay.w4g.numel(), lay.wexp4.numel()) == (nc, ng, ne)
            assert lay.w4c.dtype == lay.w4g.dtype == torch.uint8 and lay.wexp4.dtype == torch.int32
            assert 8 * (nc + ng) == 4.25 * ops.q8_elems(lay.geom_q8)[0]
            # the engine's operands are the packer's for the block's weights
            b, e, _ = q[lay.li + 1]
            assert torch.equal(lay.wexp4[:lay.cout].cpu(), e)
        else:
            assert lay.form == "dense" and lay.w4c is None and lay.w4g is None and lay.wexp4 is None
    # formats are the fp8 engine's: conv22 writes fp16 for conv23, conv3 reads a cast copy
    by = {lay.li + 1: lay for lay in e4.layers}
    assert not by[22].q8_y and all(by[c].q8_y for c in range(3, 22)) and by[13].q8_y2 and by[3].xq is not None
    b8, b4 = weight_operand_bytes(e8, EXPECTED), weight_operand_bytes(e4, EXPECTED)
    print("resident weight-operand bytes of conv3-conv22: fp8 %d, fp8-w4 %d (%.3f x)" % (b8, b4, b4 / b8))
    assert b4 < 0.54 * b8                                   # 4.25 / 8 of the bytes, exponents on both sides


def test_w4_blocks_inside_the_engine(dev, quantised):
    blocks, m, q, x, state, ref32 = quantised
    with torch.no_grad():
        m.precision = "fp8-w4"
        m(x.to(dev))
    eng = engine_for(m, x)
    over = []
    worst = check_blocks(eng, q, eng.fp8_w4_layers, over, R.MISMATCH_CAP)
    print("worst byte mismatch share over conv3-conv22: %.3g" % worst)
    assert not over, "; ".join(over)


def test_w4_equals_fp8_on_the_dequantised_weights_and_error_level(dev, quantised):
    """Model B holds the values A's codes stand for (values * 2^-e4_f, fp32-exact) and runs under "fp8".  B's filter maxima are
    128 or 192 times 2^-e4_f, so mcamd_pack_q8 picks e4_f + 1 and its bytes are exactly twice the w4 values; S doubles exactly
    in fp32 and the epilogue's power of two halves it: the logits are EQUAL.  The error level against the fp32 oracle:
    e_engine <= 1.10 e_ref, e_ref from q8_ref.forward on B's state (the same arithmetic, by the same argument)."""
    blocks, m, q, x, state, ref32 = quantised
    mb = dequantised_model(dev, q)
    with torch.no_grad():
        m.precision = "fp8-w4"
        a = m(x.to(dev)).cpu()
        mb.precision = "fp8"
        b = mb(x.to(dev)).cpu()
        assert engine_for(mb, x, "fp8").fp8_layers == EXPECTED
        m.precision = "fp8"
        a8 = m(x.to(dev)).cpu()
        ref4 = R.forward(blocks, {k: v.cpu() for k, v in mb.state_dict().items()}, x, EXPECTED)
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, b), "fp8-w4 differs from fp8 on the dequantised weights in %d logits" % int((a != b).sum())
    e_engine, e_ref, e_fp8 = rel_l2(a, ref32), rel_l2(ref4, ref32), rel_l2(a8, ref32)
    print("fp8-w4 engine %.4f, w4 restatement %.4f against the fp32 oracle (ratio %.3f); fp8 engine %.4f"
          % (e_engine, e_ref, e_engine / e_ref, e_fp8))
    assert e_engine <= 1.10 * e_ref


def test_w4_fp8_mfma_model(dev, quantised, setenv):
    """MCAMD_Q8_MFMA=1: every w4 block recomputed inside q8_ref.FP8_MFMA_CAP (adjacent codes only), and against the "fp8" engine
    on the dequantised weights block by block under the same rule (whether they were equal as well is printed)."""
    setenv("MCAMD_Q8_MFMA", "1")
    blocks, m0, q, x, state, ref32 = quantised
    _, m = model(dev)
    mb = dequantised_model(dev, q)
    with torch.no_grad():
        m.precision = "fp8-w4"
        a = m(x.to(dev)).cpu()
        mb.precision = "fp8"
        b = mb(x.to(dev)).cpu()
    ea, eb = engine_for(m, x), engine_for(mb, x, "fp8")
    assert ea.fp8_w4_layers == EXPECTED and eb.fp8_layers == EXPECTED
    over = []
    worst = check_blocks(ea, q, EXPECTED, over, R.FP8_MFMA_CAP)
    worst_ab = 0.0
    for c in EXPECTED:
        ia, ib = ea.q8_block_io(c), eb.q8_block_io(c)
        for name in ("y", "y2"):
            if ia[name] is None:
                continue
            if ia[name + "_f8"]:
                share, adjacent = R.byte_mismatch(ia[name], ib[name])
                worst_ab = max(worst_ab, share)
                assert adjacent, "conv%d %s: fp8-w4 and fp8 differ by more than one code" % (c, name)
                if share > R.FP8_MFMA_CAP:
                    over.append("conv%d %s: fp8-w4 vs fp8 on the dequantised weights, share %.3g" % (c, name, share))
            else:
                assert rel_l2(ia[name], ib[name]) < TOL
    print("fp8 MFMA: worst share against the float64 reference %.3g; against fp8 on the dequantised weights %.3g; logits equal: %s"
          % (worst, worst_ab, torch.equal(a, b)))
    assert not over, "; ".join(over)


def test_w4_rules_switching_allocation_and_detect(dev, quantised):
    blocks, m0, q, x0, state, ref32 = quantised
    _, m = model(dev)
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(9)).to(dev)
    m.precision = "fp8-w4"
    m.train()
    with pytest.raises(McamdError, match="fp8-w4"):
        m(x)
    m.eval()
    m.sparse = "2:4"
    with torch.no_grad(), pytest.raises(McamdError, match="fp8-w4"):
        m(x)
    m.sparse = None
    m.splitk = True
    with torch.no_grad(), pytest.raises(McamdError, match="fp8-w4"):
        m(x)
    m.splitk = False
    with torch.no_grad():
        m.precision = "fp8"
        q8a = m(x)
        m.precision = "fp8-w4"
        w4a = m(x)
        m.precision = "fp8"
        q8b = m(x)
        m.precision = "fp8-w4"
        w4b = m(x)
        assert torch.equal(q8a, q8b) and torch.equal(w4a, w4b) and not torch.equal(q8a, w4a)
        m(x)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats(dev)
        m(x)
        torch.cuda.synchronize()
        after = torch.cuda.memory_stats(dev)
    assert after["num_alloc_retries"] == before["num_alloc_retries"]
    assert after["segment.all.allocated"] == before["segment.all.allocated"]
    m.precision = "fp8"
    d8 = m.detect(x)
    m.precision = "fp8-w4"
    d4 = m.detect(x)
    assert len(d8) == len(d4) and all(u.shape == v.shape and u.dtype == v.dtype and u.device == v.device for u, v in zip(d8, d4))


def test_w4_slim_model_keeps_its_slim_blocks(dev, tmp_path):
    """A slim_export model: the blocks "fp8" runs as "q8_slim" keep that form, every block "fp8" runs as "q8" takes the 4-bit
    form, and the model still runs."""
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(blocks, seed=0))
    m.to(dev)
    m.set_masks(quick_filter_prune(m, 60.0))
    m.eval()
    s = slim.slim_export(m, str(tmp_path / "slim60.cfg"))
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        s.precision = "fp8"
        d = s(x)
        f8 = {lay.li + 1: lay.form for lay in engine_for(s, x, "fp8").layers}
        s.precision = "fp8-w4"
        got = s(x)
        eng = engine_for(s, x)
        f4 = {lay.li + 1: lay.form for lay in eng.layers}
    assert "q8_slim" in f8.values()
    assert f4 == {n: ("q8_w4" if form == "q8" else form) for n, form in f8.items()}
    assert eng.fp8_w4_layers == [n for n, form in sorted(f8.items()) if form == "q8"]
    assert bool(torch.isfinite(got).all()) and got.shape == d.shape
    print("slim60: forms %r; fp8-w4 vs fp8 rel-L2 %.3g" % (sorted(set(f4.values())), rel_l2(got.cpu(), d.cpu())))
