"""Darknet.precision = "fp8-splitk": the low-batch form of the fp8 inference engine (csrc/conv_q8_splitk.hip) on a
synthetic-init YOLOv2-VOC at 416x416 -- which fp8 blocks split at B = 1, every fp8 block recomputed in float64 from the codes
the engine fed it (the method of test_q8_model_gpu.check_blocks, restated here), the end-to-end error LEVEL against the CPU
restatement (two 8-bit engines are never compared output to output), plan replay, precision switches, no allocation in a
warm forward, a batch the policy leaves alone, the precision / mode rules, a slim_export model and model.detect."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, slim, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import quick_filter_prune  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402
import q8_ref as R  # noqa: E402
import q8_slim_ref as S  # noqa: E402

TOL = 1e-3
EXPECTED = list(range(3, 23))      # conv3 ... conv22
MUST_SPLIT = {14, 16, 18, 19, 20, 22}
PINNED = "splitk=True runs in the plain-fp16 inference engine only"


def engine_for(m, x, prec="fp8-splitk"):
    return [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and k[3] == prec and not e.train_layout][0]


def convs_of(m):
    return [mod[0] for mod in m.models if isinstance(mod, torch.nn.Sequential) and hasattr(mod[0], "mask_flag")]


@functools.lru_cache(maxsize=None)
def dense(dev):
    """The model in eval mode, one image, and for it the fp32 oracle's logits and the fp8 restatement's (conv3 - conv22
    quantised): computed once, shared, left unchanged."""
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(blocks, seed=1))
    m.to(dev).eval()
    x1 = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(5))
    state = {k: v.cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref32 = O.forward(blocks, state, x1, training=False)
        ref8 = R.forward(blocks, state, x1, EXPECTED)
    return m, x1.to(dev), ref32, ref8


def check_blocks(m, eng, convs, over, cap, tables=False):
    """Recompute fp8 blocks from the codes the engine fed them (its own buffers after a forward, Engine.q8_block_io), in
    float64 (`tables`: with the conv's border table, a slim model).  A differing byte that is not the adjacent code, or an fp16
    destination off by more than TOL, fails at once; blocks above the byte-mismatch cap are collected in `over` and asserted by
    the caller at its end, so that every block is still recomputed."""
    layers = convs_of(m)
    worst = 0.0
    for c in convs:
        io = eng.q8_block_io(c)
        conv = layers[c - 1]
        mask = conv.mask.cpu() if conv.mask_flag else None
        w8, e = R.quantise_weights(conv.weight.data.cpu(), mask)
        slope = R.SLOPE if io["slope"] != 1.0 else 1.0
        tab = getattr(conv, "border_bias", None) if tables else None
        if tables:
            v = S.block_border(io["x8"], w8, e, io["scale"], io["shift"], tab.cpu() if tab is not None else None, slope)
        else:
            v = R.block(io["x8"], w8, e, io["scale"], io["shift"], slope)
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


@pytest.mark.parametrize("mfma", [0, 1])
def test_b1_layers_blocks_and_error_level(dev, mfma, setenv):
    """B = 1: the set of fp8 blocks is "fp8"'s, the 13x13 3x3 layers split, EVERY fp8 block is recomputed inside the project's
    cap of its MFMA form, and e_engine <= 1.10 e_ref against the fp32 oracle (the rule of test_fp8_error_level)."""
    setenv("MCAMD_Q8_MFMA", str(mfma))
    m, x, ref32, ref8 = dense(dev)
    try:
        m.precision = "fp8-splitk"
        with torch.no_grad():
            got = m(x).clone()
        eng = engine_for(m, x)
        assert eng.fp8_layers == EXPECTED
        assert set(eng.fp8_splitk_layers) >= MUST_SPLIT and set(eng.fp8_splitk_layers) <= set(eng.fp8_layers), eng.fp8_splitk_layers
        assert eng.splitk_layers == [] and eng.fp8_sparse_layers == []
        for lay in eng.layers:
            assert [lay.sp_on, lay.bs_on, lay.sk_on, lay.q8_on].count(True) == (lay.form != "dense"), lay.li + 1
            assert (lay.form == "q8_splitk") == (lay.li + 1 in eng.fp8_splitk_layers) and (lay.sk_slices >= 2) == (lay.form == "q8_splitk")
        over = []
        worst = check_blocks(m, eng, eng.fp8_layers, over, R.FP8_MFMA_CAP if mfma else R.MISMATCH_CAP)
        e_engine, e_ref = rel_l2(got.cpu(), ref32), rel_l2(ref8, ref32)
        print("MCAMD_Q8_MFMA=%d B=1: split layers %s; worst byte mismatch share over conv3-conv22 %.3g; engine %.4f, q8_ref %.4f "
              "against the fp32 oracle (ratio %.3f)" % (mfma, eng.fp8_splitk_layers, worst, e_engine, e_ref, e_engine / e_ref))
        assert not over, "; ".join(over)
        assert bool(torch.isfinite(got).all()) and e_engine <= 1.10 * e_ref
    finally:
        m.precision = "auto"


def test_b1_plan_replay_precision_switches_and_no_allocation(dev):
    m, x, _, _ = dense(dev)
    try:
        with torch.no_grad():
            m.precision = "fp8-splitk"
            sk = m(x).clone()
            assert torch.equal(m(x), sk), "the replayed plan differs from the recorded forward"
            m.precision = "fp8"
            q = m(x).clone()
            assert engine_for(m, x, "fp8").fp8_splitk_layers == [] and engine_for(m, x, "fp8").fp8_layers == EXPECTED
            m.precision = "fp16"
            d = m(x).clone()
            for prec, want in (("fp8-splitk", sk), ("fp8", q), ("fp16", d), ("fp8", q), ("fp8-splitk", sk)):
                m.precision = prec
                assert torch.equal(m(x), want), "%s: the engine does not give its earlier logits back" % prec
            print("B=1 fp8-splitk vs fp8 engine rel-L2 %.3g (summation order only)" % rel_l2(sk.cpu(), q.cpu()))
            m(x)
            torch.cuda.synchronize()
            before = torch.cuda.memory_stats(dev)
            m(x)
            torch.cuda.synchronize()
            after = torch.cuda.memory_stats(dev)
        assert after["num_alloc_retries"] == before["num_alloc_retries"]
        assert after["segment.all.allocated"] == before["segment.all.allocated"]
    finally:
        m.precision = "auto"


def test_b32_runs_exactly_the_fp8_launches(dev):
    m, _, _, _ = dense(dev)
    x = torch.rand(32, 3, 416, 416, generator=torch.Generator().manual_seed(6)).to(dev)
    try:
        with torch.no_grad():
            m.precision = "fp8"
            q = m(x).clone()
            m.precision = "fp8-splitk"
            sk = m(x)
            eng = engine_for(m, x)
            assert eng.fp8_splitk_layers == [] and eng.fp8_layers == EXPECTED
            assert torch.equal(sk, q)
    finally:
        m.precision = "auto"


def test_rules(dev):
    m, x, _, _ = dense(dev)
    try:
        m.precision = "fp8-splitk"
        m.train()
        with pytest.raises(McamdError, match="inference only"):
            m(torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(9)).to(dev))
        m.eval()
        m.splitk = True
        for prec in ("fp8-splitk", "fp8"):
            m.precision = prec
            with torch.no_grad(), pytest.raises(McamdError, match=PINNED) as err:
                m(x)
            assert "'fp8-splitk'" in str(err.value) and "model.splitk = False" in str(err.value)
        m.precision = "mixed"
        with torch.no_grad(), pytest.raises(McamdError, match=PINNED) as err:
            m(x)
        assert "fp8-splitk" not in str(err.value)
    finally:
        m.splitk = False
        m.eval()
        m.precision = "auto"


def test_detect_shapes(dev):
    m, x, _, _ = dense(dev)
    try:
        m.precision = "fp8"
        base = m.detect(x)
        m.precision = "fp8-splitk"
        got = m.detect(x)
        assert engine_for(m, x).fp8_splitk_layers
        assert [(t.shape, t.dtype) for t in got] == [(t.shape, t.dtype) for t in base]
    finally:
        m.precision = "auto"


def test_slim_model(dev, tmp_path):
    """quick_filter_prune(60) -> slim_export at B = 1: the blocks with a border table or a ragged cin keep the slim fp8 kernel
    (none of them splits), the set of fp8 blocks is "fp8"'s, and the logits sit at the restatement's error level."""
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(blocks, seed=0))
    m.to(dev)
    masks = quick_filter_prune(m, 60.0)
    m.set_masks(masks)
    m.eval()
    cfg = str(tmp_path / "slim60.cfg")
    s = slim.slim_export(m, cfg)
    x1 = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref32 = O.forward(blocks, {k: v.cpu() for k, v in m.state_dict().items()}, x1, training=False, masks=[k.cpu() for k in masks])
        s.precision = "fp8"
        s(x1.to(dev))
        fp8_layers = list(engine_for(s, x1, "fp8").fp8_layers)
        s.precision = "fp8-splitk"
        got = s(x1.to(dev)).clone()
        eng = engine_for(s, x1)
        assert torch.equal(s(x1.to(dev)), got)
        tables = {i + 1: c.border_bias.cpu() for i, c in enumerate(convs_of(s)) if getattr(c, "border_bias", None) is not None}
        ref8 = S.forward(O.parse_cfg(cfg), {k: v.cpu() for k, v in s.state_dict().items()}, x1, fp8_layers, tables)
    by = {lay.li + 1: lay for lay in eng.layers}
    slim_blocks = [n for n in eng.fp8_layers if by[n].q8_slim]
    assert eng.fp8_layers == fp8_layers and slim_blocks, (eng.fp8_layers, fp8_layers)
    assert set(slim_blocks) & set(eng.fp8_splitk_layers) == set() and set(eng.fp8_splitk_layers) <= set(eng.fp8_layers)
    assert all(by[n].form == "q8_splitk" and by[n].border is None and by[n].cin % 64 == 0 for n in eng.fp8_splitk_layers)
    over = []
    check_blocks(s, eng, eng.fp8_layers, over, R.MISMATCH_CAP, tables=True)
    e_engine, e_ref = rel_l2(got.cpu(), ref32), rel_l2(ref8, ref32)
    print("slim60 B=1: fp8 blocks %s, slim ones %s, split ones %s; engine %.4f, q8_slim_ref %.4f against the fp32 masked-dense "
          "oracle (ratio %.3f)" % (eng.fp8_layers, slim_blocks, eng.fp8_splitk_layers, e_engine, e_ref, e_engine / e_ref))
    assert not over, "; ".join(over)
    assert bool(torch.isfinite(got).all()) and e_engine <= 1.10 * e_ref
