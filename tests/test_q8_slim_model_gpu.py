"""Darknet.precision = "fp8" / "fp8-2:4" on slim_export models: which blocks of the filter-pruned, physically
slim YOLOv2-VOC are quantised, every fp8 block recomputed from the codes the engine fed it (float64 restatement with the
border table, q8_slim_ref.block_border), the end-to-end error LEVEL against the fp32 oracle's masked-dense logits (outputs
of two fp8 implementations are never compared end to end), the sparse precision, no allocation in a warm forward and the
precision rules."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, ops, slim, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import quick_filter_prune, nm_prune  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402
import q8_ref as R  # noqa: E402
import q8_slim_ref as S  # noqa: E402

TOL = 1e-3
# input channels of conv1 .. conv23 of the 60 % slim model (oracle init seed 0, the reference's filter ranking)
SLIM60_CIN = [3, 8, 8, 8, 8, 8, 32, 16, 8, 176, 8, 56, 16, 40, 200, 32, 648, 32, 440, 736, 40, 800, 984]
CIN_RULE_60 = [7, 10, 12] + list(range(14, 23))


def build(dev, perc, tmp, seed=0):
    """(dense cfg blocks, masked-dense model, its masks, slim cfg blocks, slim model)"""
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(blocks, seed=seed))
    m.to(dev)
    masks = quick_filter_prune(m, perc)
    m.set_masks(masks)
    m.eval()
    cfg = str(tmp / ("slim%d.cfg" % int(perc)))
    s = slim.slim_export(m, cfg)
    return blocks, m, masks, O.parse_cfg(cfg), s


@pytest.fixture(scope="module")
def slim60(dev, tmp_path_factory):
    return build(dev, 60.0, tmp_path_factory.mktemp("slim60"))


def engine_for(m, x, prec="fp8"):
    return [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and k[3] == prec and not e.train_layout][0]


def convs_of(m):
    return [mod[0] for mod in m.models if isinstance(mod, torch.nn.Sequential) and hasattr(mod[0], "mask_flag")]


def expected_layers(m, s, eng):
    """The rule of DESIGN.md 3m from slim_summary and the engine's geometries: conv n in 2 .. 22 is an fp8 block when
    round_up(cin, 64) <= 2 cin and mcamd_conv_fwd_q8_slim_ok accepts the block on a byte buffer just wide enough."""
    out = []
    for (n, _, cout, _, cin), lay in zip(slim.slim_summary(m, s), eng.layers):
        assert (lay.li + 1, lay.cin, lay.cout) == (n, cin, cout)
        if not 2 <= n <= 22:
            continue
        cp = ops.round_up(cin, 64)
        ld = max(lay.tin.ld, ops.round_up(lay.tin.choff + cp, 16))
        if cp <= 2 * cin and ops.conv_fwd_q8_slim_ok(ops.geom(eng.B, lay.H, lay.W, lay.k, cin, cout, ld, lay.tin.choff, 0, 0)):
            out.append(n)
    return out


def check_blocks(s, eng, convs, over, cap=R.MISMATCH_CAP):
    """Recompute fp8 blocks of a slim model from the codes the engine fed them (its own buffers after a forward), in
    float64, with the conv's border table.  A differing byte that is not the adjacent code, or an fp16 destination off by
    more than TOL, fails at once; blocks above the byte-mismatch cap are collected in `over` for the caller's end."""
    layers = convs_of(s)
    worst = 0.0
    for c in convs:
        io = eng.q8_block_io(c)
        conv = layers[c - 1]
        mask = conv.mask.cpu() if conv.mask_flag else None
        w8, e = R.quantise_weights(conv.weight.data.cpu(), mask)
        assert io["x8"].shape[1] == conv.weight.shape[1]
        tab = getattr(conv, "border_bias", None)
        v = S.block_border(io["x8"], w8, e, io["scale"], io["shift"], tab.cpu() if tab is not None else None,
                           R.SLOPE if io["slope"] != 1.0 else 1.0)
        for name, got, f8, dst in (("y", io["y"], io["y_f8"], io["dst"]), ("y2", io["y2"], io["y2_f8"], "plain")):
            if got is None:
                continue
            if f8:
                share, adjacent = R.byte_mismatch(got, R.store_bytes(v, dst))
                worst = max(worst, share)
                print("conv%d %s (cin %d%s): byte mismatch share %.3g" % (c, name, conv.weight.shape[1], ", table" if tab is not None else "", share))
                assert adjacent, "conv%d %s: a differing byte is not the adjacent e4m3 code" % (c, name)
                if share > cap:
                    over.append("conv%d %s: share of differing bytes %.3g" % (c, name, share))
            else:
                err = rel_l2(got, R.store_fp16(v, dst))
                print("conv%d %s (cin %d%s): fp16 rel-L2 %.3g" % (c, name, conv.weight.shape[1], ", table" if tab is not None else "", err))
                assert err < TOL, "conv%d %s: fp16 rel-L2 %.3g" % (c, name, err)
    return worst


def tables_of(s):
    return {i + 1: c.border_bias.cpu() for i, c in enumerate(convs_of(s)) if getattr(c, "border_bias", None) is not None}


@pytest.fixture(scope="module")
def slim60_refs(slim60):
    """One input, the fp32 oracle's masked-dense logits for it, and the slim model's CPU state: shared, left unchanged."""
    blocks, m, masks, sblocks, s = slim60
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref32 = O.forward(blocks, {k: v.cpu() for k, v in m.state_dict().items()}, x, training=False, masks=[k.cpu() for k in masks])
    return x, ref32, {k: v.cpu() for k, v in s.state_dict().items()}


def run_model_60(dev, slim60, slim60_refs, cap):
    blocks, m, masks, sblocks, s = slim60
    x, ref32, sstate = slim60_refs
    assert [r[4] for r in slim.slim_summary(m, s)] == SLIM60_CIN
    with torch.no_grad():
        s.precision = "fp16"
        d = s(x.to(dev)).cpu()
        s.precision = "fp8"
        got = s(x.to(dev)).cpu()
        eng = engine_for(s, x)
        layers = list(eng.fp8_layers)
        s.precision = "auto"
    print("slim60 fp8_layers: %r" % layers)
    assert layers == expected_layers(m, s, eng)
    assert set(range(14, 21)) | {22} <= set(layers) and set(layers) <= set(CIN_RULE_60)
    assert [n for n in range(2, 23) if ops.round_up(SLIM60_CIN[n - 1], 64) <= 2 * SLIM60_CIN[n - 1]] == CIN_RULE_60
    over = []
    worst = check_blocks(s, eng, layers, over, cap)
    with torch.no_grad():
        ref8 = S.forward(sblocks, sstate, x, layers, tables_of(s))
    e_engine, e_ref, e_fp16 = rel_l2(got, ref32), rel_l2(ref8, ref32), rel_l2(d, ref32)
    print("slim60: worst byte mismatch share %.3g; against the fp32 masked-dense oracle: fp8 engine %.4f, q8_slim_ref %.4f "
          "(ratio %.3f), slim fp16 engine %.2e" % (worst, e_engine, e_ref, e_engine / e_ref, e_fp16))
    assert not over, "; ".join(over)
    assert e_engine <= 1.10 * e_ref


def test_slim60_fp8_layers_blocks_and_error_level(dev, slim60, slim60_refs):
    """YOLOv2-VOC, 60 % of the filters removed, 416 x 416, B = 2: the set of fp8 blocks, EVERY fp8 block teacher-forced, and
    e_engine <= 1.10 e_ref against the fp32 oracle (the bound of test_q8_model_gpu.py)."""
    run_model_60(dev, slim60, slim60_refs, R.MISMATCH_CAP)


def test_slim60_fp8_mfma(dev, setenv, slim60, slim60_refs):
    """... and with MCAMD_Q8_MFMA=1: the same set (the rule does not depend on the MFMA form), blocks inside FP8_MFMA_CAP."""
    setenv("MCAMD_Q8_MFMA", "1")
    run_model_60(dev, slim60, slim60_refs, R.FP8_MFMA_CAP)


def test_slim60_non_square_input(dev, slim60):
    """Input 3 x 3 x 96 x 32: the final grid is 3 x 1, so W = 1 sets the left and the right bit together on the 13-level
    layers (all pool inputs stay even); every fp8 block recomputed."""
    _, m, _, _, s = slim60
    x = torch.rand(3, 3, 96, 32, generator=torch.Generator().manual_seed(7)).to(dev)
    with torch.no_grad():
        s.precision = "fp8"
        q1, q2 = s(x), s(x)
        eng = engine_for(s, x)
        s.precision = "auto"
    assert q1.shape == (3, 125, 3, 1) and bool(torch.isfinite(q1).all()) and torch.equal(q1, q2)
    assert eng.fp8_layers == expected_layers(m, s, eng) and set(range(14, 21)) | {22} <= set(eng.fp8_layers)
    over = []
    check_blocks(s, eng, eng.fp8_layers, over)
    assert not over, "; ".join(over)


def test_slim40_rule_and_blocks(dev, tmp_path):
    """The 40 % model: conv14 (cin 120 -> 128), conv15 (cin 576: a multiple of 64, but with a table) and conv22 (cin 1040 ->
    1088, the concatenation) on a 160 x 160 input (a 5 x 5 final grid: every class and an interior)."""
    _, m, _, _, s = build(dev, 40.0, tmp_path)
    cin = {r[0]: r[4] for r in slim.slim_summary(m, s)}
    assert (cin[14], cin[15], cin[22]) == (120, 576, 1040)
    x = torch.rand(2, 3, 160, 160, generator=torch.Generator().manual_seed(8)).to(dev)
    with torch.no_grad():
        s.precision = "fp8"
        s(x)
    eng = engine_for(s, x)
    print("slim40 fp8_layers: %r" % eng.fp8_layers)
    assert eng.fp8_layers == expected_layers(m, s, eng) and {14, 15, 22} <= set(eng.fp8_layers)
    by = {lay.li + 1: lay for lay in eng.layers}
    assert by[15].border is not None and by[15].q8_slim and by[14].q8_slim and by[22].q8_slim
    over = []
    check_blocks(s, eng, [14, 15, 22], over)
    assert not over, "; ".join(over)


def test_slim60_fp8_sparse_precision(dev, tmp_path):
    """"fp8-2:4" on the 60 % slim model after nm_prune: it runs, blocks with a table or a ragged cin take the dense fp8 kernel
    (none of them is in fp8_sparse_layers) and fp8_layers is what "fp8" gives."""
    _, m, _, _, s = build(dev, 60.0, tmp_path)
    s.set_masks(nm_prune(s))
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        s.precision = "fp8"
        a = s(x)
        dense_layers = list(engine_for(s, x).fp8_layers)
        s.precision = "fp8-2:4"
        b = s(x)
        eng = engine_for(s, x, "fp8-2:4")
    by = {lay.li + 1: lay for lay in eng.layers}
    assert eng.fp8_layers == dense_layers == expected_layers(m, s, eng)
    assert all(by[n].border is None and by[n].cin % 64 == 0 for n in eng.fp8_sparse_layers)
    assert bool(torch.isfinite(b).all())
    if not eng.fp8_sparse_layers:       # every launch is the dense fp8 one: the two precisions agree bit for bit
        assert torch.equal(a, b)
    over = []
    check_blocks(s, eng, [7, 14, 22], over)
    assert not over, "; ".join(over)


def test_slim60_fp8_allocation_mode_and_precision_switch(dev, slim60):
    _, _, _, _, s = slim60
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(10)).to(dev)
    try:
        s.precision = "fp8"
        s.train()
        with pytest.raises(McamdError):
            s(x)
        s.eval()
        with torch.no_grad():
            first = s(x).clone()
            s(x)
            torch.cuda.synchronize()
            before = torch.cuda.memory_stats(dev)
            s(x)
            torch.cuda.synchronize()
            after = torch.cuda.memory_stats(dev)
            assert after["num_alloc_retries"] == before["num_alloc_retries"]
            assert after["segment.all.allocated"] == before["segment.all.allocated"]
            s.precision = "fp16"
            d = s(x).clone()
            assert engine_for(s, x, "fp16").fp8_layers == []
            s.precision = "fp8"
            again = s(x)
            assert torch.equal(again, first), "fp8 -> fp16 -> fp8 reproduces the first result bit for bit"
            assert not torch.equal(d, first)
    finally:
        s.eval()
        s.precision = "auto"
