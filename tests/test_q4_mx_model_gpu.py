"""Darknet.precision = "fp4-mx": the "fp8-w4-mx" engine of YOLOv2-VOC with MXFP4 activations in front of its fp4-operand blocks
(csrc/conv_q4_mx.hip, engine._Q4Mx) -- which blocks take the form, Darknet.fp4_skip, determinism, the "w4" model
file round trip, the precision's rules and the error level against the fp32 oracle.  Seed-1 random-init weights, B = 1."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402
import test_q8_w4_model_gpu as M  # noqa: E402  (helpers only: model, engine_for, EXPECTED)

# logits' rel-L2 from the fp32 oracle, measured on an MI355X ("fp8-w4-mx" 0.356, "fp8" 0.130 on the same model and input).  The run
# is deterministic; the margin of 1.25 is for toolchain changes that move single-code flips.
MEASURED = 0.4666


@pytest.fixture(scope="module")
def runs(dev):
    """(model, input, run(precision, skip) -> (engine, logits), the "fp8-w4-mx" logits)"""
    _, m = M.model(dev)
    x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(5)).to(dev)

    def run(prec, skip=(), model=None):
        mm = model or m
        mm.precision, mm.fp4_skip = prec, skip
        with torch.no_grad():
            out = mm(x).cpu()
        return M.engine_for(mm, x, prec), out

    return m, x, run, run("fp8-w4-mx")[1]


def test_default_layers_determinism_and_model_file(runs, dev, tmp_path):
    m, x, run, _ = runs
    eng, got = run("fp4-mx")
    assert eng.fp4_layers == eng.fp8_w4_mx_layers == M.EXPECTED
    assert all(lay.form == ("q4_mx" if lay.li + 1 in M.EXPECTED else "dense") for lay in eng.layers)
    assert bool(torch.isfinite(got).all()) and torch.equal(run("fp4-mx")[1], got), "two forwards are bit-equal"
    path = str(tmp_path / "m.mcz")
    m.save_compressed(path, "w4", eng.fp8_w4_mx_layers)
    r = nets.Darknet(YOLOV2_VOC_CFG)
    r.to(dev)
    r.load_weights(path)
    r.eval()
    assert torch.equal(run("fp4-mx", model=r)[1], got), "a \"w4\" model file round trip"


def test_skipping_every_block_is_fp8_w4_mx(runs):
    _, _, run, mx = runs
    eng, got = run("fp4-mx", skip=tuple(M.EXPECTED))
    assert eng.fp4_layers == [] and eng.fp8_w4_mx_layers == M.EXPECTED and torch.equal(got, mx)


@pytest.mark.parametrize("conv", [3, 10, 21])        # behind the fp16 -> fp8 edge cast; a 1x1 block; the route input, cin 1280
def test_one_block(runs, conv):
    _, _, run, mx = runs
    eng, got = run("fp4-mx", skip=[c for c in M.EXPECTED if c != conv])
    assert eng.fp4_layers == [conv] and eng.fp8_w4_mx_layers == M.EXPECTED
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, mx)


def test_rules(runs):
    m, x, run, _ = runs
    m.precision, m.fp4_skip = "fp4-mx", ()
    m.train()
    with pytest.raises(McamdError, match="fp4-mx"):
        m(x)
    m.eval()
    for name, value, off in (("sparse", "2:4", None), ("splitk", True, False), ("lowrank", True, False)):
        setattr(m, name, value)
        with torch.no_grad(), pytest.raises(McamdError, match="fp4-mx"):
            m(x)
        setattr(m, name, off)


def test_error_level(runs):
    m, x, run, mx = runs
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    with torch.no_grad():
        ref32 = O.forward(blocks, {k: v.cpu() for k, v in m.state_dict().items()}, x.cpu(), training=False)
    e4, e_mx = rel_l2(run("fp4-mx")[1], ref32), rel_l2(mx, ref32)
    e_late = rel_l2(run("fp4-mx", skip=tuple(range(3, 9)))[1], ref32)
    print("logits rel-L2 from the fp32 oracle: fp4-mx %.4f, fp4-mx with fp4_skip = conv3-conv8 %.4f, fp8-w4-mx %.4f" % (e4, e_late, e_mx))
    assert e4 < 1.0 and e4 <= 1.25 * MEASURED
