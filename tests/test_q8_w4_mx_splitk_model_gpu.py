"""Darknet.precision = "fp8-w4-mx-splitk": the low-batch form of the "fp8-w4-mx" engine (csrc/conv_q8_w4_mx.hip,
engine._Q8W4MxSplitK) on the small seeded YOLOv2-VOC of the sibling model tests -- which blocks split at B = 1,
the logits against "fp8-w4-mx" beside what the fp8 pair's summation order costs, a batch the policy leaves alone, the "w4"
model file round trip and the precision's rules."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from util import rel_l2  # noqa: E402
import test_q8_w4_model_gpu as M  # noqa: E402  (helpers only: model, engine_for, EXPECTED)

NEW = "fp8-w4-mx-splitk"
SPLIT_B1 = [9, 11] + list(range(13, 21)) + [22]


def _run(m, x, prec):
    m.precision = prec
    with torch.no_grad():
        out = m(x).clone()
    return M.engine_for(m, x, prec), out


def test_b1_split_layers_logits_and_model_file(dev, setenv, tmp_path):
    # (the fp8 pair in the fp8-MFMA form: the instruction whose arithmetic the fp4 operand shares)
    setenv("MCAMD_Q8_MFMA", "1")
    m = M.model(dev)[1]
    x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(5)).to(dev)
    _, q = _run(m, x, "fp8")
    esk, sk = _run(m, x, "fp8-splitk")
    emx, mx = _run(m, x, "fp8-w4-mx")
    ex, got = _run(m, x, NEW)
    assert ex.fp8_w4_mx_splitk_layers == esk.fp8_splitk_layers == SPLIT_B1
    assert ex.fp8_w4_mx_layers == ex.fp8_layers == M.EXPECTED and ex.fp8_splitk_layers == [] and ex.splitk_layers == []
    assert emx.fp8_w4_mx_splitk_layers == [] and emx.fp8_w4_mx_layers == M.EXPECTED
    for lay in ex.layers:
        n = lay.li + 1
        assert lay.form == ("q8_w4_mx_splitk" if n in SPLIT_B1 else "q8_w4_mx" if n in M.EXPECTED else "dense"), n
        assert (lay.sk_slices >= 2) == (n in SPLIT_B1) and not (lay.form == "q8_w4_mx_splitk" and lay.geom_q8.pad)
    d_pair, d_new = rel_l2(sk.cpu(), q.cpu()), rel_l2(got.cpu(), mx.cpu())
    print("B=1 rel-L2 by summation order: fp8-splitk from fp8 %.3g, %s from fp8-w4-mx %.3g" % (d_pair, NEW, d_new))
    assert bool(torch.isfinite(got).all()) and d_new <= 2.0 * d_pair, (d_new, d_pair)
    with torch.no_grad():
        assert torch.equal(m(x), got), "the replayed plan differs from the recorded forward"
    # a model and its reloaded "w4" model file run on equal operands
    path = str(tmp_path / "m.mcz")
    m.save_compressed(path, "w4", ex.fp8_w4_mx_layers)
    r = nets.Darknet(YOLOV2_VOC_CFG)
    r.to(dev)
    r.load_weights(path)
    r.eval()
    er, again = _run(r, x, NEW)
    assert er.fp8_w4_mx_splitk_layers == SPLIT_B1 and torch.equal(again, got)
    # the rules of "fp8-w4-mx"
    m.train()
    with pytest.raises(McamdError, match=NEW):
        m(x)
    m.eval()
    for name, value, off in (("sparse", "2:4", None), ("splitk", True, False)):
        setattr(m, name, value)
        with torch.no_grad(), pytest.raises(McamdError, match=NEW):
            m(x)
        setattr(m, name, off)


def test_b8_runs_exactly_the_unsplit_launches(dev):
    m = M.model(dev)[1]
    x = torch.rand(8, 3, 416, 416, generator=torch.Generator().manual_seed(6)).to(dev)
    _, mx = _run(m, x, "fp8-w4-mx")
    ex, got = _run(m, x, NEW)
    assert ex.fp8_w4_mx_splitk_layers == [] and ex.fp8_w4_mx_layers == M.EXPECTED
    assert torch.equal(got, mx)
