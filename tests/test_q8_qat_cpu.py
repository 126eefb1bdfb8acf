"""CPU checks of fp8 quantisation-aware training (Darknet.precision = "fp8-qat"): the restatement
(q8_qat_ref.py) against q8_ref.py and against float64 autograd, the fp16 exactness of the dgrad operand, and the new entry
points."""
import os
import re
import subprocess
import sys

import torch
import torch.nn.functional as F

from modelcompression_amd import _lib, ops
import q8_ref as R
import q8_qat_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mcamd_conv_fwd_q8_stats_rows", "mcamd_fakequant_q8", "mcamd_cast_q8_train")
# (cin, cout, k): the distinct filter shapes of conv3 ... conv22 of yolov2-voc
YOLO_FILTERS = [(64, 128, 3), (128, 64, 1), (128, 256, 3), (256, 128, 1), (256, 512, 3), (512, 256, 1), (512, 1024, 3),
                (1024, 512, 1), (1024, 1024, 3), (512, 64, 1), (1280, 1024, 3)]


def _operands(seed, B, cin, cout, k, H, W, masked):
    gen = torch.Generator().manual_seed(seed)
    a8 = R.q(2.0 * F.leaky_relu(torch.randn(B, cin, H, W, generator=gen), 0.1))
    w = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    mask = (torch.rand(cout, cin, k, k, generator=gen) < 0.5).float() if masked else None
    gamma, beta = torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.2
    return a8, w, mask, gamma, beta


def test_qat_entry_points_are_exported():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    assert "dst_q8" in hdr and "dst2_q8" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mcamd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert [f[0] for f in _lib.ActDesc._fields_][-2:] == ["dst_q8", "dst2_q8"]
    for fn in ("conv_fwd_q8_raw", "conv_fwd_q8_stats_rows", "fakequant_q8"):
        assert hasattr(ops, fn), fn


def test_stats_rows_query_host_logic():
    """One slab row per tile of 128 pixels; 0 for a geometry without an fp8 form."""
    for B, H, W in ((2, 9, 11), (1, 13, 13), (2, 26, 26), (64, 104, 104)):
        g = ops.geom(B, H, W, 3, 64, 128, 64)
        assert ops.conv_fwd_q8_stats_rows(g) == (B * H * W + 127) // 128
    assert ops.conv_fwd_q8_stats_rows(ops.geom(1, 16, 16, 3, 32, 64, 32)) == 0


def test_training_block_equals_q8_ref_block_code_for_code():
    """With scale / shift taken from the batch statistics of its own y, the training block IS q8_ref.block: the same codes
    in every destination form, and fp16 twins that hold deq(code) / 2 exactly."""
    for seed, (cin, cout, k, masked) in enumerate([(64, 72, 3, False), (128, 64, 1, True), (192, 128, 3, True)]):
        a8, w, mask, gamma, beta = _operands(seed, 2, cin, cout, k, 10, 12, masked)
        w8, e = R.quantise_weights(w, mask)
        y, scale, shift, v = Q.train_block(a8, w8, e, gamma, beta)
        v_ref = R.block(a8, w8, e, scale, shift, R.SLOPE)
        # the batch statistics are the ones nn.BatchNorm2d takes
        bn = torch.nn.BatchNorm2d(cout).double()
        bn.weight.data.copy_(gamma), bn.bias.data.copy_(beta)
        z = bn(y.double()).detach()
        assert float((z - (y.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))).abs().max()) < 1e-5
        for dst in ("plain", "pool", "reorg"):
            codes, twin = Q.store_pair(v, dst)
            assert torch.equal(codes, R.store_bytes(v_ref, dst)), (seed, dst)
            assert torch.equal(twin.half().float(), twin), "the fp16 twin holds deq(code) / 2 exactly"
        # y is the convolution of the dequantised operands
        yc = F.conv2d(Q.x_q(a8).double(), Q.w_q(w8, e).double(), None, 1, (k - 1) // 2)
        assert float((yc - y).abs().max()) <= 1e-12 * float(y.abs().max())


def test_straight_through_gradients_equal_float64_autograd_at_the_quantised_point():
    """QatConv's dX / dW are the gradients of the UNQUANTISED convolution evaluated at (x_q, w_q) (times the mask)."""
    for seed, (cin, cout, k, masked) in enumerate([(64, 24, 3, True), (64, 16, 1, False)]):
        gen = torch.Generator().manual_seed(40 + seed)
        x = F.leaky_relu(torch.randn(2, cin, 7, 9, generator=gen), 0.1).double().requires_grad_()
        w = (torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5).double().requires_grad_()
        mask = (torch.rand(cout, cin, k, k, generator=gen) < 0.5).double() if masked else None
        G = torch.randn(2, cout, 7, 9, generator=gen).double()
        out = Q.QatConv.apply(x, w, mask)
        (out * G).sum().backward()
        w8, e = R.quantise_weights(w.detach().float(), mask.float() if masked else None)
        xq = Q.x_q(R.q(2.0 * x.detach())).double().requires_grad_()
        wq = Q.w_q(w8, e).double().requires_grad_()
        ref = F.conv2d(xq, wq, None, 1, (k - 1) // 2)
        assert torch.equal(out.detach(), ref.detach())
        (ref * G).sum().backward()
        dw_ref = wq.grad * mask if masked else wq.grad
        assert float((x.grad - xq.grad).norm() / xq.grad.norm()) < 1e-12
        assert float((w.grad - dw_ref).norm() / dw_ref.norm()) < 1e-12
        if masked:
            assert bool((w.grad[mask == 0] == 0).all())


def test_fp16_holds_w_q_exactly_on_he_initialised_yolov2_filters():
    """The dgrad operand fp16(w_q) is w_q itself for initialisation-sized weights; scaled by 1/300 (below anything BatchNorm
    training produces) the loss stays under 5e-5 rel-L2, far inside the dgrad tolerance."""
    gen = torch.Generator().manual_seed(7)
    for cin, cout, k in YOLO_FILTERS:
        w = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
        wq = Q.fakequant(w)
        assert torch.equal(wq.half().float(), wq), (cin, cout, k)
        small = Q.fakequant(w / 300.0)
        loss = float((small.half().float() - small).double().norm() / small.double().norm())
        assert loss < 5e-5, (cin, cout, k, loss)


def test_cast_train_restatement():
    gen = torch.Generator().manual_seed(3)
    x16 = (torch.randn(4000, generator=gen) * 3).half()
    x16[0] = 300.0
    codes, back = Q.cast_train(x16)
    assert torch.equal(codes, R.q(2.0 * x16.float()))
    assert torch.equal(back.half().float(), back) and float(back[0]) == 224.0
    assert torch.equal(Q.cast_train(back.half())[0], codes), "the written-back values quantise to the same codes"


def test_precision_env_reaches_darknet():
    env = dict(os.environ, MCAMD_PRECISION="fp8-qat")
    code = ("from modelcompression_amd import nets, YOLOV2_VOC_CFG; m = nets.Darknet(YOLOV2_VOC_CFG); print(m.precision)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "fp8-qat"


def test_fixture_cfg_block_kinds():
    """tests/golden/q8_qat.cfg holds every kind of fp8 block the training path has."""
    from oracle import darknet_ref as O
    plan = O.plan(O.parse_cfg(os.path.join(ROOT, "tests", "golden", "q8_qat.cfg")))
    fmt = R._formats(plan, list(range(3, 11)))
    convs = {op["id"]: (i, op) for i, op in enumerate(plan) if op["type"] == "conv"}
    assert all(convs[i][1]["cin"] % 64 == 0 for i in range(3, 11)) and convs[2][1]["cin"] == 32
    assert convs[10][1]["cin"] == 192 and convs[4][1]["k"] == 1
    assert fmt[convs[3][0]] and fmt[6] and fmt[8] and fmt[9] and fmt[13]      # plain, pool, y2, pool + y2, reorg as bytes
    assert not fmt[convs[2][0]] and not fmt[convs[10][0]]                    # the fp16 -> fp8 edge; the fp8 -> fp16 edge
