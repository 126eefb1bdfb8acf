"""Darknet.precision = "fp8-qat": fp8 quantisation-aware training on tests/golden/q8_qat.cfg -- every kernel of a
training step teacher-forced against the restatement (q8_qat_ref.py) from the engine's own tensors, the error level of the
train-mode logits, the eval path (the "fp8" engine bit for bit), a short training run, bit reproducibility with and without
launch plans, and one YOLOv2-VOC step at the real shapes."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, ops, YOLOV2_VOC_CFG, _lib as L  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import weight_prune  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2, nchw_to_raw  # noqa: E402
import q8_ref as R  # noqa: E402
import q8_qat_ref as Q  # noqa: E402

CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "q8_qat.cfg")
EXPECTED = list(range(3, 11))        # conv3 ... conv10 of q8_qat.cfg
TOL = 1e-3


def model(dev, seed=0, cfg=CFG, masked=False, prec="fp8-qat"):
    blocks = O.parse_cfg(cfg)
    m = nets.Darknet(cfg)
    m.load_state_dict(O.init_state(blocks, seed=seed))
    m.to(dev)
    m.precision = prec
    if masked:
        m.set_masks(weight_prune(m, 60.0))
    return blocks, m


def train_engine(m):
    return [e for e in m._engines.values() if e.train_layout and e.precision == "fp8-qat"][0]


def train_step(m, x, seed):
    m.train()
    out = m(x)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed))
    m.zero_grad()
    out.backward(gout.to(x.device))
    return out.detach().cpu()


def check_raw(io, conv, what, images=None, mfma=False):
    """The engine's fp32 y against the float64 restatement from the engine's own input codes."""
    mask = conv.mask.cpu() if conv.mask_flag else None
    w8, e = R.quantise_weights(conv.weight.data.cpu(), mask)
    assert torch.equal(io["wexp"], e), what + ": exponents"
    sel = slice(None) if images is None else images
    a8, y = io["x8"][sel], io["y"][sel]
    y_ref = Q.raw(a8, w8, e)
    if mfma:
        err, bar = rel_l2(y, y_ref), TOL
    else:
        k = w8.shape[-1]
        cpu_err = rel_l2(F.conv2d(Q.x_q(a8), Q.w_q(w8, e), None, 1, (k - 1) // 2), y_ref)
        err, bar = rel_l2(y, y_ref), max(1e-6, 4 * cpu_err)
    print("%s: y rel-L2 %.3g (bar %.3g)" % (what, err, bar))
    assert err <= bar, what
    return w8, e, mask


def teacher_forced(dev, seed, masked, mfma=False, only=None):
    """One training step; for every fp8 block, each kernel against the restatement fed with the ENGINE'S OWN tensors."""
    blocks, m = model(dev, seed=seed, masked=masked)
    B = 2
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(seed + 100)).to(dev)
    train_step(m, x, seed + 200)
    eng = train_engine(m)
    assert eng.fp8_layers == EXPECTED
    S = eng.grad_scale
    for c in (only or eng.fp8_layers):
        lay, io, what = eng.layers[c - 1], eng.qat_block_io(c), "conv%d" % c
        conv, bn = lay.conv, lay.bn
        w8, e, mask = check_raw(io, conv, what, mfma=mfma)
        # what the weight gradient multiplies is what the forward multiplied
        assert torch.equal(io["x16"], Q.x_q(io["x8"])), what + ": fp16 input is not deq(code) / 2"
        # batch statistics of the engine's own y
        scale, shift, mean, var = Q.batch_coeffs(io["y"], bn.weight.detach().cpu(), bn.bias.detach().cpu(), bn.eps)
        assert rel_l2(io["scale"], scale) < 1e-5 and float((io["shift"] - shift).abs().max()) < 1e-5 * (1 + float(shift.abs().max()))
        # output codes from its own y and ITS coefficients
        v = Q.act(io["y"], io["scale"], io["shift"], R.SLOPE if io["slope"] != 1.0 else 1.0)
        for o8, o16, dst, name in ((io["out8"], io["out16"], io["dst"], "out"), (io["out2_8"], io["out2_16"], "plain", "out2")):
            if o16 is None:
                continue
            if o8 is not None:
                share, adjacent = R.byte_mismatch(o8, R.store_bytes(v, dst))
                print("%s %s: byte mismatch share %.3g" % (what, name, share))
                assert adjacent and share <= R.MISMATCH_CAP, what + " " + name
                assert torch.equal(o16, R.deq(o8) / 2.0), what + " " + name + ": fp16 twin"
            else:
                assert rel_l2(o16, R.store_fp16(v, dst)) < TOL, what + " " + name
        # backward of BatchNorm + LeakyReLU + pool / reorg / route from the saved fp32 y and the engine's G
        ot = lay.out_t
        cons = eng.consumer_of[lay.out_id]
        cd = ot.C
        G = cons.gin.view(B, ot.H, ot.W, cons.tin.ld)[..., ot.choff:ot.choff + cd].permute(0, 3, 1, 2).float().cpu() / S
        G2 = c2 = t2 = None
        if lay.out2_id is not None and lay.out2_id in eng.consumer_of:
            c2, t2 = eng.consumer_of[lay.out2_id], lay.out2_t
            G2 = c2.gin.view(B, lay.H, lay.W, c2.tin.ld)[..., t2.choff:t2.choff + t2.C].permute(0, 3, 1, 2).float().cpu() / S
        yl = io["y"].double().requires_grad_(True)
        gam = bn.weight.detach().cpu().double().requires_grad_(True)
        bet = bn.bias.detach().cpu().double().requires_grad_(True)
        z = F.batch_norm(yl, None, None, gam, bet, True, 0.1, bn.eps)
        # LeakyReLU is not differentiable at 0: elements within rounding of it are taken out on both sides (G zeroed there,
        # the product's backward entry point issued again), as tests/test_model_gpu.py does
        kink = z.detach().abs() < 1e-5
        eng_dy, eng_dg, eng_db = lay.dy, bn.weight.grad, bn.bias.grad
        if bool(kink.any()):
            kg = kink.float()
            badG = (F.max_pool2d(kg, 2, 2) if lay.mode == L.DST_POOL else O.reorg(kg, 2) if lay.mode == L.DST_REORG else kg) > 0
            G = G.masked_fill(badG, 0.0)
            if G2 is not None:
                G2 = G2.masked_fill(kink, 0.0)
            gbuf = nchw_to_raw(G * S, cons.tin.ld, ot.choff)
            g2buf = nchw_to_raw(G2 * S, c2.tin.ld, t2.choff) if G2 is not None else None
            eng_dy = ops.alloc_padded(B, lay.H, lay.W, lay.cout_p, dev, pad=lay.pad)
            eng_dg, eng_db = bn.weight.grad.clone(), bn.bias.grad.clone()
            eng.bn_act_bwd_layer(lay, gbuf, cons.tin.ld, ot.choff, g2buf, c2.tin.ld if c2 is not None else 0,
                                 t2.choff if t2 is not None else 0, eng_dy, eng_dg, eng_db, S)
        a = F.leaky_relu(z, lay.slope)
        o = F.max_pool2d(a, 2, 2) if lay.mode == L.DST_POOL else O.reorg(a, 2) if lay.mode == L.DST_REORG else a
        loss = (o * G.double()).sum()
        if G2 is not None:
            loss = loss + (a * G2.double()).sum()
        loss.backward()
        dy = ops.padded_view(eng_dy, B, lay.H, lay.W, lay.cout_p, lay.pad)[:, 1:-1, 1:-1, :lay.cout].permute(0, 3, 1, 2).float().cpu() / S
        errs = (rel_l2(dy, yl.grad), rel_l2(eng_dg.cpu(), gam.grad), rel_l2(eng_db.cpu(), bet.grad))
        print("%s: bn_act_bwd %.3g dgamma %.3g dbeta %.3g" % ((what,) + errs))
        assert max(errs) < 2e-3, what
        # straight-through: dX = dgrad(dY, w_q), dW = wgrad(dY, x_q) * mask, from the step's own dY
        dY = io["dy"].double() / S
        wq = Q.w_q(w8, e)
        assert torch.equal(io["w_q"], wq), what + ": w_q"
        assert torch.equal(wq.half().float(), wq), what + ": fp16(w_q) is exact"
        pad = (lay.k - 1) // 2
        xq = io["x16"].double()
        dx_ref = torch.nn.grad.conv2d_input(xq.shape, wq.double(), dY, 1, pad)
        dw_ref = torch.nn.grad.conv2d_weight(xq, wq.shape, dY, 1, pad)
        if mask is not None:
            dw_ref = dw_ref * mask.double()
        dw = conv.weight.grad.cpu()
        e_dx, e_dw = rel_l2(io["gin"] / S, dx_ref), rel_l2(dw, dw_ref)
        print("%s: dX %.3g dW %.3g" % (what, e_dx, e_dw))
        assert e_dx < TOL and e_dw < TOL, what
        if mask is not None:
            assert bool((dw[mask == 0] == 0).all()), what + ": masked positions of dW"
    return blocks, m, eng, x


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "weight60"])
def test_teacher_forced_training_step(dev, masked):
    teacher_forced(dev, 3 + int(masked), masked)


def test_teacher_forced_training_step_fp8_mfma(dev, setenv):
    setenv("MCAMD_Q8_MFMA", "1")
    teacher_forced(dev, 5, True, mfma=True)


def test_fp16_to_fp8_edge_block(dev):
    """conv3 reads conv2's fp16 output through the training cast: its codes are q(2 x16) of what conv2 wrote, the fp16
    slice holds deq(code) / 2 afterwards, and conv2 -- an fp16 block -- wrote fp16(v) and trains as in the "fp16" engine."""
    blocks, m, eng, x = teacher_forced(dev, 7, False, only=[3])
    by = {lay.li + 1: lay for lay in eng.layers}
    assert by[3].xq is not None and all(by[c].xq is None for c in range(4, 11))
    assert not by[2].q8_on and by[2].y.dtype == torch.float16
    io = eng.qat_block_io(3)
    # conv2's activation pass recomputed from its own fp16 y: the slice holds the dequantised codes of THAT fp16 tensor
    l2 = by[2]
    y2 = l2.y.view(2, l2.H, l2.W, l2.cout).permute(0, 3, 1, 2).float().cpu()
    v2 = Q.act(y2, l2.scale.cpu(), l2.shift.cpu(), R.SLOPE)
    codes, back = Q.cast_train(R.store_fp16(v2))
    share, adjacent = R.byte_mismatch(io["x8"], codes)
    print("edge: code mismatch share %.3g" % share)
    assert adjacent and share <= R.MISMATCH_CAP     # (fp32 against float64 evaluation of v moves a code only at a tie)
    assert torch.equal(io["x16"], R.deq(io["x8"]) / 2.0)
    # the same model under "fp16": conv1 and conv2 run identical kernels on identical inputs
    m.precision = "fp16"
    train_step(m, x, 207)
    e16 = [e for e in m._engines.values() if e.train_layout and e.precision == "fp16"][0]
    assert torch.equal(e16.layers[1].y, l2.y), "conv2's raw output differs from the fp16 engine's"


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "weight60"])
def test_train_logits_error_level(dev, masked):
    """e_engine <= 1.10 e_ref against the fp32 oracle's train-mode logits (the bar test_q8_model_gpu.py uses for eval)."""
    blocks, m = model(dev, seed=1, masked=masked)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    state = {k: v.cpu().clone() for k, v in m.state_dict().items()}
    cm = [mod[0].mask.cpu() for mod in m.models if isinstance(mod, torch.nn.Sequential) and hasattr(mod[0], "mask_flag")] if masked else None
    m.train()
    with torch.no_grad():
        got = m(x.to(dev)).cpu()
        ref32 = O.forward(blocks, state, x, training=True, masks=cm)
        ref8 = Q.forward_train(blocks, state, x, EXPECTED, masks=cm)
    e_engine, e_ref = rel_l2(got, ref32), rel_l2(ref8, ref32)
    print("train logits: engine %.4f, restatement %.4f against the fp32 oracle (ratio %.3f)" % (e_engine, e_ref, e_engine / e_ref))
    assert train_engine(m).fp8_layers == EXPECTED
    assert e_engine <= 1.10 * e_ref


def test_eval_is_the_fp8_engine_and_other_precisions_still_refuse_training(dev):
    blocks, m = model(dev, seed=2, masked=True)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(11)).to(dev)
    m.eval()
    with torch.no_grad():
        q = m(x)
        ev = [e for e in m._engines.values() if not e.train_layout and e.precision == "fp8-qat"][0]
        m.precision = "fp8"
        p = m(x)
        e8 = [e for e in m._engines.values() if not e.train_layout and e.precision == "fp8"][0]
    assert torch.equal(q, p), "eval under fp8-qat is not the fp8 engine bit for bit"
    assert ev.fp8_layers == e8.fp8_layers == EXPECTED
    m.precision = "fp8-qat"
    train_step(m, x, 12)
    assert train_engine(m).fp8_layers == ev.fp8_layers
    for prec in ("fp8", "fp8-2:4"):
        m.precision = prec
        m.train()
        with pytest.raises(McamdError, match="inference only"):
            m(x)


def _run_steps(dev, prec, steps=20):
    blocks, m = model(dev, seed=4, masked=True, prec=prec)
    from modelcompression_amd.synthetic import synthetic_batch
    B = 2
    x = synthetic_batch(B, 64, 64, seed=1, device=dev)
    g = torch.Generator().manual_seed(3)
    target = torch.zeros(B, 250)
    for b in range(B):
        for k in range(3):
            target[b, 5 * k:5 * k + 5] = torch.tensor([float(torch.randint(0, 20, (1,), generator=g)),
                                                       *(0.2 + 0.6 * torch.rand(2, generator=g)).tolist(),
                                                       *(0.1 + 0.3 * torch.rand(2, generator=g)).tolist()])
    target = target.to(dev)
    masks = [mod[0].mask.clone() for mod in m.models if isinstance(mod, torch.nn.Sequential) and hasattr(mod[0], "mask_flag")]
    opt = torch.optim.SGD(m.parameters(), lr=1e-4 / B, momentum=0.9, weight_decay=0.0005 * B)
    m.train()
    losses = []
    for _ in range(steps):
        out = m(x)
        loss = m.loss(out, target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return m, masks, losses, x


def test_short_training_run(dev):
    """Twenty SGD steps on one fixed synthetic batch with RegionLoss."""
    m, masks, losses, x = _run_steps(dev, "fp8-qat")
    _, _, losses16, _ = _run_steps(dev, "fp16")
    print("loss ratio after 20 steps: fp8-qat %.4f (%.4f -> %.4f), fp16 %.4f (%.4f -> %.4f)"
          % (losses[-1] / losses[0], losses[0], losses[-1], losses16[-1] / losses16[0], losses16[0], losses16[-1]))
    assert all(l == l and abs(l) < 1e9 for l in losses), "loss not finite"
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    convs = [p for p in m.parameters() if p.dim() == 4]
    for p, mk in zip(convs, masks):
        assert bool((p.detach()[mk == 0] == 0).all()), "a masked weight moved"
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 20, k
    if losses16[-1] < losses16[0]:
        assert losses[-1] < losses[0]
    m.precision = "fp8"
    m.eval()
    with torch.no_grad():
        out = m(x)
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("plan", ["1", "0"], ids=["plans", "no-plans"])
def test_training_step_is_bit_reproducible(dev, monkeypatch, plan):
    monkeypatch.setenv("MCAMD_PLAN", plan)       # read once per engine
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(21)).to(dev)
    grads = []
    for _ in range(2):
        _, m = model(dev, seed=6, masked=True)
        outs = [train_step(m, x, 22), train_step(m, x, 22)]      # (the second step replays the recorded plans)
        assert train_engine(m).use_plan == (plan == "1")
        grads.append([outs[1]] + [p.grad.detach().cpu().clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_yolov2_step_at_real_shapes(dev):
    """One YOLOv2-VOC step at B = 2, 416x416: the index arithmetic at real sizes, every fp8 block's y on image 0."""
    blocks, m = model(dev, seed=0, cfg=YOLOV2_VOC_CFG)
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(31)).to(dev)
    out = train_step(m, x, 32)
    eng = train_engine(m)
    assert eng.fp8_layers == list(range(3, 23))
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    for c in eng.fp8_layers:
        check_raw(eng.qat_block_io(c), eng.layers[c - 1].conv, "conv%d" % c, images=slice(0, 1))
