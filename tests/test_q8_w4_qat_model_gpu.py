"""Darknet.precision = "fp8-w4-qat": 4-bit quantisation-aware training on tests/golden/q8_qat.cfg -- the forms
of the training engine, every kernel of a training step teacher-forced against the restatement (w4_qat_ref.py) from the engine's
own tensors with test_q8_qat_model_gpu.py's bars, equality in training with an "fp8-qat" model that holds the dequantised
weights, the eval path (the "fp8-w4" engine bit for bit), the error level of the train-mode logits, a short training run, bit
reproducibility with and without launch plans, one YOLOv2-VOC step at the real shapes and one distillation step."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, ops, YOLOV2_VOC_CFG, _lib as L  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2, nchw_to_raw  # noqa: E402
import q8_ref as R  # noqa: E402
import q8_qat_ref as Q  # noqa: E402
import w4_ref as W  # noqa: E402
import w4_qat_ref as Q4  # noqa: E402
import test_q8_qat_model_gpu as T8  # noqa: E402  (helpers only: model, train_step, _run_steps, CFG, EXPECTED, TOL)

PREC = "fp8-w4-qat"
EXPECTED, TOL = T8.EXPECTED, T8.TOL


def model(dev, seed=0, cfg=T8.CFG, masked=False, prec=PREC):
    return T8.model(dev, seed=seed, cfg=cfg, masked=masked, prec=prec)


def train_engine(m, prec=PREC):
    return [e for e in m._engines.values() if e.train_layout and e.precision == prec][0]


def convs_of(m):
    return [mod[0] for mod in m.models if isinstance(mod, torch.nn.Sequential) and hasattr(mod[0], "mask_flag")]


def check_operands_and_raw(io, conv, what, images=None, mfma=False):
    """The engine's codes, shift bytes and exponents against w4_ref (exactly), its fp32 y against the float64 restatement from
    the engine's own input codes (test_q8_qat_model_gpu.check_raw's bars)."""
    mask = conv.mask.cpu() if conv.mask_flag else None
    w = conv.weight.data.cpu()
    codes, g, e4, values, w8 = W.quantise(w, mask)
    assert torch.equal(io["wexp"], e4), what + ": exponents"
    assert torch.equal(io["gshift"], W.shift_rows(g)), what + ": shift bytes"
    assert torch.equal(io["codes"], W.code_rows(codes)), what + ": codes"
    sel = slice(None) if images is None else images
    a8, y = io["x8"][sel], io["y"][sel]
    y_ref = Q.raw(a8, w8, e4)
    if mfma:
        err, bar = rel_l2(y, y_ref), TOL
    else:
        k = w8.shape[-1]
        cpu_err = rel_l2(F.conv2d(Q.x_q(a8), Q.w_q(w8, e4), None, 1, (k - 1) // 2), y_ref)
        err, bar = rel_l2(y, y_ref), max(1e-6, 4 * cpu_err)
    print("%s: y rel-L2 %.3g (bar %.3g)" % (what, err, bar))
    assert err <= bar, what
    return w8, e4, mask


def teacher_forced(dev, seed, masked, mfma=False):
    """test_q8_qat_model_gpu.teacher_forced for w4 blocks: one training step; for every fp8 block, each kernel against the
    restatement fed with the ENGINE'S OWN tensors."""
    blocks, m = model(dev, seed=seed, masked=masked)
    B = 2
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(seed + 100)).to(dev)
    T8.train_step(m, x, seed + 200)
    eng = train_engine(m)
    assert eng.fp8_w4_layers == eng.fp8_layers == EXPECTED
    S = eng.grad_scale
    for c in eng.fp8_layers:
        lay, io, what = eng.layers[c - 1], eng.qat_block_io(c), "conv%d" % c
        conv, bn = lay.conv, lay.bn
        w8, e4, mask = check_operands_and_raw(io, conv, what, mfma=mfma)
        assert torch.equal(io["x16"], Q.x_q(io["x8"])), what + ": fp16 input is not deq(code) / 2"
        scale, shift, mean, var = Q.batch_coeffs(io["y"], bn.weight.detach().cpu(), bn.bias.detach().cpu(), bn.eps)
        assert rel_l2(io["scale"], scale) < 1e-5 and float((io["shift"] - shift).abs().max()) < 1e-5 * (1 + float(shift.abs().max()))
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
        G = cons.gin.view(B, ot.H, ot.W, cons.tin.ld)[..., ot.choff:ot.choff + ot.C].permute(0, 3, 1, 2).float().cpu() / S
        G2 = c2 = t2 = None
        if lay.out2_id is not None and lay.out2_id in eng.consumer_of:
            c2, t2 = eng.consumer_of[lay.out2_id], lay.out2_t
            G2 = c2.gin.view(B, lay.H, lay.W, c2.tin.ld)[..., t2.choff:t2.choff + t2.C].permute(0, 3, 1, 2).float().cpu() / S
        yl = io["y"].double().requires_grad_(True)
        gam = bn.weight.detach().cpu().double().requires_grad_(True)
        bet = bn.bias.detach().cpu().double().requires_grad_(True)
        z = F.batch_norm(yl, None, None, gam, bet, True, 0.1, bn.eps)
        kink = z.detach().abs() < 1e-5        # (LeakyReLU's kink taken out on both sides, as test_q8_qat_model_gpu.py does)
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
        wq = Q4.fakequant(conv.weight.data.cpu(), mask)
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


def _dequantised_twin(dev, ma, seed, masked):
    """Model B: the same network (and masks) with the weights of the w4 blocks replaced by the values their codes stand for."""
    _, mb = model(dev, seed=seed, masked=False, prec="fp8-qat")
    ca, cb = convs_of(ma), convs_of(mb)
    if masked:
        mb.set_masks([c.mask.clone() for c in ca])
    for c in EXPECTED:
        mask = ca[c - 1].mask.cpu() if ca[c - 1].mask_flag else None
        cb[c - 1].weight.data.copy_(Q4.fakequant(ca[c - 1].weight.data.cpu(), mask).to(dev))
    mb.invalidate_packed()
    return mb


def _step_state(m):
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
    stats = {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}
    return grads, stats


def _cross_engine(dev, seed, masked):
    _, ma = model(dev, seed=seed, masked=masked)
    mb = _dequantised_twin(dev, ma, seed, masked)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(seed + 300)).to(dev)
    oa, ob = T8.train_step(ma, x, seed + 400), T8.train_step(mb, x, seed + 400)
    assert train_engine(ma).fp8_layers == train_engine(mb, "fp8-qat").fp8_layers == EXPECTED
    assert train_engine(mb, "fp8-qat").fp8_w4_layers == []
    return oa, ob, _step_state(ma), _step_state(mb)


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "weight60"])
def test_training_equals_fp8_qat_on_the_dequantised_weights(dev, masked):
    """Model B holds w_q and trains one step under "fp8-qat": its bytes are exactly twice A's with exponent e4_f + 1, so S doubles
    exactly and the epilogue's power of two halves it; B's fake quantisation returns w_q itself, so the dgrad operand is the same.
    Train-mode logits, every conv and BatchNorm gradient and the running statistics are EQUAL in the default form."""
    oa, ob, (ga, sa), (gb, sb) = _cross_engine(dev, 8 + int(masked), masked)
    assert bool(torch.isfinite(oa).all()) and torch.equal(oa, ob), "train-mode logits differ in %d elements" % int((oa != ob).sum())
    assert set(ga) == set(gb) and set(sa) == set(sb)
    bad = [n for n in ga if not torch.equal(ga[n], gb[n])]
    assert not bad, "gradients differ: %s" % bad
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, "running statistics differ: %s" % bad
    assert any(bool((g != 0).any()) for g in ga.values())


def test_training_against_fp8_qat_on_the_dequantised_weights_fp8_mfma(dev, setenv):
    """MCAMD_Q8_MFMA=1: the fp8 MFMA's group truncation sees operands twice as large in B -- logits and gradients at the project's
    1e-3; whether they were equal as well is printed."""
    setenv("MCAMD_Q8_MFMA", "1")
    oa, ob, (ga, sa), (gb, sb) = _cross_engine(dev, 10, True)
    equal = torch.equal(oa, ob) and all(torch.equal(ga[n], gb[n]) for n in ga)
    print("fp8 MFMA: fp8-w4-qat against fp8-qat on the dequantised weights: equal = %s, logits rel-L2 %.3g" % (equal, rel_l2(oa, ob)))
    assert rel_l2(oa, ob) < TOL
    for n in ga:
        if float(gb[n].abs().max()) > 0:
            assert rel_l2(ga[n], gb[n]) < TOL, n


def test_eval_is_the_fp8_w4_engine_and_fp8_w4_still_refuses_training(dev):
    blocks, m = model(dev, seed=2, masked=True)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(11)).to(dev)
    m.eval()
    with torch.no_grad():
        q = m(x)
        ev = [e for e in m._engines.values() if not e.train_layout and e.precision == PREC][0]
        m.precision = "fp8-w4"
        p = m(x)
        e4 = [e for e in m._engines.values() if not e.train_layout and e.precision == "fp8-w4"][0]
    assert torch.equal(q, p), "eval under fp8-w4-qat is not the fp8-w4 engine bit for bit"
    assert ev.fp8_layers == e4.fp8_layers == ev.fp8_w4_layers == e4.fp8_w4_layers == EXPECTED
    m.precision = PREC
    T8.train_step(m, x, 12)
    assert train_engine(m).fp8_w4_layers == EXPECTED
    m.precision = "fp8-w4"
    m.train()
    with pytest.raises(McamdError, match="inference only"):
        m(x)
    # sparse and splitk stay off, and the refusals name the precision
    m.precision = PREC
    m.eval()
    for attr, val in (("sparse", "2:4"), ("splitk", True)):
        setattr(m, attr, val)
        with torch.no_grad(), pytest.raises(McamdError, match=PREC):
            m(x)
        setattr(m, attr, None if attr == "sparse" else False)


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "weight60"])
def test_train_logits_error_level(dev, masked):
    """e_engine <= 1.10 e_ref against the fp32 oracle's train-mode logits (the existing rule)."""
    blocks, m = model(dev, seed=1, masked=masked)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    state = {k: v.cpu().clone() for k, v in m.state_dict().items()}
    cm = [c.mask.cpu() for c in convs_of(m)] if masked else None
    m.train()
    with torch.no_grad():
        got = m(x.to(dev)).cpu()
        ref32 = O.forward(blocks, state, x, training=True, masks=cm)
        ref4 = Q4.forward_train(blocks, state, x, EXPECTED, masks=cm)
    e_engine, e_ref = rel_l2(got, ref32), rel_l2(ref4, ref32)
    print("train logits: engine %.4f, restatement %.4f against the fp32 oracle (ratio %.3f)" % (e_engine, e_ref, e_engine / e_ref))
    assert train_engine(m).fp8_layers == EXPECTED
    assert e_engine <= 1.10 * e_ref


def test_short_training_run(dev):
    """Twenty SGD steps on one fixed synthetic batch with RegionLoss (test_q8_qat_model_gpu._run_steps' recipe)."""
    m, masks, losses, x = T8._run_steps(dev, PREC)
    _, _, losses16, _ = T8._run_steps(dev, "fp16")
    print("loss ratio after 20 steps: fp8-w4-qat %.4f (%.4f -> %.4f), fp16 %.4f (%.4f -> %.4f)"
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
    m.precision = "fp8-w4"
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
        outs = [T8.train_step(m, x, 22), T8.train_step(m, x, 22)]      # (the second step replays the recorded plans)
        assert train_engine(m).use_plan == (plan == "1")
        grads.append([outs[1]] + [p.grad.detach().cpu().clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_yolov2_step_at_real_shapes(dev):
    """One YOLOv2-VOC step at B = 2, 416x416: the index arithmetic at real sizes, every w4 block's operands and y on image 0."""
    blocks, m = model(dev, seed=0, cfg=YOLOV2_VOC_CFG)
    x = torch.rand(2, 3, 416, 416, generator=torch.Generator().manual_seed(31)).to(dev)
    out = T8.train_step(m, x, 32)
    eng = train_engine(m)
    assert eng.fp8_w4_layers == eng.fp8_layers == list(range(3, 23))
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    for c in eng.fp8_layers:
        check_operands_and_raw(eng.qat_block_io(c), eng.layers[c - 1].conv, "conv%d" % c, images=slice(0, 1))


def test_one_distillation_step(dev):
    """One DistillLoss step toward an fp16 teacher's eval logits under the precision: a finite loss and finite gradients
    (train.py, StepGuard, dp.py, TEACHER= and DISTILL= need nothing new)."""
    from modelcompression_amd.distill import DistillLoss
    from modelcompression_amd.synthetic import synthetic_batch
    _, teacher = model(dev, seed=4, prec="fp16")
    _, student = model(dev, seed=4, masked=True)
    x = synthetic_batch(2, 64, 64, seed=1, device=dev)
    teacher.eval()
    with torch.no_grad():
        t = teacher(x)
    crit = DistillLoss.from_model(student).to(dev)
    student.train()
    out = student(x)
    loss = crit(out, t)
    student.zero_grad()
    loss.backward()
    assert bool(torch.isfinite(loss.detach()).all()) and float(loss.detach()) > 0
    grads = [p.grad for p in student.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and any(bool((g != 0).any()) for g in grads)
    assert train_engine(student).fp8_w4_layers == EXPECTED
