"""The distillation loss without a device: the closed-form gradient of distill_ref.py against float64 autograd of the torch
restatement (an independent check of the derivation), the float32 restatement against the float64 reference on every input
of test_distill_gpu.py -- which yields the GPU test's tolerance --, the planted rows, the argument validation of
mcamd_distill_loss and train()'s new keywords."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from modelcompression_amd import _lib, ops
from modelcompression_amd.distill import DistillLoss
from distill_ref import EPS32, EPS64
import distill_cases as DC

P = 4096        # a non-null address that is never dereferenced: every call below fails validation first


def restatement(name, sname, tau, dtype):
    B, A, Cn, H, W, _ = DC.CASES[name]
    S, T = DC.make(name)
    obj, box, cls = DC.SCALES[sname]
    mod = DistillLoss(num_classes=Cn, anchors_cell=A, obj_scale=obj, box_scale=box, cls_scale=cls, temperature=tau)
    s = S.to(dtype).clone().requires_grad_(True)
    t = T.to(dtype).clone().requires_grad_(True)
    val = mod(s, t)
    val.backward()
    assert t.grad is None                                     # the teacher is detached
    return float(val.detach()), s.grad.numpy().astype(np.float64)


@pytest.mark.parametrize("name, sname, tau", DC.ALL, ids=DC.IDS)
def test_closed_form_gradient_is_the_float64_autograd_gradient(name, sname, tau):
    ref = DC.reference(name, sname, tau)
    val, grad = restatement(name, sname, tau, torch.float64)
    assert np.isfinite(grad).all() and np.isfinite(ref.grad).all() and np.isfinite(ref.loss)
    nz = ref.scale > 0
    units = np.abs(grad - ref.grad)[nz] / (EPS64 * ref.scale[nz])
    print("%s: float64 autograd within %.1f units of eps64 * scale, loss %.12g against %.12g"
          % (name, units.max(), val, ref.loss))
    assert (np.abs(grad - ref.grad) <= 1e3 * EPS64 * ref.scale).all()
    assert abs(val - ref.loss) <= 1e3 * EPS64 * ref.loss_abs


def test_restatement_against_reference_gives_the_gpu_tolerance():
    """The yardstick of test_distill_gpu.py: the largest |float32 restatement - reference| in units of eps32 * scale, over
    all elements of all its inputs, scale sets and temperatures."""
    worst = worst_loss = 0.0
    for name in DC.CASES:
        case = case_loss = 0.0
        for sname in DC.SCALES:
            for tau in DC.TAUS:
                ref = DC.reference(name, sname, tau)
                val, grad = restatement(name, sname, tau, torch.float32)
                assert np.isfinite(grad).all() and np.isfinite(val)
                # (autograd's log_softmax backward does not give the exact zeros of the closed form where S == T: those
                # elements are measured like every other; the kernel's exact zeros are asserted on the device)
                nz = ref.scale > 0
                assert not grad[~nz].any(), (name, sname, tau)
                units = np.abs(grad - ref.grad)[nz] / (EPS32 * ref.scale[nz])
                case, case_loss = max(case, float(units.max())), max(case_loss, abs(val - ref.loss) / (EPS32 * ref.loss_abs))
        print("%-6s gradient %.2f units, loss %.2f units of eps32 * scale" % (name, case, case_loss))
        worst, worst_loss = max(worst, case), max(worst_loss, case_loss)
    print("yardstick: gradient %.2f, loss %.2f units" % (worst, worst_loss))
    # K was derived from these figures (distill_cases.py); should they grow, K has to be derived again
    assert 4.0 * max(worst, worst_loss) <= DC.K
    assert DC.K == 2.0 ** np.ceil(np.log2(4.0 * max(DC.YARDSTICK, DC.LOSS_YARDSTICK)))


@pytest.mark.parametrize("name", list(DC.CASES))
def test_planted_rows_are_there_and_give_no_nan(name):
    B, A, Cn, H, W, _ = DC.CASES[name]
    S, T = DC.make(name)
    s, t = (x.view(B, A, 5 + Cn, H * W)[0, 0] for x in (S, T))
    assert torch.equal(s[:, 0], t[:, 0]) and not s[:, 5].any() and not t[:, 5].any()
    assert s[0, 1] == 30 and s[1, 1] == -30 and s[4, 1] == 30 and t[0, 2] == -30 and t[1, 2] == 30 and t[4, 2] == 88
    assert t[5, 3] == 60 and (Cn < 3 or (t[6, 3] == -60 and t[7, 3] == 0))
    assert float(s[5:, 4].max()) == 30 and (Cn == 1 or float(s[5:, 4].max() - s[5:, 4].min()) == 60)
    assert (s[4, 6] == 88) == (name != "b4")
    for sname in DC.SCALES:
        for tau in DC.TAUS:
            ref = DC.reference(name, sname, tau)
            for dtype in (torch.float32, torch.float64):
                val, grad = restatement(name, sname, tau, dtype)
                assert np.isfinite(val) and np.isfinite(grad).all()
            assert np.isfinite(ref.grad).all() and np.isfinite(ref.scale).all() and np.isfinite(ref.strict).all()
            g = ref.grad.reshape(B, A, 5 + Cn, H * W)[0, 0]
            assert not g[:, 0].any() and not g[:, 5].any()                    # S == T and all zeros: exactly 0
            if Cn >= 3 and tau == 1.0:
                # the teacher's -60 classes: pt = exp(-120) is 0 in float32, their term is 0 and not NaN
                assert np.float32(np.exp(-120.0)) == 0
            if Cn == 1:
                assert not ref.grad.reshape(B, A, 6, H * W)[:, :, 5].any()    # one class: p = 1 on both sides


def test_restatement_is_non_finite_for_non_finite_logits():
    B, A, Cn, H, W, _ = DC.CASES["a1c80"]
    S, T = DC.make("a1c80")
    mod = DistillLoss(num_classes=Cn, anchors_cell=A)
    assert np.isfinite(float(mod(S, T)))
    for ch in (0, 2, 4, 7):
        for bad in (float("nan"), float("inf"), float("-inf")):
            s, t = S.clone(), T.clone()
            s[0, ch, 1, 1] = bad
            assert not np.isfinite(float(mod(s, T))), (ch, bad)
            t[0, ch, 2, 2] = bad
            assert not np.isfinite(float(mod(S, t))), (ch, bad)


def test_from_model_takes_the_region_layer():
    import os
    from modelcompression_amd.nets import Darknet
    model = Darknet(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini.cfg"))
    mod = DistillLoss.from_model(model, temperature=2.0, box_scale=3.0)
    assert (mod.num_classes, mod.num_anchors) == (model.num_classes, model.num_anchors)
    assert mod.fused and mod.temperature == 2.0 and mod.box_scale == 3.0 and mod.obj_scale == mod.cls_scale == 1.0
    with pytest.raises(ValueError, match="temperature"):
        DistillLoss(temperature=0.0)


# ---- the C ABI's validation (no launch)
def desc(**kw):
    d = _lib.DistillDesc()
    d.student, d.teacher, d.B, d.H, d.W, d.num_anchors, d.num_classes = P, P, 2, 13, 13, 5, 20
    d.obj_scale = d.box_scale = d.cls_scale = d.temperature = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def err():
    return _lib.lib().mcamd_last_error().decode()


def call(d, loss=P, grad=P, ws=P, ws_bytes=None):
    lib = _lib.lib()
    ws_bytes = lib.mcamd_distill_loss_workspace_bytes(d.B, d.num_anchors) if ws_bytes is None else ws_bytes
    return lib.mcamd_distill_loss(C.byref(d), loss, grad, ws, ws_bytes, None)


@pytest.mark.parametrize("bad, text", [
    (dict(student=None), "null argument"),
    (dict(teacher=None), "null argument"),
    (dict(B=0), "bad shape"),
    (dict(H=0), "bad shape"),
    (dict(W=0), "bad shape"),
    (dict(num_anchors=0), "0 anchors <= 8"),
    (dict(num_anchors=9), "9 anchors <= 8"),
    (dict(num_classes=0), "0 classes"),
    (dict(temperature=0.0), "temperature 0 must be positive"),
    (dict(temperature=-1.0), "temperature -1 must be positive"),
    (dict(temperature=float("nan")), "must be positive"),
])
def test_distill_loss_refuses_bad_descriptors(bad, text):
    assert call(desc(**bad)) == -1                                   # MCAMD_EINVAL
    assert err().startswith("distill_loss:") and text in err(), err()


def test_distill_loss_refuses_null_pointers_and_a_short_workspace():
    lib = _lib.lib()
    assert lib.mcamd_distill_loss(None, P, P, P, 1 << 20, None) == -1 and "distill_loss: null argument" in err()
    for kw in (dict(loss=None), dict(grad=None), dict(ws=None)):
        assert call(desc(), **kw) == -1 and "distill_loss: null argument" in err(), kw
    need = lib.mcamd_distill_loss_workspace_bytes(3, 5)
    assert need == 3 * 5 * 4 and lib.mcamd_distill_loss_workspace_bytes(0, 0) == 4       # one float per (image, anchor)
    assert call(desc(B=3), ws_bytes=need - 1) == -1
    assert err().startswith("distill_loss: workspace") and str(need - 1) in err() and str(need) in err(), err()


def test_wrapper_has_no_cpu_path():
    with pytest.raises(_lib.McamdError, match="no CPU path"):
        ops.distill_loss(torch.zeros(1, 125, 13, 13), torch.zeros(1, 125, 13, 13), 5, 20)


# ---- train()'s keywords
def test_train_signature_ends_with_the_new_keywords():
    from modelcompression_amd.train import YOLOv2Train
    params = list(inspect.signature(YOLOv2Train.train).parameters.values())[-3:]
    assert [(p.name, p.default) for p in params] == [("RESIDENT", False), ("TEACHER", None), ("DISTILL", None)]


def test_distill_without_teacher_raises():
    from modelcompression_amd.train import YOLOv2Train
    with pytest.raises(ValueError, match="DISTILL needs a TEACHER"):
        YOLOv2Train().train('', '', '', '', '', '', '', 'tests/golden/mini.cfg', '', 4, 10, MAX_EPOCHS=1,
                            DISTILL=DistillLoss())
