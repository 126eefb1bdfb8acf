"""csrc/region_loss.hip without a device: the float64 reference of the region loss (region_loss_ref.py) against the values
recorded from the real reference, the torch restatement (RegionLoss on CPU tensors) against that reference on every input of
test_region_loss_gpu.py -- which yields the GPU test's tolerance --, what those inputs contain, and the argument
validation of mcamd_region_loss."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from modelcompression_amd import _lib, ops
from modelcompression_amd.region_loss import RegionLoss
from region_loss_ref import region_loss_ref, EPS32
import region_loss_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
P = 4096        # a non-null address that is never dereferenced: every call below fails validation first


def test_reference_matches_the_recorded_golden_values():
    gold = np.load(os.path.join(HERE, "golden", "region_loss.npz"))
    for case in (0, 1):
        ref = region_loss_ref(gold["c%d_out" % case], gold["c%d_target" % case], RC.BENCH_ANCHORS, 5, 20,
                              (1.0, 1.0, 5.0, 1.0), 0.6)
        loss, grad = float(gold["c%d_loss" % case]), gold["c%d_grad" % case].astype(np.float64)
        err = float(np.abs(ref.grad - grad).max())
        print("golden case %d: loss %.6f (recorded %.6f), largest gradient error %.1e of %.2g"
              % (case, ref.loss, loss, err, np.abs(grad).max()))
        assert abs(ref.loss - loss) <= 1e-6 * abs(loss)
        assert err <= 1e-6 * np.abs(grad).max()


def restatement(name, scales_name):
    """(loss, gradient) of the torch restatement on make(name), with the out-of-range labels replaced by class 0 (its
    cross_entropy raises for them, as the reference's does)."""
    B, A, Cn, H, W, _, _ = RC.CASES[name]
    out, target = RC.make(name)
    mod = RegionLoss(num_classes=Cn, anchor_list=RC.anchors_for(A), anchors_cell=A)
    mod.coord_scale, mod.noobject_scale, mod.object_scale, mod.class_scale = RC.SCALES[scales_name]
    mod.thresh = RC.THRESH
    o = out.clone().requires_grad_(True)
    val = mod(o, RC.labels_in_range(target, Cn))
    val.backward()
    return float(val.detach()), o.grad.numpy().astype(np.float64)


def test_restatement_against_reference_gives_the_gpu_tolerance():
    """The yardstick of test_region_loss_gpu.py: the largest |restatement - reference| in units of eps32 * scale, over all
    elements of all its inputs (class labels in range, see restatement())."""
    worst = worst_loss = 0.0
    for name, sname in RC.ALL:
        ref = RC.reference(name, sname, in_range_labels=True)
        val, grad = restatement(name, sname)
        assert np.isfinite(grad).all() and np.isfinite(ref.grad).all() and np.isfinite(ref.loss)
        zero = ref.grad == 0
        assert not grad[zero].any(), (name, sname)
        units = np.abs(grad - ref.grad)[~zero] / (EPS32 * ref.scale[~zero])
        lunits = abs(val - ref.loss) / (EPS32 * ref.loss_abs)
        print("%-10s %-9s loss %.6f (float64 %.6f, %.2f units), gradient %.2f units, largest gradient %.3g"
              % (name, sname, val, ref.loss, lunits, units.max(), np.abs(ref.grad).max()))
        worst, worst_loss = max(worst, float(units.max())), max(worst_loss, lunits)
    print("yardstick: gradient %.2f, loss %.2f units of eps32 * scale" % (worst, worst_loss))
    # K was derived from this figure (region_loss_cases.py); should it grow, K has to be derived again
    assert 4.0 * max(worst, worst_loss) <= RC.K


@pytest.mark.parametrize("name, sname", RC.ALL, ids=RC.IDS)
def test_inputs_are_away_from_every_discontinuity(name, sname):
    """A float32 evaluation may decide three comparisons differently from float64 (region_loss_ref.py: margins); every input
    keeps 1e-4 from each, so the GPU comparison excludes no cell.  Two more decisions depend on the number format and are
    kept as far: int(x * W) and the float32 overflow of exp(exp(o))."""
    for in_range in (False, True):
        ref = RC.reference(name, sname, in_range)
        assert min(ref.margins) >= 1e-4, ref.margins
    B, A, Cn, H, W, _, _ = RC.CASES[name]
    out, target = RC.make(name)
    t = target.view(B, 50, 5)
    for col, n in ((1, W), (2, H)):
        f32 = (t[:, :, col] * float(n)).to(torch.int64)
        f64 = (t[:, :, col].double() * float(n)).to(torch.int64)
        assert torch.equal(f32, f64)
    wh = out.view(B, A, 5 + Cn, H, W)[:, :, 2:4].double()
    assert not ((wh > 4.1) & (wh < 4.9)).any()                # overflow at 4.4855 (w) down to 4.458 (w * the largest anchor)


@pytest.mark.parametrize("name", list(RC.CASES))
def test_inputs_contain_what_they_were_built_for(name):
    B, A, Cn, H, W, _, _ = RC.CASES[name]
    out, target = RC.make(name)
    ref = RC.reference(name, "s3_05_5_2")
    info = ref.info
    print(name, {k: v for k, v in info.items() if k != "assigned"}, "counts", ref.counts, "margins", ref.margins)
    t = target.view(B, 50, 5)
    assert (t[0, :, 1] != 0).all() and int((t[1, :, 1] != 0).long().cumprod(0).sum()) == 6      # 50 boxes; 6, then ignored rows
    assert info["ignored_rows"] >= 3 and ref.counts[0] == 50 + 6 * (1 + (B > 3))
    if B >= 3:
        assert not t[2].any()
    assert info["silenced"] >= 1 and info["overwritten"] >= 1 and ref.counts[1] >= 1
    assert info["clamped"] >= 1 and info["fallback"] >= 1 and info["out_of_range"] >= 1
    assert info["truncated_labels"] >= 1 and info["inf_boxes"] >= 1
    # the duplicated box: rows 5 and 40 share every coordinate, and row 40's class is the one that is trained
    assert torch.equal(t[0, 5, 1:], t[0, 40, 1:]) and (Cn == 1 or t[0, 5, 0] != t[0, 40, 0])
    assert float(out.view(B, A, 5 + Cn, H, W)[:, :, 2:4].max()) > 4.5


def desc(**kw):
    d = _lib.RegionDesc()
    d.output, d.target, d.B, d.H, d.W, d.num_anchors, d.num_classes, d.max_boxes = P, P, 2, 13, 13, 5, 20, 50
    for i in range(10):
        d.anchors[i] = 1.0 + i
    d.coord_scale = d.noobject_scale = d.object_scale = d.class_scale = 1.0
    d.thresh = 0.6
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def err():
    return _lib.lib().mcamd_last_error().decode()


def call(d, loss=P, grad=P, counts=None, ws=P, ws_bytes=None):
    lib = _lib.lib()
    ws_bytes = lib.mcamd_region_loss_workspace_bytes(d.B) if ws_bytes is None else ws_bytes
    return lib.mcamd_region_loss(C.byref(d), loss, grad, counts, ws, ws_bytes, None)


@pytest.mark.parametrize("bad, text", [
    (dict(output=None), "null argument"),
    (dict(target=None), "null argument"),
    (dict(B=0), "bad shape"),
    (dict(H=0), "bad shape"),
    (dict(W=0), "bad shape"),
    (dict(num_anchors=0), "bad shape"),
    (dict(num_classes=0), "bad shape"),
    (dict(num_anchors=9), "9 anchors <= 8"),
    (dict(max_boxes=49), "hold 50 boxes (got 49)"),
    (dict(max_boxes=51), "hold 50 boxes (got 51)"),
])
def test_region_loss_refuses_bad_descriptors(bad, text):
    assert call(desc(**bad)) == -1
    assert err().startswith("region_loss:") and text in err(), err()


def test_region_loss_refuses_null_pointers():
    lib = _lib.lib()
    assert lib.mcamd_region_loss(None, P, P, None, P, 1 << 20, None) == -1 and "region_loss: null argument" in err()
    for kw in (dict(loss=None), dict(grad=None), dict(ws=None)):
        assert call(desc(), **kw) == -1 and "region_loss: null argument" in err(), kw


def test_region_loss_workspace_size_and_short_workspace():
    lib = _lib.lib()
    one = lib.mcamd_region_loss_workspace_bytes(1)
    assert one > 0 and lib.mcamd_region_loss_workspace_bytes(0) == one and lib.mcamd_region_loss_workspace_bytes(-1) == one
    need = lib.mcamd_region_loss_workspace_bytes(3)
    assert need >= 3 * 8 * 4                                        # one partial sum per (image, anchor <= 8)
    assert call(desc(B=3), ws_bytes=need - 1) == -3                 # MCAMD_EWORKSPACE
    assert err().startswith("region_loss: workspace") and str(need - 1) in err() and str(need) in err(), err()


def test_wrapper_has_no_cpu_path():
    """(the wrapper's own shape checks come after this one: test_region_loss_gpu.py reads their messages)"""
    for ch, anchors in ((125, RC.BENCH_ANCHORS), (124, RC.BENCH_ANCHORS), (125, RC.BENCH_ANCHORS[:8])):
        with pytest.raises(_lib.McamdError):
            ops.region_loss(torch.zeros(1, ch, 13, 13), torch.zeros(1, 250), anchors, 5, 20, 1, 1, 5, 1, 0.6)
