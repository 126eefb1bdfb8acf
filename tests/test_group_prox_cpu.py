"""Proximal group lasso without a device (sparsify.py, csrc/group_prox.hip's C surface): the symbols, the
refusals of mcamd_group_prox, the package's torch path against the numpy restatement (gprox_ref.py) bit for bit, the boundary
n2 == thr2 from both sides on integer data, the gate cases, GroupLasso.masks() on tests/golden/mini.cfg, and the checks of
YOLOv2Train.GROUP_LASSO."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import modelcompression_amd
from modelcompression_amd import _lib, nets, ops, sparsify
from modelcompression_amd._lib import McamdError
from modelcompression_amd.pruning.weightPruning import methods
from modelcompression_amd.sparsify import GroupLasso, torch_block_prox, torch_gate_prox
from modelcompression_amd.synthetic import init_synthetic
import gprox_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "golden", "mini.cfg")
NAMES = ("mcamd_gprox_seg_workgroups", "mcamd_group_prox")


def bits(a):
    return np.asarray(a, np.float32).view(np.int32)


# ----------------------------------------------------------------------------- the C surface
def test_symbols_are_declared_bound_exported_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mcamd_g(?:prox|roup_prox)\w*)\(", hdr))
    assert declared == set(NAMES) == set(k for k in _lib.SIGNATURES if re.match(r"mcamd_g(prox|roup_prox)", k))
    lib = _lib.lib()
    assert all(hasattr(lib, name) for name in NAMES)
    body = re.search(r"typedef struct mcamd_gprox_seg \{(.*?)\} mcamd_gprox_seg;", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.GproxSeg._fields_] and C.sizeof(_lib.GproxSeg) == 40
    for name, value in (("MCAMD_GPROX_BLOCK", _lib.GPROX_BLOCK), ("MCAMD_GPROX_GATE", _lib.GPROX_GATE)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
    assert _lib.SIGNATURES["mcamd_group_prox"][1][3:5] == [C.c_double, C.c_float]
    src = open(os.path.join(ROOT, "modelcompression_amd", "build.py")).read()
    assert re.search(r'"group_prox.hip": \["-ffp-contract=off"\]', src)
    assert callable(ops.GroupProxTable) and callable(ops.GroupProxTable.step)
    assert modelcompression_amd.GroupLasso is methods.GroupLasso is sparsify.GroupLasso


def seg(**kw):
    s = _lib.GproxSeg()
    s.w, s.nz = 4096, 8192
    s.kind, s.cout, s.cin, s.khw, s.wg0 = _lib.GPROX_BLOCK, 70, 64, 9, 0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


GATE = dict(kind=_lib.GPROX_GATE, cin=1, khw=1)


@pytest.mark.parametrize("bad,text", [
    (dict(w=None), "null tensor"),
    (dict(w=4098), "4-byte aligned"),
    (dict(nz=8194), "4-byte aligned"),
    (dict(cin=48), "blocks need cin % 32 == 0 (cin 48)"),
    (dict(cin=3), "blocks need cin % 32 == 0 (cin 3)"),
    (dict(cout=0), "bad shape"),
    (dict(kind=2), "unknown kind 2"),
    (dict(wg0=1), "wg0 1 is not the running sum 0"),
    (dict(GATE, cin=2), "a gate is [C][1][1]"),
])
def test_group_prox_refuses_bad_tables(bad, text):
    """Every argument error is refused before a launch (the pointers are never dereferenced: this runs without a device)."""
    lib = _lib.lib()
    arr = (_lib.GproxSeg * 1)(seg(**bad))
    assert lib.mcamd_group_prox(arr, 4096, 1, 0.25, 0.5, None, None) == -1
    err = lib.mcamd_last_error().decode()
    assert text in err and err.startswith("group_prox:"), err


def test_group_prox_refuses_bad_arguments_and_inconsistent_offsets():
    lib = _lib.lib()
    err = lambda: lib.mcamd_last_error().decode()
    one = (_lib.GproxSeg * 1)(seg())
    assert lib.mcamd_group_prox(None, 4096, 1, 0.25, 0.5, None, None) == -1 and "null argument" in err()
    assert lib.mcamd_group_prox(one, None, 1, 0.25, 0.5, None, None) == -1 and "null argument" in err()
    assert lib.mcamd_group_prox(one, 4096, 0, 0.25, 0.5, None, None) == -1 and "null argument" in err()
    assert lib.mcamd_group_prox(one, 4100, 1, 0.25, 0.5, None, None) == -1 and "misaligned" in err()
    assert lib.mcamd_group_prox(one, 4096, 1, 0.25, 0.5, 4098, None) == -1 and "misaligned" in err()
    for tau2 in (-1.0, float("inf"), float("nan")):
        assert lib.mcamd_group_prox(one, 4096, 1, tau2, 0.5, None, None) == -1 and "tau2 must be finite" in err()
    for tau in (-1.0, float("inf"), float("nan")):
        assert lib.mcamd_group_prox(one, 4096, 1, 0.25, tau, None, None) == -1 and "tau_gate must be finite" in err()
    # (70, 64, 9): 2 filter blocks x 1 channel block, all taps in one workgroup; a gate of 600 channels: 2 workgroups
    assert lib.mcamd_gprox_seg_workgroups(C.byref(seg())) == 2
    assert lib.mcamd_gprox_seg_workgroups(C.byref(seg(cout=128, cin=192))) == 6
    assert lib.mcamd_gprox_seg_workgroups(C.byref(seg(cout=96, cin=32))) == 2
    assert lib.mcamd_gprox_seg_workgroups(C.byref(seg(cout=600, **GATE))) == 2
    assert lib.mcamd_gprox_seg_workgroups(C.byref(seg(cin=3))) == 0
    two = (_lib.GproxSeg * 2)(seg(), seg(cout=600, wg0=3, **GATE))
    assert lib.mcamd_group_prox(two, 4096, 2, 0.25, 0.5, None, None) == -1 and "segment 1: wg0 3 is not the running sum 2" in err()


# ----------------------------------------------------------------------------- the torch path against the restatement
@pytest.mark.parametrize("shape", R.BLOCKS, ids=lambda s: "x".join(map(str, s)))
def test_torch_block_path_equals_the_restatement(shape):
    w = R.block_weights(shape, R.TAU, seed=sum(shape))
    want, want_nz = R.block_prox(w, R.TAU * R.TAU)
    got, nz = torch.from_numpy(w.copy()), torch.full((R.nblocks(*shape),), -1, dtype=torch.int32)
    torch_block_prox(got, R.TAU * R.TAU, nz)
    assert np.array_equal(bits(got.numpy()), bits(want)) and np.array_equal(nz.numpy(), want_nz)
    if want_nz.size >= 9:              # (the 1-tap shapes have one or two blocks: both sides over the set, below)
        zero = 1.0 - want_nz.mean()
        assert 0.1 < zero < 0.9, "the seeded scales must put blocks on both sides (%.2f zero)" % zero
    # a zeroed block is +0.0 by bit pattern; a kept one is not all zero and no |w| grew
    blocks = np.repeat(np.repeat(want_nz.reshape(R.block_dims(*shape)[0], -1, shape[2]), 64, axis=0)[:shape[0]],
                       R.block_dims(*shape)[2], axis=1)
    assert (bits(want)[blocks == 0] == 0).all() and (np.abs(want) <= np.abs(w)).all()


def test_the_one_tap_cases_fall_on_both_sides():
    flags = np.concatenate([R.block_prox(R.block_weights(s, R.TAU, seed=sum(s)), R.TAU * R.TAU)[1] for s in R.BLOCKS if s[2] == 1])
    assert flags.size == 3 and 0 < flags.sum() < 3


@pytest.mark.parametrize("c", R.GATES)
def test_torch_gate_path_equals_the_restatement(c):
    g = R.gate_weights(c, R.TAU, seed=c)
    want, want_nz = R.gate_prox(g, R.TAU)
    got, nz = torch.from_numpy(g.copy()), torch.full((c,), -1, dtype=torch.int32)
    torch_gate_prox(got, R.TAU, nz)
    assert np.array_equal(bits(got.numpy()), bits(want)) and np.array_equal(nz.numpy(), want_nz)


def test_lam_zero_leaves_every_bit():
    for shape in R.BLOCKS[:4]:
        w = R.block_weights(shape, R.TAU, seed=1)
        got = torch.from_numpy(w.copy())
        torch_block_prox(got, 0.0)
        assert np.array_equal(bits(got.numpy()), bits(w)) and np.array_equal(bits(R.block_prox(w, 0.0)[0]), bits(w))
    g = R.gate_weights(255, R.TAU, seed=2)
    got = torch.from_numpy(g.copy())
    torch_gate_prox(got, 0.0)
    assert np.array_equal(bits(got.numpy()), bits(g)) and np.array_equal(bits(R.gate_prox(g, 0.0)[0]), bits(g))


def boundary_weights(ones):
    """(128, 64, 9) zeros; block (fb 1, cb 0, tap 4) holds `ones` ones, the others nothing."""
    w = np.zeros((128, 64, 9), np.float32)
    blk = np.zeros(4096, np.float32)
    blk[:ones] = 1.0
    w[64:, :, 4] = np.random.RandomState(0).permutation(blk).reshape(64, 64)
    return w


@pytest.mark.parametrize("path", ["numpy", "torch"])
def test_boundary_from_both_sides(path):
    """tau2 = 0.25, n_g = 4096, thr2 = 1024: 1024 ones are n2 == thr2 and go, 1025 ones stay with s = 1 - sqrt(1024 / 1025)."""
    def run(w):
        if path == "numpy":
            return R.block_prox(w, 0.25)
        t, nz = torch.from_numpy(w.copy()), torch.zeros(18, dtype=torch.int32)
        torch_block_prox(t, 0.25, nz)
        return t.numpy(), nz.numpy()
    out, nz = run(boundary_weights(1024))
    assert (bits(out) == 0).all() and not nz.any()
    w = boundary_weights(1025)
    out, nz = run(w)
    s = np.float32(np.float64(1.0) - np.sqrt(np.float64(1024.0) / np.float64(1025.0)))
    assert nz.sum() == 1 and nz[(1 * 1 + 0) * 9 + 4] == 1
    assert np.array_equal(bits(out), bits(w * s)) and (out != 0).sum() == 1025


@pytest.mark.parametrize("path", ["numpy", "torch"])
def test_gate_cases(path):
    tau = np.float32(0.3)
    g = np.array([tau, -tau, -0.5, 0.75, np.nan, 0.1, -0.0], np.float32)
    if path == "numpy":
        out, nz = R.gate_prox(g, float(tau))
    else:
        t, f = torch.from_numpy(g.copy()), torch.zeros(7, dtype=torch.int32)
        torch_gate_prox(t, float(tau), f)
        out, nz = t.numpy(), f.numpy()
    assert bits(out)[0] == 0 and bits(out)[1] == 0 and bits(out)[5] == 0 and bits(out)[6] == 0      # +0.0 by bit pattern
    assert out[2] == np.float32(np.float32(0.5) - tau) * -1 and out[3] == np.float32(0.75) - tau
    assert np.isnan(out[4]) and list(nz) == [0, 0, 1, 1, 1, 0, 0]


def test_non_finite_blocks_are_not_hidden():
    w = R.block_weights((64, 64, 9), R.TAU, seed=3) * np.float32(100.0)
    w[3, 5, 0], w[7, 9, 1] = np.inf, np.nan
    for out in (R.block_prox(w, 0.25)[0], None):
        if out is None:
            t = torch.from_numpy(w.copy())
            torch_block_prox(t, 0.25)
            out = t.numpy()
        assert np.array_equal(bits(out[:, :, 0]), bits(w[:, :, 0]))          # Inf: n2 = Inf, s = 1
        assert np.isnan(out[:, :, 1]).all()                                  # NaN: the whole block
        assert np.isfinite(out[:, :, 2:]).all()


# ----------------------------------------------------------------------------- the model interface
def mini():
    return init_synthetic(nets.Darknet(MINI), seed=0)


def test_step_and_masks_on_the_mini_model():
    model = mini()
    ps = [p for p in model.parameters() if p.dim() != 1]
    elig = [p.dim() == 4 and p.shape[1] % 32 == 0 for p in ps]
    assert elig == [False] + [True] * 6
    # previously set masks: every other input channel of the eligible layers off
    old = [torch.ones_like(p.data) for p in ps]
    for o in old[1:]:
        o[:, ::2] = 0
    model.set_masks(old)
    scores = []
    for p, e in zip(ps, elig):
        if e:
            w = p.detach().numpy().reshape(p.shape[0], p.shape[1], -1)
            for fb in range(0, p.shape[0], 64):
                kb = 64 if p.shape[1] % 64 == 0 else 32
                blk = w[fb:fb + 64].reshape(min(64, p.shape[0] - fb), -1, kb, w.shape[2]).astype(np.float64)
                scores.append(np.sqrt((blk * blk).mean((0, 2))).reshape(-1))
    tau = float(np.median(np.concatenate(scores)))
    before = [p.detach().numpy().copy() for p in ps]
    serial = model._weights_serial
    gl = GroupLasso(model, lam=tau / 1e-5, granularity="block")
    assert gl.zero_fraction() == 0.0
    gl.step(1e-5, skip=torch.ones(1))
    assert all(np.array_equal(bits(p.detach().numpy()), bits(b)) for p, b in zip(ps, before)) and gl.zero_fraction() == 0.0
    gl.step(1e-5, skip=torch.zeros(1))
    assert model._weights_serial == serial + 1
    tau = 1e-5 * (tau / 1e-5)
    flags = gl.nonzero_flags()
    assert flags[0] is None and np.array_equal(bits(ps[0].detach().numpy()), bits(before[0]))
    want_masks = []
    for p, b, f, e, o in zip(ps, before, flags, elig, old):
        if not e:
            want_masks.append(o.numpy())
            continue
        want, nz = R.block_prox(b, tau * tau)
        assert np.array_equal(bits(p.detach().numpy()), bits(want)) and np.array_equal(f.numpy(), nz)
        cout, cin, khw = p.shape[0], p.shape[1], p.shape[2] * p.shape[3]
        nfb, ncb, kb = R.block_dims(cout, cin, khw)
        keep = np.repeat(np.repeat(nz.reshape(nfb, ncb, khw), 64, axis=0)[:cout], kb, axis=1).reshape(p.shape)
        want_masks.append(o.numpy() * keep.astype(np.float32))
    frac = gl.zero_fraction()
    print("zero-block fraction of the seeded mini model at the median block RMS: %.4f" % frac)
    assert 0.25 < frac < 0.75
    masks = gl.masks()
    assert len(masks) == len(ps)
    for m, want in zip(masks, want_masks):
        assert m.dtype == torch.float32 and np.array_equal(m.numpy(), want)
    assert all(float(m[:, ::2].abs().sum()) == 0 for m in masks[1:])
    assert any(0 < float(m.mean()) < 0.5 for m in masks[1:])                    # both factors at work in one layer


def test_filter_granularity_on_the_mini_model():
    model = mini()
    ps = [p for p in model.parameters() if p.dim() != 1]
    bns = [seq[1] for seq in model.models if isinstance(seq, torch.nn.Sequential) and len(seq) > 1
           and isinstance(seq[1], torch.nn.BatchNorm2d)]
    assert len(bns) == len(ps) - 1
    before = [bn.weight.detach().numpy().copy() for bn in bns]
    convs = [p.detach().numpy().copy() for p in ps]
    tau = float(np.median(np.abs(np.concatenate(before))))
    gl = GroupLasso(model, lam=tau, granularity="filter")
    gl.step(1.0)
    masks = gl.masks()
    for bn, b, f, m, p in zip(bns, before, gl.nonzero_flags(), masks, ps):
        want, nz = R.gate_prox(b, tau)
        assert np.array_equal(bits(bn.weight.detach().numpy()), bits(want)) and np.array_equal(f.numpy(), nz)
        keep = (want != 0).astype(np.float32).reshape(-1, 1, 1, 1)
        assert np.array_equal(m.numpy(), np.broadcast_to(keep, tuple(p.shape)))
    assert gl.nonzero_flags()[-1] is None and float(masks[-1].min()) == 1            # the last conv has no gate
    assert all(np.array_equal(bits(p.detach().numpy()), bits(c)) for p, c in zip(ps, convs))     # conv weights untouched
    assert 0.25 < gl.zero_fraction() < 0.75


def test_group_lasso_refusals():
    model = mini()
    with pytest.raises(McamdError, match=r"lam must be a finite number >= 0 \(got -1"):
        GroupLasso(model, -1.0, "block")
    with pytest.raises(McamdError, match="lam must be a finite number"):
        GroupLasso(model, float("nan"), "block")
    with pytest.raises(McamdError, match=r"granularity must be one of \('block', 'filter'\) \(got 'weight'\)"):
        GroupLasso(model, 1.0, "weight")
    half = mini()
    half.models[0][0].weight.data = half.models[0][0].weight.data.double()
    with pytest.raises(McamdError, match="fp32 tensors on one device"):
        GroupLasso(half, 1.0, "block")
    tied = mini()
    tied.models[2][0].share_flag = True
    with pytest.raises(McamdError, match="tied by set_codebooks"):
        GroupLasso(tied, 1.0, "block")
    with pytest.raises(McamdError, match=r"lr \* lam must be a finite number"):
        GroupLasso(model, 1.0, "block").step(float("inf"))


def test_train_checks_group_lasso_before_anything_else():
    from modelcompression_amd.train import YOLOv2Train
    assert YOLOv2Train.GROUP_LASSO is None
    assert not any("lasso" in n.lower() for n in inspect.signature(YOLOv2Train.train).parameters)
    args = ('', '', '', '', '', '', 'p_', MINI, '', 2, 10)

    def run(value, **kw):
        t = YOLOv2Train()
        t.GROUP_LASSO = value
        t.train(*args, **kw)
    for bad in (1.0, {"lam": 1.0}, {"lam": 1.0, "granularity": "block", "schedule": 1}):
        with pytest.raises(ValueError, match="GROUP_LASSO must be None or a dict"):
            run(bad)
    with pytest.raises(McamdError, match=r"train: GROUP_LASSO: lam must be a finite number >= 0 \(got -0.5\)"):
        run({"lam": -0.5, "granularity": "block"})
    with pytest.raises(McamdError, match=r"train: GROUP_LASSO: granularity must be one of"):
        run({"lam": 0.5, "granularity": "weight"})
    with pytest.raises(ValueError, match="SHARE and GROUP_LASSO cannot be combined"):
        run({"lam": 0.5, "granularity": "block"}, SHARE=4)
    assert YOLOv2Train.GROUP_LASSO is None
