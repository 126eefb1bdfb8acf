"""The proximal group-lasso kernel (csrc/group_prox.hip) through the C surface against the numpy restatement
of include/mcamd.h (gprox_ref.py): which blocks go to zero and the flags exactly, zeroed elements +0.0 by bit pattern, kept
elements within MAX_ULP fp32 steps of the restatement, gates exactly; every segment alone and all of them in ONE table, every
library call under torch.cuda.set_sync_debug_mode("error").

Every tensor the table names sits inside a larger buffer between canaries, at an offset that is 4-byte aligned and no more.

MAX_ULP and its derivation: gprox_ref.py.  The tests print how many elements differ at all."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gprox_ref as R  # noqa: E402
from modelcompression_amd import _lib, ops  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402

MAX_ULP = R.MAX_ULP
GUARD = {torch.float32: 61, torch.int32: 3}
CANARY = -7
TAU2 = R.TAU * R.TAU


@contextlib.contextmanager
def no_sync():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


class Arena:
    """Tensors between canaries."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def put(self, host):
        g = GUARD[host.dtype]
        buf = torch.full((host.numel() + 2 * g,), CANARY, dtype=host.dtype, device=self.dev)
        view = buf[g:g + host.numel()].view(host.shape)
        view.copy_(host)
        self.bufs.append((buf, g, host.numel()))
        return view

    def intact(self):
        return all(bool((b[:g] == CANARY).all()) and bool((b[g + n:] == CANARY).all()) for b, g, n in self.bufs)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


@pytest.fixture(scope="module")
def cases():
    """[(kind, host weights, reference weights, reference flags)], computed once and left unchanged."""
    out = []
    for shape in R.BLOCKS:
        w = R.block_weights(shape, R.TAU, seed=sum(shape))
        out.append(("block", w) + R.block_prox(w, TAU2))
    for c in R.GATES:
        g = R.gate_weights(c, R.TAU, seed=c)
        out.append(("gate", g) + R.gate_prox(g, R.TAU))
    return out


def build(dev, cases):
    arena, items = Arena(dev), []
    for kind, w, _, nz in cases:
        items.append(dict(w=arena.put(torch.from_numpy(w.copy())), nz=arena.put(torch.full((nz.size,), -1, dtype=torch.int32)),
                          gate=kind == "gate"))
    return arena, items


def compare(items, cases, what):
    """Asserts the contract; returns (elements that differ from the restatement at all, kept elements compared)."""
    differ = kept = 0
    for s, (it, (kind, w, want, nz)) in enumerate(zip(items, cases)):
        got = it["w"].detach().cpu().numpy()
        assert np.array_equal(it["nz"].cpu().numpy(), nz), "%s: segment %d flags" % (what, s)
        if kind == "gate":
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), "%s: gate segment %d" % (what, s)
            continue
        zero = want.view(np.int32) == 0
        assert np.array_equal(got.view(np.int32) == 0, zero), "%s: segment %d: the +0.0 elements differ" % (what, s)
        steps = R.ulp_steps(got, want)
        differ += int((steps != 0).sum())
        kept += int((~zero).sum())
        assert int(steps.max()) <= MAX_ULP, "%s: segment %d: %d fp32 steps from the restatement" % (what, s, int(steps.max()))
    return differ, kept


def test_all_segments_in_one_table_and_launch(dev, cases):
    arena, items = build(dev, cases)
    table = ops.GroupProxTable(items)
    assert table.nseg == len(R.BLOCKS) + len(R.GATES)
    assert table.workgroups == 1 + 1 + 2 + 2 + 6 + 2 + 1 + 1 + 2
    with no_sync():
        table.step(R.TAU)
    differ, kept = compare(items, cases, "one table")
    print("one table: %d of %d kept elements differ from the restatement" % (differ, kept))
    assert arena.intact()
    # the step is a function of the operands alone: the same input gives the same bits again
    arena2, items2 = build(dev, cases)
    ops.GroupProxTable(items2).step(R.TAU)
    for a, b in zip(items, items2):
        assert np.array_equal(bits(a["w"]), bits(b["w"])) and torch.equal(a["nz"], b["nz"])


@pytest.mark.parametrize("index", range(len(R.BLOCKS) + len(R.GATES)),
                         ids=["x".join(map(str, s)) for s in R.BLOCKS] + ["gate%d" % c for c in R.GATES])
def test_each_segment_alone(dev, cases, index):
    one = cases[index:index + 1]
    arena, items = build(dev, one)
    with no_sync():
        ops.GroupProxTable(items).step(R.TAU)
    differ, kept = compare(items, one, "alone")
    print("%d of %d kept elements differ from the restatement" % (differ, kept))
    assert arena.intact()


def test_null_flags_are_not_written(dev, cases):
    arena, items = build(dev, cases)
    for it in items:
        del it["nz"]
    with no_sync():
        ops.GroupProxTable(items).step(R.TAU)
    for it, (kind, _, want, _) in zip(items, cases):
        assert int(R.ulp_steps(it["w"].cpu().numpy(), want).max()) <= (0 if kind == "gate" else MAX_ULP)
    assert arena.intact()


def test_skip_leaves_every_bit(dev, cases):
    arena, items = build(dev, cases)
    table = ops.GroupProxTable(items)
    with no_sync():
        table.step(R.TAU, skip=torch.ones(1, device=dev))
    for it, (_, w, _, nz) in zip(items, cases):
        assert np.array_equal(bits(it["w"]), w.view(np.int32)) and bool((it["nz"] == -1).all())
    with no_sync():
        table.step(R.TAU, skip=torch.zeros(1, device=dev))            # *skip == 0: the step runs
    compare(items, cases, "skip = 0")
    assert arena.intact()


def test_lam_zero_leaves_every_weight(dev, cases):
    arena, items = build(dev, cases)
    with no_sync():
        ops.GroupProxTable(items).step(0.0)
    for it, (_, w, _, _) in zip(items, cases):
        assert np.array_equal(bits(it["w"]), w.view(np.int32)) and bool((it["nz"] == 1).all())
    assert arena.intact()


def boundary_weights(ones):
    w = np.zeros((128, 64, 9), np.float32)
    blk = np.zeros(4096, np.float32)
    blk[:ones] = 1.0
    w[64:, :, 4] = np.random.RandomState(0).permutation(blk).reshape(64, 64)
    return w


def test_boundary_from_both_sides_on_the_device(dev):
    """tau2 = 0.25, n_g = 4096, thr2 = 1024: integer data, so n2 is exact whatever the order."""
    for ones in (1024, 1025):
        w = boundary_weights(ones)
        arena = Arena(dev)
        it = dict(w=arena.put(torch.from_numpy(w.copy())), nz=arena.put(torch.full((18,), -1, dtype=torch.int32)))
        ops.GroupProxTable([it]).step(0.5)
        got, nz = it["w"].cpu().numpy(), it["nz"].cpu().numpy()
        if ones == 1024:
            assert (got.view(np.int32) == 0).all() and not nz.any()
        else:
            s = np.float64(1.0) - np.sqrt(np.float64(1024.0) / np.float64(1025.0))
            want = (w.astype(np.float64) * s).astype(np.float32)
            assert nz.sum() == 1 and nz[13] == 1 and (got != 0).sum() == 1025
            assert int(R.ulp_steps(got, want).max()) <= MAX_ULP and (got.view(np.int32)[w == 0] == 0).all()
        assert arena.intact()


@pytest.mark.parametrize("shape", [(64, 64, 9), (64, 64, 1), (70, 64, 25)], ids=lambda s: "x".join(map(str, s)))
def test_non_finite_blocks_are_not_hidden(dev, shape):
    w = (R.block_weights(shape, R.TAU, seed=3) * np.float32(100.0)).astype(np.float32)
    want_finite = R.block_prox(w, TAU2)[0]
    taps = shape[2]
    w[3, 5, 0] = np.inf
    if taps > 1:
        w[7, 9, 1] = np.nan
    else:
        w = np.concatenate([w, w[:, :, :1].copy()], axis=0)           # a second filter block to hold the NaN
        w[64 + 7, 9, 0] = np.nan
        want_finite = np.concatenate([want_finite, want_finite], axis=0)
    arena = Arena(dev)
    it = dict(w=arena.put(torch.from_numpy(w.copy())), nz=arena.put(torch.full((R.nblocks(*w.shape),), -1, dtype=torch.int32)))
    ops.GroupProxTable([it]).step(R.TAU)
    got = it["w"].cpu().numpy()
    assert np.array_equal(got[:64, :, 0].view(np.int32), w[:64, :, 0].view(np.int32))         # Inf: n2 = Inf, s = 1
    nan_block = got[:64, :, 1] if taps > 1 else got[64:, :, 0]
    assert np.isnan(nan_block).all()                                                            # NaN: the whole block
    if taps > 2:
        assert int(R.ulp_steps(got[:, :, 2:], want_finite[:, :, 2:]).max()) <= MAX_ULP
    assert bool((it["nz"] == 1).all()) and arena.intact()


def test_refusals_write_nothing(dev, cases):
    """Every refusal returns MCAMD_EINVAL without a launch: the tensors and the flags keep their bits."""
    arena, items = build(dev, cases[:1] + cases[-1:])
    table = ops.GroupProxTable(items)
    lib, tab = _lib.lib(), table.table.data_ptr()
    skip = torch.zeros(1, device=dev)

    def call(arr=table.arr, tab=tab, nseg=2, tau2=TAU2, tau=R.TAU, skip_ptr=skip.data_ptr()):
        rc = lib.mcamd_group_prox(arr, tab, nseg, tau2, tau, skip_ptr, None)
        return rc, lib.mcamd_last_error().decode()

    def edited(index, **kw):
        arr = (_lib.GproxSeg * 2)()
        C.memmove(arr, table.arr, C.sizeof(arr))
        for k, v in kw.items():
            setattr(arr[index], k, v)
        return arr
    refused = [
        (call(arr=None), "null argument"), (call(tab=None), "null argument"), (call(nseg=0), "null argument"),
        (call(tab=tab + 4), "misaligned"), (call(skip_ptr=skip.data_ptr() + 2), "misaligned"),
        (call(tau2=-1.0), "tau2 must be finite"), (call(tau2=float("inf")), "tau2 must be finite"),
        (call(tau2=float("nan")), "tau2 must be finite"), (call(tau=-1.0), "tau_gate must be finite"),
        (call(tau=float("nan")), "tau_gate must be finite"),
        (call(arr=edited(0, w=None)), "null tensor"), (call(arr=edited(0, w=items[0]["w"].data_ptr() + 2)), "4-byte aligned"),
        (call(arr=edited(0, nz=items[0]["nz"].data_ptr() + 1)), "4-byte aligned"),
        (call(arr=edited(0, cin=48)), "blocks need cin % 32 == 0"), (call(arr=edited(0, kind=5)), "unknown kind"),
        (call(arr=edited(1, wg0=7)), "wg0 7 is not the running sum 1"), (call(arr=edited(1, khw=3)), "a gate is [C][1][1]"),
    ]
    torch.cuda.synchronize()
    for (rc, err), text in refused:
        assert rc == -1 and text in err and err.startswith("group_prox:"), (rc, err, text)
    for it, (_, w, _, _) in zip(items, cases[:1] + cases[-1:]):
        assert np.array_equal(bits(it["w"]), w.view(np.int32)) and bool((it["nz"] == -1).all())
    assert arena.intact()
    with pytest.raises(McamdError, match="cin % 32 == 0"):
        ops.GroupProxTable([dict(w=torch.zeros(8, 3, 9, device=dev))])
    with pytest.raises(McamdError, match="nz must be a contiguous int32 tensor of 9 entries"):
        ops.GroupProxTable([dict(w=torch.zeros(64, 64, 9, device=dev), nz=torch.zeros(8, dtype=torch.int32, device=dev))])
    with pytest.raises(McamdError, match="skip must be a device fp32 scalar"):
        table.step(R.TAU, skip=torch.zeros(2, device=dev))


def test_step_records_into_a_launch_plan(dev, cases):
    """Like the other per-step calls: recorded while a plan records (nothing runs), replayed by the plan."""
    arena, items = build(dev, cases)
    table = ops.GroupProxTable(items)
    plan = ops.Plan([torch.cuda.current_stream()])
    with plan:
        table.step(R.TAU)
    assert plan.launches == 1
    for it, (_, w, _, _) in zip(items, cases):
        assert np.array_equal(bits(it["w"]), w.view(np.int32))
    with no_sync():
        plan.run()
    compare(items, cases, "replay")
    assert arena.intact()
