"""The Taylor-importance kernel (csrc/taylor.hip) against the numpy restatement of include/mcamd.h
(taylor_ref.py): every accumulator bit for bit -- fp32 and float64 compared as integer patterns, no tolerance -- with all
segments in ONE table, every library call under torch.cuda.set_sync_debug_mode("error").

Every tensor the table names sits inside a larger buffer between canaries, at an offset that is 4-byte (fp32) or 8-byte
(float64) aligned and no more: a gradient is a view into a flat buffer."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import taylor_ref as R  # noqa: E402
from modelcompression_amd import ops  # noqa: E402

# (cout, cin, khw, bias): kb 64 with a ragged filter block; kb 32; several workgroups with a tail; no block form, with a bias
CONVS = [(70, 64, 9, False), (64, 96, 1, False), (136, 96, 9, False), (5, 3, 9, True)]
GATES = [70, 5]
# beyond the list above: 25 taps (the direct form); the last conv of a network (block AND filter scores, a bias); 2 taps
EXTRA = [(130, 64, 25, False), (125, 64, 1, True), (66, 32, 2, True)]
GUARD = {torch.float32: 61, torch.float64: 3}
CANARY = -7.0


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


def nblocks(cout, cin, khw):
    return ((cout + 63) // 64) * (cin // (64 if cin % 64 == 0 else 32)) * khw


def build(dev, convs, gates, seed, outputs=("acc_w", "acc_b", "acc_f")):
    """(arena, items for ops.TaylorTable, host state for the restatement).  Conv segments take acc_w, acc_b where the layer
    has a block form, and acc_f where the layer has a bias (a conv without BatchNorm); accumulators start from random values."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    arena, items, host = Arena(dev), [], []
    for cout, cin, khw, bias in convs:
        h = dict(w=rnd(cout, cin, khw) * 0.1, acc_w=rnd(cout, cin, khw).abs(), acc_b=None, acc_f=None, bias=None, gate=False)
        if cin % 32 == 0:
            h["acc_b"] = rnd(nblocks(cout, cin, khw)).double().abs()
        if bias:
            h["bias"], h["acc_f"] = rnd(cout), rnd(cout).double().abs()
        for name in ("acc_w", "acc_b", "acc_f"):
            if name not in outputs:
                h[name] = None
        if h["acc_w"] is None and h["acc_b"] is None and h["acc_f"] is None:
            continue
        it = dict(w=arena.put(h["w"]), g=arena.put(torch.zeros(cout, cin, khw)))
        if bias:
            it["bias"], it["gbias"] = arena.put(h["bias"]), arena.put(torch.zeros(cout))
        for name in ("acc_w", "acc_b", "acc_f"):
            if h[name] is not None:
                it[name] = arena.put(h[name])
        items.append(it), host.append(h)
    for C in gates if "acc_f" in outputs else []:
        h = dict(w=rnd(C) + 1.0, bias=rnd(C), acc_f=rnd(C).double().abs(), gate=True)
        items.append(dict(gate=True, w=arena.put(h["w"]), g=arena.put(torch.zeros(C)), bias=arena.put(h["bias"]),
                          gbias=arena.put(torch.zeros(C)), acc_f=arena.put(h["acc_f"])))
        host.append(h)
    return arena, items, host


def fresh_gradients(items, host, seed):
    gen = torch.Generator().manual_seed(seed)
    for it, h in zip(items, host):
        h["g"] = torch.randn(h["w"].shape, generator=gen)
        it["g"].copy_(h["g"])
        if h["bias"] is not None:
            h["gbias"] = torch.randn(h["bias"].shape, generator=gen)
            it["gbias"].copy_(h["gbias"])


def reference_step(host):
    for h in host:
        if h["gate"]:
            acc = h["acc_f"].numpy()
            R.gate_step(h["w"].numpy(), h["g"].numpy(), h["bias"].numpy(), h["gbias"].numpy(), acc)
        else:
            n = lambda t: None if t is None else t.numpy()
            R.conv_step(h["w"].numpy(), h["g"].numpy(), n(h["bias"]), n(h.get("gbias")), n(h["acc_w"]), n(h["acc_b"]), n(h["acc_f"]))


def same_bits(got, want):
    bits = torch.int32 if want.dtype == torch.float32 else torch.int64
    return got.dtype == want.dtype and torch.equal(got.cpu().contiguous().view(bits), want.contiguous().view(bits))


def assert_equal(items, host, what):
    for s, (it, h) in enumerate(zip(items, host)):
        for name in ("acc_w", "acc_b", "acc_f"):
            if h.get(name) is not None:
                assert same_bits(it[name], h[name]), "%s: segment %d %s differs from the restatement" % (what, s, name)


@pytest.mark.parametrize("convs,gates", [(CONVS, GATES), (EXTRA, [300])], ids=["issue-table", "extra-table"])
def test_three_steps_equal_the_restatement_bit_for_bit(dev, convs, gates):
    arena, items, host = build(dev, convs, gates, seed=1)
    steps = torch.zeros(1, dtype=torch.int32, device=dev)
    table = ops.TaylorTable(items, steps)
    assert table.nseg == len(convs) + len(gates)
    for step in range(3):
        fresh_gradients(items, host, seed=10 + step)
        with no_sync():
            table.accumulate()
        reference_step(host)
        assert_equal(items, host, "step %d" % step)
    assert int(steps.item()) == 3 and arena.intact()


def test_skip_changes_nothing_and_leaves_steps_alone(dev):
    arena, items, host = build(dev, CONVS, GATES, seed=2)
    steps = torch.full((1,), 5, dtype=torch.int32, device=dev)
    table = ops.TaylorTable(items, steps)
    fresh_gradients(items, host, seed=20)
    before = [{k: v.clone() for k, v in it.items() if k.startswith("acc")} for it in items]
    with no_sync():
        table.accumulate(skip=torch.ones(1, device=dev))
    assert int(steps.item()) == 5
    for it, b in zip(items, before):
        assert all(same_bits(it[k], v.cpu()) for k, v in b.items())
    with no_sync():
        table.accumulate(skip=torch.zeros(1, device=dev))       # *skip == 0: the step counts
    reference_step(host)
    assert_equal(items, host, "skip = 0")
    assert int(steps.item()) == 6 and arena.intact()


@pytest.mark.parametrize("outputs", [("acc_b", "acc_f"), ("acc_w", "acc_f"), ("acc_w", "acc_b"), ("acc_b",), ("acc_f",)],
                         ids=lambda o: "+".join(o))
def test_null_outputs_are_not_computed_or_written(dev, outputs):
    """Each output switched off in turn: the others still equal the restatement, and no canary around any tensor moved."""
    arena, items, host = build(dev, CONVS + EXTRA, GATES, seed=3, outputs=outputs)
    assert all(it.get(name) is None for it in items for name in ("acc_w", "acc_b", "acc_f") if name not in outputs)
    steps = torch.zeros(1, dtype=torch.int32, device=dev)
    table = ops.TaylorTable(items, steps)
    for step in range(2):
        fresh_gradients(items, host, seed=30 + step)
        with no_sync():
            table.accumulate()
        reference_step(host)
    assert_equal(items, host, "outputs %r" % (outputs,))
    assert int(steps.item()) == 2 and arena.intact()
    for it, h in zip(items, host):                  # the operands are read only
        assert same_bits(it["w"], h["w"]) and same_bits(it["g"], h["g"])


def test_wrapper_refuses_wrong_sizes_and_types(dev):
    from modelcompression_amd._lib import McamdError
    w = torch.zeros(64, 64, 9, device=dev)
    steps = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(McamdError, match="acc_b holds 8 entries, 9 expected"):
        ops.TaylorTable([dict(w=w, g=w.clone(), acc_b=torch.zeros(8, dtype=torch.float64, device=dev))], steps)
    with pytest.raises(McamdError, match="contiguous torch.float64"):
        ops.TaylorTable([dict(w=w, g=w.clone(), acc_b=torch.zeros(9, device=dev))], steps)
    w3 = torch.zeros(8, 3, 9, device=dev)
    with pytest.raises(McamdError, match="cin % 32 == 0"):
        ops.TaylorTable([dict(w=w3, g=w3.clone(), acc_b=torch.zeros(9, dtype=torch.float64, device=dev))], steps).accumulate()
    with pytest.raises(McamdError, match="skip must be a device fp32 scalar"):
        ops.TaylorTable([dict(w=w, g=w.clone(), acc_w=w.clone())], steps).accumulate(skip=torch.zeros(2, device=dev))


def test_accumulate_records_into_a_launch_plan(dev):
    """Like the other per-step calls: recorded while a plan records (nothing runs), replayed by the plan."""
    arena, items, host = build(dev, CONVS, GATES, seed=4)
    steps = torch.zeros(1, dtype=torch.int32, device=dev)
    table = ops.TaylorTable(items, steps)
    fresh_gradients(items, host, seed=40)
    plan = ops.Plan([torch.cuda.current_stream()])
    with plan:
        table.accumulate()
    assert plan.launches == 1 and int(steps.item()) == 0
    with no_sync():
        plan.run()
        plan.run()
    reference_step(host)
    reference_step(host)
    assert_equal(items, host, "two replays")
    assert int(steps.item()) == 2 and arena.intact()
