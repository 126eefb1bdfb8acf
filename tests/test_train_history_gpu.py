"""A training engine's step does not depend on its history: one Darknet (`hist`) is driven through a scripted sequence of
states on the SAME training engine object -- optimizer steps, set_masks with magnitude and filter masks, a mask that revives
removed filters, masks edited in place, masks off, load_state_dict, weights edited through .data, BatchNorm momentum and
buffers changed and replaced, the data-parallel divisor, another stream, the gradient-ready hook, eval forwards in between, a
second training engine, block-sparse training -- and at every state three models do the same training step (forward on a
fixed image, zero_grad(), backward with a fixed logit gradient):

  hist    the model with the history;
  fresh   a newly constructed model built from a snapshot of hist's weights, statistics, masks and options, taken before
          hist's step (the step updates the running statistics);
  direct  another such model whose engine was constructed under MCAMD_PLAN=0 (the per-launch path, no recorded plans).

Logits, every parameter's gradient, every running_mean / running_var / num_batches_tracked after the step and
grad_overflowed() must be bit-equal between the three: no tolerance anywhere.  fresh and direct agreeing while hist differs
from both says that something the engine caches (a per-layer cache keyed on the plan epoch, the pack state, a buffer the
compaction assumes to be zero) is stale; hist and fresh agreeing while direct differs says that a recorded plan replays
something the layer walk would not issue.  Where the script says so (from the state with the masks off onwards, around every
change of the weights) an eval-mode forward of hist is compared bit for bit with a fresh model's as well: the eval engine
shares weights, running statistics and the model's "weights were replaced" flag with the training one.

What the test found when it was written, both fixed in Engine.pack: an engine built for a model whose flag another engine
had already cleared (the second training engine after grad_scale was halved) kept the static default e4m3 weight exponents
instead of reading them on its first pack, and after a .data edit + invalidate_packed() only the first engine that packed
saw the flag -- the eval engine went on with the old packed weights (Darknet._weights_serial now tells every engine).

One history-dependent choice exists by design: the per-layer exponent of the e4m3 weight bytes of the "mixed" precision,
Engine._refresh_f8_wexp -- "One host read, taken when the model says its weights were replaced (load_state_dict /
load_weights / invalidate_packed, and the first pack) -- not per step: SGD moves a layer's largest weight by far less than the
2x of headroom."  The comparison is not loosened for it: every state asserts as a precondition that hist's and fresh's engines
hold the same exponents, the script changes the scale of weights only through load_state_dict, and the filter it removes by
editing a mask in place is one that does not hold its layer's largest weight.

Out of scope: engine attributes that tests poke directly (eng.bwd_from_act, eng.dgrad_bn_sums, eng.bwd1x1, ...) and the
environment switches Engine.__init__ reads are not public state, and flipping them after a plan exists is not supported.

The script keeps a reference to every tensor it replaces (old masks, old parameter storage, old buffers): a stale plan then
reads old VALUES and the test fails on numbers -- it never reads released memory.

Darknet keeps at most three engines and drops the oldest, so the states that build more (the eval forward at B = 1 behind the
second training engine) come last, and plain fp16 runs its block-sparse states in front of them: every other state runs on
the first engine object, which is asserted."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd.pruning.weightPruning.methods import block_prune, weight_prune  # noqa: E402
import train_history_cases as H  # noqa: E402

# test id -> (precision, network); "auto" runs as "mixed"
RUNS = [("auto", "chain"), ("auto", "mini"), ("auto", "f8"), ("fp16x3", "chain"), ("fp16x3", "mini"), ("fp16", "mini"),
        ("fp8-qat", "q8"), ("fp8-w4-qat", "q8")]
SEEN = {}          # test id -> set of the FEATURES its hist engines ran (test_every_feature_occurred)


class Script:
    def __init__(self, dev, monkeypatch, tmp_path, prec, net):
        self.dev, self.monkeypatch, self.prec, self.net = dev, monkeypatch, prec, net
        self.cfg = H.cfg_path(net, tmp_path)
        self.hist = H.new_model(self.cfg, dev, prec)
        self.x, self.gout = H.batch(net, dev), None
        self.first = None
        self.keep = []                 # every tensor the script replaces stays alive
        self.rows, self.failures = [], []
        self.prev_plans, self.prev_alive = {}, None      # engine -> its (forward, backward) plans at its last step

    def convs(self):
        return H.convs_of(self.hist)

    def set_masks(self, masks):
        self.keep += [c.mask for c in self.convs() if c.mask_flag] + list(masks)
        self.hist.set_masks(masks)

    def direct_model(self, snap):
        """A fresh model whose engine is constructed with MCAMD_PLAN=0 (Engine.__init__ reads it once); the variable is back
        before anything else runs, so an engine hist builds later is not affected."""
        m = H.fresh_from(snap, self.cfg, self.dev)
        with self.monkeypatch.context() as mp:
            mp.setenv("MCAMD_PLAN", "0")
            eng = H.train_engine(m, self.x)
        assert not eng.use_plan
        return m, eng

    def state(self, what, same_engine=True, hook=None, eval_x=None):
        """One state of the script: snapshot, hist's step, the same step of `fresh` and `direct`, the comparison."""
        hist = self.hist
        what = "%s/%s %s" % (self.prec, self.net, what)
        snap = H.snapshot(hist)
        hist._grad_ready_hook = hook
        res = H.step(hist, self.x, self.gout)
        hist._grad_ready_hook = None
        if self.gout is None:
            self.gout = H.gout_for(res.logits.shape, self.dev)
        eng = H.train_engine(hist, self.x)
        if self.first is None:
            self.first = eng
        if same_engine:
            assert eng is self.first, what + ": the sequence must run on one engine object"
        fresh = H.fresh_from(snap, self.cfg, self.dev)
        ref = H.step(fresh, self.x, self.gout)
        eng_f = H.train_engine(fresh, self.x)
        assert eng_f is not eng and eng_f.use_plan and eng.use_plan
        direct, eng_d = self.direct_model(snap)
        res_d = H.step(direct, self.x, self.gout)
        assert H.train_engine(direct, self.x) is eng_d and eng_d._bwd_plan is None and not eng_d._fwd_plans
        # the precondition of the comparison, and the first line of a failure: the one history-dependent choice (module
        # docstring), the e4m3 weight exponents, is the same in all three engines
        wexp = [[lay.f8_wexp for lay in e.layers] for e in (eng, eng_f, eng_d)]
        bad = []
        if not wexp[0] == wexp[1] == wexp[2]:
            bad.append("%s: PRECONDITION: the engines hold different f8_wexp: hist %s, fresh %s, direct %s"
                       % ((what,) + tuple(wexp)))
        bad += H.differences(res, ref, what + ": hist vs fresh") + H.differences(res, res_d, what + ": hist vs direct") \
            + H.differences(ref, res_d, what + ": fresh vs direct")
        if eval_x is not None:
            snap2 = H.snapshot(hist)
            hist.eval()
            with torch.no_grad():
                out = hist(eval_x).clone()
                out_f = H.fresh_from(snap2, self.cfg, self.dev, training=False)(eval_x)
            hist.train()
            torch.cuda.synchronize()
            if not torch.equal(out, out_f):
                bad.append("%s: eval logits at B = %d differ from a fresh model's in %d of %d elements"
                           % (what, eval_x.shape[0], int((out != out_f).sum()), out.numel()))
        alive = H.alive_filters(hist)
        f, plans = H.features(eng, self.prev_plans.get(eng), alive, self.prev_alive)
        self.prev_plans[eng], self.prev_alive = plans, alive
        self.rows.append((what + (" FAILED" if bad else ""), f))
        self.failures += bad
        return res, eng

    def finish(self):
        seen = set().union(*[f for _, f in self.rows])
        SEEN["%s-%s" % (self.prec, self.net)] = seen
        print("\n" + H.table("%s / %s" % (self.prec, self.net), self.rows))
        assert not self.failures, "\n".join(self.failures)


def run_script(dev, monkeypatch, tmp_path, prec, net):
    s = Script(dev, monkeypatch, tmp_path, prec, net)
    hist = s.hist
    qat = prec in ("fp8-qat", "fp8-w4-qat")
    edit_conv = H.NETS[net][3]
    w0 = [c.weight.detach().clone() for c in s.convs()]

    # 1. dense first step, then an identical one that replays both plans
    s.state("1a dense, first step")
    s.state("1b dense, replayed")
    # 2. an optimizer step updates the weights in place
    opt = torch.optim.SGD(hist.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4)
    opt.step()
    s.state("2 SGD step")
    # 3. a 60 % magnitude mask removes no filter
    s.set_masks(weight_prune(hist, 60.0))
    s.state("3 magnitude mask 60 %")
    # 4. filter mask A: compaction, folded consumers, pool_act_on off, the perm path of the BatchNorm kernels
    s.set_masks(H.filter_masks(hist, net, 0))
    _, eng = s.state("4 filter mask A")
    assert any(lay.perm is not None for lay in eng.layers), "mask A must compact a block"
    # 5. filter mask B revives filters A removed and removes filters A kept (set_mask zeroes masked weights for good: the
    #    original weights go back in first, as a pruning round that reloads its checkpoint does, so that the revived
    #    filters compute something)
    for c, w in zip(s.convs(), w0):
        c.weight.data.copy_(w)
    s.set_masks(H.filter_masks(hist, net, 1))
    s.state("5 filter mask B")
    # 6. mask B edited in place on the same tensor objects: only _version changes.  The filter removed is the kept one
    #    with the smallest largest weight, so the layer's e4m3 exponent does not depend on it (module docstring)
    c = s.convs()[edit_conv - 1]
    alive = c.mask.reshape(c.mask.shape[0], -1).amax(1) != 0
    big = c.weight.data.abs().reshape(c.weight.shape[0], -1).amax(1)
    j = int(torch.nonzero(~alive).flatten()[0])
    k = int(torch.where(alive & (big > 0), big, torch.full_like(big, float("inf"))).argmin())
    assert bool(alive[k]) and not bool(alive[j]) and float(big[k]) < float(big[alive].max())
    ptrs = [(cc.mask.data_ptr(), cc.mask._version) for cc in s.convs()]
    c.mask[j] = 1
    c.mask[k] = 0
    assert [cc.mask.data_ptr() for cc in s.convs()] == [p for p, _ in ptrs] and c.mask._version > ptrs[edit_conv - 1][1]
    s.state("6 mask B edited in place")
    # 7. masks off: every filter is live again
    for c in s.convs():
        c.mask_flag = False
    _, eng = s.state("7 masks off", eval_x=s.x)               # (the eval engine exists from here on)
    assert all(lay.perm is None and lay.fold is None for lay in eng.layers)
    # 8. load_state_dict with every conv weight x 64, then x 1/64 of the original
    base = {k_: v.detach().clone() for k_, v in hist.state_dict().items()}
    for tag, mul in (("8a weights x 64", 64.0), ("8b weights x 1/64", 1.0 / 64.0)):
        hist.load_state_dict({k_: (v * mul if v.dim() == 4 and k_.endswith(".weight") else v.clone()) for k_, v in base.items()})
        s.state(tag, eval_x=s.x)
    hist.load_state_dict(base)
    s.state("8c the weights of state 7 again", eval_x=s.x)
    # 9. a weight edited through .data, then invalidate_packed()
    s.convs()[2].weight.data.mul_(1.5)
    hist.invalidate_packed()
    s.state("9 .data edit + invalidate_packed", eval_x=s.x)

    def item_16():
        """Eval forwards between training steps (under the qat precisions on the fp8 / w4 engine), and a second training
        engine beside the first, which must still be right when the model returns to it."""
        s.state("16a eval at B = %d between steps" % s.x.shape[0], eval_x=s.x)
        hist.grad_scale = hist.grad_scale / 2
        _, eng2 = s.state("16b grad_scale halved: a second engine", same_engine=False)
        assert eng2 is not s.first
        hist.grad_scale = hist.grad_scale * 2
        s.state("16c grad_scale restored: the first engine")
        # (the eval engine of B = 1 is the model's fourth: the first training engine goes once its step is done)
        s.state("16d eval at B = 1 between steps", eval_x=s.x[:1].contiguous())
        s.state("16e after the eval forwards", same_engine=False)
        return s.finish()
    if qat:               # (the qat precisions run items 1 - 9 and 16)
        return item_16()
    # 10. BatchNorm momentum 0.1 -> 0.3
    for bn in H.bns_of(hist):
        assert bn.momentum == 0.1
        bn.momentum = 0.3
    s.state("10 bn.momentum 0.3")
    # 11. running statistics re-initialised in place on two layers
    bns = H.bns_of(hist)
    for bn in (bns[1], bns[-1]):
        bn.running_mean.zero_()
        bn.running_var.fill_(1)
    s.state("11 running statistics reset in place")
    # 12. those buffers replaced by new tensors on the same two layers, and one conv weight's storage replaced
    for bn in (bns[1], bns[-1]):
        s.keep += [bn.running_mean, bn.running_var]
        bn.running_mean = bn.running_mean.clone()
        bn.running_var = bn.running_var.clone()
    p = s.convs()[3].weight
    s.keep.append(p.data)
    p.data = p.data.clone()
    res1, _ = s.state("12 buffers and a weight's storage replaced")
    # 13. the data-parallel divisor: at 2.0 every parameter gradient is exactly half of the one at 1.0
    hist._grad_div = 2.0
    res2, _ = s.state("13a _grad_div 2.0")
    for n_ in res1.grads:
        if not torch.equal(res2.grads[n_], res1.grads[n_] * 0.5):
            s.failures.append("%s/%s 13a: grad of %s at _grad_div 2.0 is not half of the one at 1.0 in %d of %d elements"
                              % (prec, net, n_, int((res2.grads[n_] != res1.grads[n_] * 0.5).sum()), res1.grads[n_].numel()))
    hist._grad_div = 1.0
    s.state("13b _grad_div 1.0")
    # 14. the step issued on another stream, then on the default stream again
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        s.state("14a on a non-default stream")
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    s.state("14b on the default stream again")
    # 15. the gradient-ready hook: the slices tile [0, total_params) exactly once, the gradients are those without it
    slices = []

    def hook(flat, lo, hi, fence=None):
        slices.append((lo, hi))
        if fence is not None:
            with fence():
                pass
    hook.takes_fence = True
    _, eng = s.state("15 gradient-ready hook", hook=hook)      # (fresh and direct run without the hook)
    pos = 0
    for lo, hi in sorted(slices):
        assert lo == pos and hi > lo, ("the hook's slices must tile the flat gradient", sorted(slices))
        pos = hi
    assert pos == eng.total_params
    if prec == "fp16":
        # 17. block-sparse training (in front of the states that build further engines: module docstring)
        s.set_masks(block_prune(hist, 75.0, per_layer=True))
        hist.sparse_train, hist.sparse_train_max_kept = "block", 1.0
        _, eng = s.state("17a sparse_train block, max_kept 1")
        chosen, kept = list(eng.bsparse_train_layers), dict(eng.bsparse_train_kept)
        assert chosen and len(set(kept[n_] for n_ in chosen)) > 1, (chosen, kept)
        fr = sorted(set(kept[n_] for n_ in chosen))
        hist.sparse_train_max_kept = 0.5 * (fr[0] + fr[1])        # between two layers' kept fractions: the set shrinks
        _, eng = s.state("17b max_kept between two kept fractions")
        assert eng.bsparse_train_layers and eng.bsparse_train_layers != chosen, (eng.bsparse_train_layers, chosen, kept)
        hist.sparse_train_max_kept = 1.0
        c = s.convs()[chosen[-1] - 1]
        v = c.mask._version
        c.mask[:, : c.mask.shape[1] // 2] = 0                      # the K chunks of half the input channels go
        c.mask[: min(8, c.mask.shape[0])] = 0                      # ... and a few whole filters
        assert c.mask._version > v
        s.state("17c block mask edited in place")
        hist.sparse_train = None
        _, eng = s.state("17d sparse_train None")
        assert eng.bsparse_train_layers == []
    # 16. eval forwards between training steps, and a second training engine
    return item_16()


@pytest.mark.parametrize("prec,net", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_training_step_does_not_depend_on_history(dev, monkeypatch, tmp_path, prec, net):
    run_script(dev, monkeypatch, tmp_path, prec, net)


def test_every_feature_occurred(dev):
    """Over the whole file the hist engines replayed and re-recorded both plans, took the one-launch 1x1 backward, the fused
    BatchNorm + 1x1 forward, the dgrad launch with BatchNorm sums and the fp8 correction form, ran with perm and fold set,
    with pool_act_on on and off, with block-sparse forward and dgrad launches, and met a filter that was dead in one state
    and live in the next.  Reads what the tests above recorded: run the file as a whole.  (`dev`: skipped without a GPU.)"""
    ids = ["%s-%s" % r for r in RUNS]
    assert sorted(SEEN) == sorted(ids), "run the whole file: the history tests record what their engines ran"
    seen = set().union(*SEEN.values())
    print({k: sorted(v) for k, v in SEEN.items()})
    assert seen == set(H.FEATURES), sorted(set(H.FEATURES) - seen)
    assert "f8" in SEEN["auto-f8"]
