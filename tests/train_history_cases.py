"""The pieces of tests/test_train_history_gpu.py: the small networks, the snapshot of a model's state, a freshly constructed
model built from it, one training step, the bit-for-bit comparison of two steps and the record of what the engine under test
actually ran.  Test-side only."""
import collections
import os

import torch

from modelcompression_amd import nets
from oracle import darknet_ref as O
from test_bwd1x1_gpu import CHAIN_CFG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (cfg file or None = CHAIN_CFG, image size, batch, the conv block whose filter mask is edited in place,
#          {conv number: (filters mask A removes, filters mask B removes)})
# chain: conv2 and conv4 are compacted under A and fold into the 1x1 blocks behind them; B revives conv2 entirely, revives
#        conv4's filters 64 .. 127 and removes its filters 0 .. 31 (kept under A), and compacts conv6.
# mini:  conv2 keeps 0 .. 23 under A and 24 .. 63 under B (every filter changes sides), conv4 is compacted under A only,
#        conv3 under B only.
# q8:    conv3 / conv5 as the chain's conv2 / conv4 (conv5 is compacted in front of a pool and folds into conv6), conv7 under
#        B only.
# f8:    the network whose conv8 multiplies fp8 correction terms under "mixed" (golden/f8_hist.cfg): conv2 / conv4 as the
#        chain's conv2 / conv4 (conv4 folds into conv5), conv8 itself is compacted under B only.
NETS = {
    "chain": (None, 32, 2, 4, {2: (range(64, 128), ()), 4: (range(64, 256), list(range(0, 32)) + list(range(128, 256))),
                               6: ((), range(44, 64))}),
    "mini": (os.path.join(GOLDEN, "mini.cfg"), 64, 2, 2, {2: (range(24, 64), range(0, 24)), 4: (range(40, 64), ()),
                                                          3: ((), range(16, 32))}),
    "q8": (os.path.join(GOLDEN, "q8_qat.cfg"), 64, 2, 5, {3: (range(64, 128), ()),
                                                          5: (range(64, 128), list(range(0, 32)) + list(range(96, 128))),
                                                          7: ((), range(64, 128))}),
    "f8": (os.path.join(GOLDEN, "f8_hist.cfg"), 288, 2, 4, {2: (range(256, 512), ()),
                                                            4: (range(128, 512), list(range(0, 64)) + list(range(256, 512))),
                                                            8: ((), range(64, 128))}),
}

FEATURES = ("fwd replay", "bwd replay", "fwd re-record", "bwd re-record", "bwd1x1", "fused 1x1", "dgrad sums", "f8", "perm",
            "fold", "pool_act on", "pool_act off", "bst fwd", "bst dgrad", "revived")

Snapshot = collections.namedtuple("Snapshot", "state masks precision grad_scale sparse_train sparse_train_max_kept grad_div bn")
Step = collections.namedtuple("Step", "logits grads stats overflow")


def cfg_path(net, tmp_path):
    cfg = NETS[net][0]
    if cfg is None:
        cfg = str(tmp_path / "chain.cfg")
        if not os.path.exists(cfg):
            with open(cfg, "w") as f:
                f.write(CHAIN_CFG)
    return cfg


def convs_of(m):
    return [mod[0] for mod in m.models if isinstance(mod, torch.nn.Sequential) and hasattr(mod[0], "mask_flag")]


def bns_of(m):
    return [mod for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d)]


def new_model(cfg, dev, prec):
    m = nets.Darknet(cfg)
    m.load_state_dict(O.init_state(O.parse_cfg(cfg), seed=0))
    m.to(dev).train()
    m.precision = prec
    return m


def batch(net, dev):
    """The fixed image; the fixed logit gradient is drawn when the first step tells its shape (gout_for)."""
    _, size, B, _, _ = NETS[net]
    return torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(11)).to(dev)


def gout_for(shape, dev):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(12)) * 0.05).to(dev)


def filter_masks(m, net, which):
    """Filter masks A (which = 0) or B (1) of NETS[net]: ones, with whole filters zeroed."""
    spec = NETS[net][4]
    out = []
    for n, c in enumerate(convs_of(m), 1):
        k = torch.ones_like(c.weight.data)
        dead = list(spec.get(n, ((), ()))[which])
        if dead:
            k[dead] = 0
        out.append(k)
    return out


def alive_filters(m):
    """Per conv block the flags of the filters a forward computes something for (all of them without a mask)."""
    out = []
    for c in convs_of(m):
        if c.mask_flag:
            out.append((c.mask.reshape(c.mask.shape[0], -1).amax(1) != 0).cpu())
        else:
            out.append(torch.ones(c.weight.shape[0], dtype=torch.bool))
    return out


def snapshot(m):
    """What a freshly constructed model needs to be in the state `m` is in now: taken BEFORE m's step, which updates the
    running statistics."""
    flags = [c.mask_flag for c in convs_of(m)]
    assert all(flags) or not any(flags)
    return Snapshot({k: v.detach().clone() for k, v in m.state_dict().items() if not k.endswith(".mask")},
                    [c.mask.detach().clone() for c in convs_of(m)] if all(flags) else None,
                    m.precision, m.grad_scale, m.sparse_train, m.sparse_train_max_kept, float(getattr(m, "_grad_div", 1.0)),
                    [(bn.momentum, bn.eps) for bn in bns_of(m)])


def fresh_from(snap, cfg, dev, training=True):
    """A newly constructed model with the weights, statistics, masks and options of the snapshot."""
    m = nets.Darknet(cfg)
    m.load_state_dict(snap.state)
    m.to(dev)
    if snap.masks is not None:
        m.set_masks([k.clone() for k in snap.masks])
    m.precision, m.grad_scale = snap.precision, snap.grad_scale
    m.sparse_train, m.sparse_train_max_kept = snap.sparse_train, snap.sparse_train_max_kept
    m._grad_div = snap.grad_div
    for bn, (mom, eps) in zip(bns_of(m), snap.bn):
        bn.momentum, bn.eps = mom, eps
    m.train(training)
    return m


def train_engine(m, x):
    """The engine a training-mode forward of `m` on `x` runs on (built when there is none yet)."""
    assert m.training
    return m._engine_for(x)


def step(m, x, gout):
    """One training step: forward, zero_grad(), backward with the fixed logit gradient."""
    out = m(x)
    m.zero_grad()
    out.backward(gout_for(out.shape, x.device) if gout is None else gout)
    torch.cuda.synchronize()
    return Step(out.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()},
                {k: v.detach().clone() for k, v in m.state_dict().items()
                 if k.endswith(("running_mean", "running_var", "num_batches_tracked"))},
                m.grad_overflowed())


def differences(a, b, what):
    """One line per tensor of two steps that is not bit-equal: its name and the count of differing elements."""
    out = []

    def cmp(name, p, q):
        if p.shape != q.shape:
            out.append("%s: %s has shapes %s and %s" % (what, name, tuple(p.shape), tuple(q.shape)))
        elif not torch.equal(p, q):
            out.append("%s: %s differs in %d of %d elements" % (what, name, int((p != q).sum()) or -1, p.numel()))
    cmp("logits", a.logits, b.logits)
    for part, kind in ((a.grads, "grad of "), (a.stats, "")):
        other = b.grads if part is a.grads else b.stats
        assert part.keys() == other.keys(), what
        for k in part:
            cmp(kind + k, part[k], other[k])
    if a.overflow != b.overflow:
        out.append("%s: grad_overflowed() is %s and %s" % (what, a.overflow, b.overflow))
    return out


def features(eng, prev_plans, alive, prev_alive):
    """What the engine under test ran in the step just done, as the set of FEATURES names.  `prev_plans`: the (forward,
    backward) plan objects of the step before on the same engine, or None."""
    f = set()
    plans = (eng._fwd_plans.get(True), eng._bwd_plan)
    assert eng.use_plan and plans[0] is not None and plans[1] is not None
    if prev_plans is not None:
        for name, now, before in zip(("fwd", "bwd"), plans, prev_plans):
            if now is before and now.launches > 0:
                f.add(name + " replay")
            elif now is not before:
                f.add(name + " re-record")
    # (the per-layer caches the layer walk filled: entries of the current plan epoch only -- older ones are dropped when
    # something is inserted, not before)
    now = lambda cache: [v for k, v in cache.items() if k[-1] == eng._plan_epoch]
    if any(now(eng._bwd1x1_cache)):
        f.add("bwd1x1")
    if any(v is not None for v in now(eng._fused_1x1_cache)):
        f.add("fused 1x1")
    if any(v is not None for v in now(eng._dgrad_sums_cache)):
        f.add("dgrad sums")
    if eng.precision == "mixed" and any(lay.f8 for lay in eng.layers):
        f.add("f8")
    if any(lay.perm is not None for lay in eng.layers):
        f.add("perm")
    if any(lay.fold is not None for lay in eng.layers):
        f.add("fold")
    f.add("pool_act on" if eng.pool_act_on else "pool_act off")
    if eng.bsparse_train_layers:
        f.add("bst fwd")
    if eng.bsparse_train_dgrad_layers:
        f.add("bst dgrad")
    if prev_alive is not None and any(bool((now & ~before).any()) for now, before in zip(alive, prev_alive)):
        f.add("revived")
    return f, plans


def table(title, rows):
    """The state x feature table: one line per state, one column per feature."""
    lines = ["%s: state x feature (%s)" % (title, ", ".join("%d = %s" % (i, n) for i, n in enumerate(FEATURES)))]
    lines.append("%-44s %s" % ("state", " ".join("%2d" % i for i in range(len(FEATURES)))))
    for what, f in rows:
        lines.append("%-44s %s" % (what, " ".join(" x" if n in f else " ." for n in FEATURES)))
    return "\n".join(lines)
