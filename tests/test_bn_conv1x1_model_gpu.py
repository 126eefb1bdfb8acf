"""The engine's fused PLAIN -> 1x1 forward route (Engine._fused_1x1, MCAMD_FUSE_BN_1X1) against the two-kernel route on a
small network: a 3x3 stem + maxpool, a 3x3 block with 64 filters, a 1x1 BatchNorm block, a 3x3 block and a linear 1x1 head
at 32 x 32, B = 2, precision "mixed".  Two SGD steps in training mode with the route on and off, each with launch plans on
and off: logits, the flat gradient, the updated weights and the BatchNorm running statistics are bit-equal across the four
runs.  The same model in eval mode likewise.

Whether the "on" runs took the route is asserted from the engine's launch counter, against what the engine's plan allows:
a training engine keeps tensors up to 26 pixels wide in the shared-halo form, which mcamd_bn_act_conv1x1_ok refuses, and the
"mixed" training budget leaves this small network's 1x1 block on plain operands (level 1) -- so at 32 x 32 / "mixed" the
training runs all stay on two kernels (and must still agree), while the eval engine (padded buffers, the 1x1 block on split
operands) takes the route.  The second case is the same network at 64 x 64 (32 x 32 behind the pool: padded form, as at the
104- and 52-pixel layers of YOLOv2) in precision "fp16x3" (every block on split operands): there the fused launch runs
inside the SGD steps, and the test insists that it does."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets  # noqa: E402

CFG = """[net]
batch=1
height=%(size)d
width=%(size)d
channels=3
momentum=0.9
decay=0.0005
learning_rate=0.001
max_batches=100
policy=steps
steps=40,60
scales=.1,.1

[convolutional]
batch_normalize=1
filters=32
size=3
stride=1
pad=1
activation=leaky

[maxpool]
size=2
stride=2

[convolutional]
batch_normalize=1
filters=64
size=3
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=64
size=1
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=64
size=3
stride=1
pad=1
activation=leaky

[convolutional]
filters=125
size=1
stride=1
pad=1
activation=linear

[region]
anchors = 1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071
bias_match=1
classes=20
coords=4
num=5
softmax=1
jitter=.3
rescore=1
object_scale=5
noobject_scale=1
class_scale=1
coord_scale=1
absolute=1
thresh = .6
random=0
"""

RUNS = [("1", "1"), ("1", "0"), ("0", "1"), ("0", "0")]      # (MCAMD_FUSE_BN_1X1, MCAMD_PLAN)


CASES = [(32, "mixed"), (64, "fp16x3")]      # (input size, precision)


@pytest.fixture(scope="module", params=CASES, ids=["in%d-%s" % c for c in CASES])
def net(request, tmp_path_factory):
    size, precision = request.param
    p = tmp_path_factory.mktemp("bn_conv1x1") / ("pair%d.cfg" % size)
    p.write_text(CFG % dict(size=size))
    return str(p), size, precision


def _model(cfg_path, dev, state, precision):
    m = nets.Darknet(cfg_path)
    if state is not None:
        m.load_state_dict(state)
    m.precision = precision
    return m.to(dev)


def _inputs(size):
    g = torch.Generator().manual_seed(11)
    return torch.rand(2, 3, size, size, generator=g), torch.randn(2, 125, size // 2, size // 2, generator=g)


def _took_route(m, fuse, size, must):
    """The launch counter against what the engine's plan allows; `must`: this case has to exercise the route."""
    eng = list(m._engines.values())[-1]
    conv1x1 = eng.layers[2]
    assert conv1x1.k == 1 and conv1x1.bn is not None
    able = eng._pad_for(size // 2) == 0 and conv1x1.level == 3      # padded form behind the pool, 1x1 block on split operands
    assert able or not must, (eng.precision, size, conv1x1.level)
    assert (eng.fused_1x1_launches > 0) == (fuse == "1" and able), (fuse, size, eng.fused_1x1_launches)


def _state0(cfg_path):
    torch.manual_seed(5)
    m = nets.Darknet(cfg_path)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.5, 0.5)
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
    return {k: v.clone() for k, v in m.state_dict().items()}


def test_training_steps_bit_equal(dev, net, monkeypatch):
    cfg_path, size, precision = net
    state, (x, gout) = _state0(cfg_path), _inputs(size)
    res = {}
    for fuse, plan in RUNS:
        monkeypatch.setenv("MCAMD_FUSE_BN_1X1", fuse)
        monkeypatch.setenv("MCAMD_PLAN", plan)
        m = _model(cfg_path, dev, state, precision).train()
        opt = torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9)
        outs = []
        for _ in range(2):
            out = m(x.to(dev))
            opt.zero_grad()
            out.backward(gout.to(dev))
            flat = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone()
            opt.step()
            outs += [out.detach().clone(), flat]
        _took_route(m, fuse, size, must=precision == "fp16x3")
        outs.append(torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone())
        outs.append(torch.cat([b.detach().reshape(-1).float() for n, b in m.named_buffers() if "running" in n]).clone())
        res[(fuse, plan)] = outs
        del m, opt
    ref = res[RUNS[-1]]
    assert all(torch.isfinite(t).all() for t in ref)
    for key in RUNS[:-1]:
        for i, (a, b) in enumerate(zip(res[key], ref)):
            assert torch.equal(a, b), "run %s differs from the two-kernel route in output %d: max |d| %g" % (
                key, i, (a - b).abs().max().item())


def test_eval_bit_equal(dev, net, monkeypatch):
    cfg_path, size, precision = net
    state, (x, _) = _state0(cfg_path), _inputs(size)
    res = {}
    for fuse, plan in RUNS:
        monkeypatch.setenv("MCAMD_FUSE_BN_1X1", fuse)
        monkeypatch.setenv("MCAMD_PLAN", plan)
        m = _model(cfg_path, dev, state, precision).eval()
        with torch.no_grad():
            res[(fuse, plan)] = m(x.to(dev)).clone()
        _took_route(m, fuse, size, must=True)
        del m
    assert torch.isfinite(res[RUNS[-1]]).all()
    for key in RUNS[:-1]:
        assert torch.equal(res[key], res[RUNS[-1]]), key
