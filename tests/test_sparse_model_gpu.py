"""Darknet.sparse = "2:4": inference of an nm_prune-masked YOLOv2-VOC on the sparse MFMA (csrc/conv_sparse.hip) -- which
blocks go sparse, accuracy against the fp32 masked-dense oracle and the dense fp16 engine, no allocation in a warm
forward, the precision rule, and training left untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, YOLOV2_VOC_CFG, ops  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import nm_prune  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from util import rel_l2  # noqa: E402


def pruned(dev, seed=0):
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    m = nets.Darknet(YOLOV2_VOC_CFG)
    m.load_state_dict(O.init_state(blocks, seed=seed))
    m.to(dev)
    masks = nm_prune(m)
    m.set_masks(masks)
    return blocks, m, masks


def engine(m):
    return [e for e in m._engines.values() if not e.train_layout][0]


def test_sparse_yolov2_layers_and_accuracy(dev):
    blocks, m, masks = pruned(dev)
    m.eval()
    m.precision = "fp16"
    x1 = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ref1 = O.forward(blocks, {k: v.cpu() for k, v in m.state_dict().items()}, x1, training=False,
                         masks=[k.cpu() for k in masks])
        d1 = m(x1.to(dev)).cpu()
        m.sparse = "2:4"
        s1 = m(x1.to(dev)).cpu()
    assert engine(m).sparse_layers == list(range(2, 23))
    es, ed = rel_l2(s1, ref1), rel_l2(d1, ref1)
    print("B=1 vs fp32 masked-dense oracle: 2:4 %.2e, dense fp16 %.2e" % (es, ed))
    assert es < 1.5 * ed + 5e-4 and es < 2.5e-3
    # B = 128 and a non-square input against the dense fp16 engine on the same masked weights
    for (B, H, W) in ((128, 416, 416), (4, 352, 480)):
        x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
        with torch.no_grad():
            m.sparse = None
            d = m(x)
            m.sparse = "2:4"
            s = m(x)
            assert len(engine_for(m, x).sparse_layers) > 0
            e = rel_l2(s.cpu(), d.cpu())
            m.sparse = None                 # and back: the recorded forward plan must switch to the dense launches again
            assert torch.equal(m(x), d) and engine_for(m, x).sparse_layers == []
            m.sparse = "2:4"
            assert torch.equal(m(x), s)
        print("B=%d %dx%d: 2:4 vs dense fp16 engine rel-L2 %.2e" % (B, H, W, e))
        assert e < 1e-3
    # a warm forward allocates nothing from the device
    with torch.no_grad():
        m(x)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats(dev)
        m(x)
        torch.cuda.synchronize()
        after = torch.cuda.memory_stats(dev)
    assert after["num_alloc_retries"] == before["num_alloc_retries"]
    assert after["segment.all.allocated"] == before["segment.all.allocated"]


def engine_for(m, x):
    return [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and not e.train_layout][0]


def test_sparse_needs_fp16_eval(dev):
    _, m, _ = pruned(dev, seed=1)
    m.eval()
    m.sparse = "2:4"
    x = torch.rand(1, 3, 416, 416).to(dev)
    for prec in ("mixed", "auto", "fp16x3"):
        m.precision = prec
        with torch.no_grad(), pytest.raises(McamdError):
            m(x)
    m.precision = "fp16"
    m.sparse = "3:4"
    with torch.no_grad(), pytest.raises(McamdError):
        m(x)


def test_sparse_training_untouched(dev):
    """A training step with sparse="2:4" set is bit-identical to the same step without it; the masks stay 2:4."""
    results = []
    for mode in (None, "2:4"):
        torch.manual_seed(0)
        _, m, masks = pruned(dev, seed=2)
        m.train()
        m.precision = "fp16"
        m.sparse = mode
        opt = torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9)
        x = torch.rand(4, 3, 416, 416, generator=torch.Generator().manual_seed(6)).to(dev)
        out = m(x)
        loss = (out.float() ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        results.append((out.detach().clone(), [p.detach().clone() for p in m.parameters()]))
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        for p in m.parameters():
            if p.dim() == 4 and p.shape[1] % 4 == 0:
                ops.nm_violations((p.detach() != 0).float().contiguous(), cnt)
        assert int(cnt.item()) == 0
    assert torch.equal(results[0][0], results[1][0])
    assert all(torch.equal(a, b) for a, b in zip(results[0][1], results[1][1]))
