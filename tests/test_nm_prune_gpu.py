"""nm_prune (2:4 magnitude pruning along the input channels, an addition beyond the reference) against a numpy
restatement: per group of 4 consecutive input channels at a fixed (filter, tap), a stable argsort of -|w * old_mask|
keeps its first 2 entries (with their old mask value)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import nets, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import nm_prune, weight_prune  # noqa: E402
from modelcompression_amd.synthetic import init_synthetic  # noqa: E402


def nm_ref(w, old):
    """numpy restatement of the 2:4 mask of one OIHW tensor."""
    O, I = w.shape[:2]
    if I % 4 != 0:
        return old.copy()
    a = np.abs(w * old).reshape(O, I // 4, 4, -1)                 # [O][group][4][tap]
    order = np.argsort(-a, axis=2, kind="stable")
    rank = np.argsort(order, axis=2, kind="stable")
    keep = (rank < 2).astype(np.float32)
    return (keep * old.reshape(O, I // 4, 4, -1)).reshape(w.shape).astype(np.float32)


def model(dev, seed=0):
    m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), seed).to(dev)
    return m


def inject_ties(m):
    """Equal magnitudes inside some groups (both signs): the lower channel must win."""
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 4 and p.shape[1] % 4 == 0:
                p[:, 0:4, 0, 0] = 0.5
                p[0, 4:8, 0, 0] = torch.tensor([-0.25, 0.25, 0.25, -0.25])
                p[1, 8:12, -1, -1] = torch.tensor([0.0, 0.0, 0.0, 0.0])
                p[2, 12:16, 0, -1] = torch.tensor([0.1, -0.3, 0.3, 0.1])


def check(m, masks, olds):
    ps = [p for p in m.parameters() if p.dim() != 1]
    assert len(masks) == len(ps)
    for p, mk, old in zip(ps, masks, olds):
        ref = nm_ref(p.detach().cpu().numpy(), old)
        assert mk.shape == p.shape and mk.dtype == torch.float32
        assert np.array_equal(mk.cpu().numpy(), ref)


def test_nm_prune_matches_numpy(dev):
    m = model(dev)
    inject_ties(m)
    masks = nm_prune(m)
    olds = [np.ones(tuple(p.shape), np.float32) for p in m.parameters() if p.dim() != 1]
    check(m, masks, olds)
    # unmasked layers with Cin % 4 == 0 keep exactly half; conv1 (3 input channels) is all ones
    for p, mk in zip([p for p in m.parameters() if p.dim() != 1], masks):
        if p.shape[1] % 4 == 0:
            assert int(mk.sum().item()) * 2 == p.numel()
        else:
            assert bool((mk == 1).all())
    assert masks[0].shape[1] == 3 and bool((masks[0] == 1).all())


def test_nm_prune_composes_with_weight_prune(dev):
    m = model(dev, seed=1)
    inject_ties(m)
    wm = weight_prune(m, 50.0)
    m.set_masks(wm)
    olds = [k.cpu().numpy() for k in wm]
    masks = nm_prune(m)
    check(m, masks, olds)
    for mk, old in zip(masks, wm):
        assert bool((mk <= old).all())                      # never revives a pruned weight
    assert torch.equal(masks[0], wm[0])                     # conv1: its old mask unchanged


@pytest.mark.parametrize("nm", [(1, 4), (2, 8), (4, 8), (1, 2)])
def test_nm_prune_other_patterns_raise(dev, nm):
    m = model(dev)
    with pytest.raises(McamdError):
        nm_prune(m, *nm)
