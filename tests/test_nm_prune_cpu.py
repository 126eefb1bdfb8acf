"""nm_prune without a GPU: the CPU path raises (there is none), and the 2:4 entry points are bound."""
import pytest

from modelcompression_amd import nets, YOLOV2_VOC_CFG, _lib
from modelcompression_amd._lib import McamdError
from modelcompression_amd.pruning.weightPruning.methods import nm_prune


def test_nm_prune_cpu_model_raises():
    m = nets.Darknet(YOLOV2_VOC_CFG)
    with pytest.raises(McamdError):
        nm_prune(m)


def test_nm_prune_only_2_4():
    m = nets.Darknet(YOLOV2_VOC_CFG)
    with pytest.raises(McamdError):
        nm_prune(m, 1, 4)


def test_sparse_symbols_declared():
    for name in ("mcamd_nm_mask", "mcamd_nm_violations", "mcamd_pack_sparse24", "mcamd_sparse24_elems",
                 "mcamd_conv_fwd_sparse24", "mcamd_conv_fwd_sparse24_ok"):
        assert name in _lib.SIGNATURES


def test_model_sparse_defaults_to_none():
    assert nets.Darknet(YOLOV2_VOC_CFG).sparse is None
