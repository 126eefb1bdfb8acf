"""mcamd_bn_act_conv1x1_ok (host logic, no GPU): over the convolution blocks of yolov2-voc.cfg at B = 64, 416 x 416, each as
the split-operand consumer of a PLAIN producer that writes hi | lo planes, the predicate accepts exactly conv4's and conv7's
forward.  conv10 / 12 / 15 / 17 have more filters than one column tile, conv21 more input channels than a thread can keep
converted, conv23 a filter count that is no multiple of 8; the 3x3 blocks have taps."""
import pytest

from modelcompression_amd import ops
from modelcompression_amd import _lib as L

B = 64
# (conv number, H = W, cin, cout, ksize) of reference cfg/yolov2-voc.cfg behind the first block
VOC = [(2, 208, 32, 64, 3), (3, 104, 64, 128, 3), (4, 104, 128, 64, 1), (5, 104, 64, 128, 3), (6, 52, 128, 256, 3),
       (7, 52, 256, 128, 1), (8, 52, 128, 256, 3), (9, 26, 256, 512, 3), (10, 26, 512, 256, 1), (11, 26, 256, 512, 3),
       (12, 26, 512, 256, 1), (13, 26, 256, 512, 3), (14, 13, 512, 1024, 3), (15, 13, 1024, 512, 1), (16, 13, 512, 1024, 3),
       (17, 13, 1024, 512, 1), (18, 13, 512, 1024, 3), (19, 13, 1024, 1024, 3), (20, 13, 1024, 1024, 3), (21, 26, 512, 64, 1),
       (22, 13, 1280, 1024, 3), (23, 13, 1024, 125, 1)]


def pair(H, cin, cout, k):
    d = ops.act_geom(B, H, H, cin, cin, 0, 0.1, L.DST_PLAIN, 2 * cin, 0, planes=2, dst_plane=cin, dst_pad=0)
    g = ops.geom(B, H, H, k, 3 * cin, cout, 2 * cin, 0, 0, 0, 2 * cin)
    return d, g


def test_predicate_accepts_exactly_conv4_and_conv7():
    accepted = [n for n, H, cin, cout, k in VOC if ops.bn_act_conv1x1_ok(*pair(H, cin, cout, k))]
    assert accepted == [4, 7]


@pytest.mark.parametrize("n", [10, 12, 15, 17, 21, 23])
def test_other_1x1_blocks_are_refused(n):
    _, H, cin, cout, k = next(v for v in VOC if v[0] == n)
    d, g = pair(H, cin, cout, k)
    assert k == 1 and not ops.bn_act_conv1x1_ok(d, g)
    assert ops.bn_act_conv1x1_stats_rows(d, g) == 0


def test_accepted_rows_are_the_two_kernel_route_s():
    """The fused launch keeps the persistent slots of the forward it replaces: same slab shape."""
    for n in (4, 7):
        _, H, cin, cout, k = next(v for v in VOC if v[0] == n)
        d, g = pair(H, cin, cout, k)
        assert ops.bn_act_conv1x1_stats_rows(d, g) == ops.stats_rows(g, L.EPI_RAW_F32) > 0


def test_narrow_consumer_is_refused():
    """Up to 32 filters the consumer's own forward takes igemm_kernel's 32-column tile, whose waves sum the statistics in
    rows of 32 pixels: the fused launch (rows of 64) could not reproduce that slab bit for bit."""
    assert ops.bn_act_conv1x1_ok(*pair(104, 128, 40, 1))
    assert not ops.bn_act_conv1x1_ok(*pair(104, 128, 32, 1))
