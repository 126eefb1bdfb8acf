"""mcamd_conv_bwd1x1_ok and its queries (host logic, no GPU), and which blocks the engine sends down the one-launch backward:
of yolov2-voc.cfg at B = 64, 416 x 416 exactly conv4 and conv7 -- the other 1x1 blocks have no (cout, cin) instance, the 3x3
blocks have taps -- and no block that runs a compacted or folded geometry."""
import types

import pytest
import torch

from modelcompression_amd import ops
from modelcompression_amd.engine import Engine

B = 64
# (conv number, H = W, cin, cout, ksize) of reference cfg/yolov2-voc.cfg behind the first block
VOC = [(2, 208, 32, 64, 3), (3, 104, 64, 128, 3), (4, 104, 128, 64, 1), (5, 104, 64, 128, 3), (6, 52, 128, 256, 3),
       (7, 52, 256, 128, 1), (8, 52, 128, 256, 3), (9, 26, 256, 512, 3), (10, 26, 512, 256, 1), (11, 26, 256, 512, 3),
       (12, 26, 512, 256, 1), (13, 26, 256, 512, 3), (14, 13, 512, 1024, 3), (15, 13, 1024, 512, 1), (16, 13, 512, 1024, 3),
       (17, 13, 1024, 512, 1), (18, 13, 512, 1024, 3), (19, 13, 1024, 1024, 3), (20, 13, 1024, 1024, 3), (21, 26, 512, 64, 1),
       (22, 13, 1280, 1024, 3), (23, 13, 1024, 125, 1)]
GRID = 256               # MCAMD_BWD1X1_GRID (csrc/kernels.h): one workgroup per CU


def geom(H, cin, cout, k, pad=0, **kw):
    # the split-operand engines' input buffers hold a hi and a lo plane: rows of 2 cin, the block reads the first cin
    return ops.geom(B, H, H, k, cin, cout, kw.pop("x_ld", 2 * cin), kw.pop("x_choff", 0), pad=pad, **kw)


def test_predicate_accepts_exactly_conv4_and_conv7():
    for pad in (0, 1):
        accepted = [n for n, H, cin, cout, k in VOC if ops.conv_bwd1x1_ok(geom(H, cin, cout, k, pad))[0]]
        assert accepted == [4, 7]


@pytest.mark.parametrize("n", [v[0] for v in VOC if v[0] not in (4, 7)])
def test_refusals_say_why(n):
    _, H, cin, cout, k = next(v for v in VOC if v[0] == n)
    g = geom(H, cin, cout, k)
    ok, why = ops.conv_bwd1x1_ok(g)
    assert not ok
    assert ("ksize must be 1" in why) if k == 3 else (("multiples of 8" in why) if n == 23 else ("no kernel instance" in why))
    assert ops.conv_bwd1x1_sums_rows(g) == 0 and ops.conv_bwd1x1_wgrad_splits(g) == 0 and ops.conv_bwd1x1_workspace_bytes(g) == 0


def test_refused_forms_and_alignment():
    assert ops.conv_bwd1x1_ok(geom(104, 128, 64, 1))[0]
    for g, word in ((geom(104, 128, 64, 1, x_wrap=256), "dense geometry"),                  # the forward's wrapped operand
                    (geom(104, 128, 64, 1, x_f8=2), "dense geometry"),
                    (geom(104, 128, 64, 1, x_ld=132), "groups of 8"),
                    (geom(104, 128, 64, 1, x_ld=256, x_choff=132), "groups of 8"),
                    (geom(104, 128, 64, 1, x_ld=128, x_choff=8), "groups of 8"),            # slice past the row
                    (ops.geom(B, 416, 416, 3, 3, 32, 4, 0, stem=1), "ksize must be 1")):
        ok, why = ops.conv_bwd1x1_ok(g)
        assert not ok and word in why, (why, word)
    assert ops.conv_bwd1x1_ok(geom(104, 128, 64, 1, x_ld=512, x_choff=136))[0]              # a concat member at an offset


def test_row_queries():
    for n in (4, 7):
        _, H, cin, cout, k = next(v for v in VOC if v[0] == n)
        for batch in (1, 2, B):
            g = ops.geom(batch, H, H, k, cin, cout, 2 * cin)
            # the grid is a function of nothing but the kernel: sums rows = weight-gradient splits = workgroups
            assert ops.conv_bwd1x1_sums_rows(g) == ops.conv_bwd1x1_wgrad_splits(g) == GRID
            assert ops.conv_bwd1x1_workspace_bytes(g) == GRID * cout * cin * 4


def _engine_stub(geoms, on=True):
    lays = [types.SimpleNamespace(li=i + 1, gin=object(), fused_stem=False, stem_shadow=False, fold=None, gather=False,
                                  in_perm=None, geom=g, geom_act=g) for i, g in enumerate(geoms)]
    eng = types.SimpleNamespace(bwd1x1=on, _plan_epoch=0, _bwd1x1_cache={}, _bwd1x1_ws=None, layers=lays,
                                device=torch.device("cpu"))
    return eng, lays


def test_engine_routes_conv4_and_conv7_only():
    eng, lays = _engine_stub([geom(H, cin, cout, k, pad=1) for _, H, cin, cout, k in VOC])
    took = [VOC[i][0] for i, lay in enumerate(lays) if Engine._bwd1x1_route(eng, lay)]
    assert took == [4, 7]
    # one workspace for both, sized for the larger (conv7: 128 x 256 floats per workgroup)
    assert eng._bwd1x1_ws.numel() == GRID * 128 * 256 * 4
    off, lays0 = _engine_stub([geom(H, cin, cout, k, pad=1) for _, H, cin, cout, k in VOC], on=False)
    assert not any(Engine._bwd1x1_route(off, lay) for lay in lays0) and off._bwd1x1_ws is None


@pytest.mark.parametrize("what", ["gather", "compacted-geometry", "fold", "in_perm", "first-block", "no-gin"])
def test_engine_keeps_compacted_and_folded_blocks_on_two_launches(what):
    g = geom(104, 128, 64, 1, pad=1)
    eng, (lay,) = _engine_stub([g])
    assert Engine._bwd1x1_route(eng, lay)
    eng, (lay,) = _engine_stub([g])
    if what == "gather":
        lay.gather = True                                  # kept filters only, scattered by the finish kernel's maps
    elif what == "compacted-geometry":
        lay.geom_act = geom(104, 128, 64, 1, pad=1)        # the launch geometry is not the dense one (equal numbers or not)
    elif what == "fold":
        lay.fold = object()                                # kept inputs + the ones channel
    elif what == "in_perm":
        lay.in_perm = object()
    elif what == "first-block":
        lay.li = 0
    else:
        lay.gin = None
    assert not Engine._bwd1x1_route(eng, lay)
