"""What the exact bn_conv1x1_kernel tests (test_bn1x1_instances_gpu.py) rest on, checked without a GPU: the sweep of
mcamd_bn_act_conv1x1_info -- the launch's own choice function -- reaches the six instances the launch can start and no other;
the case table names the instance the query names, covers every instance in both kinds and every boundary tag on both column
tiles; every case's operands and reference meet the conditions of exactness; the value cases' references hold the planted
conversion edges; and the query refuses what the launch entry refuses."""
import ctypes as C
import functools
import os
import re

import pytest
import torch

from modelcompression_amd import ops, _lib as L
import bn1x1_cases as BC

ALL = BC.CASES + BC.ONEHOT


@functools.lru_cache(maxsize=None)
def _ref(c):
    o = BC.operands(c)
    return o, BC.reference(c, o)


def test_query_is_declared_bound_exported_and_documented():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mcamd.h")).read(), flags=re.S)
    name = "mcamd_bn_act_conv1x1_info"
    assert name in set(re.findall(r"\b(mcamd_[a-z0-9_]+)\s*\(", hdr)) and name in L.SIGNATURES and hasattr(L.lib(), name)
    fields = re.search(r"typedef struct mcamd_bn_conv1x1_instance \{(.*?)\}", hdr, re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [f[0] for f in L.BnConv1x1Instance._fields_] == list(ops.BnConv1x1Info._fields)
    assert C.sizeof(L.BnConv1x1Instance) == 28
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    assert name in doc and "mcamd_bn_conv1x1_instance" in doc


def test_every_instance_is_reachable_and_no_other():
    seen = BC.reachable()
    assert set(seen) == set(BC.INSTANCES), set(seen) ^ set(BC.INSTANCES)
    # the launch dimensions are the instance's: 4 waves per 64 columns, two stages of (128 + BN) rows of 64 halfs
    for (bn, cb), (B, H, W, P, cout) in seen.items():
        i = BC.info_of(BC.case("probe", "value", B, H, W, P, cout, (bn, cb)))
        assert (i.bn, i.cb, i.threads, i.lds_bytes) == (bn, cb, 4 * bn, 2 * (128 + bn) * 8 * 16), i
        assert i.grid == ops.round_up(i.rows, 8) + 8 and 1 <= i.rows <= i.num_mtiles


def test_table_names_the_instance_the_query_names():
    for c in ALL:
        d, g = BC.act_desc_of(c), BC.geom_of(c)
        assert ops.bn_act_conv1x1_ok(d, g), c.name
        i = BC.info_of(c)
        assert (i.bn, i.cb) == c.expect, (c.name, i)
        assert i.rows == ops.bn_act_conv1x1_stats_rows(d, g) == ops.stats_rows(g, L.EPI_RAW_F32), c.name
        assert i.num_mtiles == -(-c.M // 128) and i.rows <= i.num_mtiles, (c.name, i)
        assert set(c.tags) <= BC.boundary_tags(c, i), (c.name, set(c.tags) - BC.boundary_tags(c, i))


def test_table_covers_every_instance_in_both_kinds():
    for kind, cases in (("exact", BC.EXACT), ("value", BC.VALUE)):
        got = {c.expect for c in cases}
        assert got == set(BC.INSTANCES), (kind, got ^ set(BC.INSTANCES))
    for special in ("onehot-hi", "onehot-lo"):
        assert {c.expect for c in BC.ONEHOT if c.special == special} == set(BC.INSTANCES), special


def test_table_covers_every_boundary_on_both_tiles():
    for bn in (64, 128):
        got = set()
        for c in BC.CASES:
            if c.expect[0] == bn:
                got |= BC.boundary_tags(c, BC.info_of(c))
        assert set(BC.BOUNDARIES) <= got, (bn, set(BC.BOUNDARIES) - got)
    # ragged cout on both tiles, at the narrowest cout each tile takes and in between
    for bn, lo in ((64, 40), (128, 104)):
        assert any(c.expect[0] == bn and c.cout == lo for c in BC.CASES) and any(c.expect[0] == bn and lo < c.cout < bn for c in BC.CASES), bn
    # the alignment edge of the 16-byte loads, in both kinds
    for kind in ("exact", "value"):
        assert any(c.kind == kind and c.py_choff % 8 == 4 for c in BC.CASES), kind


def test_persistent_slots_stay_with_the_existing_test():
    """"mtiles>slots" needs more tiles than the launch's slot target: the table leaves it to
    test_bn_conv1x1_gpu.py::test_persistent_workgroup_takes_two_tiles, whose shape carries the tag; no table case does."""
    c = BC.persistent_case()
    i = BC.info_of(c)
    assert "mtiles>slots" in BC.boundary_tags(c, i) and i.rows < i.num_mtiles < 2 * i.rows
    assert not any("mtiles>slots" in BC.boundary_tags(k, BC.info_of(k)) for k in ALL)


def test_table_sizes():
    for c in ALL:
        assert c.M * max(c.P, c.cout) <= 100000, c.name


@pytest.mark.parametrize("c", ALL, ids=str)
def test_operands_meet_the_conditions_of_exactness(c):
    o, ref = _ref(c)
    assert BC.exactness(c, o, ref) == [], c.name
    b1, b2 = BC.stats_bounds(c, ref)
    assert bool(torch.isfinite(ref.y).all()) and bool(torch.isfinite(b1).all()) and bool(torch.isfinite(b2).all())
    if c.kind == "exact":
        assert float(BC.y_bound(c, ref).max()) == 0.0
        # the derived slab bound is a small fraction of the sums it guards
        assert bool((b2 <= 2.0 ** -15 * ref.s2 + 1e-300).all()), c.name
    else:
        assert BC.planted_edges(c, ref) == [], c.name
        # the derived bound on y stays far below the lo plane's contribution: a launch that dropped a part would miss it
        part = ref.lo.abs() @ ref.w_hi.abs().t()
        assert float(BC.y_bound(c, ref).max()) < 0.01 * float(part.max()), c.name


@pytest.mark.parametrize("c", BC.ONEHOT, ids=str)
def test_onehot_results_name_their_channel(c):
    """Every output of a one-hot case is one triple of products, and over the filters it identifies the channel: laying the
    value at any other channel, or reading the other plane in any part, changes the row."""
    o, ref = _ref(c)
    M, P = c.M, c.P
    m = torch.arange(M)
    ch = BC.onehot_channel(m, P)
    assert set(ch.tolist()) == set(range(P)), "not every channel is hit"
    nz = (ref.v != 0)
    assert bool((nz.sum(1) == 1).all()) and torch.equal(nz.nonzero()[:, 1], ch)
    hi, lo = ref.hi[m, ch], ref.lo[m, ch]
    assert bool((lo == 0).all()) == (c.special == "onehot-hi") and bool((hi != 0).all())
    for other in (1, 8, 64 % P or 8):                                    # a neighbour, the next piece, the next K block
        k = (ch + other) % P
        moved = hi.view(M, 1) * (ref.w_hi[:, k].t() + ref.w_lo[:, k].t()) + lo.view(M, 1) * ref.w_hi[:, k].t()
        assert bool((moved != ref.y).any(1).all()), (c.name, other)
    wh, wl = ref.w_hi[:, ch].t(), ref.w_lo[:, ch].t()
    part1_reads_hi = hi.view(M, 1) * wh * 2 + hi.view(M, 1) * wl
    part2_reads_lo = hi.view(M, 1) * wh + lo.view(M, 1) * wh + lo.view(M, 1) * wl
    assert bool((part1_reads_hi != ref.y).all()) and bool((part2_reads_lo != ref.y).all()), c.name


def test_query_refuses_what_the_launch_refuses():
    """The refusals of test_bn_conv1x1_gpu.py::test_refusals, and a null output: MCAMD_EINVAL with the predicate's reason."""
    B, H, W, P = 2, 9, 8, 128
    ok = BC.case("ok", "value", B, H, W, P, 64, (64, 2))
    d_ok = BC.act_desc_of(ok)

    def act(**over):
        kw = dict(planes=2, dst_plane=P, dst_pad=0)
        kw.update(over)
        return ops.act_geom(B, H, W, P, P, 0, 0.1, L.DST_PLAIN, 2 * P, 0, **kw)
    refused = {
        "cout256": (d_ok, ops.geom(B, H, W, 1, 3 * P, 256, 2 * P, 0, 0, 0, 2 * P)),
        "cin96": (ops.act_geom(B, H, W, 96, 96, 0, 0.1, L.DST_PLAIN, 192, 0, planes=2, dst_plane=96, dst_pad=0),
                  ops.geom(B, H, W, 1, 288, 64, 192, 0, 0, 0, 192)),
        "shared-halo": (act(dst_pad=1), ops.geom(B, H, W, 1, 3 * P, 64, 2 * P, 0, 0, 1, 2 * P)),
        "x_f8": (act(planes=4), ops.geom(B, H, W, 1, 2 * P, 64, 2 * P, 0, 0, 0, 0, x_f8=P)),
        "cout32": (d_ok, ops.geom(B, H, W, 1, 3 * P, 32, 2 * P, 0, 0, 0, 2 * P)),
        "cout72": (d_ok, ops.geom(B, H, W, 1, 3 * P, 72, 2 * P, 0, 0, 0, 2 * P)),
        "cin192-cout64": (ops.act_geom(B, H, W, 192, 192, 0, 0.1, L.DST_PLAIN, 384, 0, planes=2, dst_plane=192, dst_pad=0),
                          ops.geom(B, H, W, 1, 576, 64, 384, 0, 0, 0, 384)),
        "py_choff2": (ops.act_geom(B, H, W, P, P + 4, 2, 0.1, L.DST_PLAIN, 2 * P, 0, planes=2, dst_plane=P, dst_pad=0), BC.geom_of(ok)),
    }
    lib = L.lib()
    out = L.BnConv1x1Instance()
    assert lib.mcamd_bn_act_conv1x1_info(C.byref(d_ok), C.byref(BC.geom_of(ok)), C.byref(out)) == 0 and (out.bn, out.cb) == (64, 2)
    for name, (d, g) in refused.items():
        assert not ops.bn_act_conv1x1_ok(d, g), name
        with pytest.raises(L.McamdError, match="mcamd_bn_act_conv1x1_ok"):
            ops.bn_act_conv1x1_info(d, g)
        # the launch entry gives the same code and the same reason (the predicate runs before any pointer is read)
        rc_q = lib.mcamd_bn_act_conv1x1_info(C.byref(d), C.byref(g), C.byref(out))
        why_q = lib.mcamd_last_error().split(b": ", 1)[1]
        rc_l = lib.mcamd_bn_act_conv1x1_fwd(C.byref(d), C.byref(g), None, None, None)
        why_l = lib.mcamd_last_error().split(b": ", 1)[1]
        assert rc_q == rc_l != 0 and why_q == why_l, (name, rc_q, rc_l, why_q, why_l)
    assert lib.mcamd_bn_act_conv1x1_info(C.byref(d_ok), C.byref(BC.geom_of(ok)), None) != 0
    assert lib.mcamd_bn_act_conv1x1_info(None, None, C.byref(out)) != 0
