"""Coverage of tests/test_bsparse_wgrad_instances_gpu.py, proved without a GPU: what mcamd_conv_wgrad_bsparse can launch (asked
from the launch's own plan function through mcamd_conv_wgrad_bsparse_plan), that the cases of tests/bsparse_wgrad_cases.py
reach wgrad9_kernel at both pixel steps, the one-tap 64 x 64 instance of wgrad_kernel and every lane grouping of the finish
kernel's select form, which geometries are accepted, how the split count follows the kept tile count, and that EQUAL is the
right comparison for every case.  The numpy restatement of the lists is checked on masks whose lists are known by hand."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops, _lib as L  # noqa: E402
import bsparse_wgrad_cases as BC  # noqa: E402


def test_accepted_and_refused_geometries(setenv):
    setenv("MCAMD_WGRAD9", "1")
    ok = ops.conv_wgrad_bsparse_ok
    assert ok(ops.geom(2, 13, 13, 3, 128, 128, 128)) and ok(ops.geom(2, 13, 13, 1, 128, 128, 128))
    assert ok(ops.geom(2, 13, 13, 3, 128, 128, 128, pad=1)) and ok(ops.geom(1, 4, 208, 3, 64, 64, 64))
    assert ok(ops.geom(2, 13, 13, 1, 64, 128, 192, 128))                         # an input slice inside a wider buffer
    assert not ok(ops.geom(2, 13, 13, 3, 96, 128, 96)), "cin % 64"
    assert not ok(ops.geom(2, 13, 13, 1, 128, 96, 128)), "cout % 64"
    assert not ok(ops.geom(2, 13, 13, 3, 128, 160, 128)), "cout % 64"
    assert not ok(ops.geom(1, 4, 216, 3, 64, 64, 64)), "the 9-tap kernel stops at 208 pixels per row"
    assert ok(ops.geom(1, 4, 216, 1, 64, 64, 64)), "... the 1x1 kernel does not"
    assert not ok(ops.geom(2, 16, 16, 3, 3, 64, 4, stem=1)), "stem"
    for field, value in (("x_wrap", 128), ("x_f8", 64)):
        h = ops.geom(2, 13, 13, 3, 128, 128, 128)
        setattr(h, field, value)
        assert not ok(h), field
    setenv("MCAMD_WGRAD9", "0")                    # what mcamd_wgrad_use9 requires: the switch
    assert not ok(ops.geom(2, 13, 13, 3, 128, 128, 128)) and ok(ops.geom(2, 13, 13, 1, 128, 128, 128))
    setenv("MCAMD_WGRAD9", "1")
    assert ops.wgrad_bsparse_elems(ops.geom(2, 13, 13, 3, 128, 192, 128)) == (6, 12)
    assert ops.wgrad_bsparse_elems(ops.geom(2, 13, 13, 1, 1280, 1024, 1280)) == (320, 640)
    for call in (ops.wgrad_bsparse_elems, lambda g: ops.conv_wgrad_bsparse_plan(g, 1)):
        with pytest.raises(L.McamdError):
            call(ops.geom(2, 13, 13, 3, 96, 128, 96))
    with pytest.raises(L.McamdError):
        ops.conv_wgrad_bsparse_plan(ops.geom(2, 13, 13, 3, 128, 128, 128), 5)     # 4 tiles
    assert len(L.SIGNATURES["mcamd_conv_wgrad_bsparse"][1]) == 16


def test_cases_reach_every_instance(setenv):
    setenv("MCAMD_WGRAD9", "1")
    cs = BC.WGRAD_BSPARSE_CASES
    assert len({c.name for c in cs}) == len(cs)
    comp, fin, kinds = set(), set(), {}
    for c in cs:
        g = BC.geom_of(c)
        assert ops.conv_wgrad_bsparse_ok(g), c.name
        gen = torch.Generator().manual_seed(1)
        tiles, words, allw, (nt, npairs) = BC.lists_of(BC.make_mask(c, gen).numpy())
        p = ops.conv_wgrad_bsparse_plan(g, nt)
        nsplit = c.nsplit or p.nsplit
        assert p.finish == L.WFIN_VEC, (c.name, p)
        got = (BC.compute_of(p), (BC.VEC, c.k * c.k, BC.finish_sg(nsplit)))
        assert got == c.expect, (c.name, got)
        if c.k == 3:
            assert p.kp == BC.nine_kp(c), c.name
        assert (p.nsplit, p.pix_per_split) == BC.split_rule(c, nt), (c.name, p)
        assert p.bytes == p.nsplit * c.cout * c.cin * c.k * c.k * 4
        want = set(c.tags) | BC.REQUIRED_TAGS.get(c.name, set())
        assert want <= BC.tags_of(c, nsplit), (c.name, want, BC.tags_of(c, nsplit))
        comp.add(got[0])
        fin.add(got[1])
        kinds.setdefault(got[0], set()).add(c.mask)
        # EQUAL is the right comparison: integer operands in [-3, 3], every partial sum below 2^24
        assert 3 * 3 * BC.pixels_enumerated(c) < 2 ** 24, c.name
        # the mask kind is what its name says
        if c.mask == "empty":
            assert nt == 0 and npairs == 0
        if c.mask == "full":
            assert nt == len(allw) and npairs == nt * c.k * c.k
        if c.mask == "tile-cleared":
            assert allw[0] == 0 and nt >= 1 and 0 not in tiles
        if c.mask == "one-tap" and c.k == 3:
            assert allw[-1] == 1 << 8 and tiles[-1] == len(allw) - 1
        if c.mask == "unaligned":
            m = BC.make_mask(c, torch.Generator().manual_seed(1))
            blocks = m.reshape(c.cout // 64, 64, c.cin // 64, 64, -1).permute(0, 2, 4, 1, 3).reshape(-1, 64 * 64)
            part = (blocks.sum(1) > 0) & (blocks.sum(1) < 64 * 64)
            assert bool(part.any()), "a kept block with holes that no block mask would have"
    assert comp == {BC.N64, BC.N32, BC.G1}
    # every finish kernel the plan can name: the vector kernel's select form at SG 1 / 8 / 32, for both kernel sizes
    assert fin == {(BC.VEC, kk, sg) for kk in (1, 9) for sg in (1, 8, 32)}
    for inst in (BC.N64, BC.N32, BC.G1):
        assert kinds[inst] >= set(BC.MASK_KINDS), (inst, kinds[inst])


def test_the_plan_can_name_nothing_else(setenv):
    """Over channel counts, images from one tile to the training batch and every kept tile count: the 9-tap kernel at 32 or 64
    pixels per step (never the wide form) or the one-tap 64 x 64 instance, always the vector finish kernel."""
    setenv("MCAMD_WGRAD9", "1")
    seen = set()
    for (B, H, W) in ((1, 8, 8), (2, 13, 13), (8, 26, 26), (64, 13, 13), (8, 52, 52), (64, 104, 104), (16, 208, 208)):
        for cin, cout in ((64, 64), (128, 256), (1280, 1024), (512, 1024)):
            for k in (1, 3):
                g = ops.geom(B, H, W, k, cin, cout, cin)
                nt = ops.wgrad_bsparse_elems(g)[0]
                for kept in sorted({0, 1, min(2, nt), nt // 4, nt // 2, nt}):
                    p = ops.conv_wgrad_bsparse_plan(g, kept)
                    seen.add((BC.compute_of(p), p.finish, p.sg))
    assert {s[0] for s in seen} == {BC.N64, BC.N32, BC.G1}
    assert {s[1] for s in seen} == {L.WFIN_VEC} and {s[2] for s in seen} == {1, 8, 32}


def test_nsplit_follows_the_kept_tile_count(setenv):
    """The split rule is the dense plans' cost rule on the kept tile count: restated in bsparse_wgrad_cases.split_rule.  Fewer
    kept tiles never give fewer splits, on full lists a 3x3 geometry whose dense plan is the narrow 9-tap kernel gets the dense
    plan's split, and the launch takes whatever count it is handed (mcamd_conv_wgrad_bsparse's nsplit argument)."""
    setenv("MCAMD_WGRAD9", "1")
    setenv("MCAMD_WGRAD9W", "1")
    setenv("MCAMD_WGRAD9W_MINW", "40")
    differ = 0
    for (B, H, W, k, cin, cout) in ((64, 13, 13, 3, 1024, 1024), (64, 13, 13, 1, 1024, 512), (64, 26, 26, 3, 256, 512),
                                    (64, 26, 26, 1, 512, 256), (2, 13, 13, 3, 128, 128), (8, 52, 52, 3, 128, 256)):
        c = BC.case("g", B, H, W, k, cin, cout, "full", None)
        g = BC.geom_of(c)
        nt = ops.wgrad_bsparse_elems(g)[0]
        last = None
        for kept in range(0, nt + 1, max(1, nt // 32)):
            p = ops.conv_wgrad_bsparse_plan(g, kept)
            assert (p.nsplit, p.pix_per_split) == BC.split_rule(c, kept), (B, H, W, k, cin, cout, kept, p)
            last = last or p.nsplit
        full, few = ops.conv_wgrad_bsparse_plan(g, nt), ops.conv_wgrad_bsparse_plan(g, max(1, nt // 8))
        differ += few.nsplit != full.nsplit
        dense = ops.wgrad_plan_info(g)
        if dense.family == L.WGRAD_NINE:
            assert (dense.kp, dense.nsplit, dense.pix_per_split) == (full.kp, full.nsplit, full.pix_per_split)
        assert ops.conv_wgrad_bsparse_plan(g, 0).nsplit == ops.conv_wgrad_bsparse_plan(g, 1).nsplit
    assert differ >= 3, "the split count must depend on the kept tile count"


def test_lists_restatement_on_known_masks():
    m = np.zeros((128, 192, 3, 3), np.float32)
    m[0, 0, 0, 0] = 1.0            # tile 0, tap 0
    m[63, 191, 2, 2] = -2.0        # tile 2, tap 8
    m[64, 64, 1, 1] = 1.0          # tile 4, tap 4
    m[127, 127, 1, 2] = 0.5        # tile 4, tap 5
    m[100, 10, 0, 0] = -0.0        # minus zero is zero
    tiles, words, allw, counts = BC.lists_of(m)
    assert tiles.tolist() == [0, 2, 4] and words.tolist() == [1, 256, 48] and allw.tolist() == [1, 0, 256, 0, 48, 0]
    assert counts == (3, 4)
    m1 = np.zeros((128, 128, 1, 1), np.float32)
    m1[70, 5] = 1.0
    tiles, words, allw, counts = BC.lists_of(m1)
    assert tiles.tolist() == [2] and words.tolist() == [1] and counts == (1, 1)
