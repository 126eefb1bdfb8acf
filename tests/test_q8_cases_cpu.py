"""Coverage of tests/test_q8_instances_gpu.py, proved without a GPU: what the fp8 launches can choose (asked from their own
choice through mcamd_conv_fwd_q8_info), that the cases of tests/q8_cases.py reach all of it in both MFMA forms with every
destination form, every format pairing, every named boundary condition and every value edge, and that EQUAL is the right
comparison for every case."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops, _lib as L  # noqa: E402
import q8_cases as QC  # noqa: E402
import q8_ref as R  # noqa: E402
import q8_sparse_ref as SP  # noqa: E402
import sparse_cases as SC  # noqa: E402


def test_q8_instances_are_the_expected_set(setenv):
    """The twenty instances, and no other: four kernels x (128, 64 in the default form; 256, 128, 64 on the fp8 MFMA), over
    both settings of MCAMD_Q8_MFMA, every filter and channel count from 8 to 1344 in steps of 8 the form accepts and images
    from one pixel to the training batch."""
    seen = QC.reachable(setenv)
    assert seen == set(QC.INSTANCES) and len(seen) == 20


def test_q8_info_follows_the_switch(setenv):
    g = ops.geom(2, 13, 13, 3, 64, 512, 64)
    for form in (ops.Q8_FORM_INFER, ops.Q8_FORM_RAW, ops.Q8_FORM_BORDER, ops.Q8_FORM_SPARSE):
        setenv("MCAMD_Q8_MFMA", "1")
        assert tuple(ops.conv_fwd_q8_info(g, form)) == (256, 128, 1, 3, 3, 2, 16)
        setenv("MCAMD_Q8_MFMA", "0")
        assert tuple(ops.conv_fwd_q8_info(g, form)) == (128, 128, 0, 3, 3, 4, 32)
    slim = ops.geom(2, 13, 13, 3, 72, 40, 128)
    assert tuple(ops.conv_fwd_q8_info(slim, ops.Q8_FORM_BORDER)) == (64, 128, 0, 3, 3, 1, 8)
    with pytest.raises(L.McamdError):
        ops.conv_fwd_q8_info(slim, ops.Q8_FORM_INFER)           # cin % 64 != 0: the slim form only
    with pytest.raises(L.McamdError):
        ops.conv_fwd_q8_info(g, 4)


def test_q8_cases_reach_every_instance_and_boundary(setenv):
    cs = QC.Q8_CASES
    assert len({c.name for c in cs}) == len(cs)
    tags_of, by_inst = {}, {i: [] for i in QC.INSTANCES}
    for c in cs:
        QC.apply_env(c, setenv)
        g = QC.geom_of(c)
        assert ops.conv_fwd_q8_slim_ok(g) if c.fam == "slim" else ops.conv_fwd_q8_ok(g), c.name
        r = QC.info_of(c)
        assert QC.instance_of(c, r) == c.expect and (r.bnp, r.stages) == (128, 3), (c.name, r)
        o, ref = QC.operands_and_reference(c)
        t = QC.boundary_tags(c, r) | QC.value_tags(c, o, ref)
        assert set(c.tags) <= t, (c.name, r, set(c.tags) - t)
        # (a tag counts for the family, the MFMA form and the tile width of the case that claims or meets it)
        tags_of.setdefault((c.fam, r.f8mfma, "64" if r.bmw == 64 else "wide"), set()).update(t)
        by_inst[c.expect].append(c)
    per_family = {"dense": QC.BOUNDARIES_INFERENCE, "sparse": QC.BOUNDARIES_INFERENCE, "raw": QC.BOUNDARIES_RAW, "slim": QC.BOUNDARIES_SLIM}
    missing = {}
    for fam in QC.FORMS:
        for mfma in (0, 1):
            for width in ("64", "wide"):
                want = set(QC.BOUNDARIES_BOTH + per_family[fam] + (QC.BOUNDARIES_64 if width == "64" else ()))
                miss = want - tags_of.get((fam, mfma, width), set())
                if miss:
                    missing[(fam, mfma, width)] = miss
    assert missing == {}, missing
    # every instance with every destination form and every format pairing (the raw form has one: fp32 rows)
    for inst, mine in by_inst.items():
        assert mine, inst
        if inst[0] == "raw":
            assert {c.stats for c in mine} == {True, False}, inst
            continue
        if inst[0] == "dense":
            mine = [c for c in mine if c.fam == "dense"]       # (the slim launches without a table are extra)
        assert {c.dst for c in mine} == set(QC.DSTS), (inst, {c.dst for c in mine})
        assert {c.fmt for c in mine} == set(QC.FMTS), (inst, {c.fmt for c in mine})
        assert {c.k for c in mine} == {1, 3}, inst
        if inst[0] == "sparse":
            assert len({c.mask for c in mine}) >= 3, inst
    for kind in QC.MASK_KINDS:
        assert sum(1 for c in cs if c.mask == kind) >= 3, kind
    # slim: all border classes of a 3x3 kernel (a large image, H = 1, 2x2), with a table
    classes = set()
    for c in cs:
        if c.fam == "slim" and c.table and c.k == 3:
            classes |= QC.border_classes(c)
    assert classes >= QC.ALL_BORDER_CLASSES, QC.ALL_BORDER_CLASSES - classes
    assert {"H==1", "2x2", "table-null"} <= set().union(*(v for (fam, _, _), v in tags_of.items() if fam == "slim"))
    # every value edge somewhere, in the default form and (but for w-subnormal) on the fp8 MFMA
    for mfma in (0, 1):
        claimed = set().union(*(set(c.tags) for c in cs if c.mfma == mfma))
        want = set(QC.VALUE_TAGS) - ({"w-subnormal"} if mfma else set())
        assert want <= claimed, (mfma, want - claimed)
    # slope 1 in one case per family with an epilogue, a long chunk loop per family, the shapes' limits
    for fam in ("dense", "slim", "sparse"):
        assert any(c.slope == 1.0 for c in cs if c.fam == fam), fam
    for fam in QC.FORMS:
        assert any(c.cin == 1280 and c.k == 3 and (c.B, c.H, c.W) == (2, 13, 13) for c in cs if c.fam == fam), fam
    assert all(c.M <= 1200 and 8 <= c.cout <= 512 and (c.cin <= 328 or c.cin == 1280) for c in cs)
    names = {c.name: c for c in cs}
    assert {(names[n].kernel, names[n].mfma) for n in QC.DETERMINISM_CASES} == {(k, m) for k in QC.KERNELS for m in (0, 1)}


@pytest.mark.parametrize("c", QC.Q8_CASES, ids=str)
def test_q8_case_is_exact(c):
    """The conditions of exactness on this case's own reference (q8_cases.exactness), exact operand codes, exponents that
    differ from filter to filter, and the weights of the kind the case names."""
    for plant in ((True, False) if "overflow" in c.special else (True,)):
        o, ref = QC.operands_and_reference(c, plant)
        assert QC.exactness(c, o, ref) == [], c.name
        assert len(o.planted) == (2 if "overflow" in c.special and plant else 0)
    o, ref = QC.operands_and_reference(c)
    assert not bool(((o.a8 & 0x7F) == 0x7F).any()) and not bool(((ref.w8 & 0x7F) == 0x7F).any())
    wm = o.w if o.mask is None else o.w * o.mask
    # the weight codes are exact: deq(w8) = w * mask * 2^e
    assert torch.equal(R.deq(ref.w8).double(), wm.double() * torch.pow(2.0, ref.e.double()).view(-1, 1, 1, 1))
    assert len(set(ref.e.tolist())) >= 3 and len(set(ref.e[-min(c.cout, 64):].tolist())) >= 2
    if c.fam == "raw":
        assert bool(torch.isfinite(ref.raw).all()) and (ref.s1 is not None)
        return
    for t in (ref.y, ref.y2):
        if t is not None:
            assert t.dtype == torch.uint8 or bool(torch.isfinite(t).all())
    assert (ref.y2 is not None) == (c.dst == "pool+y2")
    if c.fam == "sparse":
        cnt = SC.group_counts(wm)
        eff = SC.first_two(wm)
        if c.mask == "bad":
            assert int(cnt.max()) == 4 and not torch.equal(eff, wm) and int(SC.group_counts(eff).max()) == 2
        else:
            assert int(cnt.max()) == 2 and torch.equal(eff, wm)
        if c.mask == "upto2":
            assert bool((cnt == 0).any()) and bool((cnt == 1).any()) and int((wm != 0).sum((1, 2, 3)).min()) == 0
        if c.mask == "none":
            assert o.mask is None
        # the packing restated: compress / decompress rebuild the codes the reference multiplies
        kept, words = SP.compress(ref.w8, SP.keep_positions(wm))
        assert torch.equal(R.deq(SP.decompress(kept, words)), R.deq(SP.dense_rows(ref.w8_eff)))
    if c.fam == "slim" and c.table:
        assert torch.equal(o.border * 4.0, (o.border * 4.0).round()) and bool((o.border != 0).any())
    if c.k_tap > c.cin:
        assert o.fill is not None and bool(((o.fill & 0x7F) != 0).all()) and bool(((o.fill & 0x7F) != 0x7F).all())


def test_q_against_the_integer_restatement():
    """q8_ref.q (torch's float8_e4m3fn cast behind a clamp) against q8_cases.q_int (clamp + round to nearest, ties to the even
    code, on integers) over every value 2 v that occurs in any case's reference -- ties, saturation, both zeros and
    subnormals included -- over every e4m3 value and every midpoint between neighbours, and around the clamp."""
    vals = [torch.tensor([0.0, -0.0, 448.0, -448.0, 449.0, 464.0, 465.0, 480.0, -480.0, 1e6, -1e6, 2.0 ** -10, -2.0 ** -10,
                          3 * 2.0 ** -11, 2.0 ** -11, -2.0 ** -11, 2.0 ** -9, 2.0 ** -6, 2.0 ** -6 - 2.0 ** -10], dtype=torch.float64)]
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    grid = R.deq(codes[(codes & 0x7F) != 0x7F]).double().sort().values
    vals += [grid, (grid[1:] + grid[:-1]) / 2, grid * (1 + 2.0 ** -20), grid * (1 - 2.0 ** -20)]
    for c in QC.Q8_CASES:
        if c.fam != "raw":
            _, ref = QC.operands_and_reference(c)
            vals.append(ref.v2x.flatten().unique())
    v = torch.cat(vals)
    assert torch.equal(v.float().double(), v), "fp32 numbers: q() sees them unrounded"
    got, tie, odd = QC.q_int(v)
    want = R.q(v.float())
    assert torch.equal(got, want), "%d codes differ; first value %r" % (int((got != want).sum()), float(v[got != want][0]))
    assert not bool(((want & 0x7F) == 0x7F).any())
    assert int(tie.sum()) > 1000 and bool((tie & odd).any()) and bool((tie & ~odd).any())
    # a tie goes to the even code: the stored code is even wherever the value was a tie
    assert bool(((got[tie] & 1) == 0).all())
