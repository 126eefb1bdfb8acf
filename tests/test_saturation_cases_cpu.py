"""The cases of tests/saturation_cases.py do what tests/test_grad_saturation_gpu.py relies on -- proved in float64, no GPU:
every G0 is an fp16 number, the planted element lands where intended (LeakyReLU side, window position) at 0.97 / 1.03 of the
clamp, and nothing else comes near it."""
import pytest
import torch

from modelcompression_amd import _lib as L
import saturation_cases as SC
from saturation_cases import ABOVE, BELOW, F16_MAX, PMEAN, PNEG, PPOS, PRUNED, S


def _others_max(dy, plants):
    d = dy.abs().clone()
    d[:, PRUNED] = 0.0                    # (the reference knows no dy_keep: the kernel writes exact zeros there)
    for p, ch in plants:
        d[p, ch] = 0.0
    return float(d.max())


@pytest.mark.parametrize("position", SC.POSITIONS)
@pytest.mark.parametrize("shape", list(SC.SHAPES))
@pytest.mark.parametrize("vname", [v[0] for v in SC.VARIANTS])
def test_plant_case(vname, shape, position):
    c = SC.build(vname, shape, position)
    dec = SC.decisions(c)
    pos, arg = dec
    N = c.M
    for src in SC.sources(c.variant):
        kap = SC.kappas(c, src, dec)
        assert kap[PPOS] > 0 > kap[PNEG]
        for ch in (PPOS, PNEG):
            pl = c.plants[src][ch]
            p = pl["p"]
            # the intended side, and the size kappa has by the formula
            assert bool(pos[p, ch]) == pl["positive"]
            s = 1.0 if pl["positive"] else c.slope
            ykd = c.yk[:, ch].double()
            xh = float((ykd[p] - ykd.mean()) * c.invstd[ch])
            formula = float(c.scale[ch]) * s * (1.0 - 1.0 / N - xh * xh / N)
            assert abs(kap[ch] - formula) <= 1e-6 * abs(formula), (kap[ch], formula)
            if c.mode == L.DST_POOL:
                q = pl["row"] if src == "g" else c.plants["g"][ch]["row"]
                b, rem = divmod(q, (c.H // 2) * (c.W // 2))
                a = int(arg[b, rem // (c.W // 2), rem % (c.W // 2), 0, ch])
                assert a == c.plants["g"][ch]["k"]                          # g lands on the window's argmax ...
                assert (a == pl["k"]) == (src == "g")                       # ... and g2 on another element of it
        for factor, lo, hi in ((BELOW, 0.95, 0.99), (ABOVE, 1.01, 1.05)):
            vals = {ch: SC.g0(kap[ch], factor) for ch in (PPOS, PNEG)}
            for v in vals.values():
                assert SC.f16(v) == v and 0 < v <= F16_MAX
            gq, g2q = SC.with_g(c, src, vals)
            dy = SC.reference(c, gq, g2q, dec)[0] * S                       # as stored: grad_scale x dY
            plants = [(c.plants[src][ch]["p"], ch) for ch in (PPOS, PNEG)]
            for (p, ch), sign in zip(plants, (1.0, -1.0)):
                t = float(dy[p, ch])
                assert lo * F16_MAX < sign * t < hi * F16_MAX, (vname, src, ch, t)
                assert int(dy[:, ch].abs().argmax()) == p                   # (reorg: the sub-position is that element)
            assert _others_max(dy, plants) < 0.5 * F16_MAX
            assert float(dy[:, PRUNED].abs().max()) > F16_MAX               # extreme without dy_keep: the kernel writes 0
    # positions: first and last item of the launch
    row = c.plants["g"][PPOS]["row"]
    assert row == {"first": 0, "middle": c.P // 2 + 1, "last": c.P - 1}[position]
    if position == "first":
        assert c.plants["g"][PPOS]["p"] == 0
    if position == "last":
        assert c.plants["g"][PPOS]["p"] == c.M - 1


def test_case_table_reaches_every_route():
    names = {v for v, _, _ in SC.plant_cases()}
    assert names == {v[0] for v in SC.VARIANTS} and len(names) == 18
    assert {s for _, s, _ in SC.plant_cases()} == set(SC.SHAPES)
    ks = {SC.WINDOW_K[p] for p in SC.POSITIONS}
    assert 0 in ks and 3 in ks
    fam = [SC.VARIANT[n] for n in SC.MEAN_VARIANTS]
    assert {(v[1], v[4], bool(v[5])) for v in fam} == {(L.DST_PLAIN, False, False), (L.DST_POOL, False, False),
                                                       (L.DST_POOL, True, False), (L.DST_REORG, False, False),
                                                       (L.DST_PLAIN, False, True), (L.DST_POOL, False, True)}
    assert all(v[6] == 0.1 for v in fam)
    assert set(SC.NONARG_VARIANTS) == {v[0] for v in SC.VARIANTS if v[1] == L.DST_POOL and not v[4]}


@pytest.mark.parametrize("vname", SC.MEAN_VARIANTS)
def test_mean_case(vname):
    c = SC.build(vname, "c64", kind="mean")
    dec = SC.decisions(c)
    assert abs(float(c.scale[PMEAN])) * SC.MEAN_G / 4 > ABOVE * F16_MAX
    gq, g2q = SC.with_g(c, channel_g=SC.MEAN_G)
    dy = SC.reference(c, gq, g2q, dec)[0] * S
    big = dy[:, PMEAN].abs() > ABOVE * F16_MAX
    assert int(big.sum()) > c.M // 2 and bool((dy[:, PMEAN][big] > 0).any()) and bool((dy[:, PMEAN][big] < 0).any())
    if c.mode == L.DST_POOL:             # non-argmax elements among them: -(P u + Q) only
        arg = dec[1]
        isarg = torch.zeros(c.B, c.H // 2, c.W // 2, 4, c.C, dtype=torch.bool).scatter_(3, arg, True)
        nonarg = ~isarg
        full = SC._win(dy.view(c.B, c.H, c.W, c.C), c.B, c.H, c.W)
        assert int((full[..., PMEAN].abs()[nonarg[..., PMEAN]] > ABOVE * F16_MAX).sum()) > c.M // 4
    assert _others_max(dy, [(p, PMEAN) for p in range(c.M)]) < 0.5 * F16_MAX


@pytest.mark.parametrize("vname", SC.NONARG_VARIANTS)
def test_nonarg_case(vname):
    c = SC.build(vname, "c64", kind="nonarg")
    dec = SC.decisions(c)
    pos, arg = dec
    assert bool((arg[..., PMEAN] == 0).all())                    # element 0 of every window is pooled; j is element 2
    j = c.nonarg_p
    kap = SC.kappa_channel(c, dec, j)
    for factor, lo, hi in ((BELOW, 0.95, 0.99), (ABOVE, 1.01, 1.05)):
        G = SC.g0(kap, factor)
        assert SC.f16(G) == G and 0 < G <= F16_MAX
        gq, g2q = SC.with_g(c, channel_g=G)
        dy = SC.reference(c, gq, g2q, dec)[0] * S
        assert lo * F16_MAX < abs(float(dy[j, PMEAN])) < hi * F16_MAX
        assert _others_max(dy, [(j, PMEAN)]) < 0.5 * F16_MAX
