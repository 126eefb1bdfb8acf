"""Every kernel instance mcamd_conv_wgrad can launch, against an EXACT reference.

x and dy hold small integers, which fp16 represents exactly.  Every product is an integer, and while
max|x| * max|dy| * (pixels enumerated, halo included) < 2^24 every partial sum, in every summation order, is an integer
that fp32 represents exactly: MFMA accumulation, the sum over the waves, the slab reduction and the scaling by
1 / grad_scale (a power of two) are all exact.  The reference is the same sum in float64 on the CPU, times the mask,
divided by grad_scale, and the result must EQUAL it: a kernel that drops the last pixels of a split, reads a tap one
pixel off at a border or counts a halo pixel twice is off by at least one integer unit.

tests/wgrad_cases.py holds the cases; test_host_cpu.py proves (without a GPU) that they reach every instance the plan
rules can name.  Channels outside the x and dy slices hold NaN, dw starts as NaN (a sentinel with a row map) and the
split-K workspace starts as NaN, so a leak from a neighbour's channels, an unwritten element and a slab element that is
summed without having been written all show."""
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
import wgrad_cases as WC  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0.3            # no multiple of 2^-8: never a value the kernels can produce from integer operands
DRAWS = {2: (-2, -1, 0, 1, 1, 2), 3: (-3, -2, -1, 0, 1, 1, 2, 3)}     # uneven, so that errors do not cancel


def _draw(gen, values, shape):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=gen)]


def _fill(dev, c, t, ld, choff, width, pad):
    """[B][C][H][W] (cpu, fp16-exact values) -> padded NHWC fp16 device buffer of `ld` channels with the tensor at channel
    `choff`; the slice [choff, choff + width) is zero beyond the tensor and around the image, every other channel is NaN."""
    buf = ops.alloc_padded(c.B, c.H, c.W, ld, dev, pad=pad)
    npix = c.B * (c.H + 1) * (c.W + 1) + c.W + 2 if pad else c.B * (c.H + 2) * (c.W + 2)
    flat = buf[:npix * ld].view(npix, ld)
    flat[:, :choff] = float("nan")
    flat[:, choff + width:] = float("nan")
    C_ = t.shape[1]
    ops.padded_view(buf, c.B, c.H, c.W, ld, pad)[:, 1:-1, 1:-1, choff:choff + C_] = t.permute(0, 2, 3, 1).to(dev).half()
    return buf


def _reference(x, dy, k):
    """sum over pixels of dy[b, n, h, w] * x[b, c, h + ty - 1, w + tx - 1] in float64: [cout][cin][k][k]."""
    B, cin, H, W = x.shape
    dy2 = dy.double().permute(1, 0, 2, 3).reshape(dy.shape[1], -1)
    r = (k - 1) // 2
    xp = torch.nn.functional.pad(x.double(), (r, r, r, r))
    ref = torch.empty(dy.shape[1], cin, k, k, dtype=torch.float64)
    for ty in range(k):
        for tx in range(k):
            xs = xp[:, :, ty:ty + H, tx:tx + W].permute(1, 0, 2, 3).reshape(cin, -1)
            ref[:, :, ty, tx] = dy2 @ xs.t()
    return ref


def _operands(c, gaussian=False):
    gen = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    if gaussian:
        x = torch.randn(c.B, c.cin, c.H, c.W, generator=gen)
        dy = torch.randn(c.B, c.cout, c.H, c.W, generator=gen)
    else:
        x = _draw(gen, (0, 1, 1, 2) if c.stem else DRAWS[c.vmax], (c.B, c.cin, c.H, c.W))
        dy = _draw(gen, DRAWS[c.vmax], (c.B, c.cout, c.H, c.W))
    n_rows = c.cout_full or c.cout
    rows = torch.randperm(n_rows, generator=gen)[:c.cout] if c.cout_full else None
    cols = torch.randperm(c.cin, generator=gen) if c.perm_cols else None
    mask = None
    if c.mask:
        mask = (torch.rand(n_rows, c.cin, c.k, c.k, generator=gen) > 0.3).float()      # scattered weights ...
        mask[torch.randperm(n_rows, generator=gen)[:max(1, n_rows // 8)]] = 0.0          # ... and whole filters removed
    return x, dy, rows, cols, mask


def _launch(dev, c, p, x, dy, rows, cols, mask):
    g = WC.geom_of(c)
    cin_tap = 4 if c.stem else ops.round_up(c.cin, 32)
    dy_ld = c.dy_ld or p.rows_pad
    xb = _fill(dev, c, x, g.x_ld, c.x_choff, cin_tap, c.pad)
    dyb = _fill(dev, c, dy, dy_ld, c.dy_choff, c.cout, c.pad)
    n_rows = c.cout_full or c.cout
    dw = torch.full((n_rows, c.cin, c.k, c.k), SENTINEL if c.cout_full else float("nan"), device=dev)
    db = torch.full((c.cout,), float("nan"), device=dev) if c.dbias else None
    ws = torch.full((ops.wgrad_workspace_bytes(g) // 4,), float("nan"), device=dev).view(torch.uint8)
    ops.conv_wgrad(g, xb, dyb, dy_ld, c.dy_choff, dw, mask.to(dev) if mask is not None else None, grad_scale=c.grad_scale,
                   dbias=db, workspace=ws, rows=rows.to(dev, torch.int32) if rows is not None else None,
                   cols=cols.to(dev, torch.int32) if cols is not None else None)
    torch.cuda.synchronize()
    return dw.cpu(), db.cpu() if db is not None else None


def _check_plan(c, setenv):
    """The query must still name the instance and the boundary conditions the case was written for."""
    WC.apply_env(c, setenv)
    p = WC.plan_of(c)
    assert (WC.compute_of(p), WC.finish_of(p, c.k, c.stem)) == c.expect, (c.name, p)
    assert set(c.tags) <= WC.boundary_tags(c, p), (c.name, p)
    return p


@pytest.mark.parametrize("c", WC.WGRAD_CASES, ids=str)
def test_wgrad_instance_exact(dev, c, setenv):
    p = _check_plan(c, setenv)
    x, dy, rows, cols, mask = _operands(c)
    # the condition of exactness, on this case's own inputs
    bound = float(x.abs().max()) * float(dy.abs().max()) * WC.pixels_enumerated(c)
    assert bound < 2 ** 24, (c.name, bound)
    ref = _reference(x, dy, c.k)                         # physical order [cout][cin][k][k]
    n_rows = c.cout_full or c.cout
    want = torch.full((n_rows, c.cin, c.k, c.k), SENTINEL if c.cout_full else float("nan"), dtype=torch.float64)
    r_idx = rows if rows is not None else torch.arange(c.cout)
    c_idx = cols if cols is not None else torch.arange(c.cin)
    scat = torch.empty(c.cout, c.cin, c.k, c.k, dtype=torch.float64)
    scat[:, c_idx] = ref                                 # dW[rows[n]][cols[ch]] receives the gradient of physical (n, ch)
    exact = scat * (mask[r_idx].double() if mask is not None else 1.0) / c.grad_scale
    want[r_idx] = exact
    want = want.float()
    assert bool((want[r_idx].double() == exact).all()), "the reference itself must be an fp32 number"

    dw, db = _launch(dev, c, p, x, dy, rows, cols, mask)

    bad = ~(dw == want)                                  # NaN compares unequal: an unwritten or polluted element is `bad`
    if bool(bad.any()):
        idx = bad.nonzero()
        units = ((dw.double() - want.double()) * c.grad_scale)[bad]
        raise AssertionError("%s: %d of %d elements of dw differ from the exact sum; first (row, cin, ky, kx) %s, got %r want %r; "
                             "difference in integer units: min %r max %r; rows touched %s"
                             % (c.name, int(bad.sum()), dw.numel(), idx[0].tolist(), float(dw[bad][0]), float(want[bad][0]),
                                float(units.min()), float(units.max()), sorted(set(idx[:, 0].tolist()))[:16]))
    if mask is not None:
        assert bool((dw[r_idx][mask[r_idx] == 0] == 0).all()), "masked weight gradients must be exactly zero"
    if c.cout_full:
        untouched = torch.ones(n_rows, dtype=torch.bool)
        untouched[rows] = False
        assert bool((dw[untouched] == SENTINEL).all()), "rows outside the row map must not be written"
    if c.dbias:
        want_db = (dy.double().sum((0, 2, 3)) / c.grad_scale).float()
        assert bool((db == want_db).all()), (c.name, "dbias", (db.double() - want_db.double()).abs().max())


@pytest.mark.parametrize("name", WC.DETERMINISM_CASES)
def test_wgrad_is_deterministic(dev, name, setenv):
    """include/mcamd.h: "Deterministic (slab reduction, no atomics)".  Gaussian operands (sums that DO depend on the order),
    several splits, two launches into fresh buffers: bit-equal."""
    c = next(c for c in WC.WGRAD_CASES if c.name == name)
    p = _check_plan(c, setenv)
    assert p.nsplit > 1
    x, dy, rows, cols, mask = _operands(c, gaussian=True)
    dw1, db1 = _launch(dev, c, p, x, dy, rows, cols, mask)
    dw2, db2 = _launch(dev, c, p, x, dy, rows, cols, mask)
    assert torch.equal(dw1.view(torch.int32), dw2.view(torch.int32))
    assert not bool(torch.isnan(dw1[rows] if rows is not None else dw1).any())
    if db1 is not None:
        assert torch.equal(db1.view(torch.int32), db2.view(torch.int32))
