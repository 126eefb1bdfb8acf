"""The list launch of the weight gradient (mcamd_conv_wgrad_bsparse), every case against an EXACT reference.

The method of tests/test_wgrad_instances_gpu.py: x and dy hold small integers, so every product and every partial sum in
every summation order is an integer below 2^24 that fp32 represents exactly, and the result must EQUAL the float64 sum times
the mask, divided by grad_scale.  tests/bsparse_wgrad_cases.py holds the cases and the masks; test_bsparse_wgrad_cases_cpu.py
proves without a GPU that they reach every instance the plan can name.  dw starts as NaN and the split-K workspace holds NaN
bit patterns: a skipped tile or tap that the finish pass reads, an element that nobody writes and a masked element that is
multiplied instead of selected all show.  Then, on random fp16 operands, bit-pattern equalities: the list launch against the
full-list launch at the same split count, the full-list launch against mcamd_conv_wgrad where the dense plan is the same
kernel, and the device-built lists against the numpy restatement."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops, _lib as L  # noqa: E402
import bsparse_wgrad_cases as BC  # noqa: E402
from test_wgrad_instances_gpu import _draw, _reference, DRAWS  # noqa: E402

pytestmark = pytest.mark.gpu


def _fill(dev, c, t, ld, choff, width):
    """[B][C][H][W] (cpu, fp16-exact) -> padded NHWC fp16 buffer of `ld` channels with the tensor at `choff`; channels
    outside [choff, choff + width) hold NaN, the halo of the slice is zero."""
    buf = ops.alloc_padded(c.B, c.H, c.W, ld, dev, pad=c.pad)
    npix = c.B * (c.H + 1) * (c.W + 1) + c.W + 2 if c.pad else c.B * (c.H + 2) * (c.W + 2)
    flat = buf[:npix * ld].view(npix, ld)
    flat[:, :choff] = float("nan")
    flat[:, choff + width:] = float("nan")
    ops.padded_view(buf, c.B, c.H, c.W, ld, c.pad)[:, 1:-1, 1:-1, choff:choff + t.shape[1]] = t.permute(0, 2, 3, 1).to(dev).half()
    return buf


def _operands(c, gaussian=False):
    gen = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    mask = BC.make_mask(c, gen)
    if gaussian:
        return torch.randn(c.B, c.cin, c.H, c.W, generator=gen), torch.randn(c.B, c.cout, c.H, c.W, generator=gen), mask
    return _draw(gen, DRAWS[3], (c.B, c.cin, c.H, c.W)), _draw(gen, DRAWS[3], (c.B, c.cout, c.H, c.W)), mask


class _Run:
    """The device operands of one case; launch() runs the list launch into fresh NaN buffers."""

    def __init__(self, dev, c, x, dy, mask):
        self.dev, self.c, self.g = dev, c, BC.geom_of(c)
        self.dy_ld = c.dy_ld or c.cout
        self.xb = _fill(dev, c, x, c.cin, 0, c.cin)
        self.dyb = _fill(dev, c, dy, self.dy_ld, c.dy_choff, c.cout)
        self.mask = mask.to(dev)
        self.tiles, self.words, self.counts = ops.wgrad_bsparse_lists(self.g, self.mask)
        torch.cuda.synchronize()
        self.ntiles = int(self.counts[0])

    def _buffers(self, nsplit):
        c = self.c
        dw = torch.full((c.cout, c.cin, c.k, c.k), float("nan"), device=self.dev)
        db = torch.full((c.cout,), float("nan"), device=self.dev) if c.dbias else None
        # NaN and Inf bit patterns: what an earlier layer's slabs may have left there
        ws = torch.full((nsplit * c.cout * c.cin * c.k * c.k,), float("nan"), device=self.dev)
        ws[1::3] = float("inf")
        return dw, db, ws.view(torch.uint8)

    def launch(self, nsplit, full=False):
        c = self.c
        dw, db, ws = self._buffers(nsplit)
        tiles, words, n = self.tiles, self.words, self.ntiles
        if full:
            tiles, words = ops.wgrad_bsparse_full_lists(self.g, self.dev)
            n = tiles.numel()
        ops.conv_wgrad_bsparse(self.g, self.xb, self.dyb, self.dy_ld, c.dy_choff, dw, self.mask, tiles, words, n, nsplit,
                               grad_scale=c.grad_scale, dbias=db, workspace=ws)
        torch.cuda.synchronize()
        return dw.cpu(), db.cpu() if db is not None else None

    def dense(self):
        c = self.c
        dw = torch.full((c.cout, c.cin, c.k, c.k), float("nan"), device=self.dev)
        db = torch.full((c.cout,), float("nan"), device=self.dev) if c.dbias else None
        ops.conv_wgrad(self.g, self.xb, self.dyb, self.dy_ld, c.dy_choff, dw, self.mask, grad_scale=c.grad_scale, dbias=db)
        torch.cuda.synchronize()
        return dw.cpu(), db.cpu() if db is not None else None


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("c", BC.WGRAD_BSPARSE_CASES, ids=str)
def test_list_launch_exact(dev, c, setenv):
    setenv("MCAMD_WGRAD9", "1")
    x, dy, mask = _operands(c)
    bound = float(x.abs().max()) * float(dy.abs().max()) * BC.pixels_enumerated(c)
    assert bound < 2 ** 24, (c.name, bound)
    run = _Run(dev, c, x, dy, mask)

    # the device-built lists are the numpy restatement's
    tiles, words, allw, (nt, npairs) = BC.lists_of(mask.numpy())
    n_all = len(allw)
    assert run.counts.cpu().tolist() == [nt, npairs], c.name
    assert run.tiles.cpu().numpy().tolist() == tiles.tolist() + [0] * (n_all - nt), c.name
    assert run.words.cpu().numpy().tolist() == words.tolist() + [0] * (n_all - nt) + allw.tolist(), c.name

    nsplit = BC.nsplit_of(c, nt)
    p = ops.conv_wgrad_bsparse_plan(run.g, nt)
    assert (BC.compute_of(p), (BC.VEC, c.k * c.k, BC.finish_sg(nsplit))) == c.expect, (c.name, p)
    want = (_reference(x, dy, c.k) * mask.double() / c.grad_scale).float()
    dw, db = run.launch(nsplit)
    bad = ~(dw == want)                                  # NaN compares unequal: an unwritten or polluted element is `bad`
    if bool(bad.any()):
        idx = bad.nonzero()
        units = ((dw.double() - want.double()) * c.grad_scale)[bad]
        raise AssertionError("%s: %d of %d elements of dw differ from the exact sum; first (row, cin, ky, kx) %s, got %r want %r; "
                             "difference in integer units: min %r max %r; (filter tile, channel tile, tap) touched %s"
                             % (c.name, int(bad.sum()), dw.numel(), idx[0].tolist(), float(dw[bad][0]), float(want[bad][0]),
                                float(units.min()), float(units.max()),
                                sorted({(int(i[0]) // 64, int(i[1]) // 64, int(i[2]) * c.k + int(i[3])) for i in idx[:4096]})[:12]))
    masked = dw[mask == 0]
    assert bool((masked.view(torch.int32) == 0).all()), "masked weight gradients must be exactly +0.0"
    if c.dbias:
        want_db = (dy.double().sum((0, 2, 3)) / c.grad_scale).float()
        assert bool((db == want_db).all()), (c.name, "dbias", (db.double() - want_db.double()).abs().max())


@pytest.mark.parametrize("c", [c for c in BC.WGRAD_BSPARSE_CASES if c.mask in ("random", "holes", "unaligned", "one-tap")], ids=str)
def test_list_launch_equals_full_list_launch(dev, c, setenv):
    """Random fp16 operands (sums that DO depend on the order): skipping changes no bit, at the same split count."""
    setenv("MCAMD_WGRAD9", "1")
    x, dy, mask = _operands(c, gaussian=True)
    run = _Run(dev, c, x, dy, mask)
    nsplit = BC.nsplit_of(c, run.ntiles)
    a, da = run.launch(nsplit)
    b, db = run.launch(nsplit, full=True)
    assert not bool(torch.isnan(a).any()) and not bool(torch.isnan(b).any())
    assert _same_bits(a, b), c.name
    assert bool((a[mask == 0].view(torch.int32) == 0).all())
    if da is not None:
        assert _same_bits(da, db)


@pytest.mark.parametrize("name", BC.DENSE_EQUAL)
def test_full_list_launch_equals_the_dense_entry(dev, name, setenv):
    """Where mcamd_conv_wgrad's plan is the narrow 9-tap kernel at the same pixels per step, the full-list launch at its
    split count runs the same staging, MFMA sequence, slab store and order of slab additions: the same bits."""
    for k_, v_ in (("MCAMD_WGRAD9", "1"), ("MCAMD_WGRAD9W", "1"), ("MCAMD_WGRAD9W_MINW", "40")):
        setenv(k_, v_)
    c = next(c for c in BC.WGRAD_BSPARSE_CASES if c.name == name)
    x, dy, mask = _operands(c, gaussian=True)
    run = _Run(dev, c, x, dy, mask)
    dense = ops.wgrad_plan_info(run.g)
    assert dense.family == L.WGRAD_NINE and dense.kp == c.expect[0][1], dense
    a, da = run.launch(dense.nsplit, full=True)
    b, db = run.dense()
    # Where the mask is zero the dense finish pass multiplies (sum * 0: +0.0 or -0.0 by the sign of the sum) and the list
    # launch selects the constant +0.0: the one place where the two entries differ by design, in the sign bit of a zero.
    kept = mask != 0
    assert int(kept.sum()) > 0 and int((~kept).sum()) > 0
    assert _same_bits(a[kept], b[kept]), (name, int((a[kept].view(torch.int32) != b[kept].view(torch.int32)).sum()))
    assert bool((a[~kept].view(torch.int32) == 0).all()) and bool((b[~kept] == 0).all())
    if da is not None:
        assert _same_bits(da, db)
    # ... and so does the launch on the short lists
    s, _ = run.launch(dense.nsplit)
    assert _same_bits(s[kept], b[kept]) and _same_bits(s, a), name


def test_refusals(dev, setenv):
    setenv("MCAMD_WGRAD9", "1")
    c = BC.WGRAD_BSPARSE_CASES[0]
    x, dy, mask = _operands(c)
    run = _Run(dev, c, x, dy, mask)
    dw, db, ws = run._buffers(1)
    for nsplit in (0, 10 ** 6):
        with pytest.raises(L.McamdError, match="nsplit"):
            ops.conv_wgrad_bsparse(run.g, run.xb, run.dyb, run.dy_ld, c.dy_choff, dw, run.mask, run.tiles, run.words, run.ntiles,
                                   nsplit, workspace=ws)
    with pytest.raises(L.McamdError, match="workspace"):
        ops.conv_wgrad_bsparse(run.g, run.xb, run.dyb, run.dy_ld, c.dy_choff, dw, run.mask, run.tiles, run.words, run.ntiles, 2,
                               workspace=ws)
    with pytest.raises(L.McamdError, match="tiles"):
        ops.conv_wgrad_bsparse(run.g, run.xb, run.dyb, run.dy_ld, c.dy_choff, dw, run.mask, run.tiles, run.words, 5, 1, workspace=ws)
