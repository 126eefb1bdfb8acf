"""Every raw-epilogue bsparse_kernel instance that mcamd_conv_fwd_bsparse_raw and mcamd_conv_dgrad_bsparse can launch, and
mcamd_bsparse_lists_dgrad (csrc/conv_bsparse.hip, the training form behind Darknet.sparse_train = "block"), against an
EXACT reference, with the method of test_bsparse_instances_gpu.py and test_conv_instances_gpu.py.

The operands hold small integers, so every partial sum in every order is an integer that fp32 holds and the stored fp16
values are exact (conv_cases.exactness, asserted per case).  The reference is float64 F.conv2d / F.conv_transpose2d with
w * mask.  The launch on the device's lists AND the launch on full lists must each EQUAL it as fp16 bit patterns in
NaN-filled buffers -- forward: y and the statistics slab (every row written; the float64 sum of the rows is the sum over
all pixels: conv_cases.reference's convention for "fwd-raw16-stats"); dgrad: gin inside its slice, everything outside it
still NaN.  The lists must equal bsparse_ref.chunk_lists on the numpy packing of the direction.  No tolerance in this
file.  tests/bsparse_train_cases.py holds the cases; test_bsparse_train_cases_cpu.py proves their coverage."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops, _lib as L  # noqa: E402
import bsparse_train_cases as TC  # noqa: E402
from util import NAN, fill_padded  # noqa: E402

pytestmark = pytest.mark.gpu


def _check_info(c, setenv):
    TC.apply_env(c, setenv)
    r = TC.info_of(c)
    assert (r.bm, r.bk, r.stages) == c.expect, (c.name, r)
    return r


def _pack(dev, c, o):
    wp, wd = ops.pack_weights(TC.geom_of(c), o.w.to(dev).contiguous(), o.mask.to(dev).contiguous(), c.fwd, c.dgrad)
    return wp if c.fwd else wd


def _lists(c, wp):
    return (ops.bsparse_lists_dgrad if c.dgrad else ops.bsparse_lists)(TC.geom_of(c), wp)


def _launch(dev, c, r, act, wp, count, lst, all_chunks=False):
    """One launch into NaN-filled outputs: (y [B][n][H][W], everything of y outside the slice, slab or None, overflow flag)."""
    g = TC.geom_of(c)
    in_ld = c.ld or c.kpad
    ab = fill_padded(dev, c, act, in_ld, c.choff, c.kpad, c.pad)
    y_ld = c.y_ld or c.n
    y = torch.full((c.M * y_ld,), NAN, dtype=torch.float16, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    stats = None
    if c.dgrad:
        ops.conv_dgrad_bsparse(g, ab, in_ld, c.choff, wp, count, lst, y, y_ld, c.y_choff, overflow=flag, all_chunks=all_chunks)
    else:
        if c.stats:
            stats = torch.full((r.mtiles, 2, ops.round_up(c.n, 256)), NAN, dtype=torch.float32, device=dev)
        ops.conv_fwd_bsparse_raw(g, ab, wp, count, lst, y, y_ld, c.y_choff, stats=stats, all_chunks=all_chunks, overflow=flag)
    torch.cuda.synchronize()
    v = y.view(c.B, c.H, c.W, y_ld)
    rest = torch.cat([v[..., :c.y_choff].reshape(-1), v[..., c.y_choff + c.n:].reshape(-1)])
    return v[..., c.y_choff:c.y_choff + c.n].permute(0, 3, 1, 2).cpu(), rest.cpu(), (stats.cpu() if stats is not None else None), int(flag.item())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_equal(c, r, what, got, want):
    assert got.dtype == torch.float16 and got.shape == want.shape, (c.name, what, got.dtype, got.shape, want.shape)
    assert bool((want.half().double() == want).all()), "the reference holds values that are no fp16 numbers"
    bad = _bits(got) != _bits(want.half())
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    first = tuple(idx[0].tolist())
    raise AssertionError("%s (bsparse_kernel<%d, %d, %d, RAW_F16>): %d of %d elements of %s differ from the exact result; first (image, "
                         "channel, y, x) %s, got %r want %r; %d NaN among them; channel tiles touched %s"
                         % (c.name, r.bm, r.bk, r.stages, int(bad.sum()), bad.numel(), what, list(first), float(got[first]),
                            float(want[first]), int((torch.isnan(got) & bad).sum()), sorted(set((idx[:, 1] // r.bn).tolist()))[:16]))


def _check(c, r, ref, res, how):
    got, rest, stats, _ = res
    _assert_equal(c, r, "y (%s)" % how, got, ref.y)
    assert bool(torch.isnan(rest).all()), "%s: %d elements outside the slice were written (%s)" % (c.name, int((~torch.isnan(rest)).sum()), how)
    if c.stats:
        s1, s2 = TC.stats_reference(ref)
        assert not bool(torch.isnan(stats[:, :, :c.n]).any()), "%s: slab rows %s hold NaN (%s)" % (
            c.name, torch.isnan(stats[:, :, :c.n]).any(2).any(1).nonzero().flatten().tolist()[:16], how)
        s = stats.double().sum(0)[:, :c.n]        # every per-row partial is an exact integer
        for which, want in ((0, s1), (1, s2)):
            bad = ~(s[which] == want)
            assert not bool(bad.any()), "%s (%s): statistics %s of %d channels differ; first channel %d got %r want %r" % (
                c.name, how, ("sum y", "sum y^2")[which], int(bad.sum()), int(bad.nonzero()[0]), float(s[which][bad][0]), float(want[bad][0]))
    else:
        assert stats is None


@pytest.mark.parametrize("c", TC.TRAIN_CASES, ids=str)
def test_bsparse_train_instance_exact(dev, c, setenv):
    r = _check_info(c, setenv)
    o, ref = TC.operands_and_reference(c)
    assert TC.exactness(c, o, ref) == [], c.name
    packed, rc, rl = TC.lists_ref(c, o)
    wp = _pack(dev, c, o)
    got_bits = wp.cpu().numpy().view(np.uint16)[:packed.size].reshape(packed.shape)
    assert np.array_equal(got_bits, packed.view(np.uint16)), "%s: the device packing differs from its numpy restatement" % c.name

    count, lst = _lists(c, wp)
    assert count.dtype == torch.int32 and lst.dtype == torch.int32 and tuple(lst.shape) == rl.shape
    assert torch.equal(count.cpu(), torch.from_numpy(rc)), "%s: counts %s, want %s" % (c.name, count.cpu().tolist(), rc.tolist())
    assert torch.equal(lst.cpu(), torch.from_numpy(rl)), "%s: the lists differ in tiles %s" % (
        c.name, (lst.cpu() != torch.from_numpy(rl)).any(1).nonzero().flatten().tolist())

    res = _launch(dev, c, r, o.act, wp, count, lst)
    _check(c, r, ref, res, "lists")
    full = _launch(dev, c, r, o.act, wp, count, lst, all_chunks=True)
    _check(c, r, ref, full, "all chunks")
    if not c.overflow:
        assert res[3] == 0 and full[3] == 0, "nothing was clamped: the overflow flag must stay 0"
        return
    assert res[3] == 1 and full[3] == 1, "a value was clamped to +-65504: the overflow flag must be set"
    for (b, ch, h, x, sign) in o.planted:
        assert float(res[0][b, ch, h, x]) == sign * 65504.0
    o2, ref2 = TC.operands_and_reference(c, plant=False)
    assert TC.exactness(c, o2, ref2) == []
    res2 = _launch(dev, c, r, o2.act, wp, count, lst)
    _assert_equal(c, r, "y (nothing planted)", res2[0], ref2.y)
    assert res2[3] == 0, "nothing was clamped: the overflow flag must stay 0"


@pytest.mark.parametrize("form", TC.FORMS)
@pytest.mark.parametrize("inst", TC.INSTANCES, ids=lambda i: "bm%d-bk%d" % i[:2])
def test_bsparse_train_clamps_foreign_lists(dev, inst, form, setenv):
    """A count above the chunk count and indices outside [0, nchunks) are clamped into range: the launch stays inside its
    operands and computes what the clamped list says -- here every chunk once, the exact result of the full lists."""
    c = TC.foreign_case(form, inst)
    r = _check_info(c, setenv)
    o, ref = TC.operands_and_reference(c)
    assert TC.exactness(c, o, ref) == []
    assert TC.lists_ref(c, o)[1].tolist() == [c.nchunks]
    wp = _pack(dev, c, o)
    foreign = list(range(c.nchunks))
    foreign[0], foreign[-1] = -7, c.nchunks - 1 + 10 ** 6          # clamped to 0 and to nchunks - 1
    count = torch.tensor([10 ** 6], dtype=torch.int32, device=dev)
    lst = torch.tensor([foreign], dtype=torch.int32, device=dev)
    res = _launch(dev, c, r, o.act, wp, count, lst)
    _check(c, r, ref, res, "foreign list")
    assert res[3] == 0


@pytest.mark.parametrize("inst", TC.INSTANCES, ids=lambda i: "bm%d-bk%d" % i[:2])
def test_bsparse_raw_statistics_are_of_the_stored_values(dev, inst, setenv):
    """A forward with statistics that clamps two elements: the slab sums the values AS STORED (+-65504 there), the
    convention of mcamd_conv_fwd for this epilogue, not the accumulators -- exactly, on the lists and on full lists."""
    c = TC.stats_saturate_case(inst)
    r = _check_info(c, setenv)
    o, ref = TC.operands_and_reference(c)
    assert TC.stats_saturate_exactness(c, o, ref) == []
    wp = _pack(dev, c, o)
    count, lst = _lists(c, wp)
    for how, kw in (("lists", {}), ("all chunks", dict(all_chunks=True))):
        res = _launch(dev, c, r, o.act, wp, count, lst, **kw)
        _check(c, r, ref, res, how)
        assert res[3] == 1, "a value was clamped to +-65504: the overflow flag must be set"


def test_bsparse_raw_refuses_other_epilogues(dev, setenv):
    """epi.mode must be MCAMD_EPI_RAW_F16: anything else is MCAMD_EINVAL, and nothing is launched."""
    import ctypes as C
    c = TC.foreign_case("fwd", TC.INSTANCES[0])
    TC.apply_env(c, setenv)
    o, _ = TC.operands_and_reference(c)
    wp = _pack(dev, c, o)
    count, lst = _lists(c, wp)
    g = TC.geom_of(c)
    ab = fill_padded(dev, c, o.act, c.kpad, 0, c.kpad, c.pad)
    y = ops.alloc_padded(c.B, c.H, c.W, c.n, dev)
    for mode in (L.EPI_PAD_F16, L.EPI_NCHW_F32, L.EPI_RAW_F32):
        e = ops._epi(mode, y, c.n, 0)
        rc = L.lib().mcamd_conv_fwd_bsparse_raw(C.byref(g), ops.ptr(ab), ops.ptr(wp), ops.ptr(count), ops.ptr(lst), C.byref(e), ops.stream_ptr())
        assert rc == -1, mode          # MCAMD_EINVAL
