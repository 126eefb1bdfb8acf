"""Every bsparse_kernel instance mcamd_conv_fwd_bsparse can launch and bsparse_lists_kernel (csrc/conv_bsparse.hip, the
zero-chunk-skipping forward behind Darknet.sparse = "block"), against an EXACT reference, with the method of
test_conv_instances_gpu.py and test_sparse_instances_gpu.py.

The operands hold small integers; while max|x| * max|w| * (taps * channels) is below 2^24 every partial sum in every order is
an integer that fp32 holds, and the epilogue (scales 1/4 .. 2, shifts in steps of 1/4, slope 1/8) is exact as long as the
result is an fp16 number.  The reference is float64 F.conv2d of x with w * mask, the epilogue, then max_pool2d / reorg.  The
launch on the device's lists AND the launch on full lists must each EQUAL it as fp16 bit patterns -- two comparisons with
the reference, not one through the other -- in both `pad` forms of x: a list entry skipped, repeated or read one place off,
a chunk staged from the wrong (channel block, tap), a wrong border pixel of the shared-halo form or a wrong row of a tile
that spans two images is off by at least one unit (test_bsparse_cases_cpu.py proves that every listed chunk is visible in
every tile).  The lists themselves must equal bsparse_ref.chunk_lists.  There is no tolerance in this file.

tests/bsparse_cases.py holds the cases; test_bsparse_cases_cpu.py proves without a GPU that they reach every instance with
every destination form, `pad` form, boundary condition, list length around the ring's depth and mask kind.  Channels
outside the operand slice hold NaN, the halo holds zero; every output starts as NaN everywhere, halo and guard bands
included, and must stay so outside the interior of its slice."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
import bsparse_cases as BC  # noqa: E402
from util import NAN, whole, fill_padded, padded_split, is_sentinel  # noqa: E402

pytestmark = pytest.mark.gpu


def _check_info(c, setenv):
    """The query must still name the instance and the boundary conditions the case was written for."""
    BC.apply_env(c, setenv)
    r = BC.info_of(c)
    assert (r.bm, r.bk, r.stages) == c.expect, (c.name, r)
    assert set(c.tags) <= BC.boundary_tags(c, r), (c.name, r, BC.boundary_tags(c, r))
    return r


def _pack(dev, c, o):
    return ops.pack_weights(BC.geom_of(c), o.w.to(dev).contiguous(), o.mask.to(dev).contiguous(), True, False)[0]


def _launch(dev, c, act, wp, count, lst, scale, shift, dst=None, all_chunks=False):
    """One launch into NaN-filled outputs.  Returns {name: (got NCHW, everything outside the slice)} and the overflow flag."""
    dst = dst or c.dst
    xb = fill_padded(dev, c, act, c.ld or c.cin, c.choff, c.cin, c.pad)
    Ho, Wo = (c.H, c.W) if dst == "plain" else (c.H // 2, c.W // 2)
    y_ld = c.y_ld or c.cdst
    y = ops.alloc_padded(c.B, Ho, Wo, y_ld, dev)
    whole(y).fill_(NAN)
    y2, y2_ld, y2_choff = None, 0, 0
    if dst == "pool+y2":
        y2_ld, y2_choff = c.y2_slice
        y2 = ops.alloc_padded(c.B, c.H, c.W, y2_ld, dev)
        whole(y2).fill_(NAN)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.conv_fwd_bsparse(BC.geom_of(c), xb, wp, count, lst, y, y_ld, c.y_choff, scale.to(dev), shift.to(dev), BC.SLOPE,
                         dst_mode=BC.DSTS[dst], y2=y2, y2_ld=y2_ld, y2_choff=y2_choff, all_chunks=all_chunks, overflow=flag)
    torch.cuda.synchronize()
    out = {"y": padded_split(y, c.B, Ho, Wo, y_ld, c.y_choff, c.cdst)}
    if y2 is not None:
        out["y2"] = padded_split(y2, c.B, c.H, c.W, y2_ld, y2_choff, c.cout)
    return out, int(flag.item())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_equal(c, r, what, got, want):
    """got fp16, want float64 [B][n][h][w]: the fp16 bit patterns must be the reference's (NaN, an unwritten or polluted
    element, compares unequal)."""
    assert got.dtype == torch.float16 and got.shape == want.shape, (c.name, what, got.dtype, got.shape, want.shape)
    assert bool((want.half().double() == want).all()), "the reference holds values that are no fp16 numbers"
    bad = _bits(got) != _bits(want.half())
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    first = tuple(idx[0].tolist())
    raise AssertionError("%s (bsparse_kernel<%d, %d, %d>): %d of %d elements of %s differ from the exact result; first (image, "
                         "channel, y, x) %s, got %r want %r; %d sentinels among them; channel tiles touched %s"
                         % (c.name, r.bm, r.bk, r.stages, int(bad.sum()), bad.numel(), what, list(first), float(got[first]),
                            float(want[first]), int((is_sentinel(got) & bad).sum()), sorted(set((idx[:, 1] % c.cout // r.bn).tolist()))[:16]))


def _assert_untouched(c, what, rest):
    keep = is_sentinel(rest)
    assert bool(keep.all()), "%s: %d elements of %s outside the slice were written" % (c.name, int((~keep).sum()), what)


def _check_outputs(c, r, ref, out, how):
    for name, want in (("y", ref.y), ("y2", ref.y2)):
        if want is None:
            continue
        got, rest = out[name]
        _assert_equal(c, r, "%s (%s)" % (name, how), got, want)
        _assert_untouched(c, "%s (%s)" % (name, how), rest)
    if c.dst == "pool+y2":
        assert torch.equal(_bits(out["y"][0]), _bits(F.max_pool2d(out["y2"][0].float(), 2, 2).half())), "y is not max_pool2d(y2), bit for bit"


@pytest.mark.parametrize("c", BC.BSPARSE_CASES, ids=str)
def test_bsparse_instance_exact(dev, c, setenv):
    r = _check_info(c, setenv)
    o, ref = BC.operands_and_reference(c)
    assert BC.exactness(c, o, ref) == [], c.name            # the conditions of exactness, on this case's own reference
    packed, rc, rl = BC.lists_ref(c, o)
    wp = _pack(dev, c, o)
    if c.mask == "negzero":
        # the premise of the case: the dropped blocks hold -0.0, sign bit and all
        got_bits = wp.cpu().numpy().view(np.uint16).reshape(packed.shape)
        assert np.array_equal(got_bits, packed.view(np.uint16)) and int((got_bits == 0x8000).sum()) >= c.ntiles * c.kb

    count, lst = ops.bsparse_lists(BC.geom_of(c), wp)
    assert count.dtype == torch.int32 and lst.dtype == torch.int32 and tuple(lst.shape) == rl.shape
    assert torch.equal(count.cpu(), torch.from_numpy(rc)), "%s: counts %s, want %s" % (c.name, count.cpu().tolist(), rc.tolist())
    assert torch.equal(lst.cpu(), torch.from_numpy(rl)), "%s: the lists differ in tiles %s" % (
        c.name, (lst.cpu() != torch.from_numpy(rl)).any(1).nonzero().flatten().tolist())

    out, flag = _launch(dev, c, o.act, wp, count, lst, o.scale, o.shift)
    _check_outputs(c, r, ref, out, "lists")
    full, flag_full = _launch(dev, c, o.act, wp, count, lst, o.scale, o.shift, all_chunks=True)
    _check_outputs(c, r, ref, full, "all chunks")
    if c.dst == "pool":
        # the same launch with the full-resolution copy: the pooled output does not depend on it
        out2, _ = _launch(dev, c, o.act, wp, count, lst, o.scale, o.shift, dst="pool+y2")
        assert torch.equal(_bits(out["y"][0]), _bits(out2["y"][0])), "pool and pool+y2 differ in y"
        _assert_untouched(c, "y (with y2)", out2["y"][1])
        _assert_untouched(c, "y2", out2["y2"][1])
    if not c.overflow:
        assert flag == 0 and flag_full == 0, "nothing was clamped: the overflow flag must stay 0"
        return
    assert flag == 1 and flag_full == 1, "a value was clamped to +-65504: the overflow flag must be set"
    got = out["y"][0]
    for (b, ch, h, x, sign) in o.planted:
        assert float(got[b, ch, h, x]) == sign * 65504.0
    o2, ref2 = BC.operands_and_reference(c, plant=False)
    assert BC.exactness(c, o2, ref2) == []
    out2, flag2 = _launch(dev, c, o2.act, wp, count, lst, o2.scale, o2.shift)
    _assert_equal(c, r, "y (nothing planted)", out2["y"][0], ref2.y)
    assert flag2 == 0, "nothing was clamped: the overflow flag must stay 0"


@pytest.mark.parametrize("inst", BC.INSTANCES, ids=lambda i: "bm%d-bk%d" % i[:2])
def test_bsparse_clamps_foreign_lists(dev, inst, setenv):
    """A count above the chunk count and indices outside [0, nchunks) are clamped into range: the launch stays inside its
    operands and computes what the clamped list says -- here every chunk once, the exact result of the full lists."""
    c = BC.foreign_case(inst)
    r = _check_info(c, setenv)
    o, ref = BC.operands_and_reference(c)
    assert BC.exactness(c, o, ref) == []
    _, rc, _ = BC.lists_ref(c, o)
    assert rc.tolist() == [c.nchunks]
    wp = _pack(dev, c, o)
    foreign = list(range(c.nchunks))
    foreign[0], foreign[-1] = -7, c.nchunks - 1 + 10 ** 6          # clamped to 0 and to nchunks - 1
    count = torch.tensor([10 ** 6], dtype=torch.int32, device=dev)
    lst = torch.tensor([foreign], dtype=torch.int32, device=dev)
    out, flag = _launch(dev, c, o.act, wp, count, lst, o.scale, o.shift)
    _check_outputs(c, r, ref, out, "foreign list")
    assert flag == 0


@pytest.mark.parametrize("name", BC.DETERMINISM_CASES)
def test_bsparse_is_deterministic(dev, name, setenv):
    """Gaussian operands (sums that DO depend on the order) and two launches into fresh buffers: bit-equal, and no sentinel
    left inside the slice."""
    c = next(c for c in BC.BSPARSE_CASES if c.name == name)
    _check_info(c, setenv)
    o = BC.operands(c, gaussian=True)
    wp = _pack(dev, c, o)
    count, lst = ops.bsparse_lists(BC.geom_of(c), wp)
    a, _ = _launch(dev, c, o.act, wp, count, lst, o.scale, o.shift)
    b, _ = _launch(dev, c, o.act, wp, count, lst, o.scale, o.shift)
    for what in a:
        assert not bool(is_sentinel(a[what][0]).any()), what
        assert torch.equal(_bits(a[what][0]), _bits(b[what][0])), what
        _assert_untouched(c, what, a[what][1])
