"""mcamd_conv_fwd_q4_mx_a4 / mcamd_conv_fwd_q8_w4_mx_a4 (csrc/conv_epi.h store_pad_tile_a4): the conv epilogue
writes MXFP4 codes and scale words, through ops, on all three tiles and both partial N tiles.

  1. integer-exact operands: the whole destination equals float64 conv -> affine + leaky -> e4m3(2 v) -> pool / reorg -> a4_ref's
     cast where the call writes, and the sentinel it was filled with everywhere else (halo rows, channels outside the slice);
  2. Gaussian operands: codes and scale words, interior and halo, equal the existing kernel into an e4m3 buffer + ops.cast_a4_mx;
  3. what the header refuses raises; both *_a4 pointers NULL is the existing entry point bit for bit.

M = 150 (PLAIN) / 180 (POOL, REORG): a partial second pixel tile, pooled rows over two tiles.  Helpers: test_q4_mx_kernels_gpu's."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
import a4_ref as A  # noqa: E402
import q8_cases as QC  # noqa: E402
import w4_cases as WC  # noqa: E402
import test_q8_instances_gpu as T  # noqa: E402  (helpers only)
import test_q8_w4_mx_kernels_gpu as MX  # noqa: E402  (helpers only: _pack)
import test_q4_mx_kernels_gpu as Q4  # noqa: E402  (helpers only: _case, _operands)

pytestmark = pytest.mark.gpu
FILL = 0xAB
ENTRIES = ("q4_mx", "q8_w4_mx")


def _case(k, cin, dst, cout, **kw):
    B, HW = (6, 5) if dst == "plain" else (5, 6)
    return Q4._case("%dx%d-%s-n%d" % (k, k, dst, cout), B, HW, HW, k, cin, cout, dst=dst, fmt="f8", draw="d1", **kw)


# (case, format of y, format of y2, channels of y's destination or 0 = its own, choff)
CASES = [(_case(k, cin, dst, n), "a4", "a4", 0, 0) for k, cin in ((3, 64), (1, 128)) for dst in ("plain", "pool+y2", "reorg")
         for n in (64, 128, 192, 256, 320)]
CASES += [(_case(3, 64, "plain", 128), "a4", "a4", 192, 64),       # a slice of a wider destination
          (_case(1, 128, "pool+y2", 192), "a4", "f8", 0, 0), (_case(1, 128, "pool+y2", 192), "f8", "a4", 0, 0)]
IDS = ["%s-%s+%s%s" % (c.name, fy, fy2, "-choff%d" % off if off else "") for c, fy, fy2, _, off in CASES]


def _halo_pair(rows, ch, dev, fill):
    """an MXFP4 destination of `rows` x `ch`: filled with `fill`, or (None) with the halo's contents"""
    nc, ns = ops.a4_mx_elems(rows, ch)
    if fill is not None:
        return torch.full((nc,), fill, dtype=torch.uint8, device=dev), torch.full((ns,), fill, dtype=torch.uint8, device=dev)
    return torch.zeros(nc, dtype=torch.uint8, device=dev), torch.tensor([127, 127, 0, 0], dtype=torch.uint8, device=dev).repeat(ns // 4)


def _launch(dev, entry, c, o, packed, fy, fy2, ch=0, choff=0, fill=None, fused=True):
    """One launch of `entry`'s *_a4 op (fused = False: of the existing op, every destination e4m3).  Returns name -> the
    destination on the CPU: (codes, scale bytes) of an MXFP4 one, the padded byte buffer of an e4m3 one."""
    g = QC.geom_of(c)
    x = T._input(dev, c, o)
    ins = ops.cast_a4_mx(x, c.B * (c.H + 2) * (c.W + 2), c.ld or c.cin, c.choff, c.cin) if entry == "q4_mx" else (x,)
    Ho, Wo = (c.H, c.W) if c.dst == "plain" else (c.H // 2, c.W // 2)
    ch = ch or c.cdst
    dsts, kw = {}, {}
    for name, fmt, rows, chn, off in (("y", fy, c.B * (Ho + 2) * (Wo + 2), ch, choff), ("y2", fy2, c.B * (c.H + 2) * (c.W + 2), c.cout, 0)):
        if name == "y2" and c.dst != "pool+y2":
            continue
        if fmt == "a4" and fused:
            dsts[name] = _halo_pair(rows, chn, dev, fill)
            kw[name + "_a4"] = (*dsts[name], chn, off)
        else:
            dsts[name] = (torch.zeros(rows * chn, dtype=torch.uint8, device=dev),)
            kw.update({name: dsts[name][0], name + "_ld": chn, name + "_choff": off, name + "_f8": True})
    fn = getattr(ops, "conv_fwd_%s%s" % (entry, "_a4" if fused else ""))
    fn(g, *ins, *packed, scale=T._dev(o.scale, dev), shift=T._dev(o.shift, dev), slope=c.slope, dst_mode=QC.DSTS[c.dst], **kw)
    torch.cuda.synchronize()
    return {name: tuple(t.cpu() for t in d) for name, d in dsts.items()}


def _padded_rows(b, ch, choff):
    """NCHW bytes -> the destination's padded rows [B (H + 2) (W + 2)][ch], zero outside the slice, and the mask of what is written"""
    B, C, H, W = b.shape
    full = torch.zeros(B, H + 2, W + 2, ch, dtype=torch.uint8)
    wr = torch.zeros(B, H + 2, W + 2, ch, dtype=torch.bool)
    full[:, 1:-1, 1:-1, choff:choff + C] = b.permute(0, 2, 3, 1)
    wr[:, 1:-1, 1:-1, choff:choff + C] = True
    return full.view(-1, ch), wr.view(-1, ch)


def _want(b, fmt, ch, choff, fill):
    """what a destination of NCHW bytes `b` must hold: a4_ref's cast in mcamd.h's layout (`fill` where nothing is written)"""
    rows, wr = _padded_rows(b, ch, choff)
    if fmt != "a4":
        return (rows.flatten(),)
    codes, scales = A.packed(*A.cast(rows)[:2])
    if fill is not None:
        codes[~wr[:, 0::2]] = fill
        scales[~wr[:, 0::16]] = fill
    return codes.flatten(), scales.flatten()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("c, fy, fy2, ch, choff", CASES, ids=IDS)
def test_exact_and_nothing_else_written(dev, entry, c, fy, fy2, ch, choff):
    o = Q4._operands(c)
    ref, _ = WC.reference(c, o)
    assert QC.exactness(c, o, ref) == [], c.name             # on the reference's operands, never from kernel output
    got = _launch(dev, entry, c, o, MX._pack(dev, c, o), fy, fy2, ch, choff, fill=FILL)
    for name, b, fmt, chn, off in (("y", ref.y, fy, ch or c.cdst, choff), ("y2", ref.y2, fy2, c.cout, 0)):
        if b is not None:
            for what, g, w in zip(("codes", "scale words"), got[name], _want(b, fmt, chn, off, FILL)):
                assert torch.equal(g, w), "%s %s %s: %d bytes differ" % (c.name, name, what, int((g != w).sum()))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("c, fy, fy2, ch, choff", CASES, ids=IDS)
def test_bit_equal_to_the_unfused_path(dev, entry, c, fy, fy2, ch, choff):
    o = Q4._operands(c, gaussian=True)
    packed = MX._pack(dev, c, o)
    got = _launch(dev, entry, c, o, packed, fy, fy2, ch, choff)
    base = _launch(dev, entry, c, o, packed, fy, fy2, ch, choff, fused=False)
    for name, fmt, chn in (("y", fy, ch or c.cdst), ("y2", fy2, c.cout)):
        if name in got:
            want = base[name]
            if fmt == "a4":
                want = tuple(t.cpu() for t in ops.cast_a4_mx(want[0].to(dev), want[0].numel() // chn, chn, 0, chn))
            assert all(torch.equal(g, w) for g, w in zip(got[name], want)), (c.name, name)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("what", ["cout 96", "choff 32", "misaligned scales"])
def test_validation(dev, entry, what):
    c = _case(1, 128, "plain", 96 if what == "cout 96" else 64)
    o = Q4._operands(c)
    ch = 192
    codes, scales = _halo_pair(c.B * (c.H + 2) * (c.W + 2) + 1, ch, dev, None)
    dst = (codes, scales[1:] if what == "misaligned scales" else scales, ch, 32 if what == "choff 32" else 64)
    x = T._input(dev, c, o)
    ins = ops.cast_a4_mx(x, c.B * (c.H + 2) * (c.W + 2), c.cin, 0, c.cin) if entry == "q4_mx" else (x,)
    with pytest.raises(McamdError):
        getattr(ops, "conv_fwd_%s_a4" % entry)(QC.geom_of(c), *ins, *MX._pack(dev, c, o), y_a4=dst)


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_destinations_are_the_existing_entry_point(dev, entry):
    c = _case(3, 64, "pool+y2", 192)
    o = Q4._operands(c, gaussian=True)
    packed = MX._pack(dev, c, o)
    a, b = _launch(dev, entry, c, o, packed, "f8", "f8"), _launch(dev, entry, c, o, packed, "f8", "f8", fused=False)
    assert all(torch.equal(a[n][0], b[n][0]) for n in ("y", "y2"))
