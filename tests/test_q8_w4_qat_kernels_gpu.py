"""mcamd_conv_fwd_q8_w4_raw and mcamd_fakequant_q8_w4 (csrc/conv_q8_w4.hip): every kernel instance of the training
forward of a 4-bit block, in both MFMA forms (MCAMD_Q8_MFMA 0 / 1).  There is no tolerance in this file:

  1. on Gaussian operands the kernel equals mcamd_conv_fwd_q8 in raw mode on mcamd_unpack_q8_w4's bytes with the same exponents,
     y and the statistics slab, bit for bit; the output slice and the slab are pre-filled with NaN: every slab row is written,
     nothing outside the y slice changes; with statistics off no slab is touched;
  2. on integer draws (with 5 and 7, which the grid cannot hold) y equals the float64 reference on w4_ref's bytes and the slab
     the exact sums (the conditions of exactness are asserted on the reference's operands, here and in test_q8_w4_qat_cpu.py);
  3. two launches are bit-equal;
  4. mcamd_fakequant_q8_w4 equals the restatement, adversarial filters and pad rows included, and deq(unpacked bytes) * 2^-e4_f.

The launch helpers and the raw checks are test_q8_instances_gpu.py's."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import ops  # noqa: E402
import q8_cases as QC  # noqa: E402
import q8_ref as R  # noqa: E402
import w4_cases as WC  # noqa: E402
import w4_ref as W  # noqa: E402
import w4_qat_cases as C4  # noqa: E402
import w4_qat_ref as Q4  # noqa: E402
import test_q8_instances_gpu as T  # noqa: E402  (helpers only: _check_info, _input, _launch, _check_raw, _dev)
from util import NAN  # noqa: E402

pytestmark = pytest.mark.gpu


def _pack(dev, c, o):
    return ops.pack_q8_w4(QC.geom_of(c), T._dev(o.w, dev), T._dev(o.mask, dev))


def _launch(dev, c, o, packed, xb=None):
    """T._launch's raw branch for mcamd_conv_fwd_q8_w4_raw: one launch into NaN-filled y and slab."""
    g = QC.geom_of(c)
    xb = T._input(dev, c, o) if xb is None else xb
    codes, gshift, wexp = packed
    y_ld = c.y_ld or c.cout
    y = torch.full((c.M, y_ld), NAN, device=dev)
    slab = torch.full((ops.conv_fwd_q8_stats_rows(g), 2, ops.round_up(c.cout, 256)), NAN, device=dev) if c.stats else None
    ops.conv_fwd_q8_w4_raw(g, xb, codes, gshift, wexp, y, y_ld, c.y_choff, stats=slab)
    torch.cuda.synchronize()
    return {"y": y.cpu(), "slab": slab.cpu() if slab is not None else None}


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. same bytes, same result
@pytest.mark.parametrize("c", C4.CASES, ids=str)
def test_w4_raw_equals_the_fp8_raw_kernel_on_the_expanded_bytes(dev, c, setenv):
    r = T._check_info(c, setenv)
    o = C4.operands(c, gaussian=True)
    g = QC.geom_of(c)
    packed = _pack(dev, c, o)
    wq = ops.unpack_q8_w4(g, packed[0], packed[1])
    xb = T._input(dev, c, o)
    a = _launch(dev, c, o, packed, xb=xb)
    b, _ = T._launch(dev, c, o, (wq, None, packed[2]), xb=xb)
    sl = slice(c.y_choff, c.y_choff + c.cout)
    assert not bool(torch.isnan(a["y"][:, sl]).any()) and bool((a["y"][:, sl] != 0).any())
    assert torch.equal(_bits(a["y"]), _bits(b["y"])), "%s: y differs from mcamd_conv_fwd_q8 (raw) on the same bytes in %d elements" % (
        c.name, int((_bits(a["y"]) != _bits(b["y"])).sum()))
    rest = a["y"].clone()
    rest[:, sl] = NAN
    T._assert_untouched(c, "y", rest)
    if not c.stats:
        assert a["slab"] is None and b["slab"] is None
        return
    assert a["slab"].shape[0] == r.mtiles
    nwritten = ops.round_up(c.cout, r.bmw)
    assert not bool(torch.isnan(a["slab"][:, :, :nwritten]).any()), "%s: a slab row was not written" % c.name
    assert bool(torch.isnan(a["slab"][:, :, nwritten:]).all()), "%s: slab columns beyond the last filter tile were written" % c.name
    assert torch.equal(_bits(a["slab"]), _bits(b["slab"])), "%s: the slab differs from mcamd_conv_fwd_q8 (raw) on the same bytes" % c.name


def test_w4_raw_without_statistics_touches_no_slab(dev, setenv):
    """epi->stats NULL: a slab that lies right behind y in the same allocation keeps its NaN fill."""
    c = next(c for c in C4.CASES if c.name == "r128-r-stats")._replace(stats=False)
    T._check_info(c._replace(tags=()), setenv)
    o = C4.operands(c, gaussian=True)
    g = QC.geom_of(c)
    y_ld = c.y_ld or c.cout
    rows, ld = ops.conv_fwd_q8_stats_rows(g), ops.round_up(c.cout, 256)
    buf = torch.full((c.M * y_ld + rows * 2 * ld,), NAN, device=dev)
    codes, gshift, wexp = _pack(dev, c, o)
    ops.conv_fwd_q8_w4_raw(g, T._input(dev, c, o), codes, gshift, wexp, buf[:c.M * y_ld].view(c.M, y_ld), y_ld, c.y_choff, stats=None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[c.M * y_ld:]).all()), "the launch without statistics wrote behind y"
    assert not bool(torch.isnan(buf[:c.M * y_ld].view(c.M, y_ld)[:, c.y_choff:c.y_choff + c.cout]).any())


# ------------------------------------------------------------------------------------------------ 2. exact against float64
@pytest.mark.parametrize("c", C4.CASES, ids=str)
def test_w4_raw_instance_exact(dev, c, setenv):
    r = T._check_info(c, setenv)
    o, ref, draw = C4.operands_and_reference(c)
    assert QC.exactness(c, o, ref) == [], c.name            # on the reference's operands, never from kernel output
    packed = _pack(dev, c, o)
    assert torch.equal(packed[2][:c.cout].cpu(), ref.e), "exponents"
    T._check_raw(c, r, o, ref, _launch(dev, c, o, packed))


# ------------------------------------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("name", C4.DETERMINISM_CASES)
def test_w4_raw_is_deterministic(dev, name, setenv):
    c = next(c for c in C4.CASES if c.name == name)
    T._check_info(c, setenv)
    o = C4.operands(c, gaussian=True)
    packed = _pack(dev, c, o)
    a, b = _launch(dev, c, o, packed), _launch(dev, c, o, packed)
    sl = slice(c.y_choff, c.y_choff + c.cout)
    assert not bool(torch.isnan(a["y"][:, sl]).any()) and torch.equal(a["y"][:, sl], b["y"][:, sl])
    assert not bool(torch.isnan(a["slab"][:, :, :c.cout]).any()) and torch.equal(a["slab"][:, :, :c.cout], b["slab"][:, :, :c.cout])


# ------------------------------------------------------------------------------------------------ 4. fake quantisation
def _sets():
    gen = torch.Generator().manual_seed(14)
    w1 = torch.randn(72, 64, 3, 3, generator=gen) * 0.04
    w2 = torch.randn(136, 128, 1, 1, generator=gen) * 0.1
    w3 = WC.adversarial(gen)
    m3 = (torch.rand(w3.shape, generator=gen) > 0.4).float()
    m3[7] = 0.0
    m3[9, 32:64] = 0.0
    return [("gauss-72x64x3", w1, None), ("gauss-136x128x1", w2, None), ("adversarial", w3, None), ("adversarial-masked", w3, m3)]


@pytest.mark.parametrize("name, w, mask", _sets(), ids=lambda v: v if isinstance(v, str) else "")
def test_fakequant_equals_the_restatement(dev, name, w, mask):
    cout, cin, k, _ = w.shape
    g = ops.geom(1, 8, 8, k, cin, cout, cin)
    npad, ktot = ops.round_up(cout, 256), cin * k * k
    codes, gshift, wexp = ops.pack_q8_w4(g, w.to(dev).contiguous(), mask.to(dev).contiguous() if mask is not None else None)
    # (the destination lies in front of a NaN guard: exactly cout * cin * k * k floats are written, no pad row reaches it)
    buf = torch.full((w.numel() + 4096,), NAN, device=dev)
    out = buf[:w.numel()].view(w.shape)
    ops.fakequant_q8_w4(g, codes, gshift, wexp, out)
    wq8 = ops.unpack_q8_w4(g, codes, gshift)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool(torch.isnan(buf[w.numel():]).all()), "written behind the OIHW tensor"
    want = Q4.fakequant(w, mask)
    bad = _bits(got) != _bits(want)
    assert not bool(bad.any()), "%s: %d of %d values differ from the restatement; first (o, i, h, w) %s got %r want %r" % (
        name, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), float(got[bad][0]), float(want[bad][0]))
    if mask is not None:
        assert bool((_bits(got)[mask == 0] == 0).all()), "a masked weight is not exactly +0"
    # ... and the values of the bytes the forward multiplies, in mcamd_pack_q8's layout, times 2^-e4_f
    rows = R.deq(wq8.cpu().view(npad, ktot)[:cout]).double() * torch.pow(2.0, -wexp[:cout].cpu().double()).view(-1, 1)
    assert torch.equal(W.dense_rows(got).double(), rows), "fakequant is not deq(unpacked bytes) * 2^-e4_f"
