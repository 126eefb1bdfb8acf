"""CPU checks of 4-bit quantisation-aware training (Darknet.precision = "fp8-w4-qat"): the restatement
(w4_qat_ref.py) against q8_qat_ref.py on w4_ref.py's bytes and against float64 autograd, the fp16 exactness of the dgrad operand,
the new entry points and their refusals, the precision's plumbing, and the cases of test_q8_w4_qat_kernels_gpu.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from modelcompression_amd import _lib as L, ops
import q8_cases as QC
import q8_ref as R
import q8_qat_ref as Q
import w4_cases as WC
import w4_ref as W
import w4_qat_cases as C4
import w4_qat_ref as Q4
from test_q8_qat_cpu import YOLO_FILTERS, _operands

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mcamd_conv_fwd_q8_w4_raw", "mcamd_fakequant_q8_w4")


# ------------------------------------------------------------------------------------------------ the restatement
def test_training_block_equals_q8_qat_ref_on_the_w4_bytes_code_for_code():
    """conv(x_q, w_q) on the values IS q8_qat_ref.train_block on w4_ref.quantise's bytes with e4: the same y (float64, exactly:
    the two differ by powers of two), hence the same coefficients and the same codes in every destination form -- and the same
    as the fp8 quantiser's block on the dequantised weights ("model B"), whose bytes are twice these with exponent e4 + 1."""
    for seed, (cin, cout, k, masked) in enumerate([(64, 72, 3, False), (128, 64, 1, True), (192, 128, 3, True)]):
        a8, w, mask, gamma, beta = _operands(seed, 2, cin, cout, k, 10, 12, masked)
        codes, g, e4, values, w8 = W.quantise(w, mask)
        y, scale, shift, v = Q4.train_block(a8, w, mask, gamma, beta)
        y8, scale8, shift8, v8 = Q.train_block(a8, w8, e4, gamma, beta)
        assert torch.equal(y, y8) and torch.equal(scale, scale8) and torch.equal(shift, shift8) and torch.equal(v, v8)
        for dst in ("plain", "pool", "reorg"):
            assert torch.equal(Q.store_pair(v, dst)[0], Q.store_pair(v8, dst)[0]), (seed, dst)
        wq = Q4.fakequant(w, mask)
        b8, e8 = R.quantise_weights(wq, None)
        live = wq.flatten(1).abs().amax(1) > 0
        assert torch.equal(e8[live], e4[live] + 1) and torch.equal(R.deq(b8).double(), 2.0 * values)
        assert torch.equal(Q.train_block(a8, b8, e8, gamma, beta)[0], y)


def test_fakequant_equals_w4_ref_dequantised():
    gen = torch.Generator().manual_seed(11)
    w = WC.adversarial(gen)
    mask = (torch.rand(w.shape, generator=gen) > 0.4).float()
    mask[7] = 0.0
    for m in (None, mask):
        codes, g, e4, values, w8 = W.quantise(w, m)
        wq = Q4.fakequant(w, m)
        assert torch.equal(wq, W.dequantised(values, e4))
        assert torch.equal(wq.double(), values * torch.pow(2.0, -e4.double()).view(-1, 1, 1, 1)), "the fp32 value is exact"
        assert torch.equal(wq, Q.w_q(w8, e4)), "... and what the bytes stand for"
        if m is not None:
            assert bool((wq[m == 0] == 0).all()) and bool((codes[m == 0] == 0).all()), "a masked weight has code 0 and value 0"
        assert bool((wq[3] == 0).all())                                   # the all-zero filter


def test_fp16_holds_w_q_exactly_on_he_initialised_yolov2_filters():
    """One mantissa bit: fp16(w_q) is w_q while it stays in fp16's normal range."""
    gen = torch.Generator().manual_seed(7)
    for cin, cout, k in YOLO_FILTERS:
        w = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
        wq = Q4.fakequant(w)
        assert torch.equal(wq.half().float(), wq), (cin, cout, k)
        nz = wq[wq != 0].abs()
        assert float(nz.min()) >= 2.0 ** -14 and float(nz.max()) < 65504.0


def test_straight_through_gradients_equal_float64_autograd_at_the_quantised_point():
    """W4QatConv's dX / dW are the gradients of the UNQUANTISED convolution evaluated at (x_q, w_q) (times the mask); a weight
    its group rounds to code 0 still receives its gradient."""
    for seed, (cin, cout, k, masked) in enumerate([(64, 24, 3, True), (64, 16, 1, False)]):
        gen = torch.Generator().manual_seed(60 + seed)
        x = F.leaky_relu(torch.randn(2, cin, 7, 9, generator=gen), 0.1).double().requires_grad_()
        w0 = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
        w0[1, :32] *= 2.0 ** -12                                          # a group far below its filter's scale: all codes 0
        w = w0.double().requires_grad_()
        mask = (torch.rand(cout, cin, k, k, generator=gen) < 0.5).double() if masked else None
        G = torch.randn(2, cout, 7, 9, generator=gen).double()
        out = Q4.W4QatConv.apply(x, w, mask)
        (out * G).sum().backward()
        xq = Q.x_q(R.q(2.0 * x.detach())).double().requires_grad_()
        wq = Q4.fakequant(w.detach().float(), mask.float() if masked else None).double().requires_grad_()
        ref = F.conv2d(xq, wq, None, 1, (k - 1) // 2)
        assert torch.equal(out.detach(), ref.detach())
        (ref * G).sum().backward()
        dw_ref = wq.grad * mask if masked else wq.grad
        assert float((x.grad - xq.grad).norm() / xq.grad.norm()) < 1e-12
        assert float((w.grad - dw_ref).norm() / dw_ref.norm()) < 1e-12
        if masked:
            assert bool((w.grad[mask == 0] == 0).all())
        zero = (wq.detach()[1, :32] == 0) & ((mask[1, :32] != 0) if masked else True)
        assert bool(zero.any()) and bool((w.grad[1, :32][zero] != 0).all()), "code 0 does not cut the gradient"


def test_forward_train_restatement_is_the_fp8_qat_one_on_the_dequantised_state():
    from oracle import darknet_ref as O
    blocks = O.parse_cfg(os.path.join(ROOT, "tests", "golden", "q8_qat.cfg"))
    state = O.init_state(blocks, seed=0)
    st, mk = Q4.dequantised_state(blocks, state, list(range(3, 11)))
    assert mk is None
    changed = [k for k in state if not torch.equal(state[k], st[k])]
    assert sorted(int(re.search(r"conv(\d+)\.weight$", k).group(1)) for k in changed) == list(range(3, 11))
    for k in changed:
        assert torch.equal(st[k], Q4.fakequant(state[k].float()))


# ------------------------------------------------------------------------------------------------ entry points
def test_w4_qat_entry_points_are_exported():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    assert "fp8-w4-qat" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mcamd_[a-z0-9_]+)\s*\(", hdr))
    lib = L.lib()
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    for fn in ("conv_fwd_q8_w4_raw", "fakequant_q8_w4"):
        assert hasattr(ops, fn), fn


def test_launch_entries_refuse_bad_arguments_before_launching():
    """Made-up addresses are never touched: every call below is refused on the host."""
    lib = L.lib()
    g = ops.geom(2, 9, 11, 3, 64, 72, 64)
    bad = ops.geom(1, 208, 208, 3, 32, 64, 32)                           # cin % 64 != 0
    fake = C.c_void_p(4096)
    rows = ops.conv_fwd_q8_stats_rows(g)
    assert rows == 2

    def epi(mode=L.EPI_RAW_F32, stats=None, stats_rows=0, stats_ld=0, y=4096, y_ld=72):
        e = L.ConvEpilogue()
        e.mode, e.y, e.y_ld, e.stats, e.stats_rows, e.stats_ld = mode, y, y_ld, stats, stats_rows, stats_ld
        return e

    raw = lib.mcamd_conv_fwd_q8_w4_raw
    for args in ((None, fake, fake, fake), (fake, None, fake, fake), (fake, fake, None, fake), (fake, fake, fake, None)):
        assert raw(C.byref(g), *args, C.byref(epi()), None) == -1 and b"null input" in lib.mcamd_last_error(), args
    assert raw(C.byref(g), fake, fake, fake, fake, None, None) == -1
    assert raw(None, fake, fake, fake, fake, C.byref(epi()), None) == -1
    assert raw(C.byref(g), fake, fake, fake, fake, C.byref(epi(y=None)), None) == -1 and b"null output" in lib.mcamd_last_error()
    assert raw(C.byref(bad), fake, fake, fake, fake, C.byref(epi()), None) == -1 and b"mcamd_conv_fwd_q8_w4_ok" in lib.mcamd_last_error()
    for mode in (L.EPI_PAD_F16, L.EPI_RAW_F16, L.EPI_NCHW_F32):
        assert raw(C.byref(g), fake, fake, fake, fake, C.byref(epi(mode=mode)), None) == -1
        assert b"MCAMD_EPI_RAW_F32" in lib.mcamd_last_error(), mode
    for r_ in (rows - 1, rows + 1, 0):
        assert raw(C.byref(g), fake, fake, fake, fake, C.byref(epi(stats=4096, stats_rows=r_, stats_ld=256)), None) == -1
        assert b"stats_rows must be %d" % rows in lib.mcamd_last_error(), r_
    assert raw(C.byref(g), fake, fake, fake, fake, C.byref(epi(stats=4096, stats_rows=rows, stats_ld=128)), None) == -1
    assert b"stats_ld" in lib.mcamd_last_error()
    assert raw(C.byref(g), fake, fake, fake, fake, C.byref(epi(y_ld=64)), None) == -1          # the slice does not fit
    # the inference entry keeps refusing the raw mode with its own message
    assert lib.mcamd_conv_fwd_q8_w4(C.byref(g), fake, fake, fake, fake, C.byref(epi()), 0, 0, None) == -1
    assert b"MCAMD_EPI_PAD_F16" in lib.mcamd_last_error()
    fq = lib.mcamd_fakequant_q8_w4
    for args in ((None, fake, fake, fake), (fake, None, fake, fake), (fake, fake, None, fake), (fake, fake, fake, None)):
        assert fq(C.byref(g), *args, None) == -1 and b"null pointer" in lib.mcamd_last_error(), args
    assert fq(None, fake, fake, fake, fake, None) == -1
    assert fq(C.byref(bad), fake, fake, fake, fake, None) == -1 and b"mcamd_conv_fwd_q8_w4_ok" in lib.mcamd_last_error()


# ------------------------------------------------------------------------------------------------ the precision
def test_precision_env_reaches_darknet():
    env = dict(os.environ, MCAMD_PRECISION="fp8-w4-qat")
    code = ("from modelcompression_amd import nets, YOLOV2_VOC_CFG; m = nets.Darknet(YOLOV2_VOC_CFG); print(m.precision, m.sparse, m.splitk)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "fp8-w4-qat None False"


def test_engine_knows_the_precision_and_still_refuses_an_unknown_one_by_name():
    from modelcompression_amd.engine import Engine
    with pytest.raises(L.McamdError, match="'fp8-w4-qat'") as ei:
        Engine(None, 1, 416, 416, "cpu", precision="fp8-w4-qa")
    assert "'fp8-w4'" in str(ei.value) and "'fp8-qat'" in str(ei.value) and "'fp8-w4-qa'" in str(ei.value)


def test_form_table_trains_the_w4_form():
    from modelcompression_amd import engine as E
    form = E._FORMS["q8_w4"]
    assert form.bufs == (("w4c", torch.uint8), ("w4g", torch.uint8), ("wexp4", torch.int32))
    assert (form.fwd, form.elems, form.packer, form.geom) == ("conv_fwd_q8_w4", "q8_w4_elems", "pack_q8_w4", "geom_q8")
    assert type(form).qat_raw is not E._Q8.qat_raw and type(form).pack is not E._Q8.pack
    assert "w_q" in E._LAYER_FIELDS and E._Layer().w_q is None


# ------------------------------------------------------------------------------------------------ the GPU file's cases
def test_raw_cases_reach_every_instance(setenv):
    """The raw launch takes mcamd_q8_choice's tile of the raw fp8 block; the cases reach all five instances of
    w4_cases.INSTANCES with every row, the long-K row on (0, 128) and (1, 256)."""
    reached = {}
    for c in C4.CASES:
        QC.apply_env(c, setenv)
        r = QC.info_of(c)
        assert QC.instance_of(c, r) == c.expect, c.name
        assert list(r) == list(WC.info_of(c)), "the w4 query names the same tile"
        assert set(c.tags) - set(QC.VALUE_TAGS) <= QC.boundary_tags(c, r), c.name
        reached.setdefault((r.f8mfma, r.bmw), set()).add(c.name.split("-", 1)[1])
    assert set(reached) == set(WC.INSTANCES)
    for inst, rows in reached.items():
        assert rows >= set(C4.ROWS), (inst, rows)
    assert "long-k" in reached[(0, 128)] and "long-k" in reached[(1, 256)]
    assert set(C4.DETERMINISM_CASES) <= {c.name for c in C4.CASES}


@pytest.mark.parametrize("c", C4.CASES, ids=str)
def test_raw_case_meets_the_conditions_of_exactness(c):
    """From the reference's operands alone: exact fp32 sums in any order, fp32 raw values, per-channel sums of squares exact in
    fp32 (condition 3), and under the fp8 MFMA every product inside its width.  Rounding happens; every instance keeps the
    r-stats row on some draw."""
    o, ref, draw = C4.operands_and_reference(c)
    assert QC.exactness(c, o, ref) == [], (c.name, draw)
    if not c.wdraw.startswith("s"):
        assert draw in ("W4_DRAW", "W4_DRAW_F16")
        s = o.w.double() * torch.pow(2.0, ref.e.double()).view(-1, 1, 1, 1)
        assert bool((R.deq(ref.w8).double() != s).any()), "some weight is not on the grid: the quantiser rounds"
    if c.stats:
        assert ref.s1.shape == (-(-c.M // 128), c.cout) and bool((ref.s2 > 0).any())
        assert torch.equal(ref.s2.float().double(), ref.s2) and torch.equal(ref.s1.float().double(), ref.s1)
