"""What the exact bn_act_fwd_kernel tests (test_act_instances_gpu.py) rest on, checked without a GPU: the case table reaches
every instance mcamd_bn_act_fwd can launch (asked through mcamd_bn_act_fwd_instance, the launch's own decision function) and
every addressing / storage combination the table promises; the float64 restatement agrees with torch's operators; every case's
operands satisfy the conditions that make the result independent of the kernel's arithmetic order; and the query refuses
what the launch refuses."""
import ctypes as C
import functools
import itertools

import pytest
import torch

from modelcompression_amd import ops, _lib as L
import act_cases as A
import act_ref as R

IDS = [c.name for c in A.CASES]


def case_args(c, y, scale, shift, dst, dst2=None, border=None, pool_act=None, dst_q8=None, dst2_q8=None):
    """the arguments of ops.bn_act_fwd / ops.bn_act_fwd_instance for a case and its buffers"""
    return ((c.B, c.H, c.W, c.C, y, c.y_ld, c.y_choff, scale, shift, c.slope, c.mode, dst, c.dst_ld, c.dst_choff),
            dict(dst2=dst2, dst2_ld=c.dst2_ld, dst2_choff=c.dst2_choff, border=border, planes=c.planes, dst_plane=c.dst_plane,
                 dst2_plane=c.dst2_plane, dst_pad=c.dst_pad, dst2_pad=c.dst2_pad, planes2=c.planes2 if c.dst2 else 0,
                 pool_act=pool_act, pool_act_ld=c.pool_act_ld, pool_act_pad=c.pool_act_pad, dst_q8=dst_q8, dst2_q8=dst2_q8))


@functools.lru_cache(maxsize=None)
def query(c):
    """the instance the library names for a case; host memory stands for the buffers (the query reads no pointer)"""
    f32, f16, u8 = torch.zeros(8), torch.zeros(8, dtype=torch.float16), torch.zeros(8, dtype=torch.uint8)
    a, kw = case_args(c, f32 if c.y32 else f16, f32, f32, f16, dst2=f16 if c.dst2 else None,
                      border=torch.zeros(16, c.C) if c.border else None, pool_act=f16 if c.pool_act else None,
                      dst_q8=u8 if c.twin else None, dst2_q8=u8 if c.twin2 else None)
    return ops.bn_act_fwd_instance(*a, **kw)


def test_query_is_declared_bound_exported_and_documented():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mcamd.h")).read(), flags=re.S)
    name = "mcamd_bn_act_fwd_instance"
    assert name in set(re.findall(r"\b(mcamd_[a-z0-9_]+)\s*\(", hdr)) and name in L.SIGNATURES and hasattr(L.lib(), name)
    fields = re.search(r"typedef struct mcamd_act_instance \{(.*?)\}", hdr, re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [f[0] for f in L.ActInstance._fields_]
    assert C.sizeof(L.ActInstance) == 40 and hasattr(ops, "bn_act_fwd_instance")
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    assert name in doc and "mcamd_act_instance" in doc


def test_table_reaches_all_48_instances():
    got = set()
    for c in A.CASES:
        q = query(c)
        assert (q.mode, q.fixed, q.y32, q.planes, q.q8) == A.instance(c), c.name
        assert q.planes2 == c.planes2 and q.items == c.B * c.H * c.W // (1 if c.mode == A.PLAIN else 4) * (c.C // 8), c.name
        assert q.grid == min(4096, (q.items + 255) // 256), c.name
        got.add(A.instance(c))
    assert len(A.all_instances()) == 48 and got == A.all_instances(), got ^ A.all_instances()
    # FIXED and !FIXED at each channel count of the list, in every mode
    for mode in (A.PLAIN, A.POOL, A.REORG):
        for C_, fixed in [(v, True) for v in A.FIXED_C] + [(v, False) for v in A.RAGGED_C]:
            assert any(c.mode == mode and c.C == C_ and query(c).fixed == fixed for c in A.CASES), (mode, C_)


def test_table_sizes():
    for c in A.SMALL:
        assert c.B * c.C * c.H * c.W <= 100000 and c.H <= 12 and c.W <= 12, c.name
        if c.C == 2056:
            assert (c.B, c.H, c.W) == (1, 2, 2)
        elif (c.H, c.W) != (1, 1):                       # the one case that reaches border class 15
            assert c.B == 2 and c.H != c.W, c.name
    big = {c.name: c for c in A.BIG}
    assert len(big) == 2
    for c in A.BIG:
        q = query(c)
        assert q.items > 4096 * 256 and q.grid == 4096 and c.y32 and c.planes == 1 and not c.border and c.mode == A.PLAIN
    assert sorted((query(c).fixed, c.C, c.B, c.H, c.W) for c in A.BIG) == [(False, 200, 2, 146, 144), (True, 2048, 1, 66, 64)]


def test_table_mixed_forms():
    pairs = {(c.planes, c.planes2) for c in A.CASES if c.mode == A.POOL and c.dst2 and c.planes >= 2}
    assert pairs >= set(itertools.product((2, 3, 4), repeat=2)), pairs


def test_table_addressing():
    by_form = {}
    for c in A.SMALL:
        by_form.setdefault((c.y32, c.planes, c.q8), []).append(c)
    assert len(by_form) == 8
    for form, cs in by_form.items():
        assert all(c.dst_choff != 0 for c in cs), form
        assert any(c.dst2 and c.dst2_choff != 0 for c in cs), form
        assert all(c.dst2_choff != 0 for c in cs if c.dst2), form
        assert all(c.y_choff != 0 and c.y_ld > c.C + c.y_choff for c in cs), form
        if form[1] >= 2:
            assert all(c.dst_plane > (4 * c.C if c.mode == A.REORG else c.C) for c in cs), form
            assert {c.dst_pad for c in cs} == {0, 1}, form
    assert {(c.dst_pad, c.dst2_pad) for c in A.SMALL if c.dst2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # form 4 as the second member of a route (dst_choff = ca, dst_plane = ca + cb), in every mode
    for mode in (A.PLAIN, A.POOL, A.REORG):
        assert any(c.mode == mode and c.planes == 4 and c.dst_choff >= 64 and
                   c.dst_plane == c.dst_choff + (4 * c.C if mode == A.REORG else c.C) for c in A.CASES), mode
    pa = [c for c in A.CASES if c.pool_act]
    assert any(c.pool_act_ld > c.C for c in pa) and {c.pool_act_pad for c in pa} == {0, 1}
    assert all(A.planted(c) for c in pa)
    assert len({(c.dst_pad, c.dst2_pad, c.pool_act_pad) for c in pa if c.dst2}) >= 4


def test_table_border_classes():
    seen = set()
    for mode in (A.PLAIN, A.POOL, A.REORG):
        cs = [c for c in A.CASES if c.border and c.mode == mode]
        assert cs, mode
        for c in cs:
            seen |= set(R.border_class(c.H, c.W).reshape(-1).tolist())
    assert seen == set(range(16)), seen
    plain = [c for c in A.CASES if c.border and c.mode == A.PLAIN]
    assert any(c.H == 1 and c.W > 1 for c in plain) and any(c.W == 1 and c.H > 1 for c in plain)


def test_table_byte_twins():
    for mode in (A.POOL, A.REORG):
        combos = {(c.twin, c.twin2) for c in A.CASES if c.q8 and c.mode == mode and c.dst2}
        assert combos == {(True, False), (False, True), (True, True)}, (mode, combos)
    assert any(c.q8 and c.mode == A.PLAIN for c in A.CASES) and any(c.q8 and c.mode == A.POOL and not c.dst2 for c in A.CASES)


def test_same_operand_group():
    ops_ = [A.operands(c) for c in A.SAME_OPERANDS]
    assert [c.planes for c in A.SAME_OPERANDS] == [1, 2, 3, 4] and all(c.y32 and c.dst2 for c in A.SAME_OPERANDS)
    for o in ops_[1:]:
        assert torch.equal(o.y, ops_[0].y) and torch.equal(o.scale, ops_[0].scale) and torch.equal(o.shift, ops_[0].shift)


@pytest.mark.parametrize("c", A.CASES + A.SAME_OPERANDS[:1], ids=IDS + [A.SAME_OPERANDS[0].name])
def test_operands_exact_and_reference_anchored(c):
    """The grid conditions hold on the operands (so fused and unfused fp32 evaluation, and the float64 path, give one number),
    the planted edges are there, and the restatement equals F.leaky_relu / F.max_pool2d / Reorg of the reference network
    (src/nets.py:802-821, 648-667, as oracle/darknet_ref.py states it) in float64."""
    op = A.operands(c)
    v = A.exactness(c, op)
    assert R.anchor(c, op) <= 1e-12
    assert bool((op.scale < 0).any())
    if c.big:
        return
    assert float(v.abs().max()) > 65504, "no value clamps hi"
    assert float((2 * v).abs().max()) > 448
    if c.planes == 4 or c.q8:
        codes = R.x8(v)
        assert bool((codes == 0x7E).any()) and not bool(((codes & 0x7F) == 0x7F).any())
        if c.slope == 1.0:
            assert bool((codes == 0xFE).any())
    sub = (v != 0) & (v.abs() < 2.0 ** -14)
    assert bool(sub.any()), "no fp16-subnormal value"
    assert bool(((v == 0) & torch.signbit(v)).any()) and bool(((v == 0) & ~torch.signbit(v)).any()), "+0 and -0"
    if c.planes >= 2:
        assert float((R.bits16(R.lo16(v)) & 0x7FFF != 0).double().mean()) > 0.5, "lo planes mostly zero"
    if c.pool_act:
        bits, moved = R.pool_act_bits(v)
        assert moved >= 1 + 2 + 3 + 3, "the planted windows move 9 elements"
        w = R.window(v)[:, 0]                                             # image 0
        assert bool((w[:, 9, 1, 1] < 0).all())                           # the all-negative window
        assert float(w[2, 8, 0, 0] - w[0, 8, 0, 0]) == (2.0 ** -12 if c.y32 else 2.0 ** -4) and float(w[0, 8, 0, 0]) >= 4


def test_lo8_codes_are_varied():
    """The e4m3 correction strings carry real information: over the form-4 cases most codes of the format occur."""
    seen = set()
    for c in A.SMALL:
        if c.planes == 4:
            seen |= set(R.lo8(R.activation(c, A.operands(c))).reshape(-1).tolist())
    assert len(seen) >= 200, len(seen)


# ------------------------------------------------------------------------------------------------ the query's refusals
def _desc(**over):
    """a valid POOL descriptor with made-up addresses (every refusal comes before the launch: none is touched)"""
    d = L.ActDesc()
    d.B, d.H, d.W, d.C = 2, 4, 6, 64
    d.y = d.scale = d.shift = d.dst = d.dst2 = 4096
    d.y_ld, d.dst_ld, d.dst2_ld, d.mode, d.y_dtype, d.slope = 64, 256, 256, A.POOL, 1, 0.1
    d.planes, d.dst_plane, d.dst2_plane = 2, 64, 64
    for k, v in over.items():
        setattr(d, k, v)
    return d


REFUSED = [dict(y=None), dict(dst=None), dict(scale=None), dict(shift=None), dict(C=0), dict(C=36), dict(y_ld=60), dict(y_choff=4),
           dict(dst_ld=252), dict(dst_choff=4), dict(dst2_ld=250), dict(dst2_choff=2), dict(H=5), dict(W=3), dict(mode=A.PLAIN),
           dict(y_dtype=2), dict(planes=5), dict(planes=-1), dict(planes2=1), dict(planes=1, planes2=2), dict(planes2=7),
           dict(dst_plane=60), dict(dst_plane=56), dict(dst_plane=200), dict(planes=3, dst_plane=128), dict(planes=4, dst_plane=136),
           dict(dst2_plane=56), dict(dst2_plane=200), dict(planes2=4, dst2_plane=136), dict(dst_pad=2), dict(dst2_pad=-1),
           dict(pool_act=4096, pool_act_ld=60), dict(pool_act=4096, pool_act_ld=56), dict(pool_act=4096, pool_act_ld=64, pool_act_pad=2),
           dict(pool_act=4096, pool_act_ld=64, mode=A.REORG, dst_plane=256, dst_ld=1024),
           dict(planes=4, y_dtype=0), dict(dst_q8=4096), dict(dst_q8=4096, planes=1, y_dtype=0),
           dict(dst2_q8=4096, planes=1, dst2=None), dict(dst_q8=4096, planes=1, pool_act=4096, pool_act_ld=64), dict(mode=3), dict(mode=-1)]


def test_query_refuses_what_the_launch_refuses():
    lib = L.lib()
    out = L.ActInstance()
    assert lib.mcamd_bn_act_fwd_instance(C.byref(_desc()), C.byref(out)) == 0 and (out.mode, out.fixed, out.y32, out.planes, out.planes2,
                                                                                   out.q8, out.items, out.grid) == (1, 1, 1, 2, 2, 0, 96, 1)
    ok_variants = [dict(planes=0, planes2=0), dict(dst2=None, dst2_plane=3), dict(pool_act=4096, pool_act_ld=72, pool_act_pad=1),
                   dict(planes=1, dst_q8=4096, dst2_q8=4096)]
    for over in ok_variants:
        assert lib.mcamd_bn_act_fwd_instance(C.byref(_desc(**over)), C.byref(out)) == 0, over
    for over in REFUSED:
        d = _desc(**over)
        rc_q = lib.mcamd_bn_act_fwd_instance(C.byref(d), C.byref(out))
        msg_q = lib.mcamd_last_error()
        rc_l = lib.mcamd_bn_act_fwd(C.byref(d), None)
        msg_l = lib.mcamd_last_error()
        assert rc_q != 0 and rc_q == rc_l and msg_q == msg_l and msg_q.startswith(b"bn_act_fwd"), (over, rc_q, rc_l, msg_q, msg_l)
    assert lib.mcamd_bn_act_fwd_instance(None, C.byref(out)) == lib.mcamd_bn_act_fwd(None, None) != 0
    assert lib.mcamd_bn_act_fwd_instance(C.byref(_desc()), None) != 0
