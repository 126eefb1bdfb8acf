"""Host logic of the split-K fp4-operand forward (csrc/conv_q8_w4_mx.hip, api.hip; Darknet.precision = "fp8-w4-mx-splitk",
DESIGN.md 3zi): the entry points, the policy shared with the fp8 pair, every refusal (each comes before the first launch), the
precision name and form, and the conditions of exactness of every case of test_q8_w4_mx_splitk_kernels_gpu.py.  No GPU."""
import ctypes as C
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import _lib as L, ops  # noqa: E402
import q8_cases as QC  # noqa: E402
import w4_mx_splitk_cases as XC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mcamd_conv_fwd_q8_w4_mx_splitk_info", "mcamd_conv_fwd_q8_w4_mx_splitk")


def _geom(B, k, cin, cout, h, w, **kw):
    return ops.geom(B, h, w, k, cin, cout, ops.round_up(cin, 64), **kw)


def test_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcamd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcamd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(L.lib(), name) and hasattr(ops, name[6:]), name
    assert len(L.SIGNATURES[NEW[0]][1]) == 4 and len(L.SIGNATURES[NEW[1]][1]) == 12


@pytest.mark.parametrize("B", [1, 8])
def test_policy_is_the_fp8_pairs(B):
    g = _geom(B, 3, 1280, 256, 13, 13)
    for S in (0, 16):
        a, b = ops.conv_fwd_q8_w4_mx_splitk_info(g, slices=S), ops.conv_fwd_q8_splitk_info(g, slices=S)
        for f in ("slices", "chunks", "tiles", "bm", "bn", "bk", "workspace_bytes"):
            assert getattr(a, f) == getattr(b, f), (B, S, f)
    assert (a.chunks, a.bm, a.bn, a.bk) == (180, 64, 64, 64)
    assert B > 1 or ops.conv_fwd_q8_w4_mx_splitk_info(g).slices >= 2


def _refused(rc, *words):
    assert rc == -1
    text = L.lib().mcamd_last_error().decode()
    for wd in words:
        assert wd in text, (wd, text)


def test_refusals():
    lib = L.lib()
    info = L.SplitkInfo()
    ok = _geom(1, 3, 128, 64, 13, 13)
    chunks = ops.conv_fwd_q8_w4_mx_splitk_info(ok).chunks
    q = lambda g, dst=0, slices=0: lib.mcamd_conv_fwd_q8_w4_mx_splitk_info(C.byref(g), dst, slices, C.byref(info))
    name = "conv_fwd_q8_w4_mx_splitk_info"
    _refused(q(_geom(1, 3, 128, 64, 13, 13, pad=1)), name, "pad")
    _refused(q(ops.geom(1, 13, 13, 3, 96, 64, 128)), name, "cin 96")                  # a slim geometry
    _refused(q(ops.geom(1, 32, 32, 3, 3, 32, 4, stem=1)), name, "stem")
    _refused(q(ok, slices=chunks + 1), name, "slices", "chunks")
    _refused(q(ok, slices=-1), name, "negative")
    _refused(q(ok, dst=7), name, "dst_mode")

    # the launch entry: made-up addresses are never touched
    fake = C.c_void_p(4096)
    e = L.ConvEpilogue()
    e.mode, e.y_ld, e.y, e.slope = L.EPI_PAD_F16, 64, 4096, 0.1
    need = ops.conv_fwd_q8_w4_mx_splitk_info(ok, slices=2).workspace_bytes

    def run(g=ok, epi=e, slices=2, ws=fake, nbytes=need, x=fake, codes=fake, scales=fake, we=fake):
        return lib.mcamd_conv_fwd_q8_w4_mx_splitk(C.byref(g), x, codes, scales, we, C.byref(epi), 1, 0, slices, ws, nbytes, None)

    name = "conv_fwd_q8_w4_mx_splitk:"
    for kw in (dict(x=None), dict(codes=None), dict(scales=None), dict(we=None)):
        _refused(run(**kw), name, "null input")
    _refused(run(ws=None), name, "null workspace", str(need))
    _refused(run(nbytes=need - 1), name, "workspace_bytes", str(need))
    _refused(run(ws=C.c_void_p(4096 + 8)), name, "16-byte aligned")
    _refused(run(slices=chunks + 1, nbytes=1 << 40), name, "slices", "chunks")
    _refused(run(g=_geom(1, 3, 128, 64, 13, 13, pad=1)), name, "pad")
    _refused(run(g=ops.geom(1, 13, 13, 3, 96, 64, 128)), name, "cin 96")
    e2 = L.ConvEpilogue()
    e2.mode, e2.y_ld, e2.y = L.EPI_RAW_F32, 64, 4096
    _refused(run(epi=e2), name, "MCAMD_EPI_PAD_F16")
    e3 = L.ConvEpilogue()
    e3.mode, e3.y_ld, e3.y, e3.slope, e3.stats, e3.stats_rows, e3.stats_ld = L.EPI_PAD_F16, 64, 4096, 0.1, 4096, 1, 256
    _refused(run(epi=e3), name, "stats")


def test_precision_name_and_form():
    from modelcompression_amd import engine as E
    with pytest.raises(L.McamdError, match="'fp8-w4-mx-splitk'"):
        E.Engine(None, 1, 416, 416, "cpu", precision="fp8-w4-mx-split")
    form, base = E._FORMS["q8_w4_mx_splitk"], E._FORMS["q8_w4_mx"]
    assert isinstance(form, E._Q8W4Mx) and form.fwd == "conv_fwd_q8_w4_mx_splitk"
    assert (form.elems, form.packer, form.geom, form.bufs) == (base.elems, base.packer, "geom_q8", base.bufs)
    assert type(form).pack is type(base).pack                                          # the same packing: the values of the codes
    lay = E._Layer()
    lay.form = "q8_w4_mx_splitk"
    assert lay.q8_on and [lay.sp_on, lay.bs_on, lay.sk_on, lay.q8_on].count(True) == 1 and not lay.q8s_on and not lay.q8_slim


@pytest.mark.parametrize("sc", XC.CASES, ids=XC.case_id)
def test_case_meets_the_conditions_of_exactness(sc):
    """On the reference's operands: every partial sum in every order is an fp32 number, so any grouping of chunks is exact."""
    c = sc.c
    for plant in ((True, False) if "overflow" in c.special else (True,)):
        o, ref = XC.operands_and_reference(c, plant=plant)
        assert QC.exactness(c, o, ref) == [], (c.name, plant)
    assert ops.conv_fwd_q8_w4_mx_splitk_info(QC.geom_of(c), QC.DSTS[c.dst]).chunks == sc.chunks
