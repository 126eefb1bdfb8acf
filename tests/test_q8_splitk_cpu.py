"""Host logic of the fp8 split-K forward (csrc/conv_q8_splitk.hip, api.hip; Darknet.precision = "fp8-splitk"):
the slice policy on YOLOv2-VOC's fp8 blocks -- it is the fp16 pair's, answer for answer --, the info query, every refusal
(nothing here launches: each refusal comes before the first launch), the precision name, and the conditions of exactness of
every case of test_q8_splitk_kernels_gpu.py.  No GPU."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import _lib as L, ops, YOLOV2_VOC_CFG  # noqa: E402
import q8_cases as QC  # noqa: E402
import q8_splitk_cases as SKC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8_CONVS = range(3, 23)                  # conv3 ... conv22: Engine.fp8_layers of YOLOv2-VOC
MUST_SPLIT = (14, 16, 18, 19, 20, 22)     # the 13x13 3x3 layers
NEW = ("mcamd_conv_fwd_q8_splitk_info", "mcamd_conv_fwd_q8_splitk")


def _conv_stack():
    spec = importlib.util.spec_from_file_location("conv_route_table", os.path.join(ROOT, "tools", "conv_route_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.conv_stack(YOLOV2_VOC_CFG, 416, 416)


def _geom(B, k, cin, cout, h, w, **kw):
    return ops.geom(B, h, w, k, cin, cout, ops.round_up(cin, 64), **kw)


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mcamd_[a-z0-9_]+)\s*\(", hdr))
    lib = L.lib()
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES["mcamd_conv_fwd_q8_splitk_info"][1]) == 4 and len(L.SIGNATURES["mcamd_conv_fwd_q8_splitk"][1]) == 11


@pytest.mark.parametrize("B", [1, 2, 4, 8, 64])
def test_policy_is_the_fp16_pairs_on_every_fp8_block(B):
    stack = _conv_stack()
    assert len(stack) == 23
    split = []
    for n in FP8_CONVS:
        k, cin, cout, h, w = stack[n - 1]
        assert cin % 64 == 0
        g = _geom(B, k, cin, cout, h, w)
        q, f = ops.conv_fwd_q8_splitk_info(g), ops.conv_fwd_splitk_info(g, L.EPI_PAD_F16)
        assert f.bk == 64 and q.bk == 64, (n, f.bk, q.bk)                      # both walk 64-wide chunks here
        assert (q.slices, q.chunks, q.tiles) == (f.slices, f.chunks, f.tiles), (B, n)
        assert q.chunks == k * k * cin // 64 and q.workspace_bytes == f.workspace_bytes
        if q.slices >= 2:
            split.append(n)
    if B == 1:
        assert set(split) >= set(MUST_SPLIT), split
    if B == 64:
        assert split == []


@pytest.mark.parametrize("shape, n", [((1, 3, 128, 64, 13, 13), 18), ((2, 3, 64, 72, 6, 10), 9), ((1, 1, 192, 64, 13, 13), 3),
                                      ((1, 3, 1280, 256, 13, 13), 180)])
def test_forced_slices_chunk_ranges_and_workspace(shape, n):
    B, k, cin, cout, h, w = shape
    g = _geom(B, k, cin, cout, h, w)
    prev = 0
    for S in range(1, min(n, 16) + 1):
        info = ops.conv_fwd_q8_splitk_info(g, slices=S)
        assert info.slices == S and info.chunks == n and (info.bm, info.bn, info.bk) == (64, 64, 64)
        assert info.tiles == -(-B * h * w // info.bm) * -(-cout // info.bn)
        # the ranges the partial kernel walks: [floor(s n / S), floor((s + 1) n / S))
        ranges = [(s * n // S, (s + 1) * n // S) for s in range(S)]
        assert ranges[0][0] == 0 and ranges[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and all(lo < hi for lo, hi in ranges)
        assert info.workspace_bytes >= prev and info.workspace_bytes >= S * B * h * w * cout * 4
        prev = info.workspace_bytes


def test_policy_constants_are_switches(setenv):
    g = _geom(1, 3, 1024, 1024, 13, 13)
    base = ops.conv_fwd_q8_splitk_info(g)
    setenv("MCAMD_SPLITK_CUS", "512")
    more = ops.conv_fwd_q8_splitk_info(g)
    assert more.slices > base.slices and more.tiles * more.slices <= 512
    setenv("MCAMD_SPLITK_MIN_CHUNKS", str(base.chunks))
    assert ops.conv_fwd_q8_splitk_info(g).slices == 1


def _refused(rc, *words):
    assert rc == -1
    text = L.lib().mcamd_last_error().decode()
    for wd in words:
        assert wd in text, (wd, text)


def test_refusals():
    lib = L.lib()
    info = L.SplitkInfo()
    ok = _geom(1, 3, 128, 64, 13, 13)
    assert lib.mcamd_conv_fwd_q8_splitk_info(C.byref(ok), 0, 0, C.byref(info)) == 0
    chunks = info.chunks

    def q(g, dst=0, slices=0):
        return lib.mcamd_conv_fwd_q8_splitk_info(C.byref(g) if g is not None else None, dst, slices, C.byref(info))

    _refused(q(None), "null geometry")
    _refused(q(ops.geom(1, 32, 32, 3, 3, 32, 4, stem=1)), "stem")
    _refused(q(_geom(1, 3, 128, 64, 13, 13, pad=1)), "pad")
    _refused(q(ops.geom(1, 13, 13, 3, 96, 64, 128)), "cin 96", "cin % 64")
    _refused(q(ok, slices=chunks + 1), "slices", "chunks")
    _refused(q(ok, slices=-1), "slices", "negative")
    _refused(q(ok, dst=7), "dst_mode")
    assert lib.mcamd_conv_fwd_q8_splitk_info(C.byref(ok), 0, 0, None) == -1

    # the launch entry: every refusal comes before the first launch, so made-up addresses are never touched
    fake = C.c_void_p(4096)
    e = L.ConvEpilogue()
    e.mode, e.y_ld, e.y, e.slope = L.EPI_PAD_F16, 64, 4096, 0.1
    need = ops.conv_fwd_q8_splitk_info(ok, slices=2).workspace_bytes

    def run(g=ok, epi=e, slices=2, ws=fake, nbytes=need, x=fake, w=fake, we=fake):
        return lib.mcamd_conv_fwd_q8_splitk(C.byref(g) if g is not None else None, x, w, we,
                                            C.byref(epi) if epi is not None else None, 1, 0, slices, ws, nbytes, None)

    _refused(run(g=None), "null geometry")
    _refused(run(epi=None), "null epilogue")
    for kw in (dict(x=None), dict(w=None), dict(we=None)):
        _refused(run(**kw), "null input")
    _refused(run(ws=None), "null workspace", str(need))
    _refused(run(nbytes=need - 1), "workspace_bytes", str(need))
    _refused(run(ws=C.c_void_p(4096 + 8)), "16-byte aligned", str(need))
    _refused(run(slices=chunks + 1, nbytes=1 << 40), "slices", "chunks")
    _refused(run(slices=-1), "slices", "negative")
    _refused(run(g=ops.geom(1, 32, 32, 3, 3, 32, 4, stem=1)), "stem")
    _refused(run(g=_geom(1, 3, 128, 64, 13, 13, pad=1)), "pad")
    _refused(run(g=ops.geom(1, 13, 13, 3, 96, 64, 128)), "cin 96")
    for mode in (L.EPI_RAW_F16, L.EPI_NCHW_F32, L.EPI_RAW_F32):
        e2 = L.ConvEpilogue()
        e2.mode, e2.y_ld, e2.y = mode, 64, 4096
        _refused(run(epi=e2), "mode %d" % mode, "MCAMD_EPI_PAD_F16")
    e3 = L.ConvEpilogue()
    e3.mode, e3.y_ld, e3.y, e3.slope, e3.stats, e3.stats_rows, e3.stats_ld = L.EPI_PAD_F16, 64, 4096, 0.1, 4096, 1, 256
    _refused(run(epi=e3), "stats")


def test_precision_env_reaches_darknet():
    env = dict(os.environ, MCAMD_PRECISION="fp8-splitk")
    code = ("from modelcompression_amd import nets, YOLOV2_VOC_CFG; m = nets.Darknet(YOLOV2_VOC_CFG); print(m.precision, m.splitk)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "fp8-splitk False"


def test_unknown_precision_raises_and_the_message_lists_the_new_name():
    from modelcompression_amd.engine import Engine
    with pytest.raises(L.McamdError, match="'fp8-splitk'"):
        Engine(None, 1, 416, 416, "cpu", precision="fp8-split")


def test_form_table_has_the_new_form():
    from modelcompression_amd import engine as E
    form = E._FORMS["q8_splitk"]
    assert isinstance(form, E._Q8) and form.fwd == "conv_fwd_q8_splitk" and hasattr(ops, form.fwd)
    assert (form.elems, form.packer, form.geom, form.bufs) == (E._FORMS["q8"].elems, E._FORMS["q8"].packer, "geom_q8", E._FORMS["q8"].bufs)
    lay = E._Layer()
    lay.form = "q8_splitk"
    assert lay.q8_on and [lay.sp_on, lay.bs_on, lay.sk_on, lay.q8_on].count(True) == 1 and not lay.q8s_on and not lay.q8_slim


@pytest.mark.parametrize("sc", SKC.SPLITK_CASES, ids=SKC.case_id)
def test_case_meets_the_conditions_of_exactness(sc):
    """Every kernel case of the GPU file, in the MFMA form it runs in: the fp32 sum is exact in ANY order (so a split sum
    equals the unsplit one), the fp16 outputs are fp16 numbers, and under the fp8 MFMA every product is inside its width."""
    c = sc.c
    o, ref = QC.operands_and_reference(c)
    assert QC.exactness(c, o, ref) == [], c.name
    if o.planted:
        o2, ref2 = QC.operands_and_reference(c, plant=False)
        assert QC.exactness(c, o2, ref2) == [], c.name
    info = ops.conv_fwd_q8_splitk_info(QC.geom_of(c), QC.DSTS[c.dst])
    assert info.chunks == sc.chunks
    for S in sc.slices:
        assert 1 <= SKC.resolved(sc, S) <= min(sc.chunks, 16) or S == sc.chunks
