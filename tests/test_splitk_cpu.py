"""Host logic of the split-K forward (csrc/conv_splitk.hip, api.hip): the slice policy on YOLOv2-VOC's conv stack, the
info query and every refusal, through the library, without a GPU (nothing here launches: each refusal comes before the
first launch)."""
import ctypes as C
import importlib.util
import os

import pytest

from modelcompression_amd import _lib as L, ops, YOLOV2_VOC_CFG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_CHUNKS = 8          # MCAMD_SPLITK_MIN_CHUNKS' default (csrc/conv_splitk.hip)
BIG_3X3 = (14, 16, 18, 19, 20, 22)      # the 13x13 3x3 layers (conv numbers)


def _conv_stack():
    spec = importlib.util.spec_from_file_location("conv_route_table", os.path.join(ROOT, "tools", "conv_route_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.conv_stack(YOLOV2_VOC_CFG, 416, 416)


def _geom(B, k, cin, cout, h, w, **kw):
    return ops.geom(B, h, w, k, cin, cout, ops.round_up(cin, 32), **kw)


def test_policy_splits_the_13x13_layers_at_batch_1():
    stack = _conv_stack()
    assert len(stack) == 23
    for n in BIG_3X3:
        k, cin, cout, h, w = stack[n - 1]
        assert (k, h, w) == (3, 13, 13), (n, stack[n - 1])
        info = ops.conv_fwd_splitk_info(_geom(1, k, cin, cout, h, w), L.EPI_PAD_F16)
        assert info.slices >= 2, (n, info.slices)
        assert 128 <= info.tiles * info.slices <= 512, (n, info.tiles, info.slices)
        assert info.chunks // info.slices >= MIN_CHUNKS, (n, info.chunks, info.slices)      # the shortest slice: floor(n / S)
        assert info.chunks == 9 * ops.round_up(cin, 32) // info.bk


def test_policy_splits_nothing_at_batch_64():
    for (k, cin, cout, h, w) in _conv_stack()[1:]:
        for mode in (L.EPI_PAD_F16, L.EPI_RAW_F16):
            assert ops.conv_fwd_splitk_info(_geom(64, k, cin, cout, h, w), mode).slices == 1, (k, cin, cout, h, w)


def test_policy_constants_are_switches(setenv):
    g = _geom(1, 3, 1024, 1024, 13, 13)
    base = ops.conv_fwd_splitk_info(g, L.EPI_PAD_F16)
    setenv("MCAMD_SPLITK_CUS", "512")
    more = ops.conv_fwd_splitk_info(g, L.EPI_PAD_F16)
    assert more.slices > base.slices and more.tiles * more.slices <= 512
    setenv("MCAMD_SPLITK_MIN_CHUNKS", str(base.chunks))
    assert ops.conv_fwd_splitk_info(g, L.EPI_PAD_F16).slices == 1


@pytest.mark.parametrize("shape, n", [((1, 3, 128, 64, 13, 13), 18), ((2, 3, 96, 72, 6, 10), 27), ((1, 1, 192, 64, 13, 13), 3)])
def test_info_query_chunk_ranges_and_workspace(shape, n):
    B, k, cin, cout, h, w = shape
    g = _geom(B, k, cin, cout, h, w)
    prev = 0
    for S in range(1, min(n, 16) + 1):
        info = ops.conv_fwd_splitk_info(g, L.EPI_PAD_F16, slices=S)
        assert info.slices == S and info.chunks == n
        assert info.tiles == -(-B * h * w // info.bm) * -(-cout // info.bn)
        # the ranges the partial kernel walks: [floor(s n / S), floor((s + 1) n / S))
        ranges = [(s * n // S, (s + 1) * n // S) for s in range(S)]
        assert ranges[0][0] == 0 and ranges[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and all(lo < hi for lo, hi in ranges)
        assert info.workspace_bytes >= prev and info.workspace_bytes >= S * B * h * w * cout * 4
        prev = info.workspace_bytes


def _refused(rc, *words):
    assert rc == -1
    text = L.lib().mcamd_last_error().decode()
    for wd in words:
        assert wd in text, (wd, text)


def test_refusals():
    lib = L.lib()
    info = L.SplitkInfo()
    ok = _geom(1, 3, 128, 64, 13, 13)
    assert lib.mcamd_conv_fwd_splitk_info(C.byref(ok), L.EPI_PAD_F16, 0, 0, C.byref(info)) == 0

    def q(g, mode=L.EPI_PAD_F16, dst=0, slices=0):
        return lib.mcamd_conv_fwd_splitk_info(C.byref(g) if g is not None else None, mode, dst, slices, C.byref(info))

    _refused(q(None), "null geometry")
    _refused(q(ops.geom(1, 32, 32, 3, 3, 32, 4, stem=1)), "stem")
    _refused(q(_geom(1, 3, 128, 64, 13, 13, pad=1)), "pad")
    _refused(q(ops.geom(1, 13, 13, 3, 192, 64, 128, x_wrap=128)), "x_wrap")
    _refused(q(ops.geom(1, 13, 13, 3, 128, 64, 128, x_f8=64)), "x_f8")
    _refused(q(ok, mode=L.EPI_NCHW_F32), "mode 1")
    _refused(q(ok, mode=L.EPI_RAW_F32), "mode 3")
    _refused(q(ok, slices=info.chunks + 1), "slices", "chunks")
    _refused(q(ok, slices=-1), "slices")
    _refused(q(ok, mode=L.EPI_RAW_F16, dst=L.DST_POOL), "dst_mode")

    # the launch entry: every refusal comes before the first launch, so made-up addresses are never touched
    fake = C.c_void_p(4096)
    e = L.ConvEpilogue()
    e.mode, e.y_ld, e.y, e.slope = L.EPI_PAD_F16, 64, 4096, 0.1
    need = ops.conv_fwd_splitk_info(ok, L.EPI_PAD_F16, slices=2).workspace_bytes

    def run(g=ok, epi=e, slices=2, ws=fake, nbytes=need):
        return lib.mcamd_conv_fwd_splitk(C.byref(g) if g is not None else None, fake, fake,
                                         C.byref(epi) if epi is not None else None, slices, ws, nbytes, None)

    _refused(run(g=None), "null geometry")
    _refused(run(epi=None), "null epilogue")
    _refused(run(ws=None), "null workspace")
    _refused(run(nbytes=need - 1), "workspace_bytes", str(need))
    _refused(run(slices=info.chunks + 1, nbytes=1 << 40), "slices", "chunks")
    _refused(run(g=_geom(1, 3, 128, 64, 13, 13, pad=1)), "pad")
    for mode in (L.EPI_NCHW_F32, L.EPI_RAW_F32):
        e2 = L.ConvEpilogue()
        e2.mode, e2.y_ld, e2.y = mode, 64, 4096
        _refused(run(epi=e2), "mode %d" % mode)
    e3 = L.ConvEpilogue()
    e3.mode, e3.y_ld, e3.y, e3.stats, e3.stats_rows, e3.stats_ld = L.EPI_RAW_F16, 64, 4096, 4096, 1, 256
    _refused(run(epi=e3), "stats")


def test_darknet_splitk_defaults_to_false(monkeypatch):
    from modelcompression_amd.nets import Darknet
    monkeypatch.delenv("MCAMD_SPLITK", raising=False)
    assert Darknet(os.path.join(ROOT, "tests", "golden", "mini.cfg")).splitk is False
