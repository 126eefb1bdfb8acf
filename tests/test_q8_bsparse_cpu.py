"""Host logic of the block-sparse fp8 forward (csrc/conv_q8_bsparse.hip, api.hip; Darknet.precision = "fp8-block",
DESIGN.md 3za): the entry points, the form table, the precision name, the policy constant, the geometry and instance queries,
every refusal that comes before a launch, and the numpy restatement of the byte lists against bsparse_ref's.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modelcompression_amd import _lib as L, ops, nets, YOLOV2_VOC_CFG  # noqa: E402
import bsparse_ref as BR  # noqa: E402
import q8_bsparse_ref as R  # noqa: E402
import q8_ref as Q  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mcamd_conv_fwd_q8_bsparse_ok": "conv_fwd_q8_bsparse_ok", "mcamd_q8_bsparse_elems": "q8_bsparse_elems",
       "mcamd_q8_bsparse_lists": "q8_bsparse_lists", "mcamd_conv_fwd_q8_bsparse": "conv_fwd_q8_bsparse",
       "mcamd_conv_fwd_q8_bsparse_info": "conv_fwd_q8_bsparse_info"}
OLD_PRECISIONS = ("fp16", "fp16x3", "mixed", "fp8", "fp8-2:4", "fp8-splitk", "fp8-qat", "fp8-w4", "fp8-w4-qat")


def test_entry_points_are_declared_exported_bound_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mcamd_[a-z0-9_]+)\s*\(", hdr))
    lib = L.lib()
    for name, wrapper in NEW.items():
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
        assert callable(getattr(ops, wrapper, None)), wrapper
    # mcamd_conv_fwd_q8's argument order with the lists behind wexp
    assert len(L.SIGNATURES["mcamd_conv_fwd_q8_bsparse"][1]) == len(L.SIGNATURES["mcamd_conv_fwd_q8"][1]) + 2 == 10
    assert len(L.SIGNATURES["mcamd_q8_bsparse_lists"][1]) == 5 and len(L.SIGNATURES["mcamd_conv_fwd_q8_bsparse_info"][1]) == 2


def test_form_table_has_the_new_form():
    from modelcompression_amd import engine as E
    form = E._FORMS["q8_bsparse"]
    assert isinstance(form, E._Q8) and form.fwd == "conv_fwd_q8_bsparse" and hasattr(ops, form.fwd)
    assert [name for name, _ in form.bufs] == ["wq", "wexp", "bs_count", "bs_list"] and form.geom == "geom_q8"
    assert form.bufs[:2] == E._FORMS["q8"].bufs and all(dt == torch.int32 for _, dt in form.bufs[2:])
    lay = E._Layer()
    lay.form = "q8_bsparse"
    assert lay.q8_on and [lay.sp_on, lay.bs_on, lay.sk_on, lay.q8_on].count(True) == 1 and not lay.q8s_on and not lay.q8_slim


def test_unknown_precision_raises_and_names_every_precision():
    from modelcompression_amd.engine import Engine
    with pytest.raises(L.McamdError) as ei:
        Engine(None, 1, 416, 416, "cpu", precision="fp8-bloc")
    for name in OLD_PRECISIONS + ("fp8-block",):
        assert "'%s'" % name in str(ei.value), name


def test_precision_env_reaches_darknet():
    env = dict(os.environ, MCAMD_PRECISION="fp8-block")
    code = ("from modelcompression_amd import nets, YOLOV2_VOC_CFG; m = nets.Darknet(YOLOV2_VOC_CFG); "
            "print(m.precision, m.sparse, m.splitk)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "fp8-block None False"


def test_policy_constants():
    from modelcompression_amd import engine
    m = nets.Darknet(YOLOV2_VOC_CFG)
    assert m.fp8_block_max_kept == engine.Q8_BSPARSE_MAX_KEPT and 0.0 <= m.fp8_block_max_kept <= 1.0
    assert m.sparse_max_kept == engine.BSPARSE_MAX_KEPT and m.sparse is None


def test_geometry_and_instance_queries(setenv):
    """mcamd_conv_fwd_q8_bsparse_ok / _elems / _info: host logic only."""
    ok = ops.geom(2, 13, 13, 3, 1280, 1024, 1280)
    assert ops.conv_fwd_q8_bsparse_ok(ok) and ops.q8_bsparse_elems(ok) == (16, 16 * 180)
    assert ops.q8_bsparse_elems(ops.geom(2, 9, 11, 3, 128, 200, 192, 32)) == (4, 4 * 18)
    assert ops.q8_bsparse_elems(ops.geom(2, 12, 12, 1, 256, 136, 320, 64)) == (3, 3 * 4)
    for bad in (ops.geom(2, 13, 13, 3, 3, 32, 4, stem=1),                     # the first layer
                ops.geom(2, 13, 13, 3, 96, 64, 128),                          # cin not a multiple of 64
                ops.geom(2, 13, 13, 3, 128, 64, 128, pad=1),                  # the shared-halo form
                ops.geom(2, 13, 13, 5, 64, 64, 64),                           # ksize
                ops.geom(2, 13, 13, 3, 64, 60, 64),                           # cout not a multiple of 8
                ops.geom(2, 13, 13, 3, 64, 64, 64, 32)):                      # slice outside x_ld
        assert not ops.conv_fwd_q8_bsparse_ok(bad)
        for query in (ops.q8_bsparse_elems, ops.conv_fwd_q8_bsparse_info):
            with pytest.raises(L.McamdError):
                query(bad)
    for mfma in (0, 1):
        setenv("MCAMD_Q8_MFMA", str(mfma))
        for (B, h, w, k, cin, cout) in ((2, 13, 13, 3, 1280, 1024), (2, 9, 11, 3, 128, 200), (128, 26, 26, 3, 256, 512)):
            g = ops.geom(B, h, w, k, cin, cout, cin)
            info = ops.conv_fwd_q8_bsparse_info(g)
            mt, nt = -(-B * h * w // 128), -(-cout // 64)
            assert info == ops.Q8Info(64, 128, mfma, 3, mt, nt, -(-mt // 8) * 8 * nt)
            assert info.f8mfma == ops.conv_fwd_q8_info(g).f8mfma


def test_refusals_before_any_launch():
    lib = L.lib()
    fake = C.c_void_p(4096)
    ok = ops.geom(1, 13, 13, 3, 128, 64, 128)
    e = L.ConvEpilogue()
    e.mode, e.y_ld, e.y, e.slope = L.EPI_PAD_F16, 64, 4096, 0.1

    def refused(rc, *words):
        assert rc == -1
        text = lib.mcamd_last_error().decode()
        for wd in words:
            assert wd in text, (wd, text)

    def run(g=ok, epi=e, x=fake, w=fake, we=fake, cnt=fake, lst=fake):
        return lib.mcamd_conv_fwd_q8_bsparse(C.byref(g), x, w, we, cnt, lst, C.byref(epi) if epi is not None else None, 1, 0, None)

    for kw in (dict(x=None), dict(w=None), dict(we=None), dict(cnt=None), dict(lst=None)):
        refused(run(**kw), "null input")
    refused(run(g=ops.geom(1, 13, 13, 3, 128, 64, 128, pad=1)), "mcamd_conv_fwd_q8_bsparse_ok")
    refused(run(g=ops.geom(1, 13, 13, 3, 96, 64, 128)), "mcamd_conv_fwd_q8_bsparse_ok")
    for mode in (L.EPI_RAW_F16, L.EPI_NCHW_F32, L.EPI_RAW_F32):
        e2 = L.ConvEpilogue()
        e2.mode, e2.y_ld, e2.y = mode, 64, 4096
        refused(run(epi=e2), "MCAMD_EPI_PAD_F16")
    refused(lib.mcamd_q8_bsparse_lists(C.byref(ok), None, fake, fake, None), "null pointer")
    refused(lib.mcamd_q8_bsparse_lists(C.byref(ok), C.c_void_p(4096 + 8), fake, fake, None), "16-byte aligned")
    # 8193 chunks of one tap: more flags than the list kernel holds
    refused(lib.mcamd_q8_bsparse_lists(C.byref(ops.geom(1, 4, 4, 1, 8193 * 64, 64, 8193 * 64)), fake, fake, fake, None), "8192")


@pytest.mark.parametrize("shape", [(136, 128, 3), (72, 256, 1), (200, 192, 3)])
def test_byte_lists_agree_with_the_fp16_lists(shape):
    """On a packing whose bytes are non-zero exactly where the fp16 values are, the byte lists are bsparse_ref.chunk_lists of
    the fp16 packing (kb = 64: the same K order); both e4m3 zeros count as zero, and a weight that rounds to the zero byte
    drops its chunk from the byte lists only."""
    cout, cin, k = shape
    gen = torch.Generator().manual_seed(cout + cin)
    w = torch.randn(cout, cin, k, k, generator=gen)
    w = w + 0.5 * torch.sign(w)                                   # |w| in [0.5, ~5]: no value rounds to zero in either format
    nfb, ncb, kb = BR.block_dims(cout, cin, k * k)
    assert kb == 64
    keep = (torch.rand(nfb * ncb * k * k, generator=gen) > 0.6).to(torch.int32).numpy()
    keep[:ncb * k * k] = 0                                        # tile 0 empty
    mask = torch.from_numpy(BR.block_mask(keep, (cout, cin, k, k)))
    w8, e = Q.quantise_weights(w, mask)
    packed8 = R.pack_bytes(w8.numpy())
    packed16 = BR.pack_fwd(w.numpy(), mask.numpy())
    assert packed8.shape == packed16.shape and np.array_equal((packed8 & 0x7F) != 0, packed16 != 0)
    assert bool((packed8 == 0x80).any()), "negative weights under the mask pack to -0: the case the sign mask is for"
    count, lst = R.chunk_lists(packed8, cout)
    rc, rl = BR.chunk_lists(packed16, cout, kb)
    assert np.array_equal(count, rc) and np.array_equal(lst, rl) and count[0] == 0
    assert abs(R.kept_fraction(packed8, cout) - rc.sum() / rl.size) < 1e-15
    # a kept chunk of a tile that keeps another one, shrunk by 2^-20: every filter's exponent still comes from the other
    # chunks (its largest weight lands in (224, 448]), so the shrunk weights land below 448 * 2^-20 < 2^-10, half the smallest
    # e4m3 subnormal, and round to the zero byte -- while 0.5 * 2^-20 is still an fp16 subnormal
    t = int(np.nonzero(rc >= 2)[0][0])
    q = int(rl[t, 0])
    cb, tap = q // (k * k), q % (k * k)
    w2 = w.clone()
    w2[64 * t:64 * t + 64, 64 * cb:64 * cb + 64, tap // k, tap % k] *= 2.0 ** -20
    w8b, _ = Q.quantise_weights(w2, mask)
    c2, l2 = R.chunk_lists(R.pack_bytes(w8b.numpy()), cout)
    c16, _ = BR.chunk_lists(BR.pack_fwd(w2.numpy(), mask.numpy()), cout, kb)
    assert c2[t] == rc[t] - 1 and q not in l2[t, :c2[t]].tolist() and c16[t] == rc[t]
