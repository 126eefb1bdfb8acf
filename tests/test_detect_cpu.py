"""csrc/detect.hip without a device: the three entry points are declared, exported, bound and wrapped, and every argument
error is refused before a launch with a message in mcamd_last_error()."""
import ctypes as C
import os
import re

import pytest
import torch

from modelcompression_amd import _lib, ops, nets2_utils as U
from modelcompression_amd.predict import PASCALVOCEval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcamd_region_decode", "mcamd_nms", "mcamd_detect")
P = 4096        # a non-null, 16-byte aligned address that is never dereferenced: every call below fails validation first


def desc(**kw):
    d = _lib.DetectDesc()
    d.output, d.B, d.H, d.W, d.num_anchors, d.num_classes = P, 2, 13, 13, 5, 20
    for i in range(10):
        d.anchors[i] = 1.0 + i
    d.conf_thresh, d.nms_thresh = 0.25, 0.45
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def err():
    return _lib.lib().mcamd_last_error().decode()


def test_symbols_are_declared_exported_bound_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.lib()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct mcamd_detect_desc" in hdr
    for f in (ops.region_decode, ops.nms, ops.detect, U.detections_device, U.detections_fused):
        assert callable(f)
    assert ops.DETECT_MAX_ROWS == 2048
    assert isinstance(PASCALVOCEval.fused, bool)
    src = open(os.path.join(ROOT, "modelcompression_amd", "build.py")).read()
    assert re.search(r'"detect\.hip": \["-ffp-contract=off"\]', src)


@pytest.mark.parametrize("bad, text", [
    (dict(output=None), "null argument"),
    (dict(num_anchors=9), "9 anchors <= 8"),
    (dict(num_anchors=0), "bad shape"),
    (dict(num_classes=81), "81 classes <= 80"),
    (dict(num_classes=0), "bad shape"),
    (dict(B=0), "bad shape"),
    (dict(H=0), "bad shape"),
    (dict(H=21, W=20), "2100 rows per image, at most 2048"),        # 21 x 20 x 5
    (dict(H=1 << 15, W=1 << 15, num_anchors=8), "at most 2048"),    # the row count does not wrap in 32 bits
])
def test_decode_and_detect_refuse_bad_descriptors(bad, text):
    lib = _lib.lib()
    d = desc(**bad)
    assert lib.mcamd_region_decode(C.byref(d), P, P, None) == -1
    assert text in err() and err().startswith("region_decode:"), err()
    assert lib.mcamd_detect(C.byref(d), P, P, P, None, None, None) == -1
    assert text in err() and err().startswith("detect:"), err()


def test_null_pointers_are_refused():
    lib = _lib.lib()
    d = desc()
    assert lib.mcamd_region_decode(None, P, P, None) == -1 and "null argument" in err()
    for args in ((None, P), (P, None)):
        assert lib.mcamd_region_decode(C.byref(d), *args, None) == -1 and "region_decode: null argument" in err()
    assert lib.mcamd_detect(None, P, P, P, None, None, None) == -1 and "null argument" in err()
    for args in ((None, P, P), (P, None, P), (P, P, None)):
        assert lib.mcamd_detect(C.byref(d), *args, None, None, None) == -1 and "detect: null argument" in err()
    for args in ((None, P, P, P), (P, None, P, P), (P, P, None, P), (P, P, P, None)):
        b, c, o, k = args
        assert lib.mcamd_nms(b, c, 1, 8, 0.45, o, k, None) == -1 and "nms: null argument" in err()


def test_nms_refuses_bad_sizes():
    lib = _lib.lib()
    assert lib.mcamd_nms(P, P, 1, 2049, 0.45, P, P, None) == -1 and "2049 boxes per image, at most 2048" in err()
    assert lib.mcamd_nms(P, P, 1, 0, 0.45, P, P, None) == -1 and "bad shape" in err()
    assert lib.mcamd_nms(P, P, 0, 8, 0.45, P, P, None) == -1 and "bad shape" in err()
    assert lib.mcamd_nms(P + 4, P, 1, 8, 0.45, P, P, None) == -1 and "16-byte aligned" in err()


def test_wrappers_have_no_cpu_path():
    out = torch.zeros(1, 125, 13, 13)
    anchors = [1.0] * 10
    with pytest.raises(_lib.McamdError):
        ops.region_decode(out, anchors, 5, 20)
    with pytest.raises(_lib.McamdError):
        ops.nms(torch.zeros(1, 4, 4), torch.zeros(1, 4), 0.45)
    with pytest.raises(_lib.McamdError):
        U.detections_device(out, 0.25, 0.45, 20, anchors, 5)
    with pytest.raises(_lib.McamdError):
        U.detections_fused(out, 0.25, 0.45, 20, anchors, 5)
