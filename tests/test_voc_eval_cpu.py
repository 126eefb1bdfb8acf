"""csrc/voc_eval.hip without a device: the "%f" rounding it reproduces, the numpy restatement of its contract
(tests/voc_eval_ref.py) against the untouched PASCALVOCEval.voc_eval through real detection files, the ground-truth table,
and the argument validation of both entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import voc_eval_ref as R
from modelcompression_amd import _lib, ops
from modelcompression_amd.predict import PASCALVOCEval
from modelcompression_amd.voc_eval import VOCGroundTruth, DeviceVOCEval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096        # a non-null address that is never dereferenced: every call below fails validation first
IDS = ["img%06d" % i for i in range(4)]


def err():
    return _lib.lib().mcamd_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------- q
def test_q_is_the_percent_f_round_trip():
    rng = np.random.RandomState(0)
    ties = (np.arange(-4001, 4001, 2) / 128.0).astype(np.float32)           # odd multiples of 1/128: exact ties at 1e-6
    v = np.concatenate([rng.rand(60000).astype(np.float32), (rng.rand(60000) * 600 - 50).astype(np.float32), ties,
                        np.array([0.0, -0.0, 1.0, 0.0078125, -0.0078125, 0.0234375, 5e-7, 1.5e-6, 549.9999], dtype=np.float32)])
    assert v.size >= 100000 and (v < 0).sum() > 1000
    assert '%f' % np.float32(0.0078125) == '0.007812' and '%f' % np.float32(0.0234375) == '0.023438'     # ties go to even
    got = R.q(v)
    want = np.array([float('%f' % x) for x in v])
    assert np.array_equal(got, want)
    assert np.array_equal(R.q(ties), np.array([float('%f' % x) for x in ties]))


# --------------------------------------------------------------------------------- restatement against voc_eval itself
def write_detection_files(case, outdir, prefix, num_classes):
    """The lines predict() writes for the kept rows: the same torch arithmetic on fp32 tensors, the same format."""
    os.makedirs(outdir, exist_ok=True)
    fps = [open('%s/%s%s.txt' % (outdir, prefix, c), 'w') for c in R.CLASSES[:num_classes]]
    rows_c, probs_c = torch.from_numpy(case.rows), torch.from_numpy(case.probs)
    emit_c = probs_c > case.conf_thresh
    for b in range(case.rows.shape[0]):
        width, height = case.sizes[b]
        for r in range(int(case.nkept[b])):
            top_c = int(rows_c[b, r, 6])
            cls = [top_c] + [c for c in torch.nonzero(emit_c[b, r]).flatten().tolist() if c != top_c]
            box = rows_c[b, r, :4]
            x1, y1 = (box[0] - box[2] / 2.0) * width, (box[1] - box[3] / 2.0) * height
            x2, y2 = (box[0] + box[2] / 2.0) * width, (box[1] + box[3] / 2.0) * height
            for cls_id in cls:
                fps[cls_id].write('%s %f %f %f %f %f\n' % (IDS[case.first_image + b], probs_c[b, r, cls_id], x1, y1, x2, y2))
    for f in fps:
        f.close()


EXTRA = [("extra000", [(0, 0, (1, 1, 20, 20)), (4, 1, (5, 5, 30, 30)), (7, 0, (2, 2, 9, 9))])]


def test_restatement_equals_voc_eval_through_text_files(tmp_path):
    case = R.craft_case(seed=0)
    NC = 20
    pascal, listfile = R.write_devkit(tmp_path / "kit", IDS, case.sizes, case.gt, extra=EXTRA)
    ev = PASCALVOCEval(None, '', '', None, pascal, listfile, str(tmp_path / "det"), 'det_', str(tmp_path / "pkl"))
    write_detection_files(case, ev.EVAL_OUTPUTDIR, ev.EVAL_PREFIX, NC)
    records = R.emit(case.rows, case.probs, case.nkept, case.conf_thresh, 0, case.sizes)
    assert R.tie_free(records)
    # the arg-max class is emitted even where its probability is at or below the threshold
    for b, r, c in case.forced:
        assert case.probs[b, r, c] <= np.float32(case.conf_thresh) and any(t[0] == c and t[2] == b and t[3] == r for t in records)
    keys, flags, cls = R.match(records, case.gt)
    assert (np.diff(keys) > 0).all()
    npos = R.count_npos(case.gt + [EXTRA[0][1]], NC)
    base = os.path.join(pascal, 'VOC2007')
    interesting = 0
    for c in range(NC):
        rec, prec, ap = ev.voc_eval(os.path.join(ev.EVAL_OUTPUTDIR, 'det_{:s}.txt'), os.path.join(base, 'Annotations', '{:s}.xml'),
                                    os.path.join(base, 'ImageSets', 'Main', 'test.txt'), R.CLASSES[c], ev.EVAL_OUTPUTDIR_PKL,
                                    0.5, True)
        rrec, rprec, rap = R.curves(flags[cls == c], npos[c])
        assert np.array_equal(rec, rrec) and np.array_equal(prec, rprec) and ap == rap, c
        interesting += 0 < ap < 1
    assert interesting >= 3
    # the crafted rows of image 3: IoU exactly 0.5 is an fp; double hits; the doubled object; the difficult one
    by_row = {(int(k >> 56), int(k >> 11) & ((1 << 25) - 1), int(k & 2047)): f for k, f in zip(keys, flags)}
    g, d = np.array([10., 10., 19., 19.]), np.array([10., 10., 19., 14.])
    inters = (min(g[2], d[2]) - max(g[0], d[0]) + 1.) * (min(g[3], d[3]) - max(g[1], d[1]) + 1.)
    assert inters / ((d[2] - d[0] + 1.) * (d[3] - d[1] + 1.) + (g[2] - g[0] + 1.) * (g[3] - g[1] + 1.) - inters) == 0.5
    assert by_row[(0, 3, 0)] == R.FP
    assert sorted(by_row[(0, 3, r)] for r in (1, 2)) == [R.TP, R.FP]
    assert sorted(by_row[(1, 3, r)] for r in (3, 4, 5)) == [R.TP, R.FP, R.FP]
    assert by_row[(2, 3, 6)] == R.NEITHER and by_row[(3, 3, 7)] == R.TP


def test_ties_follow_the_stable_order():
    case = R.craft_case(seed=0, ties=True)
    records = R.emit(case.rows, case.probs, case.nkept, case.conf_thresh, 0, case.sizes)
    assert not R.tie_free(records)
    keys, _, _ = R.match(records, case.gt)
    assert (np.diff(keys) > 0).all()                       # a total order all the same


# ---------------------------------------------------------------------------------------------------------- ground truth
def test_ground_truth_table(tmp_path):
    case = R.craft_case(seed=0)
    pascal, listfile = R.write_devkit(tmp_path / "kit", IDS, case.sizes, case.gt, extra=EXTRA)
    base = os.path.join(pascal, 'VOC2007')
    ev = PASCALVOCEval(None, '', '', None, pascal, listfile, '', '', '')
    files = open(listfile).read().split()
    anno, iset = os.path.join(base, 'Annotations', '{:s}.xml'), os.path.join(base, 'ImageSets', 'Main', 'test.txt')
    gt = VOCGroundTruth(ev.parse_rec, anno, iset, files, R.CLASSES, torch.device("cpu"))
    assert gt.num_images == 4 and gt.max_objects == 64 and gt.ids == IDS
    assert gt.box.dtype == torch.int32 and gt.cls.dtype == torch.uint8 and gt.difficult.dtype == torch.uint8
    assert gt.count.tolist() == [9, 64, 0, 5] and gt.size.tolist() == [list(s) for s in case.sizes]
    for i, objs in enumerate(case.gt):
        for g, (c, d, box) in enumerate(objs):
            assert gt.box[i, g].tolist() == list(box) and int(gt.cls[i, g]) == c and int(gt.difficult[i, g]) == d
    assert np.array_equal(gt.npos.numpy(), R.count_npos(case.gt + [EXTRA[0][1]], 20))        # over the image set
    # an evaluation image that the image set does not list
    with pytest.raises(_lib.McamdError, match="stranger"):
        VOCGroundTruth(ev.parse_rec, anno, iset, files + [os.path.join(base, 'JPEGImages', 'stranger.png')], R.CLASSES, "cpu")
    # 65 objects in one image
    many = [R._grid_objects(None, 500, 375, 64, 20) + [(0, 0, (1, 1, 5, 5))]]
    pascal2, listfile2 = R.write_devkit(tmp_path / "kit2", ["crowd"], [(500, 375)], many)
    base2 = os.path.join(pascal2, 'VOC2007')
    with pytest.raises(_lib.McamdError, match="crowd.*65 objects"):
        VOCGroundTruth(ev.parse_rec, os.path.join(base2, 'Annotations', '{:s}.xml'),
                       os.path.join(base2, 'ImageSets', 'Main', 'test.txt'), open(listfile2).read().split(), R.CLASSES, "cpu")


# ------------------------------------------------------------------------------------------------------------ the library
def test_symbols_are_declared_exported_bound_and_built():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcamd.h")).read(), flags=re.S)
    lib = _lib.lib()
    for name in ("mcamd_voc_match", "mcamd_voc_ap"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct mcamd_voc_match_desc" in hdr
    src = open(os.path.join(ROOT, "modelcompression_amd", "build.py")).read()
    assert re.search(r'"voc_eval\.hip": \["-ffp-contract=off"\]', src)
    assert ops.VOC_MAX_OBJECTS == 64
    assert R.make_key(3, 250000, 5, 7) == (3 << ops.VOC_KEY_CLASS_SHIFT) | (750000 << ops.VOC_KEY_SCORE_SHIFT) | (
        5 << ops.VOC_KEY_IMAGE_SHIFT) | 7


def match_desc(**kw):
    d = _lib.VocMatchDesc()
    for f in ("rows", "probs", "nkept", "gt_box", "gt_cls", "gt_difficult", "gt_count", "image_size", "keys", "flags", "counters"):
        setattr(d, f, P)
    d.B, d.N, d.C, d.G, d.conf_thresh, d.ovthresh, d.first_image, d.capacity = 4, 845, 20, 64, 0.005, 0.5, 0, 1024
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("bad, text", [
    (dict(G=65), "65 ground-truth objects per image, at most 64"),
    (dict(C=81), "81 classes, at most 80"),
    (dict(N=2049), "2049 rows per image, at most 2048"),
    (dict(B=0), "bad shape"),
    (dict(N=0), "bad shape"),
    (dict(G=0), "bad shape"),
    (dict(capacity=0), "capacity 0"),
    (dict(first_image=-1), "the key holds 25 bits"),
    (dict(first_image=(1 << 25) - 3), "the key holds 25 bits"),
] + [({f: None}, "null argument") for f in ("rows", "probs", "nkept", "gt_box", "gt_cls", "gt_difficult", "gt_count",
                                            "image_size", "keys", "flags", "counters")])
def test_voc_match_refuses_bad_arguments(bad, text):
    assert _lib.lib().mcamd_voc_match(C.byref(match_desc(**bad)), None) == -1
    assert text in err() and err().startswith("voc_match:"), err()


def test_voc_match_refuses_a_null_descriptor():
    assert _lib.lib().mcamd_voc_match(None, None) == -1 and "voc_match: null argument" in err()


def test_voc_ap_refuses_bad_arguments():
    lib = _lib.lib()
    good = [P, P, P, 1024, P, 20, P, None, None, None]
    for i in (0, 1, 2, 4, 6):
        args = list(good)
        args[i] = None
        assert lib.mcamd_voc_ap(*args) == -1 and "voc_ap: null argument" in err()
    for i, v, text in ((5, 81, "81 classes, at most 80"), (5, 0, "bad shape"), (3, 0, "capacity 0")):
        args = list(good)
        args[i] = v
        assert lib.mcamd_voc_ap(*args) == -1 and text in err(), err()


def test_wrappers_have_no_cpu_path(tmp_path):
    z = torch.zeros
    with pytest.raises(_lib.McamdError):
        ops.voc_match(z(1, 4, 8), z(1, 4, 20), z(1, dtype=torch.int32), 0.005, 0.5, 0, z(1, 1, 4, dtype=torch.int32),
                      z(1, 1, dtype=torch.uint8), z(1, 1, dtype=torch.uint8), z(1, dtype=torch.int32), z(1, 2, dtype=torch.int32),
                      z(8, dtype=torch.int64), z(8, dtype=torch.uint8), z(2, dtype=torch.int64))
    with pytest.raises(_lib.McamdError):
        ops.voc_ap(z(8, dtype=torch.int64), z(8, dtype=torch.uint8), z(2, dtype=torch.int64), z(20, dtype=torch.int32))
    case = R.craft_case(seed=0)
    pascal, listfile = R.write_devkit(tmp_path / "kit", IDS, case.sizes, case.gt)
    base = os.path.join(pascal, 'VOC2007')
    ev = PASCALVOCEval(None, '', '', None, pascal, listfile, '', '', '')
    gt = VOCGroundTruth(ev.parse_rec, os.path.join(base, 'Annotations', '{:s}.xml'),
                        os.path.join(base, 'ImageSets', 'Main', 'test.txt'), open(listfile).read().split(), R.CLASSES, "cpu")
    acc = DeviceVOCEval(gt, 20, capacity=64)
    with pytest.raises(_lib.McamdError):
        acc.add(torch.from_numpy(case.rows), torch.from_numpy(case.probs), torch.from_numpy(case.nkept), 0, 0.005)


def test_predict_device_eval_refuses_what_it_cannot_do(tmp_path):
    from modelcompression_amd import nets
    model = nets.Darknet(os.path.join(ROOT, "tests", "golden", "mini.cfg"))
    case = R.craft_case(seed=0)
    pascal, listfile = R.write_devkit(tmp_path / "kit", IDS, case.sizes, case.gt)
    ev = PASCALVOCEval(model, '', '', None, pascal, '', str(tmp_path / "d"), 'det_', str(tmp_path / "p"))
    with pytest.raises(_lib.McamdError, match="image list"):
        ev.predict(DEVICE_EVAL=True)
    ev = PASCALVOCEval(model, '', '', None, str(tmp_path / "nowhere"), listfile, str(tmp_path / "d"), 'det_', str(tmp_path / "p"))
    with pytest.raises(_lib.McamdError, match="annotations"):
        ev.predict(DEVICE_EVAL=True)
    ev = PASCALVOCEval(model, '', '', None, pascal, listfile, str(tmp_path / "d"), 'det_', str(tmp_path / "p"))
    with pytest.raises(_lib.McamdError, match="on the GPU"):
        ev.predict(DEVICE_EVAL=True)                       # the model is on the CPU
