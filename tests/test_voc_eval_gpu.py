"""csrc/voc_eval.hip on the device, exactly: mcamd_voc_match's keys and flags against the numpy restatement of the contract
(tests/voc_eval_ref.py, itself held to PASCALVOCEval.voc_eval by test_voc_eval_cpu.py), mcamd_voc_ap's rec / prec / ap
against voc_eval's last lines and voc_ap, and predict(DEVICE_EVAL=True) against the file path on a generated devkit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import voc_eval_ref as R  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from modelcompression_amd import _lib, nets, nets2_utils as U  # noqa: E402
from modelcompression_amd.data import VOCList  # noqa: E402
from modelcompression_amd.predict import PASCALVOCEval  # noqa: E402
from modelcompression_amd.voc_eval import VOCGroundTruth, DeviceVOCEval  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "golden", "mini.cfg")
NC = 20


def ground_truth(root, ids, sizes, gt, dev, images=None):
    pascal, listfile = R.write_devkit(root, ids, sizes, gt, images=images)
    base = os.path.join(pascal, 'VOC2007')
    ev = PASCALVOCEval(None, '', '', None, pascal, listfile, '', '', '')
    return VOCGroundTruth(ev.parse_rec, os.path.join(base, 'Annotations', '{:s}.xml'),
                          os.path.join(base, 'ImageSets', 'Main', 'test.txt'), open(listfile).read().split(), R.CLASSES[:NC], dev)


_REF = {}


def reference(ties):
    """ties -> (case, keys, flags, class of every record) of the crafted case; computed once."""
    if ties not in _REF:
        case = R.craft_case(seed=0, ties=ties)
        records = R.emit(case.rows, case.probs, case.nkept, case.conf_thresh, 0, case.sizes)
        assert R.tie_free(records) != ties
        _REF[ties] = (case,) + R.match(records, case.gt)
    return _REF[ties]


@pytest.fixture(scope="module")
def crafted_gt(dev, tmp_path_factory):
    case = reference(False)[0]
    return ground_truth(tmp_path_factory.mktemp("kit"), ["img%06d" % i for i in range(4)], case.sizes, case.gt, dev)


def add_case(acc, case, dev, batches=((0, 4),)):
    for lo, hi in batches:
        acc.add(torch.from_numpy(case.rows[lo:hi]).to(dev), torch.from_numpy(case.probs[lo:hi]).to(dev),
                torch.from_numpy(case.nkept[lo:hi]).to(dev), lo, case.conf_thresh)


# --------------------------------------------------------------------------------------------------------------- match
@pytest.mark.parametrize("ties, batches", [(False, ((0, 4),)), (True, ((0, 4),)), (True, ((2, 4), (0, 1), (1, 2)))])
def test_match_keys_and_flags_equal_the_restatement(dev, crafted_gt, ties, batches):
    """B = 4, N = 256: nkept 0 and N, rows beyond nkept poisoned (NaN, 1e30), 64 objects and none, difficult and doubled
    objects, double hits, IoU exactly 0.5, a forced arg-max class below the threshold; with `ties`, scores that tie after
    q() within and across images (in any batch order: the key is a total order)."""
    case, keys, flags, _ = reference(ties)
    assert crafted_gt.max_objects == 64 and crafted_gt.count.tolist() == [9, 64, 0, 5]
    assert case.nkept.tolist() == [0, 256, 40, 64] and np.isnan(case.rows[0]).all() and (case.probs[2, 40:] == 1e30).all()
    acc = DeviceVOCEval(crafted_gt, NC, capacity=1 << 14)
    add_case(acc, case, dev, batches)
    got_keys, got_flags = acc.records()
    assert acc.counters.tolist() == [len(keys), 0]
    assert np.array_equal(got_keys, keys)
    assert np.array_equal(got_flags, flags)
    assert set(flags.tolist()) == {R.NEITHER, R.TP, R.FP}
    # IoU exactly 0.5 (test_voc_eval_cpu confirms the value): row 0 of image 3, class 0, is an fp
    at = {(int(k >> 56), int(k >> 11) & ((1 << 25) - 1), int(k & 2047)): f for k, f in zip(got_keys, got_flags)}
    assert at[(0, 3, 0)] == R.FP
    for b, r, c in case.forced:
        assert (c, b, r) in at and case.probs[b, r, c] <= np.float32(case.conf_thresh)


def test_match_sorts_2048_rows_of_one_class(dev, tmp_path):
    """The capacity of the in-wave sort: B = 1, N = nkept = 2048, every row emitted in class 0 (and only there)."""
    rng = np.random.RandomState(3)
    N = 2048
    gt = [[(0, int(j % 5 == 4), (40 * j + 3, 30 * (j % 7) + 2, 40 * j + 33, 30 * (j % 7) + 28)) for j in range(12)]]
    rows, probs = np.zeros((1, N, 8), dtype=np.float32), np.zeros((1, N, NC), dtype=np.float32)
    probs[0, :, 0] = (rng.permutation(900000)[:N] + 50000) / 1e6
    probs[0, ::9, 0] = probs[0, 5, 0]                         # and a long run of equal scores: ordered by row
    probs[0, :, 1:] = 0.001
    for r in range(N):
        _, _, box = gt[0][rng.randint(12)]
        rows[0, r, :4] = R._row_for(np.array(box) + rng.uniform(-8, 8, 4), 500, 375)
    rows[0, :, 4], rows[0, :, 5], rows[0, :, 7] = 0.9, probs[0, :, 0], np.arange(N)
    nkept = np.array([N], dtype=np.int32)
    table = ground_truth(tmp_path / "kit", ["one"], [(500, 375)], gt, dev)
    acc = DeviceVOCEval(table, NC, capacity=4096)
    acc.add(torch.from_numpy(rows).to(dev), torch.from_numpy(probs).to(dev), torch.from_numpy(nkept).to(dev), 0, 0.005)
    keys, flags, _ = R.match(R.emit(rows, probs, nkept, 0.005, 0, [(500, 375)]), gt)
    assert len(keys) == N
    got_keys, got_flags = acc.records()
    assert np.array_equal(got_keys, keys) and np.array_equal(got_flags, flags)
    assert (flags == R.TP).sum() == 10 and (flags == R.NEITHER).sum() > 0       # ten objects are not difficult


def test_overflow_is_counted_and_nothing_is_written_past_the_buffer(dev, crafted_gt):
    case, keys, _, _ = reference(False)
    cap, guard = 1000, 4096
    assert len(keys) > cap + 100
    acc = DeviceVOCEval(crafted_gt, NC, capacity=cap)
    big_keys = torch.full((cap + guard,), -7, dtype=torch.int64, device=dev)
    big_flags = torch.full((cap + guard,), 0xAB, dtype=torch.uint8, device=dev)
    big_keys[:cap], big_flags[:cap] = acc.keys, acc.flags
    acc.keys, acc.flags = big_keys[:cap], big_flags[:cap]
    add_case(acc, case, dev)
    torch.cuda.synchronize()
    assert (big_keys[cap:] == -7).all() and (big_flags[cap:] == 0xAB).all()
    assert acc.counters.tolist() == [len(keys), len(keys) - cap]
    assert set(big_keys[:cap].tolist()) <= set(keys.tolist())            # what was written is whole records
    with pytest.raises(_lib.McamdError, match="capacity of 1000"):
        acc.finish()


# ------------------------------------------------------------------------------------------------------------------ ap
@pytest.mark.parametrize("ties", [False, True])
def test_ap_rec_and_prec_equal_voc_eval(dev, crafted_gt, ties):
    """Per class against voc_eval's last lines and voc_ap; class 19 has no records, classes 5 .. 18 have npos = 0."""
    case, keys, flags, cls = reference(ties)
    npos = R.count_npos(case.gt, NC)
    assert np.array_equal(crafted_gt.npos.cpu().numpy(), npos) and (npos[5:] == 0).all() and (cls != 19).all() and (cls == 18).any()
    acc = DeviceVOCEval(crafted_gt, NC, capacity=1 << 14)
    add_case(acc, case, dev)
    aps, mAP = acc.finish()
    assert aps.dtype == np.float64 and acc.num_records == len(keys)
    want = [R.curves(flags[cls == c], npos[c]) for c in range(NC)]
    for c in range(NC):
        rec, prec = acc.curves(c) if c in (0, 1, 4, 18, 19) else (None, None)
        if rec is not None:
            assert np.array_equal(rec, want[c][0]) and np.array_equal(prec, want[c][1]), c
        assert aps[c] == want[c][2], c
    assert mAP == float(np.mean([w[2] for w in want]))
    assert aps[19] == 0.0 and sum(0 < a < 1 for a in aps) >= 3


def test_add_makes_no_host_synchronisation(dev, crafted_gt):
    case = reference(False)[0]
    acc = DeviceVOCEval(crafted_gt, NC, capacity=1 << 14)
    rows, probs, nkept = (torch.from_numpy(a).to(dev) for a in (case.rows, case.probs, case.nkept))
    acc.add(rows, probs, nkept, 0, case.conf_thresh)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        acc.add(rows[2:], probs[2:], nkept[2:], 2, case.conf_thresh)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert acc.counters[0].item() > 0


# ---------------------------------------------------------------------------------------------------------- end to end
SEED, GAIN = 1, 2.0      # chosen on the CPU (oracle logits): eight classes with 0 < AP < 1, no tied scores


def test_predict_device_eval_equals_the_file_path(dev, tmp_path):
    blocks = O.parse_cfg(MINI)
    state = O.init_state(blocks, seed=SEED)
    last = [k for k in state if k.endswith("weight") and state[k].dim() == 4][-1]
    state[last] = state[last] * GAIN                       # spread the logits: detections above 0.25 in most images
    model = nets.Darknet(MINI)
    model.load_state_dict(state)
    model = model.to(dev).eval()
    images, sizes = R.make_images(SEED, 16)
    ids = ["pic%03d" % i for i in range(16)]
    pascal, listfile = R.write_devkit(tmp_path / "kit", ids, sizes, [[]] * 16, images=images)
    # ground truth from the model's own detections at 0.25, in the batches predict() forms
    ds = VOCList(listfile, shape=(model.width, model.height), train=False)
    parts = []
    with torch.no_grad():
        for lo in range(0, 16, 4):
            x = torch.stack([ds[i][0] for i in range(lo, lo + 4)]).to(dev)
            parts.append(U.detections_device(model(x), 0.25, 0.45, model.num_classes, model.anchors, model.num_anchors))
    rows, probs, nkept = (torch.cat([p[i] for p in parts]).cpu().numpy() for i in range(3))
    gt = R.ground_truth_from_detections(rows, probs, nkept, sizes, SEED)
    R.write_devkit(tmp_path / "kit", ids, sizes, gt, images=images)
    print("kept per image", nkept.tolist(), "objects per image", [len(g) for g in gt])

    ev = PASCALVOCEval(model, MINI, '', None, pascal, listfile, str(tmp_path / "det"), 'det_', str(tmp_path / "pkl"))
    ev.fused = True
    mAP_file = ev.predict(BATCH_SIZE=4, CONF_THRESH=0.25, NMS_THRESH=0.45)
    aps_file = ev.aps.copy()
    for c in R.CLASSES:                                    # the file leg has no tied scores within a class
        scores = [line.split()[1] for line in open(os.path.join(ev.EVAL_OUTPUTDIR, 'det_%s.txt' % c))]
        assert len(set(scores)) == len(scores), c
    ev2 = PASCALVOCEval(model, MINI, '', None, pascal, listfile, str(tmp_path / "det2"), 'det_', str(tmp_path / "pkl2"))
    mAP_dev = ev2.predict(BATCH_SIZE=4, CONF_THRESH=0.25, NMS_THRESH=0.45, DEVICE_EVAL=True)
    print("file path", aps_file.tolist(), mAP_file)
    print("device   ", ev2.aps.tolist(), mAP_dev)
    assert not os.path.exists(ev2.EVAL_OUTPUTDIR)          # no detection files
    assert ev2.num_detections == ev.num_detections
    assert ev2.aps.dtype == np.float64 and np.array_equal(ev2.aps, aps_file)
    assert mAP_dev == mAP_file == ev2.mAP
    assert sum(0 < a < 1 for a in aps_file) >= 3
