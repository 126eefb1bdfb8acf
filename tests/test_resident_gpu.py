"""Device-resident pictures on the GPU, every comparison bit for bit: mcamd_augment_tables against augment.resample_table
and augment.point_luts, the resident batches against the packed path and the reference's recorded output, the resize-only
descriptor (lut_off = -1) against Image.resize, the resident loaders against VOCList / VOCAugment, and the RESIDENT
switches of predict() and train() on a generated devkit."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import voc_eval_ref as R  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
from modelcompression_amd import _lib, nets, nets2_utils as U  # noqa: E402
from modelcompression_amd import augment as A  # noqa: E402
from modelcompression_amd.data import ResidentAugment, ResidentImages, ResidentList, VOCAugment, VOCList, label_path_for, read_boxes  # noqa: E402
from modelcompression_amd.predict import PASCALVOCEval  # noqa: E402
from modelcompression_amd.train import YOLOv2Train  # noqa: E402
from test_augment_cpu import load_cases, reference_output  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "golden", "mini.cfg")


def to_tensor(u8):
    return torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).float().div(255)


# -------------------------------------------------------------------------------------------------------------- tables
def device_tables(dev, crops, shape, hsv=None):
    """mcamd_augment_tables for descriptors of the given (crop_w, crop_h) -> (descriptors, int32 coef, uint8 luts)."""
    W, H = shape
    B = len(crops)
    descs = (_lib.AugmentDesc * B)()
    n = 0
    for b, (cw, ch) in enumerate(crops):
        d = descs[b]
        d.crop_w, d.crop_h = cw, ch
        d.hk, d.hcoef_off = A.table_taps(cw, W), n
        n += W * (d.hk + 2)
        d.vk, d.vcoef_off = A.table_taps(ch, H), n
        n += H * (d.vk + 2)
        d.lut_off = 768 * b if hsv is not None else -1
    host = torch.empty(C.sizeof(descs), dtype=torch.uint8)
    C.memmove(host.data_ptr(), descs, C.sizeof(descs))
    guard = 64
    coef = torch.full((n + guard,), -7, dtype=torch.int32, device=dev)
    lut = torch.full((768 * B + guard,), 0xAB, dtype=torch.uint8, device=dev)
    hsv_dev = torch.tensor(hsv, dtype=torch.float64, device=dev).reshape(B, 3) if hsv is not None else None
    desc_dev = host.to(dev)
    _lib.check(_lib.lib().mcamd_augment_tables(C.addressof(descs), desc_dev.data_ptr(), _lib.ptr(hsv_dev), B, H, W,
                                               coef.data_ptr(), n, lut.data_ptr() if hsv is not None else None,
                                               768 * B if hsv is not None else 0, _lib.stream_ptr()), "mcamd_augment_tables")
    torch.cuda.synchronize()
    assert (coef[n:] == -7).all() and (lut[768 * B:] == 0xAB).all()          # nothing past the extents
    return descs, coef[:n].cpu().numpy(), lut[:768 * B].cpu().numpy().reshape(B, 3, 256)


PAIRS = [(5, 5), (1, 13), (2, 32), (37, 64), (53, 48), (333, 64), (1600, 416), (2000, 13)]


@pytest.mark.parametrize("n_in, n_out", PAIRS)
def test_device_tables_equal_resample_table(dev, n_in, n_out):
    """Horizontal n_in -> n_out and, in the same image, vertical n_in -> n_out + 3 (a different table)."""
    descs, coef, _ = device_tables(dev, [(n_in, n_in)], (n_out, n_out + 3))
    d = descs[0]
    for off, k, out in ((d.hcoef_off, d.hk, n_out), (d.vcoef_off, d.vk, n_out + 3)):
        ksize, want = A.resample_table(n_in, out)
        assert ksize == k
        got = coef[off:off + out * (k + 2)].reshape(out, k + 2)
        assert got.tobytes() == want.tobytes(), (n_in, out, int((got != want).sum()))


def test_device_tables_of_one_batch_with_a_different_ksize_per_image(dev):
    crops = [(64, 48), (37, 53), (333, 250), (1, 2), (1600, 1200), (48, 64)]
    W, H = 64, 48
    descs, coef, _ = device_tables(dev, crops, (W, H))
    assert len({d.hk for d in descs}) >= 4 and descs[0].hk == descs[0].vk == 1
    for d, (cw, ch) in zip(descs, crops):
        for off, k, n_in, out in ((d.hcoef_off, d.hk, cw, W), (d.vcoef_off, d.vk, ch, H)):
            want = A.resample_table(n_in, out)[1]
            assert coef[off:off + out * (k + 2)].tobytes() == want.tobytes(), (cw, ch, n_in, out)


def test_device_luts_equal_point_luts(dev):
    hsv = [(h, s, e) for h in (-0.5, -0.1, 0, 0.1, 0.5) for s in (1 / 1.5, 1, 1.5) for e in (1 / 1.5, 1, 1.5)]
    for seed in range(16):
        p = A.draw_params(random.Random(100 + seed), 500, 375)
        hsv.append((p.dhue, p.dsat, p.dexp))
    _, _, luts = device_tables(dev, [(8, 8)] * len(hsv), (8, 8), hsv)
    for got, (h, s, e) in zip(luts, hsv):
        want = A.point_luts(h, s, e)
        assert np.array_equal(got, want), (h, s, e, int((got != want).sum()))


# -------------------------------------------------------------------------------------------------------- augmentation
SIZES = [(24, 31), (333, 250), (37, 53), (200, 150), (64, 48), (101, 77), (250, 333), (48, 64)]      # (w, h)
SHAPE = (64, 48)


def ragged_set():
    sources = [A.synthetic_source(w, h, 3 * i + 2) for i, (w, h) in enumerate(SIZES)]
    params = [A.draw_params(random.Random(40 + i), w, h) for i, (w, h) in enumerate(SIZES)]
    assert {p.flip for p in params} == {0, 1}
    assert any(p.pleft < 0 or p.ptop < 0 for p in params)                                   # crops that start outside
    assert any(p.pleft + p.swidth - 1 > w or p.ptop + p.sheight - 1 > h for p, (w, h) in zip(params, SIZES))
    return sources, params


def test_resident_batches_equal_the_packed_path(dev):
    sources, params = ragged_set()
    order = [5, 0, 7, 2, 1, 6, 3, 4]
    res = ResidentImages.from_sources(sources, dev)
    before = res.buf.clone()
    want, _ = A.DeviceAugmenter(SHAPE, dev)(A.pack_batch([sources[i] for i in order], [params[i] for i in order], SHAPE))
    aug = A.DeviceAugmenter(SHAPE, dev, res)
    host, _ = aug(A.pack_resident(res, order, [params[i] for i in order], SHAPE, device_tables=False))
    assert torch.equal(host, want)
    pb = A.pack_resident(res, order, [params[i] for i in order], SHAPE).pin_memory()
    device, _ = aug(pb)
    assert torch.equal(device, want)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                  # the warmed call: no blocking copy, no host synchronisation
    try:
        again, target = aug(pb)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again, want) and target.shape == (8, 250)
    assert torch.equal(res.buf, before)                      # the resident pictures are only read
    for i in range(len(sources)):
        assert np.array_equal(res.source(i), sources[i])


def test_resident_fixture_cases_equal_the_reference_output(dev):
    cases = [c for c in load_cases() if c["shape"] == (416, 416)]
    assert cases
    res = ResidentImages.from_sources([c["src"] for c in cases], dev)
    x, _ = A.DeviceAugmenter((416, 416), dev, res)(A.pack_resident(res, range(len(cases)), [c["params"] for c in cases], (416, 416)))
    x = x.cpu()
    for b, c in enumerate(cases):
        assert torch.equal(x[b], to_tensor(reference_output(c))), c["name"]


# --------------------------------------------------------------------------------------------------------- resize only
@pytest.mark.parametrize("shape", [(64, 48), (416, 416)])
def test_resize_only_equals_image_resize(dev, shape):
    Image = pytest.importorskip("PIL.Image")
    sizes = [(64, 48), (37, 53), (200, 150), (500, 375)]
    sources = [A.synthetic_source(w, h, 11 + i) for i, (w, h) in enumerate(sizes)]
    res = ResidentImages.from_sources(sources, dev)
    pb = A.pack_resident(res, range(4), [A.resize_params(w, h) for w, h in sizes], shape, distort=False)
    x, _ = A.DeviceAugmenter(shape, dev, res)(pb)
    x = x.cpu().numpy()
    for b, src in enumerate(sources):
        want = np.asarray(Image.fromarray(src).resize(shape), np.float32).transpose(2, 0, 1) / 255.0
        assert x[b].shape == want.shape and np.array_equal(x[b], want), (sizes[b], shape, int((x[b] != want).sum()))


# ------------------------------------------------------------------------------------------------------------- loaders
def write_list(root, n=12):
    Image = pytest.importorskip("PIL.Image")
    imgdir, labdir = root / "JPEGImages", root / "labels"
    imgdir.mkdir()
    labdir.mkdir()
    lines = []
    for i in range(n):
        path = imgdir / ("%03d.png" % i)
        Image.fromarray(A.synthetic_source(40 + 13 * i, 90 - 5 * i, i)).save(path)
        if i != 3:                                           # one picture without a label file
            np.savetxt(labdir / ("%03d.txt" % i), [[i % 20, 0.5, 0.5, 0.3, 0.4], [1, 0.2, 0.7, 0.1, 0.2]][:1 + i % 2])
        lines.append(str(path))
    listfile = root / "list.txt"
    listfile.write_text("\n".join(lines) + "\n")
    return str(listfile), lines


def test_resident_loaders_equal_the_file_loaders(dev, tmp_path):
    listfile, lines = write_list(tmp_path)
    labels = [label_path_for(p) for p in lines]
    res = ResidentImages(lines, dev, num_workers=2)
    aug = A.DeviceAugmenter(SHAPE, dev, res)

    def batches(ds, collate_fn):
        return list(torch.utils.data.DataLoader(ds, batch_size=5, shuffle=False, num_workers=0, collate_fn=collate_fn))

    rl = ResidentList(res, labels, SHAPE)
    got = [aug(b) for b in batches(rl, rl.collate)]
    want = batches(VOCList(listfile, shape=SHAPE), None)
    assert [len(x) for x, _ in got] == [5, 5, 2]
    for (x, t), (wx, wt) in zip(got, want):
        assert torch.equal(x.cpu(), wx) and torch.equal(t.cpu(), wt)
    ra = ResidentAugment(res, [read_boxes(lp) for lp in labels], SHAPE, seed=4)
    va = VOCAugment(listfile, SHAPE, seed=4)
    plain = A.DeviceAugmenter(SHAPE, dev)
    seen = []
    for epoch in (0, 1):
        ra.set_epoch(epoch)
        va.set_epoch(epoch)
        for b, wb in zip(batches(ra, ra.collate), batches(va, A.collate_fn(SHAPE))):
            (x, t), (wx, wt) = aug(b), plain(wb)
            assert torch.equal(x, wx) and torch.equal(t, wt), epoch
            seen.append(x)
    assert not torch.equal(seen[0], seen[3])                 # epoch 1 draws other parameters


# -------------------------------------------------------------------------------------------------------- entry points
@pytest.fixture(scope="module")
def devkit(dev, tmp_path_factory):
    """A model whose logits spread, 8 pictures, ground truth from its own detections (as test_voc_eval_gpu builds it)."""
    root = tmp_path_factory.mktemp("kit")
    state = O.init_state(O.parse_cfg(MINI), seed=1)
    last = [k for k in state if k.endswith("weight") and state[k].dim() == 4][-1]
    state[last] = state[last] * 2.0
    model = nets.Darknet(MINI)
    model.load_state_dict(state)
    model = model.to(dev).eval()
    images, sizes = R.make_images(1, 8)
    ids = ["pic%03d" % i for i in range(8)]
    pascal, listfile = R.write_devkit(root, ids, sizes, [[]] * 8, images=images)
    ds = VOCList(listfile, shape=(model.width, model.height), train=False)
    with torch.no_grad():
        x = torch.stack([ds[i][0] for i in range(8)]).to(dev)
        rows, probs, nkept = (t.cpu().numpy() for t in U.detections_device(model(x), 0.25, 0.45, model.num_classes,
                                                                           model.anchors, model.num_anchors))
    R.write_devkit(root, ids, sizes, R.ground_truth_from_detections(rows, probs, nkept, sizes, 1), images=images)
    return model, pascal, listfile, root


def test_predict_resident_equals_predict_from_files(dev, devkit):
    model, pascal, listfile, root = devkit

    def ev(name):
        return PASCALVOCEval(model, MINI, '', None, pascal, listfile, str(root / name), 'det_', str(root / (name + "_pkl")))
    a, b = ev("dev_files"), ev("dev_resident")
    mAP = a.predict(3, 0.005, 0.45, DEVICE_EVAL=True)
    assert b.predict(3, 0.005, 0.45, DEVICE_EVAL=True, RESIDENT=True) == mAP
    assert np.array_equal(a.aps, b.aps) and a.num_detections == b.num_detections and (a.aps > 0).any()
    resident = b._resident
    assert b.predict(3, 0.005, 0.45, DEVICE_EVAL=True, RESIDENT=True) == mAP and b._resident is resident      # built once
    f, g = ev("files"), ev("resident")
    f.predict(3, 0.005, 0.45)
    g.predict(3, 0.005, 0.45, RESIDENT=resident)             # a set built before
    assert g.num_detections == f.num_detections > 0 and np.array_equal(f.aps, g.aps)
    for c in R.CLASSES:
        name = 'det_%s.txt' % c
        assert open(os.path.join(f.EVAL_OUTPUTDIR, name), 'rb').read() == open(os.path.join(g.EVAL_OUTPUTDIR, name), 'rb').read(), c
    short = ResidentImages.from_sources([resident.source(0)], dev)
    with pytest.raises(_lib.McamdError, match="1 resident pictures, 8 lines"):
        ev("short").predict(3, 0.005, 0.45, RESIDENT=short)


def test_train_resident_with_augment(dev, tmp_path, capsys):
    listfile, _ = write_list(tmp_path)
    model = YOLOv2Train().train('', listfile, '', '', '', '', 'p_', MINI, '', 4, 10,
                                AUGMENT=True, RESIDENT=True, DEBUG_EPOCHS=1, MAX_EPOCHS=1)
    out = capsys.readouterr().out
    assert "12 pictures resident" in out
    loss = float([l for l in out.splitlines() if "mean loss" in l][-1].split("mean loss")[1])
    assert np.isfinite(loss) and all(torch.isfinite(p).all() for p in model.parameters())
