"""Host side of the training augmentation (modelcompression_amd/augment.py) against the reference's own
data_augmentation / fill_truth_detection, recorded in tests/golden/augment_cases.npz (gen_augment_golden.py)."""
import ctypes as C
import hashlib
import os
import random

import numpy as np
import pytest
import torch

from modelcompression_amd import _lib
from modelcompression_amd import augment as A
from modelcompression_amd.data import SyntheticAugment
import augment_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def load_cases():
    z = np.load(os.path.join(HERE, "golden", "augment_cases.npz"))
    cases = []
    for ci, name in enumerate(z["names"]):
        kind, w, h, syn_seed, W, H, jitter, hue, sat, exp, seed = z["c%d_meta" % ci]
        src = z["src_jpg"] if kind == 0 else A.synthetic_source(int(w), int(h), int(syn_seed))
        assert src.shape == (int(h), int(w), 3)
        p = A.draw_params(random.Random(int(seed)), int(w), int(h), jitter, hue, sat, exp)
        cases.append(dict(name=str(name), src=src, shape=(int(W), int(H)), params=p, draws=z["c%d_draws" % ci],
                          ret=z["c%d_ret" % ci], out_sha256=str(z["c%d_out_sha256" % ci]),
                          out_shape=tuple(int(v) for v in z["c%d_out_shape" % ci]), boxes=z["c%d_boxes" % ci],
                          label=z["c%d_label" % ci], pil=str(z["pil_version"])))
    return cases


def sha256(u8):
    return hashlib.sha256(np.ascontiguousarray(u8).tobytes()).hexdigest()


def reference_output(c):
    """The reference's uint8 output of fixture case c: the numpy restatement, held to the digest of the reference's
    PIL output that the fixture stores (the pixels themselves are not stored)."""
    out = R.augment(c["src"], c["params"], c["shape"])
    assert out.shape == c["out_shape"] and sha256(out) == c["out_sha256"], c["name"]
    return out


def test_draw_params_reproduce_the_reference_draws():
    for c in load_cases():
        p, d = c["params"], c["draws"]
        assert (p.pleft, p.pright, p.ptop, p.pbot) == tuple(int(v) for v in d[:4]), c["name"]
        assert p.flip == int(d[4]) % 2 and p.dhue == d[5], c["name"]
        assert p.dsat == (d[6] if int(d[7]) % 2 else 1. / d[6]), c["name"]
        assert p.dexp == (d[8] if int(d[9]) % 2 else 1. / d[8]), c["name"]
        assert (p.flip, p.dx, p.dy, p.sx, p.sy) == tuple(c["ret"]), c["name"]


def test_transform_labels_equal_the_reference_labels():
    kept = []
    for c in load_cases():
        got = A.transform_labels(c["boxes"], c["params"])
        ref = torch.from_numpy(c["label"]).float()
        assert got.dtype == torch.float32 and got.shape == (250,)
        assert torch.equal(got, ref), c["name"]
        kept.append(int((ref.view(50, 5)[:, 3] > 0).sum()))
    assert max(kept) == 50                      # the 60-box file is capped
    assert min(kept) < 13                       # boxes cut below 0.001 are dropped


def test_numpy_restatement_reproduces_the_reference_outputs():
    """The yardstick of the GPU test, checked here against the reference's PIL output of every fixture case."""
    for c in load_cases():
        reference_output(c)


def test_resample_tables_match_pillow_resize():
    Image = pytest.importorskip("PIL.Image")
    g = np.random.default_rng(0)
    sizes = [(500, 375, 416, 416), (37, 53, 416, 416), (1600, 1200, 480, 352), (2, 2, 416, 416), (417, 300, 416, 416),
             (1, 1, 8, 8), (300, 7, 20, 3)]
    sizes += [tuple(int(v) for v in g.integers(2, 700, 4)) for _ in range(8)]
    for w, h, W, H in sizes:
        src = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(R.resize(src, W, H), np.asarray(Image.fromarray(src).resize((W, H)))), (w, h, W, H)


def test_point_luts_equal_image_point_of_the_reference_functions():
    Image = pytest.importorskip("PIL.Image")
    ramp = Image.frombytes("L", (256, 1), bytes(range(256)))
    rng = random.Random(3)
    for n in range(60):
        hue = [0.5, -0.5, 127.5 / 255, -127.5 / 255][n] if n < 4 else rng.uniform(-0.5, 0.5)
        sat, val = rng.uniform(0.2, 3.0), rng.uniform(0.2, 3.0)

        def change_hue(x):                          # dataloader.py:120-126
            x += hue * 255
            if x > 255:
                x -= 255
            if x < 0:
                x += 255
            return x
        ref = [np.asarray(ramp.point(f)).reshape(-1) for f in (change_hue, lambda i: i * sat, lambda i: i * val)]
        assert np.array_equal(A.point_luts(hue, sat, val), np.stack(ref)), (hue, sat, val)


def all_colours():
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_hsv_restatement_matches_pil_on_every_colour():
    Image = pytest.importorskip("PIL.Image")
    rgb = all_colours()
    luts = np.random.default_rng(7).integers(0, 256, (3, 256), dtype=np.uint8)
    hsv = Image.fromarray(rgb).convert("HSV")
    assert np.array_equal(R.rgb2hsv(rgb), np.asarray(hsv))
    chans = [ch.point([int(v) for v in lut]) for ch, lut in zip(hsv.split(), luts)]
    ref = np.asarray(Image.merge("HSV", chans).convert("RGB"))
    assert np.array_equal(R.distort(rgb, luts), ref)


def _params_of(items):
    return [p for _, _, p in items]


@pytest.mark.parametrize("epoch", [0, 3])
def test_parameters_depend_only_on_seed_epoch_index(epoch):
    ds = SyntheticAugment(12, shape=(96, 64), seed=5)
    ds.set_epoch(epoch)
    runs = []
    for workers in (0, 2):
        loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=workers, collate_fn=_params_of)
        runs.append([p for batch in loader for p in batch])
    assert runs[0] == runs[1]
    assert runs[0] == [ds[i][2] for i in range(12)]
    other = SyntheticAugment(12, shape=(96, 64), seed=5)
    other.set_epoch(epoch + 1)
    assert [other[i][2] for i in range(12)] != runs[0]


def _call(descs, B=1, H=8, W=8, src_bytes=1 << 20, coef_elems=1 << 20, lut_bytes=768, tmp_bytes=1 << 20, null_out=False):
    fake = 1 << 40                                   # never dereferenced: every case below fails validation first
    bt = _lib.AugmentBatch(desc=C.addressof(descs), desc_dev=fake, src=fake, src_bytes=src_bytes, coef=fake,
                           coef_elems=coef_elems, lut=fake, lut_bytes=lut_bytes, tmp=fake, tmp_bytes=tmp_bytes,
                           out=None if null_out else fake, B=B, H=H, W=W)
    return _lib.lib().mcamd_augment(C.byref(bt), None)


def test_augment_validates_arguments_without_launching():
    def desc(**kw):
        d = (_lib.AugmentDesc * 1)()
        f = dict(src_w=10, src_h=10, crop_w=9, crop_h=9, hk=5, vk=5, hcoef_off=0, vcoef_off=100)
        f.update(kw)
        for k, v in f.items():
            setattr(d[0], k, v)
        return d
    # the reference's crop of a swidth = 1 image is an image of no pixels (PIL then fails to resize it): rejected here
    for bad in (dict(crop_w=0), dict(crop_h=0), dict(crop_w=-3), dict(src_w=0), dict(hk=0), dict(lut_off=1),
                dict(hcoef_off=1 << 20), dict(vcoef_off=-1), dict(src_off=(1 << 20) - 10), dict(tmp_off=1 << 20)):
        rc = _call(desc(**bad))
        assert rc == -1, bad
        assert b"augment" in _lib.lib().mcamd_last_error()
    assert _call(desc(crop_w=0)) == -1 and b"empty crop" in _lib.lib().mcamd_last_error()
    assert _call(desc(), null_out=True) == -1
    assert _call(desc(), B=0) == -1
    assert _call(desc(), tmp_bytes=8 * 9 * 4 - 1) == -1
    assert _call(desc(tmp_off=2)) == -1
    # and the Python front end raises McamdError for an empty crop (no launch, no device needed)
    p = A.AugParams(0, 0, 0, 0, 1, 5, 0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0)
    pb = A.pack_batch([np.zeros((5, 1, 3), np.uint8)], [p], (8, 8))
    with pytest.raises(_lib.McamdError, match="empty crop"):
        A.augment_launch(pb, pb.buf, torch.empty(1, dtype=torch.uint8), torch.empty(1), stream=0)   # host memory: never reached


def test_pack_batch_rejects_what_pillow_resamples_vertically_first():
    p = A.AugParams(0, 0, 0, 0, 3, 400, 0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="taller"):
        A.pack_batch([np.zeros((400, 3, 3), np.uint8)], [p], (8, 8))
