"""Host side of the device-resident pictures (data.ResidentImages, augment.pack_resident, mcamd_augment_tables) without a
GPU: the index of the buffer, the packing against pack_batch, the tap counts, and every library refusal (each comes
before the first launch, so the made-up addresses are never touched)."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

from modelcompression_amd import _lib
from modelcompression_amd import augment as A
from modelcompression_amd.data import ResidentAugment, ResidentImages, ResidentList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(24, 31), (37, 53), (5, 1), (333, 250), (64, 48), (7, 7)]         # (w, h); 5 x 1 x 3 = 15 bytes: padding needed
DESC_FIELDS = [f for f, _ in _lib.AugmentDesc._fields_]


def sources():
    return [A.synthetic_source(w, h, 7 * i + 1) for i, (w, h) in enumerate(SIZES)]


def descs_of(pb):
    d = (_lib.AugmentDesc * pb.B)()
    C.memmove(d, pb.buf.numpy().ctypes.data, C.sizeof(d))
    return d


def test_offsets_are_aligned_and_disjoint_and_the_bytes_round_trip():
    srcs = sources()
    res = ResidentImages.from_sources(srcs, "cpu")
    assert len(res) == len(srcs) and res.offsets.dtype == np.int64
    assert res.sizes.tolist() == [[h, w] for w, h in SIZES]
    assert (res.offsets % 16 == 0).all()
    ends = res.offsets + res.sizes[:, 0] * res.sizes[:, 1] * 3
    assert (ends[:-1] <= res.offsets[1:]).all() and res.offsets[0] == 0
    assert res.nbytes == res.buf.numel() and ends[-1] <= res.nbytes < ends[-1] + 16
    flat = res.buf.numpy()
    for i, s in enumerate(srcs):
        assert np.array_equal(flat[res.offsets[i]:ends[i]].reshape(s.shape), s), i
        assert np.array_equal(res.source(i), s), i


def test_chunked_build_equals_the_build_in_one_piece(monkeypatch):
    srcs = sources()
    whole = ResidentImages.from_sources(srcs, "cpu")
    monkeypatch.setattr(ResidentImages, "CHUNK_BYTES", 4096)        # several chunks; the largest picture is its own
    parts = ResidentImages.from_sources(srcs, "cpu")
    assert torch.equal(parts.buf, whole.buf) and np.array_equal(parts.offsets, whole.offsets)


def test_built_from_files_with_and_without_workers(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    srcs = sources()
    paths = []
    for i, s in enumerate(srcs):
        paths.append(str(tmp_path / ("%d.png" % i)))
        Image.fromarray(s).save(paths[-1])
    want = ResidentImages.from_sources(srcs, "cpu")
    for workers in (0, 3, 99):                                       # 99: capped at 16
        got = ResidentImages(paths, "cpu", num_workers=workers)
        assert torch.equal(got.buf, want.buf) and np.array_equal(got.sizes, want.sizes)


@pytest.mark.parametrize("distort", [True, False])
def test_pack_resident_with_host_tables_equals_pack_batch_without_the_sources(distort):
    srcs = sources()
    res = ResidentImages.from_sources(srcs, "cpu")
    order = [3, 0, 5, 1, 4]
    params = [A.draw_params(random.Random(10 + i), SIZES[i][0], SIZES[i][1]) for i in order]
    shape = (64, 48)
    pb = A.pack_batch([srcs[i] for i in order], params, shape)
    pr = A.pack_resident(res, order, params, shape, distort=distort, device_tables=False)
    want, got = descs_of(pb), descs_of(pr)
    for b, i in enumerate(order):
        for f in DESC_FIELDS:
            if f == "src_off":
                assert got[b].src_off == res.offsets[i]
            elif f == "lut_off" and not distort:
                assert got[b].lut_off == -1
            else:
                assert getattr(got[b], f) == getattr(want[b], f), (b, f)
    assert (pr.coef_at, pr.coef_elems, pr.tmp_bytes) == (pb.coef_at, pb.coef_elems, pb.tmp_bytes)
    a, r = pb.buf.numpy(), pr.buf.numpy()
    assert np.array_equal(r[pr.coef_at:pr.coef_at + 4 * pr.coef_elems], a[pb.coef_at:pb.coef_at + 4 * pb.coef_elems])
    assert pr.resident_bytes == res.nbytes and pr.hsv_at is None
    if distort:
        assert pr.lut_at == pb.lut_at and np.array_equal(r[pr.lut_at:pr.lut_at + 768 * pr.B], a[pb.lut_at:pb.lut_at + 768 * pb.B])
        assert pr.buf.numel() == pb.lut_at + 768 * pb.B <= pb.src_at         # no source section (and no padding before it)
        assert pb.buf.numel() - pr.buf.numel() >= sum(srcs[i].nbytes for i in order)
    else:
        assert pr.lut_bytes == 0 and pr.buf.numel() == pr.lut_at


def test_pack_resident_for_device_tables_carries_three_numbers_per_image():
    res = ResidentImages.from_sources(sources(), "cpu")
    params = [A.draw_params(random.Random(i), w, h) for i, (w, h) in enumerate(SIZES[:4])]
    host = A.pack_resident(res, range(4), params, (64, 48), device_tables=False)
    pr = A.pack_resident(res, range(4), params, (64, 48))
    assert pr.buf.numel() == pr.hsv_at + 24 * 4 and pr.hsv_at % 8 == 0
    hsv = pr.buf.numpy()[pr.hsv_at:].view(np.float64).reshape(4, 3)
    assert hsv.tolist() == [[p.dhue, p.dsat, p.dexp] for p in params]
    for g, w in zip(descs_of(pr), descs_of(host)):
        assert all(getattr(g, f) == getattr(w, f) for f in DESC_FIELDS)
    assert pr.coef_at == 0 and pr.lut_at >= 4 * pr.coef_elems and pr.lut_bytes == 768 * 4


def test_table_taps_is_the_ksize_of_resample_table():
    pairs = [(n, n) for n in (1, 5, 416)] + [(1, 13), (37, 64), (1600, 416), (2000, 13), (2, 32), (53, 48), (333, 64)]
    pairs += [(a, b) for a in (1, 2, 3, 7, 13, 64, 100, 415, 416, 417, 832, 833, 1000, 4097) for b in (1, 2, 13, 48, 64, 416, 608)]
    for n_in, n_out in pairs:
        assert A.table_taps(n_in, n_out) == A.resample_table(n_in, n_out)[0], (n_in, n_out)


def test_resize_params_crop_the_whole_picture_and_distort_false_has_no_luts():
    res = ResidentImages.from_sources(sources(), "cpu")
    idx = list(range(len(SIZES)))
    p = A.resize_params(500, 375)
    assert p == A.AugParams(0, -1, 0, -1, 501, 376, 0, 0., 0., 1., 1., 0., 1., 1.)
    pr = A.pack_resident(res, idx, [A.resize_params(w, h) for w, h in SIZES], (64, 48), distort=False)
    for d, (w, h) in zip(descs_of(pr), SIZES):
        assert (d.crop_x, d.crop_y, d.crop_w, d.crop_h, d.flip) == (0, 0, w, h, 0) and (d.src_w, d.src_h) == (w, h)
        assert d.lut_off == -1
    assert descs_of(pr)[4].hk == descs_of(pr)[4].vk == 1               # 64 x 48 -> 64 x 48: identity tables


def test_resident_sets_yield_indices_and_collate_to_the_same_batches():
    srcs = sources()
    res = ResidentImages.from_sources(srcs, "cpu")
    boxes = [np.array([[i, 0.5, 0.5, 0.3, 0.4]]) for i in range(len(srcs))]
    ds = ResidentAugment(res, boxes, (64, 48), seed=3)
    ds.set_epoch(2)
    assert not hasattr(ds, "buf") and len(ds) == len(srcs)
    items = [ds[i] for i in (1, 4)]
    assert [(i, p) for i, _, p in items] == [(i, A.draw_params(A.sample_rng(3, 2, i), *SIZES[i])) for i in (1, 4)]
    pb = ds.collate(items)
    assert torch.equal(pb.target, torch.stack([A.transform_labels(b, p) for _, b, p in items])) and pb.hsv_at is not None
    targets = torch.arange(len(srcs) * 250, dtype=torch.float32).reshape(-1, 250)
    rl = ResidentList(res, targets, (64, 48))
    pb = rl.collate([rl[2], rl[0]])
    assert torch.equal(pb.target, targets[[2, 0]]) and [d.lut_off for d in descs_of(pb)] == [-1, -1]
    with pytest.raises(ValueError):
        ResidentList(res, targets[:2], (64, 48))


# ------------------------------------------------------------------------------------------------------- the library
FAKE = 1 << 40          # never dereferenced: every case below fails validation first


def _refused(rc, *words):
    assert rc == -1
    text = _lib.lib().mcamd_last_error().decode()
    for w in words:
        assert w in text, (w, text)


def _desc(**kw):
    d = (_lib.AugmentDesc * 1)()
    f = dict(src_w=10, src_h=10, crop_w=9, crop_h=9, hk=7, vk=7, hcoef_off=0, vcoef_off=100)       # 9 -> 8: 7 taps
    f.update(kw)
    for k, v in f.items():
        setattr(d[0], k, v)
    return d


def test_augment_refuses_every_negative_lut_off_but_minus_one():
    def call(d, lut=FAKE):
        bt = _lib.AugmentBatch(desc=C.addressof(d), desc_dev=FAKE, src=FAKE, src_bytes=1 << 20, coef=FAKE, coef_elems=1 << 20,
                               lut=lut, lut_bytes=768, tmp=FAKE, tmp_bytes=1 << 20, out=FAKE, B=1, H=8, W=8)
        return _lib.lib().mcamd_augment(C.byref(bt), None)
    _refused(call(_desc(lut_off=-2)), "augment", "LUTs", "-2")
    _refused(call(_desc(lut_off=-1 << 20)), "LUTs")
    _refused(call(_desc(lut_off=1)), "LUTs")
    _refused(call(_desc(lut_off=0), lut=None), "LUTs")                 # LUTs asked for, no buffer


def _tables(d, B=1, H=8, W=8, coef=FAKE, coef_elems=1 << 20, hsv=FAKE, lut=FAKE, lut_bytes=768):
    return _lib.lib().mcamd_augment_tables(C.addressof(d), FAKE, hsv, B, H, W, coef, coef_elems, lut, lut_bytes, None)


def test_augment_tables_refusals_come_before_any_launch():
    assert A.table_taps(9, 8) == 7 and A.table_taps(8, 8) == 1
    _refused(_tables(_desc(hk=5)), "augment_tables", "tap counts")
    _refused(_tables(_desc(vk=1)), "tap counts")
    _refused(_tables(_desc(crop_w=8)), "tap counts")                   # the identity table has one tap, not seven
    _refused(_tables(_desc(), coef_elems=100 + 8 * 9 - 1), "outside coef")
    _refused(_tables(_desc(hcoef_off=(1 << 20) - 71)), "outside coef")
    _refused(_tables(_desc(vcoef_off=-1)), "outside coef")
    _refused(_tables(_desc(), hsv=None), "LUTs")                       # lut_off 0 and nowhere to read (dhue, dsat, dexp)
    _refused(_tables(_desc(), lut=None), "LUTs")
    _refused(_tables(_desc(lut_off=1)), "LUTs")
    _refused(_tables(_desc(lut_off=-2)), "LUTs")
    _refused(_tables(_desc(crop_w=0)), "empty crop")
    _refused(_tables(_desc(crop_h=-4)), "empty crop")
    _refused(_tables(_desc(), coef=None), "null")
    _refused(_tables(_desc(), B=0), "batch shape")


def test_the_new_symbol_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcamd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mcamd_augment_tables\s*\(", hdr)
    assert "mcamd_augment_tables" in _lib.SIGNATURES and hasattr(_lib.lib(), "mcamd_augment_tables")
    assert len(_lib.SIGNATURES["mcamd_augment_tables"][1]) == 11
