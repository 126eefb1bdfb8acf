#!/usr/bin/env python3
"""Training augmentation figures, one JSON line:
  * device time of mcamd_augment per B=64 batch of VOC-sized sources (HIP events, warmed up), bytes moved, HBM share;
  * loader images/s with 16 workers over synthetic JPEGs in a temp dir: VOCList (PIL resize, no augmentation) and
    VOCAugment + collate + DeviceAugmenter;
  * train(..., AUGMENT=True) samples/s over 20 steps on the synthetic ragged source, next to AUGMENT=False;
  * --resident instead: the same JPEG list made resident on the device (build seconds, bytes), then, taken
    alternately in this process for --rounds rounds, images/s of the two loaders above (16 workers) and of ResidentList /
    ResidentAugment + DeviceAugmenter with 0, 4 and 16 loader workers; the median of the rounds is reported.

    python tools/augment_bench.py [--iters 50] [--images 512] [--skip-train] [--device-only] [--resident [--rounds 3]]
"""
import argparse
import contextlib
import io
import json
import os
import random
import re
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modelcompression_amd import YOLOV2_VOC_CFG, augment as A  # noqa: E402
from modelcompression_amd.data import (ResidentAugment, ResidentImages, ResidentList, VOCAugment, VOCList,  # noqa: E402
                                       label_path_for, read_boxes)

HBM_BPS = 6.3e12      # achievable copy rate, MI355X_MICROARCH


def voc_like_sources(n, seed=0):
    g = np.random.default_rng(seed)
    sizes = [(500, 375), (375, 500), (500, 333), (333, 500), (500, 400), (480, 360)]
    return [A.synthetic_source(*sizes[int(g.integers(len(sizes)))], seed=i) for i in range(n)]


def device_time(dev, iters):
    shape = (416, 416)
    sources = voc_like_sources(64)
    params = [A.draw_params(random.Random(i), s.shape[1], s.shape[0]) for i, s in enumerate(sources)]
    pb = A.pack_batch(sources, params, shape).pin_memory()
    dev_buf = pb.buf.to(dev)
    tmp = torch.empty(pb.tmp_bytes, dtype=torch.uint8, device=dev)
    x = torch.empty(64, 3, 416, 416, device=dev)
    for _ in range(10):
        A.augment_launch(pb, dev_buf, tmp, x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        A.augment_launch(pb, dev_buf, tmp, x)
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / iters
    aug = A.DeviceAugmenter(shape, dev)
    for _ in range(3):
        aug(pb)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        aug(pb)
    e1.record()
    e1.synchronize()
    ms_h2d = e0.elapsed_time(e1) / iters
    src_bytes = sum(s.nbytes for s in sources)
    moved = src_bytes + 2 * pb.tmp_bytes + x.numel() * 4
    return {"augment_ms_b64": round(ms, 4), "augment_with_h2d_ms_b64": round(ms_h2d, 4), "bytes_moved": moved,
            "source_bytes": src_bytes, "hbm_share": round(moved / (ms * 1e-3) / HBM_BPS, 3)}


def write_jpegs(root, n):
    from PIL import Image
    img_dir, lab_dir = os.path.join(root, "JPEGImages"), os.path.join(root, "labels")
    os.makedirs(img_dir)
    os.makedirs(lab_dir)
    lines = []
    for i, s in enumerate(voc_like_sources(n, seed=1)):
        p = os.path.join(img_dir, "%05d.jpg" % i)
        Image.fromarray(s).save(p, quality=90)
        np.savetxt(os.path.join(lab_dir, "%05d.txt" % i), [[i % 20, 0.5, 0.5, 0.3, 0.4]])
        lines.append(p)
    listfile = os.path.join(root, "train.txt")
    with open(listfile, "w") as f:
        f.write("\n".join(lines) + "\n")
    return listfile


def loader_rate(dev, listfile, augment):
    shape = (416, 416)
    ds = VOCAugment(listfile, shape) if augment else VOCList(listfile, shape)
    loader = torch.utils.data.DataLoader(ds, batch_size=64, shuffle=False, num_workers=16, pin_memory=True,
                                         drop_last=True, collate_fn=A.collate_fn(shape) if augment else None)
    aug = A.DeviceAugmenter(shape, dev)
    n, t0 = 0, None
    for i, batch in enumerate(loader):
        if i == 1:                       # the first batch includes the workers' start-up
            torch.cuda.synchronize()
            t0, n = time.time(), 0
        x, _ = aug(batch) if augment else (batch[0].to(dev, non_blocking=True), batch[1])
        n += x.shape[0]
    torch.cuda.synchronize()
    return round(n / (time.time() - t0), 1)


def resident_rate(dev, ds, resident, workers, passes=4):
    """images/s of a resident set's loader + DeviceAugmenter over `passes` passes (the first batch is not timed)."""
    loader = torch.utils.data.DataLoader(ds, batch_size=64, shuffle=False, num_workers=workers, pin_memory=True,
                                         drop_last=True, collate_fn=ds.collate)
    aug = A.DeviceAugmenter(ds.shape, dev, resident)
    n, t0 = 0, None
    for epoch in range(passes):
        for i, batch in enumerate(loader):
            if epoch == 0 and i == 1:
                torch.cuda.synchronize()
                t0, n = time.time(), 0
            x, _ = aug(batch)
            n += x.shape[0]
    torch.cuda.synchronize()
    return round(n / (time.time() - t0), 1)


def resident_figures(dev, listfile, rounds):
    shape = (416, 416)
    lines = VOCList(listfile, shape).lines
    res = {}
    for workers in (4, 16):
        torch.cuda.synchronize()
        t0 = time.time()
        resident = ResidentImages(lines, dev, num_workers=workers)
        res["resident_build_s_%d_threads" % workers] = round(time.time() - t0, 3)
    res["resident_images"], res["resident_bytes"] = len(resident), resident.nbytes
    labels = [label_path_for(p) for p in lines]
    sets = {"list": ResidentList(resident, labels, shape),
            "augment": ResidentAugment(resident, [read_boxes(lp) for lp in labels], shape)}
    runs = {}
    for _ in range(rounds):                      # old and new alternately: drift of the machine hits both
        for name, augment in (("list", False), ("augment", True)):
            runs.setdefault("loader_%s_files_16w_img_s" % name, []).append(loader_rate(dev, listfile, augment))
            for workers in (0, 4, 16):
                runs.setdefault("loader_%s_resident_%dw_img_s" % (name, workers), []).append(
                    resident_rate(dev, sets[name], resident, workers))
    for k, v in runs.items():
        res[k] = {"median": statistics.median(v), "runs": v}
    return res


def train_rate(augment, steps=20):
    from modelcompression_amd.train import YOLOv2Train
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        YOLOv2Train().train('', '', '', '', '', '', 'p_', YOLOV2_VOC_CFG, '', 64, 10, DEBUG_EPOCHS=steps - 1,
                            MAX_EPOCHS=1, SYNTHETIC_SAMPLES=64 * steps, AUGMENT=augment)
    return float(re.findall(r"training with ([0-9.]+) samples/s", buf.getvalue())[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--device-only", action="store_true", help="only the device time (for a profiler run)")
    ap.add_argument("--resident", action="store_true", help="file loaders against the resident loaders, alternately")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"metric": "augment", "pil": __import__("PIL").__version__}
    if a.resident:
        res["metric"] = "augment_resident"
        with tempfile.TemporaryDirectory() as root:
            res.update(resident_figures(dev, write_jpegs(root, a.images), a.rounds))
        print(json.dumps(res))
        return
    res.update(device_time(dev, a.iters))
    if a.device_only:
        print(json.dumps(res))
        return
    with tempfile.TemporaryDirectory() as root:
        listfile = write_jpegs(root, a.images)
        res["loader_voclist_img_s"] = loader_rate(dev, listfile, False)
        res["loader_augment_img_s"] = loader_rate(dev, listfile, True)
    if not a.skip_train:
        res["train_samples_s_augment_off"] = train_rate(False)
        res["train_samples_s_augment_on"] = train_rate(True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
