"""VOC07 evaluation after the forward passes: PASCALVOCEval.predict's file path (fused = True: mcamd_detect, lists, one text
file per class, voc_eval's Python matching) against predict(DEVICE_EVAL=True) (mcamd_detect, mcamd_voc_match, one sort,
mcamd_voc_ap; csrc/voc_eval.hip) on a generated devkit: grey pictures, random ground truth, and instead of a network a
module that replays stored 13x13 logits randn * 1.5 (the spread of tests/golden/postproc.npz), so that what is timed is the
evaluation and the image loader that both paths share (timed alone as `loader`).  mAP is meaningless here; the two paths
report the same one unless scores tie after the six-decimal rounding (numpy's argsort is not stable).
Thresholds (0.005, 0.45) -- the reference's evaluation -- and (0.25, 0.45).  Median of five runs.
--resident instead: the pictures made resident on the device once (build seconds, bytes), then, run by run
alternately, the loader alone from files (one worker, as predict starts it) and from the resident set (0, 4 and 16 loader
workers), and both paths of predict at (0.005, 0.45) with RESIDENT=None and RESIDENT=True.
usage: python tools/voc_eval_bench.py [images] [batch] [--json] [--resident]"""
import contextlib
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image
from modelcompression_amd import nets, YOLOV2_VOC_CFG
from modelcompression_amd.augment import DeviceAugmenter
from modelcompression_amd.data import ResidentImages, ResidentList, VOCList, label_path_for
from modelcompression_amd.predict import PASCALVOCEval

args = [a for a in sys.argv[1:] if not a.startswith("--")]
IMAGES = int(args[0]) if len(args) > 0 else 256
B = int(args[1]) if len(args) > 1 else 64
REPEATS = 5
dev = torch.device("cuda", 0)
CLASSES = PASCALVOCEval(None, '', '', None, '', '', '', '', '').VOC_CLASSES
OBJ = ("<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>%d</difficult>"
       "<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>")


def write_devkit(root, n, rng):
    base = os.path.join(root, 'VOC2007')
    for d in ('Annotations', 'ImageSets/Main', 'JPEGImages'):
        os.makedirs(os.path.join(base, d))
    paths = []
    for i in range(n):
        name, W, H = "%06d" % i, 500, 375
        body = ""
        for _ in range(rng.randint(1, 7)):
            x, y = rng.randint(0, W - 60), rng.randint(0, H - 60)
            body += OBJ % (CLASSES[rng.randint(20)], rng.rand() < 0.15, x, y, x + rng.randint(20, W - x), y + rng.randint(20, H - y))
        with open(os.path.join(base, 'Annotations', name + '.xml'), 'w') as f:
            f.write("<annotation><filename>%s</filename>%s</annotation>\n" % (name, body))
        paths.append(os.path.join(base, 'JPEGImages', name + '.png'))
        Image.fromarray(np.full((H, W, 3), 128, dtype=np.uint8)).save(paths[-1])
    with open(os.path.join(base, 'ImageSets', 'Main', 'test.txt'), 'w') as f:
        f.write(''.join("%06d\n" % i for i in range(n)))
    listfile = os.path.join(root, 'list.txt')
    with open(listfile, 'w') as f:
        f.write(''.join(p + '\n' for p in paths))
    return listfile


class Replay(torch.nn.Module):
    """Stands where the network stands in predict(): returns the stored logits of the batch."""

    def __init__(self, like, logits):
        super().__init__()
        self.width, self.height, self.num_classes = like.width, like.height, like.num_classes
        self.anchors, self.num_anchors = like.anchors, like.num_anchors
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.logits, self.calls = logits, 0

    def forward(self, x):
        out = self.logits[self.calls % len(self.logits)][:x.size(0)]
        self.calls += 1
        return out


def median_seconds(fn, what):
    fn()                                                      # warm-up (and voc_eval's annotation cache)
    v = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        v.append(time.perf_counter() - t0)
    r = {"s": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print("%s: %s" % (what, r), file=sys.stderr, flush=True)
    return r


root = tempfile.mkdtemp(prefix="voc_eval_bench_")
listfile = write_devkit(root, IMAGES, np.random.RandomState(0))
like = nets.Darknet(YOLOV2_VOC_CFG)
nb = (IMAGES + B - 1) // B
g = torch.Generator().manual_seed(0)
logits = [(torch.randn(B, 125, 13, 13, generator=g) * 1.5).to(dev) for _ in range(nb)]
model = Replay(like, logits).to(dev)
ev = PASCALVOCEval(model, YOLOV2_VOC_CFG, '', None, root, listfile, os.path.join(root, 'det'), 'det_', os.path.join(root, 'pkl'))
ev.fused = True
res = {"tool": "voc_eval_bench", "images": IMAGES, "batch": B, "repeats": REPEATS, "grid": [13, 13], "logits": "randn * 1.5"}


def run(ct, nt, device_eval, resident=None):
    model.calls = 0
    with contextlib.redirect_stdout(io.StringIO()):
        return ev.predict(BATCH_SIZE=B, CONF_THRESH=ct, NMS_THRESH=nt, DEVICE_EVAL=device_eval, RESIDENT=resident)


def loader_only():
    ds = VOCList(listfile, shape=(like.width, like.height), train=False)
    for data, _ in torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False, num_workers=1, pin_memory=True):
        data.to(dev)


def alternately(fns):
    """{name: fn} -> {name: median / min / max seconds}: one warm-up each, then REPEATS rounds that run every fn once."""
    v = {k: [] for k in fns}
    for k, fn in fns.items():
        fn()
    for _ in range(REPEATS):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            v[k].append(time.perf_counter() - t0)
    return {k: {"s": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for k, t in v.items()}


def resident_bench():
    shape = (like.width, like.height)
    lines = VOCList(listfile, shape=shape, train=False).lines
    for workers in (4, 16):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        resident = ResidentImages(lines, dev, num_workers=workers)
        res["resident_build_s_%d_threads" % workers] = round(time.perf_counter() - t0, 3)
    res["resident_bytes"] = resident.nbytes
    rl = ResidentList(resident, [label_path_for(p) for p in lines], shape)
    aug = DeviceAugmenter(shape, dev, resident)

    def resident_loader(workers):
        for batch in torch.utils.data.DataLoader(rl, batch_size=B, shuffle=False, num_workers=workers, pin_memory=True,
                                                 collate_fn=rl.collate):
            aug(batch)
    fns = {"loader_files_1w": loader_only}
    for workers in (0, 4, 16):
        fns["loader_resident_%dw" % workers] = lambda w=workers: resident_loader(w)
    res["loader"] = alternately(fns)
    r = alternately({"device_path_files": lambda: run(0.005, 0.45, True), "device_path_resident": lambda: run(0.005, 0.45, True, resident),
                     "file_path_files": lambda: run(0.005, 0.45, False), "file_path_resident": lambda: run(0.005, 0.45, False, resident)})
    run(0.005, 0.45, True)
    r["mAP_files"] = ev.mAP
    run(0.005, 0.45, True, resident)
    r["mAP_resident"] = ev.mAP
    res["conf_0.005_nms_0.45"] = r


if "--resident" in sys.argv:
    res["tool"] = "voc_eval_bench --resident"
    resident_bench()
    shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(res))
    sys.exit(0)
res["loader"] = median_seconds(loader_only, "loader")
for ct, nt in ((0.005, 0.45), (0.25, 0.45)):
    r = {"device_path": median_seconds(lambda: run(ct, nt, True), "device_path %g" % ct)}
    r["mAP_device"], r["records"] = ev.mAP, ev.num_detections
    r["file_path"] = median_seconds(lambda: run(ct, nt, False), "file_path %g" % ct)
    r["mAP_file"], r["lines"] = ev.mAP, ev.num_detections
    r["equal"] = r["mAP_device"] == r["mAP_file"]
    res["conf_%g_nms_%g" % (ct, nt)] = r
shutil.rmtree(root, ignore_errors=True)
if "--json" in sys.argv:
    print(json.dumps(res))
else:
    print("%d images in batches of %d; the loader alone %.3f s" % (IMAGES, B, res["loader"]["s"]))
    for k, r in res.items():
        if k.startswith("conf_"):
            print("%s (%d records): file path %.3f s | device path %.3f s | same mAP: %s"
                  % (k, r["records"], r["file_path"]["s"], r["device_path"]["s"], r["equal"]))
