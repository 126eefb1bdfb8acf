"""Detection post-processing per batch: the batched torch path (nets2_utils.detections), the one-launch HIP kernel
(detections_device, csrc/detect.hip) and the kernel plus the list conversion (detections_fused), each beside the fp16 eval
forward of the same batch.  13x13 logits randn * 1.5 (the spread of tests/golden/postproc.npz), thresholds
(0.005, 0.45) -- the VOC evaluation -- and (0.25, 0.45) -- deployment.
usage: python tools/detect_bench.py [batch] [iters] [--json]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from modelcompression_amd import nets, YOLOV2_VOC_CFG
from modelcompression_amd import nets2_utils as U
from modelcompression_amd.synthetic import init_synthetic, synthetic_batch

args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if len(args) > 0 else 128
K = int(args[1]) if len(args) > 1 else 100
REPEATS = 3         # timed windows per figure; the median is reported, the spread next to it
dev = torch.device("cuda", 0)


def wall(fn, iters):
    """ms per call by the host clock around a synchronise (fn may synchronise itself)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def events(fn, iters):
    """ms per call by device events (fn never synchronises)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(timer, fn, iters, what=""):
    """Median of REPEATS windows of `iters` calls after warm-up.  A call that takes long (the paths that build Python lists
    take seconds at the evaluation threshold) gets fewer calls per window: a window holds about a second of work."""
    fn()
    t = wall(fn, 1) / 1e3
    iters = max(1, min(iters, int(1.0 / max(t, 1e-6))))
    if t < 0.1:
        fn()
    v = [timer(fn, iters) for _ in range(REPEATS)]
    r = {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "calls_per_window": iters}
    print("%s: %s" % (what, r), file=sys.stderr, flush=True)
    return r


m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev).eval()
m.precision = "fp16"
x = synthetic_batch(B, 416, 416, seed=0, device=dev)
out = (torch.randn(B, 125, 13, 13, generator=torch.Generator().manual_seed(0)) * 1.5).to(dev)
res = {"tool": "detect_bench", "batch": B, "iters": K, "repeats": REPEATS, "grid": [13, 13], "logits": "randn * 1.5"}
with torch.no_grad():
    res["forward_fp16"] = measure(events, lambda: m(x), max(K // 5, 5), "forward_fp16")
    for ct, nt in ((0.005, 0.45), (0.25, 0.45)):
        a = (out, ct, nt, m.num_classes, m.anchors, m.num_anchors)
        r = {
            "torch_detections": measure(wall, lambda: U.detections(*a), K, "torch_detections %g" % ct),
            "hip_detections_device": measure(events, lambda: U.detections_device(*a), 10 * K, "hip_detections_device %g" % ct),
            "hip_detections_fused": measure(wall, lambda: U.detections_fused(*a), K, "hip_detections_fused %g" % ct),
        }
        nk = U.detections_device(*a)[2]
        r["kept_per_image"] = round(float(nk.float().mean()), 1)
        res["conf_%g_nms_%g" % (ct, nt)] = r
if "--json" in sys.argv:
    print(json.dumps(res))
else:
    print("B=%d, fp16 eval forward %.3f ms" % (B, res["forward_fp16"]["ms"]))
    for k, r in res.items():
        if k.startswith("conf_"):
            print("%s (%.1f kept per image): torch detections() %.3f ms | HIP detections_device %.4f ms | "
                  "HIP detections_fused (with lists) %.3f ms" % (k, r["kept_per_image"], r["torch_detections"]["ms"],
                                                                 r["hip_detections_device"]["ms"], r["hip_detections_fused"]["ms"]))
