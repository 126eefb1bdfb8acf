"""Low-batch inference latency of YOLOv2-VOC at 416x416, precision "fp16": the eval forward and model.detect in milliseconds
per call at B = 1, 2, 4 and 8 with Darknet.splitk off and on, for the dense model and (B = 1) for a
quick_filter_prune(60) -> slim_export model.

Method: both settings alternate in one process, PAIRS pairs; each sample is a loop of CALLS calls after warm-up with a device
synchronise only around the whole loop (host clock), so a sample is the sustained time per call, launch overhead included;
the figure quoted is the median of the samples and every sample is kept.  The per-layer table (B = 1) comes from a separate
instrumented pass (the engine's HIP events around every conv launch, plan replay off, median of PASSES passes): conv number,
tiles, slices, us unsplit, us split (partial + finish launch).  Launch counts: the library calls of the recorded forward plan
(a split block is one call and two kernels), the eval-mode bn_coeffs launches among them and the layout pass in front.

usage: python tools/latency_bench.py [--json] [--calls N] [--pairs N]        (--json: one JSON document on stdout)"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from modelcompression_amd import nets, slim, ops, YOLOV2_VOC_CFG, _lib as L
from modelcompression_amd.pruning.weightPruning.methods import quick_filter_prune
from modelcompression_amd.synthetic import init_synthetic, synthetic_batch


def arg(name, dflt):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else dflt


CALLS, PAIRS, PASSES = max(200, arg("--calls", 200)), max(4, arg("--pairs", 4)), 7
if not torch.cuda.is_available():
    raise SystemExit("latency_bench needs the GPU")
dev = torch.device("cuda", 0)


def engine(m, x):
    return [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and not e.train_layout][0]


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def sample(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS * 1e3


def latencies(m, x):
    """{"forward" / "detect": {"off" / "on": [ms per call, one per pair]}}, the settings alternated."""
    out = {"forward": {"off": [], "on": []}, "detect": {"off": [], "on": []}}
    for _ in range(PAIRS):
        for flag in (False, True):
            m.splitk = flag
            out["forward"]["on" if flag else "off"].append(sample(lambda: m(x)))
            out["detect"]["on" if flag else "off"].append(sample(lambda: m.detect(x)))
    return out


def layer_table(m, x):
    per = {}
    for flag in (False, True):
        m.splitk = flag
        m(x)
        torch.cuda.synchronize()
        eng = engine(m, x)
        acc = {}
        for _ in range(PASSES):
            eng.events = []
            m(x)
            torch.cuda.synchronize()
            for tag, lay, e0, e1, _host in eng.events:
                acc.setdefault(lay.li + 1, []).append(e0.elapsed_time(e1) * 1e3)
            eng.events = None
        per[flag] = {k: median(v) for k, v in acc.items()}
    eng = engine(m, x)
    rows = []
    for lay in eng.layers:
        form = eng._splitk_form(lay)
        tiles = slices = None
        if form is not None and not lay.geom_act.pad:
            info = ops.conv_fwd_splitk_info(lay.geom_act, form[0], form[1])
            tiles, slices = info.tiles, info.slices
        n = lay.li + 1
        rows.append({"conv": n, "tiles": tiles, "slices": slices, "split": bool(lay.sk_on),
                     "us_unsplit": per[False].get(n), "us_split": per[True].get(n) if lay.sk_on else None})
    return rows


def launches(m, x):
    out = {}
    for flag in (False, True):
        m.splitk = flag
        m(x)
        eng = engine(m, x)
        plan = eng._fwd_plans.get(False)
        out["on" if flag else "off"] = {
            "plan_calls": plan.launches if plan is not None else None,
            "bn_coeffs": sum(1 for lay in eng.layers if lay.bn is not None),
            "layout_pass": 1,
            "splitk_finish_kernels": len(eng.splitk_layers),
            "splitk_layers": list(eng.splitk_layers)}
    return out


def bench_model(m, batches, name):
    res = {"model": name, "batches": {}}
    for B in batches:
        x = synthetic_batch(B, 416, 416, seed=0, device=dev)
        r = latencies(m, x)
        r["launches"] = launches(m, x)
        if B == 1:
            r["layers"] = layer_table(m, x)
        m.splitk = False
        a = m(x).clone()
        m.splitk = True
        b = m(x)
        r["rel_l2_on_vs_off"] = float((b.double() - a.double()).norm() / a.double().norm())
        res["batches"][str(B)] = r
    m.splitk = False
    return res


def show(res):
    print("== %s" % res["model"])
    for B, r in res["batches"].items():
        for what in ("forward", "detect"):
            off, on = r[what]["off"], r[what]["on"]
            print("B=%s %-7s ms/call: off %.3f (%.3f .. %.3f)  on %.3f (%.3f .. %.3f)  x%.3f"
                  % (B, what, median(off), min(off), max(off), median(on), min(on), max(on), median(off) / median(on)))
        la = r["launches"]
        print("B=%s plan calls: off %s, on %s (+%d finish kernels); bn_coeffs launches %d, layout pass 1; split layers %s; "
              "logits rel-L2 on vs off %.2e" % (B, la["off"]["plan_calls"], la["on"]["plan_calls"], la["on"]["splitk_finish_kernels"],
                                                la["on"]["bn_coeffs"], la["on"]["splitk_layers"], r["rel_l2_on_vs_off"]))
        if "layers" in r:
            print("%-6s %6s %6s %11s %9s" % ("conv", "tiles", "slices", "us unsplit", "us split"))
            for row in r["layers"]:
                print("%-6s %6s %6s %11s %9s" % ("conv%d" % row["conv"], row["tiles"], row["slices"],
                                                 "%.1f" % row["us_unsplit"] if row["us_unsplit"] is not None else "-",
                                                 "%.1f" % row["us_split"] if row["us_split"] is not None else "-"))


with torch.no_grad():
    dense = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev)
    dense.eval()
    dense.precision = "fp16"
    results = [bench_model(dense, (1, 2, 4, 8), "yolov2-voc")]
    pruned = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev)
    pruned.set_masks(quick_filter_prune(pruned, 60.0))
    pruned.eval()
    with tempfile.TemporaryDirectory() as tmp:
        thin = slim.slim_export(pruned, os.path.join(tmp, "slim.cfg"))
        thin.eval()
        thin.precision = "fp16"
        results.append(bench_model(thin, (1,), "yolov2-voc slim60"))

doc = {"calls": CALLS, "pairs": PAIRS, "passes": PASSES, "arch": L.lib().mcamd_arch().decode(),
       "min_chunks": int(os.environ.get("MCAMD_SPLITK_MIN_CHUNKS", 8)), "cus": int(os.environ.get("MCAMD_SPLITK_CUS", 256)),
       "results": results}
if "--json" in sys.argv:
    print(json.dumps(doc, indent=1))
else:
    for r in results:
        show(r)
