"""Low-batch inference latency of YOLOv2-VOC at 416x416: the eval forward and model.detect in milliseconds per call at
B = 1, 2, 4 and 8 with split-K off and on, for the dense model and (B = 1) for a quick_filter_prune(60) -> slim_export model.
--precision fp16 (the default): precision "fp16" with Darknet.splitk off / on.  --precision fp8: the off leg is precision "fp8",
the on leg "fp8-splitk" (MCAMD_Q8_MFMA picks the MFMA form of both), and the fp16 legs of the dense model are
measured in the same process beside them.  --precision fp8-w4: the off leg is precision "fp8", the on leg "fp8-w4" (4-bit
weights) on the dense model only; nothing is split there, and the launch record and the per-layer table carry
fields of their own (`w4_layers`; `w4`, `us_fp8`, `us_fp8_w4`) in place of the split-K ones.

Method: both settings alternate in one process, PAIRS pairs; each sample is a loop of CALLS calls after warm-up with a device
synchronise only around the whole loop (host clock), so a sample is the sustained time per call, launch overhead included;
the figure quoted is the median of the samples and every sample is kept.  The per-layer table (B = 1) comes from a separate
instrumented pass (the engine's HIP events around every conv launch, plan replay off, median of PASSES passes): conv number,
tiles, slices, us unsplit, us split (partial + finish launch).  Launch counts: the library calls of the recorded forward plan
(a split block is one call and two kernels), the eval-mode bn_coeffs launches among them and the layout pass in front.

usage: python tools/latency_bench.py [--json] [--calls N] [--pairs N] [--precision fp16|fp8|fp8-w4]
                                                                             (--json: one JSON document on stdout)"""
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
PRECISION = sys.argv[sys.argv.index("--precision") + 1] if "--precision" in sys.argv else "fp16"
if PRECISION not in ("fp16", "fp8", "fp8-w4"):
    raise SystemExit("--precision must be fp16, fp8 or fp8-w4 (got %r)" % PRECISION)
W4 = PRECISION == "fp8-w4"
ON_LEG = "fp8-w4" if W4 else "fp8-splitk"      # the on leg of an fp8 model
if not torch.cuda.is_available():
    raise SystemExit("latency_bench needs the GPU")
dev = torch.device("cuda", 0)


def engine(m, x):
    """The inference engine of this input shape in the model's current precision."""
    return [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and not e.train_layout and e.precision == m.precision][0]


def leg(m, flag):
    """Split-K off / on: Darknet.splitk of a "fp16" model; the precisions "fp8" / "fp8-splitk" (or "fp8-w4") of an fp8 one."""
    if m.precision == "fp16":
        m.splitk = flag
    else:
        m.precision = ON_LEG if flag else "fp8"


def split_layers(eng):
    return list(eng.fp8_splitk_layers if eng.q8 else eng.splitk_layers)


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
            leg(m, flag)
            out["forward"]["on" if flag else "off"].append(sample(lambda: m(x)))
            out["detect"]["on" if flag else "off"].append(sample(lambda: m.detect(x)))
    return out


def layer_table(m, x):
    per = {}
    for flag in (False, True):
        leg(m, flag)
        m(x)
        torch.cuda.synchronize()
        eng = engine(m, x)
        acc = {}
        for _ in range(PASSES):
            eng.events = []
            m(x)
            torch.cuda.synchronize()
            for tag, lay, e0, e1, _host in eng.events:
                if tag == 'fwd':      # (the conv launches; an fp8 engine also times the cast pass of an fp16 -> fp8 edge)
                    acc.setdefault(lay.li + 1, []).append(e0.elapsed_time(e1) * 1e3)
            eng.events = None
        per[flag] = {k: median(v) for k, v in acc.items()}
    eng = engine(m, x)
    if W4:                      # nothing is split: the block's form on the "fp8-w4" leg and its time on either leg
        return [{"conv": lay.li + 1, "form": lay.form, "w4": lay.form == "q8_w4", "us_fp8": per[False].get(lay.li + 1),
                 "us_fp8_w4": per[True].get(lay.li + 1)} for lay in eng.layers]
    rows = []
    for lay in eng.layers:
        tiles = slices = None
        if eng.q8:              # the fp8 blocks the pair can stand in for: forms "q8" and "q8_splitk"
            split = lay.form == "q8_splitk"
            if lay.form in ("q8", "q8_splitk") and not lay.geom_q8.pad:
                info = ops.conv_fwd_q8_splitk_info(lay.geom_q8, lay.mode)
                tiles, slices = info.tiles, info.slices
        else:
            split = bool(lay.sk_on)
            form = eng._splitk_form(lay)
            if form is not None and not lay.geom_act.pad:
                info = ops.conv_fwd_splitk_info(lay.geom_act, form[0], form[1])
                tiles, slices = info.tiles, info.slices
        n = lay.li + 1
        rows.append({"conv": n, "tiles": tiles, "slices": slices, "split": split, "form": lay.form,
                     "us_unsplit": per[False].get(n), "us_split": per[True].get(n) if split else None})
    return rows


def launches(m, x):
    out = {}
    for flag in (False, True):
        leg(m, flag)
        m(x)
        eng = engine(m, x)
        plan = eng._fwd_plans.get(False)
        out["on" if flag else "off"] = {
            "plan_calls": plan.launches if plan is not None else None,
            "bn_coeffs": sum(1 for lay in eng.layers if lay.bn is not None),
            "layout_pass": 1}
        if W4:                  # (a w4 block is one launch, like the fp8 block it stands in for)
            out["on" if flag else "off"]["w4_layers"] = list(eng.fp8_w4_layers)
        else:
            out["on" if flag else "off"].update(splitk_finish_kernels=len(split_layers(eng)), splitk_layers=split_layers(eng))
    return out


def bench_model(m, batches, name):
    res = {"model": name, "precision": m.precision, "batches": {}}
    for B in batches:
        x = synthetic_batch(B, 416, 416, seed=0, device=dev)
        r = latencies(m, x)
        r["launches"] = launches(m, x)
        if B == 1:
            r["layers"] = layer_table(m, x)
        leg(m, False)
        a = m(x).clone()
        leg(m, True)
        b = m(x)
        r["rel_l2_on_vs_off"] = float((b.double() - a.double()).norm() / a.double().norm())
        res["batches"][str(B)] = r
    leg(m, False)
    return res


def show(res):
    print("== %s, precision %s" % (res["model"], res["precision"]))
    for B, r in res["batches"].items():
        for what in ("forward", "detect"):
            off, on = r[what]["off"], r[what]["on"]
            print("B=%s %-7s ms/call: off %.3f (%.3f .. %.3f)  on %.3f (%.3f .. %.3f)  x%.3f"
                  % (B, what, median(off), min(off), max(off), median(on), min(on), max(on), median(off) / median(on)))
        la = r["launches"]
        if W4:
            print("B=%s plan calls: fp8 %s, fp8-w4 %s; bn_coeffs launches %d, layout pass 1; w4 layers %s; logits rel-L2 fp8-w4 vs fp8 %.2e"
                  % (B, la["off"]["plan_calls"], la["on"]["plan_calls"], la["on"]["bn_coeffs"], la["on"]["w4_layers"], r["rel_l2_on_vs_off"]))
            for row in r.get("layers", ()):
                print("conv%-3d %-8s us fp8 %s  us fp8-w4 %s" % (row["conv"], row["form"],
                      "%.1f" % row["us_fp8"] if row["us_fp8"] is not None else "-",
                      "%.1f" % row["us_fp8_w4"] if row["us_fp8_w4"] is not None else "-"))
            continue
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
    dense.precision = "fp8" if PRECISION == "fp8-w4" else PRECISION
    results = [bench_model(dense, (1, 2, 4, 8), "yolov2-voc")]
    pruned = None if PRECISION == "fp8-w4" else init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev)
    if pruned is not None:
        pruned.set_masks(quick_filter_prune(pruned, 60.0))
        pruned.eval()
        with tempfile.TemporaryDirectory() as tmp:
            thin = slim.slim_export(pruned, os.path.join(tmp, "slim.cfg"))
            thin.eval()
            thin.precision = PRECISION
            results.append(bench_model(thin, (1,), "yolov2-voc slim60"))
    if PRECISION == "fp8":      # the fp16 split-K figures of the same run, beside the fp8 ones
        dense.precision = "fp16"
        results.append(bench_model(dense, (1, 2, 4, 8), "yolov2-voc"))

doc = {"calls": CALLS, "pairs": PAIRS, "passes": PASSES, "arch": L.lib().mcamd_arch().decode(), "precision": PRECISION,
       "on_leg": ON_LEG if PRECISION != "fp16" else "splitk", "q8_mfma": int(os.environ.get("MCAMD_Q8_MFMA", 0)),
       "min_chunks": int(os.environ.get("MCAMD_SPLITK_MIN_CHUNKS", 8)), "cus": int(os.environ.get("MCAMD_SPLITK_CUS", 256)),
       "results": results}
if "--json" in sys.argv:
    print(json.dumps(doc, indent=1))
else:
    for r in results:
        show(r)
