"""Block-sparse against dense fp16 inference of the same block_prune'd YOLOv2-VOC (synthetic weights): eval, B=128 at 416x416.
For each pruning level (block_prune(level, per_layer=True), so that every layer keeps about 1 - level / 100 of its chunks;
default levels 10 25 37.5 50 62.5 75 90) it prints per layer the kept-chunk fraction (Engine.bsparse_kept), the forward launch time of the
dense fp16 engine (sparse = None: the same commit's baseline, filter compaction included) and of the block-sparse kernel
with 128- and 64-row M tiles (MCAMD_BSPARSE_BM) -- HIP events around every launch, legs alternated in one process, median
over the repetitions of the per-repetition medians, and the spread of those -- then the whole forward of the legs, alternated
windows of `forwards` forwards, and the logits rel-L2 between them.  From the table it derives the policy constant
engine.BSPARSE_MAX_KEPT: the largest kept fraction of a level at which the default tile is at least 10 % faster than the
dense launch on every layer of conv9 .. conv22.
--precision fp8: the legs are the precisions "fp8" (the same commit's dense fp8 engine, filter compaction
included: the baseline) and "fp8-block" (fp8_block_max_kept = 1.0: every candidate on csrc/conv_q8_bsparse.hip), alternated
in one process, per layer and whole forward, in the MFMA form MCAMD_Q8_MFMA selects -- run it once per form; the whole
forward of the fp16 engine with sparse = "block" on the same masks stands beside them.  The constant derived is
engine.Q8_BSPARSE_MAX_KEPT (the smaller of the two forms' values).  Default output: profiles/q8_bsparse_bench.json, or
profiles/q8_bsparse_bench_mfma.json under MCAMD_Q8_MFMA=1.
usage: python tools/bsparse_bench.py [batch] [forwards per window] [--levels 50,75,90] [--json PATH] [--precision fp8]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

POLICY_LAYERS = range(9, 23)
POLICY_GAIN = 1.10
LEGS = ("dense", "block128", "block64")


def parse(argv):
    skip = {i + 1 for i, a in enumerate(argv) if a in ("--json", "--levels", "--precision")}
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and i not in skip]
    B = int(args[0]) if len(args) > 0 else 128
    K = int(args[1]) if len(args) > 1 else 50
    out_json = argv[argv.index("--json") + 1] if "--json" in argv else None
    levels = [float(v) for v in argv[argv.index("--levels") + 1].split(",")] if "--levels" in argv else [10.0, 25.0, 37.5, 50.0, 62.5, 75.0, 90.0]
    if B < 1 or K < 1 or not levels or not all(0.0 < v < 100.0 for v in levels):
        raise SystemExit("bsparse_bench: batch and forwards per window must be positive, levels percentages in (0, 100)")
    return B, K, out_json, levels


def median(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return 100.0 * (max(v) - min(v)) / min(v)


def policy(rows, leg="block128", base="dense"):
    """rows: dicts(level, conv, kept, <base>_ms, <leg>_ms) -> (constant, per-level table).  A level passes when `leg` is at
    least POLICY_GAIN x the dense launch on every layer of POLICY_LAYERS; the constant is the largest kept fraction of a
    passing level (the smallest among that level's layers: 1x1 layers keep whole eighths)."""
    table, const = {}, 0.0
    for level in sorted({r["level"] for r in rows}):
        pts = [(r["kept"], r[base + "_ms"] / r[leg + "_ms"], r["conv"]) for r in rows if r["level"] == level and r["conv"] in POLICY_LAYERS]
        if not pts:
            continue
        gain, worst = min((g, c) for _, g, c in pts)
        kept = min(k for k, _, _ in pts)
        table["%g" % level] = {"kept": kept, "min_gain": gain, "min_gain_conv": worst, "passes": gain >= POLICY_GAIN}
        if gain >= POLICY_GAIN and kept > const:
            const = kept
    return const, table


def main(argv):
    B, K, out_json, levels = parse(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bsparse_bench needs the GPU")
    from modelcompression_amd import nets, YOLOV2_VOC_CFG, _lib
    from modelcompression_amd.pruning.weightPruning.methods import block_prune
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    dev = torch.device("cuda", 0)
    x = synthetic_batch(B, 416, 416, seed=0, device=dev)
    rows, wholes = [], []

    for level in levels:
        m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev)
        m.set_masks(block_prune(m, level, per_layer=True))
        m.eval()
        m.precision = "fp16"
        m.sparse_max_kept = 1.0

        def select(leg):
            m.sparse = None if leg == "dense" else "block"
            os.environ["MCAMD_BSPARSE_BM"] = "64" if leg == "block64" else "128"
            _lib.reload_config()

        def engine():
            return [e for k, e in m._engines.items() if k[3] == "fp16" and not e.train_layout][0]

        def layer_times(passes=5):
            eng = engine()
            per = {}
            for _ in range(passes):
                eng.events = []
                m(x)
                torch.cuda.synchronize()
                once = {}
                for tag, lay, e0, e1, _host in eng.events:
                    once[lay.li + 1] = once.get(lay.li + 1, 0.0) + e0.elapsed_time(e1)
                for k, v in once.items():
                    per.setdefault(k, []).append(v)
                eng.events = None
            return {k: median(v) for k, v in per.items()}

        with torch.no_grad():
            ms = {leg: {} for leg in LEGS}
            rates = {leg: [] for leg in LEGS}
            logits = {}
            for rep in range(3):              # alternated: the legs see the same host / GPU conditions
                for leg in LEGS:
                    select(leg)
                    for _ in range(3):
                        y = m(x)
                    torch.cuda.synchronize()
                    logits[leg] = y.clone()
                    for k, v in layer_times().items():
                        ms[leg].setdefault(k, []).append(v)
                    for _ in range(3):
                        m(x)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(K):
                        m(x)
                    torch.cuda.synchronize()
                    rates[leg].append(B * K / (time.perf_counter() - t0))
            select("block128")
            m(x)
            eng = engine()
            kept, on = dict(eng.bsparse_kept), list(eng.bsparse_layers)
        os.environ.pop("MCAMD_BSPARSE_BM", None)
        _lib.reload_config()

        print("block_prune(%g, per_layer=True); block-sparse layers (conv numbers): %s" % (level, on))
        print("%-6s %7s %10s %12s %12s %8s %8s   spread %% (dense / 128 / 64)" % ("conv", "kept", "dense ms", "block128 ms", "block64 ms",
                                                                                "d/b128", "d/b64"))
        for k in sorted(ms["dense"]):
            t = {leg: median(ms[leg][k]) for leg in LEGS}
            sp = [spread(ms[leg][k]) for leg in LEGS]
            if k in on:
                rows.append({"level": level, "conv": k, "kept": kept[k], "dense_ms": t["dense"], "block128_ms": t["block128"],
                             "block64_ms": t["block64"], "spread_pct": sp})
            print("%-6s %7s %10.3f %12.3f %12.3f %8.2f %8.2f   %.1f / %.1f / %.1f%s"
                  % ("conv%d" % k, "%.3f" % kept[k] if k in kept else "-", t["dense"], t["block128"], t["block64"],
                     t["dense"] / t["block128"], t["dense"] / t["block64"], sp[0], sp[1], sp[2], "" if k in on else "  (dense in every leg)"))
        tot = {leg: sum(median(v) for v in ms[leg].values()) for leg in LEGS}
        print("%-6s %7s %10.3f %12.3f %12.3f %8.2f %8.2f" % ("sum", "", tot["dense"], tot["block128"], tot["block64"],
                                                         tot["dense"] / tot["block128"], tot["dense"] / tot["block64"]))
        rel = {leg: float((logits[leg].double() - logits["dense"].double()).norm() / logits["dense"].double().norm()) for leg in LEGS[1:]}
        for leg in LEGS:
            print("whole forward B=%d, %d forwards per window, %-9s %s img/s (spread %.2f %%)"
                  % (B, K, leg + ":", ["%.0f" % v for v in rates[leg]], spread(rates[leg])))
        pairs = {leg: [b / a for a, b in zip(rates["dense"], rates[leg])] for leg in LEGS[1:]}
        print("pairs block / dense: %s; logits rel-L2 against the dense engine: %s\n"
              % ({k: ["%.3f" % p for p in v] for k, v in pairs.items()}, {k: "%.2e" % v for k, v in rel.items()}))
        wholes.append({"level": level, "bsparse_layers": on, "img_s": rates, "pairs_over_dense": pairs, "rel_l2_vs_dense": rel,
                       "layer_ms_sum": tot})

    const128, per128 = policy(rows, "block128")
    const64, per64 = policy(rows, "block64")
    for name, const, per in (("BM 128", const128, per128), ("BM 64", const64, per64)):
        print("policy %s (conv9 .. conv22, every layer >= %.2f x dense): max kept %.3f; per level %s"
              % (name, POLICY_GAIN, const, {k: "%.3f: %.2f (conv%d)%s" % (v["kept"], v["min_gain"], v["min_gain_conv"], "" if v["passes"] else " -")
                                            for k, v in per.items()}))
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"B": B, "forwards_per_window": K, "levels": levels, "per_layer": True, "layers": rows, "whole_forward": wholes,
                       "policy_gain": POLICY_GAIN, "policy_layers": list(POLICY_LAYERS),
                       "max_kept_bm128": const128, "levels_bm128": per128, "max_kept_bm64": const64, "levels_bm64": per64}, f, indent=1)


FP8_LEGS = ("fp8", "fp8-block", "fp16-block")


def main_fp8(argv):
    """--precision fp8: "fp8" | "fp8-block" (and the fp16 engine with sparse = "block") on the same masks."""
    B, K, out_json, levels = parse(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bsparse_bench needs the GPU")
    from modelcompression_amd import nets, YOLOV2_VOC_CFG
    from modelcompression_amd.pruning.weightPruning.methods import block_prune
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    mfma = 1 if os.environ.get("MCAMD_Q8_MFMA", "0") == "1" else 0
    if out_json is None:
        out_json = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "q8_bsparse_bench_mfma.json" if mfma else "q8_bsparse_bench.json")
    dev = torch.device("cuda", 0)
    x = synthetic_batch(B, 416, 416, seed=0, device=dev)
    rows, wholes = [], []
    for level in levels:
        m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev)
        m.set_masks(block_prune(m, level, per_layer=True))
        m.eval()
        m.sparse_max_kept = m.fp8_block_max_kept = 1.0

        def select(leg):
            m.precision, m.sparse = ("fp16", "block") if leg == "fp16-block" else (leg, None)

        def engine():
            return [e for k, e in m._engines.items() if k[3] == m.precision and not e.train_layout][0]

        def layer_times(passes=5):
            eng = engine()
            per = {}
            for _ in range(passes):
                eng.events = []
                m(x)
                torch.cuda.synchronize()
                once = {}
                for tag, lay, e0, e1, _host in eng.events:       # (a block's cast pass counts with its launch)
                    once[lay.li + 1] = once.get(lay.li + 1, 0.0) + e0.elapsed_time(e1)
                for k, v in once.items():
                    per.setdefault(k, []).append(v)
                eng.events = None
            return {k: median(v) for k, v in per.items()}

        with torch.no_grad():
            ms = {leg: {} for leg in FP8_LEGS}
            rates = {leg: [] for leg in FP8_LEGS}
            logits = {}
            for rep in range(3):              # alternated: the legs see the same host / GPU conditions
                for leg in FP8_LEGS:
                    select(leg)
                    for _ in range(3):
                        y = m(x)
                    torch.cuda.synchronize()
                    logits[leg] = y.clone()
                    for k, v in layer_times().items():
                        ms[leg].setdefault(k, []).append(v)
                    for _ in range(3):
                        m(x)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(K):
                        m(x)
                    torch.cuda.synchronize()
                    rates[leg].append(B * K / (time.perf_counter() - t0))
            select("fp8")
            m(x)
            dense_fp8 = list(engine().fp8_layers)
            select("fp8-block")
            m(x)
            eng = engine()
            kept, on, q8 = dict(eng.fp8_block_kept), list(eng.fp8_block_layers), list(eng.fp8_layers)

        print("block_prune(%g, per_layer=True), MCAMD_Q8_MFMA=%d; fp8 layers of \"fp8\": %s; of \"fp8-block\": %s; on the block kernel: %s"
              % (level, mfma, dense_fp8, q8, on))
        print("%-6s %7s %10s %13s %8s   spread %% (fp8 / fp8-block)" % ("conv", "kept", "fp8 ms", "fp8-block ms", "f/b"))
        for k in sorted(ms["fp8"]):
            t = {leg: median(ms[leg][k]) for leg in FP8_LEGS[:2]}
            sp = [spread(ms[leg][k]) for leg in FP8_LEGS[:2]]
            if k in on:
                rows.append({"level": level, "conv": k, "kept": kept[k], "fp8_ms": t["fp8"], "fp8-block_ms": t["fp8-block"],
                             "fp8_is_q8": k in dense_fp8, "spread_pct": sp})
            print("%-6s %7s %10.3f %13.3f %8.2f   %.1f / %.1f%s"
                  % ("conv%d" % k, "%.3f" % kept[k] if k in kept else "-", t["fp8"], t["fp8-block"], t["fp8"] / t["fp8-block"],
                     sp[0], sp[1], "" if k in on else "  (the same launch in both legs)"))
        tot = {leg: sum(median(v) for v in ms[leg].values()) for leg in FP8_LEGS}
        print("%-6s %7s %10.3f %13.3f %8.2f   (fp16 sparse=block: %.3f)" % ("sum", "", tot["fp8"], tot["fp8-block"],
                                                                           tot["fp8"] / tot["fp8-block"], tot["fp16-block"]))
        rel = float((logits["fp8-block"].double() - logits["fp8"].double()).norm() / logits["fp8"].double().norm())
        for leg in FP8_LEGS:
            print("whole forward B=%d, %d forwards per window, %-11s %s img/s (spread %.2f %%)"
                  % (B, K, leg + ":", ["%.0f" % v for v in rates[leg]], spread(rates[leg])))
        pairs = {base: [b / a for a, b in zip(rates[base], rates["fp8-block"])] for base in ("fp8", "fp16-block")}
        print("pairs fp8-block / base: %s; logits equal to \"fp8\": %s (rel-L2 %.2e)\n"
              % ({k: ["%.3f" % p for p in v] for k, v in pairs.items()}, bool(torch.equal(logits["fp8-block"], logits["fp8"])), rel))
        wholes.append({"level": level, "fp8_layers_fp8": dense_fp8, "fp8_layers_fp8_block": q8, "fp8_block_layers": on, "img_s": rates,
                       "fp8_block_over": pairs, "rel_l2_vs_fp8": rel, "layer_ms_sum": tot})

    const, per = policy(rows, "fp8-block", "fp8")
    print("policy MCAMD_Q8_MFMA=%d (conv9 .. conv22, every layer >= %.2f x the fp8 launch): max kept %.3f; per level %s"
          % (mfma, POLICY_GAIN, const, {k: "%.3f: %.2f (conv%d)%s" % (v["kept"], v["min_gain"], v["min_gain_conv"], "" if v["passes"] else " -")
                                        for k, v in per.items()}))
    with open(out_json, "w") as f:
        json.dump({"B": B, "forwards_per_window": K, "levels": levels, "per_layer": True, "q8_mfma": mfma, "layers": rows,
                   "whole_forward": wholes, "policy_gain": POLICY_GAIN, "policy_layers": list(POLICY_LAYERS), "max_kept": const,
                   "levels_table": per}, f, indent=1)


if __name__ == "__main__":
    if "--precision" in sys.argv[1:]:
        prec = sys.argv[sys.argv.index("--precision") + 1]
        if prec not in ("fp16", "fp8"):
            raise SystemExit("bsparse_bench: --precision must be fp16 or fp8")
        (main_fp8 if prec == "fp8" else main)(sys.argv[1:])
    else:
        main(sys.argv[1:])
