"""Block-sparse against dense fp16 TRAINING of the same block_prune'd YOLOv2-VOC (synthetic weights): fwd + bwd + SGD steps at
416x416, precision "fp16", one process, one GPU.  For each pruning level (block_prune(level, per_layer=True);
the seven kept levels of DESIGN.md 3t) the legs sparse_train = None (the same commit's dense step, filter compaction
included: the baseline) and sparse_train = "block" with every candidate chosen (sparse_train_max_kept = 1.0) are alternated:
  * the whole step: windows of STEPS steps, legs alternated, the median over the windows and their spread;
  * per layer, from the engine's instrumented pass (HIP events around every launch, each launch alone on the GPU): the forward
    and the dgrad launch of either leg -- median over the repetitions of the per-repetition medians, and the spread of those;
  * the two list launches per chosen block per step (tag 'lists'), summed over the layers.
From the table it derives engine.BSPARSE_TRAIN_MAX_KEPT by the rule of 3t: the largest kept fraction of a level at which BOTH
the forward and the dgrad launch of every layer of conv9 .. conv22 are at least 10 % faster than the dense training launches
they replace (0.0 when no level passes).
--wgrad adds the leg sparse_train = "block-wgrad" (sparse_train_wgrad_max_kept = 1.0: every candidate's weight
gradient on the list launch), alternated with the other two in the same process, and reports per layer the weight-gradient
launch of the "block" leg (dense: compute + finish + dbias) against the list launch, the three whole steps, and
engine.BSPARSE_TRAIN_WGRAD_MAX_KEPT by the same rule on the weight-gradient launches (profiles/bsparse_train_wgrad_bench.json).
usage: python tools/bsparse_train_bench.py [B] [STEPS] [--levels 50,75,90] [--json [PATH]] [--wgrad [PATH]]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

POLICY_LAYERS = range(9, 23)
POLICY_GAIN = 1.10
LEGS = ("dense", "block")
WGRAD_LEG = "block-wgrad"
DEFAULT_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bsparse_train_bench.json")
DEFAULT_WGRAD_JSON = os.path.join(os.path.dirname(DEFAULT_JSON), "bsparse_train_wgrad_bench.json")


def parse(argv):
    levels, out_json, wgrad_json, pos = [10.0, 25.0, 37.5, 50.0, 62.5, 75.0, 90.0], None, None, []
    i = 0
    while i < len(argv):
        a = argv[i]
        if a == "--levels":
            levels = [float(v) for v in argv[i + 1].split(",")]
            i += 1
        elif a == "--json":
            if i + 1 < len(argv) and not argv[i + 1].startswith("--") and not argv[i + 1].replace(".", "").isdigit():
                out_json = argv[i + 1]
                i += 1
            else:
                out_json = DEFAULT_JSON
        elif a == "--wgrad":
            if i + 1 < len(argv) and not argv[i + 1].startswith("--") and not argv[i + 1].replace(".", "").isdigit():
                wgrad_json = argv[i + 1]
                i += 1
            else:
                wgrad_json = DEFAULT_WGRAD_JSON
        elif not a.startswith("--"):
            pos.append(a)
        i += 1
    B = int(pos[0]) if pos else 64
    K = int(pos[1]) if len(pos) > 1 else 30
    if B < 1 or K < 1 or not levels or not all(0.0 < v < 100.0 for v in levels):
        raise SystemExit("bsparse_train_bench: B and STEPS must be positive, levels percentages in (0, 100)")
    return B, K, out_json, levels, wgrad_json


def wgrad_policy(rows):
    """rows: dicts(level, conv, kept, wgrad_dense_ms, wgrad_list_ms) -> (constant, per-level table): policy()'s rule on the
    weight-gradient launch of every chosen layer of POLICY_LAYERS."""
    table, const = {}, 0.0
    for level in sorted({r["level"] for r in rows}):
        pts = [(r["wgrad_dense_ms"] / r["wgrad_list_ms"], r["conv"], r["kept"]) for r in rows
               if r["level"] == level and r["conv"] in POLICY_LAYERS]
        if not pts:
            continue
        gain, worst, _ = min(pts)
        kept = min(p[2] for p in pts)
        table["%g" % level] = {"kept": kept, "min_gain": gain, "min_gain_conv": worst, "passes": gain >= POLICY_GAIN}
        if gain >= POLICY_GAIN and kept > const:
            const = kept
    return const, table


def median(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return 100.0 * (max(v) - min(v)) / min(v)


def policy(rows):
    """rows: dicts(level, conv, kept, fwd_dense_ms, fwd_block_ms, dgrad_dense_ms, dgrad_block_ms, dgrad_on) -> (constant, per-level
    table).  A level passes when the forward AND (where the block's dgrad runs the kernel) the dgrad launch of every layer of
    POLICY_LAYERS gain at least POLICY_GAIN; the constant is the largest kept fraction of a passing level (the smallest
    among that level's layers)."""
    table, const = {}, 0.0
    for level in sorted({r["level"] for r in rows}):
        pts = []
        for r in rows:
            if r["level"] != level or r["conv"] not in POLICY_LAYERS:
                continue
            pts.append((r["fwd_dense_ms"] / r["fwd_block_ms"], r["conv"], "fwd"))
            if r["dgrad_on"]:
                pts.append((r["dgrad_dense_ms"] / r["dgrad_block_ms"], r["conv"], "dgrad"))
        if not pts:
            continue
        gain, worst, which = min(pts)
        kept = min(r["kept"] for r in rows if r["level"] == level and r["conv"] in POLICY_LAYERS)
        table["%g" % level] = {"kept": kept, "min_gain": gain, "min_gain_conv": worst, "min_gain_launch": which, "passes": gain >= POLICY_GAIN}
        if gain >= POLICY_GAIN and kept > const:
            const = kept
    return const, table


def main(argv):
    B, K, out_json, levels, wgrad_json = parse(argv)
    LEGS = globals()["LEGS"] + ((WGRAD_LEG,) if wgrad_json else ())
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bsparse_train_bench needs the GPU")
    from modelcompression_amd import nets, YOLOV2_VOC_CFG
    from modelcompression_amd.pruning.weightPruning.methods import block_prune
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    dev = torch.device("cuda", 0)
    x = synthetic_batch(B, 416, 416, seed=0, device=dev)
    gout = torch.randn(B, 125, 13, 13, generator=torch.Generator().manual_seed(1)).to(dev) * 0.01
    rows, wholes, wrows, wwholes = [], [], [], []

    for level in levels:
        m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev)
        m.set_masks(block_prune(m, level, per_layer=True))
        m.train()
        m.precision = "fp16"
        m.sparse_train_max_kept = 1.0
        m.sparse_train_wgrad_max_kept = 1.0
        opt = torch.optim.SGD(m.parameters(), lr=1e-6, momentum=0.9, weight_decay=5e-4, fused=True)

        def select(leg):
            m.sparse_train = None if leg == "dense" else leg

        def engine():
            return [e for e in m._engines.values() if e.train_layout][0]

        def step():
            out = m(x)
            opt.zero_grad()
            out.backward(gout)
            opt.step()

        def layer_times(passes=3):
            """{(tag, conv): ms} of one instrumented step, the median over `passes`; ('lists', 0): all list launches of a step"""
            eng = engine()
            per = {}
            for _ in range(passes):
                eng.events = []
                step()
                torch.cuda.synchronize()
                once = {}
                for tag, lay, e0, e1, _host in eng.events:
                    key = (tag, 0 if tag == "lists" else lay.li + 1)
                    once[key] = once.get(key, 0.0) + e0.elapsed_time(e1)
                for k, v in once.items():
                    per.setdefault(k, []).append(v)
                eng.events = None
            return {k: median(v) for k, v in per.items()}

        ms = {leg: {} for leg in LEGS}
        step_ms = {leg: [] for leg in LEGS}
        for rep in range(3):                  # alternated: the legs see the same host / GPU conditions
            for leg in LEGS:
                select(leg)
                for _ in range(3):
                    step()
                torch.cuda.synchronize()
                for k, v in layer_times().items():
                    ms[leg].setdefault(k, []).append(v)
                for _ in range(3):
                    step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(K):
                    step()
                torch.cuda.synchronize()
                step_ms[leg].append(1e3 * (time.perf_counter() - t0) / K)
        select("block")
        step()
        torch.cuda.synchronize()
        eng = engine()
        kept, on, don = dict(eng.bsparse_train_kept), list(eng.bsparse_train_layers), list(eng.bsparse_train_dgrad_layers)
        finite = all(bool(torch.isfinite(p).all()) for p in m.parameters())

        print("block_prune(%g, per_layer=True); forward on the kernel (conv numbers): %s; dgrad: %s" % (level, on, don))
        print("%-6s %7s %9s %9s %6s %9s %9s %6s   spread %% (fwd d / b, dgrad d / b)"
              % ("conv", "kept", "fwd d ms", "fwd b ms", "d/b", "dgr d ms", "dgr b ms", "d/b"))
        t = {leg: {k: median(v) for k, v in ms[leg].items()} for leg in LEGS}
        sp = {leg: {k: spread(v) for k, v in ms[leg].items()} for leg in LEGS}
        for k in sorted({c for (tag, c) in t["dense"] if tag == "fwd"}):
            fd, fb = t["dense"].get(("fwd", k), 0.0), t["block"].get(("fwd", k), 0.0)
            dd, db = t["dense"].get(("dgrad", k), 0.0), t["block"].get(("dgrad", k), 0.0)
            if k in on:
                rows.append({"level": level, "conv": k, "kept": kept[k], "fwd_dense_ms": fd, "fwd_block_ms": fb, "dgrad_dense_ms": dd,
                             "dgrad_block_ms": db, "dgrad_on": k in don,
                             "spread_pct": [sp["dense"].get(("fwd", k), 0.0), sp["block"].get(("fwd", k), 0.0),
                                            sp["dense"].get(("dgrad", k), 0.0), sp["block"].get(("dgrad", k), 0.0)]})
            print("%-6s %7s %9.3f %9.3f %6.2f %9.3f %9.3f %6.2f   %.1f / %.1f, %.1f / %.1f%s"
                  % ("conv%d" % k, "%.3f" % kept[k] if k in kept else "-", fd, fb, fd / fb if fb else 0.0, dd, db, dd / db if db else 0.0,
                     sp["dense"].get(("fwd", k), 0.0), sp["block"].get(("fwd", k), 0.0), sp["dense"].get(("dgrad", k), 0.0),
                     sp["block"].get(("dgrad", k), 0.0),
                     "" if k in don else ("  (dgrad: the same launch in both legs)" if k in on else "  (the same launches in both legs)")))
        tot = {leg: {tag: sum(v for (tg, _), v in t[leg].items() if tg == tag) for tag in ("fwd", "dgrad", "wgrad", "lists")} for leg in LEGS}
        print("sums (ms): " + "; ".join("%s: fwd %.3f dgrad %.3f wgrad %.3f lists %.3f" % (leg, tot[leg]["fwd"], tot[leg]["dgrad"],
                                                                                       tot[leg]["wgrad"], tot[leg]["lists"]) for leg in LEGS))
        for leg in LEGS:
            print("whole step B=%d, %d steps per window, %-6s %s ms, median %.3f (spread %.2f %%)"
                  % (B, K, leg + ":", ["%.3f" % v for v in step_ms[leg]], median(step_ms[leg]), spread(step_ms[leg])))
        pairs = [a / b for a, b in zip(step_ms["dense"], step_ms["block"])]
        print("pairs dense / block: %s; parameters finite: %s\n" % (["%.3f" % p for p in pairs], finite))
        wholes.append({"level": level, "fwd_layers": on, "dgrad_layers": don, "step_ms": step_ms,
                       "step_ms_median": {leg: median(step_ms[leg]) for leg in LEGS},
                       "step_spread_pct": {leg: spread(step_ms[leg]) for leg in LEGS}, "dense_over_block": pairs,
                       "launch_ms_sums": tot, "lists_ms_per_step": tot["block"]["lists"], "finite": finite})
        if wgrad_json:
            select(WGRAD_LEG)
            step()
            torch.cuda.synchronize()
            eng = engine()
            won, wkept = list(eng.bsparse_train_wgrad_layers), dict(eng.bsparse_train_wgrad_kept)
            wfinite = all(bool(torch.isfinite(p).all()) for p in m.parameters())
            print("weight gradient on the list launch (conv numbers): %s" % won)
            print("%-6s %7s %9s %9s %6s   spread %% (dense / list)" % ("conv", "kept", "wgr d ms", "wgr l ms", "d/l"))
            for k in won:
                wd, wl = t["block"].get(("wgrad", k), 0.0), t[WGRAD_LEG].get(("wgrad", k), 0.0)
                wrows.append({"level": level, "conv": k, "kept": wkept[k], "wgrad_dense_ms": wd, "wgrad_list_ms": wl,
                              "spread_pct": [sp["block"].get(("wgrad", k), 0.0), sp[WGRAD_LEG].get(("wgrad", k), 0.0)]})
                print("%-6s %7.3f %9.3f %9.3f %6.2f   %.1f / %.1f" % ("conv%d" % k, wkept[k], wd, wl, wd / wl if wl else 0.0,
                                                                     wrows[-1]["spread_pct"][0], wrows[-1]["spread_pct"][1]))
            print("pairs block / block-wgrad: %s; dense / block-wgrad: %s; parameters finite: %s\n"
                  % (["%.3f" % (a / b) for a, b in zip(step_ms["block"], step_ms[WGRAD_LEG])],
                     ["%.3f" % (a / b) for a, b in zip(step_ms["dense"], step_ms[WGRAD_LEG])], wfinite))
            wwholes.append({"level": level, "wgrad_layers": won, "step_ms": step_ms,
                            "step_ms_median": {leg: median(step_ms[leg]) for leg in LEGS},
                            "step_spread_pct": {leg: spread(step_ms[leg]) for leg in LEGS},
                            "wgrad_ms_sums": {leg: tot[leg]["wgrad"] for leg in LEGS}, "finite": wfinite})
        del m, opt, eng
        torch.cuda.empty_cache()

    const, per = policy(rows)
    print("policy (conv9 .. conv22, forward and dgrad of every layer >= %.2f x dense): max kept %.3f; per level %s"
          % (POLICY_GAIN, const, {k: "%.3f: %.2f (conv%d %s)%s" % (v["kept"], v["min_gain"], v["min_gain_conv"], v["min_gain_launch"],
                                                                  "" if v["passes"] else " -") for k, v in per.items()}))
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"B": B, "steps_per_window": K, "levels": levels, "per_layer": True, "precision": "fp16", "layers": rows,
                       "whole_step": wholes, "policy_gain": POLICY_GAIN, "policy_layers": list(POLICY_LAYERS), "max_kept": const,
                       "levels_table": per}, f, indent=1)
    if wgrad_json:
        wconst, wper = wgrad_policy(wrows)
        print("weight-gradient policy (conv9 .. conv22, the list launch of every chosen layer >= %.2f x the dense launch): max kept "
              "%.3f; per level %s" % (POLICY_GAIN, wconst, {k: "%.3f: %.2f (conv%d)%s" % (v["kept"], v["min_gain"], v["min_gain_conv"],
                                                                                        "" if v["passes"] else " -")
                                                            for k, v in wper.items()}))
        with open(wgrad_json, "w") as f:
            json.dump({"B": B, "steps_per_window": K, "levels": levels, "per_layer": True, "precision": "fp16", "layers": wrows,
                       "whole_step": wwholes, "policy_gain": POLICY_GAIN, "policy_layers": list(POLICY_LAYERS),
                       "wgrad_max_kept": wconst, "levels_table": wper}, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
