"""fp8 against fp16 inference of the same YOLOv2-VOC (synthetic weights): eval, B=128 at 416x416.
Prints the per-layer forward kernel times of both engines (HIP events around every launch, median of the instrumented
passes; the cast pass of the fp16 -> fp8 edge is charged to its block), the whole forward of both engines alternated --
three pairs of windows of at least 100 forwards each -- and the logits rel-L2 between them.
--sparse: the model is nm_prune'd (2:4 masks) and four engines are measured the same way on the same masked weights: fp16,
fp16 with sparse = "2:4", fp8 and fp8-2:4 (windows alternated over all four).
--slim PCT: the model is quick_filter_prune(PCT)'d and slim_export'ed; the slim model is measured in fp16 (its
unfused border path) and fp8 the same way, and the table names per layer cin -> round_up(cin, 64), which blocks are fp8
blocks (`slim`: on mcamd_conv_fwd_q8_slim, `table`: with a border table) and the time of each cast pass.  Run it once
without and once with MCAMD_Q8_MFMA=1 for the two forms of the fp8 kernel.
--w4: "fp8" against "fp8-w4" (4-bit weights) on the same weights, the two alternated in one process, with the
resident weight-operand bytes of the fp8 blocks under both -- once per MCAMD_Q8_MFMA form, each form in a child process of its
own started with that switch; the merged report goes to profiles/q8_w4_bench.json unless --json names another file.
usage: python tools/q8_bench.py [batch] [forwards per window] [--sparse | --slim PCT | --w4] [--json PATH]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv):
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--json", "--slim"))]
    B = int(args[0]) if len(args) > 0 else 128
    K = int(args[1]) if len(args) > 1 else 100
    out_json = argv[argv.index("--json") + 1] if "--json" in argv else None
    slim_pct = float(argv[argv.index("--slim") + 1]) if "--slim" in argv else None
    if B < 1 or K < 1:
        raise SystemExit("q8_bench: batch and forwards per window must be positive")
    if slim_pct is not None and ("--sparse" in argv or not 0.0 < slim_pct < 100.0):
        raise SystemExit("q8_bench: --slim takes a percentage in (0, 100) and does not combine with --sparse")
    if "--w4" in argv and ("--sparse" in argv or slim_pct is not None):
        raise SystemExit("q8_bench: --w4 does not combine with --sparse or --slim")
    return B, K, out_json, "--sparse" in argv, slim_pct


def main(argv):
    B, K, out_json, sparse, slim_pct = parse(argv)
    w4 = "--w4" in argv
    if w4 and "--w4-form" not in argv:
        return run_w4_forms(argv, B, K, out_json)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("q8_bench needs the GPU")
    from modelcompression_amd import nets, YOLOV2_VOC_CFG
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    dev = torch.device("cuda", 0)
    m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev)
    m.eval()
    x = synthetic_batch(B, 416, 416, seed=0, device=dev)
    modes = ("fp16", "fp8")
    if slim_pct is not None:
        import tempfile
        from modelcompression_amd import slim
        from modelcompression_amd.pruning.weightPruning.methods import quick_filter_prune
        m.set_masks(quick_filter_prune(m, slim_pct))
        with tempfile.TemporaryDirectory() as tmp:
            m = slim.slim_export(m, os.path.join(tmp, "slim.cfg"))
    if sparse:
        from modelcompression_amd.pruning.weightPruning.methods import nm_prune
        m.set_masks(nm_prune(m))
        modes = ("fp16", "fp16+2:4", "fp8", "fp8-2:4")
    if w4:
        modes = ("fp8", "fp8-w4")

    def select(mode):
        m.precision, m.sparse = mode.split("+")[0], "2:4" if mode.endswith("+2:4") else None

    def engine(mode):
        return [e for k, e in m._engines.items() if k[3] == mode.split("+")[0] and not e.train_layout][0]

    def layer_times(prec, passes=5, only=None):
        """conv number -> median ms of the block's launches (`only`: of the launches with that tag, e.g. 'cast')"""
        eng = engine(prec)
        per = {}
        for _ in range(passes):
            eng.events = []
            m(x)
            torch.cuda.synchronize()
            once = {}
            for tag, lay, e0, e1, _host in eng.events:
                if only is None or tag == only:
                    once[lay.li + 1] = once.get(lay.li + 1, 0.0) + e0.elapsed_time(e1)
            for k, v in once.items():
                per.setdefault(k, []).append(v)
            eng.events = None
        return {k: sorted(v)[len(v) // 2] for k, v in per.items()}

    def measure():
        res = {}
        for prec in modes:
            select(prec)
            for _ in range(3):
                y = m(x)
            torch.cuda.synchronize()
            res[prec] = {"logits": y.clone(), "layers": layer_times(prec)}
            if slim_pct is not None and prec == "fp8":
                res[prec]["casts"] = layer_times(prec, only="cast")
            if prec == "fp16+2:4":
                sparse_layers = list(engine(prec).sparse_layers)
        fp8_layers = list(engine("fp8").fp8_layers)
        rates = {p: [] for p in modes}
        for rep in range(3):                   # alternated: the two engines see the same host / GPU conditions
            for prec in modes:
                select(prec)
                for _ in range(5):
                    m(x)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(K):
                    m(x)
                torch.cuda.synchronize()
                rates[prec].append(B * K / (time.perf_counter() - t0))
        return res, rates, fp8_layers, sparse_layers if sparse else None

    if w4:                                     # (one MFMA form: the caller's MCAMD_Q8_MFMA, as in every other mode)
        from modelcompression_amd.engine import _FORMS
        with torch.no_grad():
            res, rates, fp8_layers, _ = measure()
        nbytes = {p: sum(getattr(lay, name).numel() * getattr(lay, name).element_size()
                         for lay in engine(p).layers if lay.li + 1 in fp8_layers for name, _ in _FORMS[lay.form].bufs) for p in modes}
        return report_w4(B, K, out_json, os.environ.get("MCAMD_Q8_MFMA", "0"), res, rates, fp8_layers,
                         list(engine("fp8-w4").fp8_w4_layers), nbytes)
    with torch.no_grad():
        res, rates, fp8_layers, sparse_layers = measure()

    if slim_pct is not None:
        return report_slim(B, K, out_json, slim_pct, engine("fp8"), res, rates)
    if sparse:
        return report_sparse(B, K, out_json, modes, res, rates, fp8_layers, list(engine("fp8-2:4").fp8_sparse_layers), sparse_layers)
    d, s = res["fp16"], res["fp8"]
    rel = float((s["logits"].double() - d["logits"].double()).norm() / d["logits"].double().norm())
    print("fp8 layers (conv numbers): %s" % fp8_layers)
    print("%-6s %10s %10s %7s" % ("conv", "fp16 ms", "fp8 ms", "ratio"))
    for k in sorted(d["layers"]):
        dm, sm = d["layers"][k], s["layers"].get(k, float("nan"))
        print("%-6s %10.3f %10.3f %7.2f%s" % ("conv%d" % k, dm, sm, dm / sm, "" if k in fp8_layers else "  (fp16)"))
    td, ts = sum(d["layers"].values()), sum(s["layers"].values())
    print("%-6s %10.3f %10.3f %7.2f" % ("sum", td, ts, td / ts))
    pairs = [b / a for a, b in zip(rates["fp16"], rates["fp8"])]
    print("whole forward B=%d, %d forwards per window: fp16 %s img/s, fp8 %s img/s, pairs fp8 / fp16 %s"
          % (B, K, ["%.0f" % r for r in rates["fp16"]], ["%.0f" % r for r in rates["fp8"]], ["%.3f" % p for p in pairs]))
    print("logits rel-L2 (fp8 vs fp16 engine, same weights): %.3e" % rel)
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"B": B, "forwards_per_window": K, "fp8_layers": fp8_layers, "fp16_ms": d["layers"], "fp8_ms": s["layers"],
                       "fp16_img_s": rates["fp16"], "fp8_img_s": rates["fp8"], "pairs": pairs, "rel_l2": rel}, f, indent=1)


def run_w4_forms(argv, B, K, out_json):
    """--w4: one child process per MCAMD_Q8_MFMA form (the library reads the switch once per process), their reports merged."""
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {"B": B, "forwards_per_window": K, "forms": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for mfma in ("0", "1"):
            part = os.path.join(tmp, "form%s.json" % mfma)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), str(B), str(K), "--w4", "--w4-form", "--json", part],
                               env=dict(os.environ, MCAMD_Q8_MFMA=mfma))
            if r.returncode != 0:
                raise SystemExit("q8_bench --w4: the MCAMD_Q8_MFMA=%s run failed (exit %d)" % (mfma, r.returncode))
            with open(part) as f:
                out["forms"][mfma] = json.load(f)
    out_json = out_json or os.path.join(root, "profiles", "q8_w4_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(out, f, indent=1)


def report_w4(B, K, out_json, mfma, res, rates, fp8_layers, w4_layers, nbytes):
    d, s = res["fp8"], res["fp8-w4"]
    rel = float((s["logits"].double() - d["logits"].double()).norm() / d["logits"].double().norm())
    print("MCAMD_Q8_MFMA=%s; fp8 layers %s; w4 layers %s" % (mfma, fp8_layers, w4_layers))
    print("%-6s %10s %10s %9s" % ("conv", "fp8 ms", "fp8-w4 ms", "w4 / fp8"))
    for k in sorted(d["layers"]):
        dm, sm = d["layers"][k], s["layers"].get(k, float("nan"))
        print("%-6s %10.3f %10.3f %9.2f%s" % ("conv%d" % k, dm, sm, sm / dm, "" if k in w4_layers else "  (not w4)"))
    td, ts = sum(d["layers"].values()), sum(s["layers"].values())
    print("%-6s %10.3f %10.3f %9.2f" % ("sum", td, ts, ts / td))
    for p in ("fp8", "fp8-w4"):
        r = rates[p]
        print("whole forward B=%d, %d forwards per window, %-7s %s img/s (spread %.2f %%)"
              % (B, K, p + ":", ["%.0f" % v for v in r], 100.0 * (max(r) - min(r)) / min(r)))
    pairs = [b / a for a, b in zip(rates["fp8"], rates["fp8-w4"])]
    print("pairs fp8-w4 / fp8 (img/s): %s" % ["%.3f" % p for p in pairs])
    print("resident weight-operand bytes of the fp8 blocks: fp8 %d, fp8-w4 %d (%.4f x)"
          % (nbytes["fp8"], nbytes["fp8-w4"], nbytes["fp8-w4"] / nbytes["fp8"]))
    print("logits rel-L2 (fp8-w4 vs fp8 engine, same weights): %.3e" % rel)
    sys.stdout.flush()
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"fp8_layers": fp8_layers, "fp8_w4_layers": w4_layers, "fp8_ms": d["layers"], "fp8_w4_ms": s["layers"],
                       "fp8_img_s": rates["fp8"], "fp8_w4_img_s": rates["fp8-w4"], "pairs_w4_over_fp8": pairs,
                       "weight_operand_bytes": nbytes, "rel_l2_w4_vs_fp8": rel}, f, indent=1)


def report_slim(B, K, out_json, pct, eng, res, rates):
    d, s = res["fp16"], res["fp8"]
    rel = float((s["logits"].double() - d["logits"].double()).norm() / d["logits"].double().norm())
    mfma = os.environ.get("MCAMD_Q8_MFMA", "0")
    fp8_layers = list(eng.fp8_layers)
    print("slim %g %%, MCAMD_Q8_MFMA=%s; fp8 layers (conv numbers): %s" % (pct, mfma, fp8_layers))
    print("%-6s %5s %8s %10s %10s %9s %7s  %s" % ("conv", "cin", "cin_pad", "fp16 ms", "fp8 ms", "(cast ms)", "ratio", "block"))
    rows = []
    for lay in eng.layers:
        k = lay.li + 1
        dm, sm, cm = d["layers"].get(k, float("nan")), s["layers"].get(k, float("nan")), s["casts"].get(k)
        on = k in fp8_layers
        kind = "fp16" if not on else "fp8" + (" slim" if lay.q8_slim else "") + (" table" if lay.border is not None else "")
        if not on and lay.border is not None:
            kind += " table (unfused)"
        cp = (lay.cin + 63) // 64 * 64 if on else lay.cin
        rows.append({"conv": k, "cin": lay.cin, "cin_pad": cp, "cout": lay.cout, "fp16_ms": dm, "fp8_ms": sm, "cast_ms": cm, "block": kind})
        print("%-6s %5d %8d %10.3f %10.3f %9s %7.2f  %s" % ("conv%d" % k, lay.cin, cp, dm, sm, "" if cm is None else "%.3f" % cm, dm / sm, kind))
    td, ts = sum(d["layers"].values()), sum(s["layers"].values())
    print("%-6s %5s %8s %10.3f %10.3f %9.3f %7.2f" % ("sum", "", "", td, ts, sum(s["casts"].values()), td / ts))
    for p in ("fp16", "fp8"):
        r = rates[p]
        print("whole forward B=%d, %d forwards per window, %-5s %s img/s (spread %.2f %%)"
              % (B, K, p + ":", ["%.0f" % v for v in r], 100.0 * (max(r) - min(r)) / min(r)))
    pairs = [b / a for a, b in zip(rates["fp16"], rates["fp8"])]
    print("pairs fp8 / fp16: %s" % ["%.3f" % p for p in pairs])
    print("logits rel-L2 (fp8 vs fp16 engine, same slim weights): %.3e" % rel)
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"B": B, "forwards_per_window": K, "slim_pct": pct, "mfma": mfma, "fp8_layers": fp8_layers, "layers": rows,
                       "fp16_img_s": rates["fp16"], "fp8_img_s": rates["fp8"], "pairs": pairs, "rel_l2": rel}, f, indent=1)


def report_sparse(B, K, out_json, modes, res, rates, fp8_layers, fp8_sparse_layers, sparse_layers):
    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())
    print("2:4 fp16 layers: %s\nfp8 layers: %s\n2:4 fp8 layers: %s" % (sparse_layers, fp8_layers, fp8_sparse_layers))
    print("%-6s " % "conv" + " ".join("%12s" % (p + " ms") for p in modes) + "  fp8-2:4: /fp8  /fp16+2:4  /fp16")
    ms = {p: res[p]["layers"] for p in modes}
    for k in sorted(ms["fp16"]):
        t = [ms[p].get(k, float("nan")) for p in modes]
        print("%-6s " % ("conv%d" % k) + " ".join("%12.3f" % v for v in t)
              + "  %12.2f %10.2f %6.2f" % (t[2] / t[3], t[1] / t[3], t[0] / t[3]))
    tot = [sum(ms[p].values()) for p in modes]
    print("%-6s " % "sum" + " ".join("%12.3f" % v for v in tot) + "  %12.2f %10.2f %6.2f" % (tot[2] / tot[3], tot[1] / tot[3], tot[0] / tot[3]))
    for p in modes:
        r = rates[p]
        print("whole forward B=%d, %d forwards per window, %-9s %s img/s (spread %.2f %%)"
              % (B, K, p + ":", ["%.0f" % v for v in r], 100.0 * (max(r) - min(r)) / min(r)))
    pairs = {q: [b / a for a, b in zip(rates[q], rates["fp8-2:4"])] for q in modes[:3]}
    for q in modes[:3]:
        print("pairs fp8-2:4 / %s: %s" % (q, ["%.3f" % v for v in pairs[q]]))
    rels = {p: rel(res[p]["logits"], res["fp16"]["logits"]) for p in modes[1:]}
    print("logits rel-L2 against the fp16 engine (same masked weights): %s" % {p: "%.3e" % v for p, v in rels.items()})
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"B": B, "forwards_per_window": K, "mfma": os.environ.get("MCAMD_Q8_MFMA", "0"), "modes": list(modes),
                       "sparse_layers": sparse_layers, "fp8_layers": fp8_layers, "fp8_sparse_layers": fp8_sparse_layers,
                       "ms": ms, "img_s": rates, "pairs_fp8_2_4_over": pairs, "rel_l2_vs_fp16": rels}, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
