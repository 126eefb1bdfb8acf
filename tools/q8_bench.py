"""fp8 against fp16 inference of the same YOLOv2-VOC (synthetic weights): eval, B=128 at 416x416.
Prints the per-layer forward kernel times of both engines (HIP events around every launch, median of the instrumented
passes; the cast pass of the fp16 -> fp8 edge is charged to its block), the whole forward of both engines alternated --
three pairs of windows of at least 100 forwards each -- and the logits rel-L2 between them.
usage: python tools/q8_bench.py [batch] [forwards per window] [--json PATH]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv):
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--json")]
    B = int(args[0]) if len(args) > 0 else 128
    K = int(args[1]) if len(args) > 1 else 100
    out_json = argv[argv.index("--json") + 1] if "--json" in argv else None
    if B < 1 or K < 1:
        raise SystemExit("q8_bench: batch and forwards per window must be positive")
    return B, K, out_json


def main(argv):
    B, K, out_json = parse(argv)
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

    def engine(prec):
        return [e for k, e in m._engines.items() if k[3] == prec and not e.train_layout][0]

    def layer_times(prec, passes=5):
        eng = engine(prec)
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
        return {k: sorted(v)[len(v) // 2] for k, v in per.items()}

    with torch.no_grad():
        res = {}
        for prec in modes:
            m.precision = prec
            for _ in range(3):
                y = m(x)
            torch.cuda.synchronize()
            res[prec] = {"logits": y.clone(), "layers": layer_times(prec)}
        fp8_layers = list(engine("fp8").fp8_layers)
        rates = {p: [] for p in modes}
        for rep in range(3):                   # alternated: the two engines see the same host / GPU conditions
            for prec in modes:
                m.precision = prec
                for _ in range(5):
                    m(x)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(K):
                    m(x)
                torch.cuda.synchronize()
                rates[prec].append(B * K / (time.perf_counter() - t0))

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


if __name__ == "__main__":
    main(sys.argv[1:])
