"""Taylor-importance pruning (modelcompression_amd/importance.py, csrc/taylor.hip) of YOLOv2-VOC on synthetic
weights and images: what the per-step accumulation costs, and what the ranking does to the loss right after pruning.

  time     the training step of train() (forward, RegionLoss, backward, StepGuard, fused SGD) at 416x416 in the default
           training precision, without and with TaylorImportance.accumulate(skip=guard.found) between StepGuard.decide and
           optimizer.step(), and the accumulate launch alone (all three granularities, and the weight scores alone).  The
           leg without the call is the step as it was before this tool existed.  The legs alternate in one process, ROUNDS
           rounds; each sample is a window of STEPS calls after its own warm-up with a device synchronise only around the
           window (host clock).  Quoted: the median of the samples and their spread, and the launch's GB/s against the
           bytes it has to move: w and g read, acc_w read and written (16 bytes per weight; the block and filter
           accumulators are 0.03 % of that and are not counted).
  quality  the seeded random-init model scored for STEPS batches of synthetic images (forward, RegionLoss, backward, no
           optimizer step), then pruned once per granularity and percentage by Taylor importance and by its magnitude twin
           (weight_prune, block_prune, quick_filter_prune) from the same dense weights; quoted is the region loss on
           held-out images right after pruning, NO retraining, forward on batch statistics (the running statistics of a
           random-init model mean nothing).  Also the fraction of weight scores that are exactly 0 (fp32 underflow of
           (g w)^2).  A network without trained structure: an error level, NOT an mAP claim.

usage: python tools/taylor_bench.py time [batch] [steps per window] [--json]
       python tools/taylor_bench.py quality [batch] [scoring steps] [--json]
--json merges the mode's result into profiles/taylor_bench.json."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
JSON_PATH = os.path.join(ROOT, "profiles", "taylor_bench.json")
ROUNDS = 5
PERCENTAGES = {"weight": (50, 80), "block": (50, 75), "filter": (40, 60)}


def parse(argv):
    if not argv or argv[0] not in ("time", "quality"):
        raise SystemExit(__doc__)
    args = [a for a in argv[1:] if not a.startswith("--")]
    a0 = int(args[0]) if len(args) > 0 else (64 if argv[0] == "time" else 16)
    a1 = int(args[1]) if len(args) > 1 else (20 if argv[0] == "time" else 8)
    if a0 < 1 or a1 < 1:
        raise SystemExit("taylor_bench: batch and step counts must be positive")
    return argv[0], a0, a1, "--json" in argv


def targets(B, torch, seed=3):
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(B, 250)
    for b in range(B):                      # 3 boxes per image: [cls, x, y, w, h]
        for k in range(3):
            t[b, 5 * k:5 * k + 5] = torch.tensor([float(torch.randint(0, 20, (1,), generator=g)),
                                                  *(0.2 + 0.6 * torch.rand(2, generator=g)).tolist(),
                                                  *(0.1 + 0.3 * torch.rand(2, generator=g)).tolist()])
    return t


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def spread(v):
    return 100.0 * (max(v) - min(v)) / min(v)


def save(key, doc):
    old = {}
    if os.path.exists(JSON_PATH):
        with open(JSON_PATH) as f:
            old = json.load(f)
    old[key] = doc
    os.makedirs(os.path.dirname(JSON_PATH), exist_ok=True)
    with open(JSON_PATH, "w") as f:
        json.dump(old, f, indent=1)
        f.write("\n")


def run_time(B, K, want_json):
    import torch
    from modelcompression_amd import nets, YOLOV2_VOC_CFG
    from modelcompression_amd.importance import TaylorImportance
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    from modelcompression_amd.train import StepGuard
    dev = torch.device("cuda", 0)
    model = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev).train()
    x, target = synthetic_batch(B, 416, 416, seed=1, device=dev), targets(B, torch).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=1e-5, momentum=0.9, dampening=0, weight_decay=0.0005 * B, fused=True)
    guard = StepGuard(model, opt, dev)
    imp_all = TaylorImportance(model)
    imp_w = TaylorImportance(model, block=False, filter=False)
    nweights = sum(p.numel() for p in imp_all.params)
    launch_bytes = 16 * nweights

    def step(imp):
        loss = model.loss(model(x), target)
        opt.zero_grad()
        loss.backward()
        guard.decide(loss)
        if imp is not None:
            imp.accumulate(skip=guard.found)
        opt.step()

    step(None)                                 # gradients exist from here on (views of one persistent buffer)
    legs = {
        "step plain": lambda: step(None),
        "step + accumulate (all)": lambda: step(imp_all),
        "step + accumulate (weight)": lambda: step(imp_w),
        "accumulate alone (all)": imp_all.accumulate,
        "accumulate alone (weight)": imp_w.accumulate,
    }
    ms = {name: [] for name in legs}
    for _ in range(ROUNDS):                        # alternated: the legs see the same host / GPU conditions
        for name, fn in legs.items():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / K)
            try:
                guard.finish()                     # a non-finite loss is reported one step late: attribute it to its leg
            except FloatingPointError:
                raise SystemExit("taylor_bench: non-finite training loss in leg %r" % name)
    guard.finish()
    print("YOLOv2-VOC 416x416, B=%d, %d calls per window, %d rounds, %d steps skipped by StepGuard, %d weights, %d segments, "
          "%d workgroups; ms per call: median (min .. max, spread)"
          % (B, K, ROUNDS, guard.skipped, nweights, imp_all._table.nseg, imp_all._table.workgroups))
    for name, v in ms.items():
        print("%-28s %8.3f (%.3f .. %.3f, %.2f %%)" % (name, median(v), min(v), max(v), spread(v)))
    plain = median(ms["step plain"])
    gbs = {}
    for kind in ("all", "weight"):
        alone = median(ms["accumulate alone (%s)" % kind])
        gbs[kind] = launch_bytes / (alone * 1e-3) / 1e9
        print("accumulate (%s) adds %.3f ms to the %.3f ms step (%.2f %%); alone it takes %.3f ms = %.0f GB/s of the %.1f MB "
              "it has to move" % (kind, median(ms["step + accumulate (%s)" % kind]) - plain, plain,
                                  100 * (median(ms["step + accumulate (%s)" % kind]) - plain) / plain, alone, gbs[kind],
                                  launch_bytes / 1e6))
    if want_json:
        save("time", {"B": B, "calls_per_window": K, "rounds": ROUNDS, "skipped_steps": guard.skipped, "weights": nweights,
                      "segments": imp_all._table.nseg, "workgroups": imp_all._table.workgroups, "launch_bytes": launch_bytes,
                      "ms_per_call": ms, "median_ms": {k: median(v) for k, v in ms.items()},
                      "spread_percent": {k: spread(v) for k, v in ms.items()}, "launch_GBps": gbs,
                      "scoring_steps_accumulated": imp_all.steps()})


def run_quality(B, steps, want_json):
    import torch
    from modelcompression_amd import nets, YOLOV2_VOC_CFG
    from modelcompression_amd.importance import TaylorImportance, taylor_prune
    from modelcompression_amd.pruning.weightPruning.methods import weight_prune, block_prune, quick_filter_prune
    from modelcompression_amd.pruning.weightPruning.utils import prune_rate
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    dev = torch.device("cuda", 0)
    model = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev).train()
    convs = [p for p in model.parameters() if p.dim() == 4]
    dense = [p.data.clone() for p in convs]
    held = [(synthetic_batch(B, 416, 416, seed=100 + i, device=dev), targets(B, torch, seed=200 + i).to(dev)) for i in range(2)]

    def held_out_loss():
        with torch.no_grad():
            return sum(float(model.loss(model(x), t)) for x, t in held) / len(held)

    imp = TaylorImportance(model)
    for s in range(steps):
        x, t = synthetic_batch(B, 416, 416, seed=10 + s, device=dev), targets(B, torch, seed=50 + s).to(dev)
        model.zero_grad()
        model.loss(model(x), t).backward()
        imp.accumulate()
    model.zero_grad()
    scores = imp.weight_scores()
    zero = sum(int((a == 0).sum()) for a in scores) / sum(a.numel() for a in scores)
    base = held_out_loss()
    print("B=%d, %d scoring steps accumulated (%d asked); dense held-out region loss %.5g; weight scores exactly 0: %.4f %%"
          % (B, imp.steps(), steps, base, 100 * zero))
    twins = {"weight": weight_prune, "block": block_prune, "filter": quick_filter_prune}
    rows = []
    for gran, percs in PERCENTAGES.items():
        for perc in percs:
            row = {"granularity": gran, "percent": perc}
            for name in ("magnitude", "taylor"):
                for p, w in zip(convs, dense):          # from the same dense weights, with no mask left from the last run
                    p.data.copy_(w)
                model.set_masks([torch.ones_like(w) for w in dense])
                masks = twins[gran](model, perc) if name == "magnitude" else taylor_prune(model, perc, imp, gran)
                model.set_masks(masks)
                row[name] = {"pruned_percent": float(prune_rate(model, False)), "held_out_loss": held_out_loss()}
            rows.append(row)
            print("%-6s %3d %%: held-out region loss right after pruning  magnitude %.5g (%.1f %% of the weights pruned)   "
                  "taylor %.5g (%.1f %%)   dense %.5g"
                  % (gran, perc, row["magnitude"]["held_out_loss"], row["magnitude"]["pruned_percent"],
                     row["taylor"]["held_out_loss"], row["taylor"]["pruned_percent"], base))
    if want_json:
        save("quality", {"B": B, "scoring_steps": imp.steps(), "dense_held_out_loss": base,
                         "weight_scores_exactly_zero_percent": 100 * zero, "rows": rows,
                         "note": "random-init network, synthetic images, no retraining: an error level, not mAP"})


def main(argv):
    import torch
    what, a0, a1, want_json = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("taylor_bench needs the GPU")
    (run_time if what == "time" else run_quality)(a0, a1, want_json)


if __name__ == "__main__":
    main(sys.argv[1:])
