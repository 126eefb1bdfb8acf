"""Retraining low-rank layers in factored form (lowrank.FactorSGD, csrc/lowrank_train.hip) of YOLOv2-VOC on
synthetic weights: what the factor step costs behind the dense "fp16" training step, and what 100 factored steps do to the
error of the factored eval engine.

  time      one fwd + RegionLoss + bwd + SGD step at 416x416 in "fp16" without and with FactorSGD.step at ranks 64, 128 and
            256, on every block lowrank_factor's rule accepts at that rank, alternated in one process (three rounds, each window
            after its own warm-up, ended by a device synchronise).  Then the library call alone (HIP events around 20 calls) and
            its achieved fp32 rate, counted as 3 * 2 * sum(Cout K r), against the MI355X's fp32 matrix peak of 157.3 TFLOP/s (AMD
            Instinct MI355X data sheet), and the dense weight-gradient launches of the same blocks from one instrumented step
            (1x1 blocks whose weight gradient is part of the fused backward launch have no launch of their own: left out and
            counted).  The factors of this mode are seeded Gaussians of the weights' scale, not an SVD: a time does not depend
            on the values, and three float64 SVD passes over the model cost minutes of device time.
  accuracy  the seeded random-init model, lowrank_factor(energy=0.8), 100 factored steps toward the unfactored model's fp16
            logits (sum of squares / batch; SGD, momentum 0.9): rel-L2 of the lowrank = True eval logits to those logits before
            and after, on the training images and on held-out ones.  A RANDOM-INIT network without trained structure on
            synthetic images: an error level, NOT an mAP claim.

usage: python tools/lowrank_train_bench.py time [batch] [steps per window] [--json PATH]
       python tools/lowrank_train_bench.py accuracy [batch] [steps] [--json PATH]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.q8_qat_bench import parse, targets, spread  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12
RANKS = (64, 128, 256)


def gaussian_factors(model, r, torch):
    """One (U, V) or None per conv block by lowrank_factor's acceptance rule (inner BatchNorm block, r <= min(Cout, K),
    r (K + Cout) < K Cout), with seeded Gaussian entries whose product has the weight's scale."""
    from modelcompression_amd.lowrank import _inner_bn
    g, out = torch.Generator().manual_seed(r), []
    for i, conv, ok in _inner_bn(model):
        w = conv.weight.data
        cout, K = w.shape[0], w[0].numel()
        if not ok or r > min(cout, K) or r * (K + cout) >= K * cout:
            out.append(None)
            continue
        s = (float(w.std()) / r ** 0.5) ** 0.5
        out.append((s * torch.randn((r,) + tuple(w.shape[1:]), generator=g), s * torch.randn(cout, r, generator=g)))
    return out


def run_time(B, K, out_json):
    import torch
    from modelcompression_amd import nets, YOLOV2_VOC_CFG, lowrank
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    dev = torch.device("cuda", 0)
    x, target = synthetic_batch(B, 416, 416, seed=1, device=dev), targets(B, torch).to(dev)
    m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev).train()
    m.precision = "fp16"
    opt = torch.optim.SGD(m.parameters(), lr=1e-6 / B, momentum=0.9, weight_decay=0.0005 * B, fused=True)
    lr = 1e-6 / B

    def step(fs):
        out = m(x)
        loss = m.loss(out, target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if fs is not None:
            fs.step(lr)
        return loss

    def window(fs):
        for _ in range(5):
            step(fs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            step(fs)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / K

    result = {"B": B, "steps_per_window": K, "peak_fp32_matrix_tflops": PEAK_FP32_MATRIX / 1e12, "ranks": {}}
    for r in RANKS:
        m.set_factors(gaussian_factors(m, r, torch))
        fs = lowrank.FactorSGD(m, momentum=0.9, weight_decay=0.0005 * B)
        ms = {"dense": [], "factored": []}
        for rep in range(3):                       # alternated: the legs see the same host / GPU conditions
            ms["dense"].append(window(None))
            ms["factored"].append(window(fs))      # (fs owns its weights: the stale W of the dense windows is overwritten)
        # the library call alone
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fs._table.step(lr, 0.9, 0.0005 * B)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            fs._table.step(lr, 0.9, 0.0005 * B)
        e1.record()
        torch.cuda.synchronize()
        call_ms = e0.elapsed_time(e1) / 20
        flops = sum(3 * 2 * c.weight.shape[0] * c.weight[0].numel() * r for _, c in fs.blocks)
        # the dense weight-gradient launches of the same blocks, one instrumented step
        eng = [e for k, e in m._engines.items() if e.train_layout][0]
        eng.events = []
        step(None)
        torch.cuda.synchronize()
        own = {i for i, _ in fs.blocks}
        wgrad = {}
        for tag, lay, a, b, _host in eng.events:
            if tag == "wgrad" and lay.li + 1 in own:
                wgrad[lay.li + 1] = wgrad.get(lay.li + 1, 0.0) + a.elapsed_time(b)
        eng.events = None
        over = [f - d for f, d in zip(ms["factored"], ms["dense"])]
        info = {"blocks": sorted(own), "ms_per_step": ms, "spread_percent": {k: spread(v) for k, v in ms.items()},
                "overhead_ms_pairs": over, "overhead_percent_pairs": [100 * o / d for o, d in zip(over, ms["dense"])],
                "call_ms": call_ms, "call_gflop": flops / 1e9, "call_tflops": flops / call_ms / 1e9,
                "share_of_fp32_matrix_peak": flops / (call_ms * 1e-3) / PEAK_FP32_MATRIX,
                "workspace_bytes": fs._table.workspace.numel() * 4, "workgroups": list(fs._table.workgroups),
                "dense_wgrad_launch_ms_same_blocks": sum(wgrad.values()),
                "blocks_without_a_wgrad_launch_of_their_own": sorted(own - set(wgrad))}
        result["ranks"][str(r)] = info
        print("rank %d, B=%d, %d steps per window, blocks %s" % (r, B, K, sorted(own)))
        for k, v in ms.items():
            print("  %-9s %s ms (spread %.2f %%)" % (k + ":", ["%.3f" % t for t in v], spread(v)))
        print("  overhead per step, pairs: %s ms (%s %%)" % (["%.3f" % o for o in over],
                                                            ["%.2f" % p for p in info["overhead_percent_pairs"]]))
        print("  the call alone: %.3f ms, %.2f GFLOP, %.2f TFLOP/s fp32 = %.1f %% of the matrix peak; dense wgrad launches of "
              "the same blocks: %.3f ms (%d blocks have none of their own)"
              % (call_ms, flops / 1e9, info["call_tflops"], 100 * info["share_of_fp32_matrix_peak"],
                 info["dense_wgrad_launch_ms_same_blocks"], len(info["blocks_without_a_wgrad_launch_of_their_own"])))
        m.set_factors([None] * len(gaussian_factors(m, r, torch)))
    if out_json:
        with open(out_json, "w") as f:
            json.dump(result, f, indent=1)


def run_accuracy(B, steps, out_json):
    import torch
    from modelcompression_amd import nets, YOLOV2_VOC_CFG, lowrank, lowrank_factor
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    dev = torch.device("cuda", 0)
    x, x_held = synthetic_batch(B, 416, 416, seed=1, device=dev), synthetic_batch(B, 416, 416, seed=2, device=dev)

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    def evaluate(m, images, lowrank_on):
        m.eval()
        m.lowrank = lowrank_on
        with torch.no_grad():
            y = m(images).clone()
        m.lowrank = False
        return y

    m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev)
    m.precision = "fp16"
    m.train()
    with torch.no_grad():                  # settle the running statistics on this batch (q8_qat_bench.py accuracy)
        for _ in range(60):
            m(x)
    teacher, teacher_held = evaluate(m, x, False), evaluate(m, x_held, False)
    m.set_factors(lowrank_factor(m, energy=0.8))
    m.lowrank_max_cost, m.lowrank_min_tiles = 1.0, 1
    ranks = {i: c.factor_u.shape[0] for i, c in lowrank.fresh_blocks(m)}
    before, before_held = rel(evaluate(m, x, True), teacher), rel(evaluate(m, x_held, True), teacher_held)
    print("B=%d, energy 0.8, ranks %s: lowrank eval vs the unfactored fp16 logits BEFORE %.4f (held-out %.4f)"
          % (B, ranks, before, before_held))
    runs = []
    state = {k: v.clone() for k, v in m.state_dict().items()}
    for lr in (1e-6, 3e-6, 1e-5):
        m.load_state_dict(state)
        m.set_factors([(c.factor_u, c.factor_v) if getattr(c, "factor_u", None) is not None else None
                       for _, c in lowrank._blocks(m)])
        opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=0.9)
        fs = lowrank.FactorSGD(m, momentum=0.9)
        m.train()
        losses = []
        for it in range(steps):
            loss = ((m(x) - teacher) ** 2).sum() / B
            opt.zero_grad()
            loss.backward()
            opt.step()
            fs.step(lr)
            if it in (0, steps - 1):
                losses.append(float(loss.detach()))
        fresh = all(lowrank.is_fresh(m, c) for _, c in fs.blocks)
        after, held = rel(evaluate(m, x, True), teacher), rel(evaluate(m, x_held, True), teacher_held)
        runs.append({"lr": lr, "steps": steps, "loss_first": losses[0], "loss_last": losses[-1], "after": after,
                     "after_held_out": held, "factors_fresh": fresh})
        print("lr %.0e, %d factored steps: loss %.4g -> %.4g; lowrank eval AFTER %.4f (held-out %.4f); factors fresh: %s"
              % (lr, steps, losses[0], losses[-1], after, held, fresh))
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"B": B, "energy": 0.8, "ranks": ranks, "before": before, "before_held_out": before_held, "runs": runs,
                       "note": "random-init network without trained structure, synthetic images: an error level, NOT an mAP claim"},
                      f, indent=1)


def main(argv):
    import torch
    what, a0, a1, out_json, _ = parse(argv, 64 if argv and argv[0] == "time" else 4, 20 if argv and argv[0] == "time" else 100)
    if not torch.cuda.is_available():
        raise SystemExit("lowrank_train_bench needs the GPU")
    (run_time if what == "time" else run_accuracy)(a0, a1, out_json)


if __name__ == "__main__":
    main(sys.argv[1:])
