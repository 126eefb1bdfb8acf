"""fp8 quantisation-aware training (Darknet.precision = "fp8-qat") of YOLOv2-VOC on synthetic weights: what a
training step costs against the "fp16" engine, and what a short fine-tune does to the fp8 inference error.

  time      one fwd + RegionLoss + bwd + SGD step at 416x416 in "fp16", in "fp8-qat" and in "fp8-qat" with MCAMD_Q8_MFMA=1,
            in alternated windows (three rounds over the three modes, each window after its own warm-up, ended by a device
            synchronise); per-kernel-class times of one instrumented step of each mode (HIP events, one stream).
  accuracy  eval "fp8" logits' rel-L2 to the fp32 oracle (oracle/darknet_ref.py, CPU) before and after a short "fp8-qat"
            fine-tune toward the "fp16" engine's logits of the same images (sum of squares / batch; SGD, momentum 0.9), for
            a few learning rates from the same start.  A RANDOM-INIT network on synthetic images: an error level, not mAP.

--w4 (4-bit quantisation-aware training, Darknet.precision = "fp8-w4-qat"):
  time      the legs are "fp16", "fp8-qat" and "fp8-w4-qat", alternated in one process, three rounds, once per MFMA form
            (MCAMD_Q8_MFMA 0, then 1); the ratios of the new leg to both baselines are reported per round;
  accuracy  the same measurement for both lines from the same run: eval "fp8" before / after an "fp8-qat" fine-tune, and eval
            "fp8-w4" before / after an "fp8-w4-qat" fine-tune -- same images, teacher, learning rates and start.

usage: python tools/q8_qat_bench.py time [batch] [steps per window] [--w4] [--json PATH]
       python tools/q8_qat_bench.py accuracy [batch] [steps] [--w4] [--json PATH]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv, d0, d1):
    if not argv or argv[0] not in ("time", "accuracy"):
        raise SystemExit(__doc__)
    rest = argv[1:]
    args = [a for i, a in enumerate(rest) if not a.startswith("--") and (i == 0 or rest[i - 1] != "--json")]
    a0 = int(args[0]) if len(args) > 0 else d0
    a1 = int(args[1]) if len(args) > 1 else d1
    if a0 < 1 or a1 < 1:
        raise SystemExit("q8_qat_bench: batch and step counts must be positive")
    return argv[0], a0, a1, rest[rest.index("--json") + 1] if "--json" in rest else None, "--w4" in rest


def targets(B, torch):
    g = torch.Generator().manual_seed(3)
    t = torch.zeros(B, 250)
    for b in range(B):                      # 3 boxes per image: [cls, x, y, w, h]
        for k in range(3):
            t[b, 5 * k:5 * k + 5] = torch.tensor([float(torch.randint(0, 20, (1,), generator=g)),
                                                  *(0.2 + 0.6 * torch.rand(2, generator=g)).tolist(),
                                                  *(0.1 + 0.3 * torch.rand(2, generator=g)).tolist()])
    return t


def spread(v):
    return 100.0 * (max(v) - min(v)) / min(v)


def run_time_w4(B, K, out_json):
    """--w4: "fp16", "fp8-qat" and "fp8-w4-qat" alternated, three rounds, once per MFMA form."""
    import torch
    from modelcompression_amd import nets, YOLOV2_VOC_CFG, _lib
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    dev = torch.device("cuda", 0)
    m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev).train()
    x, target = synthetic_batch(B, 416, 416, seed=1, device=dev), targets(B, torch).to(dev)
    opt = torch.optim.SGD(m.parameters(), lr=1e-6 / B, momentum=0.9, weight_decay=0.0005 * B, fused=True)
    legs = ("fp16", "fp8-qat", "fp8-w4-qat")

    def step():
        out = m(x)
        loss = m.loss(out, target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    result = {"B": B, "steps_per_window": K, "legs": list(legs), "forms": {}}
    for mfma in (0, 1):
        os.environ["MCAMD_Q8_MFMA"] = str(mfma)
        _lib.reload_config()
        ms = {p: [] for p in legs}
        for rep in range(3):                   # alternated: the legs see the same host / GPU conditions
            for leg in legs:
                m.precision = leg
                for _ in range(5):
                    step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(K):
                    loss = step()
                torch.cuda.synchronize()
                ms[leg].append(1e3 * (time.perf_counter() - t0) / K)
                assert bool(torch.isfinite(loss)), leg
        eng = [e for k, e in m._engines.items() if k[3] == "fp8-w4-qat" and e.train_layout][0]
        ratios = {base: [a / b for a, b in zip(ms["fp8-w4-qat"], ms[base])] for base in legs[:2]}
        print("MCAMD_Q8_MFMA=%d, B=%d, %d steps per window; w4 layers (conv numbers): %s" % (mfma, B, K, eng.fp8_w4_layers))
        for leg in legs:
            print("  %-11s %s ms (spread %.2f %%)" % (leg + ":", ["%.3f" % v for v in ms[leg]], spread(ms[leg])))
        for base in legs[:2]:
            print("  pairs fp8-w4-qat ms / %s ms: %s" % (base, ["%.3f" % v for v in ratios[base]]))
        result["forms"]["MCAMD_Q8_MFMA=%d" % mfma] = {"ms_per_step": ms, "spread_percent": {p: spread(ms[p]) for p in legs},
                                                      "pairs_w4_qat_over": ratios, "fp8_w4_layers": list(eng.fp8_w4_layers)}
    os.environ["MCAMD_Q8_MFMA"] = "0"
    _lib.reload_config()
    if out_json:
        with open(out_json, "w") as f:
            json.dump(result, f, indent=1)


def run_time(B, K, out_json):
    import torch
    from modelcompression_amd import nets, YOLOV2_VOC_CFG, _lib
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    dev = torch.device("cuda", 0)
    m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev).train()
    x, target = synthetic_batch(B, 416, 416, seed=1, device=dev), targets(B, torch).to(dev)
    opt = torch.optim.SGD(m.parameters(), lr=1e-6 / B, momentum=0.9, weight_decay=0.0005 * B, fused=True)
    modes = ("fp16", "fp8-qat", "fp8-qat+fp8mfma")

    def select(mode):
        m.precision = mode.split("+")[0]
        os.environ["MCAMD_Q8_MFMA"] = "1" if mode.endswith("+fp8mfma") else "0"
        _lib.reload_config()

    def step():
        out = m(x)
        loss = m.loss(out, target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    def classes(mode):
        """Per-kernel-class milliseconds of one instrumented step (per-launch events serialise the two streams)."""
        eng = [e for k, e in m._engines.items() if k[3] == mode.split("+")[0] and e.train_layout][0]
        eng.events = []
        step()
        torch.cuda.synchronize()
        per = {}
        for tag, lay, e0, e1, _host in eng.events:
            key = tag + ("" if getattr(lay, "q8_on", False) and mode != "fp16" else "(fp16 blocks)")
            per[key] = per.get(key, 0.0) + e0.elapsed_time(e1)
        eng.events = None
        return per

    ms, kern = {p: [] for p in modes}, {}
    for mode in modes:
        select(mode)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        kern[mode] = classes(mode)
    for rep in range(3):                       # alternated: the modes see the same host / GPU conditions
        for mode in modes:
            select(mode)
            for _ in range(5):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                loss = step()
            torch.cuda.synchronize()
            ms[mode].append(1e3 * (time.perf_counter() - t0) / K)
            assert bool(torch.isfinite(loss)), mode
    select("fp16")
    fp8_layers = [e for k, e in m._engines.items() if k[3] == "fp8-qat" and e.train_layout][0].fp8_layers
    print("fp8 layers (conv numbers): %s" % fp8_layers)
    for mode in modes:
        print("step B=%d, %d steps per window, %-16s %s ms (spread %.2f %%)" % (B, K, mode + ":", ["%.3f" % v for v in ms[mode]],
                                                                            spread(ms[mode])))
    pairs = {q: [a / b for a, b in zip(ms["fp16"], ms[q])] for q in modes[1:]}
    for q in modes[1:]:
        print("pairs fp16 ms / %s ms: %s" % (q, ["%.3f" % v for v in pairs[q]]))
    for mode in modes:
        print("kernel classes, one instrumented step, %s: %s" % (mode, {k: "%.3f" % v for k, v in sorted(kern[mode].items())}))
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"B": B, "steps_per_window": K, "fp8_layers": list(fp8_layers), "modes": list(modes), "ms_per_step": ms,
                       "spread_percent": {p: spread(ms[p]) for p in modes}, "pairs_fp16_over": pairs,
                       "kernel_class_ms_one_step": kern}, f, indent=1)


def run_accuracy(B, steps, out_json, w4=False):
    import torch
    from modelcompression_amd import nets, YOLOV2_VOC_CFG
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    from oracle import darknet_ref as O
    dev = torch.device("cuda", 0)
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    x = synthetic_batch(B, 416, 416, seed=1, device=dev)
    x_held = synthetic_batch(B, 416, 416, seed=2, device=dev)      # images the fine-tune never sees

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    def fresh():
        m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev)
        # the synthetic running statistics are unrelated to the synthetic weights: settle them on this batch first, so that
        # the eval-mode network is the train-mode one (60 train-mode forwards in "fp16", no update of any parameter)
        m.precision = "fp16"
        m.train()
        with torch.no_grad():
            for _ in range(60):
                m(x)
        return m

    def evaluate(m, prec, images=None):
        m.precision = prec
        m.eval()
        with torch.no_grad():
            return m(x if images is None else images).cpu()

    def oracle(m, images=None):
        state = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        with torch.no_grad():
            return O.forward(blocks, state, (x if images is None else images).cpu(), training=False)

    m = fresh()
    teacher, ref32, ref32_held = evaluate(m, "fp16").to(dev), oracle(m), oracle(m, x_held)
    if w4:
        lines = {}
        for train_prec, prec in (("fp8-qat", "fp8"), ("fp8-w4-qat", "fp8-w4")):
            lines[prec] = accuracy_line(B, steps, train_prec, prec, fresh, evaluate, oracle, rel, m, teacher, ref32, ref32_held,
                                        x, x_held, torch)
        if out_json:
            with open(out_json, "w") as f:
                json.dump({"B": B, "steps": steps, "fp16_vs_fp32_oracle": rel(teacher.cpu(), ref32), "lines": lines,
                           "note": "random-init network, synthetic images: an error level, not mAP"}, f, indent=1)
        return
    before, before_held = rel(evaluate(m, "fp8"), ref32), rel(evaluate(m, "fp8", x_held), ref32_held)
    print("B=%d: eval fp16 engine vs fp32 oracle %.4f; eval fp8 BEFORE the fine-tune %.4f (held-out images %.4f)"
          % (B, rel(teacher.cpu(), ref32), before, before_held))
    runs = []
    for lr in (1e-6, 3e-6, 1e-5):      # (1e-4 diverges)
        m = fresh()
        opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=0.9)
        m.precision = "fp8-qat"
        m.train()
        losses = []
        for it in range(steps):
            out = m(x)
            loss = ((out - teacher) ** 2).sum() / B
            opt.zero_grad()
            loss.backward()
            opt.step()
            if it in (0, steps - 1):
                losses.append(float(loss.detach()))
        q = evaluate(m, "fp8")
        after, own, held = rel(q, ref32), rel(q, oracle(m)), rel(evaluate(m, "fp8", x_held), ref32_held)
        runs.append({"lr": lr, "steps": steps, "loss_first": losses[0], "loss_last": losses[-1],
                     "fp8_vs_fp32_oracle_of_the_original_weights": after, "fp8_vs_fp32_oracle_of_the_tuned_weights": own,
                     "held_out_fp8_vs_fp32_oracle_of_the_original_weights": held})
        print("lr %.0e, %d steps: distillation loss %.4g -> %.4g; eval fp8 AFTER: %.4f to the original network's fp32 logits "
              "(held-out images %.4f), %.4f to the tuned network's own fp32 logits"
              % (lr, steps, losses[0], losses[-1], after, held, own))
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"B": B, "before_fp8_vs_fp32_oracle": before, "before_held_out": before_held,
                       "fp16_vs_fp32_oracle": rel(teacher.cpu(), ref32), "runs": runs,
                       "note": "random-init network, synthetic images: an error level, not mAP"}, f, indent=1)


def accuracy_line(B, steps, train_prec, prec, fresh, evaluate, oracle, rel, m0, teacher, ref32, ref32_held, x, x_held, torch):
    """--w4: one line of the measurement -- eval `prec` before, then after `steps` steps under `train_prec` toward the fp16
    logits, per learning rate from the same start (run_accuracy's method)."""
    before, before_held = rel(evaluate(m0, prec), ref32), rel(evaluate(m0, prec, x_held), ref32_held)
    print("B=%d: eval %s BEFORE the fine-tune %.4f (held-out images %.4f)" % (B, prec, before, before_held))
    runs = []
    for lr in (1e-6, 3e-6, 1e-5):
        m = fresh()
        opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=0.9)
        m.precision = train_prec
        m.train()
        losses = []
        for it in range(steps):
            out = m(x)
            loss = ((out - teacher) ** 2).sum() / B
            opt.zero_grad()
            loss.backward()
            opt.step()
            if it in (0, steps - 1):
                losses.append(float(loss.detach()))
        q = evaluate(m, prec)
        after, own, held = rel(q, ref32), rel(q, oracle(m)), rel(evaluate(m, prec, x_held), ref32_held)
        runs.append({"lr": lr, "steps": steps, "loss_first": losses[0], "loss_last": losses[-1],
                     "vs_fp32_oracle_of_the_original_weights": after, "vs_fp32_oracle_of_the_tuned_weights": own,
                     "held_out_vs_fp32_oracle_of_the_original_weights": held})
        print("%s, lr %.0e, %d steps: distillation loss %.4g -> %.4g; eval %s AFTER: %.4f to the original network's fp32 logits "
              "(held-out images %.4f), %.4f to the tuned network's own fp32 logits"
              % (train_prec, lr, steps, losses[0], losses[-1], prec, after, held, own))
    return {"train_precision": train_prec, "eval_precision": prec, "before_vs_fp32_oracle": before, "before_held_out": before_held,
            "runs": runs}


def main(argv):
    import torch
    what, a0, a1, out_json, w4 = parse(argv, 64 if argv and argv[0] == "time" else 4, 100)
    if not torch.cuda.is_available():
        raise SystemExit("q8_qat_bench needs the GPU")
    if what == "time":
        (run_time_w4 if w4 else run_time)(a0, a1, out_json)
    else:
        run_accuracy(a0, a1, out_json, w4)


if __name__ == "__main__":
    main(sys.argv[1:])
