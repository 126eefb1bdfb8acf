"""Knowledge distillation in the retraining step (train(TEACHER=...), modelcompression_amd/distill.py) of
YOLOv2-VOC on synthetic weights and images: what the teacher costs per step, and what the distillation term does to a
pruned student's distance from its teacher.

  time      the training step of train() (forward, RegionLoss, backward, StepGuard, fused SGD) at 416x416 in the default
            training precision: plain, with a frozen teacher in "fp16" (teacher forward + DistillLoss added), and with the
            teacher in the default eval precision; and the teacher's eval forward alone in both precisions.  The legs
            alternate in one process, ROUNDS rounds; each sample is a window of STEPS steps after its own warm-up with a
            device synchronise only around the window (host clock).  Quoted: the median of the samples, and their spread.
  accuracy  a weight_prune(80) student against its dense synthetic-init teacher: retrained for STEPS steps (train()'s SGD
            rule) with the region loss alone and with region + distillation, from the same start, on one batch of synthetic
            images; then the eval-mode student's logits' rel-L2 to the teacher's on held-out images, and the DistillLoss
            of the same logits (the quantity the term minimises; the class term is blind to a common shift of the class
            logits, the rel-L2 is not).  A RANDOM-INIT network on synthetic images: an error level, NOT an mAP claim.

usage: python tools/distill_bench.py time [batch] [steps per window] [--json]
       python tools/distill_bench.py accuracy [batch] [steps] [--json]
--json merges the mode's result into profiles/distill_bench.json."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
JSON_PATH = os.path.join(ROOT, "profiles", "distill_bench.json")
ROUNDS = 5


def parse(argv):
    if not argv or argv[0] not in ("time", "accuracy"):
        raise SystemExit(__doc__)
    args = [a for a in argv[1:] if not a.startswith("--")]
    a0 = int(args[0]) if len(args) > 0 else (64 if argv[0] == "time" else 16)
    a1 = int(args[1]) if len(args) > 1 else (20 if argv[0] == "time" else 100)
    if a0 < 1 or a1 < 1:
        raise SystemExit("distill_bench: batch and step counts must be positive")
    return argv[0], a0, a1, "--json" in argv


def targets(B, torch):
    g = torch.Generator().manual_seed(3)
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


def sgd(model, B, torch):
    """train()'s optimizer: lr 1e-5, the cfg's momentum, weight_decay = decay * batch, one fused kernel."""
    return torch.optim.SGD(model.parameters(), lr=1e-5, momentum=0.9, dampening=0, weight_decay=0.0005 * B, fused=True)


def run_time(B, K, want_json):
    import torch
    from modelcompression_amd import nets, YOLOV2_VOC_CFG
    from modelcompression_amd.distill import DistillLoss
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    from modelcompression_amd.train import StepGuard
    dev = torch.device("cuda", 0)
    student = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev).train()
    x, target = synthetic_batch(B, 416, 416, seed=1, device=dev), targets(B, torch).to(dev)
    # the synthetic running statistics are unrelated to the synthetic weights: settle them on this batch first, so that the
    # eval-mode teacher is the train-mode network (60 train-mode forwards, no update of any parameter)
    with torch.no_grad():
        for _ in range(60):
            student(x)
    teacher = nets.Darknet(YOLOV2_VOC_CFG)
    teacher.load_state_dict(student.state_dict())
    teacher = teacher.to(dev).eval().requires_grad_(False)
    default_precision = teacher.precision
    distill = DistillLoss.from_model(student).to(dev)
    opt = sgd(student, B, torch)
    guard = StepGuard(student, opt, dev)

    def step(teacher_precision):
        if teacher_precision is not None:
            teacher.precision = teacher_precision
            with torch.no_grad():
                t_out = teacher(x)
        out = student(x)
        loss = student.loss(out, target)
        if teacher_precision is not None:
            loss = loss + distill(out, t_out)
        opt.zero_grad()
        loss.backward()
        guard.decide(loss)
        opt.step()

    def forward(precision):
        teacher.precision = precision
        with torch.no_grad():
            teacher(x)

    def loss_alone():
        distill(logits, logits_t)

    with torch.no_grad():
        logits, logits_t = student(x).detach().clone(), teacher(x).detach().clone()
        first = float(distill(logits, logits_t))
    print("logits: student (train mode) |max| %.4g, teacher (eval, %s) |max| %.4g, distillation loss %.6g"
          % (float(logits.abs().max()), default_precision, float(logits_t.abs().max()), first))
    if not (first == first and abs(first) != float("inf")):
        raise SystemExit("distill_bench: the distillation loss of the start is not finite")
    legs = {
        "step plain": lambda: step(None),
        "step + teacher fp16": lambda: step("fp16"),
        "step + teacher %s" % default_precision: lambda: step(default_precision),
        "teacher forward fp16": lambda: forward("fp16"),
        "teacher forward %s" % default_precision: lambda: forward(default_precision),
        "distill loss kernel pair": loss_alone,
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
                raise SystemExit("distill_bench: non-finite training loss in leg %r" % name)
    guard.finish()
    print("YOLOv2-VOC 416x416, B=%d, %d calls per window, %d rounds, %d steps skipped by StepGuard; ms per call: median "
          "(min .. max, spread)" % (B, K, ROUNDS, guard.skipped))
    for name, v in ms.items():
        print("%-28s %8.3f (%.3f .. %.3f, %.2f %%)" % (name, median(v), min(v), max(v), spread(v)))
    plain = median(ms["step plain"])
    for prec in ("fp16", default_precision):
        extra = median(ms["step + teacher %s" % prec]) - plain
        print("teacher %-6s adds %.3f ms to the step; its forward alone is %.3f ms, the loss kernel pair %.3f ms"
              % (prec, extra, median(ms["teacher forward %s" % prec]), median(ms["distill loss kernel pair"])))
    if want_json:
        save("time", {"B": B, "calls_per_window": K, "rounds": ROUNDS, "skipped_steps": guard.skipped,
                      "default_eval_precision": default_precision,
                      "ms_per_call": ms, "median_ms": {k: median(v) for k, v in ms.items()},
                      "spread_percent": {k: spread(v) for k, v in ms.items()}})


def run_accuracy(B, steps, want_json):
    import torch
    from modelcompression_amd import nets, YOLOV2_VOC_CFG
    from modelcompression_amd.distill import DistillLoss
    from modelcompression_amd.pruning.weightPruning.methods import weight_prune
    from modelcompression_amd.pruning.weightPruning.utils import prune_rate
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch
    from modelcompression_amd.train import StepGuard
    dev = torch.device("cuda", 0)
    x, target = synthetic_batch(B, 416, 416, seed=1, device=dev), targets(B, torch).to(dev)
    x_held = synthetic_batch(B, 416, 416, seed=2, device=dev)        # images the retraining never sees

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    teacher = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev)
    # the synthetic running statistics are unrelated to the synthetic weights: settle them on this batch first, so that the
    # eval-mode teacher is the train-mode network (60 train-mode forwards, no update of any parameter)
    teacher.train()
    with torch.no_grad():
        for _ in range(60):
            teacher(x)
    teacher.eval().requires_grad_(False)
    with torch.no_grad():
        t_train, t_held = teacher(x).clone(), teacher(x_held).clone()

    def evaluate(m):
        """eval mode: (rel-L2 of the logits to the teacher's, DistillLoss against the teacher) on the training images and on
        the held-out ones."""
        m.eval()
        with torch.no_grad():
            a, b = m(x), m(x_held)
            out = rel(a, t_train), rel(b, t_held), float(measure(a, t_train)), float(measure(b, t_held))
        m.train()
        return out

    measure = DistillLoss.from_model(teacher).to(dev)

    runs = []
    for with_teacher in (False, True):
        student = nets.Darknet(YOLOV2_VOC_CFG)
        student.load_state_dict(teacher.state_dict())
        student = student.to(dev)
        student.set_masks(weight_prune(student, 80.0))
        student.train()
        rate = prune_rate(student, False)
        before = evaluate(student)
        distill = DistillLoss.from_model(student).to(dev)
        opt = sgd(student, B, torch)
        guard = StepGuard(student, opt, dev)
        first = last = None
        for it in range(steps):
            out = student(x)
            region = student.loss(out, target)
            loss = region
            if with_teacher:
                with torch.no_grad():
                    t_out = teacher(x)
                d = distill(out, t_out)
                loss = region + d
            opt.zero_grad()
            loss.backward()
            guard.decide(loss)
            opt.step()
            if it in (0, steps - 1):
                last = (float(region.detach()), float(d.detach()) if with_teacher else None)
                first = last if it == 0 else first
        guard.finish()
        after = evaluate(student)
        runs.append({"loss": "region + distillation" if with_teacher else "region", "steps": steps, "pruned_percent": rate,
                     "skipped_steps": guard.skipped,
                     "region_loss_first_last": [first[0], last[0]], "distill_loss_first_last": [first[1], last[1]],
                     "rel_l2_to_teacher_before": {"train_images": before[0], "held_out": before[1]},
                     "rel_l2_to_teacher_after": {"train_images": after[0], "held_out": after[1]},
                     "eval_distill_loss_before": {"train_images": before[2], "held_out": before[3]},
                     "eval_distill_loss_after": {"train_images": after[2], "held_out": after[3]}})
        print("B=%d, %d steps, %-21s (%.1f %% pruned, %d steps skipped): region loss %.4g -> %.4g%s; eval logits' rel-L2 to "
              "the teacher's: %.4f -> %.4f on the training images, %.4f -> %.4f held out; eval DistillLoss against the "
              "teacher: %.4g -> %.4g on the training images, %.4g -> %.4g held out"
              % (B, steps, runs[-1]["loss"], rate, guard.skipped, first[0], last[0],
                 ", distillation loss %.4g -> %.4g" % (first[1], last[1]) if with_teacher else "",
                 before[0], after[0], before[1], after[1], before[2], after[2], before[3], after[3]))
    if want_json:
        save("accuracy", {"B": B, "runs": runs, "note": "random-init network, synthetic images: an error level, not mAP"})


def main(argv):
    import torch
    what, a0, a1, want_json = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("distill_bench needs the GPU")
    (run_time if what == "time" else run_accuracy)(a0, a1, want_json)


if __name__ == "__main__":
    main(sys.argv[1:])
