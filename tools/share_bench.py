"""Weight sharing (modelcompression_amd/share.py, csrc/wshare.hip) of a seeded YOLOv2-VOC: what the clustering
and the per-step projection cost, what the "shared" compressed model file weighs, and what tying does to the logits.

  time      kmeans_share (share.ITERS rounds) on the device at 4 and 8 bits, ROUNDS alternated samples each, wall time around
            the call with a device synchronise on both sides; the numpy path of the same call on a CPU copy, ONE sample per
            width (it takes tens of seconds).  project_codebooks() alone on the tied dense model, windows of 20 calls, with
            its HBM floor: one read and one write of the fp32 weights and one read of the codes.  Then the training step of
            train() (forward, RegionLoss, backward, StepGuard, fused SGD) at 416x416 in the default training precision,
            plain and followed by project_codebooks() as train(SHARE=4) runs it: alternated windows of STEPS steps after
            their own warm-up.  Quoted: medians and spreads.
  bytes     the dense, weight_prune(80) and nm_prune models tied at 4 and 8 bits: the exact size of the "shared" file beside
            the fp16 and fp8 payloads, each also as its Huffman-coded twin (entropy="huffman"), and each ratio
            against the dense float32 .weights file.  Not timed.
  accuracy  a weight_prune(80) model against itself tied at 4 bits: rel-L2 of the eval-mode logits on held-out synthetic
            images, before and after STEPS tied training steps (train()'s SGD rule + project_codebooks) on one synthetic
            batch; the untied model takes the same steps for comparison.  A RANDOM-INIT network on synthetic images: an
            error level, NOT an mAP claim.

usage: python tools/share_bench.py time [batch] [steps per window] [--json]
       python tools/share_bench.py bytes [--json]
       python tools/share_bench.py accuracy [batch] [steps] [--json]
--json merges the mode's result into profiles/share_bench.json."""
import copy
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
JSON_PATH = os.path.join(ROOT, "profiles", "share_bench.json")
ROUNDS = 5


def parse(argv):
    if not argv or argv[0] not in ("time", "bytes", "accuracy"):
        raise SystemExit(__doc__)
    args = [a for a in argv[1:] if not a.startswith("--")]
    a0 = int(args[0]) if len(args) > 0 else (64 if argv[0] == "time" else 16)
    a1 = int(args[1]) if len(args) > 1 else (10 if argv[0] == "time" else 50)
    if a0 < 1 or a1 < 1:
        raise SystemExit("share_bench: batch and step counts must be positive")
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


def fresh(torch, dev):
    from modelcompression_amd import nets, YOLOV2_VOC_CFG
    from modelcompression_amd.synthetic import init_synthetic
    return init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), seed=0).to(dev)


def run_time(B, K, want_json):
    import torch
    from modelcompression_amd import share
    from modelcompression_amd.synthetic import synthetic_batch
    from modelcompression_amd.train import StepGuard
    dev = torch.device("cuda", 0)
    model = fresh(torch, dev)
    nweights = sum(conv.weight.numel() for _, conv in share._blocks(model))
    doc = {"model": "YOLOv2-VOC, seeded synthetic weights, %d conv weights" % nweights, "iters": share.ITERS}

    # ---- the clustering
    ms = {"device 4 bits": [], "device 8 bits": []}
    for rnd in range(ROUNDS + 1):
        for bits in (4, 8):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            share.kmeans_share(model, bits=bits)
            torch.cuda.synchronize()
            if rnd:
                ms["device %d bits" % bits].append(1e3 * (time.perf_counter() - t0))
    host = copy.deepcopy(model).cpu()
    for bits in (4, 8):
        t0 = time.perf_counter()
        share.kmeans_share(host, bits=bits)
        ms["numpy %d bits (one sample)" % bits] = [1e3 * (time.perf_counter() - t0)]
    del host
    print("kmeans_share, %d weights, %d rounds + the last assignment; ms: median (min .. max)" % (nweights, share.ITERS))
    for name, v in ms.items():
        print("%-28s %10.1f (%.1f .. %.1f)" % (name, median(v), min(v), max(v)))
    doc["kmeans_ms"] = ms
    doc["kmeans_median_ms"] = {k: median(v) for k, v in ms.items()}

    # ---- the projection alone
    model.set_codebooks(share.kmeans_share(model, bits=4))
    floor_bytes = 9 * nweights                      # fp32 read + fp32 write + one code byte per weight
    proj = []
    for _ in range(ROUNDS):
        for _ in range(5):
            model.project_codebooks()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            model.project_codebooks()
        torch.cuda.synchronize()
        proj.append(1e3 * (time.perf_counter() - t0) / 20)
    print("project_codebooks alone (dense, 4 bits): median %.3f ms (%.3f .. %.3f); HBM floor %.3f GB = %.1f GB/s at the median"
          % (median(proj), min(proj), max(proj), floor_bytes / 1e9, floor_bytes / 1e6 / median(proj)))
    doc["project_ms"] = proj
    doc["project_median_ms"] = median(proj)
    doc["project_floor_bytes"] = floor_bytes
    doc["project_floor_GBps_at_median"] = floor_bytes / 1e6 / median(proj)

    # ---- the training step, plain and tied
    plain = fresh(torch, dev).train()
    tied = fresh(torch, dev)
    tied.set_codebooks(share.kmeans_share(tied, bits=4))
    tied.train()
    x, target = synthetic_batch(B, 416, 416, seed=1, device=dev), targets(B, torch).to(dev)
    state = {}
    for name, m in (("step SHARE=None", plain), ("step SHARE=4", tied)):
        opt = sgd(m, B, torch)
        state[name] = (m, opt, StepGuard(m, opt, dev))

    def step(name):
        m, opt, guard = state[name]
        loss = m.loss(m(x), target)
        opt.zero_grad()
        loss.backward()
        guard.decide(loss)
        opt.step()
        if name == "step SHARE=4":
            m.project_codebooks()

    sms = {name: [] for name in state}
    for _ in range(ROUNDS):                        # alternated: the legs see the same host / GPU conditions
        for name in state:
            for _ in range(3):
                step(name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                step(name)
            torch.cuda.synchronize()
            sms[name].append(1e3 * (time.perf_counter() - t0) / K)
            try:
                state[name][2].finish()
            except FloatingPointError:
                raise SystemExit("share_bench: non-finite training loss in leg %r" % name)
    skipped = {name: s[2].skipped for name, s in state.items()}
    print("YOLOv2-VOC 416x416, B=%d, %d steps per window, %d rounds, steps skipped by StepGuard %r; ms per step: median "
          "(min .. max, spread)" % (B, K, ROUNDS, skipped))
    for name, v in sms.items():
        print("%-18s %8.3f (%.3f .. %.3f, %.2f %%)" % (name, median(v), min(v), max(v), spread(v)))
    extra = median(sms["step SHARE=4"]) - median(sms["step SHARE=None"])
    print("the projection adds %.3f ms to the step (%.2f %%); tied layers consistent: %s"
          % (extra, 100.0 * extra / median(sms["step SHARE=None"]), share.are_codebooks_consistent(tied)))
    doc["step"] = {"B": B, "steps_per_window": K, "rounds": ROUNDS, "skipped_steps": skipped, "ms_per_step": sms,
                   "median_ms": {k: median(v) for k, v in sms.items()}, "spread_percent": {k: spread(v) for k, v in sms.items()},
                   "tied_consistent_after": bool(share.are_codebooks_consistent(tied))}
    if want_json:
        save("time", doc)


def run_bytes(want_json):
    import torch
    from modelcompression_amd import compress, share
    from modelcompression_amd.pruning.weightPruning.methods import nm_prune, weight_prune
    dev = torch.device("cuda", 0)
    doc = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, prune in (("dense", None), ("weight_prune(80)", lambda m: weight_prune(m, 80.0)), ("nm_prune", nm_prune)):
            m = fresh(torch, dev)
            if prune is not None:
                m.set_masks(prune(m))
            plain, path = os.path.join(tmp, "m.weights"), os.path.join(tmp, "m.mcz")
            m.save_weights(plain)
            row = {"float32 .weights": os.path.getsize(plain)}
            for payload in ("fp16", "fp8"):
                m.save_compressed(path, payload)
                row[payload] = os.path.getsize(path)
                m.save_compressed(path, payload, entropy="huffman")          # the coded container
                row[payload + " huffman"] = os.path.getsize(path)
            for bits in (4, 8):
                t = copy.deepcopy(m)
                t.set_codebooks(share.kmeans_share(t, bits=bits))
                t.save_compressed(path, "shared")
                info = compress.compressed_info(path)
                assert info["bytes"] == os.path.getsize(path)
                r = fresh(torch, dev)
                r.load_weights(path)
                assert all(torch.equal(a.weight.data, b.weight.data)
                           for (_, a), (_, b) in zip(share._blocks(t), share._blocks(r))), "the file is not lossless"
                row["shared %d bits" % bits] = info["bytes"]
                t.save_compressed(path, "shared", entropy="huffman")
                coded = compress.compressed_info(path)
                assert coded["plain_bytes"] == info["bytes"] and coded["bytes"] == os.path.getsize(path)
                row["shared %d bits huffman" % bits] = coded["bytes"]
                del t, r
            row["ratio"] = {k: round(row["float32 .weights"] / v, 3) for k, v in row.items() if k != "float32 .weights"}
            doc[name] = row
            print("%-18s %11d bytes dense float32; " % (name, row["float32 .weights"])
                  + ", ".join("%s %d (%.2fx)" % (k, row[k], row["ratio"][k]) for k in row["ratio"]))
    if want_json:
        save("bytes", doc)


def run_accuracy(B, steps, want_json):
    import torch
    from modelcompression_amd import share
    from modelcompression_amd.pruning.weightPruning.methods import weight_prune
    from modelcompression_amd.synthetic import synthetic_batch
    from modelcompression_amd.train import StepGuard
    dev = torch.device("cuda", 0)
    base = fresh(torch, dev).train()
    x, target = synthetic_batch(B, 416, 416, seed=1, device=dev), targets(B, torch).to(dev)
    held = synthetic_batch(B, 416, 416, seed=2, device=dev)
    with torch.no_grad():                          # settle the synthetic running statistics on this batch (distill_bench.py)
        for _ in range(60):
            base(x)
    base.set_masks(weight_prune(base, 80.0))
    base._engines = {}                             # (engines hold streams: the copies below build their own)

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    def logits(m):
        m.eval()
        with torch.no_grad():
            out = m(held).clone()
        m.train()
        return out

    def train(m, tied):
        opt = sgd(m, B, torch)
        guard = StepGuard(m, opt, dev)
        first = last = None
        for _ in range(steps):
            loss = m.loss(m(x), target)
            opt.zero_grad()
            loss.backward()
            guard.decide(loss)
            opt.step()
            if tied:
                m.project_codebooks()
            last = loss.detach()
            first = last if first is None else first
        guard.finish()
        return float(first), float(last), guard.skipped

    untied = copy.deepcopy(base)
    doc = {"B": B, "steps": steps, "model": "YOLOv2-VOC, seeded synthetic weights, weight_prune(80)",
           "note": "a random-init network on synthetic images: an error level, not an mAP claim"}
    ref_before = logits(untied)
    tied = {}
    for bits in (4, 8):
        t = copy.deepcopy(base)
        t.set_codebooks(share.kmeans_share(t, bits=bits))
        tied[bits] = t
        doc["rel_l2_tied_%d_bits_before" % bits] = rel(logits(t), ref_before)
    u = train(untied, False)
    t = train(tied[4], True)
    ref_after = logits(untied)
    got = logits(tied[4])
    doc.update({"region_loss_first_last_untied": u[:2], "region_loss_first_last_tied_4_bits": t[:2],
                "skipped_steps": {"untied": u[2], "tied": t[2]},
                "rel_l2_tied_4_bits_after_vs_untied_after": rel(got, ref_after),
                "rel_l2_tied_4_bits_after_vs_untied_before": rel(got, ref_before),
                "rel_l2_untied_after_vs_untied_before": rel(ref_after, ref_before),
                "tied_consistent_after": bool(share.are_codebooks_consistent(tied[4]))})
    for k, v in doc.items():
        print("%-44s %s" % (k, v))
    if want_json:
        save("accuracy", doc)


def main(argv):
    mode, a0, a1, want_json = parse(argv)
    if mode == "time":
        run_time(a0, a1, want_json)
    elif mode == "bytes":
        run_bytes(want_json)
    else:
        run_accuracy(a0, a1, want_json)
    if want_json:
        print("wrote", JSON_PATH)


if __name__ == "__main__":
    main(sys.argv[1:])
