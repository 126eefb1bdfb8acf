#!/usr/bin/env python3
"""Headline benchmark: YOLOv2-VOC dense fwd+bwd(+SGD step) images/sec at 416x416 on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

N = 1 runs in this process.  N > 1: when the process was started by a launcher (WORLD_SIZE in the environment, as the
driver's `python -m torch.distributed.run ... bench.py --gpus N` does) it is one rank of N; started bare, it launches
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N` on itself as a CHILD process before anything here has
touched the GPU, forwards the child's output and exits with its code (never an exec).  MCAMD_DP_BACKEND=gloo lets the
ranks share one GPU (rehearsal on a 1-GPU box).

One step = model(x) -> mean-of-logits loss -> backward (HIP engine) -> [gradient all-reduce]
-> torch.optim.SGD step (lr 1e-5, momentum .9, weight_decay .0005*B: reference train.py:144-147)
on one resident synthetic batch of B=64 images per GPU (BASELINE.json configs[1]).
The TIMED step runs in the drop-in's default operand precision (`--precision auto` = "mixed": train-mode logits within
north_star's 1e-3 of the reference's fp32 path).
Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the headline figure
(`value`, `ms_per_step`); `--dump-outputs DIR` also writes what the last timed step computed (dump_outputs below).
Everything else is measured with `--full` only (today's complete line): a second leg times the other precision of
{mixed, fp16} and `parity` checks both against the oracle (`config.tolerance_mode`, `config.throughput_mode`), the
`roofline` figures, `cpu_baseline`, and with N > 1 the all-reduce `overlap`.
The timed region is NOT instrumented; `roofline` comes from a separate pass of a few
more steps in which every convolution launch is bracketed by HIP events on the launch stream (medians per launch), for
the dominant kernel: the implicit-GEMM MFMA convolution instance of the timed engine with the largest total time.
`roofline_weight_gradient` is the same figure for the 9-tap weight-gradient kernel, whose total time is of the same size (it
runs on the second stream in the timed step; in the serialised rocprof summary of `profiles/` it is the first line).
`cpu_baseline` is the oracle (PyTorch-CPU restatement of the reference) on the host cores (rank 0, N = 1 only).

--workload prune measures the other half of the hot path: weight_prune(80) and quick_filter_prune(40)
(reference methods.py:9-78) on the 50.6 M-weight model, HBM roofline, oracle (numpy) baseline.
"""
import os

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC for RCCL: must be set before HIP initialises

import argparse  # noqa: E402
import gc  # noqa: E402
import json  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP16_TFLOPS = 2500.0       # MI355X dense fp16 MFMA peak (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0           # HBM3E (MI355X_MICROARCH.md)
FWD_BWD_GFLOP_PER_IMG = 87.782


_JSON_FD = None


def claim_stdout():
    """Only the JSON line may reach stdout.  Libraries print banners there -- RCCL writes a "ROCm version / Hostname /
    Librccl path" block to stdout when rank 0 creates a communicator -- so file descriptor 1 is pointed at stderr for the
    whole run and the result goes to the saved descriptor."""
    global _JSON_FD
    if _JSON_FD is None:
        sys.stdout.flush()
        _JSON_FD = os.dup(1)
        os.dup2(2, 1)


def emit(obj):
    line = (json.dumps(obj) + "\n").encode()
    if _JSON_FD is None:
        sys.stdout.write(line.decode())
        sys.stdout.flush()
    else:
        sys.stdout.flush()
        os.write(_JSON_FD, line)


def host_cores():
    return len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)


def host_memory_gb():
    """Memory this process may still use: MemAvailable, capped by the cgroup limit when there is one."""
    avail = None
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                avail = int(line.split()[1]) / 1e6
    except OSError:
        pass
    for f in ("/sys/fs/cgroup/memory.max", "/sys/fs/cgroup/memory/memory.limit_in_bytes"):
        try:
            v = open(f).read().strip()
            if v.isdigit() and int(v) < (1 << 60):
                used = 0
                for u in ("/sys/fs/cgroup/memory.current", "/sys/fs/cgroup/memory/memory.usage_in_bytes"):
                    try:
                        used = int(open(u).read().strip())
                        break
                    except (OSError, ValueError):
                        continue
                lim = (int(v) - used) / 1e9
                avail = lim if avail is None else min(avail, lim)
        except OSError:
            continue
    return avail


def cpu_batch_for_host(want):
    """The fp32 autograd graph of the oracle holds ~0.32 GB per image (measured: 5.1 GB at B=16): B=64 needs ~21 GB.
    Halve the sample until it fits in half of what the host offers (a box killed by the OOM killer costs more than
    a smaller sample); the batch used is reported in `cpu_baseline.sample`."""
    mem = host_memory_gb()
    b = want
    while mem is not None and b > 4 and 0.32 * b + 2.0 > 0.5 * mem:
        b //= 2
    return b


def cpu_baseline(batch, steps):
    """Oracle fwd+bwd+SGD on ALL host cores this process may use: a bounded sample of the same workload
    (B=64, 1 warm-up + >= 3 timed steps; ~30 s on the GPU box's 16 cores)."""
    import torch
    from oracle import darknet_ref as O
    from modelcompression_amd import YOLOV2_VOC_CFG
    ncpu = host_cores()
    # oneDNN / OpenMP stop scaling on this workload well below the core count of a 2-socket host (measured on the GPU
    # box, 2 x 64-core EPYC 9575F, tools/cpu_threads_sweep.py at B=16: 16 threads 7.05 img/s, 32: 7.26, 64: 5.16,
    # 128: 2.66, 256: 0.81): the baseline uses the best setting, min(cores, 32), and reports it in `cores`
    torch.set_num_threads(max(1, int(os.environ.get("MCAMD_CPU_THREADS", min(ncpu, 32)))))
    blocks = O.parse_cfg(YOLOV2_VOC_CFG)
    state = O.init_state(blocks, seed=0)
    keys = O.param_keys(blocks)
    for k in keys:
        state[k].requires_grad_(True)
    x = torch.rand(batch, 3, 416, 416, generator=torch.Generator().manual_seed(0))
    opt = torch.optim.SGD([state[k] for k in keys], lr=1e-5, momentum=0.9, weight_decay=0.0005 * batch)
    times = []
    for it in range(steps + 1):
        t0 = time.time()
        out = O.forward(blocks, state, x, training=True)
        opt.zero_grad()
        out.sum().backward()
        opt.step()
        if it > 0:
            times.append(time.time() - t0)
    dt = sum(times) / len(times)
    return {"value": round(batch / dt, 3), "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": "B=%d fwd+bwd+SGD, 1 warm-up + %d timed steps of the same YOLOv2-VOC 416x416 workload "
                      "(oracle: fp32 PyTorch-CPU / oneDNN restatement of the reference; %d torch threads of the %d cores this "
                      "process may use -- more threads are slower, tools/cpu_threads_sweep.py)"
                      % (batch, steps, torch.get_num_threads(), ncpu)}


def dump_outputs(d, model, out, loss):
    """--dump-outputs DIR: what a caller of the timed step holds after the LAST timed step, as float32 .npy files --
    logits.npy (region-layer logits of that step's forward), loss.npy, grad_sample.npy / weight_sample.npy (the parameters'
    gradients and their values after the SGD update, concatenated in parameters() order) and bn_running_stats.npy (every
    BatchNorm running_mean, then every running_var).  An array of more entries than its cap is a fixed sample: the sorted
    distinct indices of a seeded draw, the same for every run and build, so that two builds compare entry for entry
    (at most 4 M + 2 x 2 M float32 entries, 32 MB, plus the running statistics)."""
    import numpy as np
    import torch

    def sample(t, cap, seed):
        t = t.detach().reshape(-1)
        if t.numel() > cap:
            idx = np.unique(np.random.default_rng(seed).integers(0, t.numel(), cap))
            t = t[torch.from_numpy(idx).to(t.device)]
        return t.float().cpu().numpy()

    params = list(model.parameters())
    grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in params]
    stats = [b for n, b in model.named_buffers() if n.endswith("running_mean")] + \
            [b for n, b in model.named_buffers() if n.endswith("running_var")]
    arrays = {"logits": sample(out, 1 << 22, 1),
              "loss": loss.detach().float().reshape(1).cpu().numpy(),
              "grad_sample": sample(torch.cat([g.reshape(-1) for g in grads]), 1 << 21, 2),
              "weight_sample": sample(torch.cat([p.detach().reshape(-1) for p in params]), 1 << 21, 2),
              "bn_running_stats": torch.cat([b.reshape(-1).float() for b in stats]).cpu().numpy()}
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), a)


def spawn_ranks(n):
    """Bare `python bench.py --gpus N`: run the N ranks as a child torch.distributed.run job.  Nothing in this process
    has initialised the GPU (no torch.cuda call; torch is not even imported yet)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", str(max(1, host_cores() // n)))
    return subprocess.run(cmd, env=env).returncode


def bench_slim(args, model, dev, rank):
    """BASELINE configs[4]: eval forward of the physically slim model next to the masked-dense one, in the plain
    fp16 MFMA mode the config names and in the eval default ("mixed": split operands, logits within 1e-3)."""
    import tempfile
    import torch
    from modelcompression_amd import slim
    from modelcompression_amd.synthetic import synthetic_batch
    B = args.batch
    with tempfile.TemporaryDirectory() as tmp:
        thin = slim.slim_export(model, os.path.join(tmp, "slim.cfg"))
    rows = slim.slim_summary(model, thin)
    x = synthetic_batch(B, 416, 416, seed=rank, device=dev)
    model.eval()
    res = {}
    with torch.no_grad():
        for prec in ("fp16", "mixed"):
            for name, net in (("masked_dense", model), ("slim", thin)):
                net.precision = prec
                for _ in range(args.warmup):
                    net(x)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    net(x)
                torch.cuda.synchronize()
                res[(name, prec)] = (time.perf_counter() - t0) / args.steps
    if rank == 0:
        t = res[("slim", "fp16")]
        emit({
            "metric": "images/sec (inference forward, 416x416)", "value": round(B / t, 1), "unit": "images/s",
            "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(t * 1e3, 3),
            "higher_is_better": True, "dtype": "fp16", "data": "synthetic",
            "config": {"workload": "YOLOv2-VOC filter-pruned 60 %% physically slim eval forward, B=%d, plain fp16 MFMA operands "
                                   "(BASELINE configs[4])" % B,
                       "filters_kept": sum(r[2] for r in rows), "filters_dense": sum(r[1] for r in rows),
                       "masked_dense_images_per_s": round(B / res[("masked_dense", "fp16")], 1),
                       "slim_images_per_s_mixed_precision": round(B / res[("slim", "mixed")], 1),
                       "masked_dense_images_per_s_mixed_precision": round(B / res[("masked_dense", "mixed")], 1)}})


def bench_prune(args, model, dev):
    """The pruning half of the hot path on the full 50.6 M-weight model: wall time of weight_prune(80) and
    quick_filter_prune(40) (host percentile bookkeeping and the one device->host read included), the HBM roofline
    of the magnitude-select scan, and the oracle's numpy restatement on the host as the CPU baseline."""
    import numpy as np
    import torch
    from modelcompression_amd import ops
    from modelcompression_amd.pruning.weightPruning.methods import weight_prune, quick_filter_prune
    ws = [p.data for p in model.parameters() if p.dim() != 1]
    n = sum(w.numel() for w in ws)

    def wall(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    reps = max(args.steps, 3)
    t_w = wall(lambda: weight_prune(model, 80.0), reps)
    t_f = wall(lambda: quick_filter_prune(model, 40.0), reps)

    # dominant kernel: select_hist_kernel, one launch per radix pass over all 50.6 M magnitudes (4 B read per weight).
    # HIP events (torch's current stream IS the launch stream of every ops.* call) around mcamd_kth_magnitude:
    # 3 radix passes (both order statistics share them) = 3 scan launches + 3 one-block bin-scan launches.
    k = int(0.8 * (n - 1))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ops.kth_magnitude(ws, k)
    ms = []
    for _ in range(reps):
        e0.record()
        ops.kth_magnitude(ws, k)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    per_pass_ms = min(ms) / 3.0
    bytes_per_launch = 4.0 * n
    achieved = bytes_per_launch / (per_pass_ms * 1e-3) / 1e9
    # filter scores: every weight read once (4 B), 23 layers
    convs = [p.data for p in model.parameters() if p.dim() == 4]
    ops.filter_scores(convs[0])
    fs = []
    for _ in range(reps):
        e0.record()
        for w in convs:
            ops.filter_scores(w)
        e1.record()
        e1.synchronize()
        fs.append(e0.elapsed_time(e1))
    score_gbs = 4.0 * n / (min(fs) * 1e-3) / 1e9

    res = {
        "metric": "weights ranked per second (weight_prune 80 % on YOLOv2-VOC, 50.6 M weights)",
        "value": round(n / t_w / 1e6, 1), "unit": "Mweights/s", "n_gpus": 1, "steps": reps, "warmup": 1,
        "ms_per_step": round(t_w * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": "weight_prune(80) + quick_filter_prune(40) on the seeded full-size YOLOv2-VOC model "
                               "(reference methods.py:9-78), masks left on the GPU",
                   "weights": n, "weight_prune_ms": round(t_w * 1e3, 3), "quick_filter_prune_ms": round(t_f * 1e3, 3),
                   "filter_scores_all_layers_ms": round(min(fs), 4), "filter_scores_GBps": round(score_gbs, 1)},
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                     "frac": round(achieved / PEAK_HBM_GBS, 4), "traffic": None,
                     "kernel": "select_hist_kernel (one radix pass of the k-th magnitude select over all 23 weight tensors)",
                     "algorithmic_bytes_per_launch": bytes_per_launch, "avg_launch_ms": round(per_pass_ms, 4),
                     "note": "mcamd_kth_magnitude event time / 3 passes: includes the three one-block bin-scan launches"},
    }
    if not args.no_cpu_baseline:
        from oracle import prune_ref as PR
        params = [p.detach().cpu().numpy() for p in model.parameters()]
        t0 = time.time()
        PR.weight_prune(params, 80.0)
        c_w = time.time() - t0
        t0 = time.time()
        PR.quick_filter_prune(params, 40.0)
        c_f = time.time() - t0
        res["cpu_baseline"] = {"value": round(n / c_w / 1e6, 2), "unit": "Mweights/s", "cores": 1, "kind": "port",
                               "sample": "the oracle's numpy restatement on the same 50.6 M weights, one call each: "
                                         "weight_prune %.2f s, quick_filter_prune %.2f s (the reference itself spends "
                                         "25.4 s / 2.9 s, SURVEY section 6: a Python list of 50.6 M scalars)" % (c_w, c_f),
                               "quick_filter_prune_s": round(c_f, 3), "weight_prune_s": round(c_w, 3)}
    emit(res)


def roofline_pass(args, model, main_prec, step, fence, step_ms, rank):
    """--full: per-kernel figures of the timed engine from an instrumented pass of a few more steps after the timed
    region -- the `roofline` of the dominant kernel, `roofline_weight_gradient`, `event_pass`, the per-kernel fields
    of `config` -- and the --layer-table file.  Returns those fields of the result line."""
    import torch
    from modelcompression_amd import ops
    # ---- roofline of the dominant kernel, from a SEPARATE instrumented pass (the timed region above carries no events):
    # every conv launch bracketed by HIP events on the launch stream
    eng = [e for e in model._engines.values() if e.precision == main_prec and e.grad_scale == float(model.grad_scale)][0]
    # One instrumented step at a time, harvested before the next: at most one step's events are alive (round 3 kept all
    # 5 x 138 timing events until the end), the event objects are reused, and the garbage collector is kept out of the
    # pass (its pauses over the whole run are measured by main's `gc_watch` and reported).  Per launch the MEDIAN over the
    # instrumented steps is published -- one outlier pair (BENCH_r03: one 117 ms ('wgrad', layer) pair in 5 steps made
    # "wgrad 26.251 ms per step") cannot poison a figure -- and the slowest pair is reported with its host-side times.
    nprof = max(1, args.profile_steps)
    pool_all = [torch.cuda.Event(enable_timing=True) for _ in range(2 * 4 * len(eng.layers))]
    per = {}
    worst = None
    gc.collect()
    gc.disable()
    try:
        for sidx in range(nprof):
            eng.events, eng.event_pool = [], list(pool_all)
            step()
            fence()
            for tag, lay, e0, e1, host in eng.events:
                ms = e0.elapsed_time(e1)
                a = per.setdefault((tag, lay.li), [[], lay])
                a[0].append(ms)
                if worst is None or ms > worst[0]:
                    worst = (ms, tag, lay.li, sidx, host)
    finally:
        eng.events, eng.event_pool = None, None
        gc.enable()

    def median(v):
        v = sorted(v)
        return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
    per = {k: [median(v[0]) * len(v[0]), len(v[0]), v[1]] for k, v in per.items()}      # (median x n, n, layer): as the mean was
    tot = {"fwd": [0.0, 0.0], "dgrad": [0.0, 0.0], "wgrad": [0.0, 0.0]}
    rows = []
    by_tile = {}     # kernel instance (BM, BN, BK, kind, epilogue) -> [ms, algorithmic flop, launches, executed MFMA flop]
    for (tag, li), (ms, n, lay) in sorted(per.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        fl = eng.conv_flops(lay)                       # ALGORITHMIC flops: 2 M Cout Cin k^2 of the reference's convolution
        avg = ms / n
        # a split-operand forward launch multiplies the K-concatenated problem: `level` MFMA products per algorithmic one
        # (fp8-correction form, lay.f8: one fp16 product + two e4m3 products at twice the rate = 2 fp16-equivalent products)
        level = (2 if getattr(lay, "f8", False) else lay.level) if (tag == "fwd" and eng.precise) else 1
        tile = None
        if tag != "wgrad" and not (li == 0 and (lay.fused_stem or getattr(lay, "stem_split", False))):
            g_ = lay.geom_f if (tag == "fwd" and eng.precise) else lay.geom_act
            epi = (1 if lay.is_last else (3 if eng.precise else 0)) if tag == "fwd" else 0
            f8 = 1 if (tag == "fwd" and getattr(lay, "f8", False)) else 0
            tile = ops.tile_info(g_, dgrad=(tag == "dgrad")) + (epi, f8)   # (the instrumented pass runs every launch alone)
        tot[tag][0] += avg
        tot[tag][1] += fl
        rows.append("%-6s conv%-2d %4dx%-4d cin %4d cout %4d k%d  %8.3f ms  %8.1f TFLOP/s%s  tile %s" % (
            tag, li + 1, lay.H, lay.W, lay.cin, lay.cout, lay.k, avg, fl / avg / 1e9,
            (" (x%d %s: %.1f executed)" % (level, "fp16-equivalent MFMA products, fp16 + 2 fp8" if getattr(lay, "f8", False) and tag == "fwd"
                                           else "MFMA products", level * fl / avg / 1e9)) if level > 1 else "", tile))
        if tile is not None:
            b = by_tile.setdefault(tile, [0.0, 0.0, 0, 0.0])
            b[0] += ms
            b[1] += fl * n
            b[2] += n
            b[3] += level * fl * n
    # The 9-tap weight gradient (csrc/conv_wgrad.hip: wgrad9_kernel for the 26x26 / 13x13 layers, its wide form from 40 pixels
    # per row) is the other kernel of the step's size: reported beside the dominant convolution instance.  An event pair of
    # tag 'wgrad' brackets the launch AND its slab-reduction pass (mcamd_conv_wgrad is one call).
    wg9 = {}
    for (tag, li), (ms, n, lay) in per.items():
        cin_eff = lay.fold_aug if lay.fold is not None else lay.cin
        if tag == "wgrad" and lay.k == 3 and li > 0 and cin_eff % 64 == 0 and lay.n_act % 32 == 0:
            b = wg9.setdefault("wgrad9w_kernel<64,3>" if lay.W >= 40 else "wgrad9_kernel<64>", [0.0, 0.0, 0])
            b[0] += ms
            b[1] += eng.conv_flops(lay) * n
            b[2] += n
    # the dominant kernel = the implicit-GEMM instance with the largest total time
    dom_tile = max(by_tile, key=lambda t: by_tile[t][0])
    dom_ms, dom_flop, dom_n, dom_exec = by_tile[dom_tile]
    achieved = dom_flop / (dom_ms * 1e-3) / 1e12 if dom_ms > 0 else 0.0
    executed = dom_exec / (dom_ms * 1e-3) / 1e12 if dom_ms > 0 else 0.0
    # HBM bytes per launch of that kernel: PMC counters cannot be read from inside this process; they are
    # collected by tools/collect_profiles.sh on the same command (FETCH_SIZE and WRITE_SIZE in separate
    # rocprofv3 passes, FETCH_SIZE doubled per the gfx950 correction) and committed under profiles/.
    traffic = traffic_source = None
    tfile = os.path.join(ROOT, "profiles", "dominant_kernel_traffic.json")
    if os.path.exists(tfile):
        try:
            tj = json.load(open(tfile))
            want = {2: "void igemm_pp_kernel<%d, %d, %d, %s>" % (dom_tile[4], dom_tile[0], dom_tile[1], "32, true" if dom_tile[5] else "16, false")}.get(
                dom_tile[3], "void igemm_kernel<%d, %d," % dom_tile[:2])
            if tj["kernel"].startswith(want):
                traffic = round(tj["hbm_bytes_per_launch"])
                traffic_source = tj.get("source", "profiles/dominant_kernel_traffic.json")
        except Exception:
            traffic = None
    if rank == 0 and args.layer_table:
        with open(args.layer_table, "w") as f:
            f.write("\n".join(rows) + "\n")
            for tag, (ms, fl) in tot.items():
                f.write("TOTAL %-6s %8.3f ms/step  %8.1f TFLOP/s\n" % (tag, ms, fl / ms / 1e9 if ms else 0))
            f.write("step %.3f ms (uninstrumented); conv kernels %.3f ms\n" % (step_ms, sum(v[0] for v in tot.values())))
    res = {"config": {"conv_kernel_ms_per_step": {k: round(v[0], 3) for k, v in tot.items()},
                      "conv_kernel_tflops": {k: round(v[1] / v[0] / 1e9, 1) if v[0] else 0.0 for k, v in tot.items()}},
        "roofline": {"bound": "mfma", "achieved": round(achieved, 1), "peak": PEAK_FP16_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(achieved / PEAK_FP16_TFLOPS, 4), "traffic": traffic, "traffic_source": traffic_source,
                     "algorithmic_gflop_per_launch": round(dom_flop / max(dom_n, 1) / 1e9, 2),
                     # split-operand launches execute 3 MFMA products per algorithmic multiply -- one fp16 + two fp8 at twice
                     # the rate (= 2 fp16-equivalent products) in the fp8-correction form: the rate the matrix cores actually
                     # ran at, in fp16-equivalent flops (achieved counts the reference's 2 M N K only, as the contract asks)
                     "mfma_tflops_executed": round(executed, 1), "mfma_frac_executed": round(executed / PEAK_FP16_TFLOPS, 4),
                     "kernel": ("igemm_pp_kernel<%d,%d,%d,%s> %dx%dx%d ping-pong (%s launches of that instance)" % (
                                    (dom_tile[4],) + dom_tile[:2] + ("32,true" if dom_tile[5] else "16",) + dom_tile[:3] +
                                    (("split-operand conv forward with fp8 correction terms, fp32 raw output" if dom_tile[5] else
                                      "split-operand conv forward, fp32 raw output") if dom_tile[4] == 3 else "conv fwd + dgrad",))
                                if dom_tile[3] == 2 else
                                "igemm_kernel<%d,%d,..,%d,2,%d> (conv launches of that instance)" % (dom_tile[:3] + (dom_tile[4],))),
                     "launches_per_step": dom_n // nprof,
                     "avg_launch_ms": round(dom_ms / max(dom_n, 1), 4),
                     "measured": "HIP events around every launch in %d extra steps after the timed region; per launch the "
                                 "median over those steps" % nprof},
    }
    if wg9:
        wk = max(wg9, key=lambda k_: wg9[k_][0])
        wms, wfl, wn = wg9[wk]
        res["roofline_weight_gradient"] = {
            "bound": "mfma", "achieved": round(wfl / (wms * 1e-3) / 1e12, 1), "peak": PEAK_FP16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(wfl / (wms * 1e-3) / 1e12 / PEAK_FP16_TFLOPS, 4), "kernel": wk + " + its slab-reduction pass",
            "launches_per_step": wn // nprof, "avg_launch_ms": round(wms / max(wn, 1), 4),
            "ms_per_step": round(wms / nprof, 3), "dominant_conv_instance_ms_per_step": round(dom_ms / nprof, 3),
            "note": "the weight-gradient kernel with the largest total time, same event pass (it runs on the second stream in "
                    "the timed step); ALGORITHMIC flops 2 M Cout Cin 9 of the launches' layers"}
    # the instrumented pass, as evidence: what the slowest single event pair was and what the host did inside it
    # (seconds spent in [event record, library call, event record]); a per-step sum of kernel times cannot exceed ~1.5 steps
    # (the timed step overlaps the weight gradients with the rest; serialised they add ~10 %)
    res["event_pass"] = {"steps": nprof, "statistic": "median per launch",
                         "max_pair_ms": round(worst[0], 3), "max_pair_at": {"tag": worst[1], "conv": worst[2] + 1, "step": worst[3]},
                         "max_pair_host_ms": [round(v * 1e3, 3) for v in worst[4]]}
    if rank != 0:
        return res
    ksum = sum(v[0] for v in tot.values())
    assert ksum < 1.5 * step_ms, ("instrumented pass inconsistent with the timed step: conv kernels %.3f ms per step vs %.3f ms "
                                 "per step; slowest pair %r" % (ksum, step_ms, worst))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", "--per-gpu-batch", dest="batch", type=int, default=64,
                    help="images per GPU (BASELINE configs[3] = 256 over 8 GPUs: --per-gpu-batch 32)")
    ap.add_argument("--loss", default="mean", choices=["mean", "region"],
                    help="mean = mean of the logits (the headline line); region = the real train.py step: RegionLoss on "
                         "synthetic boxes + the device-side overflow / non-finite policy (train.StepGuard), reference "
                         "train.py:214-235")
    ap.add_argument("--precision", default="auto", choices=["auto", "mixed", "fp16"],
                    help="operand precision of the TIMED step: auto = the drop-in's training default (`mixed`: split hi/lo "
                         "operands, train-mode logits within north_star's 1e-3); fp16 = plain operands, the throughput opt-in")
    ap.add_argument("--no-tolerance-mode", "--no-second-precision", dest="no_tolerance_mode", action="store_true",
                    help="skip the second timed leg (the OTHER precision of {mixed, fp16}) and the parity check")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=64)
    ap.add_argument("--cpu-steps", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=5, help="instrumented steps (untimed) for the roofline entry")
    ap.add_argument("--layer-table", default="", help="write the per-launch timing table to this file")
    ap.add_argument("--transport", default=None, choices=["fp32", "fp16"], help="gradient all-reduce transport (N > 1)")
    ap.add_argument("--workload", default="dense", choices=["dense", "filter40", "weight80", "slim60", "prune"],
                    help="dense = BASELINE configs[1] (the default bench line); filter40 / weight80 = the retrain step of "
                         "configs[2] / configs[3] with the reference's masks; slim60 = configs[4], eval forward of the "
                         "physically slim 60 %% filter-pruned model (use --batch 128); prune = the mask computation itself")
    ap.add_argument("--full", action="store_true",
                    help="dense / filter40 / weight80: also measure and check what the headline figure does not need -- the "
                         "second precision's leg, parity against the oracle, the instrumented roofline pass (--layer-table), "
                         "cpu_baseline and, with N > 1, the all-reduce overlap legs")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step computed to DIR/<name>.npy (float32; see dump_outputs)")
    args = ap.parse_args()
    if args.layer_table and not args.full:
        ap.error("--layer-table comes from the instrumented pass of --full")
    if args.dump_outputs and args.workload in ("prune", "slim60"):
        ap.error("--dump-outputs: the training-step workloads only (dense, filter40, weight80)")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))
    claim_stdout()

    import torch
    import torch.distributed as dist
    from modelcompression_amd import nets, dp, YOLOV2_VOC_CFG

    # every pause of Python's cyclic garbage collector over the run (a host-side pause inside a step is a GPU-side gap once
    # it outlasts the queued work): [generation, milliseconds, region] -- `region` is set around the timed loops
    gc_log, gc_t0, region = [], [0.0], ["setup"]

    def gc_watch(phase, info):
        if phase == "start":
            gc_t0[0] = time.perf_counter()
        else:
            gc_log.append((info.get("generation", -1), (time.perf_counter() - gc_t0[0]) * 1e3, region[0]))
    gc.callbacks.append(gc_watch)
    from modelcompression_amd import engine as engine_mod
    from modelcompression_amd.synthetic import init_synthetic, synthetic_batch

    # MCAMD_DP_BACKEND=gloo lets several ranks share one GPU (rehearsal of the N>1 path on a 1-GPU box)
    backend = os.environ.get("MCAMD_DP_BACKEND") or None
    ndev = max(torch.cuda.device_count(), 1)
    os.environ["LOCAL_RANK"] = str(int(os.environ.get("LOCAL_RANK", "0")) % ndev)
    rank, world = dp.init_from_env(backend)
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, "--gpus %d but WORLD_SIZE=%d" % (args.gpus, world)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    model = nets.Darknet(YOLOV2_VOC_CFG)
    init_synthetic(model, seed=0)
    model.to(dev).train()
    if args.workload == "prune":
        return bench_prune(args, model, dev)
    # the timed precision: the drop-in's default unless asked otherwise; the other one of {mixed, fp16} is the second leg
    main_prec = "fp16" if args.precision == "fp16" else "mixed"
    other_prec = "mixed" if main_prec == "fp16" else "fp16"
    model.precision = args.precision
    B = args.batch
    wl_name = "dense (0% prune)"
    masks = None
    if args.workload != "dense":
        from modelcompression_amd.pruning.weightPruning.methods import weight_prune, quick_filter_prune
        if args.workload == "weight80":
            masks, wl_name = weight_prune(model, 80.0), "weight-pruned 80 % (magnitude masks)"
        else:
            perc = 40.0 if args.workload == "filter40" else 60.0
            masks, wl_name = quick_filter_prune(model, perc), "filter-pruned %g %% (kept filters only)" % perc
        if world > 1 or (dp.rehearsal() and dist.is_initialized()):
            dp.broadcast_masks(masks, src=0)
        model.set_masks(masks)
    if args.workload == "slim60":
        return bench_slim(args, model, dev, rank)
    # same update rule as train.py:144-147; torch's fused multi-tensor implementation (one kernel per dtype/device)
    opt = torch.optim.SGD(model.parameters(), lr=1e-5, momentum=0.9, dampening=0, weight_decay=0.0005 * B, fused=True)
    reducer = None
    dp_on = world > 1 or (dp.rehearsal() and dist.is_initialized())     # MCAMD_DP_REHEARSE=1: one-rank RCCL rehearsal
    if dp_on:
        # static weight masks (configs[3]): only the kept gradient entries travel
        reducer = dp.attach(model, dp.GradReducer(transport=args.transport),
                            masks=masks if args.workload == "weight80" else None)
    x = synthetic_batch(B, 416, 416, seed=rank, device=dev)   # resident in HBM before the timed region
    state0 = None
    if args.full and not args.no_tolerance_mode and not args.no_cpu_baseline and not dp_on:
        state0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}   # for the parity check below
    guard = target = None
    if args.loss == "region":
        # the real training step (reference train.py:214-235): RegionLoss on seeded synthetic boxes, resident in HBM, and
        # train.py's skip policy -- decided on the device, read by the host one step late (no synchronisation in the step)
        from modelcompression_amd.data import SyntheticDetection
        from modelcompression_amd.train import StepGuard
        ds = SyntheticDetection(B, shape=(416, 416), seed=100 + rank)
        target = torch.stack([ds[i][1] for i in range(B)]).float().to(dev)
        region_loss = model.loss
        region_loss.seen = 0
        guard = StepGuard(model, opt, dev)

    steps_done = [0]
    last = [None, None]     # (logits, loss) of the latest step: what --dump-outputs writes after the timed ones

    def step():
        steps_done[0] += 1
        out = model(x)
        if guard is not None:
            region_loss.seen = region_loss.seen + B * world
            loss = region_loss(out, target)
            opt.zero_grad()
            loss.backward()
            guard.decide(loss)
            opt.step()
            last[0], last[1] = out, loss
            return
        # mean of the logits: dL/dlogit = 1 / (B * 125 * 13 * 13).  (Rounds 1's sum-of-logits loss, dL/dlogit = 1, makes
        # gradients of 1e3-1e5 that lr 1e-5 turns into O(1) weight updates: the run diverged within a few steps and
        # only the fp16 saturation of the stored gradients kept it finite -- the overflow flag now shows that.)
        loss = out.float().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        last[0], last[1] = out, loss

    def fence():
        if dp_on:
            dist.barrier(device_ids=[local]) if dist.get_backend() == "nccl" else dist.barrier()
        torch.cuda.synchronize()

    # fp16 gradient storage: the engine keeps grad_scale x gradient and saturates at +-65504 (flagged).  Settle the
    # scale during warm-up the way train.py does per step (skip + reduce, all ranks together), then time with it fixed.
    skipped_warm = 0
    if guard is None:
        for it in range(10):
            step()
            over = model.grad_overflowed()
            if dp_on:
                over = not dp.all_ranks_ok(not over, dev)
            if not over:
                break
            model.grad_scale = model.grad_scale / 16.0
    else:
        for it in range(24):                  # StepGuard settles the scale itself (halving, one step late)
            step()
        guard.finish()
        skipped_warm = guard.skipped
    for _ in range(max(args.warmup, 1)):      # builds and warms the engine of the final scale
        step()
    if guard is not None:
        guard.finish()
        skipped_warm = guard.skipped
    gc.collect()      # (a full collection now, so that none falls into the timed steps by accident of the allocation count)
    fence()
    region[0] = "timed"
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    dt = time.perf_counter() - t0
    region[0] = "after"
    flat = model._last_flat_grad
    assert flat is not None and bool(torch.isfinite(flat).all()), "non-finite gradients in the timed run"
    if guard is not None:
        guard.finish()
        assert guard.skipped == skipped_warm, "a step of the timed run was skipped (fp16 gradient overflow)"
    else:
        assert not model.grad_overflowed(), "a scaled gradient saturated the fp16 range in the timed run"
    if reducer is not None:
        assert not reducer.transport_overflowed(), "the fp16 all-reduce transport clamped a gradient in the timed run"
    if dp_on:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        # every rank must hold the same averaged gradient and the same weights after the same steps
        sig = torch.stack([flat.double().sum(), flat.double().abs().sum(),
                           sum(p.detach().double().sum() for p in model.parameters())])
        lo, hi = sig.clone(), sig.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        # (bit-identical is what a ring / tree all-reduce delivers; a last-bit difference between ranks would not
        # invalidate the timing, a real divergence does)
        spread = float(((hi - lo).abs() / hi.abs().clamp_min(1e-30)).max())
        assert spread < 1e-6, "ranks diverged: gradient / weight checksums differ (%s vs %s)" % (lo.tolist(), hi.tolist())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, last[0], last[1])

    # ---- how much of the gradient all-reduce is hidden under the backward pass (N > 1 / rehearsal): the same collectives
    # alone on an idle GPU, and the same step without them (hooks detached; the ranks' weights drift apart from here on,
    # which no later leg depends on)
    overlap = None
    red_steps = red_bytes = red_colls = 0
    if dp_on:
        red_steps, red_bytes, red_colls = steps_done[0], reducer.bytes_reduced, reducer.collectives
    if dp_on and args.full:
        k = max(3, min(args.steps, 10))
        tmp = torch.zeros_like(flat)
        pre, reducer.prescaled = reducer.prescaled, True
        reducer.reduce_flat(tmp)
        fence()
        ta = time.perf_counter()
        for _ in range(k):
            reducer.reduce_flat(tmp)
        fence()
        t_ar = (time.perf_counter() - ta) / k
        reducer.prescaled = pre
        hooks = (model._grad_ready_hook, model._grad_hook)
        model._grad_ready_hook = model._grad_hook = None
        step()
        fence()
        ta = time.perf_counter()
        for _ in range(k):
            step()
        fence()
        t_nodp = (time.perf_counter() - ta) / k
        model._grad_ready_hook, model._grad_hook = hooks
        tt = torch.tensor([t_ar, t_nodp], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        t_ar, t_nodp = (float(v) for v in tt.tolist())
        t_dp = dt / args.steps
        overlap = {"allreduce_alone_ms": round(t_ar * 1e3, 3), "step_without_allreduce_ms": round(t_nodp * 1e3, 3),
                   "step_ms": round(t_dp * 1e3, 3),
                   "hidden_frac": round(max(0.0, min(1.0, (t_nodp + t_ar - t_dp) / t_ar)), 3) if t_ar > 0 else None}

    step_ms = dt / args.steps * 1e3
    roof = roofline_pass(args, model, main_prec, step, fence, step_ms, rank) if args.full else None

    # ---- second timed leg: the OTHER precision of {mixed, fp16} -- same step, same batch, same barriers.  `mixed` (split
    # hi/lo operands on all but the costliest blocks, engine.py) meets north_star's 1e-3 on the region-layer logits; plain
    # `fp16` is the throughput opt-in
    def leg_info(prec, seconds):
        e_ = [e for e in model._engines.values() if e.precision == prec][-1]
        d = {"precision": prec, "images_per_s": round(world * B * args.steps / seconds, 2),
             "ms_per_step": round(seconds / args.steps * 1e3, 3)}
        if prec == "mixed":
            d["plain_fp16_blocks"] = [l.li + 1 for l in e_.layers if l.level == 1]
            d["fp8_correction_blocks"] = [l.li + 1 for l in e_.layers if getattr(l, "f8", False)]
            d["note"] = ("forward convolutions on split operands with fp32 raw outputs: x_hi*w_hi on fp16 MFMAs plus the correction "
                         "products x_lo*w_hi + x_hi*w_lo -- from e4m3 copies on block-scaled fp8 MFMAs in `fp8_correction_blocks`, "
                         "from fp16 lo planes in the other split blocks; `plain_fp16_blocks` multiply x_hi*w_hi only; the first "
                         "block fused on split operands; backward on plain fp16 operands")
        else:
            d["note"] = "plain fp16 MFMA operands everywhere: its train-mode logits do NOT meet 1e-3 (see `parity`)"
        return d
    legs = {main_prec: leg_info(main_prec, dt)}
    if args.full and not args.no_tolerance_mode:
        model.precision = other_prec
        for _ in range(max(2, min(args.warmup, 3))):
            step()
        if guard is not None:
            guard.finish()
        gc.collect()
        fence()
        region[0] = "timed_second_precision"
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        fence()
        dt_m = time.perf_counter() - t1
        region[0] = "after"
        if dp_on:
            t = torch.tensor([dt_m], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt_m = float(t.item())
        assert not model.grad_overflowed(), "a scaled gradient saturated the fp16 range in the second-precision run"
        legs[other_prec] = leg_info(other_prec, dt_m)
        model.precision = args.precision
    # ---- parity of what was timed: training-mode logits (batch statistics) of both precisions against the fp32 oracle
    # on the SAME weights and the same batch (rank 0, N = 1; the oracle is the checker, ~5 s of host time)
    parity = None
    if state0 is not None and rank == 0:
        from oracle import darknet_ref as O
        blocks_o = O.parse_cfg(YOLOV2_VOC_CFG)
        xc = x.cpu()
        masks_c = [m_.cpu() for m_ in masks] if masks is not None else None
        torch.set_num_threads(max(1, int(os.environ.get("MCAMD_CPU_THREADS", min(host_cores(), 32)))))
        with torch.no_grad():
            ref = O.forward(blocks_o, state0, xc, training=True, masks=masks_c)
        parity = {"reference": "oracle (fp32 PyTorch-CPU restatement of nets.py:720-774), training-mode forward, B=%d" % B,
                  "bar": 1e-3}
        for prec in ("fp16", "mixed"):
            model.load_state_dict(state0)
            model.precision = prec
            with torch.no_grad():
                got = model(x).cpu()
            parity["train_logits_rel_l2_" + prec] = float("%.3e" % ((got.double() - ref.double()).norm() / ref.double().norm()))
        model.precision = args.precision
        for prec in legs:
            legs[prec]["train_logits_rel_l2"] = parity["train_logits_rel_l2_" + prec]
    # every rank's probe result (engine.py _probe_side_stream): a rank whose second stream shares the launch stream's hardware
    # queue runs its weight gradients serialised and would bound the whole job
    ssc = next(iter(engine_mod.Engine._SIDE_STREAMS.values()), (None, None))[1]
    ssc_all = [ssc]
    if dp_on:
        flag = torch.tensor([-1 if ssc is None else int(bool(ssc))], device=dev, dtype=torch.int32)
        got = [torch.zeros_like(flag) for _ in range(world)]
        dist.all_gather(got, flag)
        ssc_all = [None if int(t.item()) < 0 else bool(int(t.item())) for t in got]
    if rank != 0:
        return
    value = world * B * args.steps / dt
    res = {
        "metric": "images/sec (fwd+bwd, 416x416)", "value": round(value, 2), "unit": "images/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(step_ms, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "fp16", "data": "synthetic",
        "config": {"workload": "YOLOv2-VOC %s fwd+bwd+SGD step, B=%d per GPU, 416x416 (BASELINE configs[%d])" % (
                       wl_name, B, {"dense": 1, "filter40": 2, "weight80": 3}[args.workload]),
                   "global_batch": world * B, "input": "3x416x416", "parallelism": "dp%d" % world,
                   "loss": ("RegionLoss on synthetic boxes + train.StepGuard (the train.py step)" if guard is not None
                            else "mean of the logits"),
                   "precision": ("mixed (the drop-in's training default: forward convolutions on split hi/lo fp16 operands "
                                 "except the blocks listed in `tolerance_mode`, train-mode logits within north_star's 1e-3, see "
                                 "`parity`; `throughput_mode` = plain fp16 operands, the explicit opt-in)") if main_prec == "mixed" else
                                ("fp16 (plain fp16 MFMA operands: the throughput opt-in; its train-mode logits do NOT meet "
                                 "north_star's 1e-3, see `parity`; `tolerance_mode` is the default precision, which does)"),
                   "timed_precision": main_prec,
                   "tolerance_mode": legs.get("mixed"),
                   "throughput_mode": legs.get("fp16"),
                   "grad_scale": model.grad_scale,
                   # engine.py _get_side_stream: the weight-gradient stream was PROBED to run beside the launch stream
                   # (None: overlap off or probe disabled; False: no concurrent stream found, the step is serialised)
                   "second_stream_concurrent": next(iter(engine_mod.Engine._SIDE_STREAMS.values()), (None, None))[1],
                   "conv_tflops_whole_step": round(value * FWD_BWD_GFLOP_PER_IMG / 1e3, 1),
                   "frac_of_fp16_mfma_peak_whole_step": round(value * FWD_BWD_GFLOP_PER_IMG / 1e3 / (PEAK_FP16_TFLOPS * world), 4)},
    }
    if roof is not None:
        res["config"].update(roof.pop("config"))
        res.update(roof)
    gcs = [g for g in gc_log if g[2].startswith("timed")]
    res["host"] = {"gc_collections": len(gc_log), "gc_max_pause_ms": round(max([g[1] for g in gc_log] or [0.0]), 2),
                   "gc_pauses_in_timed_regions": [[g[0], round(g[1], 2), g[2]] for g in gcs]}
    if args.full:
        res["parity"] = parity
    if dp_on:
        res["cpu_baseline"] = None
        res["collective"] = {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                             "second_stream_concurrent_per_rank": ssc_all,
                             "transport": reducer.transport, "kept_fraction": round(reducer.kept_fraction, 4),
                             "bytes_per_step_per_rank": red_bytes // max(1, red_steps),
                             "collectives_per_step": red_colls // max(1, red_steps),
                             "overlap": overlap}
    elif args.full and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(cpu_batch_for_host(args.cpu_batch), args.cpu_steps)
    emit(res)


if __name__ == "__main__":
    try:
        main()
    finally:
        try:
            import torch.distributed as _d
            if _d.is_available() and _d.is_initialized():
                _d.destroy_process_group()
        except Exception:
            pass
