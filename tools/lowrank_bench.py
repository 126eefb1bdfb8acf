"""Low-rank inference of YOLOv2-VOC at 416x416 (Darknet.lowrank): the fused two-GEMM launch against the dense
launch it replaces and against the unfused pair it stands in for.

Speed mode (default): exactly-low-rank seeded models -- set_factors with random U and V of rank 64, 128, 192 and 256 on every
block lowrank_factor would accept at that rank (time does not depend on the values).  Per rank:
  * the whole eval forward at batch B, Darknet.lowrank off and on alternated in one process, PAIRS pairs of `steps` calls each
    with a device synchronise around the loop (host clock): medians and spreads;
  * per chosen layer at B, 8 and 1, in us (device events around `steps` launches, median of PASSES): the dense launch (the
    engine's own conv launch with lowrank off), the unfused pair timed through ops directly (conv_fwd_raw to r channels, then
    conv_fwd_padded of the 1 x 1 block over a padded copy of them; the copy itself is NOT timed: the pair's lower bound) and the
    fused launch;
  * resident operand bytes of the chosen blocks: up + vp against wp (which stays allocated as the stale fallback).
The policy constant the table implies: over all (layer of conv9 .. conv22, rank) points at batch B sorted by cost ratio
r (Cin k k + Cout) / (Cin k k Cout), the largest ratio below the first point whose fused launch is not at least 10 % faster than
its dense launch (0.0: the cheapest point already fails).

Error mode (--error): on the seeded random-init model, rel-L2 of the fp16 eval logits after lowrank_factor(energy = 0.9 / 0.8 /
0.6) + set_factors with lowrank on, against the unfactored fp16 logits.  SYNTHETIC: a random-init spectrum is flat, so most
blocks need more than 256 singular values and stay dense; this says nothing about mAP.

usage: python tools/lowrank_bench.py B steps [--json] [--error]      (--json: the document also goes to profiles/lowrank_bench.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from modelcompression_amd import nets, ops, lowrank, YOLOV2_VOC_CFG, _lib as L
from modelcompression_amd.synthetic import init_synthetic, synthetic_batch

B, STEPS = int(sys.argv[1]), int(sys.argv[2])
PAIRS, PASSES, RANKS = 5, 5, (64, 128, 192, 256)
if not torch.cuda.is_available():
    raise SystemExit("lowrank_bench needs the GPU")
dev = torch.device("cuda", 0)


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def engine(m, x):
    return [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and not e.train_layout][0]


def model():
    m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev)
    m.eval()
    m.precision, m.lowrank_max_cost, m.lowrank_min_tiles = "fp16", 1.0, 1
    return m


def random_factors(m, r):
    """Random (U, V) of rank r on every block lowrank_factor's rules accept at that rank."""
    gen, out = torch.Generator().manual_seed(r), []
    for _, conv, ok in lowrank._inner_bn(m):
        cout, K = conv.weight.shape[0], conv.weight[0].numel()
        if not ok or r * (K + cout) >= K * cout:
            out.append(None)
            continue
        s = (2.0 / K) ** 0.25 * (1.0 / r) ** 0.25
        out.append((torch.randn((r,) + tuple(conv.weight.shape[1:]), generator=gen) * s, torch.randn(cout, r, generator=gen) * s))
    return out


def device_us(fn):
    """us per call: events around STEPS calls, median of PASSES."""
    fn()
    out = []
    for _ in range(PASSES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / STEPS)
    return median(out)


def conv_us(m, x):
    """{conv number: us of its conv launch} from the engine's events, median of PASSES instrumented forwards."""
    m(x)
    eng, acc = engine(m, x), {}
    for _ in range(PASSES):
        eng.events = []
        m(x)
        torch.cuda.synchronize()
        for tag, lay, e0, e1, _host in eng.events:
            if tag == 'fwd':
                acc.setdefault(lay.li + 1, []).append(e0.elapsed_time(e1) * 1e3)
        eng.events = None
    return {k: median(v) for k, v in acc.items()}


def pair_us(eng, lay):
    g, r = lay.geom_act, lay.lr_rank
    gu, gv = ops.geom(g.B, g.H, g.W, g.ksize, g.cin, r, g.x_ld, g.x_choff), ops.geom(g.B, g.H, g.W, 1, r, g.cout, r)
    xin = eng.bufs[lay.tin.buf]
    hraw = torch.zeros(g.B * g.H * g.W * r, dtype=torch.float16, device=dev)
    hpad, y = ops.alloc_padded(g.B, g.H, g.W, r, dev), ops.alloc_padded(g.B, g.H, g.W, g.cout, dev)

    def pair():
        ops.conv_fwd_raw(gu, xin, lay.up, hraw, r)
        ops.conv_fwd_padded(gv, hpad, lay.vp, y, g.cout, 0, lay.scale, lay.shift, lay.slope)
    return device_us(pair)


def layer_rows(m, batch):
    x = synthetic_batch(batch, 416, 416, seed=0, device=dev)
    m.lowrank = False
    dense = conv_us(m, x)
    m.lowrank = True
    fused = conv_us(m, x)
    eng, rows = engine(m, x), []
    for lay in eng.layers:
        if lay.form != "lowrank":
            continue
        n, K = lay.li + 1, lay.cin * lay.k * lay.k
        info = ops.conv_fwd_lowrank_info(lay.geom_act, lay.lr_rank)
        rows.append({"conv": n, "k": lay.k, "cin": lay.cin, "cout": lay.cout, "rank": lay.lr_rank,
                     "cost": lay.lr_rank * (K + lay.cout) / float(K * lay.cout), "tiles": info.mtiles, "lds_bytes": info.lds_bytes,
                     "us_dense": dense[n], "us_pair": pair_us(eng, lay), "us_fused": fused[n],
                     "bytes_up_vp": 2 * (lay.up.numel() + lay.vp.numel()), "bytes_wp": 2 * lay.wp.numel()})
    return rows


def speed():
    levels = []
    for r in RANKS:
        m = model()
        m.set_factors(random_factors(m, r))
        x = synthetic_batch(B, 416, 416, seed=0, device=dev)
        legs = {"off": [], "on": []}
        for _ in range(PAIRS):
            for flag in (False, True):
                m.lowrank = flag
                for _ in range(5):
                    m(x)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(STEPS):
                    m(x)
                torch.cuda.synchronize()
                legs["on" if flag else "off"].append((time.perf_counter() - t0) / STEPS * 1e3)
        levels.append({"rank": r, "forward_ms": legs, "layers": {str(b): layer_rows(m, b) for b in dict.fromkeys((B, 8, 1))}})
        del m
    pts = sorted((row["cost"], row["us_dense"] / row["us_fused"], row["conv"], row["rank"])
                 for lv in levels for row in lv["layers"][str(B)] if 9 <= row["conv"] <= 22)
    const = 0.0
    for cost, gain, _, _ in pts:
        if gain < 1.1:
            break
        const = cost
    return {"levels": levels, "policy_points": pts, "implied_max_cost": const}


def error():
    base = model()
    x = synthetic_batch(2, 416, 416, seed=0, device=dev)
    ref, out = base(x).double(), []
    for e in (0.9, 0.8, 0.6):
        m = model()
        f = lowrank.lowrank_factor(m, energy=e)
        if any(t is not None for t in f):
            m.set_factors(f)
        m.lowrank = True
        y = m(x).double()
        out.append({"energy": e, "ranks": {str(k): v for k, v in engine(m, x).lowrank_ranks.items()},
                    "chosen": list(engine(m, x).lowrank_layers), "rel_l2_vs_unfactored_fp16": float((y - ref).norm() / ref.norm())})
    return out


with torch.no_grad():
    doc = {"arch": L.lib().mcamd_arch().decode(), "B": B, "steps": STEPS, "pairs": PAIRS, "passes": PASSES}
    if "--error" in sys.argv:
        doc["synthetic_error"] = error()
    else:
        doc.update(speed())
if "--json" in sys.argv:
    path = os.path.join(ROOT, "profiles", "lowrank_bench_error.json" if "--error" in sys.argv else "lowrank_bench.json")
    with open(path, "w") as fp:
        json.dump(doc, fp, indent=1)
    print(json.dumps(doc, indent=1))
elif "--error" in sys.argv:
    for r in doc["synthetic_error"]:
        print("energy %.1f (synthetic, not an mAP claim): factored %s, chosen %s, rel-L2 vs unfactored fp16 %.3e"
              % (r["energy"], r["ranks"], r["chosen"], r["rel_l2_vs_unfactored_fp16"]))
else:
    for lv in doc["levels"]:
        off, on = lv["forward_ms"]["off"], lv["forward_ms"]["on"]
        print("== rank %d  B=%d forward ms: off %.3f (%.3f .. %.3f)  on %.3f (%.3f .. %.3f)  x%.3f"
              % (lv["rank"], B, median(off), min(off), max(off), median(on), min(on), max(on), median(off) / median(on)))
        for b, rows in lv["layers"].items():
            for w in rows:
                print("B=%-3s conv%-2d %dx%d %4d->%4d cost %.3f tiles %4d  us dense %7.1f  pair %7.1f  fused %7.1f  x%.2f  bytes %d vs %d"
                      % (b, w["conv"], w["k"], w["k"], w["cin"], w["cout"], w["cost"], w["tiles"], w["us_dense"], w["us_pair"],
                         w["us_fused"], w["us_dense"] / w["us_fused"], w["bytes_up_vp"], w["bytes_wp"]))
    print("implied LOWRANK_MAX_COST: %.3f" % doc["implied_max_cost"])
