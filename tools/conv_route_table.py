"""Table of what the library's host queries answer for every conv geometry the engines build: rows of the statistics slab
(epilogue modes 0 and 3), mcamd_conv_fwd_f8_ok and mcamd_conv_tile_info (forward, dgrad, dgrad with `concurrent`).  Host
logic only: no GPU needed.  tests/test_host_cpu.py compares the committed table with the library it has built.

usage: python tools/conv_route_table.py [OUT.json]     (default: tests/golden/conv_route_table.json)
The committed table was written by the build BEFORE the single route function (api.hip conv_route) existed; rewrite it only
for a deliberate change of a route, and say which rows moved in the test.

File format: "cols" names the 12 geometry fields; a row is those 12 integers + an index into "results"; a result is
[rows(mode 0), rows(mode 3), f8_ok, tile_info fwd x 4, tile_info dgrad x 4, tile_info dgrad-concurrent x 4], with the
error text in place of the four integers where mcamd_conv_tile_info refuses the geometry.  "sections" = one list of rows
per environment (the MCAMD_* switches the tile choice reads)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COLS = ["B", "H", "W", "ksize", "cin", "cout", "x_ld", "x_choff", "stem", "pad", "x_wrap", "x_f8"]
BATCHES = (1, 2, 8, 32, 64, 128)
SIZES = ((416, 416), (352, 480), (608, 608))
ENVS = ({"MCAMD_PP": "0"}, {"MCAMD_PP": "2"}, {"MCAMD_PP": "2", "MCAMD_PP_BM": "192", "MCAMD_PP_BN": "128"},
        {"MCAMD_SMALL3X3": "0"}, {"MCAMD_SMALL3X3": "2"}, {"MCAMD_WRES": "0"}, {"MCAMD_WRES_MIN_ROUNDS": "1"},
        {"MCAMD_BK": "32"})


def conv_stack(cfg, H, W, keep=1.0):
    """(ksize, cin, cout, H, W) of every convolution of a darknet cfg; keep < 1: the widths filter pruning leaves."""
    from modelcompression_amd import nets
    shapes, out = [], []
    c, h, w = 3, H, W
    for b in nets.parse_cfg(cfg)[1:]:
        t = b["type"]
        if t == "convolutional":
            n = int(b["filters"])
            if keep < 1.0 and int(b.get("batch_normalize", 0)):
                n = max(1, round(n * keep))
            out.append((int(b["size"]), c, n, h, w))
            c = n
        elif t == "maxpool":
            h, w = h // 2, w // 2
        elif t == "reorg":
            c, h, w = c * 4, h // 2, w // 2
        elif t == "route":
            src = [shapes[len(shapes) + int(i)] for i in b["layers"].split(",")]
            c, h, w = sum(s[0] for s in src), src[0][1], src[0][2]
        shapes.append((c, h, w))
    return out


def forms(B, H, W, k, cin, cout, pad):
    """The operand forms of one layer: plain, split (3 C channels, upper third read 2 C lower), fp8 correction, a slice
    at channel 64 of a wider buffer, and split + slice."""
    from modelcompression_amd.ops import round_up
    ld = round_up(cin, 32)
    out = [(B, H, W, k, cin, cout, ld, 0, 0, pad, 0, 0), (B, H, W, k, cin, cout, ld + 64, 64, 0, pad, 0, 0)]
    if cin == 3 and pad == 0:
        out.append((B, H, W, k, 3, cout, 4, 0, 1, 0, 0, 0))
    if cin % 32 == 0:
        out.append((B, H, W, k, 3 * cin, cout, 2 * cin, 0, 0, pad, 2 * cin, 0))
        out.append((B, H, W, k, 3 * cin, cout, 2 * cin + 64, 64, 0, pad, 2 * cin, 0))
    if cin % 64 == 0:
        out.append((B, H, W, k, 2 * cin, cout, 2 * cin, 0, 0, pad, 0, cin))
    return out


def geometries(full):
    from modelcompression_amd import YOLOV2_VOC_CFG
    mini = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "mini.cfg")
    seen, out = set(), []

    def add(B, layers):
        for (k, cin, cout, h, w) in layers:
            for pad in (0, 1):
                for g in forms(B, h, w, k, cin, cout, pad):
                    if g not in seen:
                        seen.add(g)
                        out.append(g)
    for B in (BATCHES if full else (64,)):
        for (H, W) in (SIZES if full else SIZES[:1]):
            add(B, conv_stack(YOLOV2_VOC_CFG, H, W))
    for B in ((1, 2, 64) if full else (2,)):
        add(B, conv_stack(mini, 64, 64))
    add(64, conv_stack(YOLOV2_VOC_CFG, 416, 416, keep=0.6))      # 40 % of the filters pruned: ragged widths
    if full:
        add(128, conv_stack(YOLOV2_VOC_CFG, 416, 416, keep=0.4))
    return out


def query(gt):
    from modelcompression_amd import ops, _lib as L
    g = ops.geom(*gt[:12])
    res = [ops.stats_rows(g, L.EPI_RAW_F16), ops.stats_rows(g, L.EPI_RAW_F32), int(ops.conv_fwd_f8_ok(g))]
    for kw in ({}, {"dgrad": True}, {"dgrad": True, "concurrent": True}):
        try:
            res.extend(int(v) for v in ops.tile_info(g, **kw))
        except Exception as e:  # noqa: BLE001  (the error text is the recorded answer)
            res.append(str(e))
    return res


def table():
    from modelcompression_amd import _lib as L
    results, index, sections = [], {}, []
    for env in ({},) + ENVS:
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        L.reload_config()
        try:
            rows = []
            for gt in geometries(full=not env):
                r = query(gt)
                key = json.dumps(r)
                if key not in index:
                    index[key] = len(results)
                    results.append(r)
                rows.append(list(gt) + [index[key]])
            sections.append({"env": env, "rows": rows})
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k)
                else:
                    os.environ[k] = v
            L.reload_config()
    return {"cols": COLS, "results": results, "sections": sections}


def dumps(t):
    lines = ['{"cols": %s,' % json.dumps(t["cols"]), ' "results": [']
    lines.append(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in t["results"]))
    lines.append(' ],\n "sections": [')
    secs = []
    for s in t["sections"]:
        secs.append('  {"env": %s, "rows": [\n%s\n  ]}' % (
            json.dumps(s["env"]), ",\n".join("   " + json.dumps(r, separators=(",", ":")) for r in s["rows"])))
    lines.append(",\n".join(secs))
    lines.append(" ]}\n")
    return "\n".join(lines)


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "tests", "golden", "conv_route_table.json")
    t = table()
    with open(path, "w") as f:
        f.write(dumps(t))
    print("%d rows, %d distinct results -> %s" % (sum(len(s["rows"]) for s in t["sections"]), len(t["results"]), path))
