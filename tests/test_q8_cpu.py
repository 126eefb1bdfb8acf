"""CPU checks of the fp8 (e4m3) inference path: the new entry points are exported, the eligibility query's host logic,
the per-filter exponent rule, MCAMD_PRECISION=fp8, and the CPU restatement (q8_ref.py) against itself."""
import os
import re
import subprocess
import sys

import torch
import torch.nn.functional as F

from modelcompression_amd import _lib, ops
import q8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mcamd_conv_fwd_q8_ok", "mcamd_q8_elems", "mcamd_pack_q8", "mcamd_conv_fwd_q8", "mcamd_cast_q8")
# (H, cin, cout, k) of conv3 ... conv22 of yolov2-voc at 416 x 416
YOLO = [(104, 64, 128, 3), (104, 128, 64, 1), (104, 64, 128, 3), (52, 128, 256, 3), (52, 256, 128, 1), (52, 128, 256, 3),
        (26, 256, 512, 3), (26, 512, 256, 1), (26, 256, 512, 3), (26, 512, 256, 1), (26, 256, 512, 3), (13, 512, 1024, 3),
        (13, 1024, 512, 1), (13, 512, 1024, 3), (13, 1024, 512, 1), (13, 512, 1024, 3), (13, 1024, 1024, 3),
        (13, 1024, 1024, 3), (26, 512, 64, 1), (13, 1280, 1024, 3)]


def test_q8_entry_points_are_exported():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mcamd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name


def test_conv_fwd_q8_ok_host_logic():
    assert len(YOLO) == 20
    for B in (1, 128):
        for H, cin, cout, k in YOLO:
            g = ops.geom(B, H, H, k, cin, cout, ops.round_up(cin, 32))
            assert ops.conv_fwd_q8_ok(g), (B, H, cin, cout, k)
            nw, ne = ops.q8_elems(g)
            assert nw == ops.round_up(cout, 256) * k * k * cin and ne == ops.round_up(cout, 256)
    assert ops.conv_fwd_q8_ok(ops.geom(2, 13, 13, 3, 256, 512, 1280 + 256, 1024, 0, 1))      # a slice, shared-halo form
    for bad in (ops.geom(1, 208, 208, 3, 32, 64, 32),                         # conv2: cin % 64 != 0
                ops.geom(1, 13, 13, 3, 96, 64, 96),
                ops.geom(1, 416, 416, 3, 3, 32, 4, 0, 1),                     # the stem
                ops.geom(64, 13, 13, 3, 3 * 512, 1024, 2 * 512, x_wrap=1024),  # split-operand geometries
                ops.geom(64, 13, 13, 3, 2 * 512, 1024, 2 * 512, x_f8=512),
                ops.geom(1, 13, 13, 3, 64, 60, 64),                           # cout % 8 != 0
                ops.geom(1, 13, 13, 3, 64, 64, 96, 8),                        # slice offset not a multiple of 16
                ops.geom(1, 13, 13, 3, 128, 64, 128, 64)):                    # slice beyond x_ld
        assert not ops.conv_fwd_q8_ok(bad)


def _top(w):
    e = R.filter_exponents(w)
    a = w.abs().flatten(1).amax(1).double()
    return a * torch.pow(2.0, e.double()), e


def test_filter_exponents_put_the_largest_weight_in_224_448():
    gen = torch.Generator().manual_seed(0)
    w = torch.randn(512, 64, 3, 3, generator=gen) * torch.exp(4 * torch.randn(512, 1, 1, 1, generator=gen))
    top, _ = _top(w)
    assert bool(((top > 224) & (top <= 448)).all())
    n = torch.arange(-140, 100)
    for base in (1.0, 448.0, 0.875, float(torch.nextafter(torch.tensor(0.875), torch.tensor(1.0))), 0.75, 224.0):
        a = (base * torch.pow(2.0, n.double())).float()
        a = a[(a > 0) & torch.isfinite(a)]                  # fp32-subnormal maxima included
        top, e = _top(a.view(-1, 1, 1, 1))
        assert bool(((top > 224) & (top <= 448)).all()), base
    top, e = _top(torch.zeros(3, 8, 1, 1))
    assert bool((e == 0).all())
    w8, e = R.quantise_weights(torch.tensor([1.0, -0.5, 448.0 / 512, 0.0]).view(1, 4, 1, 1))
    assert int(e[0]) == 8 and R.deq(w8).flatten().tolist() == [256.0, -128.0, 224.0, 0.0]


def test_q_equals_torch_cast_on_codes_and_ties():
    codes = torch.arange(256, dtype=torch.uint8)
    vals = R.deq(codes)
    ok = ~torch.isnan(vals)
    assert int(ok.sum()) == 254
    assert torch.equal(R.q(vals[ok]), codes[ok])
    pos = vals[:0x7F].double()                                 # +0 ... 448 ascending
    ties = ((pos[:-1] + pos[1:]) / 2).float()
    for sign in (1.0, -1.0):
        t = sign * ties
        for v in (t, torch.nextafter(t, torch.zeros_like(t)), torch.nextafter(t, sign * torch.full_like(t, 1e9))):
            assert torch.equal(R.q(v), v.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
        lo, hi = codes[:0x7E].int(), codes[1:0x7F].int()
        even = torch.where(lo % 2 == 0, lo, hi) + (0 if sign > 0 else 0x80)
        assert torch.equal(R.q(t).int(), even)                 # ties to even
    assert R.q(torch.tensor([500.0, -1e9, 464.0, 1e-9, -1e-9])).tolist() == [0x7E, 0xFE, 0x7E, 0x00, 0x80]
    b = R.q(torch.randn(2, 8, 6, 6) * 3)
    assert torch.equal(R.deq(R.pool_bytes(b)), F.max_pool2d(R.deq(b), 2, 2))       # pooling codes = pooling values
    assert torch.equal(R.unkey(R.key(codes)), codes)


def test_block_float32_against_float64_is_inside_the_cap():
    """The byte-mismatch cap is one the reference alone meets: a block summed in float32 (another order and precision)
    against the float64 one."""
    gen = torch.Generator().manual_seed(1)
    worst = 0.0
    for cin, cout, k, H in ((64, 128, 3, 26), (1280, 256, 3, 13), (512, 256, 1, 26)):
        a8 = R.q(2.0 * F.leaky_relu(torch.randn(2, cin, H, H, generator=gen), 0.1))
        w = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
        mask = (torch.rand(w.shape, generator=gen) < 0.5).float()
        w8, e = R.quantise_weights(w, mask)
        scale, shift = torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.2
        v64 = R.block(a8, w8, e, scale, shift)
        v32 = R.block(a8, w8, e, scale, shift, dtype=torch.float32)
        for dst in ("plain", "pool"):
            share, adjacent = R.byte_mismatch(R.store_bytes(v32, dst), R.store_bytes(v64, dst))
            assert adjacent and share <= R.MISMATCH_CAP, (cin, dst, share)
            worst = max(worst, share)
        err = float((R.store_fp16(v32) - R.store_fp16(v64)).norm() / R.store_fp16(v64).norm())
        assert err < 1e-3
    print("worst float32 / float64 byte mismatch share: %.3g" % worst)


def test_precision_env_reaches_darknet():
    env = dict(os.environ, MCAMD_PRECISION="fp8")
    code = ("from modelcompression_amd import nets, YOLOV2_VOC_CFG; m = nets.Darknet(YOLOV2_VOC_CFG); print(m.precision)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "fp8"


def test_ref_forward_formats_and_error_level():
    """The whole-forward restatement on the mini network: no fp8 block = the fp16-storage oracle's level; quantising the
    eligible blocks raises the error to the e4m3 level and not beyond."""
    from oracle import darknet_ref as O
    blocks = O.parse_cfg(os.path.join(ROOT, "tests", "golden", "mini.cfg"))
    plan = O.plan(blocks)
    state = O.init_state(blocks, seed=0)
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        ref = O.forward(blocks, state, x)
        none = R.forward(blocks, state, x, [])
        convs = [op for op in plan if op["type"] == "conv"]
        elig = [op["id"] for op in convs[1:-1] if op["cin"] % 64 == 0]
        some = R.forward(blocks, state, x, elig)
    e0 = float((none - ref).norm() / ref.norm())
    assert e0 < 5e-3
    if elig:
        e1 = float((some - ref).norm() / ref.norm())
        print("mini network: fp16 storage %.2e, fp8 blocks %s %.2e" % (e0, elig, e1))
        assert e0 < e1 < 0.5
