"""Compressed model files (.mcz) without a device: the CPU path of compress.py writes the bytes of the numpy
restatement (wz_ref.py) and reads them back, Darknet.load_weights dispatches on the magic, damaged files are refused."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

from modelcompression_amd import _lib, compress, nets, ops
from modelcompression_amd._lib import McamdError
from modelcompression_amd.synthetic import init_synthetic
import q8_ref
import wz_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "golden", "mini.cfg")
Q8_CFG = os.path.join(ROOT, "tests", "golden", "q8_qat.cfg")
PAYLOADS = ("fp32", "fp16", "fp8")
NAMES = ("mcamd_wz_workspace_bytes", "mcamd_wz_pack", "mcamd_wz_unpack")


def make(cfg=MINI, seed=3, masked=False, seen=12345):
    model = init_synthetic(nets.Darknet(cfg), seed=seed)
    model.seen = seen
    if masked:
        g = torch.Generator().manual_seed(seed + 1)
        masks = [(torch.rand(conv.weight.shape, generator=g) > 0.8).float() for conv, _ in wz_ref.model_layers(model)]
        model.set_masks(masks)
    return model


def fp8_layers(model):
    """Some fp8 layers for a cfg of any width: every conv but the first and the last (the rule of the file under test is
    pinned separately)."""
    n = len(wz_ref.model_layers(model))
    return list(range(2, n))


def tensors(model):
    return {k: v.clone() for k, v in model.state_dict().items()}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("cfg", [MINI, Q8_CFG])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("payload", PAYLOADS)
def test_cpu_writer_matches_the_restatement(tmp_path, cfg, masked, payload):
    model = make(cfg, masked=masked)
    layers = fp8_layers(model)
    path = str(tmp_path / "m.mcz")
    compress.save_compressed(model, path, payload, layers)
    want = wz_ref.model_file(model, payload, layers)
    got = open(path, "rb").read()
    assert got == want
    # the method is the same writer
    model.save_compressed(path, payload, layers)
    assert open(path, "rb").read() == want
    if masked:
        assert any(r["words"] is not None for r in wz_ref.read(got)["records"])


@pytest.mark.parametrize("via", ["load_compressed", "load_weights"])
@pytest.mark.parametrize("payload", PAYLOADS)
def test_round_trip(tmp_path, via, payload):
    model = make(masked=True)
    layers = fp8_layers(model)
    path = str(tmp_path / "m.mcz")
    model.save_compressed(path, payload, layers)
    ref = wz_ref.read(open(path, "rb").read())
    fresh = nets.Darknet(MINI)
    if via == "load_weights":
        assert fresh.load_weights(path) is None
        masks = [conv.mask for conv, _ in wz_ref.model_layers(fresh)]
    else:
        masks = fresh.load_compressed(path)
    assert fresh.seen == 12345 and fresh._weights_dirty
    for (conv, bn), (conv0, bn0), rec, mask in zip(wz_ref.model_layers(fresh), wz_ref.model_layers(model), ref["records"], masks):
        w, m = wz_ref.decode(rec)
        assert same_bits(conv.weight.data, torch.from_numpy(w))
        assert torch.equal(mask, torch.from_numpy(m)) and conv.mask_flag and torch.equal(conv.mask, mask)
        if payload == "fp32":          # the bit patterns of weight * mask, -0 read back as +0
            wm = conv0.weight.data * conv0.mask
            assert same_bits(conv.weight.data, torch.where(wm == 0, torch.zeros_like(wm), wm))
        if bn is not None:
            for a, b in ((bn.bias, bn0.bias), (bn.weight, bn0.weight), (bn.running_mean, bn0.running_mean), (bn.running_var, bn0.running_var)):
                assert same_bits(a.data, b.data)
        else:
            assert same_bits(conv.bias.data, conv0.bias.data)
    # a second generation of the file is the first, byte for byte
    again = str(tmp_path / "again.mcz")
    fresh.save_compressed(again, payload, layers)
    if payload != "fp8":
        assert open(again, "rb").read() == open(path, "rb").read()


def test_set_masks_false_and_unmasked_files(tmp_path):
    model = make(masked=True)
    path = str(tmp_path / "m.mcz")
    model.save_compressed(path, "fp16")
    fresh = nets.Darknet(MINI)
    masks = fresh.load_compressed(path, set_masks=False)
    assert len(masks) == len(wz_ref.model_layers(fresh)) and not any(conv.mask_flag for conv, _ in wz_ref.model_layers(fresh))
    dense = make(masked=False)
    dense.save_compressed(path, "fp16")
    fresh = nets.Darknet(MINI)
    masks = fresh.load_compressed(path)
    assert all(bool((m == 1).all()) for m in masks) and not any(conv.mask_flag for conv, _ in wz_ref.model_layers(fresh))


def test_plain_weights_file_loads_as_before(tmp_path):
    model = make(masked=True)
    path = str(tmp_path / "m.weights")
    model.save_weights(path)
    assert not compress.is_compressed(path)
    fresh = nets.Darknet(MINI)
    fresh.load_weights(path)
    # the parent's reader, restated: 4 int32, then float32 arrays in save_conv_bn / save_conv order
    data = np.fromfile(path, dtype=np.float32, offset=16)
    pos = 0
    for conv, bn in wz_ref.model_layers(fresh):
        ts = [bn.bias, bn.weight, bn.running_mean, bn.running_var, conv.weight] if bn is not None else [conv.bias, conv.weight]
        for t in ts:
            assert same_bits(t.data, torch.from_numpy(data[pos:pos + t.numel()].copy()).view(t.shape))
            pos += t.numel()
        assert not conv.mask_flag
    assert pos == data.size and fresh.seen == 0


@pytest.mark.parametrize("payload", PAYLOADS)
def test_info_totals(tmp_path, payload):
    model = make(Q8_CFG, masked=True)
    layers = fp8_layers(model)
    path = str(tmp_path / "m.mcz")
    model.save_compressed(path, payload, layers)
    info = compress.compressed_info(path)
    ref = wz_ref.read(open(path, "rb").read())
    assert info["payload"] == payload and info["seen"] == 12345
    assert info["bytes"] == os.path.getsize(path) == 24 + sum(l["bytes"] for l in info["layers"])
    assert info["bytes"] == wz_ref.closed_form_bytes([(l["shape"], r["bn"], wz_ref.KIND[l["kind"]], l["kept"])
                                                      for l, r in zip(info["layers"], ref["records"])])
    for l, r in zip(info["layers"], ref["records"]):
        assert l["shape"] == r["shape"] and l["kept"] == r["kept"] and wz_ref.KIND[l["kind"]] == r["kind"]
        assert l["bitmask"] == (r["words"] is not None) and l["weights"] == int(np.prod(r["shape"]))
    plain = str(tmp_path / "m.weights")
    model.save_weights(plain)
    assert info["dense_bytes"] == os.path.getsize(plain) == wz_ref.dense_bytes([(r["shape"], r["bn"]) for r in ref["records"]])
    assert info["ratio"] == info["dense_bytes"] / info["bytes"] and info["ratio"] > 1.0
    assert info["kept"] == sum(r["kept"] for r in ref["records"])


@pytest.mark.parametrize("kind", [wz_ref.FP32, wz_ref.FP16, wz_ref.FP8])
def test_bitmask_or_dense_rule_at_its_break_even(kind):
    """(4, 64, 1, 1) = 256 weights = 4 words = 32 bytes of bit words: the bitmask pays iff 32 + kept elem < 256 elem."""
    n, elem = 256, wz_ref.ELEM[kind]
    last = (n * elem - 32 - 1) // elem          # the largest kept count with bit words
    for kept, bits in ((last, True), (last + 1, False), (n, False), (0, True)):
        assert compress.has_bits(n, kept, kind) == bits == wz_ref.bits_rule(n, kept, kind)
        w = torch.zeros(n)
        w[torch.randperm(n, generator=torch.Generator().manual_seed(kept))[:kept]] = 1.5
        w = w.view(4, 64, 1, 1)
        got, want = compress._encode_cpu(w, None, kind), wz_ref.encode_layer(w, None, kind)
        assert got["kept"] == want["kept"] == kept
        assert (got["words"] is not None) == (want["words"] is not None) == bits
        assert got["values"].tobytes() == want["values"].tobytes() and got["values"].size == (kept if bits else n)
        if bits:
            assert got["words"].tobytes() == want["words"].tobytes()


SCALED_MAX = {224.0: (224.5, 232.0), 240.0: (232.5, 247.5), 256.0: (248.5, 271.5), 448.0: (432.5, 448.0)}


def _filter_with_max_code(top, seed):
    """A (1, 64, 1, 1) filter whose largest |weight|, scaled by the filter's exponent into (224, 448], ROUNDS to the e4m3
    value `top`; smaller random weights of both signs around it, the whole filter times an arbitrary power of two."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = SCALED_MAX[top]
    w = (torch.rand(64, generator=g) * 2 - 1) * 200.0
    w[int(torch.randint(0, 64, (1,), generator=g))] = (lo + (hi - lo) * float(torch.rand(1, generator=g))) * (1 if seed % 2 else -1)
    return (w * 2.0 ** int(torch.randint(-12, 4, (1,), generator=g))).view(1, 64, 1, 1)


@pytest.mark.parametrize("top", [224.0, 240.0, 256.0, 448.0])
def test_fp8_values_are_idempotent(top):
    """Re-quantising the dequantised masters can move a filter's exponent by one with every code doubled; the VALUES
    value(code) 2^-e do not move."""
    for seed in range(20):
        w = _filter_with_max_code(top, seed)
        codes, e = q8_ref.quantise_weights(w)
        assert float(q8_ref.deq(codes).abs().max()) == top
        v1 = (q8_ref.deq(codes).double() * 2.0 ** (-e.double()).view(-1, 1, 1, 1)).float()
        enc = compress._encode_cpu(w, None, wz_ref.FP8)
        assert int(enc["exps"][0]) == int(e[0])
        rec = dict(n=64, kind=wz_ref.FP8, cout=1, kept=enc["kept"], words=enc["words"], values=enc["values"], exps=enc["exps"])
        back, _ = compress._decode_cpu(rec, "filter")
        assert same_bits(torch.from_numpy(back).view(1, 64, 1, 1), torch.where(v1 == 0, torch.zeros_like(v1), v1))
        codes2, e2 = q8_ref.quantise_weights(torch.from_numpy(back).view(1, 64, 1, 1))
        v2 = (q8_ref.deq(codes2).double() * 2.0 ** (-e2.double()).view(-1, 1, 1, 1)).float()
        assert torch.equal(v2, torch.from_numpy(back).view(1, 64, 1, 1)), (top, seed, int(e[0]), int(e2[0]))


def test_all_zero_filter():
    w = torch.randn(3, 64, 1, 1, generator=torch.Generator().manual_seed(0))
    w[1] = 0.0
    w[2, :5] = -0.0
    for kind in (wz_ref.FP32, wz_ref.FP16, wz_ref.FP8):
        enc = compress._encode_cpu(w, None, kind)
        ref = wz_ref.encode_layer(w, None, kind)
        assert enc["kept"] == ref["kept"] == 64 + 59
        keep = np.unpackbits(ref["all_words"].view(np.uint8), bitorder="little")[:192]
        assert keep[:64].all() and not keep[64:128].any() and not keep[128:133].any() and keep[133:].all()
        if kind == wz_ref.FP8:
            assert int(enc["exps"][1]) == 0 and enc["exps"].tobytes() == ref["exps"].tobytes()


def _file(tmp_path, payload="fp16"):
    model = make(masked=True)
    path = str(tmp_path / "m.mcz")
    model.save_compressed(path, payload)
    return path, open(path, "rb").read()


def test_damaged_files_are_refused(tmp_path):
    path, data = _file(tmp_path)
    bad = str(tmp_path / "bad.mcz")
    for cut in (10, 24, 40, len(data) // 2, len(data) - 1):
        open(bad, "wb").write(data[:cut])
        for call in (lambda: nets.Darknet(MINI).load_compressed(bad), lambda: compress.compressed_info(bad)):
            with pytest.raises(McamdError, match="truncated"):
                call()
    open(bad, "wb").write(data + b"\0" * 8)
    with pytest.raises(McamdError, match="behind the last record"):
        compress.compressed_info(bad)
    open(bad, "wb").write(b"MCZX" + data[4:])
    with pytest.raises(McamdError, match="magic"):
        nets.Darknet(MINI).load_compressed(bad)
    open(bad, "wb").write(data[:4] + struct.pack("<I", 2) + data[8:])
    with pytest.raises(McamdError, match="version 2"):
        nets.Darknet(MINI).load_compressed(bad)
    with pytest.raises(McamdError, match="version 2"):
        compress.compressed_info(bad)


def test_shape_mismatch_leaves_the_model_unchanged(tmp_path):
    path, data = _file(tmp_path)
    other = make(Q8_CFG, seed=9)
    before = tensors(other)
    with pytest.raises(McamdError, match="conv"):
        other.load_weights(path)
    after = tensors(other)
    assert before.keys() == after.keys() and all(same_bits(before[k].float(), after[k].float()) for k in before)
    assert other.seen == 12345 and not any(conv.mask_flag for conv, _ in wz_ref.model_layers(other))
    # the second record's cout off by one, the first one intact: still nothing is written
    cout = struct.unpack_from("<i", data, 24)[0]
    first = wz_ref.read(data)["records"][0]
    second = 24 + 32 + 4 * (-(-4 * cout // 8) * 8) + (8 * -(-int(np.prod(first["shape"])) // 64) if first["words"] is not None else 0) \
        + -(-first["values"].nbytes // 8) * 8
    c2 = struct.unpack_from("<i", data, second)[0]
    assert c2 == wz_ref.read(data)["records"][1]["shape"][0]
    mini = make(seed=11, seen=7)
    before = tensors(mini)
    bad = str(tmp_path / "bad.mcz")
    open(bad, "wb").write(data[:second + 4] + struct.pack("<i", struct.unpack_from("<i", data, second + 4)[0] + 1) + data[second + 8:])
    with pytest.raises(McamdError):
        mini.load_compressed(bad)
    after = tensors(mini)
    assert all(same_bits(before[k].float(), after[k].float()) for k in before) and mini.seen == 7


def test_out_of_scope_models_are_named():
    model = make()
    wz_ref.model_layers(model)[1][0].border_bias = torch.zeros(16, 4)
    with pytest.raises(McamdError, match="border tables of slim_export models"):
        model.save_compressed("unused.mcz")
    model = make()
    model.blocks.insert(2, {"type": "connected", "output": "4", "activation": "linear"})
    with pytest.raises(McamdError, match=r"\[connected\] block"):
        model.save_compressed("unused.mcz")
    with pytest.raises(McamdError, match="payload"):
        make().save_compressed("unused.mcz", "int4")
    assert not os.path.exists("unused.mcz")


def test_default_fp8_layers_rule():
    model = make(Q8_CFG)
    convs = wz_ref.model_layers(model)
    want = [i + 1 for i, (conv, bn) in enumerate(convs) if bn is not None and 0 < i < len(convs) - 1 and conv.weight.shape[1] % 64 == 0]
    assert compress.default_fp8_layers(model) == want and want


def test_symbols_are_declared_exported_bound_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.lib()
    for name in NAMES:
        assert re.search(r"\b(int|size_t) %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct mcamd_wz_seg" in hdr
    for f in (ops.wz_pack, ops.wz_unpack, compress.save_compressed, compress.load_compressed, compress.compressed_info,
              nets.Darknet.save_compressed, nets.Darknet.load_compressed):
        assert callable(f)
    for name, value in (("MCAMD_WZ_FP32", _lib.WZ_FP32), ("MCAMD_WZ_FP16", _lib.WZ_FP16), ("MCAMD_WZ_FP8", _lib.WZ_FP8),
                        ("MCAMD_WZ_BLOCK_WORDS", _lib.WZ_BLOCK_WORDS)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
    # the ctypes struct is the header's, field for field
    body = re.search(r"typedef struct mcamd_wz_seg \{(.*?)\} mcamd_wz_seg;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f[0] for f in _lib.WzSeg._fields_] and C.sizeof(_lib.WzSeg) == 72
    src = open(os.path.join(ROOT, "modelcompression_amd", "build.py")).read()
    assert '"wpack.hip"' in src


def seg(**kw):
    s = _lib.WzSeg()
    s.w, s.mask, s.n, s.cout, s.kind = 4096, None, 189, 3, _lib.WZ_FP16
    for k, v in kw.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("bad, text, unpack_text", [
    (dict(w=None), "bad tensor", None),
    (dict(n=0), "bad tensor", None),
    (dict(n=190), "bad tensor", None),
    (dict(kind=3), "bad value kind 3", None),
    (dict(block0=1), "block0 1 is not the running sum 0", None),
    # pack lays the words and exponents out itself; unpack reads them where the caller has them, inside the arrays given
    (dict(word0=3), "word0 3 is not the running sum 0", "bit words [3, +3) outside the 3 given"),
    (dict(word0=-1), "word0 -1 is not the running sum 0", "bit words [-1, +3) outside the 3 given"),
    (dict(kind=_lib.WZ_FP8, exp0=2), "exp0 2 is not the running sum 0", "exponents [2, +3) outside the 3 given"),
])
def test_entry_points_refuse_bad_tables(bad, text, unpack_text):
    """Every argument error is refused before a launch (the pointers below are never dereferenced)."""
    lib, P = _lib.lib(), 4096
    arr = (_lib.WzSeg * 1)(seg(**bad))
    err = lambda: lib.mcamd_last_error().decode()
    assert lib.mcamd_wz_pack(arr, P, 1, P, 3, P, P, 3, P, 1 << 20, P, 1 << 20, None) == -1
    assert text in err() and err().startswith("wz_pack:"), err()
    assert lib.mcamd_wz_unpack(arr, P, 1, P, 3, P, 3, P, 1 << 20, P, 1 << 20, None) == -1
    assert (unpack_text or text) in err() and err().startswith("wz_unpack:"), err()


def test_entry_points_refuse_short_buffers():
    lib, P = _lib.lib(), 4096
    err = lambda: lib.mcamd_last_error().decode()
    arr = (_lib.WzSeg * 1)(seg())
    assert lib.mcamd_wz_pack(None, P, 1, P, 3, P, P, 0, P, 1 << 20, P, 1 << 20, None) == -1 and "null argument" in err()
    assert lib.mcamd_wz_pack(arr, P, 1, P, 2, P, None, 0, P, 1 << 20, P, 1 << 20, None) == -1 and "3 bit words needed, room for 2" in err()
    assert lib.mcamd_wz_pack(arr, P, 1, P, 3, P, None, 0, P, 376, P, 1 << 20, None) == -1 and "room for 384 bytes" in err()
    assert lib.mcamd_wz_pack(arr, P, 1, P, 3, P, None, 0, P, 384, P, 8, None) != 0 and "workspace too small" in err()
    assert lib.mcamd_wz_workspace_bytes(1, 1) >= 8 + 4 + 8 + 4
    arr = (_lib.WzSeg * 1)(seg(kept=190))
    assert lib.mcamd_wz_unpack(arr, P, 1, P, 3, None, 0, P, 1 << 20, P, 1 << 20, None) == -1 and "kept 190 of 189" in err()
    arr = (_lib.WzSeg * 1)(seg(kept=100, val0=8))
    assert lib.mcamd_wz_unpack(arr, P, 1, P, 3, None, 0, P, 200, P, 1 << 20, None) == -1 and "outside the 200 bytes given" in err()
    arr = (_lib.WzSeg * 1)(seg(kept=100, val0=4))
    assert lib.mcamd_wz_unpack(arr, P, 1, P, 3, None, 0, P, 1 << 20, P, 1 << 20, None) == -1 and "outside" in err()
    arr = (_lib.WzSeg * 1)(seg(kept=100))
    assert lib.mcamd_wz_unpack(arr, P, 1, None, 0, None, 0, P, 1 << 20, P, 1 << 20, None) == -1 and "bit words [0, +3) outside the 0 given" in err()
    arr = (_lib.WzSeg * 1)(seg(dense=1))
    assert lib.mcamd_wz_unpack(arr, P, 1, None, 0, None, 0, P, 376, P, 1 << 20, None) == -1 and "outside the 376 bytes given" in err()


def test_refused_while_a_plan_records():
    lib, P = _lib.lib(), 4096
    streams = (C.c_void_p * 1)(None)
    assert lib.mcamd_plan_begin(streams, 1) == 0
    try:
        arr = (_lib.WzSeg * 1)(seg())
        assert lib.mcamd_wz_pack(arr, P, 1, P, 3, P, None, 0, P, 1 << 20, P, 1 << 20, None) == -1
        assert "wz_pack: not recordable" in lib.mcamd_last_error().decode()
        assert lib.mcamd_wz_unpack(arr, P, 1, P, 3, None, 0, P, 1 << 20, P, 1 << 20, None) == -1
        assert "wz_unpack: not recordable" in lib.mcamd_last_error().decode()
    finally:
        plan = lib.mcamd_plan_end()
        assert plan and lib.mcamd_plan_launches(plan) == 0
        lib.mcamd_plan_destroy(plan)


def test_wrappers_have_no_cpu_path():
    w = torch.zeros(3, 7, 3, 3)
    with pytest.raises(McamdError):
        ops.wz_pack([dict(w=w, mask=None, kind=_lib.WZ_FP16)])
    with pytest.raises(McamdError):
        ops.wz_unpack([dict(w=w, mask=None, kind=_lib.WZ_FP16, dense=1, kept=0, val0=0)], None, None, None)
