"""The "w4" payload of a compressed model file (.mcz) without a device: the CPU path of compress.py writes the
bytes of the numpy restatement (wz_w4_ref.py) and reads them back as w4_ref.dequantised masters; the bit-words rule on both
sides of its break-even; the round-trip property the losslessness claim rests on and the one corner outside it; damaged files
are refused with the model untouched."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

from modelcompression_amd import _lib, compress, nets
from modelcompression_amd._lib import McamdError
from modelcompression_amd.synthetic import init_synthetic
import w4_ref
import wz_ref
import wz_w4_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q8_CFG = os.path.join(ROOT, "tests", "golden", "q8_qat.cfg")


def make(seed=3, masked=False, seen=12345):
    model = init_synthetic(nets.Darknet(Q8_CFG), seed=seed)
    model.seen = seen
    if masked:
        g = torch.Generator().manual_seed(seed + 1)
        model.set_masks([(torch.rand(conv.weight.shape, generator=g) > 0.8).float() for conv, _ in wz_ref.model_layers(model)])
    return model


def tensors(model):
    return {k: v.clone() for k, v in model.state_dict().items()}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------- the writer and the reader
@pytest.mark.parametrize("masked", [False, True])
def test_cpu_writer_matches_the_restatement(tmp_path, masked):
    model = make(masked=masked)
    layers = compress.default_fp8_layers(model)
    assert layers == [3, 4, 5, 6, 7, 8, 9, 10]
    path = str(tmp_path / "m.mcz")
    compress.save_compressed(model, path, "w4")                  # the default layers
    want = wz_w4_ref.model_file(model, layers)
    assert open(path, "rb").read() == want
    model.save_compressed(path, "w4", layers + [2])              # conv2: 32 input channels, one group per tap
    got = open(path, "rb").read()
    assert got == wz_w4_ref.model_file(model, layers + [2]) and got != want
    recs = wz_w4_ref.read(want)["records"]
    assert [r["kind"] for r in recs] == [wz_ref.FP16] * 2 + [wz_w4_ref.W4] * 8 + [wz_ref.FP16]
    # a dense layer keeps too many codes for bit words to pay (about 12 % are zero); an 80 %-masked one has them
    assert all((r["words"] is not None) == masked for r in recs if r["kind"] == wz_w4_ref.W4)
    info = compress.compressed_info(path)
    assert info["payload"] == "w4" and [l["kind"] for l in info["layers"]] == ["fp16"] + ["w4"] * 9 + ["fp16"]


@pytest.mark.parametrize("via", ["load_compressed", "load_weights"])
@pytest.mark.parametrize("masked", [False, True])
def test_reload_gives_the_dequantised_masters_and_the_kept_bits(tmp_path, via, masked):
    model = make(masked=masked)
    layers = compress.default_fp8_layers(model)
    path = str(tmp_path / "m.mcz")
    model.save_compressed(path, "w4")
    fresh = nets.Darknet(Q8_CFG)
    if via == "load_weights":
        assert fresh.load_weights(path) is None
        masks = [conv.mask if masked else torch.ones_like(conv.weight.data) for conv, _ in wz_ref.model_layers(fresh)]
    else:
        masks = fresh.load_compressed(path)
    assert fresh.seen == 12345 and fresh._weights_dirty
    ref = wz_w4_ref.read(open(path, "rb").read())
    for i, ((conv, bn), (conv0, bn0), rec, mask) in enumerate(zip(wz_ref.model_layers(fresh), wz_ref.model_layers(model),
                                                                 ref["records"], masks)):
        m0 = conv0.mask if conv0.mask_flag else None
        if i + 1 in layers:
            codes, g, e4, values, _ = w4_ref.quantise(conv0.weight.data, m0)
            assert same_bits(conv.weight.data, w4_ref.dequantised(values, e4))
            keep = ((codes & 7) != 0).float()
            assert torch.equal(mask, keep if masked else torch.ones_like(keep))
        else:
            wm = conv0.weight.data * m0 if masked else conv0.weight.data
            assert same_bits(conv.weight.data, wm.half().float() + 0.0)        # (-0 reads back as +0)
        w, m = wz_w4_ref.decode(rec)
        assert same_bits(conv.weight.data, torch.from_numpy(w)) and torch.equal(mask, torch.from_numpy(m))
        assert conv.mask_flag == masked and (not masked or torch.equal(conv.mask, mask))
        for a, b in ((bn.bias, bn0.bias), (bn.weight, bn0.weight), (bn.running_mean, bn0.running_mean),
                     (bn.running_var, bn0.running_var)) if bn is not None else ((conv.bias, conv0.bias),):
            assert same_bits(a.data, b.data)


def test_bit_words_rule_on_both_sides():
    """(5, 32, 1, 1) = 160 weights, 3 words (n % 64 = 32) = 24 bytes against 80 bytes of codes: bit words pay iff
    24 + ceil(kept / 2) < 80, that is kept <= 110."""
    n = 160
    for kept, bits in ((0, True), (109, True), (110, True), (111, False), (112, False), (159, False), (160, False)):
        assert compress.has_bits(n, kept, _lib.WZ_W4) == bits == wz_w4_ref.bits_rule(n, kept)
        w = torch.zeros(n)
        w[torch.randperm(n, generator=torch.Generator().manual_seed(kept))[:kept]] = -1.5
        w = w.view(5, 32, 1, 1)
        got, want = compress._encode_cpu(w, None, _lib.WZ_W4), wz_w4_ref.encode_layer(w, None)
        assert got["kept"] == want["kept"] == kept
        assert (got["words"] is not None) == (want["words"] is not None) == bits
        assert got["values"].size == (kept if bits else n) and got["values"].tobytes() == want["stored"].tobytes()
        packed = compress._pack_codes(got["values"], 4)
        assert packed.tobytes() == wz_w4_ref.nibbles(want["stored"]).tobytes() and packed.size == (got["values"].size + 1) // 2
        if got["values"].size % 2:
            assert packed[-1] >> 4 == 0
        assert got["exps"].tobytes() == want["e4"].tobytes() and got["shifts"].tobytes() == want["shifts"].tobytes()
        if bits:
            assert got["words"].tobytes() == want["words"].tobytes() and int(got["words"][-1]) >> 32 == 0
    # (64, 64, 1, 1): n % 64 == 0, 512 bytes of words against 2048 of codes: ceil(kept / 2) <= 1535
    for kept, bits in ((3069, True), (3070, True), (3071, False)):
        assert compress.has_bits(4096, kept, _lib.WZ_W4) == bits == wz_w4_ref.bits_rule(4096, kept)


def test_info_totals(tmp_path):
    model = make(masked=True)
    path = str(tmp_path / "m.mcz")
    model.save_compressed(path, "w4")
    info = compress.compressed_info(path)
    ref = wz_w4_ref.read(open(path, "rb").read())
    assert info["payload"] == "w4" and info["seen"] == 12345
    assert info["bytes"] == os.path.getsize(path) == 24 + sum(l["bytes"] for l in info["layers"])
    kinds = {"w4": wz_w4_ref.W4, "fp16": wz_ref.FP16}
    assert info["bytes"] == wz_w4_ref.closed_form_bytes([(l["shape"], r["bn"], kinds[l["kind"]], l["kept"])
                                                         for l, r in zip(info["layers"], ref["records"])])
    for l, r in zip(info["layers"], ref["records"]):
        assert l["shape"] == r["shape"] and l["kept"] == r["kept"] and kinds[l["kind"]] == r["kind"]
        assert l["bitmask"] == (r["words"] is not None) and l["weights"] == int(np.prod(r["shape"]))
    assert info["kept"] == sum(r["kept"] for r in ref["records"])
    assert info["dense_bytes"] == wz_ref.dense_bytes([(r["shape"], r["bn"]) for r in ref["records"]])
    assert info["ratio"] == info["dense_bytes"] / info["bytes"] and info["ratio"] > 8.0


# ----------------------------------------------------------------------------- the losslessness claim and its boundary
def round_trip(w, mask=None):
    """(first quantisation, quantisation of its dequantised masters under the kept-bit mask a reload sets)"""
    a = w4_ref.quantise(w, mask)
    back = w4_ref.dequantised(a[3], a[2])
    return a, w4_ref.quantise(back, None), back


def adversarial():
    g = torch.Generator().manual_seed(11)
    w = torch.randn(6, 64, 3, 3, generator=g) * 0.05
    w[0, 5, 1, 1] = 40.0                                   # an outlier: every other group of the filter sits far below it
    w[1, 32:, :, :] *= 2.0 ** -20                          # a group at 2^-20 of the filter's scale: clamped at g = -5
    w[2, :32, 0, :] = 0.0                                  # all-zero groups
    w[3] = 0.0                                             # an all-zero filter
    w[4, :, :, :] = -w[4].abs()                            # one sign
    return w


@pytest.mark.parametrize("case", ["gauss3x3", "gauss1x1", "masked3x3", "masked1x1", "adversarial"])
def test_requantising_the_masters_gives_the_same_values_and_bytes(case):
    g = torch.Generator().manual_seed(5)
    if case == "adversarial":
        w, mask = adversarial(), None
    else:
        k = 3 if case.endswith("3x3") else 1
        w = torch.randn(48, 128, k, k, generator=g) * torch.pow(2.0, torch.randint(-6, 7, (48, 1, 1, 1), generator=g).float())
        mask = (torch.rand(w.shape, generator=g) > 0.8).float() if case.startswith("masked") else None
    (c1, g1, e1, v1, b1), (c2, g2, e2, v2, b2), back = round_trip(w, mask)
    assert torch.equal(e1, e2) and torch.equal(v1, v2) and torch.equal(b1, b2)
    assert same_bits(w4_ref.dequantised(v2, e2), back)
    # the dequantised filter maximum is 128 or 192 in the scaled domain (never the 224 tie, below)
    top = v1.abs().flatten(1).amax(1)
    assert set(top.tolist()) <= {0.0, 128.0, 192.0}
    # the third generation is the second, codes and shifts included
    c3, g3, e3, v3, b3 = w4_ref.quantise(w4_ref.dequantised(v2, e2), None)
    assert torch.equal(c3, c2) and torch.equal(g3, g2) and torch.equal(e3, e2)


def test_a_group_whose_maximum_rounds_to_three_comes_back_one_shift_lower():
    """Scaled group maximum 3.25 under g = 0 rounds to grid value 3 = 6 * 2^-1: the reloaded group takes g = -1 and codes of
    the doubled magnitudes, the same values."""
    w = torch.zeros(1, 64, 1, 1)
    w[0, 0] = 128.0                                        # e4_f = 0: the scaled domain is the weights'
    w[0, 32:36, 0, 0] = torch.tensor([3.25, -1.0, 0.5, 2.0])
    (c1, g1, e1, v1, b1), (c2, g2, e2, v2, b2), _ = round_trip(w)
    assert int(e1[0]) == int(e2[0]) == 0
    assert g1.view(-1).tolist() == [5, 0] and g2.view(-1).tolist() == [5, -1]
    assert c1.view(-1)[32:36].tolist() == [5, 8 | 2, 1, 4] and c2.view(-1)[32:36].tolist() == [7, 8 | 4, 2, 6]
    assert torch.equal(v1, v2) and torch.equal(b1, b2) and v1.view(-1)[32:36].tolist() == [3.0, -1.0, 0.5, 2.0]
    # ... and such groups occur in Gaussian layers too
    g = torch.Generator().manual_seed(5)
    (_, g1, _, v1, _), (_, g2, _, v2, _), _ = round_trip(torch.randn(48, 128, 3, 3, generator=g))
    assert bool((g2 == g1 - 1).any()) and bool(((g2 == g1) | (g2 == g1 - 1)).all()) and torch.equal(v1, v2)


def corner(top):
    w = torch.zeros(1, 64, 1, 1)
    w[0, 0], w[0, 32], w[0, 33] = top, 2.0 ** -14, 3 * 2.0 ** -14
    return w


def test_the_224_tie_is_the_one_filter_outside_the_claim():
    """A filter maximum of 0.875 scales to exactly 224, a tie that rounds to 256: the reloaded filter takes e4_f - 1 and every
    scaled value halves.  A group clamped at g = -5 with an odd-mantissa code cannot follow: 0.5 * 2^-5 becomes 0.25 * 2^-5 and
    ties to 0.  The same filter with maximum 0.75 (192 scaled, a grid point) stays put."""
    (c1, g1, e1, v1, b1), (c2, g2, e2, v2, b2), back = round_trip(corner(0.75))
    assert int(e1[0]) == int(e2[0]) == 8 and torch.equal(v1, v2) and torch.equal(b1, b2)
    assert back.view(-1)[[0, 32, 33]].tolist() == [0.75, 2.0 ** -14, 3 * 2.0 ** -14]
    (c1, g1, e1, v1, b1), (c2, g2, e2, v2, b2), back = round_trip(corner(0.875))
    assert int(e1[0]) == 8 and float(v1.view(-1)[0]) == 256.0 and g1.view(-1).tolist() == [6, -5]
    assert back.view(-1)[[0, 32, 33]].tolist() == [1.0, 2.0 ** -14, 3 * 2.0 ** -14]
    assert int(e2[0]) == 7 and g2.view(-1).tolist() == [5, -5]
    again = w4_ref.dequantised(v2, e2)
    assert again.view(-1)[[0, 32, 33]].tolist() == [1.0, 0.0, 2.0 ** -12] and not torch.equal(again, back)
    # the file itself still holds the first generation exactly: compress.py's codes are the restatement's in both filters
    for top in (0.75, 0.875):
        enc, want = compress._encode_cpu(corner(top), None, _lib.WZ_W4), wz_w4_ref.encode_layer(corner(top), None)
        assert enc["values"].tobytes() == want["stored"].tobytes() and enc["shifts"].tobytes() == want["shifts"].tobytes()


def test_second_generation_of_the_file_equals_the_third(tmp_path):
    for masked in (False, True):
        paths = [str(tmp_path / ("g%d.mcz" % i)) for i in range(3)]
        model = make(masked=masked)
        for i, path in enumerate(paths):
            model.save_compressed(path, "w4")
            model = nets.Darknet(Q8_CFG)
            model.load_weights(path)
        first, second, third = (open(p, "rb").read() for p in paths)
        assert second == third and len(first) >= len(second)
        # the masters do not move from the first generation on
        a, b = nets.Darknet(Q8_CFG), nets.Darknet(Q8_CFG)
        a.load_compressed(paths[0])
        b.load_compressed(paths[2])
        assert all(same_bits(x.weight.data, y.weight.data) for (x, _), (y, _) in zip(wz_ref.model_layers(a), wz_ref.model_layers(b)))


# ----------------------------------------------------------------------------- refusals
def test_damaged_files_are_refused_and_leave_the_model_untouched(tmp_path):
    model = make(masked=True)
    path, bad = str(tmp_path / "m.mcz"), str(tmp_path / "bad.mcz")
    model.save_compressed(path, "w4")
    data = open(path, "rb").read()
    recs = compress._parse(path, payload=False)["records"]
    starts = np.cumsum([24] + [r["bytes"] for r in recs])
    w4 = [(int(s), r) for s, r in zip(starts, recs) if r["kind"] == _lib.WZ_W4 and r["bits"]]
    start, rec = [(s, r) for s, r in w4 if r["kept"] % 2][0]           # an odd kept count: the last code byte has a free nibble
    last_code = rec["val0"] + (rec["kept"] + 1) // 2 - 1
    assert data[last_code] >> 4 == 0 and data[rec["shift0"]] <= 11

    def hit(offset, value):
        raw = bytearray(data)
        raw[offset] = value
        return bytes(raw)

    word = int.from_bytes(data[rec["word0"]:rec["word0"] + 8], "little")
    assert word, "the first word of an 80 %-masked record keeps something in a seeded model"
    flags = struct.unpack_from("<I", data, start + 16)[0]
    assert flags & _lib.WZ_F_BITS and flags >> 8 == _lib.WZ_W4
    cases = [
        (data[:rec["val0"] + 3], "truncated"),
        (data[:rec["shift0"] + 1], "truncated"),
        (data[:-1], "truncated"),
        (data[:rec["word0"]] + (word ^ (word & -word)).to_bytes(8, "little") + data[rec["word0"] + 8:], "bit words do not select"),
        (hit(last_code, data[last_code] | 0x30), "unused nibble"),
        (hit(rec["shift0"] + 2, 12), "group shift byte of 12"),
        (data[:start + 16] + struct.pack("<I", flags ^ _lib.WZ_F_BITS) + data[start + 20:], "damaged record header"),
        (hit(rec["val0"], data[rec["val0"]] & 0xF8), "do not hold the"),                      # a kept weight with grid index 0
        (data[:8] + struct.pack("<I", _lib.WZ_FP8) + data[12:], "damaged record header"),      # 4-bit codes in an "fp8" file
    ]
    for raw, text in cases:
        open(bad, "wb").write(raw)
        target = make(seed=9, seen=7)
        before = tensors(target)
        with pytest.raises(McamdError, match=text):
            target.load_weights(bad)
        after = tensors(target)
        assert before.keys() == after.keys() and all(same_bits(before[k].float(), after[k].float()) for k in before), text
        assert target.seen == 7 and not any(conv.mask_flag for conv, _ in wz_ref.model_layers(target))
    target = make(seed=9, seen=7)
    target.load_weights(path)                                 # the undamaged file loads
    assert target.seen == 12345


def test_a_layer_without_groups_of_32_is_refused(tmp_path):
    model = make()
    path = str(tmp_path / "m.mcz")
    with pytest.raises(McamdError, match="conv1 has 3 input channels"):
        model.save_compressed(path, "w4", [1, 3])
    with pytest.raises(McamdError, match="does not have"):
        model.save_compressed(path, "w4", [3, 40])
    assert not os.path.exists(path)


# ----------------------------------------------------------------------------- the C surface
def test_symbols_and_the_segment_struct():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.lib()
    for name in ("mcamd_wz_pack_w4", "mcamd_wz_unpack_w4"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        # the entry points of before with the shift bytes as two trailing arguments
        assert _lib.SIGNATURES[name][1][:-2] == _lib.SIGNATURES[name[:-3]][1]
    assert re.search(r"#define MCAMD_WZ_W4 %d\b" % _lib.WZ_W4, hdr) and _lib.WZ_W4 == 5 == compress.PAYLOADS["w4"]
    assert compress.VERSION == 1
    body = re.search(r"typedef struct mcamd_wz_seg \{(.*?)\} mcamd_wz_seg;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f[0] for f in _lib.WzSeg._fields_] and C.sizeof(_lib.WzSeg) == 72
    assert fields[:11] == ["w", "mask", "n", "word0", "val0", "kept", "cout", "kind", "exp0", "dense", "block0"]


def seg(**kw):
    s = _lib.WzSeg()
    s.w, s.mask, s.n, s.cout, s.kind = 4096, None, 5 * 64 * 9, 5, _lib.WZ_W4 | 9 << 8
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_entry_points_check_every_offset_before_a_launch():
    """(the pointers below are never dereferenced)"""
    lib, P = _lib.lib(), 4096
    err = lambda: lib.mcamd_last_error().decode()
    big = 1 << 20
    pack = lambda s, shifts=P, cap=big: lib.mcamd_wz_pack_w4((_lib.WzSeg * 1)(s), P, 1, P, big, P, P, big, P, big, P, big, None, shifts, cap)
    unpack = lambda s, shifts=P, cap=big, exps=big: lib.mcamd_wz_unpack_w4((_lib.WzSeg * 1)(s), P, 1, P, big, P, exps, P, big, P, big,
                                                                          None, shifts, cap)
    assert pack(seg(kind=_lib.WZ_W4 | 7 << 8)) == -1 and "needs cin % 32 == 0" in err()          # 576 weights per filter, 7 taps
    assert pack(seg(kind=_lib.WZ_W4)) == -1 and "needs cin % 32 == 0" in err()                   # no taps
    assert pack(seg(n=5 * 48 * 9)) == -1 and "needs cin % 32 == 0" in err()
    assert pack(seg(shift0=1)) == -1 and "shift0 1 is not the running sum 0" in err()
    assert pack(seg(), cap=88) == -1 and "96 shift bytes needed, room for 88" in err()           # 90 shift bytes, padded to 8
    assert pack(seg(), shifts=None) == -1 and "shift bytes needed" in err()
    assert unpack(seg(dense=1), cap=89) == -1 and "shift bytes [0, +90) outside the 89 given" in err()
    assert unpack(seg(dense=1, shift0=2), cap=105) == -1 and "shift bytes [16, +90) outside the 105 given" in err()
    assert unpack(seg(dense=1, shift0=-1)) == -1 and "shift bytes [-8, +90)" in err()
    assert unpack(seg(dense=1), shifts=None) == -1 and "outside the 0 given" in err()
    assert unpack(seg(dense=1), exps=4) == -1 and "exponents [0, +5) outside the 4 given" in err()
    assert unpack(seg(dense=1, val0=big - 2872)) == -1 and "values [" in err()                    # one byte per code: 2880
    # the entry points without shift bytes refuse the kind and keep their messages
    arr = (_lib.WzSeg * 1)(seg())
    assert lib.mcamd_wz_pack(arr, P, 1, P, big, P, P, big, P, big, P, big, None) == -1 and "goes through wz_pack_w4" in err()
    assert lib.mcamd_wz_unpack(arr, P, 1, P, big, P, big, P, big, P, big, None) == -1 and "goes through wz_unpack_w4" in err()
