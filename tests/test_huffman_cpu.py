"""Huffman-coded model files ("MCZH") without a device: the length-limited code, the streams and whole files of
the CPU path of compress.py against the numpy restatement (hz_ref.py), transcoding, loading, the parser's refusals and the
C surface."""
import ctypes as C
import heapq
import os
import re
import struct

import numpy as np
import pytest
import torch

from modelcompression_amd import _lib, compress, nets, ops, share
from modelcompression_amd._lib import McamdError
from modelcompression_amd.synthetic import init_synthetic
import hz_ref
import wz_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "golden", "mini.cfg")
NAMES = ("mcamd_hz_workspace_bytes", "mcamd_hz_histogram", "mcamd_hz_encode", "mcamd_hz_decode")
FIB = [1, 1]
while len(FIB) < 30:
    FIB.append(FIB[-1] + FIB[-2])


# ----------------------------------------------------------------------------- huffman_lengths
def unlimited(counts):
    """(cost in bits, depth) of an unlimited Huffman code of the non-zero counts, by heapq."""
    heap = [(c, i, 0) for i, c in enumerate(counts) if c > 0]
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost, tick = 0, len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
        tick += 1
    return cost, heap[0][2]


def histograms():
    rng = np.random.default_rng(11)
    out = []
    for A in (2, 12, 16, 256):
        out.append(("zero-%d" % A, [0] * A))
        out.append(("one-%d" % A, [0] * (A - 1) + [7]))
        out.append(("two-%d" % A, [3] + [0] * (A - 2) + [1000]))
        out.append(("uniform-%d" % A, [5] * A))
        out.append(("random-%d" % A, [int(c) for c in rng.integers(0, 1000, A)]))
        out.append(("skewed-%d" % A, [int(c) for c in (rng.geometric(0.2, A) ** 3) * (rng.random(A) > 0.3)]))
    out.append(("fibonacci", FIB + [0] * 226))
    return out


@pytest.mark.parametrize("name, counts", histograms(), ids=[n for n, _ in histograms()])
def test_huffman_lengths(name, counts):
    lengths = compress.huffman_lengths(counts)
    assert lengths.dtype == np.uint8 and lengths.size == len(counts)
    used = [c for c in counts if c > 0]
    for c, l in zip(counts, lengths):
        assert (l == 0) if c == 0 else (1 <= l <= 12)
    kraft = sum(1 << (12 - int(l)) for l in lengths if l)
    assert kraft == (0 if not used else 1 << 11 if len(used) == 1 else 1 << 12)
    cost = sum(c * int(l) for c, l in zip(counts, lengths))
    if used:
        best, depth = unlimited(counts)
        if depth <= 12:
            assert cost == best
        if name == "fibonacci":
            assert depth == 29                                   # the limit binds
            assert best < cost <= 5 * sum(counts)                # ceil(log2 30) bits a symbol
    assert np.array_equal(compress.huffman_lengths(counts), lengths)
    assert np.array_equal(compress.huffman_lengths(np.array(counts, dtype=np.uint64)), lengths)


def test_huffman_lengths_refuses():
    with pytest.raises(McamdError, match="negative"):
        compress.huffman_lengths([1, -1])
    with pytest.raises(McamdError, match="do not fit"):
        compress.huffman_lengths([1] * 5, limit=2)


# ----------------------------------------------------------------------------- streams
def skewed(nsym, A, seed=0):
    return np.minimum(np.random.default_rng(seed).geometric(0.35, nsym) - 1, A - 1).astype(np.uint8)


@pytest.mark.parametrize("A", [2, 16, 256])
@pytest.mark.parametrize("nsym", [0, 1, 2, 1023, 1024, 1025, 3 * 1024 + 7])
def test_streams_match_the_restatement(nsym, A):
    sy = skewed(nsym, A, seed=nsym + A)
    width = {2: 1, 16: 4, 256: 8}[A]
    stored = compress._pack_codes(sy, width)
    got = compress._hz_stream_bytes(sy, A, stored)
    assert got == hz_ref.stream_bytes(sy, A, stored.tobytes())
    back, raw, pos = hz_ref.read_stream(got, 0, A, nsym, stored.nbytes)
    assert pos == len(got)
    assert np.array_equal(back, sy) if back is not None else bytes(raw) == stored.tobytes()
    mode = struct.unpack_from("<I", got, 0)[0]
    if mode == 1:                                            # the project's own reader, through a parsed stream
        nbits = struct.unpack_from("<Q", got, 16)[0]
        nchunks, nwords = -(-nsym // 1024), -(-nbits // 64)
        st = dict(nsym=nsym, nbits=nbits, nchunks=nchunks, nwords=nwords, lengths=np.frombuffer(got, "u1", A, 24),
                  chunk_bit0=np.frombuffer(got, "<u4", nchunks, 24 + hz_ref.up8(A)), bits0=24 + hz_ref.up8(A) + hz_ref.up8(4 * nchunks))
        assert np.array_equal(compress._hz_decode_stream(got, st, "stream"), sy)
    assert len(got) <= 16 + hz_ref.up8(stored.nbytes)


def test_mode_rule_from_both_sides():
    uniform = np.arange(1 << 14, dtype=np.uint8)             # every byte value equally often: 8 bits a symbol, no gain
    got = compress._hz_stream_bytes(uniform, 256, uniform)
    assert struct.unpack_from("<I", got, 0)[0] == 0 and got[16:] == uniform.tobytes()
    sy = skewed(1 << 14, 256)
    got = compress._hz_stream_bytes(sy, 256, sy)
    assert struct.unpack_from("<I", got, 0)[0] == 1 and len(got) < sy.size // 2
    one = np.full(5000, 9, dtype=np.uint8)                   # a single symbol: length 1, code 0
    got = compress._hz_stream_bytes(one, 16, compress._pack_codes(one, 4))
    assert struct.unpack_from("<IIQQ", got, 0) == (1, 16, 5000, 5000)
    assert list(got[24:40]) == [0] * 9 + [1] + [0] * 6 and not any(got[40 + 24:])
    # exactly at the break-even the stream stays raw: strictly smaller only
    lengths = compress.huffman_lengths(np.bincount(sy, minlength=256))
    nbits = int((np.bincount(sy, minlength=256) * lengths).sum())
    body = 8 + 256 + hz_ref.up8(4 * 16) + 8 * -(-nbits // 64)
    assert compress._hz_plan(np.bincount(sy, minlength=256), 256, body)[0] == 0
    assert compress._hz_plan(np.bincount(sy, minlength=256), 256, body + 8)[0] == 1


# ----------------------------------------------------------------------------- files
def layers_of(model):
    return list(range(2, len(wz_ref.model_layers(model))))


def make(masks="dense", seed=3, seen=12345, bits=None):
    model = init_synthetic(nets.Darknet(MINI), seed=seed)
    model.seen = seen
    convs = [conv for conv, _ in wz_ref.model_layers(model)]
    g = torch.Generator().manual_seed(seed + 1)
    if masks == "pruned":                    # what weight_prune(80) leaves: the largest fifth of every layer; conv5 loses all
        ms = []
        for i, conv in enumerate(convs):
            a = conv.weight.data.abs()
            ms.append((a > a.flatten().kthvalue(int(0.8 * a.numel())).values).float() if i != 4 else torch.zeros_like(a))
        model.set_masks(ms)
    elif masks == "2:4":                     # what nm_prune(2, 4) leaves: the two largest of every four input channels
        ms = []
        for conv in convs:
            w = conv.weight.data
            if w.shape[1] % 4:
                ms.append(torch.ones_like(w))
                continue
            a = w.abs().permute(0, 2, 3, 1).reshape(-1, 4)
            m = torch.zeros_like(a).scatter_(1, a.topk(2, dim=1).indices, 1.0)
            ms.append(m.view(w.shape[0], w.shape[2], w.shape[3], w.shape[1]).permute(0, 3, 1, 2).contiguous())
        model.set_masks(ms)
    if bits is not None:
        model.set_codebooks(share.kmeans_share(model, bits=bits, iters=1))
    return model


CASES = [("fp32", None), ("fp16", None), ("fp8", None), ("w4", None), ("shared", 2), ("shared", 4), ("shared", 8)]
_FILES = {}


def files(tmp_path_factory, payload, bits, masks):
    """(model, layers, path of the "MCZW" file, path of the "MCZH" file), written once per case."""
    key = (payload, bits, masks)
    if key not in _FILES:
        d = tmp_path_factory.mktemp("hz")
        model = make(masks, bits=bits)
        layers = layers_of(model) if payload in ("fp8", "w4") else None
        plain, coded = str(d / "plain.mcz"), str(d / "coded.mcz")
        compress.save_compressed(model, plain, payload, layers)
        model.save_compressed(coded, payload, layers, entropy="huffman")
        _FILES[key] = (model, layers, plain, coded)
    return _FILES[key]


def state(model):
    out = {k: v.clone() for k, v in model.state_dict().items()}
    for i, (conv, _) in enumerate(wz_ref.model_layers(model)):
        out["mask_flag%d" % i] = torch.tensor(float(conv.mask_flag))
        if getattr(conv, "share_flag", False):
            out["codebook%d" % i], out["codes%d" % i] = conv.codebook.clone(), conv.codes.clone().float()
    out["seen"] = torch.tensor(float(model.seen))
    return out


def same_state(a, b):
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and torch.equal(a[k].float().contiguous().view(torch.int32),
                                                                               b[k].float().contiguous().view(torch.int32)) for k in a)


@pytest.mark.parametrize("masks", ["dense", "pruned", "2:4"])
@pytest.mark.parametrize("payload, bits", CASES)
def test_files(tmp_path_factory, tmp_path, payload, bits, masks):
    model, layers, plain_path, coded_path = files(tmp_path_factory, payload, bits, masks)
    plain, coded = open(plain_path, "rb").read(), open(coded_path, "rb").read()
    assert coded[:4] == b"MCZH" and plain[:4] == b"MCZW" and coded[4:24] == plain[4:24]
    # the CPU path writes the restatement's bytes, and the restatement reads them back to the "MCZW" twin
    assert coded == hz_ref.encode_file(plain)
    assert hz_ref.decode_file(coded) == plain
    # transcoding: to the plain twin, back to the coded file, and each onto itself
    a, b = str(tmp_path / "a.mcz"), str(tmp_path / "b.mcz")
    compress.transcode(coded_path, a, None)
    assert open(a, "rb").read() == plain
    compress.transcode(a, b, "huffman")
    assert open(b, "rb").read() == coded
    compress.transcode(b, b, "huffman")
    assert open(b, "rb").read() == coded
    compress.transcode(plain_path, a, None)
    assert open(a, "rb").read() == plain
    # size: never more than 16 bytes a stream above the twin; smaller on the pruned model
    nstreams = hz_ref.count_streams(plain)
    assert len(coded) <= len(plain) + 16 * nstreams
    assert nstreams > 0 or (masks == "dense" and payload in ("fp32", "fp16"))       # (dense fp32 / fp16: nothing to code)
    if masks == "pruned":
        assert len(coded) < len(plain)
    # loading either file gives the same model, bit for bit
    one, two = nets.Darknet(MINI), nets.Darknet(MINI)
    assert one.load_weights(coded_path) is None and two.load_weights(plain_path) is None
    assert same_state(state(one), state(two)) and one.seen == 12345
    assert compress.is_compressed(coded_path) and compress.is_compressed(plain_path)
    # compressed_info: the twin's is what it was, the coded file's adds the streams
    info, twin = compress.compressed_info(coded_path), compress.compressed_info(plain_path)
    assert sorted(twin) == ["bytes", "dense_bytes", "kept", "layers", "payload", "ratio", "seen", "weights"]
    assert all("streams" not in l for l in twin["layers"])
    assert info["entropy"] == "huffman" and info["plain_bytes"] == len(plain) == twin["bytes"] and info["bytes"] == len(coded)
    assert sum(len(l["streams"]) for l in info["layers"]) == nstreams
    for l, t in zip(info["layers"], twin["layers"]):
        assert {k: v for k, v in l.items() if k not in ("bytes", "streams")} == {k: v for k, v in t.items() if k != "bytes"}
        assert l["bytes"] - sum(s["bytes"] - s["raw_bytes"] for s in l["streams"]) == t["bytes"]
        for s in l["streams"]:
            assert s["mode"] in (0, 1) and s["name"] in ("group shifts", "bit words", "values", "codes")
            assert (s["bytes"] < s["raw_bytes"] + 16) if s["mode"] == 1 else (s["bytes"] == s["raw_bytes"] + 16)
    for k in twin:
        if k not in ("bytes", "ratio", "layers"):
            assert info[k] == twin[k]


def test_entropy_none_is_the_plain_file_and_other_values_are_named(tmp_path):
    model = make("pruned")
    a, b = str(tmp_path / "a.mcz"), str(tmp_path / "b.mcz")
    model.save_compressed(a, "fp16")
    model.save_compressed(b, "fp16", None, None)
    assert open(a, "rb").read() == open(b, "rb").read() == wz_ref.model_file(model, "fp16")
    for call in (lambda: model.save_compressed(b, "fp16", entropy="lz"), lambda: compress.transcode(a, b, "arithmetic")):
        with pytest.raises(McamdError, match="entropy must be None or \"huffman\""):
            call()
    assert compress.VERSION == 1 and compress.MAGIC == b"MCZW" and compress.HZ_MAGIC == b"MCZH"


def test_pruned_model_has_a_layer_without_a_kept_weight(tmp_path_factory):
    _, _, _, coded = files(tmp_path_factory, "fp8", None, "pruned")
    info = compress.compressed_info(coded)
    assert info["layers"][4]["kept"] == 0
    assert [s["nsym"] for s in info["layers"][4]["streams"] if s["name"] == "values"] == [0]
    assert any(s["mode"] == 1 for l in info["layers"] for s in l["streams"])


# ----------------------------------------------------------------------------- refusals
def coded_fp8(tmp_path):
    """An fp8 coded file of the pruned model whose LAST stream is Huffman-coded, parsed: (path, bytes, records)."""
    model = make("pruned")
    path = str(tmp_path / "m.mcz")
    model.save_compressed(path, "fp8", list(range(2, 8)), entropy="huffman")
    return path, bytearray(open(path, "rb").read()), compress._parse(path)["records"]


def refused(tmp_path, data, text, layer):
    bad = str(tmp_path / "bad.mcz")
    open(bad, "wb").write(bytes(data))
    target = make(seed=11, seen=7)
    before = state(target)
    with pytest.raises(McamdError, match=text) as e:
        target.load_weights(bad)
    assert "conv%d" % layer in str(e.value) and bad in str(e.value)
    assert same_state(before, state(target)) and target.seen == 7
    assert not any(conv.mask_flag for conv, _ in wz_ref.model_layers(target))


def patched(data, off, fmt, value):
    out = bytearray(data)
    struct.pack_into(fmt, out, off, value)
    return out


def test_the_parser_refuses_damaged_streams(tmp_path):
    path, data, recs = coded_fp8(tmp_path)
    # conv2's values: a Huffman stream of more than one chunk
    st = next(s for s in recs[1]["streams"] if s["name"] == "values")
    assert st["mode"] == 1 and st["nchunks"] > 1
    head = st["len0"] - 24
    assert struct.unpack_from("<IIQQ", data, head) == (1, 256, st["nsym"], st["nbits"])
    refused(tmp_path, patched(data, head, "<I", 2), "stream mode 2", 2)
    refused(tmp_path, patched(data, head + 4, "<I", 255), "alphabet of 255 where the record implies", 2)
    refused(tmp_path, patched(data, head + 8, "<Q", st["nsym"] - 1), "where the record implies %d over 256" % st["nsym"], 2)
    used = int(np.flatnonzero(st["lengths"])[0])
    refused(tmp_path, patched(data, st["len0"] + used, "<B", 13), "a code length of 13", 2)
    shorter = int(np.flatnonzero((st["lengths"] > 1))[0])
    refused(tmp_path, patched(data, st["len0"] + shorter, "<B", int(st["lengths"][shorter]) - 1), "Kraft sum", 2)
    refused(tmp_path, patched(data, st["len0"] + shorter, "<B", 0), "Kraft sum", 2)
    refused(tmp_path, patched(data, st["chunk0"], "<I", 1), "chunk_bit0 does not start at 0", 2)
    refused(tmp_path, patched(data, st["chunk0"] + 4, "<I", 0xFFFFFFF0), "chunk_bit0", 2)
    assert st["nchunks"] > 2
    refused(tmp_path, patched(data, st["chunk0"] + 4, "<I", int(st["chunk_bit0"][2]) + 1), "decreases", 2)
    # well-formed tables around damaged bits: a chunk no longer ends where the next one begins
    # (a prefix code can fall back into step after a flipped bit: the flip taken is one the restatement's reader rejects)
    for p in range(int(st["chunk_bit0"][1]) - 1, int(st["chunk_bit0"][1]) - 200, -1):
        flipped = patched(data, st["bits0"] + p // 8, "<B", data[st["bits0"] + p // 8] ^ (1 << p % 8))
        try:
            hz_ref.read_stream(bytes(flipped), head, 256, st["nsym"], st["nsym"])
        except AssertionError:
            break
    else:
        raise AssertionError("no flipped bit breaks the chunk")
    refused(tmp_path, flipped, "coded stream is damaged", 2)
    refused(tmp_path, patched(data, st["chunk0"] + 4, "<I", int(st["chunk_bit0"][1]) + 1), "coded stream is damaged", 2)
    # the last stream of the file: more code bits than words are present
    last = recs[-1]["streams"][-1]
    assert last["mode"] == 1 and last["bits0"] + 8 * last["nwords"] == len(data)
    refused(tmp_path, patched(data, last["len0"] - 8, "<Q", last["nbits"] + 64), "beyond the words present", 7)
    refused(tmp_path, patched(data, last["len0"] - 8, "<Q", 13 * last["nsym"]), "code bits for %d symbols" % last["nsym"], 7)
    # shortened: the last chunk cannot end at nbits (or the chunk table passes it)
    refused(tmp_path, patched(data, last["len0"] - 8, "<Q", last["nbits"] - 1), "damaged|chunk_bit0|behind the last record", 7)
    refused(tmp_path, data[:-8], "truncated", 7)
    refused(tmp_path, data[:st["bits0"] + 16], "truncated", 2)
    bad = str(tmp_path / "long.mcz")
    open(bad, "wb").write(bytes(data) + b"\0" * 8)
    for call in (lambda: make().load_weights(bad), lambda: compress.compressed_info(bad)):
        with pytest.raises(McamdError, match="behind the last record"):
            call()
    open(bad, "wb").write(bytes(data[:4]) + struct.pack("<I", 2) + bytes(data[8:]))
    with pytest.raises(McamdError, match="version 2"):
        compress.compressed_info(bad)
    open(bad, "wb").write(bytes(data[:40]))
    with pytest.raises(McamdError, match="truncated"):
        compress.compressed_info(bad)


def test_bit_words_that_do_not_select_the_kept_values_are_refused(tmp_path):
    path, data, recs = coded_fp8(tmp_path)
    plain = bytearray(hz_ref.decode_file(bytes(data)))
    twin = str(tmp_path / "twin.mcz")
    open(twin, "wb").write(bytes(plain))
    word0 = compress._parse(twin)["records"][2]["word0"]
    plain[word0] ^= 0x01                                     # one weight more or less than `kept`
    refused(tmp_path, hz_ref.encode_file(bytes(plain)), "conv3: the bit words do not select", 3)


# ----------------------------------------------------------------------------- the C surface
def test_symbols_are_declared_exported_bound_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    assert '"MCZH"' in hdr and "chunk_bit0" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.lib()
    for name in NAMES:
        assert re.search(r"\b(int|size_t) %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name, value in (("MCAMD_HZ_MAXLEN", _lib.HZ_MAXLEN), ("MCAMD_HZ_CHUNK", _lib.HZ_CHUNK), ("MCAMD_HZ_GROUP", _lib.HZ_GROUP)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
    body = re.search(r"typedef struct mcamd_hz_seg \{(.*?)\} mcamd_hz_seg;", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.HzSeg._fields_] and C.sizeof(_lib.HzSeg) == 56
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [ctype[t] for t in re.findall(r"(\w+)\s+\w+;", body)] == [f[1] for f in _lib.HzSeg._fields_]
    assert C.sizeof(_lib.WzSeg) == 72
    assert '"huff.hip"' in open(os.path.join(ROOT, "modelcompression_amd", "build.py")).read()
    for f in (ops.hz_histogram, ops.hz_encode, ops.hz_decode, compress.transcode, compress.huffman_lengths):
        assert callable(f)
    from modelcompression_amd.train import YOLOv2Train
    assert YOLOv2Train.SAVE_COMPRESSED_ENTROPY is None


def seg(**kw):
    s = _lib.HzSeg()
    s.sym0, s.nsym, s.nbits, s.word0, s.chunk0, s.popc_bits, s.block0, s.A = 0, 3000, 9000, 0, 0, 0, 0, 256
    for k, v in kw.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("bad, hist_text, code_text", [
    (dict(nsym=-1), "bad stream", "bad stream"),
    (dict(A=0), "bad stream", "bad stream"),
    (dict(A=257), "bad stream", "bad stream"),
    (dict(block0=1), "block0 1 is not the running sum 0", "block0 1 is not the running sum 0"),
    (dict(sym0=4), "symbols [4, +3000) outside", "symbols [4, +3000) outside"),
    (dict(sym0=-8), "symbols [-8, +3000) outside", "symbols [-8, +3000) outside"),
    (dict(sym0=8), "symbols [8, +3000) outside the 3000 bytes given", "symbols [8, +3000) outside the 3000 bytes given"),
    (dict(nbits=1 << 32), None, "nbits 4294967296"),
    (dict(nbits=36001), None, "nbits 36001 for 3000 symbols"),
    (dict(word0=1), None, "code words [1, +141) outside the 141 given"),
    (dict(word0=-1), None, "code words [-1, +141) outside the 141 given"),
])
def test_entry_points_refuse_bad_tables(bad, hist_text, code_text):
    """Every argument error is refused before a launch (the pointers below are never dereferenced)."""
    lib, P = _lib.lib(), 4096
    arr = (_lib.HzSeg * 1)(seg(**bad))
    err = lambda: lib.mcamd_last_error().decode()
    if hist_text:
        assert lib.mcamd_hz_histogram(arr, P, 1, P, 3000, None, P, P, 1 << 20, None) == -1
        assert hist_text in err() and err().startswith("hz_histogram:"), err()
    assert lib.mcamd_hz_encode(arr, P, 1, P, 3000, P, P, 3, P, 141, P, 1 << 20, None) == -1
    assert code_text in err() and err().startswith("hz_encode:"), err()
    assert lib.mcamd_hz_decode(arr, P, 1, P, P, 3, P, 141, P, 3000, P, None) == -1
    assert code_text in err() and err().startswith("hz_decode:"), err()


def test_entry_points_refuse_short_buffers():
    lib, P = _lib.lib(), 4096
    err = lambda: lib.mcamd_last_error().decode()
    arr = (_lib.HzSeg * 1)(seg())
    assert lib.mcamd_hz_histogram(None, P, 1, P, 3000, None, P, P, 1 << 20, None) == -1 and "null argument" in err()
    assert lib.mcamd_hz_histogram(arr, P, 1, P, 3000, None, P, P, 8, None) != 0 and "workspace too small" in err()
    assert lib.mcamd_hz_workspace_bytes(1, 1) >= 1024 + 512
    assert lib.mcamd_hz_encode(arr, P, 1, P, 3000, P, P, 2, P, 141, P, 1 << 20, None) == -1 and "chunk_bit0 [0, +3) outside the 2 given" in err()
    assert lib.mcamd_hz_encode(arr, P, 1, P, 3000, P, P, 3, P, 140, P, 1 << 20, None) == -1 and "outside the 140 given" in err()
    assert lib.mcamd_hz_encode(arr, P, 1, P, 3000, P, P, 3, P, 141, P, 8, None) != 0 and "workspace too small" in err()
    two = (_lib.HzSeg * 2)(seg(), seg(block0=1, chunk0=2, word0=141, sym0=3000))
    assert lib.mcamd_hz_encode(two, P, 2, P, 6000, P, P, 6, P, 282, P, 1 << 20, None) == -1 and "chunk0 2 is not the running sum 3" in err()
    assert lib.mcamd_hz_decode(arr, P, 1, P, P, 2, P, 141, P, 3000, P, None) == -1 and "chunk_bit0 [0, +3) outside the 2 given" in err()
    assert lib.mcamd_hz_decode(arr, P, 1, P, P, 3, P, 141, P, 2999, P, None) == -1 and "outside the 2999 bytes given" in err()
    arr = (_lib.HzSeg * 1)(seg(popc_bits=24001))
    assert lib.mcamd_hz_decode(arr, P, 1, P, P, 3, P, 141, P, 3000, P, None) == -1 and "popc_bits 24001" in err()
    arr = (_lib.HzSeg * 1)(seg(nsym=3001, popc_bits=5))
    assert lib.mcamd_hz_decode(arr, P, 1, P, P, 3, P, 141, P, 3008, P, None) == -1 and "popc_bits 5 with 3001 symbols" in err()


def test_refused_while_a_plan_records():
    lib, P = _lib.lib(), 4096
    streams = (C.c_void_p * 1)(None)
    assert lib.mcamd_plan_begin(streams, 1) == 0
    try:
        arr = (_lib.HzSeg * 1)(seg())
        assert lib.mcamd_hz_histogram(arr, P, 1, P, 3000, None, P, P, 1 << 20, None) == -1
        assert "hz_histogram: not recordable" in lib.mcamd_last_error().decode()
        assert lib.mcamd_hz_encode(arr, P, 1, P, 3000, P, P, 3, P, 141, P, 1 << 20, None) == -1
        assert "hz_encode: not recordable" in lib.mcamd_last_error().decode()
        assert lib.mcamd_hz_decode(arr, P, 1, P, P, 3, P, 141, P, 3000, P, None) == -1
        assert "hz_decode: not recordable" in lib.mcamd_last_error().decode()
    finally:
        plan = lib.mcamd_plan_end()
        assert plan and lib.mcamd_plan_launches(plan) == 0
        lib.mcamd_plan_destroy(plan)


def test_wrappers_have_no_cpu_path():
    sy = torch.zeros(100, dtype=torch.uint8)
    with pytest.raises(McamdError):
        ops.hz_histogram([sy])
    with pytest.raises(McamdError):
        ops.hz_encode([sy], [np.ones(256, dtype=np.uint8)])
    with pytest.raises(McamdError):
        ops.hz_decode([dict(nsym=100, A=256, nbits=100, lengths=np.ones(256, dtype=np.uint8),
                            chunk_bit0=torch.zeros(1, dtype=torch.int32), bits=torch.zeros(2, dtype=torch.int64))])
