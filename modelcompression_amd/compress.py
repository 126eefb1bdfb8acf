"""Compressed model files (.mcz; an addition beyond the reference, DESIGN.md 3s, include/mcamd.h).

A Darknet .weights file stores every conv weight as a dense float32, zeros included.  An .mcz file stores, per conv block,
a bitmask of the non-zero weights and only those weights, as fp32, fp16 or e4m3 codes -- exactly what the engine the file
is written for consumes, so the file is lossless for that engine:

    save_compressed(model, path, payload="fp16", layers=None)       # payload "shared": codebooks + narrow codes (below)
                                                                    # payload "w4": what the "fp8-w4" engine consumes (below)
    load_compressed(model, path, set_masks=True) -> masks
    compressed_info(path) -> dict

Payload "shared"  stores every layer Darknet.set_codebooks tied as the bitmask of its MASK, its fp32 codebook
and one code of 1, 2, 4 or 8 bits per kept weight, and every other layer as fp32; reading it gives back the tied model's
fp32 weights exactly, with its masks and codebooks.

Payload "w4"  stores the layers the "fp8-w4" engine runs in its 4-bit format as that format: one exponent per
filter, one shift byte per group of 32 input channels at one tap and one 4-bit code per weight -- the codes, shifts and exponents
of mcamd_pack_q8_w4, in OIHW order -- and every other layer as fp16.  Reading it gives fp32 masters grid[code] 2^g 2^-e4_f, which
the engine's packer turns back into the same expanded e4m3 bytes: the file is lossless for that engine.

A model on the GPU is packed and expanded by the device passes of csrc/wpack.hip (ops.wz_pack / ops.wz_unpack: all layers
through one segment table); a model on the CPU takes the torch / numpy path below, which writes and reads the same bytes.

entropy="huffman"  writes the same records in a container of its own, magic "MCZH": every uint8-symbol array (bit
words, shift bytes, e4m3 bytes, codes) is a stream of canonical length-limited Huffman codes, or raw where that is not smaller:

    save_compressed(model, path, payload, layers, entropy="huffman")
    transcode(src, dst, entropy)            # either container as either, on the host
    huffman_lengths(counts, limit=12)       # THE source of the code lengths; the file stores them

load_compressed, is_compressed and compressed_info read either container.  A model on the GPU is coded and decoded by the passes
of csrc/huff.hip (ops.hz_histogram_at / hz_encode_at / hz_decode_at); the numpy path writes the same bytes.
"""
import os
import struct

import numpy as np
import torch

from . import _lib as L
from ._lib import McamdError

MAGIC = b"MCZW"
VERSION = 1
PAYLOADS = {"fp32": L.WZ_FP32, "fp16": L.WZ_FP16, "fp8": L.WZ_FP8, "shared": L.WZ_CODE, "w4": L.WZ_W4}
KIND_NAMES = {v: k for k, v in PAYLOADS.items()}
# (WZ_CODE, WZ_W4: one byte per code in the device passes; `width` / 4 bits in the file)
ELEM = {L.WZ_FP32: 4, L.WZ_FP16: 2, L.WZ_FP8: 1, L.WZ_CODE: 1, L.WZ_W4: 1}
_CODE_DTYPE = {L.WZ_FP32: "<u4", L.WZ_FP16: "<u2", L.WZ_FP8: "u1", L.WZ_CODE: "u1", L.WZ_W4: "u1"}
_MAG_BITS = {L.WZ_FP32: 0x7FFFFFFF, L.WZ_FP16: 0x7FFF, L.WZ_FP8: 0x7F, L.WZ_W4: 0x7}
_W4_GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float64)
_W4_SHIFT_MAX = 11                           # shift bytes are g + 5, g in [-5, 6]
_HEADER = struct.Struct("<4sIIIq")          # magic, version, payload, records, seen
_RECORD = struct.Struct("<4iIIQ")           # cout, cin, kh, kw, flags, bits (WZ_CODE; 0 otherwise), kept
# the Huffman-coded container (include/mcamd.h): the same header and records, every uint8-symbol array a stream
HZ_MAGIC = b"MCZH"
HZ_VERSION = 1
ENTROPIES = (None, "huffman")
HZ_MAXLEN, HZ_CHUNK = L.HZ_MAXLEN, L.HZ_CHUNK
_STREAM = struct.Struct("<IIQ")             # mode (0 raw, 1 Huffman), alphabet, symbols


def _pad8(nbytes):
    return (nbytes + 7) // 8 * 8


def has_bits(n, kept, kind):
    """The bitmask-or-dense rule: a record carries bit words only when that is smaller.  A record of codes carries them
    whenever a weight is not kept: a code cannot say so.  A 4-bit record counts its nibbles."""
    if kind == L.WZ_CODE:
        return kept < n
    if kind == L.WZ_W4:
        return 8 * ((n + 63) // 64) + (kept + 1) // 2 < (n + 1) // 2
    return 8 * ((n + 63) // 64) + kept * ELEM[kind] < n * ELEM[kind]


def code_width(bits):
    """Bits per stored code: the smallest of 1, 2, 4, 8 that holds `bits`."""
    return next(w for w in (1, 2, 4, 8) if w >= bits)


def _pack_codes(codes, width):
    """uint8 codes -> bytes: code i in bits [width (i % per), +width) of byte i // per, per = 8 // width."""
    per = 8 // width
    if per == 1:
        return np.ascontiguousarray(codes, dtype=np.uint8)
    padded = np.zeros((codes.size + per - 1) // per * per, dtype=np.uint8)
    padded[:codes.size] = codes
    out = np.zeros(padded.size // per, dtype=np.uint8)
    for j in range(per):
        out |= (padded[j::per] << np.uint8(width * j)).astype(np.uint8)
    return out


def _unpack_codes(packed, width, count):
    per = 8 // width
    if per == 1:
        return np.ascontiguousarray(packed[:count], dtype=np.uint8)
    out = np.empty(packed.size * per, dtype=np.uint8)
    for j in range(per):
        out[j::per] = (packed >> np.uint8(width * j)) & np.uint8((1 << width) - 1)
    return out[:count]


def is_compressed(path):
    with open(path, "rb") as f:
        return f.read(4) in (MAGIC, HZ_MAGIC)


# ----------------------------------------------------------------------------- Huffman streams
def _check_entropy(entropy):
    if entropy not in ENTROPIES:
        raise McamdError("entropy must be None or \"huffman\" (got %r)" % (entropy,))


def huffman_lengths(counts, limit=HZ_MAXLEN):
    """Code lengths (uint8, one per symbol) of a length-limited Huffman code of the histogram `counts`, by package-merge: a
    symbol that does not occur gets 0, every other one 1..limit, and no prefix code with that limit costs fewer bits.  Two or
    more used symbols give a full code (Kraft sum 1); a single one gets length 1.  Deterministic: the leaves are ordered by
    (count, symbol) and at equal weight a leaf goes before a package.  THE one place the lengths of a coded file come from
    (the file stores them, so a reader never calls this)."""
    counts = [int(c) for c in counts]
    if min(counts, default=0) < 0:
        raise McamdError("huffman_lengths: a negative count")
    lengths = np.zeros(len(counts), dtype=np.uint8)
    leaves = sorted((c, (a,)) for a, c in enumerate(counts) if c > 0)
    if len(leaves) > 1 << limit:
        raise McamdError("huffman_lengths: %d symbols do not fit codes of %d bits" % (len(leaves), limit))
    if len(leaves) == 1:
        lengths[leaves[0][1][0]] = 1
    if len(leaves) < 2:
        return lengths
    merged = leaves
    for _ in range(limit - 1):
        packages = [(merged[i][0] + merged[i + 1][0], merged[i][1] + merged[i + 1][1]) for i in range(0, len(merged) - 1, 2)]
        merged = sorted(leaves + packages, key=lambda item: item[0])      # (stable)
    for _, symbols in merged[:2 * len(leaves) - 2]:
        for a in symbols:
            lengths[a] += 1
    return lengths


def _canonical_codes(lengths):
    """RFC 1951 3.2.2: the code values of the symbols with a non-zero length, increasing in (length, symbol) order."""
    lengths = np.asarray(lengths, dtype=np.int64)
    count = np.bincount(lengths, minlength=HZ_MAXLEN + 1)
    count[0] = 0
    code, nxt = 0, [0] * (HZ_MAXLEN + 1)
    for l in range(1, HZ_MAXLEN + 1):
        code = (code + int(count[l - 1])) << 1
        nxt[l] = code
    codes = np.zeros(lengths.size, dtype=np.int64)
    for a, l in enumerate(lengths):
        if l:
            codes[a] = nxt[l]
            nxt[l] += 1
    return codes


def _hz_plan(hist, A, raw_bytes):
    """(mode, lengths, nbits) of a stream from its histogram and the padded size of its array in an "MCZW" file: Huffman iff
    that body, padding included, is strictly smaller and nbits < 2^32."""
    nsym = int(hist.sum())
    if nsym == 0 or int(hist[A:].sum()):
        return 0, None, 0
    lengths = huffman_lengths(hist[:A])
    nbits = int(sum(int(c) * int(l) for c, l in zip(hist[:A], lengths)))
    body = 8 + _pad8(A) + _pad8(4 * ((nsym + HZ_CHUNK - 1) // HZ_CHUNK)) + 8 * ((nbits + 63) // 64)
    if body < raw_bytes and nbits < 1 << 32:
        return 1, lengths, nbits
    return 0, None, 0


def _hz_code_stream(symbols, lengths, nbits):
    """(chunk_bit0 <u4, bit words <u8) of the symbols under `lengths`, a million symbols at a time."""
    lens_of, codes_of = lengths.astype(np.int64), _canonical_codes(lengths)
    words = np.zeros((nbits + 63) // 64, dtype="<u8")
    chunk0 = np.zeros((symbols.size + HZ_CHUNK - 1) // HZ_CHUNK, dtype="<u4")
    base, step = 0, HZ_CHUNK << 10
    for b in range(0, symbols.size, step):
        sy = symbols[b:b + step]
        lens, codes = lens_of[sy], codes_of[sy]
        ends = np.cumsum(lens)
        first = base // 64
        starts = base - 64 * first + ends - lens              # relative to the first word this block touches
        chunk0[b // HZ_CHUNK:(b + sy.size + HZ_CHUNK - 1) // HZ_CHUNK] = (starts[::HZ_CHUNK] + 64 * first).astype("<u4")
        total = base - 64 * first + int(ends[-1])
        bit = np.zeros((total + 63) // 64 * 64, dtype=np.uint8)
        for j in range(int(lens.max())):                      # bit j of every code, most significant first
            m = lens > j
            bit[starts[m] + j] = (codes[m] >> (lens[m] - 1 - j)) & 1
        part = np.packbits(bit, bitorder="little").view("<u8")
        words[first:first + part.size] |= part
        base += int(ends[-1])
    if base != nbits:
        raise McamdError("a stream of %d code bits where its histogram gives %d" % (base, nbits))
    return chunk0, words


def _hz_pack(A, nsym, nbits, lengths, chunk0, words):
    """The bytes of a Huffman stream."""
    out = _STREAM.pack(1, A, nsym) + struct.pack("<Q", nbits)
    for a in (np.asarray(lengths[:A], dtype=np.uint8), np.asarray(chunk0, dtype="<u4"), np.asarray(words, dtype="<u8")):
        b = a.tobytes()
        out += b + b"\0" * (_pad8(len(b)) - len(b))
    return out


def _hz_raw(A, nsym, stored):
    b = stored.tobytes()
    return _STREAM.pack(0, A, nsym) + b + b"\0" * (_pad8(len(b)) - len(b))


def _hz_stream_bytes(symbols, A, stored):
    """A stream on the host: `symbols` (uint8) and `stored`, the array as an "MCZW" file stores them."""
    symbols = np.ascontiguousarray(symbols, dtype=np.uint8).reshape(-1)
    hist = np.bincount(symbols, minlength=256)
    mode, lengths, nbits = _hz_plan(hist, A, _pad8(stored.nbytes))
    if mode == 0:
        return _hz_raw(A, symbols.size, stored)
    chunk0, words = _hz_code_stream(symbols, lengths, nbits)
    return _hz_pack(A, symbols.size, nbits, lengths, chunk0, words)


def _hz_check_lengths(lengths, what):
    if int(lengths.max(initial=0)) > HZ_MAXLEN:
        raise McamdError("%s: a code length of %d (at most %d)" % (what, int(lengths.max()), HZ_MAXLEN))
    used = lengths[lengths != 0].astype(np.int64)
    kraft = int((1 << (HZ_MAXLEN - used)).sum())
    if kraft != (1 << HZ_MAXLEN - 1 if used.size == 1 else 1 << HZ_MAXLEN):
        raise McamdError("%s: the code lengths have a Kraft sum of %d / %d (a full prefix code has %d, a single symbol %d)"
                         % (what, kraft, 1 << HZ_MAXLEN, 1 << HZ_MAXLEN, 1 << HZ_MAXLEN - 1))


def _hz_decode_stream(raw, st, what):
    """The symbols (uint8) of a parsed Huffman stream, every chunk one step at a time through the 2^12 entry table.  A chunk
    that does not end exactly where the next begins (nbits for the last), or an unassigned code, is refused."""
    nsym, nbits, nchunks = st["nsym"], st["nbits"], st["nchunks"]
    lengths = st["lengths"].astype(np.int64)
    tab_sym, tab_len = np.zeros(1 << HZ_MAXLEN, dtype=np.uint8), np.zeros(1 << HZ_MAXLEN, dtype=np.int64)
    for a, (l, code) in enumerate(zip(lengths, _canonical_codes(lengths))):
        if l:                                                 # the code arrives bit-reversed at the low end of the window
            idx = int(format(int(code), "0%db" % l)[::-1], 2) + (np.arange(1 << (HZ_MAXLEN - l)) << l)
            tab_sym[idx], tab_len[idx] = a, l
    by = np.zeros(8 * st["nwords"] + 8, dtype=np.int64)
    by[:8 * st["nwords"]] = np.frombuffer(raw, "u1", 8 * st["nwords"], st["bits0"])
    pos = st["chunk_bit0"].astype(np.int64)
    end = np.append(pos[1:], nbits)
    count = np.minimum(HZ_CHUNK, nsym - HZ_CHUNK * np.arange(nchunks))
    out = np.zeros((nchunks, HZ_CHUNK), dtype=np.uint8)
    bad = np.zeros(nchunks, dtype=bool)
    for i in range(min(HZ_CHUNK, nsym)):
        act = (count > i) & ~bad
        k = pos >> 3
        window = ((by[k] | by[k + 1] << 8 | by[k + 2] << 16) >> (pos & 7)) & ((1 << HZ_MAXLEN) - 1)
        l = tab_len[window]
        ok = act & (l != 0) & (pos + l <= end)
        bad |= act & ~ok
        out[ok, i] = tab_sym[window[ok]]
        pos = pos + np.where(ok, l, 0)
    bad |= pos != end
    if bad.any():
        raise McamdError("%s: the coded stream is damaged (chunk %d does not end where the next one begins, or holds an "
                         "unassigned code)" % (what, int(np.flatnonzero(bad)[0])))
    return out.reshape(-1)[:nsym]


# ----------------------------------------------------------------------------- the model's conv blocks
def _conv_blocks(model):
    """[(conv number, MaskedConv2d, BatchNorm2d or None)] in save_weights order."""
    out = []
    for ind, block in enumerate(model.blocks[1:]):
        if block["type"] == "connected":
            raise McamdError("compressed model files store convolutional blocks only: a [connected] block is not supported")
        if block["type"] != "convolutional":
            continue
        seq = model.models[ind]
        conv, bn = seq[0], (seq[1] if int(block["batch_normalize"]) else None)
        if getattr(conv, "border_bias", None) is not None:
            raise McamdError("compressed model files do not store the border tables of slim_export models (conv%d has one): "
                             "save a slim model with save_weights" % (len(out) + 1))
        out.append((len(out) + 1, conv, bn))
    return out


def default_fp8_layers(model):
    """The conv numbers stored as e4m3 when `layers` is not given: BatchNorm blocks other than the first and the last conv
    whose input channel count is a multiple of 64 (conv3-conv22 of YOLOv2-VOC; Engine.fp8_layers is exact for any cfg)."""
    convs = _conv_blocks(model)
    return [i for i, conv, bn in convs if bn is not None and 1 < i < len(convs) and conv.weight.shape[1] % 64 == 0]


def _small_arrays(conv, bn):
    ts = [bn.bias.data, bn.weight.data, bn.running_mean, bn.running_var] if bn is not None else [conv.bias.data]
    return [t.detach().cpu().numpy().astype("<f4", copy=False) for t in ts]


def _small_targets(conv, bn):
    return [bn.bias.data, bn.weight.data, bn.running_mean, bn.running_var] if bn is not None else [conv.bias.data]


# ----------------------------------------------------------------------------- one layer on the CPU
def _codes_cpu(w, mask, kind):
    """(codes as a flat numpy array of the kind's width, exponents int32 numpy [cout] or None) of weight * mask."""
    wm = w.detach().float() * mask.float() if mask is not None else w.detach().float() * 1.0
    if kind == L.WZ_FP32:
        return wm.contiguous().view(torch.int32).numpy().reshape(-1).view("<u4"), None
    if kind == L.WZ_FP16:
        return wm.half().contiguous().view(torch.int16).numpy().reshape(-1).view("<u2"), None
    a = wm.abs().flatten(1).amax(1)
    m, x = torch.frexp(a)
    e = torch.where(m <= 0.875, 9 - x, 8 - x)
    e = torch.where(a == 0, torch.zeros_like(e), e).to(torch.int32)
    scaled = (wm.double() * torch.pow(2.0, e.double()).view(-1, 1, 1, 1)).float().clamp(-448.0, 448.0)
    return scaled.to(torch.float8_e4m3fn).contiguous().view(torch.uint8).numpy().reshape(-1), e.numpy().astype("<i4")


def _codes_w4_cpu(w, mask):
    """(codes uint8 flat OIHW, e4 int32 [cout], shift bytes uint8 flat [cout][cin / 32][kh][kw]) of weight * mask: the steps of
    mcamd_pack_q8_w4 (csrc/w4_quant.h) on exact float64 values."""
    wm = w.detach().float() * mask.float() if mask is not None else w.detach().float() * 1.0
    cout, cin, kh, kw = wm.shape
    a = wm.abs().flatten(1).amax(1)
    m, x = torch.frexp(a)
    e = torch.where(m <= 0.875, 9 - x, 8 - x) - 1
    e = torch.where(a == 0, torch.zeros_like(e), e).to(torch.int32)
    s = wm.double() * torch.pow(2.0, e.double()).view(-1, 1, 1, 1)
    amax = s.abs().view(cout, cin // 32, 32, kh, kw).amax(2)
    gm, gx = torch.frexp(amax)
    g = torch.where(gm <= 0.75, gx - 3, gx - 2).clamp(-5, 6)
    g = torch.where(amax == 0, torch.full_like(g, -5), g)
    step = torch.pow(2.0, g.double()).unsqueeze(2).expand(cout, cin // 32, 32, kh, kw).reshape(cout, cin, kh, kw)
    v = (s.abs() / step).clamp(max=6.0)
    # round to nearest onto the grid, ties to the even code (torch.round: half to even)
    c = torch.where(v < 2, torch.round(2 * v), torch.where(v < 4, torch.round(v) + 2, torch.round(0.5 * v) + 4)).long()
    c = c | (((s < 0) & (c != 0)).long() << 3)
    return (c.to(torch.uint8).numpy().reshape(-1), e.numpy().astype("<i4"), (g + 5).to(torch.uint8).numpy().reshape(-1))


def _encode_shared_cpu(codes, mask):
    codes = codes.detach().cpu().numpy().reshape(-1)
    n = codes.size
    keep = np.ones(n, dtype=bool) if mask is None else (mask.detach().cpu().numpy().reshape(-1) != 0)
    kept, words = int(keep.sum()), None
    if has_bits(n, kept, L.WZ_CODE):
        bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
        bits[:n] = keep
        words = np.packbits(bits, bitorder="little").view("<u8")
        codes = codes[keep]
    return dict(kept=kept, exps=None, words=words, values=np.ascontiguousarray(codes))


def _encode_cpu(w, mask, kind):
    shifts = None
    if kind == L.WZ_W4:
        codes, exps, shifts = _codes_w4_cpu(w, mask)
    else:
        codes, exps = _codes_cpu(w, mask, kind)
    n = codes.size
    keep = (codes & codes.dtype.type(_MAG_BITS[kind])) != 0
    kept = int(keep.sum())
    if has_bits(n, kept, kind):
        bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
        bits[:n] = keep
        words = np.packbits(bits, bitorder="little").view("<u8")
        values = codes[keep]
    else:
        words = None
        values = np.where(keep, codes, codes.dtype.type(0))
    return dict(kept=kept, exps=exps, shifts=shifts, words=words, values=np.ascontiguousarray(values))


def _check_words(rec, what):
    """The bit words of a record select exactly the `kept` values stored, and the tail bits of the last word are 0."""
    words, n = rec["words"], rec["n"]
    if words is None:
        return
    if hasattr(np, "bitwise_count"):
        ones = int(np.bitwise_count(words).sum(dtype=np.uint64))
    else:
        ones = int(np.unpackbits(words.view(np.uint8)).sum(dtype=np.uint64))
    if ones != rec["kept"] or (n % 64 and int(words[-1]) >> (n % 64)):
        raise McamdError("%s: the bit words do not select the %d values stored" % (what, rec["kept"]))


def _decode_cpu(rec, what):
    """(fp32 weights, fp32 mask) as flat numpy arrays from a parsed record with its payload."""
    n, kind = rec["n"], rec["kind"]
    dt = np.dtype(_CODE_DTYPE[kind])
    if kind == L.WZ_CODE:
        keep = np.ones(n, dtype=bool)
        if rec["words"] is not None:
            keep = np.unpackbits(rec["words"].view(np.uint8), bitorder="little")[:n].astype(bool)
        codes = np.zeros(n, dtype=np.uint8)
        codes[keep] = rec["codes"]
        rec["codes_full"] = codes
        return np.where(keep, rec["codebook"][codes], np.float32(0.0)).astype(np.float32), keep.astype(np.float32)
    if rec["words"] is not None:
        bits = np.unpackbits(rec["words"].view(np.uint8), bitorder="little")
        keep = bits[:n].astype(bool)
        codes = np.zeros(n, dtype=dt)
        codes[keep] = rec["codes"] if kind == L.WZ_W4 else rec["values"]
        mask = keep.astype(np.float32)
    else:
        codes = rec["codes"] if kind == L.WZ_W4 else rec["values"]
        mask = np.ones(n, dtype=np.float32)
    nz = (codes & dt.type(_MAG_BITS[kind])) != 0
    if kind == L.WZ_W4:                       # grid[code & 7] 2^(shift - 5 - e4_f), signed by bit 3: exact in float64, then in fp32
        cout, cin, kh, kw = rec["shape"]
        g = rec["shifts"].astype(np.int64).reshape(cout, cin // 32, 1, kh, kw) - 5
        g = np.broadcast_to(g, (cout, cin // 32, 32, kh, kw)).reshape(cout, -1)
        c = codes.reshape(cout, -1)
        w = np.ldexp(_W4_GRID[c & 7], g - rec["exps"].astype(np.int64).reshape(-1, 1)) * np.where(c & 8, -1.0, 1.0)
        return np.where(nz, w.reshape(-1), 0.0).astype(np.float32), mask
    if kind == L.WZ_FP32:
        w = codes.view("<f4")
    elif kind == L.WZ_FP16:
        w = codes.view("<f2").astype(np.float32)
    else:
        deq = torch.from_numpy(np.ascontiguousarray(codes)).view(torch.float8_e4m3fn).double().view(rec["cout"], -1)
        scale = torch.pow(2.0, -torch.from_numpy(rec["exps"].astype(np.int32)).double()).view(-1, 1)
        w = (deq * scale).float().numpy().reshape(-1)
    return np.where(nz, w, np.float32(0.0)).astype(np.float32), mask


# ----------------------------------------------------------------------------- the file
def _kinds(model, payload, layers):
    if payload not in PAYLOADS:
        raise McamdError("payload must be one of %r (got %r)" % (sorted(PAYLOADS), payload))
    convs = _conv_blocks(model)
    kind = PAYLOADS[payload]
    if kind == L.WZ_CODE:         # the layers set_codebooks tied as codes, every other layer as it is
        return convs, [L.WZ_CODE if getattr(conv, "share_flag", False) else L.WZ_FP32 for _, conv, _ in convs]
    if kind not in (L.WZ_FP8, L.WZ_W4):
        return convs, [kind] * len(convs)
    chosen = set(default_fp8_layers(model) if layers is None else [int(i) for i in layers])
    bad = sorted(chosen - set(i for i, _, _ in convs))
    if bad:
        raise McamdError("layers names conv numbers the model does not have: %r" % bad)
    if kind == L.WZ_W4:
        for i, conv, _ in convs:
            if i in chosen and conv.weight.shape[1] % 32:
                raise McamdError("conv%d has %d input channels: a layer of a \"w4\" file is stored in groups of 32 input channels"
                                 % (i, conv.weight.shape[1]))
    # every other layer of an fp8 / w4 file is what the "fp8" / "fp8-w4" engine runs there: fp16
    return convs, [kind if i in chosen else L.WZ_FP16 for i, _, _ in convs]


def _mask_of(conv):
    return conv.mask if getattr(conv, "mask_flag", False) else None


def _stream_width(kind, bits):
    """Bits per stored value of a kind whose values are uint8 symbols (WZ_FP8, WZ_CODE, WZ_W4) in an "MCZW" file."""
    return code_width(bits) if kind == L.WZ_CODE else 4 if kind == L.WZ_W4 else 8


def _code_device(items, kinds, words, counts, exps, values, shifts):
    """The device half of a coded save, behind ops.wz_pack: histograms of every stream (where a stream of values lies and how
    long it is follows from the kept counts, which are still on the device: ops.hz_histogram_at takes both from there), ONE
    read of the counts with the histograms, huffman_lengths per stream, ops.hz_encode_at, and ONE read of everything the file
    holds.  -> (counts, words, exps, values, shifts as _encode_device reads them, {(layer, stream name): stream bytes} of the
    streams that are Huffman-coded)."""
    from . import ops
    dev, nl = values.device, len(items)
    n = [it["w"].numel() for it in items]
    nw = [(x + 63) // 64 for x in n]
    V, W = values.numel(), 8 * words.numel()
    syms = torch.cat([values, words.view(torch.uint8)] + ([shifts[0]] if shifts else []))
    spans, where = [], []                     # (layer, 0 values / 1 bit words / 2 shift bytes, static offset, static count)
    w0 = s0 = 0
    for i, (it, kind) in enumerate(zip(items, kinds)):
        if kind == L.WZ_W4:
            spans.append(dict(sym0=0, nsym=n[i] // 32, A=_W4_SHIFT_MAX + 1, layer=i, name="group shifts"))
            where.append((i, 2, V + W + s0, n[i] // 32))
            s0 += _pad8(n[i] // 32)
        spans.append(dict(sym0=0, nsym=8 * nw[i], A=256, layer=i, name="bit words"))
        where.append((i, 1, V + 8 * w0, 0))
        w0 += nw[i]
        if kind in (L.WZ_FP8, L.WZ_CODE, L.WZ_W4):
            A = 1 << int(it["K"]).bit_length() - 1 if kind == L.WZ_CODE else 16 if kind == L.WZ_W4 else 256
            spans.append(dict(sym0=0, nsym=n[i], A=A, layer=i, name="values" if kind == L.WZ_FP8 else "codes"))
            where.append((i, 0, 0, 0))
    t = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)
    n_t, nw_t, el_t = t(n), t(nw), t([ELEM[k] for k in kinds])
    is_code, is_w4 = t([k == L.WZ_CODE for k in kinds]).bool(), t([k == L.WZ_W4 for k in kinds]).bool()
    kept = counts.view(torch.int64)
    bits_t = torch.where(is_code, kept < n_t, torch.where(is_w4, 8 * nw_t + (kept + 1) // 2 < (n_t + 1) // 2,
                                                          8 * nw_t + kept * el_t < n_t * el_t))       # has_bits, per layer
    stored = torch.where(bits_t, kept, n_t)
    padded = (stored * el_t + 7) // 8 * 8
    base = torch.cumsum(padded, 0) - padded
    lay, typ, off0, cnt0 = (t([w[j] for w in where]) for j in range(4))
    off = torch.where(typ == 0, base[lay], off0)
    cnt = torch.where(typ == 0, stored[lay], torch.where(typ == 1, bits_t[lay].long() * 8 * nw_t[lay], cnt0))
    hist = ops.hz_histogram_at(syms, spans, dyn=torch.stack([off, cnt], 1).contiguous())
    first = torch.cat([kept, hist.view(-1)]).cpu().numpy()                      # synchronising read 1: counts and histograms
    counts, hist = [int(c) for c in first[:nl]], first[nl:].reshape(len(spans), 256)
    # the same layout on the host, now that the counts are here
    bases, v0 = [], 0
    for i, kind in enumerate(kinds):
        bases.append(v0)
        v0 += _pad8((counts[i] if has_bits(n[i], counts[i], kind) else n[i]) * ELEM[kind])
    jobs = []
    for sp, (i, ty, o, c), h in zip(spans, where, hist):
        bits = has_bits(n[i], counts[i], kinds[i])
        if ty == 0:
            sp["sym0"], sp["nsym"] = bases[i], counts[i] if bits else n[i]
            raw = (sp["nsym"] * _stream_width(kinds[i], sp["A"].bit_length() - 1) + 7) // 8
        else:
            sp["sym0"], sp["nsym"] = o, c if ty == 2 else 8 * nw[i] if bits else 0
            raw = sp["nsym"]
        if int(h.sum()) != sp["nsym"]:
            raise McamdError("conv%d %s: the histogram counts %d of %d symbols" % (i + 1, sp["name"], int(h.sum()), sp["nsym"]))
        mode, lengths, nbits = _hz_plan(h, sp["A"], _pad8(raw))
        if mode == 1:
            jobs.append(dict(sp, nbits=nbits, lengths=lengths))
    ctab = bits = None
    parts = [values[:v0], words.view(torch.uint8), exps.view(torch.uint8)] + ([shifts[0]] if shifts else [])
    if jobs:
        ctab, bits = ops.hz_encode_at(syms, jobs, [j["lengths"] for j in jobs])
        parts += [ctab.view(torch.uint8), bits.view(torch.uint8)]
    host = torch.cat(parts).cpu().numpy()                                       # synchronising read 2: what the file holds
    cuts = np.cumsum([0] + [p.numel() for p in parts])
    piece = [host[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    streams = {}
    if jobs:
        ctab, bits = piece[-2].view("<u4"), piece[-1].view("<u8")
        c0 = b0 = 0
        for j in jobs:
            nc, nwords = (j["nsym"] + HZ_CHUNK - 1) // HZ_CHUNK, (j["nbits"] + 63) // 64
            streams[(j["layer"], j["name"])] = _hz_pack(j["A"], j["nsym"], j["nbits"], j["lengths"], ctab[c0:c0 + nc],
                                                        bits[b0:b0 + nwords])
            c0, b0 = c0 + nc, b0 + nwords
    return (counts, piece[1].view("<u8"), piece[2].view("<i4"), piece[0], piece[3] if shifts else None, streams)


def _encode_device(convs, kinds, coded=False):
    """The device path: every layer through one ops.wz_pack table, one host read of counts, words, exponents and values.
    coded: -> (records, streams of _code_device) for a Huffman-coded file."""
    from . import ops
    items = []
    for (_, conv, _), kind in zip(convs, kinds):
        w, m = conv.weight.data, _mask_of(conv)
        if kind == L.WZ_CODE:
            items.append(dict(w=conv.codes.contiguous(), mask=m.contiguous().float() if m is not None else None, kind=kind,
                              K=int(conv.codebook.numel())))
            continue
        if w.dtype != torch.float32:
            raise McamdError("compressed model files are written from fp32 master weights")
        items.append(dict(w=w.contiguous(), mask=m.contiguous().float() if m is not None else None, kind=kind))
    words, counts, exps, values, *shifts = ops.wz_pack(items)
    streams = None
    if coded:
        counts, words, exps, values, shifts, streams = _code_device(items, kinds, words, counts, exps, values, shifts)
    else:
        counts = [int(c) for c in counts.cpu().numpy().view("<u8")]                # the one synchronising read
        words, exps = words.cpu().numpy().view("<u8"), exps.cpu().numpy().astype("<i4", copy=False)
        shifts = shifts[0].cpu().numpy() if shifts else None
    sizes = []
    for it, kind, kept in zip(items, kinds, counts):
        n = it["w"].numel()
        sizes.append((kept if has_bits(n, kept, kind) else n) * ELEM[kind])
    if not coded:
        values = values[:sum(_pad8(s) for s in sizes)].cpu().numpy()
    out, w0, e0, v0, s0 = [], 0, 0, 0, 0
    for it, kind, kept, size in zip(items, kinds, counts, sizes):
        n, cout = it["w"].numel(), it["w"].shape[0]
        nwords = (n + 63) // 64
        rec = dict(kept=kept, exps=None, shifts=None, words=None, values=values[v0:v0 + size].view(_CODE_DTYPE[kind]))
        if has_bits(n, kept, kind):
            rec["words"] = words[w0:w0 + nwords]
        if kind in (L.WZ_FP8, L.WZ_W4):
            rec["exps"] = exps[e0:e0 + cout]
            e0 += cout
        if kind == L.WZ_W4:
            rec["shifts"] = shifts[s0:s0 + n // 32]
            s0 += _pad8(n // 32)
        w0 += nwords
        v0 += _pad8(size)
        out.append(rec)
    return (out, streams) if coded else out


def _write_array(f, a):
    b = a.tobytes()
    f.write(b)
    f.write(b"\0" * (_pad8(len(b)) - len(b)))


def _write_file(f, payload_kind, seen, rows, coder=None):
    """THE writer of both containers.  rows: per conv dict(shape, bn, kind, bits, kept, small, exps, shifts, codebook, words,
    values), `values` of WZ_CODE and WZ_W4 one code per byte.  coder None: an "MCZW" file.  Otherwise an "MCZH" file, and
    coder(layer, stream name, uint8 symbols, alphabet, the array as "MCZW" stores it) gives the bytes of each stream."""
    f.write(_HEADER.pack(MAGIC if coder is None else HZ_MAGIC, VERSION if coder is None else HZ_VERSION, payload_kind, len(rows),
                         seen))
    for s, row in enumerate(rows):
        def put(name, symbols, A, stored):
            if coder is None:
                _write_array(f, stored)
            else:
                f.write(coder(s, name, symbols, A, stored))

        kind, bits = row["kind"], row["bits"]
        cout, cin, kh, kw = row["shape"]
        flags = (L.WZ_F_BN if row["bn"] else 0) | (L.WZ_F_BITS if row["words"] is not None else 0) | (kind << 8)
        f.write(_RECORD.pack(cout, cin, kh, kw, flags, bits, row["kept"]))
        for a in row["small"]:
            _write_array(f, a)
        if kind in (L.WZ_FP8, L.WZ_W4):
            _write_array(f, row["exps"].astype("<i4", copy=False))
        if kind == L.WZ_W4:
            put("group shifts", row["shifts"], _W4_SHIFT_MAX + 1, row["shifts"])
        if kind == L.WZ_CODE:
            _write_array(f, row["codebook"])
        if row["words"] is not None:
            put("bit words", row["words"].view(np.uint8), 256, row["words"])
        if kind == L.WZ_FP8:
            put("values", row["values"], 256, row["values"])
        elif kind in (L.WZ_CODE, L.WZ_W4):
            width = _stream_width(kind, bits)
            put("codes", row["values"], 1 << bits if kind == L.WZ_CODE else 16,
                _pack_codes(row["values"], width) if width < 8 else row["values"])
        else:
            _write_array(f, row["values"])


def _host_coder(s, name, symbols, A, stored):
    return _hz_stream_bytes(symbols, A, stored)


def save_compressed(model, path, payload="fp16", layers=None, entropy=None):
    """Write `model` as an .mcz file.  payload: "fp32" (bit patterns of weight * mask), "fp16" (what the fp16 engines
    consume), "fp8" (the conv numbers in `layers` as e4m3 codes + one exponent per filter, every other layer as fp16;
    `layers` defaults to default_fp8_layers(model), pass Engine.fp8_layers to be exact for any cfg) or "w4" (the conv numbers
    in `layers` as 4-bit codes + one shift byte per group of 32 input channels + one exponent per filter, every other layer
    as fp16; the same default, pass Engine.fp8_w4_layers to be exact for any cfg; a chosen layer needs cin % 32 == 0).  A weight
    is stored iff its value in the payload is non-zero.  entropy: None (an "MCZW" file) or "huffman" (an "MCZH" file, DESIGN.md
    3z: the same records with the bit words, shift bytes, e4m3 bytes and codes as Huffman streams; a model on the GPU is coded
    there, ops.hz_histogram_at / ops.hz_encode_at)."""
    _check_entropy(entropy)
    convs, kinds = _kinds(model, payload, layers)
    if not convs:
        raise McamdError("the model has no convolutional block to store")
    coder = None if entropy is None else _host_coder
    if all(conv.weight.is_cuda for _, conv, _ in convs):
        encoded = _encode_device(convs, kinds, coded=entropy is not None)
        if entropy is not None:
            encoded, streams = encoded
            coder = lambda s, name, symbols, A, stored: streams.get((s, name)) or _hz_raw(A, symbols.size, stored)
    else:
        encoded = [_encode_shared_cpu(conv.codes, _mask_of(conv)) if kind == L.WZ_CODE else
                   _encode_cpu(conv.weight.data.cpu(), (_mask_of(conv).cpu() if _mask_of(conv) is not None else None), kind)
                   for (_, conv, _), kind in zip(convs, kinds)]
    rows = []
    for (_, conv, bn), kind, rec in zip(convs, kinds, encoded):
        tied = kind == L.WZ_CODE
        rows.append(dict(shape=tuple(conv.weight.shape), bn=bn is not None, kind=kind, kept=rec["kept"],
                         bits=int(conv.codebook.numel()).bit_length() - 1 if tied else 0, small=_small_arrays(conv, bn),
                         exps=rec["exps"], shifts=rec.get("shifts"), words=rec["words"], values=rec["values"],
                         codebook=conv.codebook.detach().cpu().numpy().astype("<f4", copy=False) if tied else None))
    with open(path, "wb") as f:
        _write_file(f, PAYLOADS[payload], int(model.seen), rows, coder)


def _parse(path, payload=True, decode=True):
    """Header and records of an .mcz file of either container.  payload False: shapes, kinds, counts, byte offsets and stream
    headers only.  decode False: the Huffman streams of a coded file are parsed and checked but not decoded (the device does
    that): the arrays they stand for stay None."""
    with open(path, "rb") as f:
        return _parse_open(f, path, os.path.getsize(path), payload, decode)


def _parse_open(f, path, size, payload, decode=True):
    raw = f.read() if payload else None
    pos = 0

    def take(nbytes, what):
        nonlocal pos
        if pos + nbytes > size:
            raise McamdError("%s: truncated file (%s needs %d bytes at offset %d of %d)" % (path, what, nbytes, pos, size))
        start = pos
        pos += nbytes
        return start

    def head(nbytes, what):
        start = take(nbytes, what)
        if raw is not None:
            return raw[start:start + nbytes]
        f.seek(start)
        return f.read(nbytes)

    def stream(name, A, nsym, raw_bytes, what):
        """The header of a stream and where its parts lie; a Huffman stream's lengths and chunk table are checked here."""
        start = pos
        mode, a, ns = _STREAM.unpack(head(_STREAM.size, what + " stream header"))
        if mode not in (0, 1):
            raise McamdError("%s: %s: stream mode %d (0 = raw, 1 = Huffman)" % (path, what, mode))
        if a != A or ns != nsym:
            raise McamdError("%s: %s: a stream of %d symbols over an alphabet of %d where the record implies %d over %d"
                             % (path, what, ns, a, nsym, A))
        st = dict(name=name, mode=mode, A=A, nsym=nsym, raw_bytes=_pad8(raw_bytes), off=None)
        if mode == 0:
            st["off"] = take(_pad8(raw_bytes), what)
        else:
            nbits, = struct.unpack("<Q", head(8, what + " nbits"))
            if not 0 < nsym <= nbits <= HZ_MAXLEN * nsym or nbits >= 1 << 32:
                raise McamdError("%s: %s: %d code bits for %d symbols" % (path, what, nbits, nsym))
            nchunks, nwords = (nsym + HZ_CHUNK - 1) // HZ_CHUNK, (nbits + 63) // 64
            st.update(nbits=nbits, nchunks=nchunks, nwords=nwords, len0=take(_pad8(A), what + " code lengths"),
                      chunk0=take(_pad8(4 * nchunks), what + " chunk table"))
            if pos + 8 * nwords > size:
                raise McamdError("%s: %s: truncated file: %d code bits are beyond the words present (%d bytes at offset %d of %d)"
                                 % (path, what, nbits, 8 * nwords, pos, size))
            st["bits0"] = take(8 * nwords, what + " code bits")
            if raw is not None:
                st["lengths"] = np.frombuffer(raw, "u1", A, st["len0"])
                _hz_check_lengths(st["lengths"], "%s: %s" % (path, what))
                st["chunk_bit0"] = c = np.frombuffer(raw, "<u4", nchunks, st["chunk0"])
                if int(c[0]) != 0 or bool((c[1:] < c[:-1]).any()) or int(c[-1]) > nbits:
                    raise McamdError("%s: %s: chunk_bit0 does not start at 0, decreases or passes the %d code bits" % (path, what, nbits))
        st["bytes"] = pos - start
        return st

    magic, version, pay, nrec, seen = _HEADER.unpack(head(_HEADER.size, "the header"))
    if magic not in (MAGIC, HZ_MAGIC):
        raise McamdError("%s: not a compressed model file (magic %r, expected %r or %r)" % (path, magic, MAGIC, HZ_MAGIC))
    coded = magic == HZ_MAGIC
    if version != (HZ_VERSION if coded else VERSION):
        raise McamdError("%s: compressed model file version %d is not supported (this reader reads version %d)"
                         % (path, version, HZ_VERSION if coded else VERSION))
    if pay not in KIND_NAMES:
        raise McamdError("%s: unknown payload kind %d" % (path, pay))
    recs = []
    for r in range(nrec):
        what = "conv%d" % (r + 1)
        start = pos
        cout, cin, kh, kw, flags, cbits, kept = _RECORD.unpack(head(_RECORD.size, what))
        kind = (flags >> 8) & 0xFF
        if min(cout, cin, kh, kw) <= 0 or kind not in KIND_NAMES or flags & ~(0xFF00 | L.WZ_F_BN | L.WZ_F_BITS):
            raise McamdError("%s: %s: damaged record header" % (path, what))
        if kind == L.WZ_CODE and (pay != L.WZ_CODE or not 1 <= cbits <= 8):
            raise McamdError("%s: %s: damaged record header (codes of %d bits in a %r file)" % (path, what, cbits, KIND_NAMES[pay]))
        if kind == L.WZ_W4 and (pay != L.WZ_W4 or cin % 32):
            raise McamdError("%s: %s: damaged record header (4-bit codes of %d input channels in a %r file)" % (path, what, cin,
                                                                                                            KIND_NAMES[pay]))
        n = cout * cin * kh * kw
        bits = bool(flags & L.WZ_F_BITS)
        if kept > n or bits != has_bits(n, kept, kind):
            raise McamdError("%s: %s: damaged record header (kept %d of %d weights)" % (path, what, kept, n))
        rec = dict(shape=(cout, cin, kh, kw), cout=cout, n=n, bn=bool(flags & L.WZ_F_BN), bits=bits, kind=kind, kept=kept,
                   small=[], exps=None, words=None, values=None, exp0=0, word0=0, code_bits=None, codebook=None, codes=None,
                   shifts=None, shift0=0, streams=[])

        def array(name, A, nsym, raw_bytes, label):
            """Where an array of uint8 symbols lies: (its byte offset as "MCZW" stores it, or None when it is a Huffman stream;
            its symbols decoded from that stream, or None)."""
            if not coded:
                return take(_pad8(raw_bytes), label), None
            st = stream(name, A, nsym, raw_bytes, label)
            rec["streams"].append(st)
            if st["mode"] == 1 and raw is not None and decode:
                return None, _hz_decode_stream(raw, st, "%s: %s" % (path, label))
            return st["off"], None

        for _ in range(4 if rec["bn"] else 1):
            o = take(_pad8(4 * cout), what + " per-channel arrays")
            if raw is not None:
                rec["small"].append(np.frombuffer(raw, "<f4", cout, o))
        if kind in (L.WZ_FP8, L.WZ_W4):
            o = rec["exp0"] = take(_pad8(4 * cout), what + " exponents")
            if raw is not None:
                rec["exps"] = np.frombuffer(raw, "<i4", cout, o)
        if kind == L.WZ_W4:
            o, sy = array("group shifts", _W4_SHIFT_MAX + 1, n // 32, n // 32, what + " group shifts")
            rec["shift0"] = o
            if raw is not None and o is not None:
                sy = np.frombuffer(raw, "u1", n // 32, o)
            if sy is not None:
                rec["shifts"] = sy
                if int(rec["shifts"].max()) > _W4_SHIFT_MAX:
                    raise McamdError("%s: %s: a group shift byte of %d (0..%d)" % (path, what, int(rec["shifts"].max()), _W4_SHIFT_MAX))
        if kind == L.WZ_CODE:
            rec["code_bits"] = cbits
            o = take(_pad8(4 << cbits), what + " codebook")
            if raw is not None:
                rec["codebook"] = np.frombuffer(raw, "<f4", 1 << cbits, o)
        if bits:
            nw = (n + 63) // 64
            o, sy = array("bit words", 256, 8 * nw, 8 * nw, what + " bit words")
            rec["word0"] = o
            if raw is not None and o is not None:
                rec["words"] = np.frombuffer(raw, "<u8", nw, o)
            elif sy is not None:
                rec["words"] = sy.view("<u8")
        stored = kept if bits else n
        if kind == L.WZ_CODE:
            width = code_width(cbits)
            nbytes = (stored * width + 7) // 8
            rec["val0"], sy = array("codes", 1 << cbits, stored, nbytes, what + " codes")
            if raw is not None and rec["val0"] is not None:
                rec["values"] = np.frombuffer(raw, "u1", nbytes, rec["val0"])
                sy = _unpack_codes(rec["values"], width, stored)
            if sy is not None:
                rec["codes"] = sy
                if stored and int(rec["codes"].max()) >= 1 << cbits:
                    raise McamdError("%s: %s: a code of %d with a codebook of %d entries" % (path, what, int(rec["codes"].max()),
                                                                                          1 << cbits))
        elif kind == L.WZ_W4:
            nbytes = (stored + 1) // 2
            rec["val0"], sy = array("codes", 16, stored, nbytes, what + " codes")
            if raw is not None and rec["val0"] is not None:
                rec["values"] = np.frombuffer(raw, "u1", nbytes, rec["val0"])
                sy = _unpack_codes(rec["values"], 4, stored)
                if stored % 2 and int(rec["values"][-1]) >> 4:
                    raise McamdError("%s: %s: the unused nibble behind the last code is not 0" % (path, what))
            if sy is not None:
                rec["codes"] = sy
                # a kept weight has a non-zero grid index, every other stored code is +0
                if int(np.count_nonzero(rec["codes"] & 7)) != kept or bool((rec["codes"] == 8).any()):
                    raise McamdError("%s: %s: the codes stored do not hold the %d kept weights" % (path, what, kept))
        elif kind == L.WZ_FP8:
            rec["val0"], sy = array("values", 256, stored, stored, what + " values")
            if raw is not None and rec["val0"] is not None:
                sy = np.frombuffer(raw, "u1", stored, rec["val0"])
            rec["values"] = sy
        else:
            rec["val0"] = take(_pad8(stored * ELEM[kind]), what + " values")
            if raw is not None:
                rec["values"] = np.frombuffer(raw, _CODE_DTYPE[kind], stored, rec["val0"])
        rec["bytes"] = pos - start
        recs.append(rec)
    if pos != size:
        raise McamdError("%s: %d bytes behind the last record" % (path, size - pos))
    return dict(payload=KIND_NAMES[pay], seen=seen, records=recs, bytes=size, raw=raw, entropy="huffman" if coded else None)


def _decode_device(path, recs, buf, S):
    """Decode every Huffman stream of a coded file on the device: `buf` holds S bytes of scratch and then the file; stream st
    goes to buf[st["dev0"] ...].  One read of the stream flags, the population counts of the decoded bit words and the counts
    the host parser takes of 4-bit codes; a file that fails one is refused as the numpy path refuses it."""
    from . import ops
    jobs = [(r, rec, st) for r, rec in enumerate(recs) for st in rec["streams"] if st["mode"] == 1]
    spans = [dict(sym0=st["dev0"], nsym=st["nsym"], A=st["A"], nbits=st["nbits"], word0=(S + st["bits0"]) // 8,
                  chunk0=(S + st["chunk0"]) // 4, popc_bits=rec["n"] if st["name"] == "bit words" else 0) for _, rec, st in jobs]
    stats = ops.hz_decode_at(spans, [st["lengths"] for _, _, st in jobs], buf.view(torch.int32), buf.view(torch.int64), buf)
    extra = []
    for _, rec, st in jobs:
        if rec["kind"] == L.WZ_W4 and st["name"] == "codes":
            codes = buf[st["dev0"]:st["dev0"] + st["nsym"]]
            extra += [torch.count_nonzero(codes & 7).view(1), (codes == 8).sum().view(1)]
    host = torch.cat([stats.view(-1)] + extra).cpu().numpy()                     # the one read
    stats, extra = host[:2 * len(jobs)].reshape(-1, 2), list(host[2 * len(jobs):])
    for (r, rec, st), (flag, ones) in zip(jobs, stats):
        what = "%s: conv%d" % (path, r + 1)
        if int(flag) & 1:
            raise McamdError("%s %s: the coded stream is damaged (a chunk does not end where the next one begins, or holds an "
                             "unassigned code)" % (what, st["name"]))
        if st["name"] == "bit words" and (int(flag) & 2 or int(ones) != rec["kept"]):
            raise McamdError("%s: the bit words do not select the %d values stored" % (what, rec["kept"]))
        if rec["kind"] == L.WZ_W4 and st["name"] == "codes":
            nonzero, minus0 = int(extra.pop(0)), int(extra.pop(0))
            if nonzero != rec["kept"] or minus0:
                raise McamdError("%s: the codes stored do not hold the %d kept weights" % (what, rec["kept"]))


def load_compressed(model, path, set_masks=True):
    """Fill `model` from an .mcz file: fp32 master weights (fp32 as is, fp16 widened, e4m3 as value 2^-exponent,
    4-bit codes as grid[code] 2^g 2^-e4_f), BatchNorm tensors, biases and `seen`.  Every record's shape is checked against
    the cfg before anything is written.  Returns the list of kept-bit masks (all ones for a record without a bitmask) and, when `set_masks` and at least one record has a
    bitmask, hands it to model.set_masks.  A "shared" file: the codes are widened on the host, expanded
    through the codebooks on the device (ops.WsTable.expand), and -- with `set_masks` -- the codebooks are set as
    Darknet.set_codebooks sets them, so that retraining and save_compressed(payload="shared") go on from the file."""
    convs = _conv_blocks(model)
    on_device = bool(convs) and all(conv.weight.is_cuda for _, conv, _ in convs)
    info = _parse(path, decode=not on_device)        # (a coded file's streams are decoded where the model is)
    recs = info["records"]
    if len(recs) != len(convs):
        raise McamdError("%s holds %d conv records, the cfg has %d convolutional blocks" % (path, len(recs), len(convs)))
    for (i, conv, bn), rec in zip(convs, recs):
        if tuple(conv.weight.shape) != rec["shape"] or (bn is not None) != rec["bn"]:
            raise McamdError("%s: conv%d is %s%s in the file and %s%s in the cfg" % (
                path, i, rec["shape"], " with BatchNorm" if rec["bn"] else "", tuple(conv.weight.shape),
                " with BatchNorm" if bn is not None else ""))
    for (i, _, _), rec in zip(convs, recs):           # on the host, where the words are: the same refusal on either path
        _check_words(rec, "%s: conv%d" % (path, i))
    masks, books = [], [None] * len(recs)
    if on_device:
        from . import ops
        dev = convs[0][1].weight.device
        items, shared = [], []
        buf = bytearray(info["raw"])
        # a coded file: the device buffer begins with S bytes of scratch, one range per Huffman stream, into which
        # ops.hz_decode_at writes what ops.wz_unpack reads (bit words, one byte per code, e4m3 bytes, shift bytes); the file
        # follows at byte S.  S = 0 for an "MCZW" file.
        S = 0
        for rec in recs:
            for st in rec["streams"]:
                if st["mode"] == 1:
                    st["dev0"], S = S, S + _pad8(st["nsym"])
        for s, ((_, conv, _), rec) in enumerate(zip(convs, recs)):
            if conv.weight.dtype != torch.float32 or not conv.weight.data.is_contiguous():
                raise McamdError("compressed model files are read into contiguous fp32 master weights")
            masks.append(torch.empty_like(conv.weight.data))
            at = {st["name"]: st["dev0"] for st in rec["streams"] if st["mode"] == 1}     # decoded on the device
            target, val0 = conv.weight.data, at.get("values", at.get("codes"))
            if val0 is None:
                val0 = S + rec["val0"]
            if rec["kind"] == L.WZ_CODE:
                target = torch.empty(rec["shape"], dtype=torch.uint8, device=dev)
                shared.append(s)
                books[s] = (torch.from_numpy(rec["codebook"].astype(np.float32)).to(dev), target)
            if rec["kind"] in (L.WZ_CODE, L.WZ_W4) and "codes" not in at:
                # one byte per code for the device pass, behind the file's own bytes (the sub-byte widening of codes stored
                # at their width is a host pass); the exponents and shift bytes are read in place
                val0 = S + len(buf)
                b = rec["codes"].tobytes()
                buf += b + b"\0" * (_pad8(len(b)) - len(b))
            word0 = at["bit words"] if "bit words" in at else S + rec["word0"]
            shift0 = at["group shifts"] if "group shifts" in at else S + rec["shift0"]
            items.append(dict(w=target, mask=masks[-1], kind=rec["kind"], dense=not rec["bits"], kept=rec["kept"],
                              val0=val0, word0=word0 // 8, exp0=(S + rec["exp0"]) // 4, shift0=shift0 // 8))
        if S + len(buf) >= 1 << 33:
            raise McamdError("%s: a file of 8 GiB or more is not read on the device" % path)
        # the file's bytes go up once, as they are, and are expanded next to the weights: a record's bit words, exponents
        # and values are read in place (every array of the file starts at a multiple of 8 bytes)
        if S:
            values = torch.empty(S + len(buf), dtype=torch.uint8, device=dev)
            values[S:].copy_(torch.frombuffer(buf, dtype=torch.uint8))
            _decode_device(path, recs, values, S)                 # refuses a damaged file here: the model is untouched
        else:
            values = torch.frombuffer(buf, dtype=torch.uint8).to(dev)
        words, exps = values.view(torch.int64), values.view(torch.int32)
        ops.wz_unpack(items, words, exps, values, values)
        if shared:
            table = ops.WsTable([dict(w=convs[s][1].weight.data, mask=masks[s] if recs[s]["bits"] else None, codes=books[s][1],
                                      K=1 << recs[s]["code_bits"]) for s in shared],
                                codebook=torch.cat([books[s][0] for s in shared]))
            table.expand()
    else:
        for s, ((i, conv, _), rec) in enumerate(zip(convs, recs)):
            w, m = _decode_cpu(rec, "%s: conv%d" % (path, i))
            conv.weight.data.copy_(torch.from_numpy(w).view(rec["shape"]))
            masks.append(torch.from_numpy(m).view(rec["shape"]).to(conv.weight.device))
            if rec["kind"] == L.WZ_CODE:
                books[s] = (torch.from_numpy(rec["codebook"].astype(np.float32)),
                            torch.from_numpy(rec["codes_full"]).view(rec["shape"]))
    for (_, conv, bn), rec in zip(convs, recs):
        for t, a in zip(_small_targets(conv, bn), rec["small"]):
            t.copy_(torch.from_numpy(a.astype(np.float32)))
    model.seen = int(info["seen"])
    model._mark_weights_replaced()
    if set_masks and any(rec["bits"] for rec in recs):
        model.set_masks(masks)
    if set_masks and any(b is not None for b in books):
        from . import share
        share.set_codebooks(model, books, expand_weights=False)      # (the weights above are the expansion already)
    return masks


def compressed_info(path):
    """What an .mcz file holds, from its header and record headers alone (no GPU, no model): per conv its shape, value
    kind, kept count and bytes; the totals; and the ratio against the dense float32 .weights file of the same cfg."""
    info = _parse(path, payload=False)
    layers, dense = [], 16
    for i, rec in enumerate(info["records"]):
        layers.append(dict(conv=i + 1, shape=rec["shape"], kind=KIND_NAMES[rec["kind"]], bitmask=rec["bits"], kept=rec["kept"],
                           weights=rec["n"], bytes=rec["bytes"]))
        if rec["kind"] == L.WZ_CODE:      # a tied layer: its code bits, their width in the file and the codebook's entries
            layers[-1].update(bits=rec["code_bits"], width=code_width(rec["code_bits"]), codebook=1 << rec["code_bits"])
        dense += 4 * (rec["n"] + rec["cout"] * (4 if rec["bn"] else 1))
        if info["entropy"] is not None:   # a coded file: its streams (raw_bytes: the array in the "MCZW" twin, padding included)
            layers[-1]["streams"] = [dict(name=st["name"], mode=st["mode"], nsym=st["nsym"], bytes=st["bytes"],
                                          raw_bytes=st["raw_bytes"]) for st in rec["streams"]]
    out = dict(payload=info["payload"], seen=info["seen"], layers=layers, weights=sum(l["weights"] for l in layers),
               kept=sum(l["kept"] for l in layers), bytes=info["bytes"], dense_bytes=dense, ratio=dense / info["bytes"])
    if info["entropy"] is not None:
        out.update(entropy=info["entropy"], plain_bytes=info["bytes"] - sum(st["bytes"] - st["raw_bytes"] for l in layers
                                                                           for st in l["streams"]))
    return out


def transcode(src, dst, entropy):
    """Rewrite the .mcz file `src` of either container as `dst`: entropy None an "MCZW" file, "huffman" an "MCZH" file (the
    same container included).  Host only, no model: the records are parsed, a coded file's streams decoded, and THE writer
    writes them again, so transcode(coded, dst, None) is the "MCZW" file the same save_compressed call writes."""
    _check_entropy(entropy)
    info = _parse(src)
    rows = []
    for rec in info["records"]:
        tied = rec["kind"] in (L.WZ_CODE, L.WZ_W4)
        rows.append(dict(shape=rec["shape"], bn=rec["bn"], kind=rec["kind"], bits=rec["code_bits"] or 0, kept=rec["kept"],
                         small=rec["small"], exps=rec["exps"], shifts=rec["shifts"], codebook=rec["codebook"],
                         words=rec["words"], values=rec["codes"] if tied else rec["values"]))
    with open(dst, "wb") as f:
        _write_file(f, PAYLOADS[info["payload"]], info["seen"], rows, None if entropy is None else _host_coder)
