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
        return f.read(4) == MAGIC


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


def _encode_device(convs, kinds):
    """The device path: every layer through one ops.wz_pack table, one host read of counts, words, exponents and values."""
    from . import ops
    items = []
    for (_, conv, _), kind in zip(convs, kinds):
        w, m = conv.weight.data, _mask_of(conv)
        if kind == L.WZ_CODE:
            items.append(dict(w=conv.codes.contiguous(), mask=m.contiguous().float() if m is not None else None, kind=kind))
            continue
        if w.dtype != torch.float32:
            raise McamdError("compressed model files are written from fp32 master weights")
        items.append(dict(w=w.contiguous(), mask=m.contiguous().float() if m is not None else None, kind=kind))
    words, counts, exps, values, *shifts = ops.wz_pack(items)
    counts = [int(c) for c in counts.cpu().numpy().view("<u8")]                # the one synchronising read
    words, exps = words.cpu().numpy().view("<u8"), exps.cpu().numpy().astype("<i4", copy=False)
    shifts = shifts[0].cpu().numpy() if shifts else None
    sizes = []
    for it, kind, kept in zip(items, kinds, counts):
        n = it["w"].numel()
        sizes.append((kept if has_bits(n, kept, kind) else n) * ELEM[kind])
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
    return out


def _write_array(f, a):
    b = a.tobytes()
    f.write(b)
    f.write(b"\0" * (_pad8(len(b)) - len(b)))


def save_compressed(model, path, payload="fp16", layers=None):
    """Write `model` as an .mcz file.  payload: "fp32" (bit patterns of weight * mask), "fp16" (what the fp16 engines
    consume), "fp8" (the conv numbers in `layers` as e4m3 codes + one exponent per filter, every other layer as fp16;
    `layers` defaults to default_fp8_layers(model), pass Engine.fp8_layers to be exact for any cfg) or "w4" (the conv numbers
    in `layers` as 4-bit codes + one shift byte per group of 32 input channels + one exponent per filter, every other layer
    as fp16; the same default, pass Engine.fp8_w4_layers to be exact for any cfg; a chosen layer needs cin % 32 == 0).  A weight
    is stored iff its value in the payload is non-zero."""
    convs, kinds = _kinds(model, payload, layers)
    if not convs:
        raise McamdError("the model has no convolutional block to store")
    if all(conv.weight.is_cuda for _, conv, _ in convs):
        encoded = _encode_device(convs, kinds)
    else:
        encoded = [_encode_shared_cpu(conv.codes, _mask_of(conv)) if kind == L.WZ_CODE else
                   _encode_cpu(conv.weight.data.cpu(), (_mask_of(conv).cpu() if _mask_of(conv) is not None else None), kind)
                   for (_, conv, _), kind in zip(convs, kinds)]
    with open(path, "wb") as f:
        f.write(_HEADER.pack(MAGIC, VERSION, PAYLOADS[payload], len(convs), int(model.seen)))
        for (_, conv, bn), kind, rec in zip(convs, kinds, encoded):
            cout, cin, kh, kw = conv.weight.shape
            flags = (L.WZ_F_BN if bn is not None else 0) | (L.WZ_F_BITS if rec["words"] is not None else 0) | (kind << 8)
            bits = 0
            if kind == L.WZ_CODE:
                bits = int(conv.codebook.numel()).bit_length() - 1
            f.write(_RECORD.pack(cout, cin, kh, kw, flags, bits, rec["kept"]))
            for a in _small_arrays(conv, bn):
                _write_array(f, a)
            if kind in (L.WZ_FP8, L.WZ_W4):
                _write_array(f, rec["exps"].astype("<i4", copy=False))
            if kind == L.WZ_W4:
                _write_array(f, rec["shifts"])
            if kind == L.WZ_CODE:
                _write_array(f, conv.codebook.detach().cpu().numpy().astype("<f4", copy=False))
            if rec["words"] is not None:
                _write_array(f, rec["words"])
            width = code_width(bits) if kind == L.WZ_CODE else 4 if kind == L.WZ_W4 else 8
            _write_array(f, _pack_codes(rec["values"], width) if width < 8 else rec["values"])


def _parse(path, payload=True):
    """Header and records of an .mcz file.  payload False: shapes, kinds, counts and byte offsets only."""
    with open(path, "rb") as f:
        return _parse_open(f, path, os.path.getsize(path), payload)


def _parse_open(f, path, size, payload):
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

    magic, version, pay, nrec, seen = _HEADER.unpack(head(_HEADER.size, "the header"))
    if magic != MAGIC:
        raise McamdError("%s: not a compressed model file (magic %r, expected %r)" % (path, magic, MAGIC))
    if version != VERSION:
        raise McamdError("%s: compressed model file version %d is not supported (this reader reads version %d)" % (path, version, VERSION))
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
                   shifts=None, shift0=0)
        for _ in range(4 if rec["bn"] else 1):
            o = take(_pad8(4 * cout), what + " per-channel arrays")
            if raw is not None:
                rec["small"].append(np.frombuffer(raw, "<f4", cout, o))
        if kind in (L.WZ_FP8, L.WZ_W4):
            o = rec["exp0"] = take(_pad8(4 * cout), what + " exponents")
            if raw is not None:
                rec["exps"] = np.frombuffer(raw, "<i4", cout, o)
        if kind == L.WZ_W4:
            o = rec["shift0"] = take(_pad8(n // 32), what + " group shifts")
            if raw is not None:
                rec["shifts"] = np.frombuffer(raw, "u1", n // 32, o)
                if int(rec["shifts"].max()) > _W4_SHIFT_MAX:
                    raise McamdError("%s: %s: a group shift byte of %d (0..%d)" % (path, what, int(rec["shifts"].max()), _W4_SHIFT_MAX))
        if kind == L.WZ_CODE:
            rec["code_bits"] = cbits
            o = take(_pad8(4 << cbits), what + " codebook")
            if raw is not None:
                rec["codebook"] = np.frombuffer(raw, "<f4", 1 << cbits, o)
        if bits:
            o = rec["word0"] = take(8 * ((n + 63) // 64), what + " bit words")
            if raw is not None:
                rec["words"] = np.frombuffer(raw, "<u8", (n + 63) // 64, o)
        stored = kept if bits else n
        if kind == L.WZ_CODE:
            width = code_width(cbits)
            nbytes = (stored * width + 7) // 8
            rec["val0"] = take(_pad8(nbytes), what + " codes")
            if raw is not None:
                rec["values"] = np.frombuffer(raw, "u1", nbytes, rec["val0"])
                rec["codes"] = _unpack_codes(rec["values"], width, stored)
                if stored and int(rec["codes"].max()) >= 1 << cbits:
                    raise McamdError("%s: %s: a code of %d with a codebook of %d entries" % (path, what, int(rec["codes"].max()),
                                                                                          1 << cbits))
        elif kind == L.WZ_W4:
            nbytes = (stored + 1) // 2
            rec["val0"] = take(_pad8(nbytes), what + " codes")
            if raw is not None:
                rec["values"] = np.frombuffer(raw, "u1", nbytes, rec["val0"])
                rec["codes"] = _unpack_codes(rec["values"], 4, stored)
                if stored % 2 and int(rec["values"][-1]) >> 4:
                    raise McamdError("%s: %s: the unused nibble behind the last code is not 0" % (path, what))
                # a kept weight has a non-zero grid index, every other stored code is +0
                if int(np.count_nonzero(rec["codes"] & 7)) != kept or bool((rec["codes"] == 8).any()):
                    raise McamdError("%s: %s: the codes stored do not hold the %d kept weights" % (path, what, kept))
        else:
            rec["val0"] = take(_pad8(stored * ELEM[kind]), what + " values")
            if raw is not None:
                rec["values"] = np.frombuffer(raw, _CODE_DTYPE[kind], stored, rec["val0"])
        rec["bytes"] = pos - start
        recs.append(rec)
    if pos != size:
        raise McamdError("%s: %d bytes behind the last record" % (path, size - pos))
    return dict(payload=KIND_NAMES[pay], seen=seen, records=recs, bytes=size, raw=raw)


def load_compressed(model, path, set_masks=True):
    """Fill `model` from an .mcz file: fp32 master weights (fp32 as is, fp16 widened, e4m3 as value 2^-exponent,
    4-bit codes as grid[code] 2^g 2^-e4_f), BatchNorm tensors, biases and `seen`.  Every record's shape is checked against
    the cfg before anything is written.  Returns the list of kept-bit masks (all ones for a record without a bitmask) and, when `set_masks` and at least one record has a
    bitmask, hands it to model.set_masks.  A "shared" file: the codes are widened on the host, expanded
    through the codebooks on the device (ops.WsTable.expand), and -- with `set_masks` -- the codebooks are set as
    Darknet.set_codebooks sets them, so that retraining and save_compressed(payload="shared") go on from the file."""
    convs = _conv_blocks(model)
    info = _parse(path)
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
    if all(conv.weight.is_cuda for _, conv, _ in convs):
        from . import ops
        dev = convs[0][1].weight.device
        items, shared = [], []
        buf = bytearray(info["raw"])
        for s, ((_, conv, _), rec) in enumerate(zip(convs, recs)):
            if conv.weight.dtype != torch.float32 or not conv.weight.data.is_contiguous():
                raise McamdError("compressed model files are read into contiguous fp32 master weights")
            masks.append(torch.empty_like(conv.weight.data))
            target, val0 = conv.weight.data, rec["val0"]
            if rec["kind"] == L.WZ_CODE:
                # one byte per code for the device pass, behind the file's own bytes (the sub-byte widening is a host pass)
                target, val0 = torch.empty(rec["shape"], dtype=torch.uint8, device=dev), len(buf)
                b = rec["codes"].tobytes()
                buf += b + b"\0" * (_pad8(len(b)) - len(b))
                shared.append(s)
                books[s] = (torch.from_numpy(rec["codebook"].astype(np.float32)).to(dev), target)
            if rec["kind"] == L.WZ_W4:               # one byte per code too; the exponents and shift bytes are read in place
                val0 = len(buf)
                b = rec["codes"].tobytes()
                buf += b + b"\0" * (_pad8(len(b)) - len(b))
            items.append(dict(w=target, mask=masks[-1], kind=rec["kind"], dense=not rec["bits"], kept=rec["kept"],
                              val0=val0, word0=rec["word0"] // 8, exp0=rec["exp0"] // 4, shift0=rec["shift0"] // 8))
        if len(buf) >= 1 << 33:
            raise McamdError("%s: a file of 8 GiB or more is not read on the device" % path)
        # the file's bytes go up once, as they are, and are expanded next to the weights: a record's bit words, exponents
        # and values are read in place (every array of the file starts at a multiple of 8 bytes)
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
    model._weights_dirty = True
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
    return dict(payload=info["payload"], seen=info["seen"], layers=layers, weights=sum(l["weights"] for l in layers),
                kept=sum(l["kept"] for l in layers), bytes=info["bytes"], dense_bytes=dense, ratio=dense / info["bytes"])
