"""Compressed model files (.mcz; an addition beyond the reference, DESIGN.md 3s, include/mcamd.h).

A Darknet .weights file stores every conv weight as a dense float32, zeros included.  An .mcz file stores, per conv block,
a bitmask of the non-zero weights and only those weights, as fp32, fp16 or e4m3 codes -- exactly what the engine the file
is written for consumes, so the file is lossless for that engine:

    save_compressed(model, path, payload="fp16", layers=None)
    load_compressed(model, path, set_masks=True) -> masks
    compressed_info(path) -> dict

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
PAYLOADS = {"fp32": L.WZ_FP32, "fp16": L.WZ_FP16, "fp8": L.WZ_FP8}
KIND_NAMES = {v: k for k, v in PAYLOADS.items()}
ELEM = {L.WZ_FP32: 4, L.WZ_FP16: 2, L.WZ_FP8: 1}
_CODE_DTYPE = {L.WZ_FP32: "<u4", L.WZ_FP16: "<u2", L.WZ_FP8: "u1"}
_MAG_BITS = {L.WZ_FP32: 0x7FFFFFFF, L.WZ_FP16: 0x7FFF, L.WZ_FP8: 0x7F}
_HEADER = struct.Struct("<4sIIIq")          # magic, version, payload, records, seen
_RECORD = struct.Struct("<4iIIQ")           # cout, cin, kh, kw, flags, 0, kept


def _pad8(nbytes):
    return (nbytes + 7) // 8 * 8


def has_bits(n, kept, kind):
    """The bitmask-or-dense rule: a record carries bit words only when that is smaller."""
    return 8 * ((n + 63) // 64) + kept * ELEM[kind] < n * ELEM[kind]


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


def _encode_cpu(w, mask, kind):
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
    return dict(kept=kept, exps=exps, words=words, values=np.ascontiguousarray(values))


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
    if rec["words"] is not None:
        bits = np.unpackbits(rec["words"].view(np.uint8), bitorder="little")
        keep = bits[:n].astype(bool)
        codes = np.zeros(n, dtype=dt)
        codes[keep] = rec["values"]
        mask = keep.astype(np.float32)
    else:
        codes = rec["values"]
        mask = np.ones(n, dtype=np.float32)
    nz = (codes & dt.type(_MAG_BITS[kind])) != 0
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
    if kind != L.WZ_FP8:
        return convs, [kind] * len(convs)
    chosen = set(default_fp8_layers(model) if layers is None else [int(i) for i in layers])
    bad = sorted(chosen - set(i for i, _, _ in convs))
    if bad:
        raise McamdError("layers names conv numbers the model does not have: %r" % bad)
    # every other layer of an fp8 file is what the "fp8" engine runs there: fp16
    return convs, [L.WZ_FP8 if i in chosen else L.WZ_FP16 for i, _, _ in convs]


def _mask_of(conv):
    return conv.mask if getattr(conv, "mask_flag", False) else None


def _encode_device(convs, kinds):
    """The device path: every layer through one ops.wz_pack table, one host read of counts, words, exponents and values."""
    from . import ops
    items = []
    for (_, conv, _), kind in zip(convs, kinds):
        w, m = conv.weight.data, _mask_of(conv)
        if w.dtype != torch.float32:
            raise McamdError("compressed model files are written from fp32 master weights")
        items.append(dict(w=w.contiguous(), mask=m.contiguous().float() if m is not None else None, kind=kind))
    words, counts, exps, values = ops.wz_pack(items)
    counts = [int(c) for c in counts.cpu().numpy().view("<u8")]                # the one synchronising read
    words, exps = words.cpu().numpy().view("<u8"), exps.cpu().numpy().astype("<i4", copy=False)
    sizes = []
    for it, kind, kept in zip(items, kinds, counts):
        n = it["w"].numel()
        sizes.append((kept if has_bits(n, kept, kind) else n) * ELEM[kind])
    values = values[:sum(_pad8(s) for s in sizes)].cpu().numpy()
    out, w0, e0, v0 = [], 0, 0, 0
    for it, kind, kept, size in zip(items, kinds, counts, sizes):
        n, cout = it["w"].numel(), it["w"].shape[0]
        nwords = (n + 63) // 64
        rec = dict(kept=kept, exps=None, words=None, values=values[v0:v0 + size].view(_CODE_DTYPE[kind]))
        if has_bits(n, kept, kind):
            rec["words"] = words[w0:w0 + nwords]
        if kind == L.WZ_FP8:
            rec["exps"] = exps[e0:e0 + cout]
            e0 += cout
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
    consume) or "fp8" (the conv numbers in `layers` as e4m3 codes + one exponent per filter, every other layer as fp16;
    `layers` defaults to default_fp8_layers(model), pass Engine.fp8_layers to be exact for any cfg).  A weight is stored
    iff its value in the payload is non-zero."""
    convs, kinds = _kinds(model, payload, layers)
    if not convs:
        raise McamdError("the model has no convolutional block to store")
    if all(conv.weight.is_cuda for _, conv, _ in convs):
        encoded = _encode_device(convs, kinds)
    else:
        encoded = [_encode_cpu(conv.weight.data.cpu(), (_mask_of(conv).cpu() if _mask_of(conv) is not None else None), kind)
                   for (_, conv, _), kind in zip(convs, kinds)]
    with open(path, "wb") as f:
        f.write(_HEADER.pack(MAGIC, VERSION, PAYLOADS[payload], len(convs), int(model.seen)))
        for (_, conv, bn), kind, rec in zip(convs, kinds, encoded):
            cout, cin, kh, kw = conv.weight.shape
            flags = (L.WZ_F_BN if bn is not None else 0) | (L.WZ_F_BITS if rec["words"] is not None else 0) | (kind << 8)
            f.write(_RECORD.pack(cout, cin, kh, kw, flags, 0, rec["kept"]))
            for a in _small_arrays(conv, bn):
                _write_array(f, a)
            if kind == L.WZ_FP8:
                _write_array(f, rec["exps"].astype("<i4", copy=False))
            if rec["words"] is not None:
                _write_array(f, rec["words"])
            _write_array(f, rec["values"])


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
        cout, cin, kh, kw, flags, _, kept = _RECORD.unpack(head(_RECORD.size, what))
        kind = (flags >> 8) & 0xFF
        if min(cout, cin, kh, kw) <= 0 or kind not in KIND_NAMES or flags & ~(0xFF00 | L.WZ_F_BN | L.WZ_F_BITS):
            raise McamdError("%s: %s: damaged record header" % (path, what))
        n = cout * cin * kh * kw
        bits = bool(flags & L.WZ_F_BITS)
        if kept > n or bits != has_bits(n, kept, kind):
            raise McamdError("%s: %s: damaged record header (kept %d of %d weights)" % (path, what, kept, n))
        rec = dict(shape=(cout, cin, kh, kw), cout=cout, n=n, bn=bool(flags & L.WZ_F_BN), bits=bits, kind=kind, kept=kept,
                   small=[], exps=None, words=None, values=None, exp0=0, word0=0)
        for _ in range(4 if rec["bn"] else 1):
            o = take(_pad8(4 * cout), what + " per-channel arrays")
            if raw is not None:
                rec["small"].append(np.frombuffer(raw, "<f4", cout, o))
        if kind == L.WZ_FP8:
            o = rec["exp0"] = take(_pad8(4 * cout), what + " exponents")
            if raw is not None:
                rec["exps"] = np.frombuffer(raw, "<i4", cout, o)
        if bits:
            o = rec["word0"] = take(8 * ((n + 63) // 64), what + " bit words")
            if raw is not None:
                rec["words"] = np.frombuffer(raw, "<u8", (n + 63) // 64, o)
        stored = kept if bits else n
        rec["val0"] = take(_pad8(stored * ELEM[kind]), what + " values")
        if raw is not None:
            rec["values"] = np.frombuffer(raw, _CODE_DTYPE[kind], stored, rec["val0"])
        rec["bytes"] = pos - start
        recs.append(rec)
    if pos != size:
        raise McamdError("%s: %d bytes behind the last record" % (path, size - pos))
    return dict(payload=KIND_NAMES[pay], seen=seen, records=recs, bytes=size, raw=raw)


def load_compressed(model, path, set_masks=True):
    """Fill `model` from an .mcz file: fp32 master weights (fp32 as is, fp16 widened, e4m3 as value 2^-exponent), BatchNorm
    tensors, biases and `seen`.  Every record's shape is checked against the cfg before anything is written.  Returns the
    list of kept-bit masks (all ones for a record without a bitmask) and, when `set_masks` and at least one record has a
    bitmask, hands it to model.set_masks."""
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
    masks = []
    if all(conv.weight.is_cuda for _, conv, _ in convs):
        from . import ops
        dev = convs[0][1].weight.device
        items = []
        for (_, conv, _), rec in zip(convs, recs):
            if conv.weight.dtype != torch.float32 or not conv.weight.data.is_contiguous():
                raise McamdError("compressed model files are read into contiguous fp32 master weights")
            masks.append(torch.empty_like(conv.weight.data))
            items.append(dict(w=conv.weight.data, mask=masks[-1], kind=rec["kind"], dense=not rec["bits"], kept=rec["kept"],
                              val0=rec["val0"], word0=rec["word0"] // 8, exp0=rec["exp0"] // 4))
        if info["bytes"] >= 1 << 33:
            raise McamdError("%s: a file of 8 GiB or more is not read on the device" % path)
        # the file's bytes go up once, as they are, and are expanded next to the weights: a record's bit words, exponents
        # and values are read in place (every array of the file starts at a multiple of 8 bytes)
        values = torch.frombuffer(bytearray(info["raw"]), dtype=torch.uint8).to(dev)
        words, exps = values.view(torch.int64), values.view(torch.int32)
        ops.wz_unpack(items, words, exps, values)
    else:
        for (i, conv, _), rec in zip(convs, recs):
            w, m = _decode_cpu(rec, "%s: conv%d" % (path, i))
            conv.weight.data.copy_(torch.from_numpy(w).view(rec["shape"]))
            masks.append(torch.from_numpy(m).view(rec["shape"]).to(conv.weight.device))
    for (_, conv, bn), rec in zip(convs, recs):
        for t, a in zip(_small_targets(conv, bn), rec["small"]):
            t.copy_(torch.from_numpy(a.astype(np.float32)))
    model.seen = int(info["seen"])
    model._weights_dirty = True
    if set_masks and any(rec["bits"] for rec in recs):
        model.set_masks(masks)
    return masks


def compressed_info(path):
    """What an .mcz file holds, from its header and record headers alone (no GPU, no model): per conv its shape, value
    kind, kept count and bytes; the totals; and the ratio against the dense float32 .weights file of the same cfg."""
    info = _parse(path, payload=False)
    layers, dense = [], 16
    for i, rec in enumerate(info["records"]):
        layers.append(dict(conv=i + 1, shape=rec["shape"], kind=KIND_NAMES[rec["kind"]], bitmask=rec["bits"], kept=rec["kept"],
                           weights=rec["n"], bytes=rec["bytes"]))
        dense += 4 * (rec["n"] + rec["cout"] * (4 if rec["bn"] else 1))
    return dict(payload=info["payload"], seen=info["seen"], layers=layers, weights=sum(l["weights"] for l in layers),
                kept=sum(l["kept"] for l in layers), bytes=info["bytes"], dense_bytes=dense, ratio=dense / info["bytes"])
