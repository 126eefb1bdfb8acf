"""Numpy restatement of the Huffman-coded model file ("MCZH"), written from DESIGN.md 3z and include/mcamd.h; test-side only.
It writes and reads whole files on its own: encode_file turns the bytes of an "MCZW" file into its coded twin, decode_file
turns them back.  The code lengths alone come from the project (compress.huffman_lengths, THE one source of them; the file
stores them, so reading needs nothing from the project).

  file     "MCZH", uint32 version 1, then payload, records, seen and the records as in "MCZW"
  record   the 32-byte header, per-channel arrays, exponents (fp8, w4) and codebook (codes) byte for byte; in place of the
           shift bytes (w4, alphabet 12), the bit words (as bytes, 256) and the values (e4m3 bytes 256, one symbol per code
           2^bits, one symbol per nibble 16) a STREAM; fp16 / fp32 values stay raw
  stream   uint32 mode, uint32 A, uint64 nsym; mode 0: the array as "MCZW" has it; mode 1: uint64 nbits, uint8 length[A],
           uint32 chunk_bit0[ceil(nsym / 1024)], uint64 bits[ceil(nbits / 64)], every array zero-padded to 8 bytes
  codes    canonical (RFC 1951 3.2.2), most significant bit first into successive positions, position p = bit p % 64 of
           word p / 64; mode 1 iff its body is strictly smaller than the mode-0 body and nbits < 2^32
"""
import struct

import numpy as np

FP32, FP16, FP8, CODE, W4 = 0, 1, 2, 4, 5
ELEM = {FP32: 4, FP16: 2, FP8: 1}
CHUNK, MAXLEN = 1024, 12


def pad8(b):
    return b + b"\0" * (-len(b) % 8)


def up8(n):
    return -(-n // 8) * 8


def project_lengths(counts):
    from modelcompression_amd import compress
    return compress.huffman_lengths(counts)


def canonical(lengths):
    """code values: symbols with a non-zero length in (length, symbol) order take increasing values"""
    lengths = [int(l) for l in lengths]
    codes, code, prev = [0] * len(lengths), 0, 0
    for l, a in sorted((l, a) for a, l in enumerate(lengths) if l):
        code <<= l - prev
        codes[a], code, prev = code, code + 1, l
    return np.array(codes, dtype=np.int64)


def code_bits(symbols, lengths):
    """(nbits, chunk_bit0 <u4, words <u8): every code's bits, most significant first, one after the other."""
    lengths = np.asarray(lengths, dtype=np.int64)
    lens, codes = lengths.astype(np.int32)[symbols], canonical(lengths).astype(np.int32)[symbols]
    col = np.arange(MAXLEN, dtype=np.int32)
    rows = (codes[:, None] >> np.maximum(lens[:, None] - 1 - col, 0)) & 1          # bit j of a code = its bit len - 1 - j
    seq = rows[col < lens[:, None]].astype(np.uint8)                               # row-major: the codes in order
    nbits = int(lens.sum(dtype=np.int64))
    assert seq.size == nbits
    starts = np.cumsum(lens, dtype=np.int64) - lens
    words = np.packbits(np.concatenate([seq, np.zeros(-nbits % 64, dtype=np.uint8)]), bitorder="little").view("<u8")
    return nbits, starts[::CHUNK].astype("<u4"), words


def stream_bytes(symbols, A, raw, lengths_of=project_lengths):
    """One stream: `symbols` uint8, `raw` the array as the "MCZW" file stores it (bytes, unpadded)."""
    symbols = np.asarray(symbols, dtype=np.uint8).reshape(-1)
    nsym, body0 = symbols.size, pad8(raw)
    plain = struct.pack("<IIQ", 0, A, nsym) + body0
    if nsym == 0:
        return plain
    lengths = np.asarray(lengths_of(np.bincount(symbols, minlength=A)[:A]), dtype=np.uint8)
    nbits, chunk0, words = code_bits(symbols, lengths)
    body1 = struct.pack("<Q", nbits) + pad8(lengths.tobytes()) + pad8(chunk0.tobytes()) + words.tobytes()
    if len(body1) < len(body0) and nbits < 1 << 32:
        return struct.pack("<IIQ", 1, A, nsym) + body1
    return plain


def decode_bits(lengths, nsym, nbits, chunk0, words):
    """The symbols: every chunk reads its codes bit by bit (first-code arithmetic), all chunks in step."""
    lengths = np.asarray(lengths, dtype=np.int64)
    order = sorted((int(l), a) for a, l in enumerate(lengths) if l)
    syms = np.array([a for _, a in order], dtype=np.uint8)
    count = np.bincount(lengths, minlength=MAXLEN + 2)
    count[0] = 0
    first, offs, code, o = [0] * (MAXLEN + 1), [0] * (MAXLEN + 1), 0, 0
    for l in range(1, MAXLEN + 1):
        code = (code + int(count[l - 1])) << 1
        first[l], offs[l] = code, o
        o += int(count[l])
    bit = np.concatenate([np.unpackbits(words.view(np.uint8), bitorder="little")[:nbits], np.zeros(MAXLEN + 1, dtype=np.uint8)])
    bit = bit.astype(np.int64)
    nchunks = -(-nsym // CHUNK)
    pos = chunk0.astype(np.int64)
    end = np.append(pos[1:], nbits)
    out = np.zeros((nchunks, CHUNK), dtype=np.uint8)
    todo = np.minimum(CHUNK, nsym - CHUNK * np.arange(nchunks))
    for i in range(min(CHUNK, nsym)):
        live = np.flatnonzero(todo > i)
        p, acc = pos[live], np.zeros(live.size, dtype=np.int64)
        got = np.zeros(live.size, dtype=bool)
        for l in range(1, MAXLEN + 1):
            acc = np.where(got, acc, acc << 1 | bit[np.minimum(p + l - 1, nbits)])
            hit = ~got & (acc >= first[l]) & (acc - first[l] < count[l])
            out[live[hit], i] = syms[offs[l] + acc[hit] - first[l]]
            pos[live[hit]] += l
            got |= hit
            if got.all():
                break
        assert got.all(), "an unassigned code"
    assert (pos == end).all(), "a chunk does not end where the next begins"
    return out.reshape(-1)[:nsym]


def read_stream(data, pos, A, nsym, raw_bytes):
    """-> (symbols or None, raw array bytes or None, new pos); exactly one of the two is given"""
    mode, a, n = struct.unpack_from("<IIQ", data, pos)
    assert mode in (0, 1) and a == A and n == nsym
    pos += 16
    if mode == 0:
        return None, data[pos:pos + raw_bytes], pos + up8(raw_bytes)
    nbits, = struct.unpack_from("<Q", data, pos)
    pos += 8
    lengths = np.frombuffer(data, "u1", A, pos)
    pos += up8(A)
    nchunks = -(-nsym // CHUNK)
    chunk0 = np.frombuffer(data, "<u4", nchunks, pos)
    pos += up8(4 * nchunks)
    words = np.frombuffer(data, "<u8", -(-nbits // 64), pos)
    pos += words.nbytes
    assert lengths.max() <= MAXLEN
    used = lengths[lengths > 0].astype(np.int64)
    assert int((1 << (MAXLEN - used)).sum()) == (1 << MAXLEN - 1 if used.size == 1 else 1 << MAXLEN)
    return decode_bits(lengths, nsym, nbits, chunk0, words), None, pos


def pack_codes(codes, width):
    per = 8 // width
    padded = np.concatenate([codes, np.zeros(-codes.size % per, dtype=np.uint8)]).reshape(-1, per).astype(np.uint32)
    return (padded << (width * np.arange(per, dtype=np.uint32))).sum(axis=1).astype(np.uint8)


def unpack_codes(packed, width, count):
    per = 8 // width
    return ((packed[:, None] >> (width * np.arange(per, dtype=np.uint8))) & ((1 << width) - 1)).astype(np.uint8).reshape(-1)[:count]


def _walk(data, coded, emit):
    """Both directions: walk the records of a file (`coded`: an "MCZH" file) and rebuild the other container through `emit`."""
    magic, version, payload, nrec, seen = struct.unpack_from("<4sIIIq", data, 0)
    assert magic == (b"MCZH" if coded else b"MCZW") and version == 1
    out = [struct.pack("<4sIIIq", b"MCZW" if coded else b"MCZH", 1, payload, nrec, seen)]
    pos, streams = 24, 0
    for _ in range(nrec):
        cout, cin, kh, kw, flags, bits, kept = struct.unpack_from("<4iIIQ", data, pos)
        kind, n = flags >> 8, cout * cin * kh * kw
        keep = 32 + (4 if flags & 1 else 1) * up8(4 * cout) + (up8(4 * cout) if kind in (FP8, W4) else 0)

        def symbols_array(A, nsym, raw_bytes, to_raw, to_symbols):
            """one uint8-symbol array: read it in this container, write it in the other"""
            nonlocal pos, streams
            streams += 1
            if coded:
                sy, raw, pos = read_stream(data, pos, A, nsym, raw_bytes)
                out.append(pad8(bytes(raw) if raw is not None else to_raw(sy)))
            else:
                raw = data[pos:pos + raw_bytes]
                pos += up8(raw_bytes)
                out.append(emit(to_symbols(np.frombuffer(raw, "u1")), A, raw))

        out.append(data[pos:pos + keep])
        pos += keep
        same = lambda a: a.tobytes() if hasattr(a, "tobytes") else a
        if kind == W4:
            symbols_array(12, n // 32, n // 32, same, lambda a: a)
        if kind == CODE:
            out.append(data[pos:pos + up8(4 << bits)])
            pos += up8(4 << bits)
        if flags & 2:
            symbols_array(256, 8 * -(-n // 64), 8 * -(-n // 64), same, lambda a: a)
        stored = kept if flags & 2 else n
        if kind in (FP16, FP32):
            size = up8(stored * ELEM[kind])
            out.append(data[pos:pos + size])
            pos += size
        elif kind == FP8:
            symbols_array(256, stored, stored, same, lambda a: a)
        else:
            width = 4 if kind == W4 else next(w for w in (1, 2, 4, 8) if w >= bits)
            A = 16 if kind == W4 else 1 << bits
            symbols_array(A, stored, (stored * width + 7) // 8, lambda sy: pack_codes(sy, width).tobytes(),
                          lambda a: unpack_codes(a, width, stored))
    assert pos == len(data)
    return b"".join(out), streams


def encode_file(plain, lengths_of=project_lengths):
    """bytes of an "MCZW" file -> bytes of its "MCZH" twin"""
    return _walk(plain, False, lambda sy, A, raw: stream_bytes(sy, A, raw, lengths_of))[0]


def decode_file(coded):
    """bytes of an "MCZH" file -> bytes of its "MCZW" twin"""
    return _walk(coded, True, None)[0]


def count_streams(plain):
    return _walk(plain, False, lambda sy, A, raw: b"")[1]
