"""The device passes of a Huffman-coded model file (csrc/huff.hip) through ops.hz_*: histogram = np.bincount,
chunk_bit0 and bits = the numpy restatement's (hz_ref.py) byte for byte, decode gives the symbols back, the same input twice
gives the same bytes, and a damaged stream raises its flag without a byte written outside its output range."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import compress, ops  # noqa: E402
import hz_ref  # noqa: E402

SIZES = [0, 1, 2, 1023, 1024, 1025, 3 * 1024 + 7, 200003]
FIB = [1, 1]
while len(FIB) < 30:
    FIB.append(FIB[-1] + FIB[-2])


def skewed(nsym, A, seed):
    return np.minimum(np.random.default_rng(seed).geometric(0.3, nsym) - 1, A - 1).astype(np.uint8)


def lengths_of(sy, A):
    return compress.huffman_lengths(np.bincount(sy, minlength=A)[:A])


def check_table(dev, streams, alphabets):
    """histogram, encode and decode of `streams` (numpy uint8 arrays) in ONE table against numpy and the restatement"""
    tensors = [torch.from_numpy(s).to(dev) for s in streams]
    hist = ops.hz_histogram(tensors).cpu().numpy()
    assert hist.shape == (len(streams), 256) and hist.dtype == np.int64
    for h, s in zip(hist, streams):
        assert np.array_equal(h, np.bincount(s, minlength=256))
    lengths = [lengths_of(s, A) for s, A in zip(streams, alphabets)]
    coded = ops.hz_encode(tensors, lengths, alphabets)
    again = ops.hz_encode(tensors, lengths, alphabets)
    for c, c2, s, l, A in zip(coded, again, streams, lengths, alphabets):
        nbits, chunk0, words = hz_ref.code_bits(s, l) if s.size else (0, np.zeros(0, "<u4"), np.zeros(0, "<u8"))
        assert c["nbits"] == nbits and c["nsym"] == s.size and c["A"] == A
        assert c["chunk_bit0"].cpu().numpy().view("<u4").tobytes() == chunk0.tobytes()
        assert c["bits"].cpu().numpy().view("<u8").tobytes() == words.tobytes()
        assert torch.equal(c["chunk_bit0"], c2["chunk_bit0"]) and torch.equal(c["bits"], c2["bits"])
    out, stats = ops.hz_decode(coded)
    assert not stats.cpu().numpy().any()
    for o, s in zip(out, streams):
        assert np.array_equal(o.cpu().numpy(), s)
    return coded


@pytest.mark.parametrize("A", [2, 16, 256])
def test_every_size_in_one_table(dev, A):
    check_table(dev, [skewed(n, A, seed=n + A) for n in SIZES], [A] * len(SIZES))


def test_alphabets_and_sizes_mixed_in_one_table(dev):
    alphabets = [256, 2, 16, 12, 256, 16, 2]
    sizes = [70001, 5, 1025, 4096, 0, 2047, 131072 + 3]
    streams = [skewed(n, A, seed=3 * n + A) for n, A in zip(sizes, alphabets)]
    streams[3] = np.full(4096, 7, dtype=np.uint8)            # a single symbol: length 1, code 0
    coded = check_table(dev, streams, alphabets)
    assert coded[3]["nbits"] == 4096 and not coded[3]["bits"].cpu().numpy().any()


def test_length_12_codes_across_word_and_chunk_boundaries(dev):
    """The Fibonacci histogram as a stream: its unlimited code is 29 deep, so the limit binds and 12-bit codes occur; about
    2 10^6 symbols put them across word and chunk boundaries."""
    sy = np.repeat(np.arange(30, dtype=np.uint8), FIB)
    assert sy.size == sum(FIB) > 2_000_000
    np.random.default_rng(5).shuffle(sy)
    lengths = lengths_of(sy, 30)
    assert int(lengths.max()) == 12
    for i, t in zip(np.flatnonzero(lengths[sy] == 12)[:4], (1023, 1024, 5 * 1024 - 1, 5 * 1024)):      # at chunk ends and starts
        sy[i], sy[t] = sy[t], sy[i]
    coded = check_table(dev, [sy], [30])[0]
    lens = lengths.astype(np.int64)[sy]
    starts = np.cumsum(lens) - lens
    long = lens == 12
    assert (long & (starts % 64 > 52)).any(), "a 12-bit code straddles two words"
    assert (lens[1023::1024] == 12).any() and (lens[1024::1024] == 12).any()      # 12-bit codes end and begin chunks
    assert coded["nbits"] == int(lens.sum())


def damaged(dev, coded, streams, how):
    """Decode three streams, the middle one damaged, into a buffer of canaries; -> (stats, buffer, offsets)"""
    gap = 64
    offsets, total = [], gap
    for s in streams:
        offsets.append(total)
        total += (s.size + 7) // 8 * 8 + gap
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    coded = [dict(c) for c in coded]
    how(coded[1])
    got, stats = ops.hz_decode(coded, out=out, offsets=offsets)
    host, stats = out.cpu().numpy(), stats.cpu().numpy()
    for k in (0, 2):                                         # the neighbours decode, unflagged
        assert np.array_equal(got[k].cpu().numpy(), streams[k]) and stats[k, 0] == 0
    assert stats[1, 0] & 1, "the damaged stream raises its flag"
    keep = np.ones(total, dtype=bool)
    for o, s in zip(offsets, streams):
        keep[o:o + s.size] = False
    assert (host[keep] == 0xA5).all(), "a byte outside the output ranges was written"
    return host[offsets[1]:offsets[1] + streams[1].size]


def test_a_damaged_stream_raises_its_flag_and_stays_inside_its_output(dev):
    """Bounds on a well-formed call: every address the kernel may use lies inside buffers this test owns."""
    streams = [skewed(5000, 256, 1), skewed(6 * 1024 + 100, 256, 2), skewed(3000, 16, 3)]
    alphabets = [256, 256, 16]
    tensors = [torch.from_numpy(s).to(dev) for s in streams]
    lengths = [lengths_of(s, A) for s, A in zip(streams, alphabets)]
    coded = ops.hz_encode(tensors, lengths, alphabets)
    c = coded[1]
    chunk0 = c["chunk_bit0"].cpu().numpy().view("<u4").copy()
    words = c["bits"].cpu().numpy().view("<u8").copy()

    # one flipped bit (a prefix code can fall back into step: a flip is taken that the restatement's reader rejects)
    for p in range(int(chunk0[3]) - 1, int(chunk0[3]) - 200, -1):
        bad = words.copy()
        bad[p // 64] ^= np.uint64(1) << np.uint64(p % 64)
        try:
            hz_ref.decode_bits(lengths[1], streams[1].size, c["nbits"], chunk0, bad)
        except AssertionError:
            break
    else:
        raise AssertionError("no flipped bit breaks the chunk")

    def flip(d):
        d["bits"] = torch.from_numpy(bad.view(np.int64)).to(dev)

    part = damaged(dev, coded, streams, flip)
    good = np.ones(streams[1].size, dtype=bool)
    good[2048:3072] = False                                  # chunk 2 holds the flip; every other chunk decodes
    assert np.array_equal(part[good], streams[1][good])

    def move(d):
        t = chunk0.copy()
        t[2] += 1
        d["chunk_bit0"] = torch.from_numpy(t.view(np.int32)).to(dev)

    damaged(dev, coded, streams, move)

    def shorten(d):
        d["nbits"] = c["nbits"] - 1

    part = damaged(dev, coded, streams, shorten)
    assert np.array_equal(part[:6 * 1024], streams[1][:6 * 1024])      # only the last chunk cannot end at nbits

    def unassigned(d):                                       # a single-symbol code: the other 1-bit code is unassigned
        d["lengths"] = np.eye(1, 256, 9, dtype=np.uint8)[0]
        d["A"] = 256

    damaged(dev, coded, streams, unassigned)


def test_population_counts_of_decoded_bit_words(dev):
    rng = np.random.default_rng(9)
    n = 64 * 300 - 17                                        # the last word has 17 tail bits
    keep = rng.random(n) < 0.2
    words = np.packbits(np.concatenate([keep, np.zeros(17, dtype=bool)]), bitorder="little")
    t = [torch.from_numpy(words).to(dev)]
    coded = ops.hz_encode(t, [lengths_of(words, 256)])
    coded[0]["popc_bits"] = n
    out, stats = ops.hz_decode(coded)
    assert stats.cpu().numpy().tolist() == [[0, int(keep.sum())]] and np.array_equal(out[0].cpu().numpy(), words)
    tail = words.copy()
    tail[-1] |= 0x80                                         # a bit behind the last weight
    coded = ops.hz_encode([torch.from_numpy(tail).to(dev)], [lengths_of(tail, 256)])
    coded[0]["popc_bits"] = n
    _, stats = ops.hz_decode(coded)
    assert stats.cpu().numpy().tolist() == [[2, int(keep.sum())]]
