"""csrc/wpack.hip on MCAMD_WZ_W4 segments: ops.wz_pack / ops.wz_unpack against the numpy restatement (wz_w4_ref.py) and against
the engine's own packer (ops.pack_q8_w4 read back through w4_ref), byte for byte -- bit words, kept counts, exponents, shift
bytes and code bytes, each shape alone and all of them in one table between fp16 and fp8 segments; unpacked masters and
masks by bit pattern; the same input twice gives the same bytes; a damaged record reads +0 inside its buffers.

  (5, 32, 1, 1)    160 weights: a ragged last word, one group per filter
  (3, 64, 3, 3)    27 words: a group is 32 weights strided by 9
  (70, 64, 3, 3)   630 words: 10 workgroups, filter boundaries inside a workgroup's range"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import _lib, ops  # noqa: E402
import w4_ref  # noqa: E402
import wz_ref  # noqa: E402
import wz_w4_ref  # noqa: E402

SHAPES = [(5, 32, 1, 1), (3, 64, 3, 3), (70, 64, 3, 3)]
MASKS = ["none", "random80", "2:4"]
W4 = _lib.WZ_W4


def weights(shape, seed):
    """fp32 OIHW weights with a scale of their own per filter, a few far below it (zero codes) and, with more than one group per
    filter, one group at 2^-20 of its filter's scale (clamped at g = -5) and one all-zero group."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g) * torch.pow(2.0, torch.randint(-6, 7, (shape[0], 1, 1, 1), generator=g).float())
    flat = w.view(-1)
    flat[torch.randperm(flat.numel(), generator=g)[:max(1, flat.numel() // 50)]] = 1e-9
    if shape[1] > 32:
        w[1, 32:64, 0, 0] *= 2.0 ** -20
        w[2, :32, 0, 0] = 0.0
    return w


def mask_of(name, shape, seed):
    g = torch.Generator().manual_seed(seed + 77)
    if name == "none":
        return None
    if name == "random80":
        return (torch.rand(shape, generator=g) >= 0.8).float()
    O, I, kh, kw = shape
    order = torch.rand(O, I // 4, 4, kh, kw, generator=g).argsort(dim=2)
    return (order < 2).float().view(shape)


@pytest.fixture(scope="module")
def layers():
    """{(shape, mask name): (w, mask, wz_w4_ref.encode_layer)}, computed once and left unchanged"""
    out = {}
    for si, shape in enumerate(SHAPES):
        for mi, name in enumerate(MASKS):
            w, m = weights(shape, 10 * si + mi), mask_of(name, shape, 10 * si + mi)
            out[shape, name] = (w, m, wz_w4_ref.encode_layer(w, m))
    return out


def pack(table, dev):
    items = [dict(w=w.to(dev), mask=(m.to(dev) if m is not None else None), kind=k) for w, m, k in table]
    out = ops.wz_pack(items)
    torch.cuda.synchronize()
    words, counts, exps, values = out[:4]
    shifts = out[4].cpu().numpy() if len(out) > 4 else np.zeros(0, dtype=np.uint8)
    return words.cpu().numpy().view("<u8"), counts.cpu().numpy().view("<u8"), exps.cpu().numpy(), values.cpu().numpy(), shifts


def encode(w, m, k, enc=None):
    return (enc or wz_w4_ref.encode_layer(w, m)) if k == W4 else wz_ref.encode_layer(w, m, k)


def check_pack(table, encs, dev):
    """Every output of one ops.wz_pack call against the restatements."""
    words, counts, exps, values, shifts = pack(table, dev)
    w0 = e0 = v0 = s0 = 0
    for s, ((w, m, k), enc) in enumerate(zip(table, encs)):
        n, nwords, what = w.numel(), -(-w.numel() // 64), (s, tuple(w.shape), k)
        assert int(counts[s]) == enc["kept"], what
        assert words[w0:w0 + nwords].tobytes() == enc["all_words"].tobytes(), what
        w0 += nwords
        if k in (wz_ref.FP8, W4):
            assert exps[e0:e0 + w.shape[0]].tobytes() == (enc["e4"] if k == W4 else enc["exps"]).tobytes(), what
            e0 += w.shape[0]
        if k == W4:
            assert shifts[s0:s0 + n // 32].tobytes() == enc["shifts"].tobytes(), what
            assert not shifts[s0 + n // 32:s0 + wz_w4_ref.up8(n // 32)].any(), what
            s0 += wz_w4_ref.up8(n // 32)
            want = wz_ref.pad8(enc["stored"].tobytes())                  # one byte per code in the pass
        else:
            want = wz_ref.pad8(enc["values"].tobytes())
        assert values[v0:v0 + len(want)].tobytes() == want, what
        v0 += len(want)
    assert w0 == words.size and e0 == exps.size and s0 == shifts.size and not values[v0:].any()


def check_unpack(table, encs, dev, want_masks=True):
    """ops.wz_unpack of the RESTATEMENT's arrays, laid out as a file lays them out (one buffer serves as words, exponents, shift
    bytes and values), against the restatement's decoder, by bit pattern."""
    buf, items, outs = b"", [], []
    for (w, m, k), enc in zip(table, encs):
        out_w = torch.full(w.shape, float("nan"), device=dev)
        out_m = torch.full(w.shape, float("nan"), device=dev) if want_masks else None
        outs.append((out_w, out_m))
        it = dict(w=out_w, mask=out_m, kind=k, dense=enc["words"] is None, kept=enc["kept"])
        if k in (wz_ref.FP8, W4):
            it["exp0"] = len(buf) // 4
            buf += wz_ref.pad8((enc["e4"] if k == W4 else enc["exps"]).tobytes())
        if k == W4:
            it["shift0"] = len(buf) // 8
            buf += wz_ref.pad8(enc["shifts"].tobytes())
        it["word0"] = len(buf) // 8
        if enc["words"] is not None:
            buf += enc["words"].tobytes()
        it["val0"] = len(buf)
        buf += wz_ref.pad8((enc["stored"] if k == W4 else enc["values"]).tobytes())
        items.append(it)
    raw = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
    ops.wz_unpack(items, raw.view(torch.int64), raw.view(torch.int32), raw, raw)
    for (w, m, k), enc, (out_w, out_m) in zip(table, encs, outs):
        if k == W4:
            ref_w, ref_m = wz_w4_ref.decode(dict(shape=tuple(w.shape), kind=W4, kept=enc["kept"], e4=enc["e4"], shifts=enc["shifts"],
                                                 words=enc["words"], codes=enc["stored"]))
            assert torch.equal(torch.from_numpy(ref_w), enc["masters"]), "the restatement's decoder is w4_ref.dequantised"
        else:
            ref_w, ref_m = wz_ref.decode(dict(shape=tuple(w.shape), kind=k, kept=enc["kept"], exps=enc["exps"], words=enc["words"],
                                              values=enc["values"]))
        assert out_w.cpu().numpy().view("<u4").tobytes() == ref_w.view("<u4").tobytes(), (w.shape, k)
        if want_masks:
            assert out_m.cpu().numpy().view("<u4").tobytes() == ref_m.view("<u4").tobytes(), (w.shape, k)


@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_each_shape_alone(dev, layers, shape, mask_name):
    w, m, enc = layers[shape, mask_name]
    check_pack([(w, m, W4)], [enc], dev)
    check_unpack([(w, m, W4)], [enc], dev)
    assert (enc["words"] is None) == (mask_name == "none"), "a dense layer stores all n nibbles, a pruned one bit words"


@pytest.mark.parametrize("shape", SHAPES[1:], ids=str)
@pytest.mark.parametrize("mask_name", MASKS)
def test_codes_shifts_and_exponents_are_the_engine_packers(dev, layers, shape, mask_name):
    """The same weights through ops.pack_q8_w4 (the "fp8-w4" engine's packer, cin % 64 == 0), its tile layout undone by w4_ref,
    against what ops.wz_pack computed: one rule, two layouts.  The engine's forms need cout % 8 == 0: its packer gets the
    same filters followed by all-zero ones (a filter's codes, shifts and exponent depend on that filter alone)."""
    w, m, enc = layers[shape, mask_name]
    cout, cin, k, _ = shape
    cout8 = ops.round_up(cout, 8)
    g = ops.geom(1, 8, 8, k, cin, cout8, cin)
    w8 = torch.cat([w, torch.zeros(cout8 - cout, cin, k, k)])
    m8 = torch.cat([m, torch.ones(cout8 - cout, cin, k, k)]) if m is not None else None
    codes, gshift, wexp = ops.pack_q8_w4(g, w8.to(dev).contiguous(), m8.to(dev).contiguous() if m8 is not None else None)
    words, counts, exps, values, shifts = pack([(w, m, W4)], dev)
    npad, ktot = ops.round_up(cout, 256), cin * k * k
    assert torch.equal(wexp.cpu()[:cout], torch.from_numpy(exps.astype(np.int32)))
    g_file = torch.from_numpy(shifts[:w.numel() // 32].astype(np.int64)).view(cout, cin // 32, k, k) - 5
    assert torch.equal(gshift.cpu().view(ktot // 64, npad, 2)[:, :cout], w4_ref.shift_rows(g_file))
    full = torch.from_numpy(enc["codes"].copy()).view(shape)                 # (the pass's bytes are checked against these above)
    assert torch.equal(w4_ref.codes_of_rows(codes.cpu().view(npad, ktot // 2)[:cout], cin, k), w4_ref.dense_rows(full))
    kept = np.unpackbits(words.view(np.uint8), bitorder="little")[:w.numel()].astype(bool)
    stored = values[:int(counts[0])] if enc["words"] is not None else values[:w.numel()][kept]
    assert stored.tobytes() == enc["codes"][kept].tobytes()


def mixed_table(layers):
    """all three shapes under all three masks, between fp16 and fp8 segments of shapes of their own"""
    g = torch.Generator().manual_seed(99)
    other = [(torch.randn(3, 7, 3, 3, generator=g), None, wz_ref.FP16), (torch.randn(16, 64, 1, 1, generator=g), None, wz_ref.FP8),
             (torch.randn(125, 64, 1, 1, generator=g), (torch.rand(125, 64, 1, 1, generator=g) > 0.8).float(), wz_ref.FP8),
             (torch.randn(5, 64, 3, 3, generator=g), (torch.rand(5, 64, 3, 3, generator=g) > 0.8).float(), wz_ref.FP16)]
    table, encs = [], []
    for i, (key, (w, m, enc)) in enumerate(layers.items()):
        table.append((w, m, W4))
        encs.append(enc)
        if i % 2 == 0:
            table.append(other[i // 2 % 4])
            encs.append(encode(*table[-1]))
    return table, encs


def test_all_shapes_in_one_table_with_fp16_and_fp8_segments(dev, layers):
    table, encs = mixed_table(layers)
    assert [k for _, _, k in table].count(W4) == 9 and {k for _, _, k in table} == {W4, wz_ref.FP16, wz_ref.FP8}
    assert table[0][2] == W4 and table[1][2] == wz_ref.FP16
    check_pack(table, encs, dev)
    check_unpack(table, encs, dev)
    check_unpack(table, encs, dev, want_masks=False)


def test_two_runs_give_identical_bytes(dev, layers):
    table, _ = mixed_table(layers)
    a, b = pack(table, dev), pack(table, dev)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_a_damaged_record_reads_zero_inside_its_buffers(dev, layers):
    """Bit words that select more codes than `kept` says, and a shift byte of 12: the surplus and the group read as +0.  (The
    buffer ends with the `kept` codes stored: the host checks every offset against it before the launch.)"""
    w, m, enc = layers[(70, 64, 3, 3), "random80"]
    kept = enc["kept"] - 11
    shifts = enc["shifts"].copy()
    shifts[7] = 12
    buf = wz_ref.pad8(enc["e4"].tobytes()) + wz_ref.pad8(shifts.tobytes())
    shift0, word0 = len(wz_ref.pad8(enc["e4"].tobytes())) // 8, len(buf) // 8
    buf += enc["words"].tobytes()
    val0 = len(buf)
    buf += wz_ref.pad8(enc["stored"][:kept].tobytes())
    raw = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
    out_w = torch.full(w.shape, float("nan"), device=dev)
    out_m = torch.full(w.shape, float("nan"), device=dev)
    ops.wz_unpack([dict(w=out_w, mask=out_m, kind=W4, dense=False, kept=kept, val0=val0, word0=word0, exp0=0, shift0=shift0)],
                  raw.view(torch.int64), raw.view(torch.int32), raw, raw)
    want = enc["masters"].clone().view(-1)
    want[torch.from_numpy(enc["codes"] & 7).nonzero().view(-1)[kept:]] = 0.0
    want = want.view(w.shape)
    per_filter = 64 // 32 * 9
    f, q = divmod(7, per_filter)                           # shift byte 7: filter 0, channel block 0, tap 7
    assert f == 0 and q == 7
    assert bool((want[0, :32, 2, 1] != 0).any())
    want[0, :32, 2, 1] = 0.0
    assert torch.equal(out_w.cpu().view(torch.int32), want.view(torch.int32))
    keep = torch.from_numpy(((enc["codes"] & 7) != 0).astype(np.float32)).view(w.shape)
    assert torch.equal(out_m.cpu(), keep)
