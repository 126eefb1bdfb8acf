"""csrc/wpack.hip: ops.wz_pack / ops.wz_unpack against the numpy restatement (wz_ref.py), byte for byte -- bit words, kept
counts, exponents and values of every segment, alone and as one multi-segment table; unpacked weights and masks by bit
pattern; the same input twice gives the same bytes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import ops  # noqa: E402
import wz_ref  # noqa: E402

SHAPES = [(1, 1, 1, 1), (3, 7, 3, 3), (16, 64, 1, 1), (5, 64, 3, 3), (125, 64, 1, 1), (32, 64, 3, 3), (256, 128, 3, 3)]
MASKS = ["ones", "zeros", "random80", "2:4", "last", "zero_words_then_ones", "signed_zeros"]
KINDS = [wz_ref.FP32, wz_ref.FP16, wz_ref.FP8]


def weights(shape, seed):
    """fp32 OIHW weights with a scale of their own per filter, a few weights far below the filter's largest (they round to
    the zero code in fp16 / e4m3 and are dropped) and both signs."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g) * torch.pow(2.0, torch.randint(-6, 7, (shape[0], 1, 1, 1), generator=g).float())
    flat = w.view(-1)
    n = flat.numel()
    if n >= 64:
        flat[torch.randperm(n, generator=g)[:max(1, n // 50)]] = 1e-9
    return w


def mask_of(name, shape, w, seed):
    g = torch.Generator().manual_seed(seed + 77)
    n = w.numel()
    if name == "ones":
        return torch.ones(shape)
    if name == "zeros":
        return torch.zeros(shape)
    if name == "random80":
        return (torch.rand(shape, generator=g) >= 0.8).float()
    if name == "2:4":
        if shape[1] % 4:                       # no groups of 4 input channels: the pattern over the flat index
            return torch.tensor([1.0, 0.0, 0.0, 1.0]).repeat((n + 3) // 4)[:n].view(shape).clone()
        O, I, kh, kw = shape
        order = torch.rand(O, I // 4, 4, kh, kw, generator=g).argsort(dim=2)
        return (order < 2).float().view(shape)
    if name == "last":
        m = torch.zeros(n)
        m[-1] = 1.0
        return m.view(shape)
    if name == "zero_words_then_ones":
        m = torch.ones(n)
        m[:64 * 64] = 0.0
        return m.view(shape)
    if name == "signed_zeros":                 # all-ones mask over weights holding exact zeros of both signs
        flat = w.view(-1)
        idx = torch.randperm(n, generator=g)
        flat[idx[:n // 3]] = 0.0
        flat[idx[n // 3:n // 2]] = -0.0
        return None
    raise AssertionError(name)


def layer(shape, mask_name, kind, seed):
    w = weights(shape, seed)
    return w, mask_of(mask_name, shape, w, seed), kind


def pack(layers, dev):
    items = [dict(w=w.to(dev), mask=(m.to(dev) if m is not None else None), kind=k) for w, m, k in layers]
    words, counts, exps, values = ops.wz_pack(items)
    torch.cuda.synchronize()
    return (words.cpu().numpy().view("<u8"), counts.cpu().numpy().view("<u8"), exps.cpu().numpy(), values.cpu().numpy())


def check_pack(layers, dev):
    """Every output of one ops.wz_pack call against the restatement; returns the restatement's encodings."""
    words, counts, exps, values = pack(layers, dev)
    encs = [wz_ref.encode_layer(w, m, k) for w, m, k in layers]
    w0 = e0 = v0 = 0
    for s, ((w, m, k), enc) in enumerate(zip(layers, encs)):
        nwords = -(-enc["n"] // 64)
        assert int(counts[s]) == enc["kept"], (s, w.shape)
        assert words[w0:w0 + nwords].tobytes() == enc["all_words"].tobytes(), (s, w.shape)
        w0 += nwords
        if k == wz_ref.FP8:
            assert exps[e0:e0 + w.shape[0]].tobytes() == enc["exps"].tobytes(), (s, w.shape)
            e0 += w.shape[0]
        want = wz_ref.pad8(enc["values"].tobytes())
        assert values[v0:v0 + len(want)].tobytes() == want, (s, w.shape, enc["words"] is not None)
        v0 += len(want)
    assert w0 == words.size and e0 == exps.size and not values[v0:].any()
    return encs


def check_unpack(layers, encs, dev, want_masks=True):
    """ops.wz_unpack of the RESTATEMENT's arrays (what a file holds) against the restatement's decoder, by bit pattern."""
    items, words, exps, values, v0 = [], [], [], b"", 0
    outs = []
    for (w, m, k), enc in zip(layers, encs):
        out_w = torch.full(w.shape, float("nan"), device=dev)
        out_m = torch.full(w.shape, float("nan"), device=dev) if want_masks else None
        outs.append((out_w, out_m))
        items.append(dict(w=out_w, mask=out_m, kind=k, dense=enc["words"] is None, kept=enc["kept"], val0=v0))
        if enc["words"] is not None:
            words.append(enc["words"])
        if k == wz_ref.FP8:
            exps.append(enc["exps"])
        values += wz_ref.pad8(enc["values"].tobytes())
        v0 = len(values)
    words = torch.from_numpy(np.concatenate(words).view(np.int64)).to(dev) if words else None
    exps = torch.from_numpy(np.concatenate(exps).astype(np.int32)).to(dev) if exps else None
    values = torch.frombuffer(bytearray(values), dtype=torch.uint8).to(dev) if values else None
    ops.wz_unpack(items, words, exps, values)
    for (w, m, k), enc, (out_w, out_m) in zip(layers, encs, outs):
        rec = dict(shape=tuple(w.shape), kind=k, kept=enc["kept"], exps=enc["exps"], words=enc["words"], values=enc["values"])
        ref_w, ref_m = wz_ref.decode(rec)
        assert out_w.cpu().numpy().view("<u4").tobytes() == ref_w.view("<u4").tobytes(), (w.shape, k)
        if want_masks:
            assert out_m.cpu().numpy().view("<u4").tobytes() == ref_m.view("<u4").tobytes(), (w.shape, k)


@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("kind", KINDS, ids=["fp32", "fp16", "fp8"])
def test_every_layer_alone_and_as_one_table(dev, kind, mask_name):
    layers = [layer(shape, mask_name, kind, seed) for seed, shape in enumerate(SHAPES)]
    for one in layers:
        encs = check_pack([one], dev)
        check_unpack([one], encs, dev)
    encs = check_pack(layers, dev)
    check_unpack(layers, encs, dev)
    if mask_name in ("ones", "signed_zeros"):
        assert any(e["words"] is None for e in encs), "a dense record"
    if mask_name in ("zeros", "random80", "last"):
        assert all(e["words"] is not None for e in encs if e["n"] > 64), "records with bit words"


def test_mixed_kinds_and_masks_in_one_table(dev):
    """e4m3, fp16 and fp32 records, dense and bitmask records, masked and unmasked layers next to each other."""
    layers = []
    for seed, shape in enumerate(SHAPES + SHAPES[::-1]):
        layers.append(layer(shape, MASKS[seed % len(MASKS)], KINDS[(seed * 2 + 1) % 3] if seed % 5 else wz_ref.FP8, 100 + seed))
    kinds = [k for _, _, k in layers]
    assert {wz_ref.FP8, wz_ref.FP16, wz_ref.FP32} == set(kinds) and kinds[0] == wz_ref.FP8
    encs = check_pack(layers, dev)
    assert any(e["words"] is None for e in encs) and any(e["words"] is not None for e in encs)
    check_unpack(layers, encs, dev)
    check_unpack(layers, encs, dev, want_masks=False)


def test_two_runs_give_identical_bytes(dev):
    layers = [layer(shape, "random80", KINDS[seed % 3], 200 + seed) for seed, shape in enumerate(SHAPES)]
    a, b = pack(layers, dev), pack(layers, dev)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_a_damaged_record_reads_inside_its_values(dev):
    """Bit words that select more values than `kept` says: the surplus reads as +0, nothing outside `values` is touched."""
    w, m, k = layer((16, 64, 1, 1), "random80", wz_ref.FP16, 300)
    enc = wz_ref.encode_layer(w, m, k)
    kept = enc["kept"] - 10
    out_w = torch.full(w.shape, float("nan"), device=dev)
    values = torch.frombuffer(bytearray(wz_ref.pad8(enc["values"][:kept].tobytes())), dtype=torch.uint8).to(dev)
    words = torch.from_numpy(enc["words"].view(np.int64).copy()).to(dev)
    ops.wz_unpack([dict(w=out_w, mask=None, kind=k, dense=False, kept=kept, val0=0)], words, None, values)
    ref, _ = wz_ref.decode(dict(shape=tuple(w.shape), kind=k, kept=enc["kept"], exps=None, words=enc["words"], values=enc["values"]))
    flat, got = ref.reshape(-1).copy(), out_w.cpu().numpy().reshape(-1)
    flat[np.flatnonzero(flat)[kept:]] = 0.0
    assert got.view("<u4").tobytes() == flat.view("<u4").tobytes()
