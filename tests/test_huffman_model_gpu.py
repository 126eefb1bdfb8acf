"""Huffman-coded model files through the model API on the device: the device path writes the CPU path's bytes
for every payload; a coded file loaded on the device is torch.equal to its "MCZW" twin loaded on the device in weights, masks,
codebooks and eval logits; a damaged file is refused with the model untouched; YOLOv2Train.SAVE_COMPRESSED_ENTROPY."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import compress, nets, share  # noqa: E402
from modelcompression_amd._lib import McamdError  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import nm_prune, weight_prune  # noqa: E402
from modelcompression_amd.train import YOLOv2Train  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
import hz_ref  # noqa: E402
import wz_ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
Q8_QAT = os.path.join(HERE, "golden", "q8_qat.cfg")
TWO_READERS = os.path.join(HERE, "golden", "q8_two_readers.cfg")
# payload, code bits of a tied model, the engine the file is for
CASES = [("fp32", None, "fp16"), ("fp16", None, "fp16"), ("fp8", None, "fp8"), ("w4", None, "fp8-w4"), ("shared", 2, "fp16"),
         ("shared", 4, "fp16"), ("shared", 8, "fp16")]
PRUNES = [None, "weight", "2:4", "empty"]


def model(dev, cfg=Q8_QAT, seed=3, prune=None, bits=None):
    m = nets.Darknet(cfg)
    m.load_state_dict(O.init_state(O.parse_cfg(cfg), seed=seed))
    m.to(dev)
    m.seen = 4242
    if prune in ("weight", "empty"):
        masks = weight_prune(m, 80.0)
        if prune == "empty":                                 # a layer with no kept weight
            masks[3] = torch.zeros_like(masks[3])
        m.set_masks(masks)
    elif prune == "2:4":
        m.set_masks(nm_prune(m))
    if bits is not None:
        m.set_codebooks(share.kmeans_share(m, bits=bits, iters=1))
    m.eval()
    return m


def reload(dev, cfg, path):
    m = nets.Darknet(cfg)
    m.to(dev)
    m.load_weights(path)
    m.eval()
    return m


def logits(m, x, prec):
    m.precision = prec
    m.eval()
    with torch.no_grad():
        return m(x).clone()


def state(m):
    out = {k: v.clone() for k, v in m.state_dict().items()}
    for i, (conv, _) in enumerate(wz_ref.model_layers(m)):
        out["mask_flag%d" % i] = torch.tensor(float(conv.mask_flag))
        if getattr(conv, "share_flag", False):
            out["codebook%d" % i], out["codes%d" % i] = conv.codebook.clone(), conv.codes.clone()
    return out


def same_state(a, b):
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("prune", PRUNES, ids=[str(p) for p in PRUNES])
@pytest.mark.parametrize("payload, bits, prec", CASES, ids=["%s%s" % (c[0], c[1] or "") for c in CASES])
def test_device_bytes_and_load(dev, tmp_path, payload, bits, prec, prune):
    m = model(dev, prune=prune, bits=bits)
    layers = compress.default_fp8_layers(m) if payload in ("fp8", "w4") else None
    plain, coded = str(tmp_path / "plain.mcz"), str(tmp_path / "coded.mcz")
    m.save_compressed(plain, payload, layers)
    m.save_compressed(coded, payload, layers, entropy="huffman")
    on_dev = open(coded, "rb").read()
    assert on_dev[:4] == b"MCZH" and on_dev == hz_ref.encode_file(open(plain, "rb").read())
    info = compress.compressed_info(coded)
    assert info["plain_bytes"] == os.path.getsize(plain)
    if prune:
        assert info["bytes"] < info["plain_bytes"] and any(s["mode"] == 1 for l in info["layers"] for s in l["streams"])
    # loaded on the device, the coded file is its twin: weights, masks, codebooks, BatchNorm tensors, seen, eval logits
    a, b = reload(dev, Q8_QAT, coded), reload(dev, Q8_QAT, plain)
    assert same_state(state(a), state(b)) and a.seen == b.seen == 4242
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(2)).to(dev)
    assert torch.equal(logits(a, x, prec), logits(b, x, prec))
    # ... and the CPU reader gives the same masters and masks
    c = nets.Darknet(Q8_QAT)
    c.load_weights(coded)
    for (ca, _), (cc, _) in zip(wz_ref.model_layers(a), wz_ref.model_layers(c)):
        assert torch.equal(ca.weight.data.cpu().view(torch.int32), cc.weight.data.view(torch.int32)) and ca.mask_flag == cc.mask_flag
        assert not ca.mask_flag or torch.equal(ca.mask.cpu(), cc.mask)
    # the CPU path writes the same bytes (last: the model leaves the device)
    m.cpu()
    m.save_compressed(coded + ".cpu", payload, layers, entropy="huffman")
    assert open(coded + ".cpu", "rb").read() == on_dev


def refused(dev, tmp_path, data, text):
    bad = str(tmp_path / "bad.mcz")
    open(bad, "wb").write(bytes(data))
    target = model(dev, seed=11)
    target.seen = 7
    before = state(target)
    with pytest.raises(McamdError, match=text):
        target.load_weights(bad)
    assert same_state(before, state(target)) and target.seen == 7
    assert not any(conv.mask_flag for conv, _ in wz_ref.model_layers(target))
    on_cpu = nets.Darknet(Q8_QAT)                            # the numpy path refuses the same file
    with pytest.raises(McamdError, match=text):
        on_cpu.load_weights(bad)


@pytest.mark.parametrize("payload", ["fp8", "w4"])
def test_damaged_files_are_refused_on_the_device(dev, tmp_path, payload):
    m = model(dev, prune="weight")
    plain = str(tmp_path / "plain.mcz")
    m.save_compressed(plain, payload)
    data = bytearray(open(plain, "rb").read())
    recs = compress._parse(plain)["records"]
    # bit words that do not select `kept` values, coded by the restatement (the writer would not write them)
    flipped = bytearray(data)
    flipped[recs[4]["word0"]] ^= 0x01
    refused(dev, tmp_path, hz_ref.encode_file(bytes(flipped)), "conv5: the bit words do not select")
    if payload == "w4":                                      # a stored code that is -0
        codes = bytearray(data)
        codes[recs[4]["val0"]] = (codes[recs[4]["val0"]] & 0xF0) | 0x08
        refused(dev, tmp_path, hz_ref.encode_file(bytes(codes)), "conv5: the codes stored do not hold")
    # a coded stream whose chunk no longer ends where the next begins
    coded = hz_ref.encode_file(bytes(data))
    path = str(tmp_path / "coded.mcz")
    open(path, "wb").write(coded)
    st = [s for s in compress._parse(path)["records"][4]["streams"] if s["name"] in ("values", "codes")][0]
    assert st["mode"] == 1 and st["nchunks"] > 2
    moved = bytearray(coded)
    moved[st["chunk0"] + 4:st["chunk0"] + 8] = np.array([int(st["chunk_bit0"][1]) + 1], dtype="<u4").tobytes()
    refused(dev, tmp_path, moved, "conv5 %s: the coded stream is damaged" % st["name"])


def test_train_saves_a_coded_file_beside_the_weights(dev, tmp_path):
    t = YOLOv2Train()
    t.SAVE_COMPRESSED = "fp16"
    t.SAVE_COMPRESSED_ENTROPY = "huffman"
    m = t.train('', '', '', str(tmp_path), '', '', 'p_', TWO_READERS, '', 4, 10, DEBUG_EPOCHS=0, MAX_EPOCHS=1, SYNTHETIC_SAMPLES=8,
                pruning_perc=50)
    names = sorted(os.listdir(tmp_path))
    assert len(names) == 2 and names[0].endswith(".mcz") and names[1].endswith(".weights")
    data = open(tmp_path / names[0], "rb").read()
    assert data[:4] == b"MCZH" and hz_ref.decode_file(data) == wz_ref.model_file(m, "fp16")
    info = compress.compressed_info(str(tmp_path / names[0]))
    assert info["entropy"] == "huffman" and info["payload"] == "fp16"
    # (half-pruned bit words are close to 8 bits a byte: a stream that does not pay stays raw, 16 bytes of header each)
    assert info["bytes"] <= info["plain_bytes"] + 16 * sum(len(l["streams"]) for l in info["layers"])
    r = reload(dev, TWO_READERS, str(tmp_path / names[0]))
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(7)).to(dev)
    assert torch.equal(logits(r, x, "fp16"), logits(m, x, "fp16")) and r.seen == m.seen
    t.SAVE_COMPRESSED_ENTROPY = "zip"
    with pytest.raises(ValueError, match="SAVE_COMPRESSED_ENTROPY"):
        t.train('', '', '', str(tmp_path), '', '', 'p_', TWO_READERS, '', 4, 10, DEBUG_EPOCHS=0, MAX_EPOCHS=1, SYNTHETIC_SAMPLES=8)
