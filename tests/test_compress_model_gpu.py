"""Compressed model files through the model API on the device: the lossless contract of each payload through
a fresh Darknet + load_weights(path), device-written bytes = CPU-written bytes = the numpy restatement's, masks returned and
set, YOLOv2Train.SAVE_COMPRESSED, and the default fp8 layer rule and file size on YOLOv2-VOC."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import compress, nets, YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd.pruning.weightPruning.methods import nm_prune, weight_prune  # noqa: E402
from modelcompression_amd.pruning.weightPruning.utils import are_masks_consistent, prune_rate  # noqa: E402
from modelcompression_amd.train import YOLOv2Train  # noqa: E402
from oracle import darknet_ref as O  # noqa: E402
import wz_ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "golden", "mini.cfg")
Q8_QAT = os.path.join(HERE, "golden", "q8_qat.cfg")
TWO_READERS = os.path.join(HERE, "golden", "q8_two_readers.cfg")
CFGS = [MINI, Q8_QAT, TWO_READERS]
IDS = ["mini", "q8_qat", "q8_two_readers"]


def model(dev, cfg, seed=0, prune=None):
    m = nets.Darknet(cfg)
    m.load_state_dict(O.init_state(O.parse_cfg(cfg), seed=seed))
    m.to(dev)
    m.seen = 4242
    if prune == "weight":
        m.set_masks(weight_prune(m, 80.0))
    elif prune == "2:4":
        m.set_masks(nm_prune(m))
    m.eval()
    return m


def reload(dev, cfg, path):
    m = nets.Darknet(cfg)
    m.to(dev)
    m.load_weights(path)
    m.eval()
    return m


def picture(dev, seed=1):
    return torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(seed)).to(dev)


def engine(m, x, prec):
    return [e for k, e in m._engines.items() if k[0] == tuple(x.shape) and k[3] == prec and not e.train_layout][0]


def logits(m, x, prec, sparse=None):
    m.precision, m.sparse = prec, sparse
    with torch.no_grad():
        out = m(x).clone()
    eng = engine(m, x, prec)
    return out, eng


def bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("prune", [None, "weight", "2:4"])
@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_fp32_file_is_the_model_bit_for_bit(dev, tmp_path, cfg, prune):
    m = model(dev, cfg, prune=prune)
    path = str(tmp_path / "m.mcz")
    m.save_compressed(path, "fp32")
    assert open(path, "rb").read() == wz_ref.model_file(m, "fp32")
    r = reload(dev, cfg, path)
    assert r.seen == 4242
    a, b = m.state_dict(), r.state_dict()
    assert set(k for k in a if not k.endswith("mask")) == set(k for k in b if not k.endswith("mask"))
    for (conv, bn), (conv2, bn2) in zip(wz_ref.model_layers(m), wz_ref.model_layers(r)):
        wm = conv.weight.data * conv.mask if conv.mask_flag else conv.weight.data
        assert torch.equal(bits(conv2.weight), bits(torch.where(wm == 0, torch.zeros_like(wm), wm)))
        pairs = [(bn.bias, bn2.bias), (bn.weight, bn2.weight), (bn.running_mean, bn2.running_mean),
                 (bn.running_var, bn2.running_var)] if bn is not None else [(conv.bias, conv2.bias)]
        assert all(torch.equal(bits(p), bits(q)) for p, q in pairs)


@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_fp16_file_is_lossless_for_the_fp16_engines(dev, tmp_path, cfg):
    x = picture(dev)
    path = str(tmp_path / "m.mcz")
    for prune, sparse in ((None, None), ("weight", None), ("2:4", None), ("2:4", "2:4")):
        m = model(dev, cfg, prune=prune)
        want, eng = logits(m, x, "fp16", sparse)
        m.save_compressed(path, "fp16")
        r = reload(dev, cfg, path)
        got, eng2 = logits(r, x, "fp16", sparse)
        assert torch.equal(got, want), (prune, sparse)
        assert eng2.sparse_layers == eng.sparse_layers
        if prune:
            assert all(conv.mask_flag for conv, _ in wz_ref.model_layers(r))


@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("cfg", [Q8_QAT, TWO_READERS], ids=IDS[1:])
def test_fp8_file_is_lossless_for_the_fp8_engines(dev, tmp_path, setenv, cfg, mfma):
    setenv("MCAMD_Q8_MFMA", mfma)
    x = picture(dev, seed=2)
    path = str(tmp_path / "m.mcz")
    for prune, prec in ((None, "fp8"), ("weight", "fp8"), ("2:4", "fp8"), ("2:4", "fp8-2:4")):
        m = model(dev, cfg, seed=3, prune=prune)
        want, eng = logits(m, x, prec)
        assert eng.fp8_layers
        m.save_compressed(path, "fp8", eng.fp8_layers)
        info = compress.compressed_info(path)
        assert [l["conv"] for l in info["layers"] if l["kind"] == "fp8"] == eng.fp8_layers
        assert all(l["kind"] in ("fp8", "fp16") for l in info["layers"])
        r = reload(dev, cfg, path)
        got, eng2 = logits(r, x, prec)
        assert eng2.fp8_layers == eng.fp8_layers and eng2.fp8_sparse_layers == eng.fp8_sparse_layers
        if prec == "fp8-2:4":
            assert eng.fp8_sparse_layers
        assert torch.equal(got, want), (prune, prec, mfma)


@pytest.mark.parametrize("payload", ["fp32", "fp16", "fp8"])
@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_device_bytes_are_cpu_bytes(dev, tmp_path, cfg, payload):
    m = model(dev, cfg, seed=5, prune="weight")
    layers = compress.default_fp8_layers(m)
    a, b = str(tmp_path / "dev.mcz"), str(tmp_path / "cpu.mcz")
    m.save_compressed(a, payload, layers)
    want = wz_ref.model_file(m, payload, layers)
    m.cpu()
    m.save_compressed(b, payload, layers)
    got_dev, got_cpu = open(a, "rb").read(), open(b, "rb").read()
    assert got_dev == want and got_cpu == want
    # ... and both readers give the same masters and masks
    on_dev, on_cpu = nets.Darknet(cfg).to(dev), nets.Darknet(cfg)
    md, mc = on_dev.load_compressed(a), on_cpu.load_compressed(a)
    for (c1, _), (c2, _), m1, m2 in zip(wz_ref.model_layers(on_dev), wz_ref.model_layers(on_cpu), md, mc):
        assert torch.equal(bits(c1.weight).cpu(), bits(c2.weight)) and torch.equal(m1.cpu(), m2)


@pytest.mark.parametrize("payload", ["fp32", "fp16"])
def test_masks_are_returned_and_set(dev, tmp_path, payload):
    m = model(dev, MINI, seed=7, prune="weight")
    rate = prune_rate(m, verbose=False)
    originals = [conv.mask.clone() for conv, _ in wz_ref.model_layers(m)]
    path = str(tmp_path / "m.mcz")
    m.save_compressed(path, payload)
    r = nets.Darknet(MINI).to(dev)
    masks = r.load_compressed(path)
    assert len(masks) == len(originals) and all(k.device == o.device and k.shape == o.shape for k, o in zip(masks, originals))
    assert all(torch.equal(k, o) for k, o in zip(masks, originals)), "no kept weight of a seeded model is zero"
    assert prune_rate(r, verbose=False) == rate and rate > 70.0
    assert are_masks_consistent(r, masks) and are_masks_consistent(r, originals)
    assert all(conv.mask_flag and torch.equal(conv.mask, k) for (conv, _), k in zip(wz_ref.model_layers(r), masks))
    plain = nets.Darknet(MINI).to(dev)
    again = plain.load_compressed(path, set_masks=False)
    assert all(torch.equal(k, o) for k, o in zip(again, masks)) and not any(c.mask_flag for c, _ in wz_ref.model_layers(plain))


def test_damaged_bit_words_are_refused_on_the_device_as_on_the_cpu(dev, tmp_path):
    """A record whose bit words do not select `kept` values raises on either path, before anything is written."""
    m = model(dev, MINI, seed=9, prune="weight")
    path = str(tmp_path / "m.mcz")
    m.save_compressed(path, "fp16")
    rec = [r for r in compress._parse(path, payload=False)["records"] if r["bits"]][-1]
    raw = bytearray(open(path, "rb").read())
    word = int.from_bytes(raw[rec["word0"]:rec["word0"] + 8], "little")
    lowest = word & -word
    assert lowest, "the first word of a record at 80 % sparsity keeps something in a seeded model"
    raw[rec["word0"]:rec["word0"] + 8] = (word ^ lowest).to_bytes(8, "little")          # one kept bit cleared
    open(path, "wb").write(bytes(raw))
    for r in (nets.Darknet(MINI).to(dev), nets.Darknet(MINI)):
        before = {k: v.clone() for k, v in r.state_dict().items()}
        with pytest.raises(compress.McamdError, match="bit words do not select"):
            r.load_compressed(path)
        after = r.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before)


def test_train_saves_a_compressed_file_beside_the_weights(dev, tmp_path):
    out = tmp_path / "with"
    out.mkdir()
    t = YOLOv2Train()
    t.SAVE_COMPRESSED = "fp16"
    m = t.train('', '', '', str(out), '', '', 'p_', MINI, '', 4, 10, DEBUG_EPOCHS=0, MAX_EPOCHS=1, SYNTHETIC_SAMPLES=8,
                pruning_perc=50)
    names = sorted(os.listdir(out))
    assert len(names) == 2 and names[0].endswith(".mcz") and names[1].endswith(".weights")
    assert os.path.splitext(names[0])[0] == os.path.splitext(names[1])[0]
    assert open(out / names[0], "rb").read() == wz_ref.model_file(m, "fp16")
    r = reload(dev, MINI, str(out / names[0]))
    x = picture(dev, seed=4)
    m.eval()
    want, _ = logits(m, x, "fp16")
    got, _ = logits(r, x, "fp16")
    assert torch.equal(got, want) and r.seen == m.seen
    # the default writes exactly the file train() wrote before
    bare = tmp_path / "without"
    bare.mkdir()
    YOLOv2Train().train('', '', '', str(bare), '', '', 'p_', MINI, '', 4, 10, DEBUG_EPOCHS=0, MAX_EPOCHS=1, SYNTHETIC_SAMPLES=8,
                        pruning_perc=50)
    assert os.listdir(bare) == [names[1]]
    # MODEL_WEIGHT accepts the file with no new keyword: its masks come along, and its `seen` (one epoch of 8 samples)
    # resumes the run at the second epoch
    resumed = tmp_path / "resumed"
    resumed.mkdir()
    m2 = YOLOv2Train().train('', '', '', str(resumed), '', '', 'p_', MINI, str(out / names[0]), 4, 10, DEBUG_EPOCHS=0, MAX_EPOCHS=2,
                             SYNTHETIC_SAMPLES=8)
    assert os.listdir(resumed) == ['weight-pruned-0.0-retrained-final_000002.weights']
    assert all(conv.mask_flag for conv, _ in wz_ref.model_layers(m2)) and are_masks_consistent(m2, [c.mask for c, _ in wz_ref.model_layers(r)])
    assert YOLOv2Train.SAVE_COMPRESSED is None
    t.SAVE_COMPRESSED = "int4"
    with pytest.raises(ValueError, match="SAVE_COMPRESSED"):
        t.train('', '', '', '', '', '', 'p_', MINI, '', 4, 10, MAX_EPOCHS=1, SYNTHETIC_SAMPLES=8)


def test_yolov2_default_layers_and_fp8_file_size(dev, tmp_path):
    m = model(dev, YOLOV2_VOC_CFG, seed=1, prune="2:4")
    x = torch.rand(1, 3, 416, 416, generator=torch.Generator().manual_seed(5)).to(dev)
    _, eng = logits(m, x, "fp8-2:4")
    assert compress.default_fp8_layers(m) == eng.fp8_layers == list(range(3, 23))
    path = str(tmp_path / "yolo.mcz")
    m.save_compressed(path, "fp8")
    info = compress.compressed_info(path)
    # closed form from the layer shapes: nm_prune keeps half of every conv but conv1 (3 input channels: all of it)
    records = []
    for i, (conv, bn) in enumerate(wz_ref.model_layers(m)):
        n = conv.weight.numel()
        records.append((tuple(conv.weight.shape), bn is not None, wz_ref.FP8 if 3 <= i + 1 <= 22 else wz_ref.FP16,
                        n if i == 0 else n // 2))
    assert os.path.getsize(path) == info["bytes"] == wz_ref.closed_form_bytes(records)
    assert [l["kept"] for l in info["layers"]] == [r[3] for r in records]
    assert info["dense_bytes"] == wz_ref.dense_bytes([(r[0], r[1]) for r in records])
    print("YOLOv2-VOC, nm_prune, fp8 file: %d bytes, %.2fx against %d" % (info["bytes"], info["ratio"], info["dense_bytes"]))
    assert 6.0 < info["ratio"] < 6.6          # 1/8 byte of bitmask + 1/2 byte of codes per weight against 4: 6.4x
    r = reload(dev, YOLOV2_VOC_CFG, path)
    want, _ = logits(m, x, "fp8-2:4")
    got, eng2 = logits(r, x, "fp8-2:4")
    assert eng2.fp8_sparse_layers == eng.fp8_sparse_layers and torch.equal(got, want)
