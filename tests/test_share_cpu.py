"""Weight sharing without a device: the restatement (wshare_ref.py) on hand-worked cases, the numpy path of
share.kmeans_share against it, set_codebooks / project_codebooks on a CPU model, the linearity that makes the projected
step SGD on the shared values, the "shared" payload of compressed model files, and the C entry points' refusals."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest
import torch

import modelcompression_amd
from modelcompression_amd import _lib, compress, nets, ops, share
from modelcompression_amd._lib import McamdError
from modelcompression_amd.pruning.weightPruning import methods
from modelcompression_amd.synthetic import init_synthetic
import wshare_ref as R
import wz_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "golden", "mini.cfg")
NAMES = ("mcamd_ws_workspace_bytes", "mcamd_ws_init", "mcamd_ws_iterate", "mcamd_ws_assign", "mcamd_ws_project",
         "mcamd_ws_expand")
f32 = lambda *v: np.array(v, dtype=np.float32)


def make(seed=3, masked=False, seen=777):
    model = init_synthetic(nets.Darknet(MINI), seed=seed)
    model.seen = seen
    if masked:
        g = torch.Generator().manual_seed(seed + 1)
        model.set_masks([(torch.rand(conv.weight.shape, generator=g) > 0.6).float() for conv, _ in wz_ref.model_layers(model)])
    return model


def convs_of(model):
    return [conv for conv, _ in wz_ref.model_layers(model)]


def mask_of(conv):
    return conv.mask.numpy().reshape(-1) if conv.mask_flag else None


# ----------------------------------------------------------------------------- the restatement, by hand
def test_k2_on_four_values():
    w = f32(0, 1, 2, 4)
    assert R.init(w, None, 2).tolist() == [0.0, 4.0]
    assert R.assign(f32(0, 4), w).tolist() == [0, 0, 0, 1]            # mid 2: the 2 sits on it and goes down
    c, codes = R.kmeans(w, None, 2, 1)
    assert c.tolist() == [1.0, 4.0] and codes.tolist() == [0, 0, 0, 1]
    c, codes = R.kmeans(w, None, 2, 0)
    assert c.tolist() == [0.0, 4.0] and codes.tolist() == [0, 0, 0, 1]


def test_a_tie_on_a_midpoint_goes_to_the_lower_code():
    c = f32(-1, 0, 1, 2)                                              # mid -0.5, 0.5, 1.5
    assert R.assign(c, f32(-0.5, 0.5, 1.5, np.nextafter(np.float32(0.5), np.float32(1)))).tolist() == [0, 1, 2, 2]
    assert R.assign(f32(1, 1, 1, 3), f32(1, 2, 2.5)).tolist() == [0, 2, 3]        # equal centroids are harmless


def test_an_empty_cluster_keeps_its_centroid():
    w = f32(0, 0, 3, 3)
    c, codes = R.kmeans(w, None, 4, 3)
    assert c.tolist() == [0.0, 1.0, 2.0, 3.0] and codes.tolist() == [0, 0, 3, 3]


def test_all_kept_weights_equal():
    w = f32(0.5, 7, 0.5, 0.5)
    c, codes = R.kmeans(w, f32(1, 0, 1, 1), 4, 2)
    assert c.tolist() == [0.5] * 4 and codes.tolist() == [0, 0, 0, 0]


def test_a_fully_pruned_layer():
    c, codes = R.kmeans(f32(1, 2, 3), f32(0, 0, 0), 8, 2)
    assert c.tolist() == [0.0] * 8 and codes.tolist() == [0, 0, 0]
    w, c2 = R.project(f32(1, 2, 3), f32(0, 0, 0), codes, c)
    assert w.tolist() == [1.0, 2.0, 3.0] and c2.tolist() == [0.0] * 8
    assert R.expand(c, codes, f32(0, 0, 0)).tolist() == [0.0] * 3


def test_project_and_expand_by_hand():
    w, codes, mask = f32(1, 9, 2, 5, 6), np.array([0, 1, 0, 1, 1], dtype=np.uint8), f32(1, 0, 1, 1, 1)
    got, c = R.project(w, mask, codes, f32(-1, -1, 42, 43))
    assert got.tolist() == [1.5, 9.0, 1.5, 5.5, 5.5] and c.tolist() == [1.5, 5.5, 42.0, 43.0]
    again, c2 = R.project(got, mask, codes, c)
    assert again.tobytes() == got.tobytes() and c2.tobytes() == c.tobytes()
    assert R.expand(c, codes, mask).tolist() == [1.5, 0.0, 1.5, 5.5, 5.5]


# ----------------------------------------------------------------------------- the numpy path of the package
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("bits,iters", [(1, 2), (4, share.ITERS), (8, 3)])
def test_numpy_path_equals_the_restatement(masked, bits, iters):
    model = make(masked=masked)
    out = share.kmeans_share(model, bits=bits, iters=iters)
    assert len(out) == len(convs_of(model))
    for conv, (cb, codes) in zip(convs_of(model), out):
        want_c, want_codes = R.kmeans(conv.weight.data.numpy(), mask_of(conv), 1 << bits, iters)
        assert cb.dtype == torch.float32 and codes.dtype == torch.uint8 and codes.shape == conv.weight.shape
        assert cb.numpy().tobytes() == want_c.tobytes()
        assert codes.numpy().reshape(-1).tobytes() == want_codes.tobytes()


def test_layers_and_per_layer_bits():
    model = make(masked=True)
    out = share.kmeans_share(model, bits={2: 3, 5: 8}, iters=1, layers=[2, 5])
    assert [None if e is None else e[0].numel() for e in out] == [None, 8, None, None, 256, None, None]
    assert modelcompression_amd.kmeans_share is share.kmeans_share is methods.kmeans_share


def test_refusals_by_name():
    model = make()
    for bad in (0, 9, 2.0, True, {1: 4}):
        with pytest.raises(McamdError, match="bits must be an int in 1..8"):
            share.kmeans_share(model, bits=bad)
    with pytest.raises(McamdError, match="conv numbers the model does not have"):
        share.kmeans_share(model, layers=[8])
    with pytest.raises(McamdError, match="iters must be"):
        share.kmeans_share(model, iters=-1)
    convs_of(model)[2].border_bias = torch.zeros(1)
    with pytest.raises(McamdError, match="slim_export"):
        share.kmeans_share(model)
    fc = types.SimpleNamespace(blocks=[{"type": "net"}, {"type": "connected"}], models=[None])
    with pytest.raises(McamdError, match=r"\[connected\] block is not supported"):
        share.kmeans_share(fc)


def test_set_codebooks_ties_and_projection_is_the_identity():
    model = make(masked=True)
    before = set(model.state_dict())
    assert not any(conv.share_flag for conv in convs_of(model))
    books = share.kmeans_share(model, bits=4, layers=[1, 2, 3, 4, 6, 7])
    model._weights_dirty = False
    model.set_codebooks(books)
    assert model._weights_dirty
    added = set(model.state_dict()) - before
    assert len(added) == 12 and all(k.endswith(("codebook", "codes")) for k in added)
    tied = []
    for i, (conv, entry) in enumerate(zip(convs_of(model), books)):
        assert conv.share_flag == (entry is not None) == (i != 4)
        if entry is not None:
            want = R.expand(entry[0].numpy(), entry[1].numpy(), mask_of(conv))
            assert conv.weight.data.numpy().reshape(-1).tobytes() == want.tobytes()
            tied.append(conv)
    assert share.are_codebooks_consistent(model)
    snap = [(c.weight.data.clone(), c.codebook.clone()) for c in tied]
    model.project_codebooks()
    for c, (w, cb) in zip(tied, snap):
        assert c.weight.data.numpy().tobytes() == w.numpy().tobytes() and c.codebook.numpy().tobytes() == cb.numpy().tobytes()
    # an untied weight moves off its cluster and comes back on the mean; pruned positions are not written
    conv = tied[1]
    keep = conv.mask.reshape(-1) != 0
    conv.weight.data.view(-1)[~keep] = 3.0
    first = int(torch.nonzero(keep)[0])
    conv.weight.data.view(-1)[first] += 0.25
    assert not share.are_codebooks_consistent(model)
    w0 = conv.weight.data.numpy().reshape(-1).copy()
    model.project_codebooks()
    want, want_c = R.project(w0, mask_of(conv), conv.codes.numpy(), snap[1][1].numpy())
    assert conv.weight.data.numpy().reshape(-1).tobytes() == want.tobytes() and conv.codebook.numpy().tobytes() == want_c.tobytes()
    assert (conv.weight.data.view(-1)[~keep] == 3.0).all() and share.are_codebooks_consistent(model)


def test_untied_model_keeps_its_state_dict_and_structure():
    a, b = make(), make()
    share.kmeans_share(b, bits=4)                       # (clustering alone changes nothing)
    assert list(a.state_dict()) == list(b.state_dict())
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert repr(a) == repr(b)


def test_projected_sgd_is_sgd_on_the_shared_values():
    """Three steps of SGD (momentum 0.9, weight decay) on float64 weights, each followed by the projection, against SGD on
    the K shared values with the MEAN member gradient.  Both sides are float64: 1e-12."""
    rng = np.random.default_rng(0)
    n, K, lr, mu, wd = 200, 8, 0.05, 0.9, 0.01
    codes = rng.integers(0, K - 1, n).astype(np.uint8)               # (cluster K - 1 stays empty)
    mask = (rng.random(n) > 0.3).astype(np.float32)
    keep = mask != 0
    c = np.sort(rng.normal(size=K))
    w = np.where(keep, c[codes], 0.0)
    a, b = rng.normal(size=(3, n)), rng.normal(size=(3, n))           # the loss gradient of step t: a[t] * w + b[t], masked
    buf, cbuf, cs = np.zeros(n), np.zeros(K), c.copy()
    members = [keep & (codes == k) for k in range(K)]
    for t in range(3):
        g = (a[t] * w + b[t]) * mask + wd * w
        buf = mu * buf + g
        w = w - lr * buf
        book = cs.copy()
        share.np_project(w, mask, codes, book)
        gk = np.array([(a[t][m] * cs[k] + b[t][m]).mean() + wd * cs[k] if m.any() else 0.0 for k, m in enumerate(members)])
        cbuf = mu * cbuf + gk
        cs = cs - lr * cbuf * np.array([m.any() for m in members])
        assert np.abs(book - cs).max() <= 1e-12
        assert np.abs(w[keep] - cs[codes[keep]]).max() <= 1e-12 and (w[~keep] == 0).all()
        assert len(np.unique(w[keep])) <= K


# ----------------------------------------------------------------------------- the "shared" payload
def tied_model(bits, masked=True, layers=None):
    model = make(masked=masked)
    model.set_codebooks(share.kmeans_share(model, bits=bits, iters=2, layers=layers))
    return model


def pad8(n):
    return (n + 7) // 8 * 8


def expected_bytes(model):
    total = 24
    for conv, bn in wz_ref.model_layers(model):
        cout, n = conv.weight.shape[0], conv.weight.numel()
        total += 32 + pad8(4 * cout) * (4 if bn is not None else 1)
        if conv.share_flag:
            K = conv.codebook.numel()
            width = [w for w in (1, 2, 4, 8) if (1 << w) >= K][0]
            kept = int((conv.mask != 0).sum()) if conv.mask_flag else n
            total += pad8(4 * K) + (8 * ((n + 63) // 64) if kept < n else 0) + pad8((kept * width + 7) // 8)
        else:
            wm = conv.weight.data * conv.mask if conv.mask_flag else conv.weight.data
            kept = int((wm != 0).sum())
            bits = 8 * ((n + 63) // 64) + 4 * kept < 4 * n
            total += (8 * ((n + 63) // 64) if bits else 0) + 4 * (kept if bits else n)
    return total


BITS = {1: 1, 2: 2, 3: 3, 4: 4, 6: 5, 7: 8}           # conv5 stays untied; widths 1, 2, 4, 4, 8, 8


@pytest.mark.parametrize("masked", [False, True])
def test_shared_file_size_and_round_trip(tmp_path, masked):
    model = tied_model(BITS, masked=masked, layers=list(BITS))
    p1, p2 = str(tmp_path / "a.mcz"), str(tmp_path / "b.mcz")
    model.save_compressed(p1, "shared")
    assert os.path.getsize(p1) == expected_bytes(model)
    fresh = nets.Darknet(MINI)
    masks = fresh.load_compressed(p1)
    assert fresh.seen == 777 and len(masks) == 7
    for a, b, m in zip(convs_of(model), convs_of(fresh), masks):
        assert torch.equal(a.weight.data, b.weight.data) and a.share_flag == b.share_flag and a.mask_flag == b.mask_flag
        if a.share_flag:
            assert torch.equal(a.codebook, b.codebook)
            keep = a.mask != 0 if a.mask_flag else torch.ones_like(a.weight, dtype=torch.bool)
            assert torch.equal(a.codes[keep], b.codes[keep]) and (b.codes[~keep] == 0).all()
        if a.mask_flag:
            assert torch.equal(a.mask, b.mask) and torch.equal(m, a.mask)
    fresh.save_compressed(p2, "shared")
    assert open(p1, "rb").read() == open(p2, "rb").read()
    info = compress.compressed_info(p1)
    assert info["payload"] == "shared" and info["bytes"] == os.path.getsize(p1)
    assert [l["kind"] for l in info["layers"]] == ["shared"] * 4 + ["fp32"] + ["shared"] * 2
    assert [(l["bits"], l["width"], l["codebook"]) for l in info["layers"] if l["kind"] == "shared"] == \
        [(1, 1, 2), (2, 2, 4), (3, 4, 8), (4, 4, 16), (5, 8, 32), (8, 8, 256)]
    assert "bits" not in info["layers"][4]
    # Darknet.load_weights dispatches on the magic
    again = nets.Darknet(MINI)
    again.load_weights(p1)
    assert all(torch.equal(a.weight.data, b.weight.data) for a, b in zip(convs_of(model), convs_of(again)))


def test_a_shared_value_of_exactly_zero_survives(tmp_path):
    model = make(masked=True)
    books = share.kmeans_share(model, bits=2, iters=2)
    books[1][0][1] = 0.0                                 # a cluster of conv2 sits on 0: its members are kept weights
    model.set_codebooks(books)
    conv = convs_of(model)[1]
    zeros = int(((conv.weight.data == 0) & (conv.mask != 0)).sum())
    assert zeros > 0
    path = str(tmp_path / "z.mcz")
    model.save_compressed(path, "shared")
    fresh = nets.Darknet(MINI)
    fresh.load_compressed(path)
    got = convs_of(fresh)[1]
    assert torch.equal(got.mask, conv.mask) and torch.equal(got.weight.data, conv.weight.data)
    assert int(((got.weight.data == 0) & (got.mask != 0)).sum()) == zeros
    assert compress.compressed_info(path)["layers"][1]["kept"] == int((conv.mask != 0).sum())


@pytest.mark.parametrize("masked", [False, True])
def test_existing_payloads_write_the_same_bytes(tmp_path, masked):
    """The files of the payloads that existed before are the independent restatement's (wz_ref.py), tied model or not."""
    for model in (make(masked=masked), tied_model(4, masked=masked)):
        for payload in ("fp32", "fp16", "fp8"):
            path = str(tmp_path / "m.mcz")
            compress.save_compressed(model, path, payload, [2, 3, 4])
            assert open(path, "rb").read() == wz_ref.model_file(model, payload, [2, 3, 4]), payload


def test_corrupt_shared_records_raise(tmp_path):
    model = tied_model({1: 3}, layers=[1])               # conv1: 3 bits in a width of 4, masked
    path, bad = str(tmp_path / "m.mcz"), str(tmp_path / "bad.mcz")
    model.save_compressed(path, "shared")
    raw = bytearray(open(path, "rb").read())
    conv = convs_of(model)[0]
    n = conv.weight.numel()
    codebook = 24 + 32 + 4 * pad8(4 * 32)
    codes = codebook + 32 + 8 * ((n + 63) // 64)
    assert np.frombuffer(raw, "<f4", 8, codebook).tobytes() == conv.codebook.numpy().tobytes()

    def refused(data, text):
        open(bad, "wb").write(data)
        with pytest.raises(McamdError, match=text):
            nets.Darknet(MINI).load_compressed(bad)

    hit = bytearray(raw)
    hit[codes + 5] |= 0x80                               # a code of at least 8
    refused(hit, "a code of 1[0-5] with a codebook of 8 entries")
    refused(raw[:codebook + 16], "truncated file")       # a short codebook
    hit = bytearray(raw)
    struct.pack_into("<I", hit, 24 + 20, 2)              # ... or one shorter than the codes were written for
    refused(hit, "truncated|behind the last record|a code of|damaged record header")
    hit = bytearray(raw)
    struct.pack_into("<I", hit, 24 + 20, 0)
    refused(hit, "damaged record header")
    hit = bytearray(raw)
    struct.pack_into("<I", hit, 8, _lib.WZ_FP32)         # codes in a file that says it holds none
    refused(hit, "damaged record header")
    with pytest.raises(McamdError, match="payload must be one of"):
        model.save_compressed(bad, "shared4")


def test_share_is_a_keyword_that_leaves_the_positional_parameters_alone():
    from modelcompression_amd.train import YOLOv2Train
    params = list(inspect.signature(YOLOv2Train.train).parameters)
    assert params[-3:] == ["RESIDENT", "TEACHER", "DISTILL"] and "SHARE" not in params and YOLOv2Train.SHARE is None
    t = YOLOv2Train()
    with pytest.raises(McamdError, match="bits must be an int in 1..8"):           # the keyword reaches kmeans_share ...
        t.train('', '', '', '', '', '', '', MINI, '', 4, 10, MAX_EPOCHS=1, SHARE=9)
    assert t._share_arg is None                                                      # ... and does not outlive the call
    with pytest.raises(McamdError, match="bits must be an int in 1..8"):
        t.train('', '', '', '', '', '', '', MINI, '', 4, 10, MAX_EPOCHS=1, SHARE=dict(bits=0, iters=2))
    t.SHARE = 2.5                                                                    # the attribute is the keyword's default
    with pytest.raises(McamdError, match="bits must be an int in 1..8"):
        t.train('', '', '', '', '', '', '', MINI, '', 4, 10, MAX_EPOCHS=1)
    with pytest.raises(TypeError):                                                   # one positional argument too many
        t.train('', '', '', '', '', '', '', MINI, '', 4, 10, '', -1, 0, 0., "weight", 1, 8, False, False, False, None, None, 4)


def test_save_compressed_attribute_accepts_shared():
    from modelcompression_amd.train import YOLOv2Train
    t = YOLOv2Train()
    t.SAVE_COMPRESSED = "int4"
    with pytest.raises(ValueError, match='"fp8" or "shared"'):
        t.train('', '', '', '', '', '', '', MINI, '', 4, 10, MAX_EPOCHS=1)


# ----------------------------------------------------------------------------- the C surface
def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mcamd_ws_\w+)\(", hdr))
    assert declared == set(NAMES) == set(k for k in _lib.SIGNATURES if k.startswith("mcamd_ws_"))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (mcamd_ws_\w+)", out))
    assert exported == set(NAMES)
    lib = _lib.lib()
    assert all(hasattr(lib, name) for name in NAMES)
    body = re.search(r"typedef struct mcamd_ws_seg \{(.*?)\} mcamd_ws_seg;", hdr, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.WsSeg._fields_] and C.sizeof(_lib.WsSeg) == 56
    for name, value in (("MCAMD_WS_SLAB", _lib.WS_SLAB), ("MCAMD_WZ_CODE", _lib.WZ_CODE)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
    src = open(os.path.join(ROOT, "modelcompression_amd", "build.py")).read()
    assert re.search(r'"wshare.hip": \["-ffp-contract=off"\]', src)
    for f in (ops.WsTable, share.kmeans_share, nets.Darknet.set_codebooks, nets.Darknet.project_codebooks):
        assert callable(f)


def seg(**kw):
    s = _lib.WsSeg()
    s.w, s.mask, s.codes, s.n, s.K = 4096, None, 8192, 5000, 16
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def calls(lib, arr, nseg=1, cb_cap=16, ws_bytes=1 << 20, P=4096):
    return {
        "ws_init": lambda: lib.mcamd_ws_init(arr, P, nseg, P, cb_cap, P, ws_bytes, None),
        "ws_iterate": lambda: lib.mcamd_ws_iterate(arr, P, nseg, P, cb_cap, P, P, P, ws_bytes, None),
        "ws_assign": lambda: lib.mcamd_ws_assign(arr, P, nseg, P, cb_cap, None),
        "ws_project": lambda: lib.mcamd_ws_project(arr, P, nseg, P, cb_cap, P, P, P, ws_bytes, None),
        "ws_expand": lambda: lib.mcamd_ws_expand(arr, P, nseg, P, cb_cap, None),
    }


@pytest.mark.parametrize("bad,text", [
    (dict(w=None), "bad tensor"),
    (dict(n=0), "bad tensor"),
    (dict(K=0), "K 0 is not 2^bits"),
    (dict(K=12), "K 12 is not 2^bits"),
    (dict(K=512), "K 512 is not 2^bits"),
    (dict(w=4100), "16-byte aligned"),
    (dict(mask=4104), "16-byte aligned"),
    (dict(codes=8194), "4-byte aligned"),
    (dict(slab0=1), "slab0 1 is not the running sum 0"),
    (dict(cb0=16), "cb0 16 is not the running sum 0"),
    (dict(part0=32), "part0 32 is not the running sum 0"),
])
def test_entry_points_refuse_bad_tables(bad, text):
    """Every argument error is refused before a launch (the pointers are never dereferenced: this runs without a device)."""
    lib = _lib.lib()
    arr = (_lib.WsSeg * 1)(seg(**bad))
    for name, call in calls(lib, arr).items():
        assert call() == -1, name
        err = lib.mcamd_last_error().decode()
        assert text in err and err.startswith(name + ":"), err


def test_entry_points_refuse_short_buffers_and_recordings():
    lib = _lib.lib()
    err = lambda: lib.mcamd_last_error().decode()
    arr = (_lib.WsSeg * 2)(seg(), seg(K=256, slab0=2, cb0=16, part0=32))
    for name, call in calls(lib, arr, nseg=2, cb_cap=271).items():
        assert call() == -1 and "272 codebook entries needed, room for 271" in err(), name
    need = lib.mcamd_ws_workspace_bytes(4, 2 * 16 + 2 * 256, 2)
    assert need >= (2 * 16 + 2 * 256) * 12 + 4 * 8
    for name in ("ws_init", "ws_iterate", "ws_project"):
        assert calls(lib, arr, nseg=2, cb_cap=272, ws_bytes=need - 1)[name]() != 0 and "workspace too small" in err(), name
    null = (_lib.WsSeg * 1)(seg(codes=None))
    for name in ("ws_iterate", "ws_assign", "ws_project", "ws_expand"):
        assert calls(lib, null)[name]() == -1 and "null codes" in err(), name
    assert lib.mcamd_ws_iterate(arr, 4096, 2, 4096, 272, None, 4096, 4096, 1 << 20, None) == -1 and "null argument" in err()
    assert lib.mcamd_ws_expand(None, 4096, 1, 4096, 16, None) == -1 and "null argument" in err()
    streams = (C.c_void_p * 1)(None)
    assert lib.mcamd_plan_begin(streams, 1) == 0
    try:
        one = (_lib.WsSeg * 1)(seg())
        for name, call in calls(lib, one).items():
            assert call() == -1 and (name + ": not recordable") in err(), name
    finally:
        plan = lib.mcamd_plan_end()
        if plan:
            lib.mcamd_plan_destroy(plan)


def test_wrappers_have_no_cpu_path():
    w = torch.zeros(8)
    with pytest.raises(McamdError, match="no CPU path"):
        ops.WsTable([dict(w=w, mask=None, codes=torch.zeros(8, dtype=torch.uint8), K=4)])
