"""The train / predict entry points end to end on the GPU (synthetic data: VOC is not on disk)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from modelcompression_amd import YOLOV2_VOC_CFG  # noqa: E402
from modelcompression_amd.train import YOLOv2Train  # noqa: E402
from modelcompression_amd.predict import PASCALVOCEval  # noqa: E402
from modelcompression_amd.pruning.weightPruning.utils import prune_rate  # noqa: E402


@pytest.mark.parametrize("method,perc", [("weight", 80.0), ("filter", 40.0)])
def test_prune_and_retrain_one_epoch(dev, tmp_path, method, perc):
    t = YOLOv2Train()
    model = t.train('', '', '', str(tmp_path / "log"), str(tmp_path / "val"), str(tmp_path / "pkl"), 'p_',
                    YOLOV2_VOC_CFG, '', 8, 10, pruning_perc=perc, pruning_method=method,
                    MAX_EPOCHS=1, SYNTHETIC_SAMPLES=16)
    rate = prune_rate(model, verbose=False)
    assert rate > (75.0 if method == "weight" else 10.0)       # pruned weights stayed zero through SGD (40% of the FILTERS is ~16% of the weights here)
    final = [f for f in os.listdir(tmp_path / "log") if f.endswith(".weights")]
    assert len(final) == 1 and os.path.getsize(tmp_path / "log" / final[0]) == 202704260
    for p in model.parameters():
        assert torch.isfinite(p).all()


def test_predict_plumbing(dev, tmp_path):
    from modelcompression_amd import nets
    from modelcompression_amd.synthetic import init_synthetic
    m = init_synthetic(nets.Darknet(YOLOV2_VOC_CFG), 0).to(dev)
    ev = PASCALVOCEval(m, YOLOV2_VOC_CFG, '', None, '', '', str(tmp_path / "det"), 'comp4_det_test_', str(tmp_path / "pkl"))
    ev.predict(BATCH_SIZE=4, CONF_THRESH=0.3)
    files = os.listdir(tmp_path / "det")
    assert len(files) == 20 and ev.num_detections >= 0


def test_smoke_entry(dev):
    import __graft_entry__ as g
    g.smoke()


def test_bench_plain_run_dumps_last_step(dev, tmp_path):
    """A plain `bench.py` run prints the headline line only (the rest is `--full`'s) and `--dump-outputs` writes the last
    timed step's results: float32 arrays, finite, the loss = the mean of the dumped logits (the headline loss)."""
    import json
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "8", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["value"] > 0 and res["unit"] == "images/s"
    assert res["higher_is_better"] is True and res["dtype"] == "fp16"
    assert not {"roofline", "cpu_baseline", "parity"} & set(res) and res["config"]["throughput_mode"] is None
    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert set(got) == {"logits", "loss", "grad_sample", "weight_sample", "bn_running_stats"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
    assert got["logits"].size == 8 * 125 * 13 * 13 and got["grad_sample"].size == got["weight_sample"].size > 1 << 20
    logits = got["logits"].astype(np.float64)
    assert abs(logits.mean() - float(got["loss"][0])) <= 1e-5 * np.abs(logits).mean()


def test_training_overfits_a_fixed_batch(dev):
    """End-to-end training dynamics (tools/soak.py): RegionLoss + engine backward + SGD on one fixed synthetic batch
    must drive the loss down by more than an order of magnitude -- a sign or scale error anywhere in the gradient
    path shows up here even if it slipped through the per-kernel comparisons."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "soak.py"), "80", "8", "none"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = [l for l in r.stdout.splitlines() if l.startswith("ok:")][-1]
    first, final = (float(v) for v in last.split("loss")[1].replace("->", " ").split()[:2])
    print(last)
    assert final < 0.1 * first
