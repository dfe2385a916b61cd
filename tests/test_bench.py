"""bench.py's command line: a plain run prints the headline line only and
`--dump-outputs` writes the logits of its last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("eager_forward_us", "roofline", "forward_kernels", "ops", "train_step_ms", "setup_ms", "cpu_baseline",
             "cpu_stock_csr", "gpu_stock", "configs", "config5_column_sharded")


def test_bench_options_and_step_count_checked():
    """--full and --dump-outputs exist; --steps 0 is refused before any GPU call."""
    h = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    z = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert z.returncode == 2 and "--steps" in z.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--no-graph"]], ids=["graph", "eager"])
def test_bench_plain_run_line_and_dumped_logits(extra, r8, tmp_path):
    """One plain run (15 steps, 5 per graph): the line holds the headline keys
    with ms_per_step consistent with value, none of the --full legs, and
    DIR/logits.npy is the float32 [N x 8] forward of the seeded model, within
    the suite's 1e-4 of the oracle on the same weights."""
    import torch
    import gcn_amd  # noqa: F401
    from graph_convolutional_networks_for_text_classification_amd import GCN
    from oracle import gcn_ref
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "15", "--warmup", "5", "--dump-outputs", out]
                       + extra, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 15 and d["warmup"] == 5 and d["unit"] == "edges/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["full"] is False and d["ms_per_step"] > 0
    assert d["config"]["forwards_per_graph"] == (1 if extra else 5)
    assert d["value"] == pytest.approx(2 * d["config"]["adj_nnz"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in d]
    assert os.listdir(out) == ["logits.npy"]
    z = np.load(os.path.join(out, "logits.npy"))
    assert z.dtype == np.float32 and z.shape == (r8["nodes"], r8["nclass"])
    torch.manual_seed(0)
    model = GCN(nfeat=r8["nfeat"], nhid=200, nclass=r8["nclass"], dropout=0.5)
    ref = gcn_ref.RefGCN(nfeat=r8["nfeat"], nhid=200, nclass=r8["nclass"], dropout=0.5).eval()
    ref.load_state_dict(model.state_dict())
    with torch.no_grad():
        want = ref(r8["features"], r8["adj"]).numpy()
    assert np.abs(z - want).max() <= 1e-4
