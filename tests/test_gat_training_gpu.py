"""End to end: examples/train_synthetic.py trains the reference's GAT (with full-neighbourhood evaluation blocks) and GCN models on
the API mirror, each in a fresh process, at the size of test_loader_gpu.py::test_example_training_script_runs, for one epoch."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra", [["--model_type", "gat", "--num_heads", "4", "--eval_fan_out=-1,-1"], ["--model_type", "gcn"]])
def test_example_training_script_runs_gat_and_gcn(extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), "--nodes", "60000", "--dim", "64",
                          "--batch_size", "256", "--epochs", "1", "--cache_size", "4", "--prefetch", "1"] + extra,
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    loss = re.search(r"final loss (\S+)", out.stdout)
    assert loss and math.isfinite(float(loss.group(1))), out.stdout[-2000:]
    assert "Test Acc" in out.stdout
