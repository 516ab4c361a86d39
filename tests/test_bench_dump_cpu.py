"""bench.py --dump-outputs without a GPU: dump_outputs() on CPU tensors shaped like a minibatch fetch's return (input_nodes, seeds,
blocks, features).  Float32 / float64 files only, never more than the limit in all, and a fixed sample of rows when the features do not fit.
bench.py is imported in a child process: importing it places the process on its GPU's NUMA node (COALA_NUMA=off here)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys
import torch
import bench
n, dim, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
g = torch.Generator().manual_seed(7)
ids = torch.randperm(10 * n, generator=g)[:n]
feat = torch.rand((n, dim), generator=g, dtype=torch.float32)
print(json.dumps({"limit": bench.DUMP_LIMIT_BYTES, "shapes": bench.dump_outputs(out, (ids, ids[:16], [None]), feat)}))
"""


def _dump(tmp_path, name, n, dim):
    out = str(tmp_path / name)
    env = dict(os.environ, COALA_NUMA="off")
    r = subprocess.run([sys.executable, "-c", CHILD, str(n), str(dim), out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    files = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= d["limit"]
    return d, files


def _expected(n, dim):
    import torch
    g = torch.Generator().manual_seed(7)
    ids = torch.randperm(10 * n, generator=g)[:n]
    feat = torch.rand((n, dim), generator=g, dtype=torch.float32)
    return ids.numpy(), feat.numpy()


def test_small_fetch_is_written_whole(tmp_path):
    d, files = _dump(tmp_path, "small", 3000, 64)
    ids, feat = _expected(3000, 64)
    assert set(files) == {"input_nodes", "seeds", "features"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert files["input_nodes"].dtype == np.float64 and np.array_equal(files["input_nodes"], ids.astype(np.float64))
    assert np.array_equal(files["seeds"], ids[:16].astype(np.float64))
    assert files["features"].dtype == np.float32 and np.array_equal(files["features"], feat)
    assert d["shapes"]["features"] == [3000, 64]


def test_large_fetch_is_a_fixed_sample_under_the_limit(tmp_path):
    n, dim = 20000, 1024                                   # 82 MB of features: more than the limit
    d, files = _dump(tmp_path, "large", n, dim)
    ids, feat = _expected(n, dim)
    assert set(files) == {"input_nodes", "seeds", "features", "feature_rows"}
    rows = files["feature_rows"]
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and rows[-1] < n
    assert files["features"].shape == (len(rows), dim) and len(rows) > n // 2
    assert np.array_equal(files["features"], feat[rows.astype(np.int64)])
    # the sample depends on nothing but the shape and the seed: the same rows in every run
    assert np.array_equal(rows, np.sort(np.random.default_rng(0).choice(n, size=len(rows), replace=False)).astype(np.float64))
