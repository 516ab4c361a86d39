#!/usr/bin/env python3
"""Bit comparison of the owner partition of two builds (profiles/r26_owner_partition.txt).

COALA_PARENT_LIB=<libcoala_hip.so of another commit> is loaded beside this build's library in one process (ctypes, side by side, as in
tools/attention_ab_probe.py).  The Python classes reach the library through their module's `_lib`; the probe points that name at one
library or the other, so a handle is created, driven and destroyed by the same one.  Compared with torch.equal, every output buffer whole
(prefilled with -1):
  - coala_cache_route at the shapes of tests/test_cache_gpu.py: 16,641 ids below and above 2^32 at 3 / 17 / 33 / 64 parts, packed and
    [parts][n] layout; 4096 * 1024 + 257 ids at 5 parts, packed;
  - one NeighborSampler([5, 5], bucket_by_owner=8) minibatch of 1024 seeds: every block tensor, the owner counts on device and host.
    COALA_PARENT_LIB=/path/to/parent/libcoala_hip.so python tools/partition_ab_probe.py"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import COALA_GNN_Pybind as P  # noqa: E402
import COALA_GNN.sampler as S  # noqa: E402
from COALA_GNN.synthetic import alloc_pinned_table, powerlaw_csc  # noqa: E402
from COALA_GNN_Pybind import _capi  # noqa: E402

if not os.environ.get("COALA_PARENT_LIB"):
    raise SystemExit(__doc__)
new = _capi.load()
par = C.CDLL(os.environ["COALA_PARENT_LIB"])
if par._handle == new._handle:
    raise SystemExit("COALA_PARENT_LIB is the library under test: dlopen handed back the same handle and every comparison would hold vacuously")
for name, (res, args) in _capi.SYMBOLS.items():
    getattr(par, name).restype, getattr(par, name).argtypes = res, args

torch.cuda.set_device(0)
table = alloc_pinned_table(64, 128, seed=1, device=0)  # the cold tier of the route handles (route never reads it)


def route(lib, idx, parts, stride):
    """coala_cache_route of one library on a handle of its own -> {name: tensor}."""
    P._lib = lib
    n = idx.numel()
    cache = P.Isolated_Cache(P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, 128, True), None, 0, 1, 1, table.device_ptr, num_rows=64)
    out = {k: torch.full((stride * parts if stride else n,), -1, dtype=torch.int64, device="cuda") for k in ("node_out", "map_out")}
    out["counts"] = torch.full((parts,), -1, dtype=torch.int64, device="cuda")
    out["offsets"] = torch.full((parts + 1,), -1, dtype=torch.int64, device="cuda")
    cache.route(idx.data_ptr(), n, parts, out["node_out"].data_ptr(), out["map_out"].data_ptr(), out["counts"].data_ptr(),
                out["offsets"].data_ptr(), stride)
    torch.cuda.synchronize()
    cache.close()
    return out


def minibatch(lib, d_ip, d_ix, seeds):
    """One bucketed [5, 5] minibatch from one library on a graph handle of its own -> {name: tensor or list}."""
    S._lib = lib
    smp = S.NeighborSampler([5, 5], seed=26, bucket_by_owner=8)
    g = smp.make_graph(d_ip, d_ix)
    input_nodes, _, blocks = smp.sample(g, seeds, step=3)
    torch.cuda.synchronize()
    out = {"input_nodes": input_nodes, "owner_counts": blocks[0].owner_counts, "owner_counts_host": torch.tensor(blocks[0].owner_counts_host),
           "dst_in_src": blocks[0].dst_in_src}
    for l, b in enumerate(blocks):
        out[f"block {l} src_nodes"], out[f"block {l} nbr"] = b.src_nodes, b.nbr
    g.close()
    return out


def compare(title, got):
    lines = [f"{k} {'equal' if torch.equal(got[0][k], got[1][k]) else 'DIFFERENT'}" for k in got[0]]
    print(f"{title:44s} " + ", ".join(lines))
    return sum("DIFFERENT" in x for x in lines)


bad = 0
n = 64 * 256 + 257
for parts in (3, 17, 33, 64):
    rng = np.random.default_rng(parts)
    ids = np.concatenate([rng.integers(0, 2**32, size=n // 2, dtype=np.int64), rng.integers(2**32, 2**62, size=n - n // 2, dtype=np.int64)])
    idx = torch.from_numpy(rng.permutation(ids)).cuda()
    for stride in (0, n):
        bad += compare(f"route n={n} parts={parts} stride={stride}", [route(lib, idx, parts, stride) for lib in (par, new)])
n = 4096 * 1024 + 257
idx = torch.from_numpy(np.random.default_rng(5).integers(0, 2**40, size=n, dtype=np.int64)).cuda()
bad += compare(f"route n={n} parts=5 stride=0", [route(lib, idx, 5, 0) for lib in (par, new)])
d_ip, d_ix = powerlaw_csc(200_000, 12.0, seed=8, device="cuda")
seeds = torch.from_numpy(np.random.default_rng(1).permutation(200_000)[:1024].astype(np.int64)).cuda()
bad += compare("NeighborSampler([5, 5], bucket_by_owner=8)", [minibatch(lib, d_ip, d_ix, seeds) for lib in (par, new)])
P._lib = S._lib = new
table.close()
print("done: every output equal bit for bit" if not bad else f"FAILED: {bad} outputs differ")
sys.exit(1 if bad else 0)
