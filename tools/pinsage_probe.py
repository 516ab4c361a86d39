#!/usr/bin/env python3
"""RandomWalkNeighborSampler beside NeighborSampler on one graph (profiles/r14_pinsage_sampler.txt).

Per k list (k,k) and walk setting -- DGL's example (T = 2, W = 10, p = 0.5) and a heavy one (T = 8, W = 64, p = 0.25): the time of one
call between two HIP events around sample_begin (the call's kernels, and the host's launches where those are slower; median of 20 calls
after a warm-up, the samplers alternating), the mean number of input nodes of a batch, the mean valid entries per row, and -- through
a COALA_GNN_DataLoader with no model behind it -- the wall time of a loader step (sample + fetch) and the fetch time the loader
records per step.

  python tools/pinsage_probe.py [--nodes 200000] [--degree 30] [--dim 1024] [--batch 1024] [--cache_mb 64]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, SSD_INFO  # noqa: E402
from COALA_GNN.sampler import NeighborSampler, RandomWalkNeighborSampler  # noqa: E402
from COALA_GNN.synthetic import alloc_pinned_table, block_colors, powerlaw_csc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=200_000)
ap.add_argument("--degree", type=float, default=30.0)
ap.add_argument("--dim", type=int, default=1024)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--cache_mb", type=int, default=64)
ap.add_argument("--ks", default="5,5;10,10")
ap.add_argument("--steps", type=int, default=40, help="loader steps per pass")
args = ap.parse_args()

torch.cuda.set_device(0)
N, B = args.nodes, args.batch
ip, ix = powerlaw_csc(N, args.degree, seed=1, device="cuda")
print(f"graph: powerlaw, {N} nodes, {ix.numel()} edges, max in-degree {int((ip[1:] - ip[:-1]).max())}; batch {B}; "
      f"features {args.dim} fp32 in pinned host memory, cache {args.cache_mb} MB")
g = NeighborSampler([1]).make_graph(ip, ix)
perm = torch.randperm(N, generator=torch.Generator().manual_seed(0)).cuda()
n_batches = min(16, N // B)

table = alloc_pinned_table(N, args.dim, seed=3, device=0)
tmp = tempfile.mkdtemp()
color, tk, sc, _ = block_colors(N)
files = [os.path.join(tmp, f) for f in ("color.npy", "topk.npy", "score.npy")]
for f, a in zip(files, (color, tk, sc)):
    np.save(f, a)
comm = MPI_Comm_Manager(0)
comm.initialize_nested_process_group("isolated")
ids = torch.randperm(int(0.6 * N), generator=torch.Generator().manual_seed(0))
ids = ids[: min(len(ids) // B, args.steps + 6) * B]


def one_call_ms(smp, s):
    """One call between two events on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    pending = smp.sample_begin(g, perm[(s % n_batches) * B: (s % n_batches + 1) * B], step=s)
    b.record()
    smp.sample_end(pending)
    b.synchronize()
    return a.elapsed_time(b)


def loader_pass(smp, fan):
    """One pass over the loader with nothing behind it: (wall ms per step, the loader's own fetch ms per step, rows per step)."""
    nd = Node_Distributor(comm, ids, B, *files, parsing_method="baseline")
    smp.step = 0
    loader = COALA_GNN_DataLoader(SSD_INFO(1, args.dim * 4, 1024, 0), nd, g, smp, B, args.dim, fan, args.cache_mb, "cuda:0",
                                  cache_backend="isolated", sim_buf=table, num_rows=N, shuffle=False)
    it = iter(loader)
    for _ in range(5):            # warm-up: allocations, the cache's first fills
        next(it)
    loader.COALA_GNN_Manager.get_aggregate_time()
    loader.COALA_GNN_Manager.aggregation_timer = 0.0
    torch.cuda.synchronize()
    n = rows = 0
    t0 = time.perf_counter()
    for input_nodes, _, _, feat in it:
        n += 1
        rows += input_nodes.numel()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / n * 1e3
    fetch = loader.COALA_GNN_Manager.get_aggregate_time() / n * 1e3
    del loader, it
    return wall, fetch, rows / n


SETTINGS = (("walks T=2 W=10 p=0.5", 2, 10, 0.5), ("walks T=8 W=64 p=0.25", 8, 64, 0.25))
for ks in [[int(f) for f in part.split(",")] for part in args.ks.split(";")]:
    kinds = {"NeighborSampler": NeighborSampler(ks, seed=1)}
    for name, T, W, p in SETTINGS:
        kinds[name] = RandomWalkNeighborSampler(ks, T, p, W, seed=1)
    print(f"k {ks}")
    stats = {}
    for name, smp in kinds.items():
        n_in, valid, rows = [], 0, 0
        for b in range(n_batches):
            inp, _, blocks = smp.sample(g, perm[b * B: (b + 1) * B], step=b)
            n_in.append(inp.numel())
            for blk in blocks:
                valid += int((blk.nbr >= 0).sum())
                rows += blk.num_dst * blk.nbr.shape[1]
        stats[name] = (statistics.mean(n_in), valid / max(rows, 1))
    base = stats["NeighborSampler"][0]
    for name, smp in kinds.items():
        for s in range(10):
            one_call_ms(smp, s)
    times = {name: [] for name in kinds}
    for s in range(20):            # alternating calls
        for name, smp in kinds.items():
            times[name].append(one_call_ms(smp, s) * 1e3)
    print("  sampler                     input nodes  (ratio)   valid slots   us per call (HIP events), median of 20 [min .. max]")
    for name in kinds:
        v = times[name]
        print(f"  {name:26s} {stats[name][0]:10.0f}  ({stats[name][0] / base:.3f})   {stats[name][1]:8.3f}    {statistics.median(v):8.1f}  [{min(v):.1f} .. {max(v):.1f}]")
    loads = {name: [] for name in kinds}
    for r in range(3):            # alternating passes of the loader
        for name in loads:
            loads[name].append(loader_pass(kinds[name], ks))
    print("  loader step (sample + fetch), no model   rows/step   wall ms/step [min .. max]   fetch ms/step as the loader records it [min .. max]")
    for name, v in loads.items():
        w, f = [x[0] for x in v], [x[1] for x in v]
        print(f"  {name:26s} {v[0][2]:12.0f}   {statistics.median(w):8.3f} [{min(w):.3f} .. {max(w):.3f}]   {statistics.median(f):8.3f} [{min(f):.3f} .. {max(f):.3f}]")
g.close()
table.close()
print("done")
