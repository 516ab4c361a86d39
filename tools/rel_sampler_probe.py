#!/usr/bin/env python3
"""RelNeighborSampler beside NeighborSampler and LaborSampler on one typed graph: the time of one sample() call
(profiles/r12_rel_sampler.txt).

Per sampler: HIP events around sample() on the current stream (the call returns when the host has the counts), the median of
--reps calls after --warmup calls, the samplers alternating call by call over the same batches; and the mean number of edges and
input nodes of a batch.  The graph is powerlaw_csc typed by the source node (id % num_rels) and sorted by sort_csc_by_etype.

  python tools/rel_sampler_probe.py [--nodes 200000] [--degree 30] [--batch 1024] [--num_rels 4]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import torch  # noqa: E402
from COALA_GNN.sampler import LaborSampler, NeighborSampler, RelNeighborSampler, sort_csc_by_etype  # noqa: E402
from COALA_GNN.synthetic import edge_types_by_source, powerlaw_csc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=200_000)
ap.add_argument("--degree", type=float, default=30.0)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--num_rels", type=int, default=4)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()

torch.cuda.set_device(0)
N, B, R = args.nodes, args.batch, args.num_rels
ip, ix = powerlaw_csc(N, args.degree, seed=1, device="cuda")
ix, et, _ = sort_csc_by_etype(ip, ix, edge_types_by_source(ix, R))
g = NeighborSampler.make_graph(ip, ix, edata={"etype": et})
print(f"graph: power-law, {N} nodes, {ix.numel()} edges, max in-degree {g.max_in_degree}, {R} relations (source id % {R}), sorted by type; "
      f"batch {B}; median of {args.reps} calls after {args.warmup}, HIP events around sample()")
perm = torch.randperm(N, generator=torch.Generator().manual_seed(0)).cuda()
n_batches = max(1, min(16, N // B))


def split(total):
    return [total // R + (1 if r < total % R else 0) for r in range(R)]


for total in (10, 30):
    kinds = {f"RelNeighborSampler {[split(total)] * 2}": RelNeighborSampler([split(total)] * 2, R, seed=1),
             f"NeighborSampler [{total}, {total}] edge_ids": NeighborSampler([total, total], seed=1, edge_ids=True)}
    if total == 10:
        kinds["LaborSampler [10, 10] edge_ids"] = LaborSampler([10, 10], seed=1, edge_ids=True)
    times = {k: [] for k in kinds}
    sizes = {k: [0, 0] for k in kinds}
    for s in range(args.warmup + args.reps):
        for name, smp in kinds.items():
            seeds = perm[(s % n_batches) * B: (s % n_batches + 1) * B]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            inp, _, blocks = smp.sample(g, seeds, step=s)
            b.record()
            b.synchronize()
            if s >= args.warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
                sizes[name][0] += inp.numel()
                sizes[name][1] += sum(int((blk.nbr >= 0).sum()) if blk.nbr is not None else blk.indices.numel() for blk in blocks)
    print(f"per-layer total {total}:")
    for name, v in times.items():
        print(f"  {name:46s} {statistics.median(v):8.1f} us  [{min(v):.1f} .. {max(v):.1f}]   input nodes {sizes[name][0] / args.reps:9.0f}   "
              f"edges {sizes[name][1] / args.reps:9.0f}")
g.close()
print("done")
