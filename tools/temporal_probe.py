#!/usr/bin/env python3
"""TemporalNeighborSampler beside NeighborSampler and LaborSampler on one graph (profiles/rNN_temporal_sampler.txt).

Per fan-out list and strategy: the time of one call between two HIP events around sample_begin (the call's kernels, and the host's
launches where those are slower; median of 20 calls after a warm-up, the samplers alternating in one process), and the mean number
of input nodes of a batch against the uniform sampler's.  The temporal call's window holds what the wrapper adds in front of the
kernels: torch.unique over the query times, its host read of the number of distinct times, and the pair codes.  Query times are
uniform over the range of the edge timestamps, so a row has half of its edges eligible on average.

  python tools/temporal_probe.py [--nodes 200000] [--degree 30] [--batch 1024] [--fanouts "5,5;10,10"]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import torch  # noqa: E402
from COALA_GNN.sampler import LaborSampler, NeighborSampler, TemporalNeighborSampler  # noqa: E402
from COALA_GNN.synthetic import edge_times, powerlaw_csc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=200_000)
ap.add_argument("--degree", type=float, default=30.0)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--fanouts", default="5,5;10,10")
ap.add_argument("--t_max", type=int, default=1 << 20)
args = ap.parse_args()

assert torch.cuda.is_available(), "temporal_probe needs the GPU"
torch.cuda.set_device(0)
N, B = args.nodes, args.batch
ip, ix = powerlaw_csc(N, args.degree, seed=1, device="cuda")
ts = edge_times(ip, seed=2, t_max=args.t_max)
print(f"graph: powerlaw, {N} nodes, {ix.numel()} edges, max in-degree {int((ip[1:] - ip[:-1]).max())}; batch {B}; "
      f"edge and query times uniform over [0, {args.t_max})")
g = NeighborSampler([1]).make_graph(ip, ix, edata={"ts": ts})
perm = torch.randperm(N, generator=torch.Generator().manual_seed(0)).cuda()
query = torch.randint(0, args.t_max, (N,), generator=torch.Generator().manual_seed(1)).cuda()
n_batches = min(16, N // B)


def begin(smp, s):
    seeds = perm[(s % n_batches) * B: (s % n_batches + 1) * B]
    if isinstance(smp, TemporalNeighborSampler):
        return smp.sample_begin(g, seeds, step=s, seed_times=query[seeds])
    return smp.sample_begin(g, seeds, step=s)


def one_call_ms(smp, s):
    """One call between two events on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    pending = begin(smp, s)
    b.record()
    smp.sample_end(pending)
    b.synchronize()
    return a.elapsed_time(b)


for fan in [[int(f) for f in part.split(",")] for part in args.fanouts.split(";")]:
    kinds = {"NeighborSampler": NeighborSampler(fan, seed=1), "LaborSampler": LaborSampler(fan, seed=1),
             "Temporal uniform": TemporalNeighborSampler(fan, strategy="uniform", seed=1, edge_ids=False),
             "Temporal last": TemporalNeighborSampler(fan, strategy="last", seed=1, edge_ids=False),
             "Temporal uniform + ids": TemporalNeighborSampler(fan, strategy="uniform", seed=1, edge_ids=True)}
    print(f"fan-outs {fan}")
    stats = {}
    for name, smp in kinds.items():
        n_in, n_distinct = [], []
        for s in range(n_batches):
            inp, _, _ = smp.sample_end(begin(smp, s))
            n_in.append(inp.numel())
            n_distinct.append(int(torch.unique(inp).numel()))
        stats[name] = (statistics.mean(n_in), statistics.mean(n_distinct))
    base = stats["NeighborSampler"][0]
    for name, smp in kinds.items():
        for s in range(10):
            one_call_ms(smp, s)
    times = {name: [] for name in kinds}
    for s in range(20):            # alternating calls
        for name, smp in kinds.items():
            times[name].append(one_call_ms(smp, s) * 1e3)
    print("  sampler                     input nodes  (ratio)  distinct ids   us per call (HIP events), median of 20 [min .. max]")
    for name in kinds:
        v = times[name]
        print(f"  {name:26s} {stats[name][0]:10.0f}  ({stats[name][0] / base:.3f})  {stats[name][1]:10.0f}    {statistics.median(v):8.1f}  [{min(v):.1f} .. {max(v):.1f}]")
    t, lab = statistics.median(times["Temporal uniform"]), statistics.median(times["LaborSampler"])
    print(f"  condition: a temporal call is below LaborSampler's at the same fan-outs: {'held' if t < lab else 'NOT held'} ({t:.1f} against {lab:.1f} us)")
g.close()
print("done")
