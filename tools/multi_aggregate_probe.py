#!/usr/bin/env python3
"""Multi-statistic aggregation beside the composed path on the input block of a sampled minibatch (profiles/r31_multi_aggregate.txt).

Per fan-out list and row length, mean / max / min / std of the neighbours' rows three ways, each through autograd as a layer calls it:
  native     Block.multi_aggregate(h, ('mean', 'max', 'min', 'std')): one kernel forward, one backward
  composed   the single-statistic native ops: mean_aggregate(h), max_aggregate(h), -max_aggregate(-h) and
             sqrt(relu(mean_aggregate(h * h) - mean^2) + eps), stacked: four gathers forward, four atomic scatters backward
  torch      Block.multi_aggregate_torch
Times are device-event medians of `--rounds` rounds in which the variants take turns, `--reps` calls per timed window; forward alone
(no gradient asked for) and forward + backward; and the peak allocation above the resident tensors of one forward + backward.

  python tools/multi_aggregate_probe.py [--nodes 200000] [--degree 30] [--batch 1024] [--fanouts "5,5;10,10"] [--dims 128,1024]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import torch  # noqa: E402
from COALA_GNN.sampler import NeighborSampler  # noqa: E402
from COALA_GNN.synthetic import powerlaw_csc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=200_000)
ap.add_argument("--degree", type=float, default=30.0)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--fanouts", default="5,5;10,10")
ap.add_argument("--dims", default="128,1024")
ap.add_argument("--reps", type=int, default=200, help="calls per timed window")
ap.add_argument("--rounds", type=int, default=20, help="timed windows per variant; the variants take turns")
args = ap.parse_args()

AGGS, EPS = ("mean", "max", "min", "std"), 1e-5
torch.cuda.set_device(0)
N, B = args.nodes, args.batch
ip, ix = powerlaw_csc(N, args.degree, seed=1, device="cuda")
print(f"graph: powerlaw, {N} nodes, {ix.numel()} edges, max in-degree {int((ip[1:] - ip[:-1]).max())}; batch {B}; aggregators {AGGS}")
seeds = torch.randperm(N, generator=torch.Generator().manual_seed(0))[:B].cuda()


def timed(fn, reps):
    """us per call over `reps` calls, by device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def composed(blk, h):
    mean = blk.mean_aggregate(h)
    var = blk.mean_aggregate(h * h) - mean * mean
    return torch.stack([mean, blk.max_aggregate(h), -blk.max_aggregate(-h), torch.sqrt(torch.relu(var) + EPS)], 1)


for fan in [[int(f) for f in part.split(",")] for part in args.fanouts.split(";")]:
    smp = NeighborSampler(fan, seed=1)
    g = smp.make_graph(ip, ix)
    _, _, blocks = smp.sample(g, seeds)
    blk = blocks[0]
    n_dst, edges = blk.num_dst, int((blk.nbr >= 0).sum())
    for dim in [int(d) for d in args.dims.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(dim)
        h = torch.randn(blk.num_src, dim, device="cuda", generator=gen)
        go = torch.randn(n_dst, len(AGGS), dim, device="cuda", generator=gen)
        hg = h.clone().requires_grad_(True)
        variants = {"native": lambda x: blk.multi_aggregate(x, AGGS, EPS), "composed": lambda x: composed(blk, x),
                    "torch": lambda x: blk.multi_aggregate_torch(x, AGGS, EPS)}

        def fwd_bwd(f):
            hg.grad = None
            (f(hg) * go).sum().backward()

        ops = {}
        for name, f in variants.items():
            ops[f"{name} forward"] = lambda f=f: f(h)
            ops[f"{name} forward + backward"] = lambda f=f: fwd_bwd(f)
        ref = variants["torch"](h)
        for name in ("native", "composed"):
            print(f"  largest difference of {name} from the torch path: {float((variants[name](h) - ref).abs().max()):.3e}")
        reps = {k: (args.reps if "torch" not in k else max(args.reps // 5, 2)) for k in ops}
        peak = {}
        for k, fn in ops.items():      # warm-up, and the peak allocation of one call above what is resident
            timed(fn, 3)
            hg.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[k] = (torch.cuda.max_memory_allocated() - base) / 1e6
        times = {k: [] for k in ops}
        for r in range(args.rounds):
            for k, fn in ops.items():
                times[k].append(timed(fn, reps[k]))
        print(f"fan-out {fan}, input block: {n_dst} dst rows, {blk.num_src} src rows, {edges} edges, dim {dim}")
        print(f"  bytes: gathered rows {edges * dim * 4 / 1e6:.1f} MB, out [n_dst, 4, dim] {n_dst * 4 * dim * 4 / 1e6:.1f} MB, grad_src {blk.num_src * dim * 4 / 1e6:.1f} MB")
        print(f"  variant                          us per call, median of {args.rounds} windows [min .. max]   peak allocation of a call")
        med = {}
        for k, v in times.items():
            med[k] = statistics.median(v)
            print(f"  {k:32s} {med[k]:9.1f}  [{min(v):.1f} .. {max(v):.1f}]  ({reps[k]} calls per window)   {peak[k]:8.1f} MB")
        print(f"  ratios: composed / native forward {med['composed forward'] / med['native forward']:.2f}, forward + backward "
              f"{med['composed forward + backward'] / med['native forward + backward']:.2f}; torch / native forward "
              f"{med['torch forward'] / med['native forward']:.1f}, forward + backward "
              f"{med['torch forward + backward'] / med['native forward + backward']:.1f}")
    g.close()
print("done")
