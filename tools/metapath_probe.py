#!/usr/bin/env python3
"""Typed (metapath) walks beside the untyped ones at equal hops on one graph (profiles/r28_metapath_walk.txt).

pinsage_probe.py's method: HIP events around the call, median of 20 calls after a warm-up, the variants alternating in one process.
Graph: powerlaw_csc with edge types indices % 2, sorted by type; metapath [0, 1].  Pairs: the sampler call at DGL's example setting
(2 traversals of the metapath = 4 hops, W = 10, p = 0.5, k = 5,5) beside the untyped call at T = 4; random_walk of 4 hops; a walk batch.

  python tools/metapath_probe.py [--nodes 200000] [--degree 30] [--batch 1024]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import torch  # noqa: E402
from COALA_GNN.sampler import CSCGraph, RandomWalkNeighborSampler, random_walk, sort_csc_by_etype, walk_batch_begin, walk_batch_end  # noqa: E402
from COALA_GNN.synthetic import edge_types_by_source, powerlaw_csc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=200_000)
ap.add_argument("--degree", type=float, default=30.0)
ap.add_argument("--batch", type=int, default=1024)
args = ap.parse_args()

torch.cuda.set_device(0)
N, B, PATH = args.nodes, args.batch, [0, 1]
ip, ix = powerlaw_csc(N, args.degree, seed=1, device="cuda")
ix, et, _ = sort_csc_by_etype(ip, ix, edge_types_by_source(ix, 2))
g = CSCGraph(ip, ix, edata={"etype": et})
print(f"graph: powerlaw, {N} nodes, {ix.numel()} edges, 2 relations, max in-degree {g.max_in_degree}; {B} seeds; metapath {PATH}")
perm = torch.randperm(N, generator=torch.Generator().manual_seed(0)).cuda()
n_batches = min(16, N // B)


def seeds(s):
    return perm[(s % n_batches) * B: (s % n_batches + 1) * B]


def sampler_call(smp):
    def call(s):
        return lambda: smp.sample_begin(g, seeds(s), step=s), smp.sample_end
    return call


def trace_call(**kw):
    return lambda s: (lambda: random_walk(g, seeds(s), 4, 0.5, 10, seed=1, step=s, **kw), lambda _: None)


def batch_call(**kw):
    return lambda s: (lambda: walk_batch_begin(g, seeds(s)[:128], 1.0, 1.0, 20, 10, 1, seed=1, step=s, **kw), walk_batch_end)


def one_call_us(call, s):
    begin, end = call(s)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    pending = begin()
    b.record()
    end(pending)
    b.synchronize()
    return a.elapsed_time(b) * 1e3


PAIRS = (("sampler k=5,5 W=10 p=0.5, 4 hops", sampler_call(RandomWalkNeighborSampler([5, 5], 4, 0.5, 10, seed=1)),
          sampler_call(RandomWalkNeighborSampler([5, 5], 2, 0.5, 10, seed=1, metapath=PATH))),
         ("random_walk 4 hops x 10 walks", trace_call(), trace_call(metapath=PATH)),
         ("walk_batch 128 x 10 walks, L=20, K=1", batch_call(), batch_call(metapath=PATH)))
print("  call                                       untyped us [min .. max]      typed us [min .. max]     typed / untyped")
for name, plain, typed in PAIRS:
    for s in range(10):
        one_call_us(plain, s), one_call_us(typed, s)
    t = {"plain": [], "typed": []}
    for s in range(20):            # alternating calls
        t["plain"].append(one_call_us(plain, s))
        t["typed"].append(one_call_us(typed, s))
    mp, mt = statistics.median(t["plain"]), statistics.median(t["typed"])
    print(f"  {name:40s} {mp:8.1f} [{min(t['plain']):.1f} .. {max(t['plain']):.1f}]   {mt:8.1f} [{min(t['typed']):.1f} .. {max(t['typed']):.1f}]   {mt / mp:.2f}")
g.close()
print("done")
