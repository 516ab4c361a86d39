#!/usr/bin/env python3
"""The relation-typed sum beside its torch fallback and the weighted sum on the input block of a sampled minibatch
(profiles/r10_rel_sum_aggregate.txt).

Per fan-out list, row length and number of relations R: forward, and forward + backward (gradients for h_src and w), of
Block.rel_sum_aggregate (the native kernels), of Block.rel_sum_aggregate_torch (gather, multiply, index_add into n_dst * R rows) and of
Block.weighted_sum_aggregate (the native kernel without types: the floor, it moves the same rows and writes 1 / R of the output).  All
three are called as a model calls them, through autograd, so a time holds the op's allocations and, for a backward, the memset of
grad_src.  The edge types are the source's id modulo R (synthetic.edge_types_by_source).  The ops alternate in blocks in one process;
times come from device events around a block of calls, after a warm-up; the median over the blocks is reported.

  python tools/rel_sum_probe.py [--nodes 200000] [--degree 30] [--batch 1024] [--fanouts "5,5;10,10"] [--dims 128,1024] [--rels 1,4,8]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import torch  # noqa: E402
from COALA_GNN.sampler import NeighborSampler  # noqa: E402
from COALA_GNN.synthetic import edge_types_by_source, powerlaw_csc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=200_000)
ap.add_argument("--degree", type=float, default=30.0)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--fanouts", default="5,5;10,10")
ap.add_argument("--dims", default="128,1024")
ap.add_argument("--rels", default="1,4,8")
ap.add_argument("--reps", type=int, default=300, help="calls per block (a tenth of it for the torch fallback)")
ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per op")
args = ap.parse_args()

torch.cuda.set_device(0)
N, B = args.nodes, args.batch
ip, ix = powerlaw_csc(N, args.degree, seed=1, device="cuda")
print(f"graph: powerlaw, {N} nodes, {ix.numel()} edges, max in-degree {int((ip[1:] - ip[:-1]).max())}; batch {B}")
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


for fan in [[int(f) for f in part.split(",")] for part in args.fanouts.split(";")]:
    smp = NeighborSampler(fan, seed=1, edge_ids=True)
    g = smp.make_graph(ip, ix)
    _, _, blocks = smp.sample(g, seeds)
    blk = blocks[0]
    n_dst, edges = blk.num_dst, int((blk.nbr >= 0).sum())
    src_id = blk.src_nodes[blk.nbr.clamp_min(0).long()]
    for dim in [int(d) for d in args.dims.split(",")]:
        for R in [int(r) for r in args.rels.split(",")]:
            gen = torch.Generator(device="cuda").manual_seed(dim + R)
            et = edge_types_by_source(src_id, R).to(torch.int32)
            h = torch.randn(blk.num_src, dim, device="cuda", generator=gen).requires_grad_(True)
            w = torch.rand(blk.nbr.shape, device="cuda", generator=gen).requires_grad_(True)
            go = torch.randn(n_dst, R, dim, device="cuda", generator=gen)
            go1 = go[:, 0].contiguous()

            def both(op, grad):
                def run():
                    h.grad = w.grad = None
                    (op() * grad).sum().backward()
                return run

            native = lambda: blk.rel_sum_aggregate(h, et, R, w)              # noqa: E731
            fallback = lambda: blk.rel_sum_aggregate_torch(h, et, R, w)      # noqa: E731
            wsum = lambda: blk.weighted_sum_aggregate(h, w)                   # noqa: E731
            ops = {
                "rel_sum forward": lambda: native().detach(),
                "rel_sum_torch forward": lambda: fallback().detach(),
                "weighted_sum forward": lambda: wsum().detach(),
                "rel_sum forward + backward": both(native, go),
                "rel_sum_torch forward + backward": both(fallback, go),
                "weighted_sum forward + backward": both(wsum, go1),
            }
            with torch.no_grad():
                a, b = native(), fallback()
                assert torch.allclose(a, b, rtol=1e-4, atol=1e-4), "the native forward differs from the torch path"
            assert "RelSum" in type(native().grad_fn).__name__, "not the native op"
            reps = {k: (args.reps if "torch" not in k else max(args.reps // 10, 5)) for k in ops}
            for k, fn in ops.items():
                timed(fn, 10)
            times = {k: [] for k in ops}
            for _ in range(args.blocks):
                for k, fn in ops.items():
                    times[k].append(timed(fn, reps[k]))
            print(f"fan-out {fan}, input block: {n_dst} dst rows, {blk.num_src} src rows, {edges} edges, dim {dim}, R {R}")
            print(f"  bytes: gathered rows {edges * dim * 4 / 1e6:.1f} MB, out [n_dst, R, dim] {n_dst * R * dim * 4 / 1e6:.1f} MB, "
                  f"grad_src {blk.num_src * dim * 4 / 1e6:.1f} MB")
            print(f"  op                                       us per call, median of {args.blocks} x reps [min .. max]")
            med = {}
            for k, v in times.items():
                med[k] = statistics.median(v)
                print(f"  {k:40s} {med[k]:9.1f}  [{min(v):.1f} .. {max(v):.1f}]  ({reps[k]} calls per block)")
            print(f"  ratios: torch / native forward {med['rel_sum_torch forward'] / med['rel_sum forward']:.2f}, torch / native forward + backward "
                  f"{med['rel_sum_torch forward + backward'] / med['rel_sum forward + backward']:.2f}; native / weighted_sum forward "
                  f"{med['rel_sum forward'] / med['weighted_sum forward']:.2f}, forward + backward "
                  f"{med['rel_sum forward + backward'] / med['weighted_sum forward + backward']:.2f}")
    g.close()
print("done")
