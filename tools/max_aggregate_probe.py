#!/usr/bin/env python3
"""Max aggregation beside mean aggregation on the input block of a sampled minibatch (profiles/r10_max_aggregate.txt).

Per fan-out list and row length: the native max forward (with the argmax it saves for the backward, and without it) and backward,
the native mean forward and backward on the same block, and Block.max_aggregate_torch (forward, and forward + backward through
autograd).  The native ops are called through the C ABI on buffers allocated once, so a time is the kernel plus its launch; both
backwards include the memset of grad_src that their callers owe.  The ops alternate in blocks in one process; times come from device
events around a block of calls.

  python tools/max_aggregate_probe.py [--nodes 200000] [--degree 30] [--batch 1024] [--fanouts "5,5;10,10"] [--dims 128,1024]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import torch  # noqa: E402
from COALA_GNN.sampler import NeighborSampler  # noqa: E402
from COALA_GNN.synthetic import powerlaw_csc  # noqa: E402
from COALA_GNN_Pybind import _capi, current_stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=200_000)
ap.add_argument("--degree", type=float, default=30.0)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--fanouts", default="5,5;10,10")
ap.add_argument("--dims", default="128,1024")
ap.add_argument("--reps", type=int, default=2000, help="calls per block")
ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per op")
args = ap.parse_args()

torch.cuda.set_device(0)
L = _capi.load()
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
    smp = NeighborSampler(fan, seed=1)
    g = smp.make_graph(ip, ix)
    _, _, blocks = smp.sample(g, seeds)
    blk = blocks[0]
    nbr, n_dst, f = blk.nbr, blk.num_dst, blk.nbr.shape[1]
    edges = int((nbr >= 0).sum())
    for dim in [int(d) for d in args.dims.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(dim)
        h = torch.randn(blk.num_src, dim, device="cuda", generator=gen)
        go = torch.randn(n_dst, dim, device="cuda", generator=gen)
        out, arg, gs = torch.empty_like(go), torch.empty(n_dst, dim, dtype=torch.int32, device="cuda"), torch.zeros_like(h)
        st, P = current_stream(), lambda t: t.data_ptr()
        hg = h.clone().requires_grad_(True)

        def torch_fb():
            hg.grad = None
            (blk.max_aggregate_torch(hg) * go).sum().backward()

        def max_bwd():
            gs.zero_()
            _capi.check(L.coala_block_max_aggregate_backward(0, P(arg), P(go), P(gs), n_dst, dim, st))

        def mean_bwd():
            gs.zero_()
            _capi.check(L.coala_block_mean_aggregate_backward(0, P(nbr), P(go), P(gs), n_dst, f, dim, st))

        ops = {
            "max forward (with arg)": lambda: _capi.check(L.coala_block_max_aggregate(0, P(nbr), P(h), P(out), P(arg), n_dst, f, dim, st)),
            "max forward (arg = null)": lambda: _capi.check(L.coala_block_max_aggregate(0, P(nbr), P(h), P(out), None, n_dst, f, dim, st)),
            "mean forward": lambda: _capi.check(L.coala_block_mean_aggregate(0, P(nbr), P(h), P(out), n_dst, f, dim, st)),
            "max backward (+ memset)": max_bwd,
            "mean backward (+ memset)": mean_bwd,
            "max_aggregate_torch forward": lambda: blk.max_aggregate_torch(h),
            "max_aggregate_torch forward + backward": torch_fb,
        }
        assert torch.equal(blk.max_aggregate(h), blk.max_aggregate_torch(h)), "the native forward differs from the torch path"
        reps = {k: (args.reps if "torch" not in k else max(args.reps // 10, 5)) for k in ops}
        for k, fn in ops.items():      # warm-up (the max forward first: the backward reads its arg)
            timed(fn, 10)
        times = {k: [] for k in ops}
        for r in range(args.blocks):
            for k, fn in ops.items():
                times[k].append(timed(fn, reps[k]))
        print(f"fan-out {fan}, input block: {n_dst} dst rows, {blk.num_src} src rows, {edges} edges, dim {dim}")
        print(f"  bytes: gathered rows {edges * dim * 4 / 1e6:.1f} MB, one [n_dst, dim] array {n_dst * dim * 4 / 1e6:.1f} MB, grad_src {blk.num_src * dim * 4 / 1e6:.1f} MB")
        print(f"  op                                       us per call, median of {args.blocks} x reps [min .. max]")
        med = {}
        for k, v in times.items():
            med[k] = statistics.median(v)
            print(f"  {k:40s} {med[k]:9.1f}  [{min(v):.1f} .. {max(v):.1f}]  ({reps[k]} calls per block)")
        print(f"  ratios: max fwd / mean fwd {med['max forward (with arg)'] / med['mean forward']:.2f} (arg = null: "
              f"{med['max forward (arg = null)'] / med['mean forward']:.2f}), max bwd / mean bwd "
              f"{med['max backward (+ memset)'] / med['mean backward (+ memset)']:.2f}, torch fwd / native fwd "
              f"{med['max_aggregate_torch forward'] / med['max forward (with arg)']:.1f}, torch fwd+bwd / native fwd+bwd "
              f"{med['max_aggregate_torch forward + backward'] / (med['max forward (with arg)'] + med['max backward (+ memset)']):.1f}")
    g.close()
print("done")
