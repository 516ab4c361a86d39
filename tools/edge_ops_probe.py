#!/usr/bin/env python3
"""The message-passing primitives beside their torch twins and the fused attention kernels on the input block of a sampled minibatch
(profiles/r32_edge_primitives.txt).

Per fan-out list and heads x dim, through autograd as a layer calls them:
  chain native    u_mul_e_sum(v, edge_softmax(u_dot_v(k, q) * scale)) on the native kernels
  chain torch     the same chain on the _torch twins (it materialises [E, H, D] twice)
  fused dot       Block.dot_gat_aggregate(q, k, v), one kernel each way
  fused gat       Block.gat_aggregate(el, er, v)
  u_dot_v / edge_softmax / u_mul_e_sum   each primitive alone, native and torch
Times are device-event medians of `--rounds` rounds in which the variants take turns, `--reps` calls per timed window, forward +
backward (and forward alone for the chain); and the peak allocation above the resident tensors of one forward + backward.

  python tools/edge_ops_probe.py [--nodes 200000] [--degree 30] [--batch 1024] [--fanouts "5,5;10,10"] [--shapes 4x128,4x32]"""
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
ap.add_argument("--shapes", default="4x128,4x32", help="heads x dim")
ap.add_argument("--reps", type=int, default=100, help="calls per timed window")
ap.add_argument("--rounds", type=int, default=20, help="timed windows per variant; the variants take turns")
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
    smp = NeighborSampler(fan, seed=1)
    g = smp.make_graph(ip, ix)
    _, _, blocks = smp.sample(g, seeds)
    blk = blocks[0]
    n_dst, edges = blk.num_dst, int((blk.nbr >= 0).sum())
    for H, D in [[int(x) for x in s.split("x")] for s in args.shapes.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(D)
        rand = lambda *shape: torch.randn(*shape, device="cuda", generator=gen).requires_grad_(True)
        q, k, v, el, er, e = rand(n_dst, H, D), rand(blk.num_src, H, D), rand(blk.num_src, H, D), rand(blk.num_src, H), rand(n_dst, H), rand(*blk.nbr.shape, H)
        scale = D ** -0.5
        chain = lambda t: lambda: getattr(blk, "u_mul_e_sum" + t)(v, getattr(blk, "edge_softmax" + t)(getattr(blk, "u_dot_v" + t)(k, q) * scale))
        fwd = {"fused dot": lambda: blk.dot_gat_aggregate(q, k, v, scale=scale), "fused gat": lambda: blk.gat_aggregate(el, er, v)}
        for t, name in (("", "native"), ("_torch", "torch")):
            fwd[f"chain {name}"] = chain(t)
            fwd[f"u_dot_v {name}"] = lambda t=t: getattr(blk, "u_dot_v" + t)(k, q)
            fwd[f"edge_softmax {name}"] = lambda t=t: getattr(blk, "edge_softmax" + t)(e)
            fwd[f"u_mul_e_sum {name}"] = lambda t=t: getattr(blk, "u_mul_e_sum" + t)(v, e)

        def fwd_bwd(f):
            for t in (q, k, v, el, er, e):
                t.grad = None
            out = f()
            out.backward(torch.ones_like(out))

        def no_grad(f):
            with torch.no_grad():
                f()

        ops = {f"{n} forward + backward": (lambda f=f: fwd_bwd(f)) for n, f in fwd.items()}
        ops.update({f"{n} forward": (lambda f=f: no_grad(f)) for n, f in fwd.items() if n.startswith("chain")})
        with torch.no_grad():
            ref = fwd["chain torch"]()
            for name in ("chain native", "fused dot"):
                print(f"  largest difference of {name} from the torch chain: {float((fwd[name]() - ref).abs().max()):.3e}")
        reps = {n: (args.reps if "torch" not in n else max(args.reps // 5, 2)) for n in ops}
        peak = {}
        for n, fn in ops.items():      # warm-up, and the peak allocation of one call above what is resident
            timed(fn, 3)
            for t in (q, k, v, el, er, e):
                t.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[n] = (torch.cuda.max_memory_allocated() - base) / 1e6
        times = {n: [] for n in ops}
        for r in range(args.rounds):
            for n, fn in ops.items():
                times[n].append(timed(fn, reps[n]))
        print(f"fan-out {fan}, input block: {n_dst} dst rows, {blk.num_src} src rows, {edges} edges, {H} heads x {D}")
        print(f"  bytes: gathered rows [E, H, D] {edges * H * D * 4 / 1e6:.1f} MB, a per-edge tensor {blk.nbr.numel() * H * 4 / 1e6:.2f} MB")
        print(f"  variant                              us per call, median of {args.rounds} windows [min .. max]   peak allocation of a call")
        med = {}
        for n, t in times.items():
            med[n] = statistics.median(t)
            print(f"  {n:36s} {med[n]:9.1f}  [{min(t):.1f} .. {max(t):.1f}]  ({reps[n]} calls per window)   {peak[n]:8.1f} MB")
        fb = " forward + backward"
        print(f"  ratios, forward + backward: torch chain / native chain {med['chain torch' + fb] / med['chain native' + fb]:.2f}; "
              f"native chain / fused dot {med['chain native' + fb] / med['fused dot' + fb]:.2f}; native chain / fused gat "
              f"{med['chain native' + fb] / med['fused gat' + fb]:.2f}")
    g.close()
print("done")
