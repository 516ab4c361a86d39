"""Relation-typed GAT attention (Block.rel_gat_aggregate), the native kernels against the two ways to compute it without them, at the
reference's RGAT shape (development tool).

The default synthetic graph (10 M nodes, mean in-degree 12), 1024 seeds, fan-out 5,5, the input block; 4 heads x 128; R in {1, 4, 8}
relations (the source's id modulo R), the packed tables RelGATConv builds: one row per (source, relation) pair that occurs on an edge.
Side by side, forward and forward + backward on the stream (HIP events, median of --iters):
  native     one fused forward kernel, one backward launch;
  torch      Block.rel_gat_aggregate_torch, the edge-list softmax that materialises [E, H, D];
  R x gat    R Block.gat_aggregate calls, each on a copy of the block that keeps one relation's edges (the copies are built outside the
             timed region, which flatters this path: a model would rebuild them per batch).
  python tools/rel_gat_probe.py [--iters 20]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "coala-gnn_amd"))
import torch  # noqa: E402

from COALA_GNN.sampler import Block, NeighborSampler  # noqa: E402
from COALA_GNN.synthetic import powerlaw_csc  # noqa: E402


def median_ms(fn, iters):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[iters // 2]


def probe(b, R, H, D, iters):
    gen = torch.Generator(device="cuda").manual_seed(0)
    src = b.nbr.to(torch.int64)
    etype = torch.where(src >= 0, b.src_nodes[src.clamp_min(0)] % R, 0)
    pairs, inv = torch.unique((etype * b.num_src + src)[src >= 0], return_inverse=True)
    rows = torch.full_like(src, -1)
    rows[src >= 0] = inv
    P = pairs.numel()
    el = torch.randn(P, H, device="cuda", generator=gen).requires_grad_(True)
    feat = torch.randn(P, H, D, device="cuda", generator=gen).requires_grad_(True)
    er = torch.randn(b.num_dst, R, H, device="cuda", generator=gen).requires_grad_(True)
    g = torch.randn(b.num_dst, H, D, device="cuda", generator=gen)
    by_rel = [Block(torch.arange(P, device="cuda"), torch.where(etype == r, rows, -1).to(torch.int32).contiguous(), b.num_dst) for r in range(R)]

    def r_gat():
        return sum(br.gat_aggregate(el, er[:, r], feat) for r, br in enumerate(by_rel))

    paths = (("native", lambda: b.rel_gat_aggregate(el, er, feat, etype, R, rows=rows)),
             ("torch", lambda: b.rel_gat_aggregate_torch(el, er, feat, etype, R, rows=rows)), (f"{R} x gat", r_gat))
    E = int((src >= 0).sum())
    print(f"R {R}: n_dst {b.num_dst}, n_src {b.num_src}, edges {E}, (source, relation) pairs {P}, H {H}, D {D}", flush=True)
    res = {}
    for name, op in paths:
        with torch.no_grad():
            f = median_ms(op, iters)

        def step():
            for t in (el, er, feat):
                t.grad = None
            (op() * g).sum().backward()
        res[name] = (f, median_ms(step, iters))
        print(f"  {name:8s} fwd {res[name][0]:8.3f} ms   fwd+bwd {res[name][1]:8.3f} ms", flush=True)
    n = res["native"]
    for name in list(res)[1:]:
        print(f"  native against {name}: fwd {res[name][0] / n[0]:.2f}x, fwd+bwd {res[name][1] / n[1]:.2f}x", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=10_000_000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    indptr, indices = powerlaw_csc(args.rows, 12.0, seed=0, device="cuda")
    seeds = torch.randperm(int(0.6 * args.rows), device="cuda")[:1024]
    s = NeighborSampler([5, 5])
    g = s.make_graph(indptr, indices)
    _, _, blocks = s.sample(g, seeds)
    for R in (1, 4, 8):
        probe(blocks[0], R, 4, 128, args.iters)
    g.close()
    print("not measured here: ragged (-1) blocks, a training epoch", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
