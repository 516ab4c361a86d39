"""Scaled dot-product attention aggregation, native kernels against Block.dot_gat_aggregate_torch, with GAT's figures beside them, at
the reference's GAT shape (development tool).

The default synthetic graph (10 M nodes, mean in-degree 12), 1024 seeds, 4 heads x 128: the input and the output block of fan-out 5,5
and the input block of fan-out 10,10.  On each block the dense form (k and v have one row per source node) and the packed form at
R = 1, 4 and 8 relations (k and v have one row per (source, relation) pair that occurs on an edge, the edge types the slot position
modulo R, rows as HGTConv builds them, int32).  For each of dot native, dot torch and -- dense form only -- gat native: forward, and
forward + backward, on the stream (HIP events, median of --iters), and torch.cuda.max_memory_allocated of one forward + backward above
what was allocated before it.  The last line states the condition the native path is held to: on the 5,5 input block, dense form, it is
not slower than the torch fallback, forward and forward + backward.
  python tools/dot_gat_probe.py [--iters 20]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "coala-gnn_amd"))
import torch  # noqa: E402

from COALA_GNN.nn import _pack_pairs  # noqa: E402
from COALA_GNN.sampler import NeighborSampler  # noqa: E402
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


def peak_mb(step):
    """Peak allocation of one step above the allocation it starts from, MB."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def probe(tag, b, H, D, iters, num_rels=0):
    """num_rels 0: the dense form; > 0: the packed form over the (source, relation) pairs of that many relations."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    slots = b.indices if b.nbr is None else b.nbr
    E = int((slots >= 0).sum())
    rows, P = None, b.num_src
    if num_rels:
        etype = (torch.arange(slots.numel(), device="cuda") % num_rels).view(slots.shape)
        r, pair_rel, _, _ = _pack_pairs(b, etype, num_rels, torch.device("cuda"))
        rows, P = r.to(torch.int32).view(slots.shape), int(pair_rel.numel())
    q = torch.randn(b.num_dst, H, D, device="cuda", generator=gen).requires_grad_(True)
    k = torch.randn(P, H, D, device="cuda", generator=gen).requires_grad_(True)
    v = torch.randn(P, H, D, device="cuda", generator=gen).requires_grad_(True)
    g = torch.randn(b.num_dst, H, D, device="cuda", generator=gen)
    paths = [("dot native", lambda: b.dot_gat_aggregate(q, k, v, rows=rows, validate=False), (q, k, v)),
             ("dot torch", lambda: b.dot_gat_aggregate_torch(q, k, v, rows=rows), (q, k, v))]
    if not num_rels:
        el = torch.randn(b.num_src, H, device="cuda", generator=gen).requires_grad_(True)
        er = torch.randn(b.num_dst, H, device="cuda", generator=gen).requires_grad_(True)
        paths.append(("gat native", lambda: b.gat_aggregate(el, er, v), (el, er, v)))
    form = f"packed R={num_rels}" if num_rels else "dense"
    print(f"{tag}, {form}: n_dst {b.num_dst}, n_src {b.num_src}, rows of k / v {P}, edges {E}, H {H}, D {D}; one [E, H, D] fp32 tensor is "
          f"{E * H * D * 4 / 1e6:.1f} MB", flush=True)
    res = {}
    for name, op, args in paths:
        with torch.no_grad():
            f = median_ms(op, iters)

        def step():
            for t in args:
                t.grad = None
            (op() * g).sum().backward()
        fb = median_ms(step, iters)
        for t in args:
            t.grad = None
        mem = peak_mb(step)
        res[name] = (f, fb, mem)
        print(f"  {name:11s} fwd {f:8.3f} ms   fwd+bwd {fb:8.3f} ms   peak memory of fwd+bwd {mem:8.1f} MB", flush=True)
    n, t = res["dot native"], res["dot torch"]
    line = f"  dot native against torch: fwd {t[0] / n[0]:.2f}x, fwd+bwd {t[1] / n[1]:.2f}x, peak memory {t[2] - n[2]:.1f} MB lower"
    if "gat native" in res:
        line += f"; against gat native: fwd {n[0] / res['gat native'][0]:.2f}x the time, fwd+bwd {n[1] / res['gat native'][1]:.2f}x"
    print(line, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=10_000_000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    indptr, indices = powerlaw_csc(args.rows, 12.0, seed=0, device="cuda")
    seeds = torch.randperm(int(0.6 * args.rows), device="cuda")[:1024]
    H, D = 4, 128
    cond = None
    for fan, layers in (([5, 5], (0, 1)), ([10, 10], (0,))):
        s = NeighborSampler(fan)
        g = s.make_graph(indptr, indices)
        _, _, blocks = s.sample(g, seeds)
        for layer in layers:
            for R in (0, 1, 4, 8):
                r = probe(f"fan-out {fan} {'input' if layer == 0 else 'output'} block", blocks[layer], H, D, args.iters, R)
                if fan == [5, 5] and layer == 0 and R == 0:
                    cond = r
        g.close()
    n, t = cond["dot native"], cond["dot torch"]
    ok = n[0] <= t[0] and n[1] <= t[1]
    print(f"condition (5,5 input block, dense form, median against median): native fwd {n[0]:.3f} <= torch {t[0]:.3f} ms and native fwd+bwd "
          f"{n[1]:.3f} <= torch {t[1]:.3f} ms: {'holds' if ok else 'FAILS'}", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
