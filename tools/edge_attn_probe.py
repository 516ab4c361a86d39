"""Edge-feature attention aggregation, the native kernels against Block.edge_attn_aggregate_torch, with dot-product attention's figures
beside them to show what the edge part costs (development tool).

powerlaw_csc(200000, 30) with a synthetic fp32 [num_edges, F] feature table read through edata['_ID'] (the table form), 1024 seeds,
NeighborSampler(edge_ids=True) with fan-outs 10,10 and -1,-1: the input block of each (fixed, and ragged with hub rows).  Shapes
(H, D, F) = (4, 128, 16) and (4, 128, 128).  For edge native, edge torch and dot native: forward, and forward + backward (gradients for
q, k, v, qe and efeat; q, k, v for dot), HIP events around one call, median of --iters, the three paths taking turns inside every
iteration so that what else runs on the machine hits them alike; and torch.cuda.max_memory_allocated of one forward + backward above
what was allocated before it.  The last line states the condition the native path is held to: on the 10,10 input block, at both shapes,
native forward + backward is not slower than the fallback.  The -1,-1 block is reported without a condition.
  python tools/edge_attn_probe.py [--iters 20]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "coala-gnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from COALA_GNN.sampler import NeighborSampler  # noqa: E402
from COALA_GNN.synthetic import powerlaw_csc  # noqa: E402
from time_attn_probe import medians_ms, peak_mb  # noqa: E402


def probe(tag, b, efeat, H, D, iters):
    gen = torch.Generator(device="cuda").manual_seed(0)
    F, eids = efeat.shape[1], b.edata["_ID"]
    E = int(((b.indices if b.nbr is None else b.nbr) >= 0).sum())
    mk = lambda *s: torch.randn(*s, device="cuda", generator=gen).requires_grad_(True)   # noqa: E731
    q, k, v, qe = mk(b.num_dst, H, D), mk(b.num_src, H, D), mk(b.num_src, H, D), mk(b.num_dst, H, F)
    g, ge = torch.randn(b.num_dst, H, D, device="cuda", generator=gen), torch.randn(b.num_dst, H, F, device="cuda", generator=gen)
    edge_args, dot_args = (q, k, v, qe, efeat), (q, k, v)
    ops = [("edge native", lambda: b.edge_attn_aggregate(q, k, v, qe, efeat, eids, validate=False), edge_args),
           ("edge torch", lambda: b.edge_attn_aggregate_torch(q, k, v, qe, efeat, eids), edge_args),
           ("dot native", lambda: (b.dot_gat_aggregate(q, k, v, validate=False), ge), dot_args)]

    def stepper(op, args):
        def step():
            for t in args:
                t.grad = None
            out, eagg = op()
            ((out * g).sum() + (eagg * ge).sum()).backward()
        return step
    steps = [stepper(op, args) for _, op, args in ops]
    form = "ragged" if b.nbr is None else f"fan-out {b.nbr.shape[1]}"
    print(f"{tag}: n_dst {b.num_dst}, n_src {b.num_src}, {form}, edges {E}, H {H}, D {D}, F {F}; [E, F] fp32 is {E * F * 4 / 1e6:.1f} MB, "
          f"[E, H, D] {E * H * D * 4 / 1e6:.1f} MB, [E, H, F] {E * H * F * 4 / 1e6:.1f} MB", flush=True)
    with torch.no_grad():
        fwd = medians_ms([op for _, op, _ in ops], iters)
    fb = medians_ms(steps, iters)
    res = {}
    for (name, _, args), f, t, step in zip(ops, fwd, fb, steps):
        for x in args:
            x.grad = None
        res[name] = (f, t, peak_mb(step))
        print(f"  {name:11s} fwd {f:8.3f} ms   fwd+bwd {t:8.3f} ms   peak memory of fwd+bwd {res[name][2]:8.1f} MB", flush=True)
    n, t, d = res["edge native"], res["edge torch"], res["dot native"]
    print(f"  edge native against torch: fwd {t[0] / n[0]:.2f}x, fwd+bwd {t[1] / n[1]:.2f}x, peak memory {t[2] - n[2]:.1f} MB lower; against dot "
          f"native: fwd {n[0] / d[0]:.2f}x the time, fwd+bwd {n[1] / d[1]:.2f}x", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=200_000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    indptr, indices = powerlaw_csc(args.rows, 30.0, seed=0, device="cuda")
    seeds = torch.randperm(args.rows, device="cuda")[:1024]
    gen = torch.Generator(device="cuda").manual_seed(1)
    verdicts = []
    for fan in ([10, 10], [-1, -1]):
        s = NeighborSampler(fan, edge_ids=True)
        g = s.make_graph(indptr, indices)
        _, _, blocks = s.sample(g, seeds)
        for H, D, F in ((4, 128, 16), (4, 128, 128)):
            efeat = torch.randn(indices.numel(), F, device="cuda", generator=gen).requires_grad_(True)
            r = probe(f"fan-outs {fan} input block", blocks[0], efeat, H, D, args.iters)
            if fan[0] > 0:
                verdicts.append((fan, (H, D, F), r["edge native"][1], r["edge torch"][1]))
            del efeat
        g.close()
    ok = all(n <= t for _, _, n, t in verdicts)
    for fan, shape, n, t in verdicts:
        print(f"condition, fan-outs {fan} input block, (H, D, F) = {shape}: native fwd+bwd {n:.3f} <= torch {t:.3f} ms: {'holds' if n <= t else 'FAILS'}")
    print(f"condition (median against median, the 10,10 input block at both shapes): {'holds' if ok else 'FAILS'}", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
