"""GATv2 attention aggregation, native kernels against Block.gatv2_aggregate_torch, with GAT's figures beside them, at the reference's
GAT shape (development tool).

The default synthetic graph (10 M nodes, mean in-degree 12), 1024 seeds, fan-out 5,5; input dim 1024, hidden 128, 4 heads: layer 1
aggregates feat_src [n_src, 4, 128], layer 2 feat_src [n_mid, 4, 19] (19 classes); then one -1,-1 evaluation batch.  For each block and
each of gatv2 native, gatv2 torch, gat native: forward, and forward + backward, on the stream (HIP events, median of --iters), and
torch.cuda.max_memory_allocated of one forward + backward above what was allocated before it.  The last line states the condition the
native path is held to: on the 5,5 input block it is not slower than the torch fallback, forward and forward + backward.
  python tools/gatv2_aggregate_probe.py [--iters 20]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "coala-gnn_amd"))
import torch  # noqa: E402

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


def edges(b):
    return int(b.indices.numel()) if b.nbr is None else int((b.nbr >= 0).sum())


def probe(tag, b, H, D, iters):
    gen = torch.Generator(device="cuda").manual_seed(0)
    fs = torch.randn(b.num_src, H, D, device="cuda", generator=gen).requires_grad_(True)
    fd = torch.randn(b.num_dst, H, D, device="cuda", generator=gen).requires_grad_(True)
    attn = torch.randn(1, H, D, device="cuda", generator=gen).requires_grad_(True)
    el = torch.randn(b.num_src, H, device="cuda", generator=gen).requires_grad_(True)
    er = torch.randn(b.num_dst, H, device="cuda", generator=gen).requires_grad_(True)
    g = torch.randn(b.num_dst, H, D, device="cuda", generator=gen)
    E = edges(b)
    paths = (("gatv2 native", b.gatv2_aggregate, (fs, fd, attn)), ("gatv2 torch", b.gatv2_aggregate_torch, (fs, fd, attn)),
             ("gat native", b.gat_aggregate, (el, er, fs)))
    res = {}
    print(f"{tag}: n_dst {b.num_dst}, n_src {b.num_src}, edges {E}, H {H}, D {D}; one [E, H, D] fp32 tensor is {E * H * D * 4 / 1e6:.1f} MB", flush=True)
    for name, op, args in paths:
        with torch.no_grad():
            f = median_ms(lambda: op(*args), iters)

        def step():
            for t in args:
                t.grad = None
            (op(*args) * g).sum().backward()
        fb = median_ms(step, iters)
        for t in args:
            t.grad = None
        mem = peak_mb(step)
        res[name] = (f, fb, mem)
        print(f"  {name:13s} fwd {f:8.3f} ms   fwd+bwd {fb:8.3f} ms   peak memory of fwd+bwd {mem:8.1f} MB", flush=True)
    n, t = res["gatv2 native"], res["gatv2 torch"]
    print(f"  gatv2 native against torch: fwd {t[0] / n[0]:.2f}x, fwd+bwd {t[1] / n[1]:.2f}x, peak memory {t[2] - n[2]:.1f} MB lower "
          f"(3 E H D 4 = {3 * E * H * D * 4 / 1e6:.1f} MB); against gat native: fwd {n[0] / res['gat native'][0]:.2f}x the time, "
          f"fwd+bwd {n[1] / res['gat native'][1]:.2f}x", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=10_000_000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    indptr, indices = powerlaw_csc(args.rows, 12.0, seed=0, device="cuda")
    seeds = torch.randperm(int(0.6 * args.rows), device="cuda")[:1024]
    H, hidden, classes = 4, 128, 19
    cond = None
    for fan in ([5, 5], [-1, -1]):
        s = NeighborSampler(fan)
        g = s.make_graph(indptr, indices)
        _, _, blocks = s.sample(g, seeds)
        r = probe(f"fan-out {fan} layer 1", blocks[0], H, hidden, args.iters)
        if fan == [5, 5]:
            cond = r
        probe(f"fan-out {fan} layer 2", blocks[1], H, classes, args.iters)
        g.close()
    n, t = cond["gatv2 native"], cond["gatv2 torch"]
    ok = n[0] <= t[0] and n[1] <= t[1]
    print(f"condition (5,5 input block, median against median): native fwd {n[0]:.3f} <= torch {t[0]:.3f} ms and native fwd+bwd {n[1]:.3f} <= "
          f"torch {t[1]:.3f} ms: {'holds' if ok else 'FAILS'}", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
