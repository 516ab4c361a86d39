"""GAT attention aggregation, native kernels against Block.gat_aggregate_torch, at the reference's GAT shape (development tool).

The default synthetic graph (10 M nodes, mean in-degree 12), 1024 seeds, fan-out 5,5; input dim 1024, hidden 128, 4 heads: layer 1
aggregates feat_src [n_src, 4, 128], layer 2 feat_src [n_mid, 4, 19] (19 classes); then one -1,-1 evaluation batch.  For each block:
forward, and forward + backward, on the stream (HIP events, median of --iters), and the bytes the native kernels must move, computed
from the shapes, as a share of 8 TB/s.
  python tools/gat_aggregate_probe.py [--iters 20]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "coala-gnn_amd"))
import torch  # noqa: E402

from COALA_GNN.sampler import NeighborSampler  # noqa: E402
from COALA_GNN.synthetic import powerlaw_csc  # noqa: E402

HBM = 8e12


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


def edges(b):
    return int(b.indices.numel()) if b.nbr is None else int((b.nbr >= 0).sum())


def probe(tag, b, H, D, iters):
    gen = torch.Generator(device="cuda").manual_seed(0)
    el = torch.randn(b.num_src, H, device="cuda", generator=gen).requires_grad_(True)
    er = torch.randn(b.num_dst, H, device="cuda", generator=gen).requires_grad_(True)
    feat = torch.randn(b.num_src, H, D, device="cuda", generator=gen).requires_grad_(True)
    g = torch.randn(b.num_dst, H, D, device="cuda", generator=gen)
    E = edges(b)
    slots = b.nbr.numel() if b.nbr is not None else E
    row = H * D * 4
    # forward: the rows of every edge, el of every edge, the indices, er, out and lse; backward: the rows again, g once per row,
    # out, the grad_feat atomics, el again, the grad_el atomics, grad_er
    fwd_bytes = E * row + E * H * 4 + slots * 4 + b.num_dst * (row + 2 * H * 4)
    bwd_bytes = 2 * E * row + 2 * b.num_dst * row + 2 * E * H * 4 + E * H * 4 + slots * 4 + b.num_dst * 3 * H * 4
    res = {}
    for name, op in (("native", b.gat_aggregate), ("torch", b.gat_aggregate_torch)):
        with torch.no_grad():
            f = median_ms(lambda: op(el, er, feat), iters)

        def step():
            el.grad = er.grad = feat.grad = None
            (op(el, er, feat) * g).sum().backward()
        fb = median_ms(step, iters)
        res[name] = (f, fb)
    nf, nfb = res["native"]
    tf, tfb = res["torch"]
    print(f"{tag}: n_dst {b.num_dst}, n_src {b.num_src}, edges {E}, H {H}, D {D}: native fwd {nf:.3f} ms "
          f"({fwd_bytes / 1e6:.1f} MB, {fwd_bytes / nf / 1e6:.0f} GB/s = {fwd_bytes / nf * 1e3 / HBM:.1%} of 8 TB/s), fwd+bwd {nfb:.3f} ms "
          f"({(fwd_bytes + bwd_bytes) / 1e6:.1f} MB, {(fwd_bytes + bwd_bytes) / nfb * 1e3 / HBM:.1%}); torch fwd {tf:.3f} ms, fwd+bwd {tfb:.3f} ms; "
          f"speed-up fwd {tf / nf:.2f}x, fwd+bwd {tfb / nfb:.2f}x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=10_000_000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    indptr, indices = powerlaw_csc(args.rows, 12.0, seed=0, device="cuda")
    seeds = torch.randperm(int(0.6 * args.rows), device="cuda")[:1024]
    H, hidden, classes = 4, 128, 19
    for fan in ([5, 5], [-1, -1]):
        s = NeighborSampler(fan)
        g = s.make_graph(indptr, indices)
        _, _, blocks = s.sample(g, seeds)
        probe(f"fan-out {fan} layer 1", blocks[0], H, hidden, args.iters)
        probe(f"fan-out {fan} layer 2", blocks[1], H, classes, args.iters)
        g.close()


if __name__ == "__main__":
    main()
