"""Sampler wall time per call for the BASELINE fan-outs and for full layers (fan-out -1), then a load-balance check of a full layer:
one star hub of 10^6 distinct in-neighbours against the same item count spread over 1,000 nodes of in-degree 1,000 (development
tool)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "coala-gnn_amd"))
import torch
from COALA_GNN.sampler import NeighborSampler
from COALA_GNN.synthetic import powerlaw_csc
rows = 10_000_000
torch.cuda.set_device(0)
indptr, indices = powerlaw_csc(rows, 12.0, seed=0, device="cuda")
ids = torch.randperm(6_000_000, device="cuda")
for fan, G in (([5, 5], 0), ([5, 5], 8), ([10, 10], 0), ([10, 10], 8), ([15, 10, 5], 0), ([10, 10, 10], 0), ([10, 10, 10], 8),
               ([-1], 0), ([10, -1], 0), ([-1, -1], 0)):
    s = NeighborSampler(fan, bucket_by_owner=G); g = s.make_graph(indptr, indices)
    for it in range(10): s.sample(g, ids[it * 1024:(it + 1) * 1024])
    torch.cuda.synchronize(); t0 = time.perf_counter(); N = 100; n_in = 0
    for it in range(N):
        n_in += s.sample(g, ids[(it + 10) * 1024:(it + 11) * 1024])[0].numel()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / N * 1e3
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
    for it in range(N):
        ev[it][0].record(); s.sample(g, ids[(it + 10) * 1024:(it + 11) * 1024]); ev[it][1].record()
    torch.cuda.synchronize()
    gpu = sorted(a.elapsed_time(b) for a, b in ev)[N // 2]
    print(f"fanout {fan}{' bucketed by 8 owners' if G else ''}: {wall:.3f} ms per call (host wall), {gpu:.3f} ms on the stream (HIP events, median), {n_in / N:.0f} input nodes")


def stream_ms(s, g, seeds, N=20):
    for _ in range(3):
        s.sample(g, seeds)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
    for a, b in ev:
        a.record(); s.sample(g, seeds); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[N // 2]


# load balance: nodes 0..999 have 1,000 distinct in-neighbours each, node 1000 has all 10^6 of them (the same ids)
D, K = 1000, 1000
nbrs = torch.arange(K + 1, K + 1 + D * K, device="cuda")
lb_indptr = torch.cat([torch.arange(K + 1, device="cuda") * D,
                       torch.full((D * K + 1,), 2 * D * K, device="cuda")]).to(torch.int64)
lb_indices = torch.cat([nbrs, nbrs]).to(torch.int64)
s = NeighborSampler([-1]); g = s.make_graph(lb_indptr, lb_indices)
hub = stream_ms(s, g, torch.tensor([K], device="cuda"))
spread = stream_ms(s, g, torch.arange(K, device="cuda"))
print(f"load balance, one full layer: star hub of {D * K} distinct in-neighbours {hub:.3f} ms on the stream; "
      f"{K} nodes x {D} distinct in-neighbours {spread:.3f} ms (ratio {max(hub, spread) / min(hub, spread):.2f})")
