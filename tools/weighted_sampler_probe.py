"""Uniform against edge-weighted sampler calls (NeighborSampler(prob=...)), alternating in one run and timed with HIP events after a
warm-up: the bench's default shape (10 M-node power-law graph of mean in-degree 12, batch 1024, fan-outs 5,5 and 15,10,5) and a graph
with 10^5- and 10^6-edge hubs among the seeds.  Also reports the edges scanned (the in-degrees of the destination nodes of every
weighted layer) and the weight bytes they read per call.  Run it under `rocprofv3 --kernel-trace --stats -- python ...` in a run of
its own for the per-kernel split (development tool)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "coala-gnn_amd"))
import torch  # noqa: E402
from COALA_GNN.sampler import NeighborSampler  # noqa: E402
from COALA_GNN.synthetic import powerlaw_csc  # noqa: E402

N_CALLS = int(os.environ.get("PROBE_CALLS", "100"))


def weights(n_edges, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    w = 1.0 - torch.rand(n_edges, generator=gen, device="cuda")
    w[torch.rand(n_edges, generator=gen, device="cuda") < 0.1] = 0.0
    return w


def scanned(g, blocks):
    """edges whose weight a weighted call reads: the in-degrees of every fixed layer's destination nodes"""
    deg = g.indptr[1:] - g.indptr[:-1]
    return sum(int(deg[b.dstdata["_ID"]].sum()) for b in blocks if b.nbr is not None)


def compare(label, g, fan, seed_batches):
    uni, wgt = NeighborSampler(fan, seed=1), NeighborSampler(fan, seed=1, prob="w")
    for it in range(10):
        uni.sample(g, seed_batches(it))
        wgt.sample(g, seed_batches(it))
    torch.cuda.synchronize()
    times = {"uniform": [], "weighted": []}
    rows = 0
    for it in range(N_CALLS):
        seeds = seed_batches(it + 10)
        for name, smp in (("uniform", uni), ("weighted", wgt)) if it % 2 == 0 else (("weighted", wgt), ("uniform", uni)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _, _, blocks = smp.sample(g, seeds)
            b.record()
            times[name].append((a, b))
            if name == "weighted":
                rows += scanned(g, blocks)
    torch.cuda.synchronize()
    med = {k: sorted(x.elapsed_time(y) for x, y in v)[len(v) // 2] for k, v in times.items()}
    print(f"{label} fan-out {fan}: uniform {med['uniform']:.3f} ms, weighted {med['weighted']:.3f} ms on the stream (HIP events, median of "
          f"{N_CALLS}; ratio {med['weighted'] / med['uniform']:.2f}); {rows / N_CALLS:.0f} edges scanned, {4 * rows / N_CALLS / 1e6:.2f} MB of "
          f"weights read per weighted call")


torch.cuda.set_device(0)
rows = 10_000_000
indptr, indices = powerlaw_csc(rows, 12.0, seed=0, device="cuda")
g = NeighborSampler([1]).make_graph(indptr, indices, edata={"w": weights(indices.numel(), 0)})
ids = torch.randperm(6_000_000, device="cuda")
for fan in ([5, 5], [15, 10, 5]):
    compare("IGB-medium shape, batch 1024,", g, fan, lambda it: ids[(it % 5000) * 1024:(it % 5000 + 1) * 1024])
g.close()
del g, indptr, indices
torch.cuda.empty_cache()

# hubs: a 1 M-node power-law graph (mean in-degree 10) whose nodes 0 and 1 have 10^5 and 10^6 in-edges
n = 1_000_000
ip, ix = powerlaw_csc(n, 10.0, seed=2, device="cuda")
deg = ip[1:] - ip[:-1]
deg[0], deg[1] = 100_000, 1_000_000
hub_ip = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
torch.cumsum(deg, 0, out=hub_ip[1:])
hub_ix = torch.randint(0, n, (int(hub_ip[-1]),), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
g = NeighborSampler([1]).make_graph(hub_ip, hub_ix, edata={"w": weights(hub_ix.numel(), 1)})
perm = torch.randperm(n - 2, device="cuda") + 2
for fan in ([5, 5], [15, 10, 5]):
    compare("hub graph, seeds = both hubs + 1022 others,", g, fan,
            lambda it: torch.cat([torch.tensor([0, 1], device="cuda"), perm[(it % 900) * 1022:(it % 900 + 1) * 1022]]))
    compare("hub graph, 1024 seeds without the hubs,", g, fan, lambda it: perm[(it % 900) * 1024:(it % 900 + 1) * 1024])
g.close()
