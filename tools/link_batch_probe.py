#!/usr/bin/env python3
"""What a link-prediction minibatch costs (profiles/r15_link_prediction.txt): the edge-batch kernels, their host wait and the edge
exclusion beside the plain neighbour sample of the same seed nodes, both against their torch restatements (torch.unique compaction,
torch.isin masking), pair_dot against pair_dot_torch, and a loader step.  powerlaw_csc(200000, 30) symmetrised, 1024 seed edges,
k = 1 and 5 negatives, fan-out 5,5 and 10,10; every figure is the median of 20 event-timed calls, in microseconds."""
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import torch  # noqa: E402
from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, SSD_INFO  # noqa: E402
from COALA_GNN.block_ops import pair_dot, pair_dot_torch  # noqa: E402
from COALA_GNN.color_info_gen import save_color_files  # noqa: E402
from COALA_GNN.sampler import (EdgePredictionSampler, NeighborSampler, UniformNegativeSampler, edge_batch, edge_batch_wait,  # noqa: E402
                               reverse_edge_ids)
from COALA_GNN.synthetic import alloc_pinned_table, block_colors, powerlaw_csc, symmetrize_csc  # noqa: E402

torch.cuda.set_device(0)
N, B, REPS = 200_000, 1024, 20
ip, ix = symmetrize_csc(*powerlaw_csc(N, 30.0, seed=0, device="cuda"))
E = ix.numel()
rev = reverse_edge_ids(ip, ix)
g = NeighborSampler([1]).make_graph(ip, ix)
print(f"graph: powerlaw_csc({N}, 30) symmetrised, {E} edges; {B} seed edges per batch; us, median of {REPS} event-timed calls [min .. max]")
batches = [torch.randint(0, E, (B,), generator=torch.Generator().manual_seed(i)).cuda() for i in range(REPS)]


def timed(fn, warm=3):
    """fn(i) for i < REPS, each between two events on the current stream (the host's share of a call is inside: the stream idles)."""
    for i in range(warm):
        fn(i)
    out = []
    for i in range(REPS):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn(i)
        z.record()
        z.synchronize()
        out.append(a.elapsed_time(z) * 1e3)
    return statistics.median(out), min(out), max(out)


def line(name, t):
    print(f"  {name:58s} {t[0]:9.1f}  [{t[1]:.1f} .. {t[2]:.1f}]")
    return t[0]


def torch_edge_batch(eids, k, step):
    """The edge batch in plain torch: searchsorted endpoints, torch.randint negatives (another stream of draws: the cost is the same),
    torch.unique compaction re-ordered by first appearance."""
    src, dst = ix[eids], torch.searchsorted(ip, eids, right=True) - 1
    neg = torch.randint(0, N, (eids.numel() * k,), device=eids.device)
    items = torch.cat([src, dst, neg])
    uniq, inv = torch.unique(items, return_inverse=True)
    first = torch.full((uniq.numel(),), items.numel(), dtype=torch.int64, device=items.device)
    first.scatter_reduce_(0, inv, torch.arange(items.numel(), device=items.device), "amin")
    order = torch.argsort(first)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), device=order.device)
    return uniq[order], rank[inv].to(torch.int32)


def excluded_list(eids):
    return torch.sort(torch.cat([eids, rev[eids]])).values


results = {}
for fan in ([5, 5], [10, 10]):
    for k in (1, 5):
        print(f"fan-out {fan}, k = {k}")
        wrapped = EdgePredictionSampler(NeighborSampler(fan, seed=1, edge_ids=True), exclude="reverse_id", reverse_eids=rev,
                                        negative_sampler=UniformNegativeSampler(k))
        plain = NeighborSampler(fan, seed=1, edge_ids=True)
        sampled = [wrapped.sample(g, batches[i], step=i) for i in range(REPS)]
        seeds = [s[1].seed_nodes for s in sampled]
        print(f"  seed nodes {statistics.mean(s.numel() for s in seeds):.0f}, input nodes {statistics.mean(s[0].numel() for s in sampled):.0f} (means)")
        t_wrap = line("(a) wrapper.sample(seed edges)", timed(lambda i: wrapped.sample(g, batches[i], step=i)))
        t_plain = line("(a) NeighborSampler.sample(the same seed nodes, edge ids on)", timed(lambda i: plain.sample(g, seeds[i], step=i)))
        pend = []

        def enqueue(i):   # the call before has finished (timed() synchronises): collecting it first is a host call of microseconds
            if pend:
                edge_batch_wait(pend.pop())
            pend.append(edge_batch(g, batches[i], k, seed=1, step=i))
        t_kern = line("    edge-batch kernels (enqueued, not waited for)", timed(enqueue))
        edge_batch_wait(pend.pop())
        t_wait = line("    edge batch + its host wait", timed(lambda i: edge_batch_wait(edge_batch(g, batches[i], k, seed=1, step=i))))
        unex = [plain.sample(g, seeds[i], step=i)[2] for i in range(REPS)]
        t_excl = line("    exclusion: list sort + exclude_edges on both blocks", timed(lambda i: [b.exclude_edges(excluded_list(batches[i])) for b in unex[i]]))
        print(f"    edge-batch kernels {t_kern:.1f} us, host wait {t_wait - t_kern:.1f} us, exclusion {t_excl:.1f} us; added by the wrapper: {t_wrap - t_plain:.1f} us = {100 * (t_wrap - t_plain) / t_plain:.0f} % of the plain call")
        t_tb = line("(b) torch edge batch (unique compaction)", timed(lambda i: torch_edge_batch(batches[i], k, i)))
        t_te = line("(b) torch exclusion: list sort + exclude_edges_torch (isin)", timed(lambda i: [b.exclude_edges_torch(excluded_list(batches[i])) for b in unex[i]]))
        print(f"    native edge batch + exclusion {t_wait + t_excl:.1f} us, torch restatement {t_tb + t_te:.1f} us")
        results[(tuple(fan), k)] = (t_wait + t_excl, t_tb + t_te)
nat, tor = results[((5, 5), 5)]
print(f"condition 1 (5,5, k = 5: native edge batch + exclusion no slower than the torch restatement): {nat:.1f} vs {tor:.1f} us: "
      f"{'holds' if nat <= tor else 'FAILS'}")

print("(c) pair_dot: 6144 pairs (1024 edges, k = 5) over 8192 rows")
P, rows = 6144, 8192
src = torch.randint(0, rows, (P,), device="cuda", dtype=torch.int32)
dst = torch.randint(0, rows, (P,), device="cuda", dtype=torch.int32)
s64, d64 = src.long(), dst.long()
cond2 = None
for D in (128, 256):
    h = torch.randn(rows, D, device="cuda", requires_grad=True)
    go = torch.randn(P, device="cuda")

    def both(fn, a, b):
        h.grad = None
        fn(h, a, b).backward(go)
    f_n = line(f"D = {D}: pair_dot forward", timed(lambda i: pair_dot(h.detach(), src, dst, validate=False)))
    f_t = line(f"D = {D}: pair_dot_torch forward", timed(lambda i: pair_dot_torch(h.detach(), s64, d64)))
    b_n = line(f"D = {D}: pair_dot forward + backward", timed(lambda i: both(lambda *a: pair_dot(*a, validate=False), src, dst)))
    b_t = line(f"D = {D}: pair_dot_torch forward + backward", timed(lambda i: both(pair_dot_torch, s64, d64)))
    if D == 128:
        cond2 = (f_n, f_t, b_n, b_t)
print(f"condition 2 (pair_dot no slower than its fallback at D = 128): forward {cond2[0]:.1f} vs {cond2[1]:.1f} us, forward + backward "
      f"{cond2[2]:.1f} vs {cond2[3]:.1f} us: {'holds' if cond2[0] <= cond2[1] and cond2[2] <= cond2[3] else 'FAILS'}")

print("(d) a loader step: COALA_GNN_DataLoader over edge ids, 5,5, k = 5, dim 128, isolated cache of 64 MB")
dim = 128
table = alloc_pinned_table(N, dim, seed=0, device=0)
tmp = tempfile.mkdtemp(prefix="coala_color_")
color, tk, sc, _ = block_colors(N, nodes_per_color=4096)
save_color_files(tmp, color, tk, sc)
comm = MPI_Comm_Manager(0)
comm.initialize_nested_process_group("isolated")
for name, make, items in (("seed edges through the wrapper", lambda: EdgePredictionSampler(NeighborSampler([5, 5], seed=1), exclude="reverse_id", reverse_eids=rev,
                                                                                       negative_sampler=UniformNegativeSampler(5)), E),
                          ("seed nodes, plain NeighborSampler (7 x 1024 per step)", lambda: NeighborSampler([5, 5], seed=1), N)):
    smp = make()
    bs = B if items == E else 7 * B
    ids = torch.randperm(items, generator=torch.Generator().manual_seed(2))[: bs * 44]
    nd = Node_Distributor(comm, ids, bs, *[os.path.join(tmp, f) for f in ("color.npy", "topk.npy", "score.npy")], parsing_method="baseline")
    loader = COALA_GNN_DataLoader(SSD_INFO(1, dim * 4, 1024, 0), nd, g, smp, bs, dim, smp.fanouts, 64, "cuda:0", cache_backend="isolated",
                                  sim_buf=table, num_rows=N)
    times, n_in = [], []
    a = torch.cuda.Event(enable_timing=True)
    a.record()
    for step, item in enumerate(loader):
        z = torch.cuda.Event(enable_timing=True)
        z.record()
        z.synchronize()
        if step >= 3:
            times.append(a.elapsed_time(z) * 1e3)
        n_in.append(item[0].numel())
        a = torch.cuda.Event(enable_timing=True)
        a.record()
    times = times[:REPS]
    print(f"  {name:58s} {statistics.median(times):9.1f}  [{min(times):.1f} .. {max(times):.1f}]  {statistics.mean(n_in):.0f} input nodes")
    del loader
table.close()
g.close()
print("not measured: ragged (-1) blocks, a training epoch")
print("done")
