#!/usr/bin/env python3
"""What a node2vec step costs (profiles/r20_node2vec.txt): (a) the second-order walk kernel beside random_walk, and what rejection
costs at the corners of the paper's grid; (b) the fused window loss beside the composed path -- explicit pair lists, pair_dot,
softplus -- with both paths' peak allocation; (c) a whole training step and the share of each part.
symmetrize_csc(powerlaw_csc(200000, 30)), 128 start nodes x 10 walks, L = 20, C = 10, K = 1, D = 128.  Every figure is the median of 20
event-timed calls in microseconds; the variants of a comparison alternate call by call in this one process."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import torch  # noqa: E402
from COALA_GNN import Node2Vec, SparseAdam  # noqa: E402
from COALA_GNN.block_ops import pair_dot, skipgram_loss  # noqa: E402
from COALA_GNN.sampler import CSCGraph, node2vec_random_walk, random_walk, walk_batch, walk_batch_begin, walk_batch_end  # noqa: E402
from COALA_GNN.synthetic import powerlaw_csc, symmetrize_csc  # noqa: E402

torch.cuda.set_device(0)
N, B, W, L, C, K, D, REPS = 200_000, 128, 10, 20, 10, 1, 128, 20
ip, ix = symmetrize_csc(*powerlaw_csc(N, 30.0, seed=0, device="cuda"))
g = CSCGraph(ip, ix)
print(f"graph: powerlaw_csc({N}, 30) symmetrised, {ix.numel()} edges; {B} start nodes x {W} walks, L = {L}, C = {C}, K = {K}, D = {D}; us, median of "
      f"{REPS} event-timed calls [min .. max], variants alternating")
starts = [torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(i)).cuda() for i in range(REPS)]


def alternate(fns, warm=3):
    """Every fn(i) for i < REPS, the variants taking turns, each call between two events on the current stream."""
    for i in range(warm):
        for fn in fns:
            fn(i)
    out = [[] for _ in fns]
    for i in range(REPS):
        for k, fn in enumerate(fns):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn(i)
            z.record()
            z.synchronize()
            out[k].append(a.elapsed_time(z) * 1e3)
    return [(statistics.median(o), min(o), max(o)) for o in out]


def line(name, t):
    print(f"  {name:66s} {t[0]:9.1f}  [{t[1]:.1f} .. {t[2]:.1f}]")
    return t[0]


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


# ------------------------------------------------------------------------------------------------------------------ (a) the walks
print(f"(a) walks: {B * W} walks per call")
ta = alternate([lambda i: random_walk(g, starts[i], 16, num_walks=W, seed=1, step=i),
                lambda i: node2vec_random_walk(g, starts[i], 1.0, 1.0, 16, num_walks=W, seed=1, step=i),
                lambda i: node2vec_random_walk(g, starts[i], 1.0, 1.0, L, num_walks=W, seed=1, step=i),
                lambda i: node2vec_random_walk(g, starts[i], 0.25, 4.0, L, num_walks=W, seed=1, step=i),
                lambda i: node2vec_random_walk(g, starts[i], 4.0, 0.25, L, num_walks=W, seed=1, step=i)])
for name, t in zip(("random_walk, 16 hops", "node2vec_random_walk p = q = 1, 16 hops (reported only)", f"node2vec_random_walk p = q = 1, {L} hops",
                    f"node2vec_random_walk p = 0.25 q = 4, {L} hops", f"node2vec_random_walk p = 4 q = 0.25, {L} hops"), ta):
    line(name, t)
pend = []


def enqueue(i):
    if pend:
        walk_batch_end(pend.pop())
    pend.append(walk_batch_begin(g, starts[i], 1.0, 1.0, L, W, K, seed=1, step=i))


tb = alternate([enqueue, lambda i: walk_batch(g, starts[i], 1.0, 1.0, L, W, K, seed=1, step=i), lambda i: walk_batch(g, starts[i], 0.25, 4.0, L, W, K, seed=1, step=i)])
walk_batch_end(pend.pop())
line("walk_batch kernels p = q = 1 (enqueued, not waited for)", tb[0])
line("walk_batch + its host wait, p = q = 1", tb[1])
line("walk_batch + its host wait, p = 0.25 q = 4", tb[2])

# ------------------------------------------------------------------------------------------------------------------ (b) the loss
batches = [walk_batch(g, starts[i], 1.0, 1.0, L, W, K, seed=1, step=i) for i in range(REPS)]
n_in = statistics.mean(b.input_nodes.numel() for b in batches)
a_idx = torch.arange(L + 2 - C, device="cuda")[:, None].expand(-1, C - 1).reshape(-1)
b_idx = (torch.arange(L + 2 - C, device="cuda")[:, None] + torch.arange(1, C, device="cuda")[None, :]).reshape(-1)
pairs = []   # the composed path's pair lists, built OUTSIDE the timed region (which flatters it)
for bt in batches:
    pairs.append(tuple(t[:, idx].reshape(-1).contiguous() for t in (bt.pos, bt.neg) for idx in (a_idx, b_idx)))
hs = [torch.randn(b.input_nodes.numel(), D, device="cuda", requires_grad=True) for b in batches]
print(f"(b) window loss: {B * W} positive and {B * W * K} negative rows of {L + 1}, {a_idx.numel()} pairs per row, {n_in:.0f} input nodes (mean)")


def composed(h, p):
    sp = torch.nn.functional.softplus
    pos = pair_dot(h, p[0], p[1], validate=False)
    neg = pair_dot(h, p[2], p[3], validate=False)
    keep_p, keep_n = (p[0] >= 0) & (p[1] >= 0), (p[2] >= 0) & (p[3] >= 0)
    return (sp(-pos) * keep_p).sum() / keep_p.sum().clamp_min(1) + (sp(neg) * keep_n).sum() / keep_n.sum().clamp_min(1)


def fwd_bwd(fn, i):
    hs[i].grad = None
    fn(i).backward()


fused_f = lambda i: skipgram_loss(hs[i].detach(), batches[i].pos, batches[i].neg, C, validate=False)   # noqa: E731
comp_f = lambda i: composed(hs[i].detach(), pairs[i])                                                    # noqa: E731
fused_b = lambda i: fwd_bwd(lambda j: skipgram_loss(hs[j], batches[j].pos, batches[j].neg, C, validate=False), i)   # noqa: E731
comp_b = lambda i: fwd_bwd(lambda j: composed(hs[j], pairs[j]), i)                                                    # noqa: E731
tl = alternate([fused_f, comp_f, fused_b, comp_b])
f_n = line("skipgram_loss forward", tl[0])
f_c = line("composed forward (pair lists prebuilt, pair_dot, softplus)", tl[1])
b_n = line("skipgram_loss forward + backward", tl[2])
b_c = line("composed forward + backward", tl[3])
print(f"  difference of the two losses on batch 0: {abs(float(fused_f(0)) - float(comp_f(0))):.2e}")
print(f"  peak allocation, forward + backward: fused {peak(lambda: fused_b(0)):.1f} MiB, composed {peak(lambda: comp_b(0)):.1f} MiB "
      f"(+ {sum(t.numel() * 4 for t in pairs[0]) / 2 ** 20:.1f} MiB of prebuilt pair lists)")
print(f"condition (the native loss is not slower than the composed path on this shape): forward {f_n:.1f} vs {f_c:.1f} us, forward + backward "
      f"{b_n:.1f} vs {b_c:.1f} us: {'holds' if f_n <= f_c and b_n <= b_c else 'FAILS'}")

# ------------------------------------------------------------------------------------------------------------------ (c) a step
print("(c) a training step: batch + lookup + loss + backward + SparseAdam.step(), cache of 64 MB")
model = Node2Vec(g, D, L, C, walks_per_node=W, p=1.0, q=1.0, num_negative_samples=K, cache_mb=64, device="cuda:0", seed=1)
opt = SparseAdam(model.embedding, lr=0.01)
state = {}


def part_batch(i):
    state["b"] = model.sample(starts[i], step=i)


def part_lookup(i):
    model.embedding.reset_trace()
    state["h"] = model.embedding(state["b"].input_nodes)


def part_loss(i):
    state["l"] = skipgram_loss(state["h"], state["b"].pos, state["b"].neg, C, validate=False)


def part_backward(i):
    state["h"].grad = None
    state["l"].backward(retain_graph=True)


def part_step(i):
    opt.step()
    model.embedding.trace.append((state["b"].input_nodes, state["h"]))   # the next timed call steps the same rows again


def whole(i):
    loss = model.loss(model.sample(starts[i], step=i))
    loss.backward()
    opt.step()


for i in range(3):
    whole(i)
parts = []
for name, fn, before in (("walk_batch (with its host wait)", part_batch, ()), ("lookup (cache read of the input nodes)", part_lookup, (part_batch,)),
                         ("skipgram_loss forward", part_loss, (part_batch, part_lookup)), ("backward", part_backward, (part_batch, part_lookup, part_loss)),
                         ("SparseAdam.step()", part_step, (part_batch, part_lookup, part_loss, part_backward))):
    for f in before:           # the state the part needs, made once outside its timing: the parts behind walk_batch all see one batch
        f(REPS - 1)
    parts.append((name, alternate([fn])[0]))
model.embedding.reset_trace()
t_whole = alternate([whole])[0]
total = sum(t[0] for _, t in parts)
for name, t in parts:
    line(f"{name} ({100 * t[0] / total:.0f} % of the parts)", t)
line("the whole step, as a user writes it", t_whole)
print("not measured: q != 1 inside the whole step, other optimizers than SparseAdam, D other than 128 and walks other than 21 nodes (a shape near the "
      "LDS budget, (L + 1) D close to 16384, runs one wave per block and may be slower than the fallback), graphs that are not symmetric, "
      "more than one GPU")
model.close()
g.close()
print("done")
