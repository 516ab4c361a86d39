#!/usr/bin/env python3
"""Cost of the edge ids in the sampler and the weighted sum's rate beside the mean's on the same block (profiles/r08_edge_ids_weighted_sum.txt).

Sampler: 5,5 and 15,10,5 calls at the IGB-medium shape through the C ABI, with and without edge_ids_out, in alternating blocks in one
process.  COALA_PARENT_LIB=<libcoala_hip.so of another commit> adds that library's coala_sampler_sample to the alternation as the
baseline (it is loaded side by side; its outputs must equal this build's bit for bit).  Block ops: the input block of a 5,5 sample,
forward and backward launches timed with events, with the algorithmic bytes of each."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import torch  # noqa: E402
from COALA_GNN_Pybind import _capi, current_stream  # noqa: E402
from COALA_GNN.sampler import NeighborSampler  # noqa: E402
from COALA_GNN.synthetic import powerlaw_csc  # noqa: E402

new = _capi.load()
par = C.CDLL(os.environ["COALA_PARENT_LIB"]) if os.environ.get("COALA_PARENT_LIB") else None
for n in ("coala_sampler_create", "coala_sampler_destroy", "coala_sampler_sample"):
    if par is not None:
        getattr(par, n).restype, getattr(par, n).argtypes = _capi.SYMBOLS[n]

torch.cuda.set_device(0)
N, B = 10_000_000, 1024
ip, ix = powerlaw_csc(N, 12.0, seed=0, device="cuda")
E = ix.numel()
print(f"graph: {N} nodes, {E} edges (power law, mean in-degree 12): the IGB-medium shape of bench.py; batch {B}, uniform sampling")
hn, hp = C.c_void_p(), C.c_void_p()
_capi.check(new.coala_sampler_create(0, ip.data_ptr(), ix.data_ptr(), N, E, C.byref(hn)))
assert par is None or par.coala_sampler_create(0, ip.data_ptr(), ix.data_ptr(), N, E, C.byref(hp)) == 0
perm = torch.randperm(N, generator=torch.Generator().manual_seed(0))[: B * 64].cuda()
st = current_stream()

for fanouts in ([5, 5], [15, 10, 5]):
    rev = list(reversed(fanouts))
    L = len(rev)
    caps = [B]
    for f in rev:
        caps.append(caps[-1] * (f + 1))
    src = [torch.empty(caps[l + 1], dtype=torch.int64, device="cuda") for l in range(L)]
    nbr = [torch.empty(caps[l] * rev[l], dtype=torch.int32, device="cuda") for l in range(L)]
    eid = [torch.empty(caps[l] * rev[l], dtype=torch.int64, device="cuda") for l in range(L)]
    fan = (C.c_int32 * L)(*rev)
    src_p = (C.c_void_p * L)(*[t.data_ptr() for t in src])
    nbr_p = (C.c_void_p * L)(*[t.data_ptr() for t in nbr])
    eid_p = (C.c_void_p * L)(*[t.data_ptr() for t in eid])
    lay = (_capi.SamplerLayer * L)(*[_capi.SamplerLayer(src[l].data_ptr(), nbr[l].data_ptr(), None, caps[l + 1], caps[l] * rev[l]) for l in range(L)])
    n_src = (C.c_int64 * L)()

    def call(which, step):
        seeds = perm[(step % 64) * B: (step % 64 + 1) * B]
        if which == "parent":
            rc = par.coala_sampler_sample(hp, seeds.data_ptr(), B, fan, L, 1, step, src_p, nbr_p, n_src, None, None, st)
        elif which == "new, edge_ids off":
            rc = new.coala_sampler_sample(hn, seeds.data_ptr(), B, fan, L, 1, step, src_p, nbr_p, n_src, None, None, st)
        else:
            rc = new.coala_sampler_sample_layers_edge_ids(hn, seeds.data_ptr(), B, fan, L, 1, step, lay, None, eid_p, n_src, None, None, None, st)
        assert rc == 0

    kinds = (["parent"] if par is not None else []) + ["new, edge_ids off", "new, edge_ids on"]
    keep = {}
    for k in kinds:                      # same (seed, step): same sample from all three
        call(k, 7)
        torch.cuda.synchronize()
        keep[k] = ([t.clone() for t in src], [t.clone() for t in nbr], list(n_src))
    for k in kinds[1:]:
        assert keep[k][2] == keep[kinds[0]][2]
        for l in range(L):
            ns, ne = keep[k][2][l], (keep[k][2][l - 1] if l else B) * rev[l]
            assert torch.equal(keep[k][0][l][:ns], keep[kinds[0]][0][l][:ns]) and torch.equal(keep[k][1][l][:ne], keep[kinds[0]][1][l][:ne])
    for k in kinds:
        for s in range(30):
            call(k, s)
    rounds = {k: [] for k in kinds}
    for r in range(10):                  # alternating blocks of 100 calls; a call returns when the host has its counts
        for k in kinds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(100):
                call(k, r * 100 + s)
            torch.cuda.synchronize()
            rounds[k].append((time.perf_counter() - t0) / 100 * 1e6)
    slots = sum((keep[kinds[0]][2][l - 1] if l else B) * rev[l] for l in range(L))
    print(f"fan-out {fanouts}: {slots} neighbour slots per call ({slots * 8} bytes of ids); us per call, median of 10 blocks of 100 [min .. max]")
    for k in kinds:
        v = rounds[k]
        print(f"  {k:20s} {statistics.median(v):8.1f}  [{min(v):.1f} .. {max(v):.1f}]")

# ---- the weighted sum beside the mean, on the input block of a 5,5 sample (dim 1024 as the IGB features) and at dim 128
smp = NeighborSampler([5, 5], seed=1, edge_ids=True)
g = smp.make_graph(ip, ix)
_, _, blocks = smp.sample(g, perm[:B], step=0)
b = blocks[0]
deg = (b.nbr >= 0).sum().item()
print(f"block: {b.num_dst} dst, {b.num_src} src, fan-out 5, {deg} valid edges")


def timed(fn, reps=200):
    for _ in range(20):
        fn()
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(5):
        a.record()
        for _ in range(reps):
            fn()
        z.record()
        z.synchronize()
        out.append(a.elapsed_time(z) / reps * 1e3)
    return statistics.median(out), min(out), max(out)


for dim in (1024, 128):
    h = torch.randn(b.num_src, dim, device="cuda")
    w = torch.rand(b.num_dst, 5, device="cuda")
    go = torch.randn(b.num_dst, dim, device="cuda")
    out = torch.empty(b.num_dst, dim, device="cuda")
    gs = torch.zeros(b.num_src, dim, device="cuda")
    gw = torch.empty(b.num_dst, 5, device="cuda")
    nb = b.nbr
    mean_f = lambda: new.coala_block_mean_aggregate(0, nb.data_ptr(), h.data_ptr(), out.data_ptr(), b.num_dst, 5, dim, st)
    ws_f = lambda: new.coala_block_weighted_sum(0, nb.data_ptr(), w.data_ptr(), h.data_ptr(), out.data_ptr(), b.num_dst, 5, dim, st)
    mean_b = lambda: new.coala_block_mean_aggregate_backward(0, nb.data_ptr(), go.data_ptr(), gs.data_ptr(), b.num_dst, 5, dim, st)
    ws_b = lambda: new.coala_block_weighted_sum_backward(0, nb.data_ptr(), w.data_ptr(), h.data_ptr(), go.data_ptr(), gs.data_ptr(), gw.data_ptr(),
                                                         b.num_dst, 5, dim, st)
    ws_b_src = lambda: new.coala_block_weighted_sum_backward(0, nb.data_ptr(), w.data_ptr(), h.data_ptr(), go.data_ptr(), gs.data_ptr(), None,
                                                             b.num_dst, 5, dim, st)
    ws_b_w = lambda: new.coala_block_weighted_sum_backward(0, nb.data_ptr(), w.data_ptr(), h.data_ptr(), go.data_ptr(), None, gw.data_ptr(),
                                                           b.num_dst, 5, dim, st)
    row = 4 * dim
    byt = {"mean forward": deg * (row + 4) + b.num_dst * row, "weighted sum forward": deg * (row + 8) + b.num_dst * row,
           "mean backward": b.num_dst * row + deg * 4 + deg * row, "weighted sum backward (grad_src + grad_w)": b.num_dst * row + deg * 8 + 2 * deg * row + b.num_dst * 20,
           "weighted sum backward (grad_src only)": b.num_dst * row + deg * 8 + deg * row,
           "weighted sum backward (grad_w only)": b.num_dst * row + deg * 8 + deg * row + b.num_dst * 20}
    print(f"dim {dim}: us per launch, median of 5 x 200 [min .. max]; algorithmic bytes (atomic adds counted once); GB/s")
    for name, fn in (("mean forward", mean_f), ("weighted sum forward", ws_f), ("mean backward", mean_b),
                     ("weighted sum backward (grad_src + grad_w)", ws_b), ("weighted sum backward (grad_src only)", ws_b_src),
                     ("weighted sum backward (grad_w only)", ws_b_w)):
        med, lo, hi = timed(fn)
        print(f"  {name:44s} {med:8.1f} [{lo:.1f} .. {hi:.1f}]  {byt[name] / 1e6:8.2f} MB  {byt[name] / med / 1e3:8.1f} GB/s")
new.coala_sampler_destroy(hn)
if par is not None:
    par.coala_sampler_destroy(hp)
print("done")
