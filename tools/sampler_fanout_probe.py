"""Sampler wall time per call for the BASELINE fan-outs and for full layers (fan-out -1), then a load-balance check of a full layer:
one star hub of 10^6 distinct in-neighbours against the same item count spread over 1,000 nodes of in-degree 1,000 (development
tool).

COALA_PARENT_LIB=<libcoala_hip.so of another commit> runs a side-by-side check instead (profiles/r13_sampler_refactor.txt): that
library is loaded twice (the second time from a copy, so that it is a load of its own) next to this build's, all three sample the
same graph with the same (seeds, seed, step), and
  1. every output of uniform, full, weighted and LABOR fan-out lists, with and without 8-way bucketing and edge ids, must be
     torch.equal between the parent's library and this build's (the script fails otherwise);
  2. the stream time per call (HIP events, median) is taken in the order parent, parent again, new, round after round; the two
     parent loads give the spread of the machine, and `new - parent` is printed beside it."""
import ctypes as C
import os, shutil, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "coala-gnn_amd"))
import torch
import COALA_GNN.sampler as sampler_module
from COALA_GNN_Pybind import _capi
from COALA_GNN.sampler import LaborSampler, NeighborSampler
from COALA_GNN.synthetic import powerlaw_csc
rows = 10_000_000
torch.cuda.set_device(0)
indptr, indices = powerlaw_csc(rows, 12.0, seed=0, device="cuda")
ids = torch.randperm(6_000_000, device="cuda")


def side_by_side(parent_path):
    def load(path):
        lib = C.CDLL(path)
        for name, (res, args) in _capi.SYMBOLS.items():
            if name.startswith("coala_sampler_"):
                getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
        return lib

    tmp = tempfile.mkdtemp()
    again = shutil.copy(parent_path, os.path.join(tmp, "libcoala_hip_parent_again.so"))
    libs = {"parent": load(parent_path), "parent again": load(again), "new": sampler_module._lib}
    assert len({lib._handle for lib in libs.values()}) == 3, "three separate loads"
    weights = torch.rand(indices.numel(), generator=torch.Generator().manual_seed(2)).cuda()
    weights[::7] = 0.0   # weight-0 edges are never taken
    graphs = {}
    for side, lib in libs.items():   # a sampler handle (workspace, status words, ticket) per library
        sampler_module._lib = lib
        graphs[side] = NeighborSampler.make_graph(indptr, indices, edata={"w": weights})

    def sample(side, smp, seeds, step):
        sampler_module._lib = libs[side]
        return smp.sample(graphs[side], seeds, step=step)

    def outputs(result):
        inp, _, blocks = result
        out = {"input_nodes": inp}
        for i, b in enumerate(blocks):
            for name in ("src_nodes", "nbr", "indptr", "indices", "dst_in_src", "owner_counts"):
                if getattr(b, name) is not None:
                    out[f"block {i} {name}"] = getattr(b, name)
            out[f"block {i} dst"] = b.dstdata["_ID"]
            if "_ID" in b.edata:
                out[f"block {i} edge ids"] = b.edata["_ID"]
            out[f"block {i} owner_counts_host"] = torch.tensor(b.owner_counts_host or [])
        return out

    kinds = [("uniform", [5, 5]), ("uniform", [15, 10, 5]), ("uniform", [32, 1]), ("uniform", [-1]), ("uniform", [10, -1]),
             ("weighted", [15, 10, 5]), ("labor", [10, 10])]

    def make(kind, fan, G=0, edge_ids=False):
        if kind == "labor":
            return LaborSampler(fan, seed=3, bucket_by_owner=G, edge_ids=edge_ids)
        return NeighborSampler(fan, seed=3, bucket_by_owner=G, edge_ids=edge_ids, prob="w" if kind == "weighted" else None)

    # ---- 1. bit identity
    n_cmp = 0
    for kind, fan in kinds:
        for G in (0, 8):
            for edge_ids in (False, True):
                smp = make(kind, fan, G, edge_ids)
                for step in range(3):
                    seeds = ids[step * 1024:(step + 1) * 1024]
                    want = outputs(sample("parent", smp, seeds, step))
                    got = outputs(sample("new", smp, seeds, step))
                    assert want.keys() == got.keys(), (kind, fan, G, edge_ids, sorted(want), sorted(got))
                    for name in want:
                        assert torch.equal(want[name], got[name]), f"{kind} {fan} bucketing {G} edge ids {edge_ids} step {step}: {name} differs"
                        n_cmp += 1
                print(f"bit identity: {kind} {fan}, bucketing {G}, edge ids {'on' if edge_ids else 'off'}: equal "
                      f"({want['input_nodes'].numel()} input nodes at step 2)", flush=True)
    print(f"bit identity: {n_cmp} tensors compared between the parent's library and this build's, all torch.equal")

    # ---- 2. stream time per call, the three loads taking turns
    ROUNDS, CALLS = 9, 60
    print(f"stream time per call in us (HIP events around sample(), 1024 seeds): per side the median over {ROUNDS} rounds of the median of "
          f"{CALLS} calls [fastest round .. slowest round]; spread = the larger of |parent - parent again| and a parent load's own "
          "range over its rounds")
    all_within = True
    for kind, fan in [("uniform", [5, 5]), ("uniform", [10, 10])] + kinds[1:2] + kinds[3:]:
        smp = make(kind, fan)
        for side in libs:
            for it in range(10):
                sample(side, smp, ids[it * 1024:(it + 1) * 1024], it)
        med = {side: [] for side in libs}
        for r in range(ROUNDS):
            for side in libs:
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
                for it, (a, b) in enumerate(ev):
                    a.record(); sample(side, smp, ids[(it + 10) * 1024:(it + 11) * 1024], r * CALLS + it); b.record()
                torch.cuda.synchronize()
                med[side].append(statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3)
        m = {side: statistics.median(v) for side, v in med.items()}
        spread = max(abs(m["parent"] - m["parent again"]), max(max(med[s]) - min(med[s]) for s in ("parent", "parent again")))
        diff = m["new"] - (m["parent"] + m["parent again"]) / 2
        within = diff <= spread
        all_within = all_within and within
        print(f"  {kind:8s} {str(fan):11s} " + "  ".join(f"{side} {m[side]:7.1f} [{min(med[side]):.1f} .. {max(med[side]):.1f}]" for side in libs)
              + f"  spread {spread:5.1f}  new - parent {diff:+5.1f}  {'within' if within else 'OUTSIDE'}", flush=True)
    print("every shape within the spread" if all_within else "a shape is OUTSIDE the spread")
    for side, g in graphs.items():
        sampler_module._lib = libs[side]
        g.close()
    sampler_module._lib = libs["new"]
    shutil.rmtree(tmp)


if os.environ.get("COALA_PARENT_LIB"):
    side_by_side(os.environ["COALA_PARENT_LIB"])
    sys.exit(0)
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
