"""GPU sweep of the sampler with random call sequences on one handle (tests/_sampler_sweep.py).

What no sampling kernel owns is the state a handle carries from call to call: the clean extent of the hash table, the scan ticket and
generation, the shared scratch, the ring of pinned count slots.  Here one CSCGraph handle takes 24 calls of all six kinds in a row --
sizes on the lane-group, block and tile edges, up to 8 layers, both streams, every bucketing -- and every call is compared bit for
bit with the restatements of the per-kind tests before the next is issued; then every call is replayed alone on a fresh handle and
must give the same tensors.  tests/test_sampler_sweep_cpu.py shows that the sequences reach every path of the clean-extent protocol.

Measured on an MI355X (pytest --durations): test_sequence_matches_references 0.09 .. 0.11 s per seed (1.1 s for the first test of the
process, which warms the device up; the references are made once in 1.4 s of set-up), test_each_call_replays_on_a_fresh_handle 0.03 ..
0.05 s, test_eight_outstanding_calls_of_mixed_kinds 0.12 s, test_depth_eight_every_kind 0.03 .. 0.06 s; the file in under 4 s.  The parent
commit's sampler tests take 0.1 .. 1.4 s each on the same machine (its three end-to-end training runs 5 .. 6 s)."""
import numpy as np
import pytest

import _sampler_sweep as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sweep(hiplib, oracle):
    """seq_seed -> (graph, calls, classes, references): made once per seed and shared by the tests (nothing is modified)."""
    made = {}

    def get(seq_seed):
        if seq_seed not in made:
            desc, calls = S.make_sequence(seq_seed)
            graph = S.build_graph(desc)
            made[seq_seed] = (graph, calls, S.model_handle(calls, graph.max_in_degree), [S.reference(c, graph, oracle) for c in calls])
        return made[seq_seed]
    return get


def _begin(call, g, graph, side):
    """sample_begin of the call on its stream (0: the current stream, 1: `side`) -> (sampler, pending)"""
    import torch
    smp = S.make_sampler(call)
    seeds = S.seeds_of(call, graph)
    if call.stream == 1:
        with torch.cuda.stream(side):
            return smp, smp.sample_begin(g, torch.from_numpy(seeds).cuda(), step=call.step)
    return smp, smp.sample_begin(g, torch.from_numpy(seeds).cuda(), step=call.step)


def _sample(call, g, graph, side):
    smp, pending = _begin(call, g, graph, side)
    blocks = smp.sample_end(pending)[2]
    if call.stream == 1:
        side.synchronize()
    return blocks


@pytest.mark.parametrize("seq_seed", [1, 2, 3, 4, 5, 6])
def test_sequence_matches_references(sweep, seq_seed):
    import torch
    graph, calls, model, refs = sweep(seq_seed)
    g, side = S.make_device_graph(graph), torch.cuda.Stream()
    try:
        for i, (c, ref) in enumerate(zip(calls, refs)):
            S.check_call(c, _sample(c, g, graph, side), ref, S.describe(seq_seed, i, model[i][0], c))
    finally:
        g.close()


@pytest.mark.parametrize("seq_seed", [1, 2, 3])
def test_each_call_replays_on_a_fresh_handle(sweep, seq_seed):
    """Every call once inside the sequence and once alone on a new handle: every tensor of every block equal.  No reference: a
    difference here depends on the previous calls, whatever the kind."""
    import torch
    from COALA_GNN.sampler import CSCGraph
    graph, calls, model, _ = sweep(seq_seed)
    g, side = S.make_device_graph(graph), torch.cuda.Stream()
    try:
        for i, c in enumerate(calls):
            in_sequence = S.block_tensors(_sample(c, g, graph, side))
            fresh = CSCGraph(g.indptr, g.indices, edata=g.edata)
            try:
                alone = S.block_tensors(_sample(c, fresh, graph, side))
            finally:
                fresh.close()
            assert len(in_sequence) == len(alone)
            for (name, a), (_, b) in zip(in_sequence, alone):
                same = torch.equal(a, b) if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) else a is None and b is None or a == b
                assert same, f"{name} differs from the call alone on a fresh handle: " + S.describe(seq_seed, i, model[i][0], c)
    finally:
        g.close()


def _call(kind, fanouts, n, how="perm", G=0, eid=False, stream=0, rng_seed=0, **kw):
    d = dict(T=2, W=10, p=0.5, dep=False, seed=7, step=3)
    d.update(kw)
    return S.Call(kind, fanouts, n, how, rng_seed, d["seed"], d["step"], G, eid, d["dep"], d["T"], d["W"], d["p"], stream)


def test_eight_outstanding_calls_of_mixed_kinds(hiplib, oracle):
    """Eight calls begun before any is collected fill the ring of pinned count slots (kRing = 8); they are collected in a shuffled
    order; the ninth and tenth reuse slots 0 and 1."""
    import torch
    graph = S.build_graph(("hub", 1))
    calls = [_call("uniform", [5, 5], 257, G=3, eid=True), _call("labor", [5, 2], 255, eid=True, dep=True), _call("weighted", [5], 1025, G=8),
             _call("rel", [[1, 0, 2], [0, -1, 1]], 63, how="odd", eid=True), _call("walk", [3, 2], 256, how="odd", T=3, W=17, p=0.9),
             _call("full", [2, -1, 2], 65, how="nohub", eid=True), _call("walk", [2], 1024, G=64, T=1, W=1, p=0.0),
             _call("labor", [2], 5000, how="dup", step=2**64 - 1), _call("uniform", [32], 1, G=1, seed=2**64 - 5),
             _call("rel", [2, 2], 1023, G=3, eid=True)]
    calls = [c._replace(stream=i % 2, seeds_rng=100 + i) for i, c in enumerate(calls)]
    refs = [S.reference(c, graph, oracle) for c in calls]
    assert max(max(S.layer_items(c, r)) for c, r in zip(calls, refs)) <= S.ITEM_CAP
    assert all(S.smallest_margin(r) >= 1e-9 for c, r in zip(calls, refs) if c.kind == "weighted")
    g, side = S.make_device_graph(graph), torch.cuda.Stream()
    try:
        begun = [_begin(c, g, graph, side) for c in calls[:8]]
        for i in np.random.default_rng(5).permutation(8):
            smp, pending = begun[i]
            blocks = smp.sample_end(pending)[2]
            side.synchronize()
            S.check_call(calls[i], blocks, refs[i], f"outstanding call {i}: {calls[i]}")
        begun = [_begin(c, g, graph, side) for c in calls[8:]]
        for i, (smp, pending) in zip((8, 9), begun):
            blocks = smp.sample_end(pending)[2]
            side.synchronize()
            S.check_call(calls[i], blocks, refs[i], f"call {i}, behind eight others: {calls[i]}")
    finally:
        g.close()


@pytest.mark.parametrize("gkind", ["five", "hub"])
def test_depth_eight_every_kind(hiplib, oracle, gkind):
    """COALA_SAMPLER_MAX_LAYERS = 8 lays out the count words and the pinned words; one 8-layer call per kind, with and without
    bucket_by_owner=3, with edge ids where the kind has them.  Fan-outs 1 or 2, and a -1 layer on the five-node graph."""
    import torch
    graph = S.build_graph((gkind, 1))
    five = gkind == "five"
    plain = [2, 1, 1, 2, 1, 1, 1, 2]
    mixed = [2, 1, -1, 2, 1, 1, 1, 2] if five else plain
    rel = [1, [1, 0, 1], -1 if five else [0, 1, 1], [1, 1, 0], 1, [0, 1, 1], [1, 0, 1], 2]
    n, how = (5, "perm") if five else (16, "nohub")
    calls = [_call("full" if five else "uniform", mixed, n, how, eid=True), _call("weighted", mixed, n, how, eid=True, seed=2**64 - 5),
             _call("labor", mixed, n, how, eid=True, dep=True), _call("rel", rel, n, how, eid=True), _call("walk", plain, n, how, T=4, W=16, p=0.0),
             _call("labor", plain, n, how, step=2**64 - 1)]
    g, side = S.make_device_graph(graph), torch.cuda.Stream()
    try:
        for i, c in enumerate(calls):
            c = c._replace(seeds_rng=40 + i)
            ref = S.reference(c, graph, oracle)
            assert len(ref) == S.MAX_LAYERS and max(S.layer_items(c, ref)) <= S.ITEM_CAP and S.smallest_margin(ref) >= 1e-9
            for G in (0, 3):
                c = c._replace(G=G, stream=(i + G) % 2)
                S.check_call(c, _sample(c, g, graph, side), ref, f"8 layers on the {gkind} graph: {c}")
    finally:
        g.close()
