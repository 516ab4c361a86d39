"""CPU twin of the sampler sweep (tests/_sampler_sweep.py): what the sequences contain, what the host model says of them, and that the
references alone meet the conditions the GPU sweep relies on.  No GPU, no product library.

Reference time per sequence on the CPU, measured (test_references_run_within_the_cap_and_without_near_ties prints it): 0.26, 0.20, 0.28,
0.34, 0.26 and 0.19 s for seeds 1..6 -- far below the 5 s a sequence may take, so all 24 calls stay."""
import collections
import time

import numpy as np
import pytest

import _sampler_sweep as S

SEQ_SEEDS = [1, 2, 3, 4, 5, 6]
_MADE = {}


def _sequence(seq_seed, oracle):
    """(graph, calls, classes, references, seconds the references took), computed once per seed and shared (nothing is modified)."""
    if seq_seed not in _MADE:
        desc, calls = S.make_sequence(seq_seed)
        graph = S.build_graph(desc)
        t0 = time.perf_counter()
        refs = [S.reference(c, graph, oracle) for c in calls]
        _MADE[seq_seed] = (graph, calls, S.model_handle(calls, graph.max_in_degree), refs, time.perf_counter() - t0)
    return _MADE[seq_seed]


def test_sequences_are_deterministic():
    for s in SEQ_SEEDS:
        assert S.make_sequence(s) == S.make_sequence(s)
    assert S.make_sequence(1)[1] != S.make_sequence(4)[1]


@pytest.mark.parametrize("seq_seed", SEQ_SEEDS)
def test_every_sequence_contains_what_it_must(seq_seed):
    desc, calls = S.make_sequence(seq_seed)
    graph = S.build_graph(desc)
    N = len(graph.indptr) - 1
    assert len(calls) == S.N_CALLS
    assert {c.n_seeds for c in calls} >= set(S.SIZES), "a lane-group, block or tile edge is missing"
    kinds = collections.Counter(c.kind for c in calls)
    assert all(kinds[k] >= 2 for k in S.KINDS), kinds
    deep = {c.kind for c in calls if 6 <= len(c.fanouts) <= 8 and c.n_seeds <= 16}
    assert deep == set(S.KINDS) and any(len(c.fanouts) == S.MAX_LAYERS for c in calls)
    for c in calls:
        if len(c.fanouts) >= 6:
            flat = [x for f in c.fanouts for x in (f if isinstance(f, list) else [f])]
            assert all(x in (0, 1, 2) or (x == -1 and c.kind == "full") for x in flat), c   # a mixed-full list needs its -1
        assert c.G in S.OWNER_PARTS and c.stream in (0, 1) and 1 <= len(c.fanouts) <= S.MAX_LAYERS
        seeds = S.seeds_of(c, graph)
        assert len(seeds) == c.n_seeds
        plain = len(np.unique(seeds)) == len(seeds) and np.all((seeds >= 0) & (seeds < N))
        # repeated and out-of-range seeds go only to the kinds whose own GPU tests feed them; a bucketed call gets distinct nodes
        assert plain or (c.kind in ("labor", "rel", "walk") and c.G == 0), c
        if c.how == "odd":
            assert np.any(seeds >= N) and -1 not in [x for f in c.fanouts for x in (f if isinstance(f, list) else [f])]
    # ragged layer first, last and in the middle of a mixed list (DGL order: the first layer sampled is the last entry)
    mixed = {tuple(c.fanouts) for c in calls if not any(isinstance(f, list) for f in c.fanouts)}
    assert {(-1, 2, 2), (2, -1, 2), (2, 2, -1)} <= mixed
    assert {c.G for c in calls} == set(S.OWNER_PARTS)
    # size transitions: large -> small, small -> large, and a zero-seed call between two others
    n = [c.n_seeds for c in calls]
    assert any(a >= 1000 and 0 < b <= 2 for a, b in zip(n, n[1:])) and any(0 < a <= 64 and b >= 1000 for a, b in zip(n, n[1:]))
    assert any(a > 0 and b == 0 and c > 0 for a, b, c in zip(n, n[1:], n[2:]))
    # both directions of the stream hand-over
    st = [c.stream for c in calls]
    assert (0, 1) in set(zip(st, st[1:])) and (1, 0) in set(zip(st, st[1:]))
    assert any(c.how == "odd" for c in calls) and any(c.how == "dup" for c in calls)
    assert any(c.edge_ids for c in calls) and any(not c.edge_ids for c in calls)


def test_model_covers_every_class_and_the_invariant_holds():
    """Every class of the host model occurs at least twice over the six sequences and every kind in at least three classes: the sweep
    reaches every path through the handle's clean-extent protocol.  The model's verdict on "the first layer's table prefix is clean at
    the start of the call" is `holds` for every call; if it ever is not, that is the bug: read launch_call."""
    per_class, per_kind = collections.Counter(), collections.defaultdict(set)
    for s in SEQ_SEEDS:
        desc, calls = S.make_sequence(s)
        model = S.model_handle(calls, S.build_graph(desc).max_in_degree)
        for i, (c, (cls, moved, holds)) in enumerate(zip(calls, model)):
            assert cls in S.CLASSES
            assert holds, "the table prefix is not clean: " + S.describe(s, i, cls, c)
            for name in [cls] + (["moved_stream"] if moved else []):
                per_class[name] += 1
                per_kind[c.kind].add(name)
        assert model[0][0] == "first" and not model[0][1]
        # the verdict is not vacuous: without launch_call's memsets exactly the calls that need them start on a dirty table
        broken = S.model_handle(calls, S.build_graph(desc).max_in_degree, memsets=False)
        fixed0 = [not S.layers_of(c)[0][0] and c.n_seeds > 0 for c in calls]
        assert [not b[2] for b in broken] == [f and (m[0] in ("grown", "memset") or (m[0] == "first")) for f, m in zip(fixed0, model)]
    print("calls per class over the six sequences:", dict(per_class))
    assert all(per_class[name] >= 2 for name in S.CLASSES), per_class
    assert all(len(per_kind[k]) >= 3 for k in S.KINDS), dict(per_kind)


def test_model_restates_the_table_arithmetic():
    assert [S.table_size(n) for n in (0, 1, 512, 513, 1024, 6150, S.ITEM_LIMIT)] == [1024, 1024, 1024, 2048, 2048, 16384, 2**24]
    c = S.Call("uniform", [5, 2], 100, "perm", 0, 0, 0, 0, False, False, 2, 10, 0.5, 0)
    assert S.plan(c, 9) == [300, 1800]                            # exact host bounds: cap * (f + 1)
    c = c._replace(kind="full", fanouts=[5, -1])
    assert S.plan(c, 9) == [1000, 6000]                           # cap + cap * max_in_degree, then bounded fixed layers
    c = c._replace(kind="rel", fanouts=[[1, 0, 2], [0, -1, 1]])
    assert S.plan(c, 9) == [1000, 4000]                           # a layer without -1: min(total, max_in_degree) edges per row
    c = c._replace(kind="labor", fanouts=[2], n_seeds=5000)
    assert S.plan(c, 5000) == [S.ITEM_LIMIT]
    # grown -> reuse -> memset -> ragged inherits the extent -> a fixed call inside it is reused
    mk = lambda kind, f, n, st=0: S.Call(kind, f, n, "perm", 0, 0, 0, 0, False, False, 2, 10, 0.5, st)
    seq = [mk("uniform", [2], 10), mk("uniform", [5], 2000), mk("uniform", [2], 10, 1), mk("uniform", [5], 1000, 1), mk("labor", [2], 4),
           mk("uniform", [5], 1000), mk("uniform", [1], 0), mk("uniform", [5], 1400)]
    got = S.model_handle(seq, 3)
    assert [g[0] for g in got] == ["first", "grown", "reuse", "memset", "ragged_inherits", "reuse", "empty", "memset"]
    assert [g[1] for g in got] == [False, False, True, False, True, False, False, False] and all(g[2] for g in got)


@pytest.mark.parametrize("seq_seed", SEQ_SEEDS)
def test_references_run_within_the_cap_and_without_near_ties(oracle, seq_seed):
    graph, calls, model, refs, seconds = _sequence(seq_seed, oracle)
    print(f"sequence seed {seq_seed}: references took {seconds:.2f} s")
    for i, (c, r) in enumerate(zip(calls, refs)):
        where = S.describe(seq_seed, i, model[i][0], c)
        assert len(r) == len(c.fanouts), where
        assert max(S.layer_items(c, r)) <= S.ITEM_CAP, f"{S.layer_items(c, r)} items: {where}"
        if c.kind == "weighted":    # a thousand times the tie bound: no row may be tolerated on the device
            assert S.smallest_margin(r) >= 1e-9, f"margin {S.smallest_margin(r)}: {where}"
    assert any(np.isfinite(S.smallest_margin(r)) for c, r in zip(calls, refs) if c.kind == "weighted") or len(graph.indptr) == 6


@pytest.mark.parametrize("seq_seed", [1, 2, 3])
def test_uniform_edge_ids_name_the_twins_neighbours(oracle, seq_seed):
    """uniform_ids is put together from the relation sampler's restated draw; on these multigraphs the CPU twin cannot name a position,
    but the node at every restated position must be the neighbour the twin sampled."""
    graph, calls, _, refs, _ = _sequence(seq_seed, oracle)
    seen = 0
    for c, ref in zip(calls, refs):
        if c.kind not in ("uniform", "full"):
            continue
        for r, f in zip(ref, reversed(c.fanouts)):
            if f == -1:
                continue
            nb = np.where(r["loc"] >= 0, r["src"][np.maximum(r["loc"], 0)], -1)
            assert np.array_equal(np.where(r["eid"] >= 0, graph.indices[np.maximum(r["eid"], 0)], -1), nb), c
            seen += int((r["eid"] >= 0).sum())
    assert seen > 0


def test_checker_rejects_a_wrong_block(oracle):
    """check_call on blocks made from the reference itself passes; one stale local index, one missing source node or one wrong edge id
    fails it."""
    import torch
    graph, calls, _, refs, _ = _sequence(1, oracle)

    class FakeBlock(object):
        def __init__(self, r, n_dst, f, eid):
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
            self.src_nodes, self.num_dst, self.dst_in_src, self.owner_counts = t(r["src"]), n_dst, None, None
            self.nbr = t(r["loc"]) if r["ind"] is None else None
            self.indptr = t(r["ind"]) if r["ind"] is not None else None
            self.indices = t(r["loc"]) if r["ind"] is not None else None
            self.edata = {"_ID": t(r["eid"])} if eid else {}
            if "ew" in r:
                self.edata["edge_weights"] = t(r["ew"])
            if "cnt" in r:
                self.edata.update(visit_counts=t(r["cnt"]), weights=t(r["cnt"].astype(np.float32)))

    def blocks_of(c, ref):
        out, n_dst = [], c.n_seeds
        for r, f in zip(ref, reversed(c.fanouts)):
            out.insert(0, FakeBlock(r, n_dst, f, c.edge_ids))
            n_dst = len(r["src"])
        return out

    tried = set()
    for c, ref in zip(calls, refs):
        if not c.n_seeds or c.kind in tried or len(ref[0]["src"]) < 3:
            continue
        c = c._replace(G=0)     # the reference does not depend on the bucketing
        tried.add(c.kind)
        S.check_call(c, blocks_of(c, ref), ref)
        for field in ("src", "loc") + (("eid",) if c.edge_ids else ()):
            bad = [dict(r) for r in ref]
            a = bad[0][field].copy()
            if a.size == 0:
                continue
            flat = a.reshape(-1)
            flat[-1] = flat[-1] + 1 if field != "loc" else (0 if flat[-1] != 0 else 1)
            bad[0][field] = a
            with pytest.raises(AssertionError):
                S.check_call(c, blocks_of(c, bad), ref)
    assert tried == set(S.KINDS)
