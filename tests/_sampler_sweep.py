"""Randomized call sequences on one sampler handle (tests only): the sequences, a host model of the handle, and the checker.

The sampler kernels are pinned kind by kind elsewhere; what no kernel owns is the state a handle carries from call to call -- the clean
extent of the hash table, the scan ticket and generation, the shared scratch, the ring of pinned count slots.  make_sequence(seq_seed)
gives a graph description and 24 calls of all six kinds (uniform, mixed-full, weighted, LABOR, per-relation, random-walk) whose sizes
sit on the lane-group, block and tile edges, with every size transition, depths up to COALA_SAMPLER_MAX_LAYERS = 8, both streams and all
bucketings.  model_handle() restates the host arithmetic of table_size / plan_call / grow_workspace / launch_call (coala_sampler.hip) and
classifies every call by the path it takes through that state; reference() / check_call() compare a call's blocks bit for bit with the
restatements the per-kind tests use (_full_ref, _weighted_ref, _labor_ref, _rel_fanout_ref, _pinsage_ref, _edge_id_ref).
Importable without a GPU; torch is imported only where a block is read."""
import functools
from collections import namedtuple

import numpy as np

import _labor_ref
import _pinsage_ref
import _rel_fanout_ref
import _weighted_ref
from _edge_id_ref import full_ids
from _full_ref import bucketed, fixed_layer, full_layer
from _util import csc_from_columns, edge_case_graph

KINDS = ("uniform", "full", "weighted", "labor", "rel", "walk")
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000)      # lane group, block and tile (kTile = 1024) edges
OWNER_PARTS = (0, 1, 3, 8, 64)
CLASSES = ("first", "grown", "memset", "reuse", "ragged_after_grow", "ragged_inherits", "empty", "moved_stream")
ITEM_CAP = 300_000                  # no layer of a sweep call holds more items (destination nodes + neighbour slots / edges)
ITEM_LIMIT = 8192 * 1024            # kItemLimit
MAX_LAYERS = 8                      # COALA_SAMPLER_MAX_LAYERS
HUB = 5000                          # above kHubDegree = 4096
NUM_RELS = 3
TIE = 1e-12                         # rows whose f-th and (f+1)-th restated fp64 keys are this close may resolve either way on the device
N_CALLS = 24

# kind: one of KINDS.  fanouts: DGL order (the first layer sampled is the last entry); of a rel call every entry is an int or a list of
# NUM_RELS ints.  how: 'perm' distinct nodes of the graph, 'nohub' the same without the last node, 'dup' nodes drawn with repetition,
# 'odd' the same with out-of-range ids among them.  seeds_rng: the default_rng seed the seeds are drawn from.  G: bucket_by_owner.
# dep: LaborSampler's layer_dependency.  T, W, p: the walk's num_traversals, num_random_walks, termination_prob.  stream: 0 or 1.
Call = namedtuple("Call", "kind fanouts n_seeds how seeds_rng seed step G edge_ids dep T W p stream")
Graph = namedtuple("Graph", "indptr indices etype weights max_in_degree")


# ---------------------------------------------------------------------------------------------------------------- graphs
@functools.lru_cache(maxsize=None)
def _build_graph(kind, seed):
    rng = np.random.default_rng(500 + seed)
    if kind == "typed":
        ip, ix, et, _ = _rel_fanout_ref.typed_edge_case_graph([1, 5, 32], NUM_RELS, n_plain=3000, hub_degree=HUB, seed=seed)
    else:
        if kind == "hub":
            ip, ix, _ = edge_case_graph([1, 5, 32], n_plain=3000, hub_degree=HUB, seed=seed)
        else:   # five nodes: a self-loop, a node of degree 0, a repeated in-neighbour
            ip, ix = csc_from_columns([[0, 1], [], [3, 3, 4], [2], [0, 2, 1]])
        et = rng.integers(0, NUM_RELS, size=len(ix)).astype(np.int64)
        perm = _rel_fanout_ref.sort_by_type(ip, et)       # RelNeighborSampler needs every row sorted by type
        ix, et = ix[perm], et[perm]
    w = (1.0 - rng.random(len(ix))).astype(np.float32)   # (0, 1]
    w[rng.random(len(ix)) < 0.1] = 0
    for a in (ip, ix, et, w):
        a.setflags(write=False)
    return Graph(ip, ix, et, w, int(np.diff(ip).max()))


def build_graph(desc):
    """desc: (kind, seed) as make_sequence returns it -> Graph (shared, read-only)."""
    return _build_graph(*desc)


def seeds_of(call, graph):
    N = len(graph.indptr) - 1
    rng = np.random.default_rng(call.seeds_rng)
    n = call.n_seeds
    if call.how in ("perm", "nohub"):
        pool = N - 1 if call.how == "nohub" and N > 5 else N
        assert n <= pool, (call, N)
        return rng.permutation(pool)[:n].astype(np.int64)
    s = rng.integers(0, N, size=n).astype(np.int64)
    if call.how == "odd" and n:
        bad = [N + 5, N, 2**40] + ([-1] if call.kind == "walk" else [])
        at = rng.permutation(n)[: min(len(bad), n)]
        s[at] = bad[: len(at)]
        if n > 8:
            s[rng.permutation(n)[:4]] = s[0]               # and a node four times over
    return s


# ---------------------------------------------------------------------------------------------------------------- sequences
def _rel_total(f):
    per = list(f) if hasattr(f, "__iter__") else [f] * NUM_RELS
    return -1 if -1 in per else sum(per)


def layers_of(call):
    """The call's layers in sampling order: [(ragged, fan-out)]; of a rel layer the total of its fan-outs, -1 when one of them is -1."""
    out = []
    for f in reversed(call.fanouts):
        if call.kind == "rel":
            out.append((True, _rel_total(f)))
        elif call.kind == "labor":
            out.append((True, f))
        else:
            out.append((f == -1, f))
    return out


def make_sequence(seq_seed):
    """-> ((graph kind, graph seed), [Call] * 24), deterministic in seq_seed."""
    rng = np.random.default_rng(7000 + seq_seed)
    gkind = ("hub", "typed", "five")[(seq_seed - 1) % 3]
    five = gkind == "five"
    fixed3, dup3 = ("uniform", "weighted", "walk"), ("labor", "rel", "walk")
    rot = seq_seed % 3
    walks = [(2, 10, 0.5), (3, 17, 0.9), (4, 16, 0.0), (1, 1, 0.0)]
    ones = lambda n: [int(x) for x in rng.integers(1, 3, size=n)]          # fan-outs 1 or 2

    def rel_fans(n):
        menu = [[1, 0, 1], 1, [1, 1, 0], [0, 1, 1]]
        return [menu[int(i)] for i in rng.integers(0, len(menu), size=n)]

    def fans(kind, spec):
        """spec: an explicit list, or a layer count (fan-outs 1 or 2; of a rel call, small fan-outs per relation)."""
        if isinstance(spec, int):
            return rel_fans(spec) if kind == "rel" else ones(spec)
        return list(spec)

    calls = []

    def add(kind, spec, n, how="perm", stream=None, eid=None, five_kind=None):
        if five and kind in ("uniform", "full", "weighted") and n > 2:    # five nodes: only the kinds that take repeated seeds grow
            if five_kind is None:
                n = 2
            else:
                kind, how = five_kind, "dup"
                if kind == "walk" and isinstance(spec, list):              # a walk layer has no -1
                    spec = [f if f != -1 else 2 for f in spec]
        if five and kind in dup3 and how in ("perm", "nohub") and n > 5:
            how = "dup"
        T, W, p = walks[int(rng.integers(0, len(walks)))]
        seed = [0, 7, 2**64 - 5, int(rng.integers(0, 2**62))][int(rng.integers(0, 4))]
        step = [0, 3, 2**64 - 1, int(rng.integers(0, 2**62))][int(rng.integers(0, 4))]
        if eid is None:
            eid = kind == "rel" or (kind != "walk" and bool(rng.integers(0, 2)))
        if stream is None:
            stream = int(rng.integers(0, 2))
        calls.append(Call(kind, fans(kind, spec), n, how, int(rng.integers(0, 2**31)), seed, step, 0, bool(eid), bool(rng.integers(0, 2)), T, W, p, stream))

    a, b, c = (fixed3[(rot + i) % 3] for i in range(3))
    x, y, z = (dup3[(rot + i) % 3] for i in range(3))
    # the table grows, is reused, is cleared again: small -> large -> none -> small -> medium, on alternating streams
    if seq_seed % 2:
        add(a, [2], 64, stream=0, five_kind="walk")                        # first
    else:
        add(x if x != "walk" else y, [2], 64, stream=0)                    # first, with a ragged first layer
    add(b, [5, 5], 1025, stream=0, five_kind="walk")                       # grown
    add(x, [2, 2], 0, stream=1)                                            # empty between two others; the stream moves
    add("uniform" if five else c, [2], 2, stream=1)                        # reuse
    add(a, [5], 257, stream=0, five_kind="walk")                           # memset; the stream moves back
    add(y, [5, 2], 63, stream=0)                                           # ragged first layer
    add("full", [2, 2, -1], 65, how="nohub", stream=1, five_kind="labor")
    add("labor", MAX_LAYERS, 16, how="nohub")                              # exactly 8 layers
    add("uniform", [2, -1, 2], 255, how="nohub", five_kind="rel")
    add("weighted", [5], 256, five_kind="labor")
    add("walk", [3], 1023, how="dup")
    add("labor", [5, 5], 134, how="odd", eid=True)
    add("rel", [[1, 0, 2], 5], 134, how="odd")
    add("walk", [3, 2], 134, how="odd")
    add(z, [2], 5000, how="dup")                                           # small -> large
    add(b, [32], 1)                                                        # large -> small
    add(y, [3], 0)                                                         # none
    add(c, [5, 5], 1024, five_kind="rel")                                  # small -> large
    add("full", [-1, 2, 2], 63, how="nohub")
    add("uniform", MAX_LAYERS, 16, how="nohub")
    add("full", [1, 1, 2, 1, 1, -1] if not five else [2, -1, 1, 2, -1, 1, -1], 16, how="nohub")
    add("weighted", 6, 16, how="nohub")
    add("rel", 7, 16, how="nohub")
    add("walk", 6, 16, how="nohub" if not five else "dup")
    assert len(calls) == N_CALLS
    # owner bucketing wants distinct nodes of the graph: every G goes round the calls that have them
    parts = [int(g) for _ in range(5) for g in rng.permutation(OWNER_PARTS)]
    for j, i in enumerate(i for i, c in enumerate(calls) if c.how in ("perm", "nohub")):
        calls[i] = calls[i]._replace(G=parts[j])
    return (gkind, seq_seed), calls


# ---------------------------------------------------------------------------------------------------------------- host model
def table_size(n_items):
    t = 1024
    while t < 2 * n_items:
        t <<= 1
    return t


def plan(call, max_in_degree):
    """The capacities the Python sampler passes and plan_call derives: -> items_cap of every layer, in sampling order."""
    cap, bounded, items = call.n_seeds, False, []
    for ragged, f in layers_of(call):
        if ragged:
            row = max_in_degree if call.kind != "rel" or f == -1 else min(f, max_in_degree)
            src_cap = min(cap + min(cap * row, ITEM_LIMIT), ITEM_LIMIT)
            bounded = True
        else:
            src_cap = min(cap * (f + 1), ITEM_LIMIT) if bounded else cap * (f + 1)
        items.append(src_cap)
        cap = src_cap
    return items


def model_handle(calls, max_in_degree, memsets=True):
    """The handle's host state over a sequence -> [(class, moved_stream, invariant holds)] per call.  The invariant: at the start of the
    call the first layer's table prefix is clean (and inside the allocation).  `known` is what the last kernels really left clean.
    memsets=False models a launch_call that never clears a stale table: the verdict must then fail (the CPU twin checks that it does)."""
    table_cap = clean_items = known = n_calls = 0
    last_stream, out = None, []
    for c in calls:
        moved = n_calls > 0 and c.stream != last_stream
        last_stream = c.stream
        items = plan(c, max_in_degree)
        grew = table_size(max(items)) > table_cap
        if grew:                                          # grow_workspace: a new table, nothing known about it
            table_cap, clean_items, known = table_size(max(items)), 0, 0
        ragged0, f0 = layers_of(c)[0]
        if c.n_seeds == 0:                                # empty_call: nothing is launched
            cls, holds = "empty", True
        elif ragged0:                                     # table_clear_kernel clears what the device counted; the extent is inherited
            cls = "ragged_after_grow" if clean_items == 0 else "ragged_inherits"
            items0 = max(clean_items, 1)
            holds = table_size(items0) <= table_cap and table_size(items[0]) <= table_cap
        else:
            items0 = c.n_seeds * (f0 + 1)
            stale = clean_items == 0 or table_size(items0) > table_size(clean_items)
            if stale and memsets:                         # the memsets of launch_call
                known = max(known, table_size(items0))
            cls = "grown" if grew else "memset" if stale else "reuse"
            holds = table_size(items0) <= known and table_size(items0) <= table_cap
        if c.n_seeds:
            clean_items, known = items0, table_size(items0)     # the last relabel_clear of the call
        out.append(("first" if n_calls == 0 else cls, moved, holds))
        n_calls += 1
    return out


# ---------------------------------------------------------------------------------------------------------------- references
def uniform_ids(indptr, dst, f, seed, step, layer):
    """Edge ids of a uniform fixed layer on any graph (repeated edges included): slot c of a row of more than f in-edges holds Floyd's
    c-th pick (the relation sampler's draw with one relation), a shorter row its edges in order.  int64 [n_dst, f], -1 padded."""
    dst = np.asarray(dst, dtype=np.int64)
    deg = indptr[dst + 1] - indptr[dst]
    pos = np.where(np.arange(f)[None, :] < deg[:, None], np.arange(f)[None, :], -1).astype(np.int64)
    drawn = np.nonzero(deg > f)[0]
    if len(drawn):
        pos[drawn] = _rel_fanout_ref.floyd_picks(_rel_fanout_ref.sample_key(seed, step, layer, dst[drawn]), 0, deg[drawn], f)
    return np.where(pos >= 0, indptr[dst][:, None] + pos, -1)


def reference(call, graph, oracle, seeds=None):
    """Every layer of the call in sampling order, as dicts: src, ind (None: fixed), loc, eid (None: walk), and per kind margin (weighted
    fixed layers), ew (LABOR edge weights), cnt (walk visit counts)."""
    ip, ix = graph.indptr, graph.indices
    seeds = seeds_of(call, graph) if seeds is None else seeds
    rev = list(reversed(call.fanouts))
    out = []
    if call.kind == "labor":
        for src, ind, loc, eid in _labor_ref.reference_layers(ip, ix, seeds, rev, call.seed, call.step, call.dep):
            out.append(dict(src=src, ind=ind, loc=loc, eid=eid, ew=_labor_ref.edge_weights(ind)))
    elif call.kind == "rel":
        per_rel = _rel_fanout_ref.expand_fanouts(rev, NUM_RELS)
        for src, ind, loc, eid in _rel_fanout_ref.reference_layers(ip, ix, graph.etype, seeds, per_rel, call.seed, call.step):
            out.append(dict(src=src, ind=ind, loc=loc, eid=eid))
    elif call.kind == "walk":
        thr = _pinsage_ref.threshold(call.p)
        for src, loc, cnt, _ in _pinsage_ref.reference_layers(ip, ix, seeds, rev, call.T, call.W, thr, call.seed, call.step):
            out.append(dict(src=src, ind=None, loc=loc, eid=None, cnt=cnt))
    else:
        dst = seeds
        for layer, f in enumerate(rev):
            if f == -1:
                src, ind, loc = full_layer(ip, ix, dst)
                out.append(dict(src=src, ind=ind, loc=loc, eid=full_ids(ip, dst)))
            elif call.kind == "weighted":
                src, loc, pos, margin = _weighted_ref.weighted_layer(ip, ix, graph.weights, dst, f, call.seed, call.step, layer)
                out.append(dict(src=src, ind=None, loc=loc, eid=np.where(pos >= 0, ip[dst][:, None] + pos, -1), margin=margin))
            else:
                src, loc = fixed_layer(oracle, np.ascontiguousarray(ip), np.ascontiguousarray(ix), dst, f, call.seed, call.step, layer)
                out.append(dict(src=src, ind=None, loc=loc, eid=uniform_ids(ip, dst, f, call.seed, call.step, layer)))
            dst = src
    return out


def layer_items(call, refs):
    """Items (destination nodes + neighbour slots or edges) of every layer, from the reference."""
    n_dst, out = call.n_seeds, []
    for r, f in zip(refs, reversed(call.fanouts)):
        out.append(n_dst + (int(r["ind"][-1]) if r["ind"] is not None else n_dst * f))
        n_dst = len(r["src"])
    return out


def smallest_margin(refs):
    """The smallest finite relative gap between the f-th and (f+1)-th keys over all rows of a weighted call's fixed layers (inf: none)."""
    m = [r["margin"][np.isfinite(r["margin"])] for r in refs if r.get("margin") is not None]
    m = np.concatenate(m) if m else np.zeros(0)
    return float(m.min()) if len(m) else float("inf")


# ---------------------------------------------------------------------------------------------------------------- samplers and checks
def make_sampler(call):
    from COALA_GNN.sampler import LaborSampler, NeighborSampler, RandomWalkNeighborSampler, RelNeighborSampler
    if call.kind == "labor":
        return LaborSampler(call.fanouts, seed=call.seed, bucket_by_owner=call.G, edge_ids=call.edge_ids, layer_dependency=call.dep)
    if call.kind == "rel":
        return RelNeighborSampler(call.fanouts, NUM_RELS, seed=call.seed, bucket_by_owner=call.G, edge_ids=call.edge_ids)
    if call.kind == "walk":
        return RandomWalkNeighborSampler(call.fanouts, call.T, call.p, call.W, seed=call.seed, bucket_by_owner=call.G)
    return NeighborSampler(call.fanouts, seed=call.seed, bucket_by_owner=call.G, prob="w" if call.kind == "weighted" else None,
                           edge_ids=call.edge_ids)


def make_device_graph(graph):
    import torch
    from COALA_GNN.sampler import CSCGraph
    dev = [torch.from_numpy(np.array(a)).cuda() for a in graph[:4]]   # a copy: the shared arrays are read-only
    return CSCGraph(dev[0], dev[1], edata={"etype": dev[2], "w": dev[3]})


def check_weighted_layers(blocks, ref, rev, n_seeds, step):
    """The rule of the weighted tests: every layer equal to the restatement (_weighted_ref.reference_layers' tuples), near-tie rows
    excepted and counted.  -> tolerated rows"""
    n_dst, tolerated = n_seeds, 0
    for l, (src_r, ind_r, loc_r, margin) in enumerate(ref):
        b = blocks[len(rev) - 1 - l]
        where = f"layer {l} of {rev}, {n_seeds} seeds, step {step}"
        assert b.num_dst == n_dst, where
        src = b.src_nodes.cpu().numpy()
        if ind_r is not None:
            assert np.array_equal(src, src_r) and np.array_equal(b.indptr.cpu().numpy(), ind_r), where
            assert np.array_equal(b.indices.cpu().numpy(), loc_r), where
        else:
            loc = b.nbr.cpu().numpy()
            got = np.where(loc >= 0, src[np.maximum(loc, 0)], -1)
            want = np.where(loc_r >= 0, src_r[np.maximum(loc_r, 0)], -1)
            bad = np.nonzero((got != want).any(1))[0]
            assert np.all(margin[bad] < TIE), f"rows {bad[:8]} differ beyond a near tie: {where}"
            tolerated += len(bad)
            if len(bad):     # the source lists of this layer and the next differ from here on: stop comparing
                return tolerated
            assert np.array_equal(src, src_r), f"source list differs: {where}"
            assert np.array_equal(loc, loc_r), f"nbr_local differs: {where}"
        n_dst = len(src_r)
    return tolerated


def check_weighted_call(smp, g, ip, ix, w, seeds, step, stream=None):
    """One weighted sample: every layer equal to the restatement (near-tie rows excepted and counted).  -> (blocks, tolerated rows)"""
    import torch
    if stream is None:
        _, _, blocks = smp.sample(g, torch.from_numpy(seeds).cuda(), step=step)
    else:
        with torch.cuda.stream(stream):
            _, _, blocks = smp.sample(g, torch.from_numpy(seeds).cuda(), step=step)
        stream.synchronize()
    rev = list(reversed(smp.fanouts))
    ref = _weighted_ref.reference_layers(ip, ix, w, seeds, rev, smp.seed, step)
    return blocks, check_weighted_layers(blocks, ref, rev, len(seeds), step)


def check_call(call, blocks, refs, where=""):
    """Every layer of the call's blocks against the reference, bit for bit: source list, nbr or indptr / indices, edge ids, LABOR edge
    weights, walk visit counts; the bucketed input layer through _full_ref.bucketed.  `where` names the call in a failure."""
    rev = list(reversed(call.fanouts))
    L, G = len(rev), call.G
    assert len(blocks) == L == len(refs), where
    if call.kind == "weighted" and G == 0:   # the weighted tests' rule, with no tolerated row: the reference's margins are all >= 1e-9
        tuples = [(r["src"], r["ind"], r["loc"], r.get("margin")) for r in refs]
        try:
            tolerated = check_weighted_layers(blocks, tuples, rev, call.n_seeds, call.step)
        except AssertionError as e:
            raise AssertionError(f"{e}: {where}") from None
        assert tolerated == 0, f"a row within a near tie: {where}"
    n_dst = call.n_seeds
    for l, r in enumerate(refs):
        b = blocks[L - 1 - l]
        at = f"layer {l}: {where}"
        assert b.num_dst == n_dst, at
        src, loc_r = b.src_nodes.cpu().numpy(), r["loc"]
        if G > 0 and l == L - 1:             # the input layer: owner-bucketed source list, the block re-indexed through the permutation
            want, sizes, new_of_old = bucketed(r["src"], G)
            assert np.array_equal(src, want), f"bucketed source list differs, {at}"
            assert b.owner_counts.cpu().tolist() == b.owner_counts_host == sizes.tolist(), f"owner counts differ, {at}"
            assert np.array_equal(b.dst_in_src.cpu().numpy(), new_of_old[:n_dst]), f"dst_in_src differs, {at}"
            loc_r = np.where(loc_r >= 0, new_of_old[np.maximum(loc_r, 0)], -1)
        else:
            assert b.dst_in_src is None and np.array_equal(src, r["src"]), f"source list differs, {at}"
        if r["ind"] is not None:
            assert b.nbr is None and np.array_equal(b.indptr.cpu().numpy(), r["ind"]), f"indptr differs, {at}"
            assert np.array_equal(b.indices.cpu().numpy(), loc_r), f"indices differ, {at}"
        else:
            assert b.indptr is None and tuple(b.nbr.shape) == (n_dst, rev[l]), at
            assert np.array_equal(b.nbr.cpu().numpy(), loc_r), f"nbr differs, {at}"
        if call.edge_ids:
            eid = b.edata["_ID"].cpu().numpy()
            assert eid.dtype == np.int64 and eid.shape == r["eid"].shape and np.array_equal(eid, r["eid"]), f"edge ids differ, {at}"
        else:
            assert "_ID" not in b.edata, at
        if "ew" in r:
            ew = b.edata["edge_weights"].cpu().numpy()
            assert ew.dtype == np.float32 and np.array_equal(ew.view(np.int32), r["ew"].view(np.int32)), f"edge weights differ, {at}"
        if "cnt" in r:
            cnt = b.edata["visit_counts"].cpu().numpy()
            assert cnt.dtype == np.int32 and np.array_equal(cnt, r["cnt"]), f"visit counts differ, {at}"
            assert np.array_equal(b.edata["weights"].cpu().numpy(), r["cnt"].astype(np.float32)), f"weights differ, {at}"
        n_dst = len(r["src"])


def block_tensors(blocks):
    """Every tensor of every block, named: what test_each_call_replays_on_a_fresh_handle compares with torch.equal."""
    out = []
    for i, b in enumerate(blocks):
        for name in ("src_nodes", "nbr", "indptr", "indices", "dst_in_src", "owner_counts"):
            out.append((f"blocks[{i}].{name}", getattr(b, name, None)))
        out.append((f"blocks[{i}].num_dst", b.num_dst))
        for key in ("_ID", "visit_counts", "edge_weights"):
            out.append((f"blocks[{i}].edata[{key}]", b.edata[key] if key in b.edata else None))
    return out


def describe(seq_seed, index, cls, call):
    return f"sequence seed {seq_seed}, call {index}, class {cls}: {call}"
