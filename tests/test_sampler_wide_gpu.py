"""GPU tests of the sampler on a graph of more than 2^32 edges (the scale of ogbn-papers100M symmetrised, and of IGB-full).

G (tests/_wide.py) has E just above 2^32: `indices` is int64, 34.4 GB, built on the device; a weights (fp32) or types (int32) array adds
17.2 GB and is attached one at a time.  Three copies of the sweep's small graph lie in it so that position 2^31 and position 2^32 each
fall inside a hub row and the third copy lies wholly above 2^32.  Every call goes through the Python samplers (CSCGraph.edge_weights,
check_etype_sorted, max_in_degree and the capacity arithmetic run on the 4.3 G-element tensors) and is compared bit for bit with the numpy
restatements run on the small twin T, whose edge ids are moved through to_wide(); tests/test_wide_twin_cpu.py shows on the CPU that this
is the restatement of G, that the comparison raises on a 32-bit wrap, and that the references have no near tie and reach both sides of
both boundaries.  Every test asserts that what the device returned holds edge ids below 2^31, between 2^31 and 2^32 and above 2^32, and
ids on both sides of each boundary from the row that straddles it.

Measured on an MI355X.  torch.cuda.max_memory_allocated() of the file: 81,608,746,496 bytes (PEAK_BYTES) -- `indices`, one per-edge array
and the temporaries of its validation in CSCGraph.edge_weights / check_etype_sorted.  pytest --durations: test_one_call_per_kind[rel] 3.3 s,
test_wide_then_narrow[weighted_5_5] 2.4 s, test_one_call_per_kind[weighted_5_5] and [uniform_5_5] 1.3 s and 1.5 s of set-up -- each of these
allocates and fills a 34.4 GB or 17.2 GB array, which is what takes the time; every other test 0.2 s or less; the file in 11 s.  In the
same run of the whole suite the parent commit's end-to-end training tests take 4.5 .. 5.4 s each and its slowest test 77 s
(test_bench_gpu.py)."""
import numpy as np
import pytest

import _edge_batch_ref as EB
import _sampler_sweep as S
import _wide as W
from _pinsage_ref import threshold, traces

pytestmark = pytest.mark.gpu

PEAK_BYTES = 81_608_746_496    # torch.cuda.max_memory_allocated() of this file on an MI355X; a test skips only when less than this is free
CALLS = W.wide_calls(0)
ORDER = [n for n in CALLS if n != "rel"] + ["rel"]     # the typed graph is built once: last here, first in the test that follows


@pytest.fixture(scope="module")
def wide(hiplib, oracle):
    """get(kind, extra=None) -> (Layout, CSCGraph of G, seeds, reference of a call by name).  One G is alive at a time, with at most one
    per-edge array ('w' or 'etype') attached; everything is dropped at the end."""
    import torch
    state = dict(kind=None, extra=None, lay=None, g=None, refs={})
    layouts = {}

    def drop_extra():
        g = state["g"]
        if g is not None and state["extra"] is not None:
            g.edata.pop(state["extra"], None)
            g._weights, g._etypes = {}, {}
        state["extra"] = None
        torch.cuda.empty_cache()

    def drop():
        drop_extra()
        if state["g"] is not None:
            state["g"].close()
            state["g"].indices = None
        state.update(kind=None, lay=None, g=None)
        torch.cuda.empty_cache()

    def get(kind, extra=None):
        free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved()
        if free < PEAK_BYTES:
            pytest.skip(f"{free} bytes of device memory are free, the measured peak of this file is {PEAK_BYTES}")
        if state["kind"] != kind:
            drop()
            if kind not in layouts:
                layouts[kind] = W.Layout(W.small_graph(kind, W.GRAPH_SEED))
            lay = layouts[kind]
            state.update(kind=kind, lay=lay, g=lay.device_graph())
        lay, g = state["lay"], state["g"]
        if state["extra"] != extra:
            drop_extra()
            if extra is not None:
                g.edata[extra] = lay.device_weights() if extra == "w" else lay.device_etype()
            state["extra"] = extra
        seeds = lay.seeds(W.N_SEEDS)

        def ref(name):
            if name not in state["refs"]:
                k, call = CALLS[name]
                assert k == kind
                state["refs"][name] = W.widen(lay, S.reference(call._replace(n_seeds=len(seeds)), lay.twin(), oracle, seeds))
            return state["refs"][name]
        return lay, g, seeds, ref

    yield get
    drop()
    layouts.clear()
    torch.cuda.empty_cache()


def _extra(call):
    return {"weighted": "w", "rel": "etype"}.get(call.kind)


def _block_ids(blocks):
    return np.concatenate([b.edata["_ID"].cpu().numpy().reshape(-1) for b in blocks])


def _assert_covers(lay, e, where):
    """The device's own edge ids lie below 2^31, between the boundaries and above 2^32, and each straddling hub row gave ids on both sides."""
    e = e[e >= 0]
    assert lay.boundaries == (2**31, 2**32)
    assert np.any(e < 2**31) and np.any((e >= 2**31) & (e < 2**32)) and np.any(e >= 2**32), f"a range of positions was never taken: {where}"
    assert lay.covers(e), f"a straddling row gave ids on one side of its boundary only: {where}"


def _sample(call, g, seeds):
    import torch
    return S.make_sampler(call).sample(g, torch.from_numpy(seeds).cuda(), step=call.step)[2]


# ---------------------------------------------------------------------------------------------------- 1. one call per kind
@pytest.mark.parametrize("name", ORDER)
def test_one_call_per_kind(wide, name):
    kind, call = CALLS[name]
    lay, g, seeds, ref = wide(kind, _extra(call))
    assert g.num_edges == lay.E > 2**32 and g.max_in_degree == lay.max_in_degree
    call = call._replace(n_seeds=len(seeds))
    starts = lay.indptr[seeds]
    assert np.all(np.isin(lay.hubs, seeds)) and np.any(starts > 2**32) and np.any(starts < 2**31)
    for G in (0, 4):
        c = call._replace(G=G)
        blocks = _sample(c, g, seeds)
        S.check_call(c, blocks, ref(name), f"{name}, bucket_by_owner {G}")
        if c.edge_ids:
            _assert_covers(lay, _block_ids(blocks), f"{name}, bucket_by_owner {G}")
        else:    # a walk has no edge ids: its rows are read at the positions of its nodes, which lie in all three ranges
            for b in blocks:
                at = lay.indptr[b.src_nodes.cpu().numpy()]
                assert np.any(at < 2**31) and np.any((at > 2**31) & (at < 2**32)) and np.any(at > 2**32)


# ---------------------------------------------------------------------------------------------------- 2. wide, then narrow
@pytest.mark.parametrize("name", ORDER[::-1])
def test_wide_then_narrow(wide, name):
    """The call on G, then the same Call on a device copy of T: every tensor equal, the edge ids through to_wide()."""
    import torch
    kind, call = CALLS[name]
    lay, g, seeds, _ = wide(kind, _extra(call))
    call = call._replace(n_seeds=len(seeds), G=4 if call.kind in ("full", "labor") else 0)
    on_G = S.block_tensors(_sample(call, g, seeds))
    t = lay.device_twin()
    try:
        on_T = S.block_tensors(_sample(call, t, seeds))
    finally:
        t.close()
    assert len(on_G) == len(on_T)
    ids = []
    for (what, a), (_, b) in zip(on_G, on_T):
        if isinstance(a, torch.Tensor) and what.endswith("[_ID]"):
            ids.append(a.cpu().numpy().reshape(-1))
            same = isinstance(b, torch.Tensor) and a.shape == b.shape and np.array_equal(a.cpu().numpy(), lay.to_wide(b.cpu().numpy()))
        elif isinstance(a, torch.Tensor):
            same = isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
        else:
            same = a is None and b is None or (not isinstance(b, torch.Tensor) and a == b)
        assert same, f"{what} differs between G and T: {name}"
    if call.edge_ids:
        _assert_covers(lay, np.concatenate(ids), name)


# ---------------------------------------------------------------------------------------------------- 3. random_walk
@pytest.mark.parametrize("T,Wk,p", [(2, 10, 0.5), (16, 32, 0.0)])
def test_random_walk_traces(wide, T, Wk, p):
    import torch
    from COALA_GNN.sampler import random_walk
    lay, g, seeds, _ = wide("hub")
    tr = random_walk(g, torch.from_numpy(seeds).cuda(), T, restart_prob=p, num_walks=Wk, seed=6, step=2)
    assert tr.dtype == torch.int64 and tuple(tr.shape) == (len(seeds), Wk, T + 1)
    tr = tr.cpu().numpy()
    assert np.array_equal(tr, traces(lay.indptr_T, lay.indices_T, seeds, Wk, T, threshold(p), 6, 2))
    for ids in lay.live_ids:      # walks that started in each group, the hubs among them, and moved
        assert np.any((tr[:, :, 1] >= ids[0]) & (tr[:, :, 1] <= ids[-1]))
    assert np.all(np.isin(lay.hubs, tr[:, 0, 0])) and np.all(lay.live[tr[tr >= 0]])


# ---------------------------------------------------------------------------------------------------- 4. edge batches
def _edge_batch(g, eids, k, seed, step):
    import torch
    from COALA_GNN.sampler import edge_batch, edge_batch_wait
    b = edge_batch_wait(edge_batch(g, torch.from_numpy(eids).cuda(), k, seed=seed, step=step))
    n = len(eids)
    return dict(seed_nodes=b.seed_nodes.cpu().numpy(), pos_src=b.pos_src.cpu().numpy(), pos_dst=b.pos_dst.cpu().numpy(),
                neg_dst=b.neg_dst.cpu().numpy().reshape(n, k), n_bad=0)


@pytest.mark.parametrize("k", [0, 5, 64])
def test_edge_batch(wide, k):
    import torch
    from COALA_GNN.sampler import edge_batch, edge_batch_wait
    lay, g, _, _ = wide("hub")
    eids = lay.edge_batch_eids(rng_seed=k)
    assert np.array_equal(eids[:6], [2**31 - 1, 2**31, 2**31 + 1, 2**32 - 1, 2**32, 2**32 + 1]) and eids[12] == lay.E - 1
    assert (~lay.is_live(eids)).sum() == 3 and np.any(eids[16:] > 2**32) and np.any(eids[16:] < 2**31)
    want = lay.edge_batch_ref(eids, k, seed=11, step=3)
    got = _edge_batch(g, eids, k, seed=11, step=3)
    W.same_edge_batch(got, want)
    # the endpoints are those of the wide positions: the row of B - 1, B and B + 1 is the straddling hub
    dst = got["seed_nodes"][got["pos_dst"]]
    assert np.array_equal(dst[:6], np.repeat(lay.hubs[:2], 3)) and np.array_equal(got["seed_nodes"][got["pos_src"][:6]], lay.indices_at(eids[:6]))
    bad = eids.copy()
    bad[[3, 40]] = [-1, lay.E]
    assert lay.edge_batch_ref(bad, k, seed=2, step=0)["n_bad"] == 2
    with pytest.raises(IndexError, match=f"2 of the {len(bad)} seed edges"):
        edge_batch_wait(edge_batch(g, torch.from_numpy(bad).cuda(), k, seed=2, step=0))
    W.same_edge_batch(_edge_batch(g, eids, k, seed=11, step=4), lay.edge_batch_ref(eids, k, seed=11, step=4))     # the handle stays usable


# ---------------------------------------------------------------------------------------------------- 5. exclusion
def _check_excluded(got, plain, excluded):
    """test_edge_exclude_gpu.py's comparison: the excluded block against _edge_batch_ref applied to the plain one -> the ids removed."""
    t = lambda x: None if x is None else x.cpu().numpy()
    assert np.array_equal(t(got.src_nodes), t(plain.src_nodes)) and got.num_dst == plain.num_dst
    eid = t(plain.edata["_ID"])
    if plain.nbr is not None:
        want_n, want_e = EB.exclude_fixed(t(plain.nbr), eid, excluded)
        assert got.nbr.dtype == plain.nbr.dtype and np.array_equal(t(got.nbr), want_n) and np.array_equal(t(got.edata["_ID"]), want_e)
    else:
        wp, wi, we = EB.exclude_csr(t(plain.indptr), t(plain.indices), eid, excluded)
        assert got.nbr is None and np.array_equal(t(got.indptr), wp) and np.array_equal(t(got.indices), wi) and np.array_equal(t(got.edata["_ID"]), we)
    assert not np.isin(t(got.edata["_ID"]), excluded).any()
    return np.intersect1d(eid[eid >= 0], excluded)


def test_wrapper_excludes_wide_seed_edges(wide):
    import torch
    from COALA_GNN.sampler import EdgePredictionSampler, NeighborSampler, UniformNegativeSampler
    lay, g, _, _ = wide("hub")
    ip = lay.indptr
    deg = np.diff(ip)
    rows = np.concatenate([ids[(deg[ids] >= 1) & (deg[ids] <= 5)][:12] for ids in lay.live_ids])      # rows the first layer (fan-out 5) takes whole
    eids = np.concatenate([np.arange(ip[v], ip[v + 1]) for v in rows] + [lay.edge_batch_eids(rng_seed=9, n_random=60)])
    eids = eids[lay.is_live(eids)].astype(np.int64)
    wrapped = EdgePredictionSampler(NeighborSampler([3, 5], seed=4, edge_ids=True), exclude="self", negative_sampler=UniformNegativeSampler(2))
    input_nodes, batch, blocks = wrapped.sample(g, torch.from_numpy(eids).cuda(), step=6)
    want = lay.edge_batch_ref(eids, 2, seed=4, step=6)
    assert np.array_equal(batch.seed_nodes.cpu().numpy(), want["seed_nodes"]) and np.array_equal(batch.pos_dst.cpu().numpy(), want["pos_dst"])
    assert np.array_equal(batch.pos_src.cpu().numpy(), want["pos_src"]) and np.array_equal(batch.neg_dst.cpu().numpy(), want["neg_dst"].reshape(-1))
    p_in, _, p_blocks = NeighborSampler([3, 5], seed=4, edge_ids=True).sample(g, batch.seed_nodes, step=6)
    assert torch.equal(input_nodes, p_in) and len(blocks) == len(p_blocks) == 2
    excluded = np.unique(eids)
    removed = np.concatenate([_check_excluded(got, plain, excluded) for got, plain in zip(blocks, p_blocks)])
    assert np.any(removed > 2**32) and np.any((removed > 2**31) & (removed < 2**32)) and np.any(removed < 2**31), "no wide seed edge was in a block"
    _assert_covers(lay, _block_ids(p_blocks), "the plain sample of the wrapper's seed nodes")


@pytest.mark.parametrize("fanouts", [[32], [-1]])
def test_exclude_edges_with_wide_ids(wide, fanouts):
    import torch
    from COALA_GNN.sampler import NeighborSampler
    lay, g, seeds, _ = wide("hub")
    block = NeighborSampler(fanouts, seed=4, edge_ids=True).sample(g, torch.from_numpy(seeds).cuda(), step=2)[2][0]
    eid = block.edata["_ID"].cpu().numpy().reshape(-1)
    present = np.unique(eid[eid >= 0])
    _assert_covers(lay, present, f"fan-outs {fanouts}")
    rng = np.random.default_rng(5)
    foreign = np.array([5, 2**31 + 2**20, 2**32 + 2**16, lay.E - 1], dtype=np.int64)        # filler positions: in no block
    assert not lay.is_live(foreign).any()
    near = np.array([b + d for b in lay.boundaries for d in range(-40, 40)])                # around both boundaries, inside the hub rows
    ex = np.unique(np.concatenate([rng.choice(present, len(present) // 2, replace=False), present[present > 2**32][::2], near, foreign]))
    ex_t = torch.from_numpy(ex).cuda()
    removed = _check_excluded(block.exclude_edges(ex_t), block, ex)
    _check_excluded(block.exclude_edges_torch(ex_t), block, ex)
    assert np.any(removed > 2**32) and np.any((removed > 2**31) & (removed < 2**32)) and np.any(removed < 2**31)
