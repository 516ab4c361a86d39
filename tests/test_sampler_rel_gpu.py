"""GPU tests of neighbour sampling with a fan-out per relation (COALA_GNN.sampler.RelNeighborSampler; rel_count_scan / rel_insert in
coala_sampler.hip).

The rule is exact integer arithmetic, so every output -- indptr, indices, source lists, edge ids, input and output nodes -- is compared
bit for bit with the numpy restatement of tests/_rel_fanout_ref.py (checked on its own in test_sampler_rel_cpu.py).  Every call uses at
most 512 seeds."""
import ctypes as C

import numpy as np
import pytest

from _full_ref import bucketed
from _rel_fanout_ref import expand_fanouts, reference_layers, typed_edge_case_graph

pytestmark = pytest.mark.gpu

GUARD = 67
HUB = 1_000_003
ITEM_LIMIT = 8192 * 1024


def _to_gpu(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _check_call(smp, g, ip, ix, et, seeds, step):
    """One sample of `smp` (unbucketed): every layer equal to the reference, bit for bit."""
    import torch
    input_nodes, out_nodes, blocks = smp.sample(g, torch.from_numpy(seeds).cuda(), step=step)
    rev = list(reversed(smp.rel_fanouts))
    ref = reference_layers(ip, ix, et, seeds, rev, smp.seed, step)
    n_dst = len(seeds)
    for l, (src_r, ind_r, loc_r, eid_r) in enumerate(ref):
        b = blocks[len(rev) - 1 - l]
        where = f"layer {l} of {rev}, {len(seeds)} seeds, seed {smp.seed}, step {step}"
        assert b.nbr is None and b.num_dst == n_dst, where
        assert b.indptr.dtype == torch.int64 and b.indices.dtype == torch.int32
        assert np.array_equal(b.indptr.cpu().numpy(), ind_r), f"indptr differs: {where}"
        assert np.array_equal(b.src_nodes.cpu().numpy(), src_r), f"source list differs: {where}"
        assert np.array_equal(b.indices.cpu().numpy(), loc_r), f"indices differ: {where}"
        if smp.edge_ids:
            assert b.edata["_ID"].dtype == torch.int64 and np.array_equal(b.edata["_ID"].cpu().numpy(), eid_r), f"edge ids differ: {where}"
            assert np.array_equal(b.edata[smp.etype].cpu().numpy(), et[eid_r]), where
        else:
            assert "_ID" not in b.edata
        n_dst = len(src_r)
    assert torch.equal(input_nodes, blocks[0].src_nodes) and np.array_equal(input_nodes.cpu().numpy(), ref[-1][0])
    assert torch.equal(out_nodes.cpu(), torch.from_numpy(seeds))
    return blocks


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.fixture(scope="module")
def graphs(hiplib):
    """powerlaw_csc / community_csc (200000, 30), untyped; typed(name, R) types them by source node and sorts them, once per R."""
    from COALA_GNN.sampler import RelNeighborSampler, sort_csc_by_etype
    from COALA_GNN.synthetic import community_csc, edge_types_by_source, powerlaw_csc
    raw = {name: make(200_000, 30, seed=1, device="cuda") for name, make in (("powerlaw", powerlaw_csc), ("community", community_csc))}
    made = {}

    def typed(name, R):
        if (name, R) not in made:
            d_ip, d_ix = raw[name]
            s_ix, s_et, perm = sort_csc_by_etype(d_ip, d_ix, edge_types_by_source(d_ix, R))
            assert bool((s_ix == d_ix[perm]).all())
            g = RelNeighborSampler.make_graph(d_ip, s_ix, edata={"etype": s_et})
            made[(name, R)] = (d_ip.cpu().numpy(), s_ix.cpu().numpy(), s_et.cpu().numpy(), g)
        return made[(name, R)]
    yield typed
    for _, _, _, g in made.values():
        g.close()


def _cycle(pattern, R):
    return [pattern[r % len(pattern)] for r in range(R)]


LISTS3 = [[[10, 3, 1]], [5, 5], [[32, 32, 32], [1, 0, -1]], [[-1, -1, -1], 10], [[2, 0, 4], 5, [0, 0, 7]]]
CASES = ([(3, f) for f in LISTS3] + [(1, [[10]]), (1, [5, 5]), (1, [[32], [-1]]), (1, [[2], 5, [7]])]
         + [(64, [_cycle([10, 3, 1], 64)]), (64, [2, 2]), (64, [_cycle([32, 0], 64), _cycle([1, 0, -1], 64)]), (64, [_cycle([-1], 64), 1]),
            (64, [_cycle([2, 0, 4], 64), 1, _cycle([0, 0, 7], 64)])])


@pytest.mark.parametrize("R,fanouts", CASES, ids=[f"R{R}-{i}" for i, (R, _) in enumerate(CASES)])
@pytest.mark.parametrize("name", ["powerlaw", "community"])
def test_rel_layers_exact(graphs, name, R, fanouts):
    from COALA_GNN.sampler import RelNeighborSampler
    ip, ix, et, g = graphs(name, R)
    full = any(-1 in f for f in expand_fanouts(fanouts, R))
    n_seeds = 64 if full or R == 64 else 512
    for seed, step in ((0, 0), (2**64 - 5, 2**64 - 1), (7, 5)):
        seeds = np.random.default_rng(seed % 1000 + step % 1000).permutation(len(ip) - 1)[:n_seeds].astype(np.int64)
        _check_call(RelNeighborSampler(fanouts, R, seed=seed), g, ip, ix, et, seeds, step)
    _check_call(RelNeighborSampler(fanouts, R, seed=3, edge_ids=False), g, ip, ix, et, seeds[: n_seeds // 3], 1)     # without edge ids


# ------------------------------------------------------------------------------------------------ 2. edge shapes
@pytest.fixture(scope="module")
def edge_graph(hiplib):
    """Three relations; for f in (1, 5, 32) rows whose relation-r segment has 0, f-1, f, f+1, 2f, 200 edges, rows lacking the first, a
    middle or the last relation, a row without an in-edge, self-loops, repeated neighbours, and a hub whose relation 1 has 1,000,003
    edges (above kHubDegree = 4096) beside 2 edges of relation 2."""
    import torch
    from COALA_GNN.sampler import RelNeighborSampler
    ip, ix, et, special = typed_edge_case_graph([1, 5, 32], 3, n_plain=3000, hub_degree=HUB, seed=7)
    rng = np.random.default_rng(2)
    plain = np.setdiff1d(np.arange(len(ip) - 1), special)
    seeds = np.concatenate([special, rng.choice(plain, 512 - len(special), replace=False)]).astype(np.int64)
    rng.shuffle(seeds)
    d_ip, d_ix, d_et = _to_gpu(torch, ip, ix, et)
    g = RelNeighborSampler.make_graph(d_ip, d_ix, edata={"etype": d_et})
    yield ip, ix, et, g, seeds
    g.close()


@pytest.mark.parametrize("fanouts", [[1], [5], [32], [[5, 1, 32], [32, 5, 1]], [[0, -1, 1]], [[0, 32, 1]], [[-1, 5, 0]], [[1, 0, -1], 5]])
def test_rel_on_edge_graph(edge_graph, fanouts):
    """The hub row is in every batch: [0, -1, 1] copies its 1,000,003-edge segment with the whole block, [0, 32, 1] runs Floyd on it."""
    from COALA_GNN.sampler import RelNeighborSampler
    ip, ix, et, g, seeds = edge_graph
    n = len(ip) - 1
    assert len(seeds) == 512 and (ip[seeds + 1] - ip[seeds] == 0).any() and (ip[seeds + 1] - ip[seeds] == HUB + 2).any()
    for step in (0, 1):
        _check_call(RelNeighborSampler(fanouts, 3, seed=len(fanouts)), g, ip, ix, et, seeds, step)
    if any(-1 in f for f in expand_fanouts(fanouts, 3)[1:]):   # the restatement's later layers take node ids of the graph only
        return
    # duplicate seeds (every row of a repeated node is the same row) and out-of-range seeds (empty rows; the ids stay in the list)
    odd = np.concatenate([seeds[:50], seeds[:50], [n + 5, seeds[3], n, 2**40], seeds[50:80]]).astype(np.int64)
    import torch
    smp = RelNeighborSampler(fanouts, 3, seed=1)
    _, _, blocks = smp.sample(g, torch.from_numpy(odd).cuda(), step=3)
    ref = reference_layers(ip, ix, et, odd, list(reversed(smp.rel_fanouts)), 1, 3)
    lp = blocks[-1].indptr.cpu().numpy()
    assert np.array_equal(lp, ref[0][1]) and np.array_equal(blocks[-1].edata["_ID"].cpu().numpy(), ref[0][3])
    assert np.array_equal(blocks[-1].src_nodes.cpu().numpy(), ref[0][0]) and np.array_equal(blocks[-1].indices.cpu().numpy(), ref[0][2])
    assert lp[101] == lp[100] and lp[103] == lp[102] and lp[104] == lp[103]
    assert np.array_equal(np.diff(lp)[:50], np.diff(lp)[50:100])


# ------------------------------------------------------------------------------------------------ 3. against the shipped samplers
@pytest.mark.parametrize("f", [1, 5, 32])
def test_one_relation_holds_neighbor_samplers_edges(graphs, f):
    """num_rels = 1: the sorted edge ids of every row are those of NeighborSampler([f], edge_ids=True) at the same seed and step."""
    import torch
    from COALA_GNN.sampler import NeighborSampler, RelNeighborSampler
    ip, ix, et, g = graphs("powerlaw", 1)
    seeds = torch.from_numpy(np.random.default_rng(f).permutation(len(ip) - 1)[:512]).cuda()
    for seed, step in ((4, 0), (2**64 - 5, 2**64 - 1)):
        _, _, (rb,) = RelNeighborSampler([f], 1, seed=seed).sample(g, seeds, step=step)
        _, _, (nb,) = NeighborSampler([f], seed=seed, edge_ids=True).sample(g, seeds, step=step)
        want = np.sort(nb.edata["_ID"].cpu().numpy(), 1)
        lp, eid = rb.indptr.cpu().numpy(), rb.edata["_ID"].cpu().numpy()
        got = np.full(want.shape, -1, dtype=np.int64)
        got[np.repeat(np.arange(512), np.diff(lp)), np.arange(len(eid)) - np.repeat(lp[:-1], np.diff(lp))] = eid
        assert np.array_equal(np.sort(got, 1), want)
        assert np.array_equal(np.sort(rb.src_nodes.cpu().numpy()), np.sort(nb.src_nodes.cpu().numpy()))


def test_all_minus_one_is_neighbor_samplers_full_list(graphs):
    import torch
    from COALA_GNN.sampler import NeighborSampler, RelNeighborSampler
    ip, ix, et, g = graphs("community", 3)
    seeds = torch.from_numpy(np.random.default_rng(0).permutation(len(ip) - 1)[:64]).cuda()
    for G in (0, 3):
        a = RelNeighborSampler([-1, [-1, -1, -1]], 3, seed=1, bucket_by_owner=G).sample(g, seeds, step=2)
        b = NeighborSampler([-1, -1], seed=1, bucket_by_owner=G, edge_ids=True).sample(g, seeds, step=2)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for x, y in zip(a[2], b[2]):
            assert torch.equal(x.src_nodes, y.src_nodes) and torch.equal(x.indptr, y.indptr) and torch.equal(x.indices, y.indices)
            assert torch.equal(x.edata["_ID"], y.edata["_ID"]) and torch.equal(x.dstdata["_ID"], y.dstdata["_ID"])
            assert (x.dst_in_src is None) == (y.dst_in_src is None) and (x.dst_in_src is None or torch.equal(x.dst_in_src, y.dst_in_src))


# ------------------------------------------------------------------------------------------------ 4. owner bucketing
@pytest.mark.parametrize("G", [1, 3, 8, 64])
@pytest.mark.parametrize("fanouts", [[[10, 3, 1], 5], [[1, 0, -1]]])
def test_rel_owner_bucketing(graphs, G, fanouts):
    import torch
    from COALA_GNN.sampler import RelNeighborSampler
    ip, ix, et, g = graphs("powerlaw", 3)
    smp = RelNeighborSampler(fanouts, 3, seed=3, bucket_by_owner=G)
    rev = list(reversed(smp.rel_fanouts))
    for step, n_seeds in ((0, 512), (1, 333)):
        seeds = np.random.default_rng(step).permutation(len(ip) - 1)[:n_seeds].astype(np.int64)
        ref = reference_layers(ip, ix, et, seeds, rev, 3, step)
        inp, _, blocks = smp.sample(g, torch.from_numpy(seeds).cuda(), step=step)
        src_r, ind_r, loc_r, eid_r = ref[-1]
        want, sizes, new_of_old = bucketed(src_r, G)
        dst = ref[-2][0] if len(rev) > 1 else seeds
        b0 = blocks[0]
        assert np.array_equal(inp.cpu().numpy(), want) and np.array_equal(b0.src_nodes.cpu().numpy(), want)
        assert b0.owner_counts.cpu().tolist() == b0.owner_counts_host == sizes.tolist()
        assert np.array_equal(b0.dst_in_src.cpu().numpy(), new_of_old[: len(dst)])
        assert np.array_equal(b0.indptr.cpu().numpy(), ind_r)
        assert np.array_equal(b0.indices.cpu().numpy(), new_of_old[loc_r])
        assert np.array_equal(b0.edata["_ID"].cpu().numpy(), eid_r)
        assert np.array_equal(b0.dstdata["_ID"].cpu().numpy(), dst)
        for l in range(len(rev) - 1):            # the layers behind the input layer are not bucketed
            b = blocks[len(rev) - 1 - l]
            assert b.dst_in_src is None and np.array_equal(b.src_nodes.cpu().numpy(), ref[l][0])
            assert np.array_equal(b.indices.cpu().numpy(), ref[l][2])


# ------------------------------------------------------------------------------------------------ 5. refusal
def _rel_call(L, g, d_et, seeds, rel_fanouts, specs):
    """coala_sampler_sample_layers_rel with guard-padded buffers; rel_fanouts in sampling order, specs[l] = (src_cap, edge_cap, dst_cap).
    -> (rc of the call or of the wait, buffers, n_src, n_edges)"""
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    bufs, lay = [], []
    for src_cap, edge_cap, dst_cap in specs:
        src = torch.full((src_cap + GUARD,), -77, dtype=torch.int64, device="cuda")
        nbr = torch.full((edge_cap + GUARD,), -77, dtype=torch.int32, device="cuda")
        ind = torch.full((dst_cap + 1 + GUARD,), -77, dtype=torch.int64, device="cuda")
        eid = torch.full((edge_cap + GUARD,), -77, dtype=torch.int64, device="cuda")
        bufs.append((src, nbr, ind, eid))
        lay.append(_capi.SamplerLayer(src.data_ptr(), nbr.data_ptr(), ind.data_ptr(), src_cap, edge_cap))
    n, R = len(rel_fanouts), len(rel_fanouts[0])
    n_src, n_edges = (C.c_int64 * n)(), (C.c_int64 * n)()
    eid_p = (C.c_void_p * n)(*[b[3].data_ptr() for b in bufs])
    ticket = C.c_int64(-1)
    rc = L.coala_sampler_sample_layers_rel(g._h, seeds.data_ptr(), seeds.numel(), (C.c_int32 * (n * R))(*[f for fan in rel_fanouts for f in fan]),
                                           R, n, 0, 0, (_capi.SamplerLayer * n)(*lay), d_et.data_ptr(), eid_p, None, None, None,
                                           C.byref(ticket), current_stream())
    if rc == 0:
        rc = L.coala_sampler_wait_layers(g._h, ticket.value, n_src, n_edges, None)
    torch.cuda.synchronize()
    for (src_cap, edge_cap, dst_cap), (src, nbr, ind, eid) in zip(specs, bufs):
        assert torch.all(src[src_cap:] == -77) and torch.all(nbr[edge_cap:] == -77) and torch.all(eid[edge_cap:] == -77), "write past a capacity"
        assert torch.all(ind[dst_cap + 1:] == -77), "write past indptr_local"
    return rc, bufs, list(n_src), list(n_edges)


def test_rel_refusal_names_the_layer_and_the_handle_stays_usable(graphs, edge_graph):
    import torch
    from COALA_GNN.sampler import RelNeighborSampler
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    # a -1 relation over the hub, repeated until n_dst + E passes the item limit: refused on the device, whatever the capacities
    ip, ix, et, g, seeds = edge_graph
    hub = len(ip) - 2
    assert ip[hub + 1] - ip[hub] == HUB + 2
    batch = np.concatenate([seeds[:20], np.full(9, hub)]).astype(np.int64)
    E = int(reference_layers(ip, ix, et, batch[:21], [[0, -1, 1]], 0, 0)[0][1][-2]) + 9 * (HUB + 1)
    assert len(batch) + E > ITEM_LIMIT
    d_et = g.edge_types("etype", 3)
    rc, _, _, _ = _rel_call(L, g, d_et, torch.from_numpy(batch).cuda(), [[0, -1, 1]], [(20_000, 20_000, len(batch))])
    assert rc == _capi.EINVAL and f"layer 0 holds {len(batch) + E} items" in _capi.last_error() and "over the limit" in _capi.last_error()
    with pytest.raises(RuntimeError, match=f"layer 0 holds {len(batch) + E} items"):     # sample_end is this wait
        RelNeighborSampler([[0, -1, 1]], 3).sample(g, torch.from_numpy(batch).cuda(), step=0)
    _check_call(RelNeighborSampler([[0, -1, 1], 5], 3, seed=1), g, ip, ix, et, seeds[:40], 2)      # the handle stays exact
    # capacities one short, then exactly enough, on the power-law graph
    ip, ix, et, g = graphs("powerlaw", 3)
    d_et = g.edge_types("etype", 3)
    s = np.random.default_rng(9).permutation(len(ip) - 1)[:100].astype(np.int64)
    d_s = torch.from_numpy(s).cuda()
    fans = [[5, 0, 2], [1, -1, 3]]
    (src0, ind0, loc0, eid0), (src1, ind1, loc1, eid1) = reference_layers(ip, ix, et, s, fans, 0, 0)
    E0, E1 = len(loc0), len(loc1)
    items0, items1 = 100 + E0, len(src0) + E1
    rc, _, _, _ = _rel_call(L, g, d_et, d_s, fans[:1], [(items0, E0 - 1, 100)])
    assert rc == _capi.EINVAL and f"layer 0 holds {items0} items" in _capi.last_error() and "edge_cap" in _capi.last_error()
    rc, _, _, _ = _rel_call(L, g, d_et, d_s, fans[:1], [(items0 - 1, E0, 100)])
    assert rc == _capi.EINVAL and f"layer 0 holds {items0} items" in _capi.last_error() and "src_cap" in _capi.last_error()
    rc, bufs, n_src, _ = _rel_call(L, g, d_et, d_s, fans, [(items0, E0, 100), (items1 - 1, E1, items0)])
    assert rc == _capi.EINVAL and f"layer 1 holds {items1} items" in _capi.last_error() and n_src[0] == len(src0)
    assert np.array_equal(bufs[0][0][: len(src0)].cpu().numpy(), src0), "the layer in front of the refused one is complete"
    rc, (b0, b1), n_src, n_edges = _rel_call(L, g, d_et, d_s, fans, [(items0, E0, 100), (items1, E1, items0)])
    assert rc == 0, _capi.last_error()
    assert n_src == [len(src0), len(src1)] and n_edges == [E0, E1]
    for (src, nbr, ind, eid), (src_r, ind_r, loc_r, eid_r), n_dst in ((b0, (src0, ind0, loc0, eid0), 100), (b1, (src1, ind1, loc1, eid1), len(src0))):
        assert np.array_equal(src[: len(src_r)].cpu().numpy(), src_r) and np.array_equal(ind[: n_dst + 1].cpu().numpy(), ind_r)
        assert np.array_equal(nbr[: len(loc_r)].cpu().numpy(), loc_r) and np.array_equal(eid[: len(eid_r)].cpu().numpy(), eid_r)
    _check_call(RelNeighborSampler([5, [5, 0, 2]], 3, seed=1), g, ip, ix, et, s[:30], 2)


# ------------------------------------------------------------------------------------------------ 6. argument errors
def test_rel_argument_errors(graphs):
    """Every COALA_EINVAL case of coala_sampler_sample_layers_rel on a live handle, before any launch; and the Python layer's checks of
    the graph."""
    import torch
    from COALA_GNN.sampler import RelNeighborSampler
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    ip, ix, et, g = graphs("powerlaw", 3)
    d_et = g.edge_types("etype", 3)
    seeds = torch.arange(10, device="cuda")
    bufs = [torch.empty(4096, dtype=dt, device="cuda") for dt in (torch.int64, torch.int32, torch.int64)]
    lay = (_capi.SamplerLayer * 1)(_capi.SamplerLayer(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), 4096, 4096))

    def call(fan, R, etype=d_et.data_ptr(), layers=lay):
        return L.coala_sampler_sample_layers_rel(g._h, seeds.data_ptr(), 10, (C.c_int32 * len(fan))(*fan), R, 1, 0, 0, layers, etype, None, None,
                                                 None, None, None, None)
    for R in (0, 65):
        assert call([5] * 65, R) == _capi.EINVAL and "num_rels must be 1..64" in _capi.last_error()
    for bad in (-2, 33):
        assert call([5, bad, 5], 3) == _capi.EINVAL and f"fan-out {bad}" in _capi.last_error()
    assert call([0, 0, 0], 3) == _capi.EINVAL and "every relation has fan-out 0" in _capi.last_error()
    assert call([5, 5, 5], 3, etype=None) == _capi.EINVAL and "null etype" in _capi.last_error()
    nolay = (_capi.SamplerLayer * 1)(_capi.SamplerLayer(bufs[0].data_ptr(), bufs[1].data_ptr(), None, 4096, 4096))
    assert call([5, 5, 5], 3, layers=nolay) == _capi.EINVAL and "null buffer" in _capi.last_error()
    assert call([5, 0, -1], 3) == 0, _capi.last_error()
    torch.cuda.synchronize()
    # the graph checks of the Python layer: before any launch, naming the cure
    d_ip, d_ix = _to_gpu(torch, ip, ix)
    flipped = torch.from_numpy(et).cuda().flip(0).contiguous()
    bad = RelNeighborSampler.make_graph(d_ip, d_ix, edata={"etype": flipped, "wide": torch.from_numpy(et).cuda() + 1})
    smp = RelNeighborSampler([5], 3)
    with pytest.raises(ValueError, match="sort_csc_by_etype"):
        smp.sample(bad, seeds)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        RelNeighborSampler([5], 3, etype="wide").sample(bad, seeds)
    with pytest.raises(KeyError, match="nope"):
        RelNeighborSampler([5], 3, etype="nope").sample(bad, seeds)
    assert smp.step == 0, "a refused graph does not advance the step"
    bad.edata["etype"] = torch.from_numpy(et).cuda()          # replaced: checked again, and now accepted
    _check_call(smp, bad, ip, ix, et, np.arange(10, dtype=np.int64), 0)
    assert "etype" in bad._etypes
    bad.close()
    assert not bad._etypes, "close() frees the cached types"
