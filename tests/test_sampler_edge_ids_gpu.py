"""GPU tests of the edge ids of sampled blocks (NeighborSampler(edge_ids=True), coala_sampler_sample_layers_edge_ids): exact, no
tolerance.

block.edata['_ID'] holds, for every neighbour slot, the position of its edge in the graph's CSC `indices` array.  Checked as
properties on a multigraph (repeated edges, self-loops, degree 0, degree <= fan-out, a row above the weighted sampler's hub degree
of 4096), against CPU references (tests/_edge_id_ref.py), and at the C ABI with sentinel-filled buffers.  Asking for the ids must
not change the sample: the same (seed, step) gives the same blocks bit for bit with and without them."""
import ctypes as C

import numpy as np
import pytest

from _edge_id_ref import full_ids, uniform_ids, weighted_ids
from _util import csc_from_columns, edge_case_graph

pytestmark = pytest.mark.gpu

TIE = 1e-12     # test_sampler_weighted_gpu.py: rows whose f-th and (f+1)-th fp64 keys are this close may resolve either way
HUB = 5000      # in-degree of the hub row: above kHubDegree = 4096, so a weighted layer runs it through weighted_select_hub
FANOUTS = [[5, 5], [15, -1], [-1, -1], [32, 1]]


def _to_gpu(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.fixture(scope="module")
def multigraph(hiplib):
    import torch
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, special = edge_case_graph([1, 5, 15, 32], n_plain=3000, hub_degree=HUB, seed=11)
    rng = np.random.default_rng(4)
    w = (1.0 - rng.random(len(ix))).astype(np.float32)
    w[rng.random(len(ix)) < 0.2] = 0
    plain = np.setdiff1d(np.arange(len(ip) - 1), special)
    seeds = np.concatenate([special, rng.choice(plain, 300, replace=False)]).astype(np.int64)
    rng.shuffle(seeds)
    deg = np.diff(ip)
    assert deg[seeds].max() == HUB and (deg[seeds] == 0).any() and len(ix) // 4097 >= 1
    d_ip, d_ix, d_w = _to_gpu(torch, ip, ix, w)
    g = NeighborSampler([1]).make_graph(d_ip, d_ix, edata={"w": d_w})
    yield ip, ix, w, seeds, g
    g.close()


def _check_block(b, ip, ix, w, weighted, where):
    """The published properties of one block's ids.  -> (dst ids, eid) as numpy"""
    dst = b.dstdata["_ID"].cpu().numpy()
    src = b.src_nodes.cpu().numpy()
    eid = b.edata["_ID"].cpu().numpy()
    assert eid.dtype == np.int64
    if b.nbr is None:                                     # full layer: every in-edge, in order
        assert eid.shape == tuple(b.indices.shape), where
        assert np.array_equal(eid, full_ids(ip, dst)), f"a full row's ids are not arange(indptr[v], indptr[v + 1]): {where}"
        assert np.array_equal(np.diff(b.indptr.cpu().numpy()), ip[dst + 1] - ip[dst]), where
        assert np.array_equal(ix[eid], src[b.indices.cpu().numpy()]), f"indices[eid] != src_nodes[indices]: {where}"
        return dst, eid
    nbr = b.nbr.cpu().numpy()
    assert eid.shape == nbr.shape, where
    valid = nbr >= 0
    assert np.array_equal(eid == -1, ~valid) and np.all(eid >= -1), f"eid == -1 <=> nbr == -1 fails: {where}"
    lo, hi = ip[dst][:, None], ip[dst + 1][:, None]
    assert np.all(((eid >= lo) & (eid < hi))[valid]), f"an id outside its destination's column: {where}"
    assert np.array_equal(ix[eid[valid]], src[nbr[valid]]), f"indices[eid] != src_nodes[nbr]: {where}"
    srt = np.sort(eid, axis=1)
    assert not np.any((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)), f"an edge twice in one row: {where}"
    if weighted:
        assert np.all(w[eid[valid]] > 0), f"an edge of weight 0 was sampled: {where}"
    return dst, eid


@pytest.mark.parametrize("G", [0, 4])
@pytest.mark.parametrize("fanouts", FANOUTS)
@pytest.mark.parametrize("weighted", [False, True])
def test_edge_ids_properties_and_unchanged_sample(multigraph, weighted, fanouts, G):
    import torch
    from COALA_GNN.sampler import EID, NeighborSampler
    assert EID == "_ID"
    ip, ix, w, seeds, g = multigraph
    prob = "w" if weighted else None
    d_seeds = torch.from_numpy(seeds).cuda()
    d_w = g.edata["w"]
    for seed, step in ((0, 0), (9, 2**64 - 1)):
        on = NeighborSampler(fanouts, seed=seed, bucket_by_owner=G, prob=prob, edge_ids=True).sample(g, d_seeds, step=step)[2]
        off = NeighborSampler(fanouts, seed=seed, bucket_by_owner=G, prob=prob).sample(g, d_seeds, step=step)[2]
        rev = list(reversed(fanouts))
        saw_hub = False
        for i, (a, b) in enumerate(zip(on, off)):
            where = f"block {i} of {fanouts}, weighted={weighted}, G={G}, step {step}"
            assert b.edata == {} and len(b.edata) == 0, "edge_ids=False must give an empty edata"
            assert torch.equal(a.src_nodes, b.src_nodes) and a.num_dst == b.num_dst, f"source list changed: {where}"
            for x, y in ((a.nbr, b.nbr), (a.indptr, b.indptr), (a.indices, b.indices), (a.dst_in_src, b.dst_in_src)):
                assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), f"the sample changed: {where}"
            f = rev[len(rev) - 1 - i]
            dst, eid = _check_block(a, ip, ix, w, weighted and f != -1, where)
            saw_hub |= f != -1 and bool((np.diff(ip)[dst] > 4096).any())
            # edata['w'] = graph.edata['w'][eid], 0 on padding; made on first access and kept
            assert "w" in a.edata and list(dict.keys(a.edata)) == ["_ID"]
            got = a.edata["w"]
            d_eid = a.edata["_ID"]
            want = torch.where(d_eid >= 0, d_w[d_eid.clamp_min(0)], torch.zeros((), device="cuda"))
            assert got.shape == d_eid.shape and torch.equal(got, want), f"edata['w'] differs: {where}"
            assert a.edata["w"] is got and any(t is got for t in a.tensors()) and any(t is d_eid for t in a.tensors())
            with pytest.raises(KeyError):
                a.edata["absent"]
        if rev[0] != -1:
            assert saw_hub, "the hub row was not sampled by a fixed layer"


@pytest.mark.parametrize("fanouts", FANOUTS)
def test_weighted_and_full_ids_equal_the_reference(multigraph, fanouts):
    """Per layer, from the destination nodes the device itself produced: weighted rows equal _weighted_ref's chosen positions (a row
    within a near tie of its keys excepted, and there must be almost none), full rows equal arange."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, w, seeds, g = multigraph
    rev = list(reversed(fanouts))
    near = 0
    for seed, step in ((3, 1), (2**64 - 3, 77)):
        blocks = NeighborSampler(fanouts, seed=seed, prob="w", edge_ids=True).sample(g, torch.from_numpy(seeds).cuda(), step=step)[2]
        for l, f in enumerate(rev):
            b = blocks[len(rev) - 1 - l]
            dst, eid = b.dstdata["_ID"].cpu().numpy(), b.edata["_ID"].cpu().numpy()
            if f == -1:
                assert np.array_equal(eid, full_ids(ip, dst))
                continue
            want, margin = weighted_ids(ip, ix, w, dst, f, seed, step, l)
            bad = np.nonzero((eid != want).any(1))[0]
            assert np.all(margin[bad] < TIE), f"rows {bad[:8]} of layer {l} of {rev} differ from the reference beyond a near tie"
            near += len(bad)
    assert near <= 1


@pytest.mark.parametrize("fanouts", [[5, 5], [15, 10, 5], [32, 1], [15, -1]])
def test_uniform_ids_equal_the_twin(hiplib, oracle, fanouts):
    """A graph without repeated edges (self-loops and degree 0 included): the twin's sampled neighbour names its position."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    rng = np.random.default_rng(8)
    n = 20_000
    deg = np.minimum(rng.zipf(1.6, size=n), 300) - 1
    cols = [rng.choice(n, size=d, replace=False) for d in deg]
    for v in range(0, n, 50):                              # self-loops
        if len(cols[v]) and v not in cols[v]:
            cols[v][0] = v
    ip, ix = csc_from_columns(cols)
    d_ip, d_ix = _to_gpu(torch, ip, ix)
    g = NeighborSampler([1]).make_graph(d_ip, d_ix)
    seeds = rng.permutation(n)[:700].astype(np.int64)
    rev = list(reversed(fanouts))
    for G in (0, 4):
        for seed, step in ((1, 0), (2**64 - 9, 2**63)):
            blocks = NeighborSampler(fanouts, seed=seed, bucket_by_owner=G, edge_ids=True).sample(g, torch.from_numpy(seeds).cuda(), step=step)[2]
            for l, f in enumerate(rev):
                b = blocks[len(rev) - 1 - l]
                dst, eid = b.dstdata["_ID"].cpu().numpy(), b.edata["_ID"].cpu().numpy()
                want = full_ids(ip, dst) if f == -1 else uniform_ids(oracle, ip, ix, dst, f, seed, step, l)
                assert np.array_equal(eid, want), f"layer {l} of {rev}, G={G}, step {step}"
    g.close()


GUARD = 67
MARK = -77


def _edge_id_call(L, g, seeds, fanouts, specs, weights=None, want=None):
    """coala_sampler_sample_layers_edge_ids with sentinel-filled, guard-padded buffers; specs[l] = (src_cap, edge_cap, dst_cap);
    want[l] false: a NULL entry for that layer.  -> (rc, [(src, nbr, ind, eid)], n_src, n_edges)"""
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    bufs, lay, ptrs = [], [], []
    for l, ((src_cap, edge_cap, dst_cap), f) in enumerate(zip(specs, fanouts)):
        src = torch.full((src_cap + GUARD,), MARK, dtype=torch.int64, device="cuda")
        nbr = torch.full((edge_cap + GUARD,), MARK, dtype=torch.int32, device="cuda")
        ind = torch.full((dst_cap + 1 + GUARD,), MARK, dtype=torch.int64, device="cuda") if f == -1 else None
        eid = torch.full((edge_cap + GUARD,), MARK, dtype=torch.int64, device="cuda") if want is None or want[l] else None
        bufs.append((src, nbr, ind, eid))
        lay.append(_capi.SamplerLayer(src.data_ptr(), nbr.data_ptr(), ind.data_ptr() if ind is not None else None, src_cap, edge_cap))
        ptrs.append(eid.data_ptr() if eid is not None else None)
    n = len(fanouts)
    n_src, n_edges = (C.c_int64 * n)(), (C.c_int64 * n)()
    rc = L.coala_sampler_sample_layers_edge_ids(g._h, seeds.data_ptr(), seeds.numel(), (C.c_int32 * n)(*fanouts), n, 5, 2,
                                                (_capi.SamplerLayer * n)(*lay), weights.data_ptr() if weights is not None else None,
                                                (C.c_void_p * n)(*ptrs), n_src, n_edges, None, None, current_stream())
    torch.cuda.synchronize()
    return rc, bufs, list(n_src), list(n_edges)


def test_edge_ids_at_the_abi_guards_and_refusal(multigraph):
    """Nothing is written behind the used part of an output; a NULL entry is skipped; a refused full layer leaves its edge_ids_out
    untouched, and so do the layers behind it."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    ip, ix, w, seeds, g = multigraph
    s = seeds[:200]
    d_s = torch.from_numpy(s).cuda()
    E = int((ip[s + 1] - ip[s]).sum())
    n_items = len(s) + E
    for weights in (None, g.edge_weights("w")):
        # fixed then full, roomy buffers: the used regions hold ids, everything behind them the sentinel
        specs = [(len(s) * 6 + 50, len(s) * 5 + 50, len(s)), (500_000, 400_000, len(s) * 6 + 50)]
        rc, bufs, n_src, n_edges = _edge_id_call(L, g, d_s, [5, -1], specs, weights)
        assert rc == 0, _capi.last_error()
        assert n_edges[0] == len(s) * 5 and 0 < n_edges[1] <= 400_000
        for (src, nbr, ind, eid), used in zip(bufs, n_edges):
            e, nb = eid.cpu().numpy(), nbr.cpu().numpy()
            assert np.all(e[used:] == MARK) and np.all(nb[used:] == MARK), "write behind the used region"
            assert np.array_equal(e[:used] == -1, nb[:used] == -1) and np.all(e[:used] >= -1) and np.all(e[:used] < len(ix))
        dst1 = bufs[0][0][: n_src[0]].cpu().numpy()
        assert np.array_equal(bufs[1][3][: n_edges[1]].cpu().numpy(), full_ids(ip, dst1))
        # the same call, ids wanted for the second layer only: same sample, first layer's ids skipped
        rc, bufs2, n_src2, n_edges2 = _edge_id_call(L, g, d_s, [5, -1], specs, weights, want=[False, True])
        assert rc == 0 and n_src2 == n_src and n_edges2 == n_edges and bufs2[0][3] is None
        assert torch.equal(bufs2[0][1], bufs[0][1]) and torch.equal(bufs2[1][3], bufs[1][3]) and torch.equal(bufs2[1][0], bufs[1][0])
        # a full layer one edge short of room: refused; its ids and those of the fixed layer behind it stay untouched
        rc, bufs, _, _ = _edge_id_call(L, g, d_s, [-1, 3], [(n_items, E - 1, len(s)), (n_items * 4, n_items * 3, n_items)], weights)
        assert rc == _capi.EINVAL and f"layer 0 holds {n_items} items" in _capi.last_error()
        for src, nbr, ind, eid in bufs:
            assert torch.all(eid == MARK), "a refused layer wrote edge ids"
    # NULL array: the call without ids
    from COALA_GNN_Pybind import current_stream
    src = torch.empty(len(s) * 6, dtype=torch.int64, device="cuda")
    nbr = torch.empty(len(s) * 5, dtype=torch.int32, device="cuda")
    lay = (_capi.SamplerLayer * 1)(_capi.SamplerLayer(src.data_ptr(), nbr.data_ptr(), None, len(s) * 6, len(s) * 5))
    n_src = (C.c_int64 * 1)()
    _capi.check(L.coala_sampler_sample_layers_edge_ids(g._h, d_s.data_ptr(), len(s), (C.c_int32 * 1)(5), 1, 5, 2, lay, None, None, n_src, None,
                                                       None, None, current_stream()))
    assert 0 < n_src[0] <= len(s) * 6
