"""GPU tests of full layers (fan-out -1, every in-edge) in the native sampler and of the ragged (CSR) mean aggregation.

A full layer draws no random numbers, so every output is compared bit for bit with the numpy restatement of tests/_full_ref.py
(itself pinned to the CPU twin in test_sampler_full_cpu.py); fixed layers of a mixed list are compared with the twin at their layer
index.  Aggregation bounds are the fp32 rounding bounds of test_block_ops_gpu.py (u = 2^-24): forward |got - ref| <= (cnt + 2) u
sum|x_j| / cnt, backward |got - ref| <= gamma(k + 1) sum|g_d / cnt_d| over the k contributions of a source row."""
import ctypes as C

import numpy as np
import pytest

from _full_ref import bucketed, full_layer, reference_layers
from _util import csc_from_columns, edge_case_graph

pytestmark = pytest.mark.gpu

LIMIT = 8192 * 1024
U = 2.0 ** -24
SENTINEL = np.float32(-7.25e33)
GUARD = 67


def _to_gpu(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _check_call(oracle, smp, g, ip, ix, seeds, step):
    """One sample of `smp`: every layer equal to the reference, bit for bit."""
    import torch
    input_nodes, _, blocks = smp.sample(g, torch.from_numpy(seeds).cuda(), step=step)
    rev = list(reversed(smp.fanouts))
    ref = reference_layers(oracle, ip, ix, seeds, rev, smp.seed, step)
    n_dst = len(seeds)
    for l, (src_r, ind_r, loc_r) in enumerate(ref):
        b = blocks[len(rev) - 1 - l]
        where = f"layer {l} of {rev}, {len(seeds)} seeds, step {step}"
        assert b.num_dst == n_dst, where
        assert np.array_equal(b.src_nodes.cpu().numpy(), src_r), f"source list differs: {where}"
        if ind_r is None:
            assert b.indptr is None and np.array_equal(b.nbr.cpu().numpy(), loc_r), f"fixed block differs: {where}"
        else:
            assert b.nbr is None, where
            assert b.indptr.dtype == torch.int64 and b.indices.dtype == torch.int32
            assert np.array_equal(b.indptr.cpu().numpy(), ind_r), f"indptr_local differs: {where}"
            assert np.array_equal(b.indices.cpu().numpy(), loc_r), f"nbr_local differs: {where}"
        n_dst = len(src_r)
    assert torch.equal(input_nodes, blocks[0].src_nodes)
    return blocks


# ------------------------------------------------------------------------------------------------ 1. exactness
@pytest.fixture(scope="module")
def graphs():
    import torch
    from COALA_GNN.synthetic import powerlaw_csc
    ip, ix, special = edge_case_graph([1, 5, 32], n_plain=3000, hub_degree=1_000_003, seed=7)
    rng = np.random.default_rng(2)
    plain = np.setdiff1d(np.arange(len(ip) - 1), special)
    hub_seeds = np.concatenate([special, rng.choice(plain, 200, replace=False)]).astype(np.int64)
    rng.shuffle(hub_seeds)
    d_ip, d_ix = powerlaw_csc(200_000, 10.0, seed=4, device="cuda")
    pl = (d_ip.cpu().numpy(), d_ix.cpu().numpy(), d_ip, d_ix)
    pl_seeds = rng.permutation(200_000)[:256].astype(np.int64)
    return {"hub": (ip, ix) + tuple(_to_gpu(torch, ip, ix)) + (hub_seeds,), "powerlaw": pl + (pl_seeds,)}


@pytest.mark.parametrize("fanouts", [[-1], [-1, -1], [5, -1], [-1, 5], [32, -1, 1]])
@pytest.mark.parametrize("name", ["hub", "powerlaw"])
def test_full_layers_exact(hiplib, oracle, graphs, name, fanouts):
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, d_ip, d_ix, seeds = graphs[name]
    g = NeighborSampler([1]).make_graph(d_ip, d_ix)
    if name == "hub":
        assert g.max_in_degree == 1_000_003 and (seeds == len(ip) - 2).any()
    for seed, step, k in ((0, 0, len(seeds)), (7, 2**64 - 1, len(seeds) // 3), (2**64 - 5, 2**64 - 2, 1)):
        _check_call(oracle, NeighborSampler(fanouts, seed=seed), g, ip, ix, seeds[:k], step)
    g.close()


# ------------------------------------------------------------------------------------------------ 2./3. fixed-path equivalence, bucketing
@pytest.fixture(scope="module")
def small_degree_graph():
    import torch
    rng = np.random.default_rng(5)
    n = 60_000
    ip, ix = csc_from_columns([rng.integers(0, n, size=rng.integers(0, 9)) for _ in range(n)])
    return (ip, ix) + tuple(_to_gpu(torch, ip, ix))


@pytest.mark.parametrize("G", [0, 1, 3, 8, 64])
def test_full_layer_equals_fixed_layer_when_degrees_fit(hiplib, small_degree_graph, G):
    """Every degree <= 8: layer -1 must be layer 8 with the -1 padding removed, with and without owner bucketing; the bucketed input
    layer is checked against the restatement (stable partition, bucket sizes, dst_in_src, re-indexed nbr_local)."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, d_ip, d_ix = small_degree_graph
    assert (ip[1:] - ip[:-1]).max() == 8
    g = NeighborSampler([1]).make_graph(d_ip, d_ix)
    seeds = np.random.default_rng(G).permutation(len(ip) - 1)[:3000].astype(np.int64)
    for full, fixed in (([-1], [8]), ([-1, -1], [8, 8])):
        _, _, bf = NeighborSampler(full, seed=1, bucket_by_owner=G).sample(g, torch.from_numpy(seeds).cuda(), step=3)
        _, _, bd = NeighborSampler(fixed, seed=1, bucket_by_owner=G).sample(g, torch.from_numpy(seeds).cuda(), step=3)
        for a, b in zip(bf, bd):
            assert torch.equal(a.src_nodes, b.src_nodes) and a.num_dst == b.num_dst
            dense = b.nbr.cpu().numpy()
            valid = dense >= 0
            assert np.array_equal(np.diff(a.indptr.cpu().numpy()), valid.sum(1))
            assert np.array_equal(a.indices.cpu().numpy(), dense[valid])
            if b.dst_in_src is not None:
                assert torch.equal(a.dst_in_src, b.dst_in_src) and torch.equal(a.owner_counts, b.owner_counts)
        if G:   # the bucketed full input layer against the restatement
            dst = bf[1].src_nodes.cpu().numpy() if len(full) == 2 else seeds
            src, ind, loc = full_layer(ip, ix, dst)
            want, sizes, new_of_old = bucketed(src, G)
            b0 = bf[0]
            assert np.array_equal(b0.src_nodes.cpu().numpy(), want)
            assert b0.owner_counts.cpu().tolist() == b0.owner_counts_host == sizes.tolist()
            assert np.array_equal(b0.dst_in_src.cpu().numpy(), new_of_old[: len(dst)])
            assert np.array_equal(b0.indptr.cpu().numpy(), ind)
            assert np.array_equal(b0.indices.cpu().numpy(), new_of_old[loc])
            assert np.array_equal(want[b0.dst_in_src.cpu().numpy()], dst)
    g.close()


# ------------------------------------------------------------------------------------------------ 4. the item limit
def test_full_layer_item_limit(hiplib, oracle):
    """Node 0 has LIMIT - 1 distinct in-neighbours: one seed gives exactly LIMIT items and passes.  Node 1 has LIMIT in-edges: one
    item more, refused at sample_end with the layer named; the handle then samples exactly."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    n = LIMIT
    ip = np.zeros(n + 1, dtype=np.int64)
    ip[1], ip[2:] = LIMIT - 1, 2 * LIMIT - 1
    ix = np.concatenate([np.arange(1, LIMIT), np.random.default_rng(0).permutation(LIMIT)]).astype(np.int64)
    d_ip, d_ix = _to_gpu(torch, ip, ix)
    g = NeighborSampler([1]).make_graph(d_ip, d_ix)
    smp = NeighborSampler([-1])
    inp, _, (b,) = smp.sample(g, torch.tensor([0], device="cuda"))
    assert b.num_src == LIMIT and inp.numel() == LIMIT
    assert torch.equal(inp.cpu(), torch.arange(LIMIT))
    assert torch.equal(b.indices.cpu(), torch.arange(1, LIMIT, dtype=torch.int32)) and b.indptr.tolist() == [0, LIMIT - 1]
    with pytest.raises(RuntimeError, match=f"layer 0 holds {LIMIT + 1} items"):
        smp.sample(g, torch.tensor([1], device="cuda"))
    with pytest.raises(RuntimeError, match="layer 1 holds"):
        NeighborSampler([-1, 1], seed=2).sample(g, torch.tensor([5, 1], device="cuda"))   # the full layer second, from 3 nodes
    small = np.array([0, 3, 7], dtype=np.int64)
    del d_ip, d_ix, g
    torch.cuda.empty_cache()
    rng = np.random.default_rng(1)
    ip2, ix2 = csc_from_columns([rng.integers(0, 3000, size=rng.integers(0, 40)) for _ in range(3000)])
    g2 = NeighborSampler([1]).make_graph(*_to_gpu(torch, ip2, ix2))
    _check_call(oracle, NeighborSampler([-1, 3], seed=1), g2, ip2, ix2, small, 1)
    g2.close()


def _layer_call(L, g, seeds, fanouts, specs):
    """coala_sampler_sample_layers with guard-padded buffers; specs[l] = (src_cap, edge_cap, dst_cap).  -> (rc, buffers, n_src, n_edges)"""
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    bufs, lay = [], []
    for (src_cap, edge_cap, dst_cap), f in zip(specs, fanouts):
        src = torch.full((src_cap + GUARD,), -77, dtype=torch.int64, device="cuda")
        nbr = torch.full((edge_cap + GUARD,), -77, dtype=torch.int32, device="cuda")
        ind = torch.full((dst_cap + 1 + GUARD,), -77, dtype=torch.int64, device="cuda") if f == -1 else None
        bufs.append((src, nbr, ind))
        lay.append(_capi.SamplerLayer(src.data_ptr(), nbr.data_ptr(), ind.data_ptr() if ind is not None else None, src_cap, edge_cap))
    n = len(fanouts)
    n_src, n_edges = (C.c_int64 * n)(), (C.c_int64 * n)()
    rc = L.coala_sampler_sample_layers(g._h, seeds.data_ptr(), seeds.numel(), (C.c_int32 * n)(*fanouts), n, 0, 0, (_capi.SamplerLayer * n)(*lay),
                                       n_src, n_edges, None, None, current_stream())
    torch.cuda.synchronize()
    for (src_cap, edge_cap, dst_cap), (src, nbr, ind) in zip(specs, bufs):
        assert torch.all(src[src_cap:] == -77) and torch.all(nbr[edge_cap:] == -77), "write past a capacity"
        if ind is not None:
            assert torch.all(ind[dst_cap + 1:] == -77), "write past indptr_local"
    return rc, bufs, list(n_src), list(n_edges)


def test_full_layer_capacities_at_the_abi(hiplib, oracle, graphs):
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    ip, ix, d_ip, d_ix, seeds = graphs["powerlaw"]
    from COALA_GNN.sampler import NeighborSampler
    g = NeighborSampler([1]).make_graph(d_ip, d_ix)
    s = seeds[:100]
    src_r, ind_r, loc_r = full_layer(ip, ix, s)
    E, n_items = len(loc_r), 100 + len(loc_r)
    d_s = torch.from_numpy(s).cuda()
    rc, _, _, _ = _layer_call(L, g, d_s, [-1], [(n_items, E - 1, 100)])
    assert rc == _capi.EINVAL and f"layer 0 holds {n_items} items" in _capi.last_error() and "edge_cap" in _capi.last_error()
    rc, _, _, _ = _layer_call(L, g, d_s, [-1], [(n_items - 1, E, 100)])
    assert rc == _capi.EINVAL and "src_cap" in _capi.last_error()
    # a fixed layer behind the full one, bounded on the device: too small a src_cap refuses it, naming layer 1
    worst = len(src_r) * 4
    rc, _, n_src, _ = _layer_call(L, g, d_s, [-1, 3], [(n_items, E, 100), (worst - 1, worst, n_items)])
    assert rc == _capi.EINVAL and f"layer 1 would hold {worst} items" in _capi.last_error() and n_src[0] == len(src_r)
    rc, (b0, b1), n_src, n_edges = _layer_call(L, g, d_s, [-1, 3], [(n_items, E, 100), (worst, len(src_r) * 3, n_items)])
    assert rc == 0, _capi.last_error()
    ref = reference_layers(oracle, ip, ix, s, [-1, 3], 0, 0)
    assert n_src == [len(ref[0][0]), len(ref[1][0])] and n_edges == [E, len(src_r) * 3]
    assert np.array_equal(b0[0][: n_src[0]].cpu().numpy(), src_r) and np.array_equal(b0[2][:101].cpu().numpy(), ind_r)
    assert np.array_equal(b0[1][:E].cpu().numpy(), loc_r)
    assert np.array_equal(b1[0][: n_src[1]].cpu().numpy(), ref[1][0])
    assert np.array_equal(b1[1][: n_src[0] * 3].cpu().numpy(), ref[1][2].reshape(-1))
    with pytest.raises(RuntimeError, match="outside 1..32"):   # the dense entry point keeps refusing -1
        src = torch.empty(1000, dtype=torch.int64, device="cuda")
        _capi.check(L.coala_sampler_sample(g._h, d_s.data_ptr(), 100, (C.c_int32 * 1)(-1), 1, 0, 0, (C.c_void_p * 1)(src.data_ptr()),
                                           (C.c_void_p * 1)(src.data_ptr()), (C.c_int64 * 1)(), None, None, None))
    g.close()


# ------------------------------------------------------------------------------------------------ 5. handle reuse
def test_full_and_fixed_calls_reuse_one_handle(hiplib, oracle):
    """One handle, fixed and full lists of growing and shrinking sizes, a hash-table regrowth in the middle: every call exact, so
    every call found the table clean."""
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import powerlaw_csc
    n = 300_000
    d_ip, d_ix = powerlaw_csc(n, 12.0, seed=8, device="cuda")
    ip, ix = d_ip.cpu().numpy(), d_ix.cpu().numpy()
    g = NeighborSampler([1]).make_graph(d_ip, d_ix)
    perm = np.random.default_rng(5).permutation(n).astype(np.int64)
    calls = [(1000, [5]), (1000, [-1]), (50, [-1, -1]), (5000, [10, 5]), (0, [-1]), (1, [-1]), (2000, [5, -1]), (3, [-1, 32]),
             (200_000, [31]),                     # table regrowth (6.4 M items)
             (10, [-1]), (20_000, [-1]), (7, [1, -1, 1]), (4000, [25, 10]), (300, [-1, 2]), (1, [32, 32]), (100, [-1, -1]),
             (30_000, [16]), (2, [-1])]
    for step, (k, fanouts) in enumerate(calls):
        _check_call(oracle, NeighborSampler(fanouts, seed=6), g, ip, ix, perm[:k] if step % 2 else perm[::-1][:k].copy(), step)
    g.close()


# ------------------------------------------------------------------------------------------------ 6. CSR mean aggregation
def _device(torch, arr, off, fill=None):
    flat = torch.full((off + arr.size + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    if fill is None:
        flat[off: off + arr.size] = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).cuda()
    else:
        flat[off: off + arr.size] = fill
    return flat, flat.data_ptr() + 4 * off


def _region(flat, off, shape):
    h = flat.cpu().numpy()
    n = int(np.prod(shape))
    pad = np.concatenate([h[:off], h[off + n:]])
    assert np.array_equal(pad.view(np.int32), np.full(pad.shape, SENTINEL).view(np.int32)), "write outside the output region"
    return h[off: off + n].reshape(shape)


def _csr_inputs(rng, n_dst, n_src, dim, hub):
    deg = rng.integers(0, 40, size=n_dst)
    deg[rng.random(n_dst) < 0.1] = 0                     # empty rows
    if hub:
        deg[n_dst // 2] = hub
    ind = np.zeros(n_dst + 1, dtype=np.int64)
    np.cumsum(deg, out=ind[1:])
    idx = rng.integers(0, n_src - 7, size=int(ind[-1])).astype(np.int32)
    x = rng.standard_normal((n_src, dim)).astype(np.float32)
    x[rng.random(n_src) < 0.03] *= np.float32(1e6)
    go = rng.standard_normal((n_dst, dim)).astype(np.float32)
    return ind, idx, x, go


@pytest.mark.parametrize("dim,off,hub", [(1, 0, 1_000_003), (16, 0, 1_000_003), (16, 1, 200_000), (65, 0, 50_000), (100, 0, 20_000),
                                         (100, 1, 0), (129, 1, 20_000), (1024, 0, 5000), (1024, 1, 0)])
def test_csr_mean_aggregate_against_float64(hiplib, dim, off, hub):
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    rng = np.random.default_rng(dim * 10 + off)
    n_dst, n_src = 3001, 2000
    ind, idx, x, go = _csr_inputs(rng, n_dst, n_src, dim, hub)
    d_ind, d_idx = _to_gpu(torch, ind, idx)
    h_buf, h_ptr = _device(torch, x, off)
    o_buf, o_ptr = _device(torch, np.empty((n_dst, dim), np.float32), off, fill=float(SENTINEL))
    _capi.check(L.coala_block_mean_aggregate_csr(0, d_ind.data_ptr(), d_idx.data_ptr(), h_ptr, o_ptr, n_dst, dim, current_stream()))
    got = _region(o_buf, off, (n_dst, dim)).astype(np.float64)
    deg = np.diff(ind)
    rows = np.repeat(np.arange(n_dst), deg)
    ref = np.zeros((n_dst, dim))
    mag = np.zeros((n_dst, dim))
    xd = x.astype(np.float64)
    for lo in range(0, len(idx), 1 << 18):
        np.add.at(ref, rows[lo: lo + (1 << 18)], xd[idx[lo: lo + (1 << 18)]])
        np.add.at(mag, rows[lo: lo + (1 << 18)], np.abs(xd[idx[lo: lo + (1 << 18)]]))
    c = np.maximum(deg, 1)[:, None]
    bound = (deg + 2)[:, None] * U * mag / c + 1e-30
    assert np.all(np.abs(got - ref / c) <= bound), "forward past the fp32 bound"
    assert np.all(got[deg == 0] == 0.0)
    g_buf, g_ptr = _device(torch, go, off)
    gs_buf, gs_ptr = _device(torch, np.empty((n_src, dim), np.float32), off, fill=0.0)
    _capi.check(L.coala_block_mean_aggregate_csr_backward(0, d_ind.data_ptr(), d_idx.data_ptr(), g_ptr, gs_ptr, n_dst, dim, current_stream()))
    got_b = _region(gs_buf, off, (n_src, dim)).astype(np.float64)
    ref_b = np.zeros((n_src, dim))
    mag_b = np.zeros((n_src, dim))
    t = go.astype(np.float64) / c
    src_t = torch.from_numpy(idx.astype(np.int64))
    rb, mb = torch.from_numpy(ref_b), torch.from_numpy(mag_b)
    for lo in range(0, len(idx), 1 << 18):
        r = torch.from_numpy(rows[lo: lo + (1 << 18)])
        rb.index_add_(0, src_t[lo: lo + (1 << 18)], torch.from_numpy(t)[r])
        mb.index_add_(0, src_t[lo: lo + (1 << 18)], torch.from_numpy(np.abs(t))[r])
    k = np.bincount(idx, minlength=n_src)
    kk = k[:, None].astype(np.float64)
    bound_b = (kk + 1) * U / (1 - (kk + 1) * U) * mb.numpy()
    assert np.all(np.abs(got_b - rb.numpy()) <= bound_b), "backward past the fp32 bound"
    assert np.all(got_b[k == 0] == 0.0)
    assert np.array_equal(_region(h_buf, off, (n_src, dim)), x) and np.array_equal(_region(g_buf, off, (n_dst, dim)), go)


@pytest.mark.parametrize("f,dim,off", [(32, 1024, 0), (8, 65, 1), (15, 4, 0), (1, 3, 1), (31, 129, 0)])
def test_csr_mean_aggregate_bitwise_equals_dense(hiplib, f, dim, off):
    """Rows both forms express (valid entries first, then -1 padding): the CSR kernel gives the dense kernel's bits."""
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    rng = np.random.default_rng(f + dim)
    n_dst, n_src = 5003, 900
    cnt = rng.integers(0, f + 1, size=n_dst)
    dense = rng.integers(0, n_src, size=(n_dst, f)).astype(np.int32)
    dense[np.arange(f)[None, :] >= cnt[:, None]] = -1
    ind = np.zeros(n_dst + 1, dtype=np.int64)
    np.cumsum(cnt, out=ind[1:])
    d_dense, d_ind, d_idx = _to_gpu(torch, dense, ind, dense[dense >= 0])
    x = rng.standard_normal((n_src, dim)).astype(np.float32)
    h_buf, h_ptr = _device(torch, x, off)
    a_buf, a_ptr = _device(torch, np.empty((n_dst, dim), np.float32), off, fill=float(SENTINEL))
    b_buf, b_ptr = _device(torch, np.empty((n_dst, dim), np.float32), off, fill=float(SENTINEL))
    _capi.check(L.coala_block_mean_aggregate(0, d_dense.data_ptr(), h_ptr, a_ptr, n_dst, f, dim, current_stream()))
    _capi.check(L.coala_block_mean_aggregate_csr(0, d_ind.data_ptr(), d_idx.data_ptr(), h_ptr, b_ptr, n_dst, dim, current_stream()))
    a, b = _region(a_buf, off, (n_dst, dim)), _region(b_buf, off, (n_dst, dim))
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_loader_with_full_layer(hiplib, oracle, tmp_path):
    import torch
    from _util import ColorFiles
    from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, SSD_INFO
    from COALA_GNN.harness import SageMean
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import alloc_pinned_table, block_colors, feature_rows_torch, powerlaw_csc
    torch.manual_seed(0)
    n_nodes, dim, batch, fan = 20000, 64, 64, [5, -1]
    table = alloc_pinned_table(n_nodes, dim, seed=3, device=0)
    indptr, indices = powerlaw_csc(n_nodes, 8.0, seed=1, device="cuda")
    labels = (torch.arange(n_nodes, device="cuda") * 7) % 5
    color, tk, sc, _ = block_colors(n_nodes, nodes_per_color=512)
    files = ColorFiles(tmp_path, color, tk, sc)
    comm = MPI_Comm_Manager(0)
    comm.initialize_nested_process_group("isolated")
    train_ids = torch.randperm(int(0.6 * n_nodes), generator=torch.Generator().manual_seed(0))[:64 * 6]
    nd = Node_Distributor(comm, train_ids, batch, files.color_file, files.topk_file, files.score_file, parsing_method="baseline")
    sampler = NeighborSampler(fan, seed=5)
    g = sampler.make_graph(indptr, indices, ndata={"labels": labels})
    loader = COALA_GNN_DataLoader(SSD_INFO(1, dim * 4, 1024, 0), nd, g, sampler, batch, dim, fan, 4, "cuda:0", refresh_counter=3,
                                  cache_backend="isolated", sim_buf=table, num_rows=n_nodes, prefetch=1)
    assert loader.COALA_GNN_Manager.max_sample_size == n_nodes     # min(item limit, rows): the -1 list was accepted
    model = SageMean(dim, 32, 5, 2).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    steps = 0
    for input_nodes, seeds, blocks, feat in loader:
        assert torch.equal(feat, feature_rows_torch(input_nodes, dim, 3))
        assert blocks[-1].nbr is None and blocks[0].nbr is not None and blocks[-1].num_dst == batch
        assert torch.equal(blocks[-1].dstdata["_ID"], seeds.to(blocks[-1].dstdata["_ID"].device))
        deg = (indptr[seeds.cuda() + 1] - indptr[seeds.cuda()]).cpu()
        assert torch.equal(blocks[-1].indptr.diff().cpu(), deg)
        labels_b = blocks[-1].dstdata["labels"].view(-1)
        loss = torch.nn.functional.cross_entropy(model(blocks, feat), labels_b)
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert torch.isfinite(loss)
        steps += 1
    assert steps == 5
    b = blocks[-1]
    h = torch.randn(b.num_src, 16, device="cuda", requires_grad=True)
    out = b.mean_aggregate(h)
    ref = b.mean_aggregate_torch(h.detach().double()).float()
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5)
    del loader
    table.close()
