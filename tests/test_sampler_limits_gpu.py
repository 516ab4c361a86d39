"""GPU tests of the native sampler (coala_sampler.hip) where test_sampler_gpu.py does not reach: every sample_insert_kernel<GS>
instantiation (fan-outs 1..15 -> 16 lanes, 16..31 -> 32, 32 -> 64), graphs with zero-degree nodes, degree f-1 / f / f+1,
self-loops, repeated edges and a hub of 10^6 in-edges, a layer of exactly the item limit, the hash-table reuse across calls of
one handle, and owner bucketing above 16 parts (bucket_scan_kernel loops over its columns).  Every call is compared bit for bit
with the CPU twin (oracle.sample_blocks, itself pinned to a plain-Python restatement in test_oracle_cpu.py) and checked against
the sampler's published properties."""
import ctypes as C
import os

import numpy as np
import pytest

from _util import check_block_properties, edge_case_graph

pytestmark = pytest.mark.gpu

LIMIT = 8192 * 1024           # kMaxTiles * kTile: items a layer may hold
TWIN_THREADS = min(8, os.cpu_count() or 1)


def _to_gpu(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _sample_and_check(oracle, smp, g, ip, ix, seeds, step):
    """One call of `smp` on `g`: every layer equal to the twin, and the properties of every block."""
    import torch
    input_nodes, out_nodes, blocks = smp.sample(g, torch.from_numpy(seeds).cuda(), step=step)
    rev = list(reversed(smp.fanouts))
    twin = oracle.sample_blocks(ip, ix, seeds, rev, smp.seed, step, threads=TWIN_THREADS)
    dst = seeds
    for l, (src_t, local_t, _) in enumerate(twin):
        b = blocks[len(rev) - 1 - l]
        src, loc = b.src_nodes.cpu().numpy(), b.nbr.cpu().numpy()
        assert np.array_equal(src, src_t), f"source list differs from the twin at layer {l} (fan-outs {rev}, {len(seeds)} seeds)"
        assert np.array_equal(loc, local_t), f"local indices differ from the twin at layer {l} (fan-outs {rev}, {len(seeds)} seeds)"
        check_block_properties(ip, ix, dst, rev[l], src, loc)
        dst = src
    assert torch.equal(input_nodes, blocks[0].src_nodes)
    return blocks


# ------------------------------------------------------------------------------------------------ fan-outs and edge graphs
FANOUTS = [1, 2, 15, 16, 17, 24, 25, 31, 32]


@pytest.fixture(scope="module")
def edge_graph():
    import torch
    ip, ix, special = edge_case_graph(FANOUTS, n_plain=3000, hub_degree=1_000_003, seed=7)
    d_ip, d_ix = _to_gpu(torch, ip, ix)
    rng = np.random.default_rng(1)
    plain = np.setdiff1d(np.arange(len(ip) - 1), special)
    seeds = np.concatenate([special, rng.choice(plain, 500, replace=False)])   # the hub and the zero-degree nodes included
    rng.shuffle(seeds)
    edge_nodes = np.concatenate([special[:3], special[-1:]])                   # the degree-0 nodes and the hub
    few = np.concatenate([edge_nodes, seeds[~np.isin(seeds, edge_nodes)][:296]])  # 300 seeds for the multi-layer settings
    return ip, ix, d_ip, d_ix, seeds.astype(np.int64), few.astype(np.int64)


@pytest.mark.parametrize("f", FANOUTS)
def test_sampler_every_fanout_on_edge_graph(hiplib, oracle, edge_graph, f):
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, d_ip, d_ix, seeds, _ = edge_graph
    assert ip[-1] - ip[-2] >= 10**6 and (ip[1:] == ip[:-1]).any()
    smp = NeighborSampler([f], seed=f)
    g = smp.make_graph(d_ip, d_ix)
    for step in (0, 1):
        _sample_and_check(oracle, smp, g, ip, ix, seeds, step)
    g.close()


@pytest.mark.parametrize("fanouts", [[25, 10], [10, 25], [32, 1], [1, 32], [16, 15, 31], [32, 32, 1]])
def test_sampler_multilayer_on_edge_graph(hiplib, oracle, edge_graph, fanouts):
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, d_ip, d_ix, _, few = edge_graph
    smp = NeighborSampler(fanouts, seed=3)
    g = smp.make_graph(d_ip, d_ix)
    _sample_and_check(oracle, smp, g, ip, ix, few, step=5)
    g.close()


@pytest.mark.parametrize("f", [25, 32])
def test_sampler_uniformity_wide_groups(hiplib, f):
    """At f = 25 (32-lane groups, two per wave) and f = 32 (one 64-lane group) every in-neighbour of a degree-100 node is picked
    with probability f/100: 64 such nodes (same 100 in-neighbours, different keys) x 64 steps = 4096 draws, each count within
    6 sigma of 4096 * f / 100 (the bound of test_sampler_uniformity)."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    deg, n_seed_nodes, steps = 100, 64, 64
    n = n_seed_nodes + deg
    indptr = np.concatenate([np.arange(n_seed_nodes + 1) * deg, np.full(deg, n_seed_nodes * deg)]).astype(np.int64)
    indices = np.tile(np.arange(n_seed_nodes, n, dtype=np.int64), n_seed_nodes)
    d_ip, d_ix = _to_gpu(torch, indptr, indices)
    smp = NeighborSampler([f], seed=9)
    g = smp.make_graph(d_ip, d_ix)
    seeds = torch.arange(n_seed_nodes, device="cuda")
    counts = np.zeros(deg)
    for step in range(steps):
        _, _, (b,) = smp.sample(g, seeds, step=step)
        picked = b.src_nodes.cpu().numpy()[b.nbr.cpu().numpy()]
        assert all(len(np.unique(r)) == f for r in picked)
        np.add.at(counts, picked.reshape(-1) - n_seed_nodes, 1)
    trials = n_seed_nodes * steps
    expect = trials * f / deg
    assert counts.sum() == trials * f
    assert np.all(np.abs(counts - expect) < 6 * np.sqrt(expect)), (counts.min(), counts.max(), expect)
    g.close()


# ------------------------------------------------------------------------------------------------ the item limit
@pytest.fixture(scope="module")
def limit_graph():
    """262,144 'seed' nodes with 40 in-neighbours each, all of them distinct nodes (so a layer from these seeds has as many
    distinct sources as it has items), and behind them 10.5 M nodes of in-degree 0, 1 or 2."""
    import torch
    S, D = 262_144, 40
    n = S + S * D
    rng = np.random.default_rng(3)
    deg = np.empty(n, dtype=np.int64)
    deg[:S] = D
    deg[S:] = np.arange(S, n) % 3
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = np.empty(int(indptr[-1]), dtype=np.int64)
    indices[: S * D] = S + rng.permutation(S * D)
    indices[S * D:] = rng.integers(0, n, size=len(indices) - S * D)
    d_ip, d_ix = _to_gpu(torch, indptr, indices)
    return indptr, indices, d_ip, d_ix


def test_sampler_layer_at_item_limit(hiplib, oracle, limit_graph):
    """262,144 seeds at f = 31: exactly 8,388,608 items -- all 8192 look-back status words, a 2^24-slot hash table, sample_insert
    grid-stride -- and every item a distinct node."""
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, d_ip, d_ix = limit_graph
    smp = NeighborSampler([31], seed=2)
    g = smp.make_graph(d_ip, d_ix)
    seeds = np.random.default_rng(0).permutation(262_144).astype(np.int64)
    assert len(seeds) * 32 == LIMIT
    (b,) = _sample_and_check(oracle, smp, g, ip, ix, seeds, step=1)
    assert b.num_src == LIMIT
    g.close()


def test_sampler_second_layer_at_item_limit_then_refusal(hiplib, oracle, limit_graph):
    """[31, 1] from 131,072 seeds: the first layer yields 4,194,304 distinct sources, so the second layer holds exactly the limit
    (the capacity bound).  262,145 seeds at f = 31 would hold limit + 32 items: refused, and the same handle then samples a small
    batch correctly."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, d_ip, d_ix = limit_graph
    smp = NeighborSampler([1, 31], seed=4)
    g = smp.make_graph(d_ip, d_ix)
    seeds = np.random.default_rng(1).permutation(262_144)[:131_072].astype(np.int64)
    blocks = _sample_and_check(oracle, smp, g, ip, ix, seeds, step=0)
    assert blocks[1].num_src == 131_072 * 32 and blocks[0].num_dst * 2 == LIMIT
    with pytest.raises(RuntimeError, match="would hold"):
        NeighborSampler([31], seed=4).sample(g, torch.arange(262_145, device="cuda"))
    _sample_and_check(oracle, NeighborSampler([25, 10], seed=4), g, ip, ix, seeds[:1000], step=2)
    g.close()


def test_sampler_handle_reuse_across_calls(hiplib, oracle):
    """One handle, a sequence of calls with growing and shrinking seed counts (0 and 1 among them), changing fan-outs and layer
    counts, and a hash-table regrowth in the middle.  A call's first layer runs on the table the previous call's last kernel
    cleared (clean_items), or on a freshly cleared one when it needs more; every call equals the twin."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import powerlaw_csc
    n = 300_000
    d_ip, d_ix = powerlaw_csc(n, 12.0, seed=8, device="cuda")
    ip, ix = d_ip.cpu().numpy(), d_ix.cpu().numpy()
    g = NeighborSampler([1]).make_graph(d_ip, d_ix)
    perm = np.random.default_rng(5).permutation(n).astype(np.int64)
    calls = [(1000, [10, 5]), (0, [5]), (1, [32, 32]), (1, [1]), (5000, [15, 10]),
             (20_000, [32, 1]),          # first layer f = 1 (small), second f = 32: the table is dirty beyond the first layer's part
             (30_000, [16]),             # a larger first layer than the table left clean: cleared before use
             (100, [5]), (200_000, [31]),  # hash table regrowth (6.4 M items)
             (3, [1, 1, 1]), (0, [32, 32, 32]), (20_000, [16, 17]), (1, [32]), (4000, [25, 10, 5]), (50_000, [2, 24]), (7, [31, 1])]
    def table_slots(k, fanouts):              # the hash table a call needs (table_size of its largest layer)
        cap, most = k, 0
        for f in reversed(fanouts):
            cap *= f + 1
            most = max(most, cap)
        return max(1024, 1 << int(2 * most - 1).bit_length()) if most else 1024
    grow_at = [i for i, c in enumerate(calls) if table_slots(*c) > max(table_slots(*d) for d in calls[:i] or [(0, [1])])]
    assert grow_at[-1] == calls.index((200_000, [31]))
    for step, (k, fanouts) in enumerate(calls):
        smp = NeighborSampler(fanouts, seed=6)
        _sample_and_check(oracle, smp, g, ip, ix, perm[:k] if step % 2 else perm[::-1][:k].copy(), step)
    g.close()


# ------------------------------------------------------------------------------------------------ owner bucketing
@pytest.fixture(scope="module")
def bucket_graph():
    import torch
    rng = np.random.default_rng(11)
    n = 200_000
    deg = rng.integers(0, 25, size=n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = rng.integers(0, n, size=int(indptr[-1])).astype(np.int64)
    return (indptr, indices) + tuple(_to_gpu(torch, indptr, indices))


@pytest.mark.parametrize("G", [1, 5, 16, 17, 33, 63, 64])
def test_sampler_owner_bucketing_many_parts(hiplib, oracle, bucket_graph, G):
    """bucket_by_owner=G up to 64 parts on source lists of more than 64 route tiles (> 16,384 ids, not a multiple of 256): a stable
    partition by id % G, the bucket sizes on device and on host, the input block re-indexed onto the same nodes, dst_in_src."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, d_ip, d_ix = bucket_graph
    fanouts = [10, 10]
    plain = NeighborSampler(fanouts, seed=3)
    buck = NeighborSampler(fanouts, seed=3, bucket_by_owner=G)
    g = plain.make_graph(d_ip, d_ix)
    for step, n_seeds in ((0, 400), (1, 333)):
        seeds = np.random.default_rng(step).permutation(len(ip) - 1)[:n_seeds].astype(np.int64)
        twin = oracle.sample_blocks(ip, ix, seeds, list(reversed(fanouts)), 3, step)
        in_p, _, bl_p = plain.sample(g, torch.from_numpy(seeds).cuda(), step=step)
        in_b, _, bl_b = buck.sample(g, torch.from_numpy(seeds).cuda(), step=step)
        ids = in_p.cpu().numpy()
        assert np.array_equal(ids, twin[-1][0])
        assert len(ids) > 64 * 256 and len(ids) % 256, "the source list must span more than 64 route tiles, the last one partial"
        a, b = bl_p[0], bl_b[0]
        want = np.concatenate([ids[ids % G == o] for o in range(G)])             # stable partition
        assert np.array_equal(in_b.cpu().numpy(), want)
        assert b.owner_counts.cpu().tolist() == b.owner_counts_host == [int((ids % G == o).sum()) for o in range(G)]
        assert b.num_src == a.num_src and b.num_dst == a.num_dst
        na, nb = a.nbr.cpu().numpy(), b.nbr.cpu().numpy()
        assert np.array_equal(na < 0, nb < 0)
        assert np.array_equal(ids[na[na >= 0]], want[nb[nb >= 0]])
        assert np.array_equal(want[b.dst_in_src.cpu().numpy()], ids[: a.num_dst])
        for x, y in zip(bl_p[1:], bl_b[1:]):
            assert torch.equal(x.src_nodes, y.src_nodes) and torch.equal(x.nbr, y.nbr) and y.dst_in_src is None
    g.close()


@pytest.mark.parametrize("G", [3, 64])
def test_sampler_owner_bucketing_equals_cache_route(hiplib, bucket_graph, G):
    """The sampler's bucketing and the cache's route run the same per-tile code (coala_partition.h): the bucketed input nodes, the bucket sizes
    and dst_in_src of a bucket_by_owner=G call equal what a cache handle's route gives for the unbucketed source list of the same
    call (more than 64 wave tiles)."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    from _util import PinnedTable
    P = hiplib
    ip, _, d_ip, d_ix = bucket_graph
    plain = NeighborSampler([10, 10], seed=3)
    buck = NeighborSampler([10, 10], seed=3, bucket_by_owner=G)
    g = plain.make_graph(d_ip, d_ix)
    seeds = torch.from_numpy(np.random.default_rng(0).permutation(len(ip) - 1)[:400].astype(np.int64)).cuda()
    in_p, _, bl_p = plain.sample(g, seeds, step=0)
    _, _, bl_b = buck.sample(g, seeds, step=0)
    src, b = bl_p[0].src_nodes.contiguous(), bl_b[0]
    n = src.numel()
    assert n > 64 * 256 and torch.equal(src, in_p)
    table = PinnedTable(P, np.zeros((64, 128), dtype=np.float32))
    cache = P.Isolated_Cache(P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, table.dim, True), None, 0, 1, 1, table.device_ptr, num_rows=table.rows)
    node = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    mp = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    cnt = torch.full((G,), -1, dtype=torch.int64, device="cuda")
    cache.route(src.data_ptr(), n, G, node.data_ptr(), mp.data_ptr(), cnt.data_ptr())
    assert b.src_nodes.numel() == n and torch.equal(node[:n], b.src_nodes)
    assert torch.equal(cnt, b.owner_counts) and cnt.cpu().tolist() == b.owner_counts_host
    pos = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    pos[mp] = torch.arange(n, device="cuda")                                        # pos[d] = the p with map_out[p] == d
    assert b.num_dst > 0 and torch.equal(b.dst_in_src.long(), pos[: b.num_dst])
    cache.close()
    table.close()
    g.close()


def test_sampler_owner_bucketing_refuses_65_parts(hiplib, bucket_graph):
    import torch
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN_Pybind import _capi, current_stream
    with pytest.raises(ValueError, match="bucket_by_owner"):
        NeighborSampler([5], bucket_by_owner=65)
    L = _capi.load()
    _, _, d_ip, d_ix = bucket_graph
    g = NeighborSampler([5]).make_graph(d_ip, d_ix)
    seeds = torch.arange(64, device="cuda")
    src = torch.empty(64 * 6, dtype=torch.int64, device="cuda")
    nbr = torch.empty(64 * 5, dtype=torch.int32, device="cuda")
    bucketed = torch.empty(64 * 6, dtype=torch.int64, device="cuda")
    counts = torch.empty(65, dtype=torch.int64, device="cuda")
    dst_in_src = torch.empty(64, dtype=torch.int32, device="cuda")
    bk = _capi.SamplerBucketing(65, 0, bucketed.data_ptr(), counts.data_ptr(), dst_in_src.data_ptr())
    with pytest.raises(RuntimeError, match="n_parts"):
        _capi.check(L.coala_sampler_sample(g._h, seeds.data_ptr(), 64, (C.c_int32 * 1)(5), 1, 0, 0, (C.c_void_p * 1)(src.data_ptr()),
                                           (C.c_void_p * 1)(nbr.data_ptr()), (C.c_int64 * 1)(), C.byref(bk), None, current_stream()))
    g.close()
