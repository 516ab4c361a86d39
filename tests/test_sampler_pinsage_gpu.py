"""GPU tests of random-walk neighbour sampling (COALA_GNN.sampler.RandomWalkNeighborSampler and random_walk; walk_select / walk_trace in
coala_sampler.hip).

The rule is exact integer arithmetic, so every output -- neighbours, source lists, visit counts, traces -- is compared bit for bit with
the numpy restatement of tests/_pinsage_ref.py (checked on its own in test_sampler_pinsage_cpu.py).  The graph is the smallest that
holds every way the kernel can go wrong: the degree edges, self-loops and repeated neighbours of _util.edge_case_graph, a node whose
only in-neighbour is itself, a 2-cycle, a sink one hop away, one node of in-degree 5,000 and 2,000 plain nodes."""
import ctypes as C

import numpy as np
import pytest

from _full_ref import bucketed
from _pinsage_ref import reference_layers, select, threshold, traces
from _util import csc_from_columns, edge_case_graph

pytestmark = pytest.mark.gpu

HUB = 5000
# (T, W, k, p): DGL's example setting; the smallest case; 512 visits, the whole LDS array; the heavy setting; W no power of two; k above
# the distinct visits
PARAMS = [(2, 10, 3, 0.5), (1, 1, 1, 0.0), (16, 32, 32, 0.0), (8, 64, 32, 0.25), (3, 17, 5, 0.9), (4, 16, 32, 0.0)]
# T = 2: (W, k) on both sides of every group size -- 16 lanes while max(W, k + 1) <= 16, 32 up to 32, then 64
GROUPS = [(16, 3), (17, 3), (32, 3), (33, 3), (64, 3), (16, 15), (4, 16), (32, 31), (4, 32)]


@pytest.fixture(scope="module")
def walk_graph(hiplib):
    """-> (indptr, indices, graph on the device, seeds, named nodes).  Seeds (at most 1,024): every special node, duplicates, -1 and
    num_nodes, random plain nodes."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, special = edge_case_graph([1, 3, 5, 32], n_plain=2000, hub_degree=HUB, seed=5)
    n0 = len(ip) - 1
    cols = [ix[ip[v]: ip[v + 1]] for v in range(n0)]
    own, a, b, sink, above = n0, n0 + 1, n0 + 2, n0 + 3, n0 + 4
    cols += [[own], [b], [a], [], [sink]]          # its own only in-neighbour; a 2-cycle; a sink; a node one hop above the sink
    ip, ix = csc_from_columns(cols)
    n = len(ip) - 1
    named = dict(own=own, a=a, b=b, sink=sink, above=above, hub=n0 - 1)
    assert ip[n0] - ip[n0 - 1] == HUB
    rng = np.random.default_rng(8)
    plain = np.setdiff1d(np.arange(n0), special)
    seeds = np.concatenate([special, [own, a, b, sink, above], rng.choice(plain, 500, replace=False), special[:20], [-1, n, own, n + 7]])
    seeds = seeds.astype(np.int64)
    rng.shuffle(seeds)
    assert len(seeds) <= 1024
    g = NeighborSampler.make_graph(torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda())
    yield ip, ix, g, seeds, named
    g.close()


_REFS = {}


def _reference(ip, ix, seeds, ks_rev, T, W, p, seed, step):
    """reference_layers, computed once per argument set and shared (the arrays are not modified)."""
    key = (seeds.tobytes(), tuple(ks_rev), T, W, p, seed, step)
    if key not in _REFS:
        _REFS[key] = reference_layers(ip, ix, seeds, ks_rev, T, W, threshold(p), seed, step)
    return _REFS[key]


def _check_call(smp, g, ip, ix, seeds, step):
    """One unbucketed sample of `smp`: every layer equal to the reference, bit for bit."""
    import torch
    input_nodes, out_nodes, blocks = smp.sample(g, torch.from_numpy(seeds).cuda(), step=step)
    rev = list(reversed(smp.fanouts))
    ref = _reference(ip, ix, seeds, rev, smp.num_traversals, smp.num_random_walks, smp.termination_prob, smp.seed, step)
    n_dst = len(seeds)
    assert len(blocks) == len(rev)
    for l, (src_r, loc_r, cnt_r, nbr_r) in enumerate(ref):
        b = blocks[len(rev) - 1 - l]
        k = rev[l]
        where = f"layer {l} of {rev}, T {smp.num_traversals} W {smp.num_random_walks} p {smp.termination_prob}, {len(seeds)} seeds, step {step}"
        assert b.indptr is None and b.indices is None and b.num_dst == n_dst, where
        assert b.nbr.dtype == torch.int32 and tuple(b.nbr.shape) == (n_dst, k), where
        assert np.array_equal(b.src_nodes.cpu().numpy(), src_r), f"source list differs: {where}"
        assert np.array_equal(b.nbr.cpu().numpy(), loc_r), f"nbr differs: {where}"
        assert "_ID" not in b.edata and "weights" in b.edata
        c = b.edata["visit_counts"]
        assert c.dtype == torch.int32 and np.array_equal(c.cpu().numpy(), cnt_r), f"visit counts differ: {where}"
        n_before = len(list(b.tensors()))
        w = b.edata["weights"]
        assert w.dtype == torch.float32 and tuple(w.shape) == (n_dst, k), where
        assert np.array_equal(w.cpu().numpy(), cnt_r.astype(np.float32)), f"weights differ: {where}"
        assert np.all(w.cpu().numpy()[loc_r < 0] == 0), "a padding slot has a weight"
        assert len(list(b.tensors())) == n_before + 1 and any(t is w for t in b.tensors()), "tensors() must report the weights once made"
        n_dst = len(src_r)
    assert torch.equal(input_nodes, blocks[0].src_nodes) and torch.equal(out_nodes.cpu(), torch.from_numpy(seeds))
    return blocks, ref


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("T,W,k,p", PARAMS)
def test_walk_layers_exact(walk_graph, T, W, k, p):
    from COALA_GNN.sampler import RandomWalkNeighborSampler
    ip, ix, g, seeds, named = walk_graph
    blocks, ref = _check_call(RandomWalkNeighborSampler(k, T, p, W, seed=3), g, ip, ix, seeds, 0)
    nbr = ref[0][3]
    at = {name: int(np.flatnonzero(seeds == v)[0]) for name, v in named.items()}
    assert nbr[at["own"], 0] == named["own"] and np.all(nbr[at["own"], 1:] == -1), "a self-loop-only node visits itself alone"
    assert np.all(nbr[at["sink"]] == -1) and nbr[at["above"]].tolist() == [named["sink"]] + [-1] * (k - 1)
    assert set(nbr[at["a"]][nbr[at["a"]] >= 0].tolist()) <= {named["a"], named["b"]}
    assert np.all(nbr[(seeds < 0) | (seeds >= len(ip) - 1)] == -1), "an out-of-range seed has an empty row"
    # two layers: a few seeds where k is large, all of them otherwise
    sub = seeds if k <= 5 else seeds[:48]
    _check_call(RandomWalkNeighborSampler([k, k], T, p, W, seed=2**64 - 5), g, ip, ix, sub, 2**64 - 1)


def test_three_layers_and_mixed_k(walk_graph):
    from COALA_GNN.sampler import RandomWalkNeighborSampler
    ip, ix, g, seeds, _ = walk_graph
    _check_call(RandomWalkNeighborSampler([3, 2, 4], 2, 0.5, 10, seed=1), g, ip, ix, seeds[:300], 5)


@pytest.mark.parametrize("W,k", GROUPS)
def test_group_size_boundaries(walk_graph, W, k):
    from COALA_GNN.sampler import RandomWalkNeighborSampler
    ip, ix, g, seeds, _ = walk_graph
    _check_call(RandomWalkNeighborSampler(k, 2, 0.0, W, seed=W), g, ip, ix, seeds[:257], 1)


@pytest.mark.parametrize("n_seeds", [0, 1])
def test_tiny_batches(walk_graph, n_seeds):
    from COALA_GNN.sampler import RandomWalkNeighborSampler
    ip, ix, g, seeds, named = walk_graph
    s = np.array([named["hub"]][:n_seeds], dtype=np.int64)
    blocks, _ = _check_call(RandomWalkNeighborSampler([3, 2], 2, 0.5, 10, seed=0), g, ip, ix, s, 0)
    assert blocks[-1].num_dst == n_seeds and tuple(blocks[-1].edata["weights"].shape) == (n_seeds, 2)


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_walks_are_deterministic_and_steps_differ(walk_graph):
    import torch
    from COALA_GNN.sampler import NeighborSampler, RandomWalkNeighborSampler
    ip, ix, g, seeds, _ = walk_graph
    d_seeds = torch.from_numpy(seeds).cuda()
    smp = RandomWalkNeighborSampler([5, 5], 3, 0.3, 20, seed=4)
    a = smp.sample(g, d_seeds, step=7)
    NeighborSampler([5, 5], seed=4).sample(g, d_seeds[:300], step=7)        # another kind of call on the handle in between
    b = smp.sample(g, d_seeds, step=7)
    c = smp.sample(g, d_seeds, step=8)
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x.src_nodes, y.src_nodes) and torch.equal(x.nbr, y.nbr) and torch.equal(x.edata["weights"], y.edata["weights"])
    assert not torch.equal(a[2][-1].edata["visit_counts"], c[2][-1].edata["visit_counts"]), "another step must give another sample"
    s2 = RandomWalkNeighborSampler([5, 5], 3, 0.3, 20, seed=4)
    s2.step = 7
    d = s2.sample(g, d_seeds)
    assert s2.step == 8 and torch.equal(d[0], a[0])
    # a uniform layer at the same seed and step draws from another stream
    u = NeighborSampler([5], seed=4).sample(g, d_seeds, step=7)
    w1 = RandomWalkNeighborSampler(5, 1, 0.0, 5, seed=4).sample(g, d_seeds, step=7)
    assert not torch.equal(u[0], w1[0])


# ------------------------------------------------------------------------------------------------ 3. owner bucketing
@pytest.mark.parametrize("ks", [[3, 3], [5]])
def test_walk_owner_bucketing(walk_graph, ks):
    import torch
    from COALA_GNN.sampler import RandomWalkNeighborSampler
    ip, ix, g, seeds, _ = walk_graph
    G = 4
    s = np.unique(seeds[(seeds >= 0) & (seeds < len(ip) - 1)])[:333]      # distinct nodes of the graph: the blocks' "dst first" convention
    rev = list(reversed(ks))
    ref = _reference(ip, ix, s, rev, 2, 10, 0.5, 3, 1)
    inp, _, blocks = RandomWalkNeighborSampler(ks, 2, 0.5, 10, seed=3, bucket_by_owner=G).sample(g, torch.from_numpy(s).cuda(), step=1)
    src_r, loc_r, cnt_r, _ = ref[-1]
    want, sizes, new_of_old = bucketed(src_r, G)
    dst = ref[-2][0] if len(rev) > 1 else s
    b0 = blocks[0]
    assert np.array_equal(inp.cpu().numpy(), want) and np.array_equal(b0.src_nodes.cpu().numpy(), want)
    assert b0.owner_counts.cpu().tolist() == b0.owner_counts_host == sizes.tolist()
    assert np.array_equal(b0.dst_in_src.cpu().numpy(), new_of_old[: len(dst)])
    assert np.array_equal(want[b0.dst_in_src.cpu().numpy()], dst)
    assert np.array_equal(b0.nbr.cpu().numpy(), np.where(loc_r >= 0, new_of_old[np.maximum(loc_r, 0)], -1))
    assert np.array_equal(b0.edata["weights"].cpu().numpy(), cnt_r.astype(np.float32))
    assert np.array_equal(b0.dstdata["_ID"].cpu().numpy(), dst)
    for l in range(len(rev) - 1):            # the layers behind the input layer are not bucketed
        b = blocks[len(rev) - 1 - l]
        assert b.dst_in_src is None and np.array_equal(b.src_nodes.cpu().numpy(), ref[l][0]) and np.array_equal(b.nbr.cpu().numpy(), ref[l][1])


# ------------------------------------------------------------------------------------------------ 4. traces
@pytest.mark.parametrize("T,W,p", [(2, 10, 0.5), (16, 32, 0.0), (8, 64, 0.25), (1, 1, 0.0)])
def test_random_walk_traces(walk_graph, T, W, p):
    import torch
    from COALA_GNN.sampler import RandomWalkNeighborSampler, random_walk
    ip, ix, g, seeds, _ = walk_graph
    tr = random_walk(g, torch.from_numpy(seeds).cuda(), T, restart_prob=p, num_walks=W, seed=6, step=2)
    assert tr.dtype == torch.int64 and tuple(tr.shape) == (len(seeds), W, T + 1)
    tr = tr.cpu().numpy()
    assert np.array_equal(tr, traces(ip, ix, seeds, W, T, threshold(p), 6, 2))
    # consistent with the layer: recounting a row from its traces gives the row
    k = 7
    _, _, blocks = RandomWalkNeighborSampler(k, T, p, W, seed=6).sample(g, torch.from_numpy(seeds).cuda(), step=2)
    nbr, cnt = select(tr, k)
    b = blocks[0]
    loc = b.nbr.cpu().numpy()
    got = np.where(loc >= 0, b.src_nodes.cpu().numpy()[np.maximum(loc, 0)], -1)
    assert np.array_equal(got, nbr) and np.array_equal(b.edata["visit_counts"].cpu().numpy(), cnt)
    assert tuple(random_walk(g, torch.zeros(0, dtype=torch.int64), T, num_walks=W).shape) == (0, W, T + 1)


# ------------------------------------------------------------------------------------------------ 5. consumers
@pytest.mark.parametrize("dim", [8, 128])
def test_block_ops_take_the_native_path_on_walk_blocks(walk_graph, monkeypatch, dim):
    """mean_aggregate against its float64 torch form within (cnt + 2) u sum|x_j| / cnt (test_block_ops_gpu.py), and
    weighted_sum_aggregate(h, edata['weights']) with both gradients within the bounds of test_weighted_sum_gpu.py (its _check)."""
    import torch
    from COALA_GNN import sampler as S
    from test_block_ops_gpu import U
    from test_weighted_sum_gpu import _check, _edge_list
    ip, ix, g, seeds, _ = walk_graph
    ran = []

    class Spy(object):
        def __init__(self, fn, name):
            self.fn, self.name = fn, name

        def apply(self, *a):
            ran.append(self.name)
            return self.fn.apply(*a)

    for name in ("_MeanAggregate", "_WeightedSum"):
        monkeypatch.setattr(S, name, Spy(getattr(S, name), name))
    for name in ("mean_aggregate_torch", "weighted_sum_aggregate_torch"):
        real = getattr(S.Block, name)
        monkeypatch.setattr(S.Block, name, lambda self, *a, _real=real, _name=name: (ran.append(_name), _real(self, *a))[1])
    _, _, blocks = S.RandomWalkNeighborSampler([5, 5], 2, 0.5, 10, seed=2).sample(g, torch.from_numpy(seeds).cuda(), step=0)
    for b in blocks:
        rng = np.random.default_rng(b.num_src + dim)
        x = rng.standard_normal((b.num_src, dim)).astype(np.float32)
        go = rng.standard_normal((b.num_dst, dim)).astype(np.float32)
        nbr = b.nbr.cpu().numpy()
        w = b.edata["weights"]
        del ran[:]
        m = b.mean_aggregate(torch.from_numpy(x).cuda())
        h = torch.from_numpy(x).cuda().requires_grad_(True)
        wt = w.clone().requires_grad_(True)
        out = b.weighted_sum_aggregate(h, wt)
        (out * torch.from_numpy(go).cuda()).sum().backward()
        assert ran == ["_MeanAggregate", "_WeightedSum"], ran
        cpu = S.Block(torch.arange(b.num_src), torch.from_numpy(nbr), b.num_dst)
        ref_m = cpu.mean_aggregate_torch(torch.from_numpy(x).double()).numpy()
        cnt = (nbr >= 0).sum(1)
        mag = (np.abs(x.astype(np.float64))[np.maximum(nbr, 0)] * (nbr >= 0)[..., None]).sum(1)
        bound = ((cnt + 2) * U)[:, None] * mag / np.maximum(cnt, 1)[:, None] + 1e-30
        assert np.all(np.abs(m.cpu().numpy().astype(np.float64) - ref_m) <= bound)
        rows, slots, srcs = _edge_list(nbr=nbr)
        _check(rows, slots, srcs, w.cpu().numpy(), x, go, b.num_dst, out.detach().cpu().numpy(), h.grad.cpu().numpy(), wt.grad.cpu().numpy(), "walk block")
        ref_s = cpu.weighted_sum_aggregate_torch(torch.from_numpy(x).double(), w.cpu().double())
        _check(rows, slots, srcs, w.cpu().numpy(), x, go, b.num_dst, ref_s.numpy(), None, None, "torch form")


def test_loader_with_walk_sampler(hiplib, oracle, tmp_path):
    """A short COALA_GNN_DataLoader epoch with RandomWalkNeighborSampler: on every step the rows delivered are the table's rows of input_nodes, and the
    input nodes are the reference's."""
    import torch
    from _util import ColorFiles
    from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, SSD_INFO
    from COALA_GNN.sampler import RandomWalkNeighborSampler
    from COALA_GNN.synthetic import alloc_pinned_table, block_colors, feature_rows_torch, powerlaw_csc
    n_nodes, dim, batch = 20000, 64, 64
    table = alloc_pinned_table(n_nodes, dim, seed=3, device=0)
    indptr, indices = powerlaw_csc(n_nodes, 8.0, seed=1, device="cuda")
    labels = (torch.arange(n_nodes, device="cuda") * 7) % 5
    color, tk, sc, _ = block_colors(n_nodes, nodes_per_color=512)
    files = ColorFiles(tmp_path, color, tk, sc)
    comm = MPI_Comm_Manager(0)
    comm.initialize_nested_process_group("isolated")
    train_ids = torch.randperm(int(0.6 * n_nodes), generator=torch.Generator().manual_seed(0))[:64 * 3]
    nd = Node_Distributor(comm, train_ids, batch, files.color_file, files.topk_file, files.score_file, parsing_method="baseline")
    sampler = RandomWalkNeighborSampler([5, 5], 2, 0.5, 10, seed=5)
    assert sampler.fanouts == [5, 5]
    g = sampler.make_graph(indptr, indices, ndata={"labels": labels})
    loader = COALA_GNN_DataLoader(SSD_INFO(1, dim * 4, 1024, 0), nd, g, sampler, batch, dim, sampler.fanouts, 4, "cuda:0", refresh_counter=3,
                                  cache_backend="isolated", sim_buf=table, num_rows=n_nodes, prefetch=1)
    ip, ix = indptr.cpu().numpy(), indices.cpu().numpy()
    steps = 0
    for input_nodes, seeds, blocks, feat in loader:
        assert torch.equal(feat, feature_rows_torch(input_nodes, dim, 3))
        assert all(b.nbr is not None and b.nbr.shape[1] == 5 for b in blocks) and blocks[-1].num_dst == batch
        ref = reference_layers(ip, ix, seeds.cpu().numpy(), [5, 5], 2, 10, threshold(0.5), 5, steps)
        assert np.array_equal(input_nodes.cpu().numpy(), ref[-1][0])
        assert np.array_equal(blocks[0].edata["weights"].cpu().numpy(), ref[-1][2].astype(np.float32))
        assert blocks[-1].dstdata["labels"].numel() == batch
        steps += 1
    assert steps >= 1
    del loader
    table.close()


# ------------------------------------------------------------------------------------------------ 6. arguments
def test_constructor_and_abi_refuse_bad_arguments(walk_graph):
    import torch
    from COALA_GNN.sampler import RandomWalkNeighborSampler, random_walk
    from COALA_GNN_Pybind import _capi
    ip, ix, g, seeds, _ = walk_graph
    R = RandomWalkNeighborSampler
    for bad in (lambda: R(0, 2, 0.5, 10), lambda: R(33, 2, 0.5, 10), lambda: R([5, -1], 2, 0.5, 10), lambda: R(5, 0, 0.5, 10),
                lambda: R(5, 17, 0.5, 10), lambda: R(5, 2, 0.5, 0), lambda: R(5, 2, 0.5, 65), lambda: R(5, 16, 0.5, 33),
                lambda: R(5, 2, 1.0, 10), lambda: R(5, 2, -0.1, 10), lambda: R(5, 2, float("nan"), 10), lambda: R(5, 2, 0.5, 10, prob="w"),
                lambda: R(5, 2, 0.5, 10, edge_ids=True), lambda: R([], 2, 0.5, 10), lambda: R(5, 2, 0.5, 10, bucket_by_owner=65),
                lambda: random_walk(g, torch.zeros(1, dtype=torch.int64), 17), lambda: random_walk(g, torch.zeros(1, dtype=torch.int64), 2, num_walks=65),
                lambda: random_walk(g, torch.zeros(1, dtype=torch.int64), 2, restart_prob=1.0)):
        with pytest.raises(ValueError):
            bad()
    assert R(5, 16, 0.5, 32).fanouts == [5] and R([3, 4], 2, 0.0, 10).fanouts == [3, 4]
    # the C ABI: every argument error comes back before any launch
    L = _capi.load()
    d_seeds = torch.from_numpy(seeds[:10]).cuda()
    src = torch.empty(10 * 6, dtype=torch.int64, device="cuda")
    nbr = torch.empty(10 * 5, dtype=torch.int32, device="cuda")
    ind = torch.empty(11, dtype=torch.int64, device="cuda")

    def call(f=5, T=2, W=10, thr=0, indptr_local=None, walk=True):
        lay = (_capi.SamplerLayer * 1)(_capi.SamplerLayer(src.data_ptr(), nbr.data_ptr(), indptr_local, 60, 50))
        wk = _capi.SamplerWalk(T, W, thr)
        return L.coala_sampler_sample_layers_walk(g._h, d_seeds.data_ptr(), 10, (C.c_int32 * 1)(f), 1, 0, 0, lay, C.byref(wk) if walk else None, None,
                                                  None, None, None, None, None)

    for kw, msg in ((dict(f=-1), "fan-out"), (dict(f=33), "fan-out"), (dict(f=0), "fan-out"), (dict(T=0), "num_traversals"), (dict(T=17), "num_traversals"),
                    (dict(W=0), "num_random_walks"), (dict(W=65), "num_random_walks"), (dict(T=16, W=33), "visits"), (dict(thr=1 << 53), "term_threshold"),
                    (dict(indptr_local=ind.data_ptr()), "indptr_local"), (dict(walk=False), "null")):
        assert call(**kw) == _capi.EINVAL and msg in _capi.last_error(), (kw, _capi.last_error())
    out = torch.empty(10 * 3, dtype=torch.int64, device="cuda")
    for args, msg in (((0, 2), "num_walks"), ((65, 2), "num_walks"), ((1, 0), "length"), ((1, 17), "length")):
        rc = L.coala_sampler_random_walk(g._h, d_seeds.data_ptr(), 10, args[0], args[1], 0, 0, 0, 0, out.data_ptr(), None)
        assert rc == _capi.EINVAL and msg in _capi.last_error()
    assert L.coala_sampler_random_walk(g._h, d_seeds.data_ptr(), 10, 1, 2, 1 << 53, 0, 0, 0, out.data_ptr(), None) == _capi.EINVAL
    assert L.coala_sampler_random_walk(g._h, d_seeds.data_ptr(), 10, 1, 2, 0, 0, 0, 8, out.data_ptr(), None) == _capi.EINVAL
    assert call() == 0, _capi.last_error()        # and the handle samples after all that
    torch.cuda.synchronize()
    _check_call(R(3, 2, 0.5, 10, seed=1), g, ip, ix, seeds[:40], 0)
