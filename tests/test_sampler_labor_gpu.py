"""GPU tests of LABOR layer-neighbour sampling (COALA_GNN.sampler.LaborSampler; labor_count_scan / labor_insert in coala_sampler.hip).

The rule is exact integer arithmetic, so every output -- source lists, indptr, indices, edge ids, edge weights -- is compared bit for
bit with the numpy restatement of tests/_labor_ref.py (checked on its own in test_sampler_labor_cpu.py); -1 layers of a LABOR list
come from _full_ref.full_layer.  The input-node bound of test_labor_fetches_fewer_input_nodes (0.96 of NeighborSampler's count on every
batch) is halfway between the restatement's worst batch on that set-up (0.926) and no gain at all."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _full_ref import bucketed
from _labor_ref import edge_weights, labor_key, labor_layer, reference_layers
from _util import edge_case_graph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 67
HUB = 1_000_003


def _to_gpu(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _check_call(smp, g, ip, ix, seeds, step):
    """One sample of `smp` (unbucketed): every layer equal to the reference, bit for bit."""
    import torch
    input_nodes, out_nodes, blocks = smp.sample(g, torch.from_numpy(seeds).cuda(), step=step)
    rev = list(reversed(smp.fanouts))
    ref = reference_layers(ip, ix, seeds, rev, smp.seed, step, smp.layer_dependency)
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
        else:
            assert "_ID" not in b.edata
        n_before = len(list(b.tensors()))
        w = b.edata["edge_weights"]
        assert w.dtype == torch.float32 and np.array_equal(w.cpu().numpy().view(np.int32), edge_weights(ind_r).view(np.int32)), where
        assert len(list(b.tensors())) == n_before + 1 and any(t is w for t in b.tensors()), "tensors() must report the weights once made"
        n_dst = len(src_r)
    assert torch.equal(input_nodes, blocks[0].src_nodes) and torch.equal(out_nodes.cpu(), torch.from_numpy(seeds))
    return blocks


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.fixture(scope="module")
def graphs():
    from COALA_GNN.synthetic import community_csc, powerlaw_csc
    out = {}
    for name, make in (("powerlaw", powerlaw_csc), ("community", community_csc)):
        d_ip, d_ix = make(200_000, 30, seed=1, device="cuda")
        out[name] = (d_ip.cpu().numpy(), d_ix.cpu().numpy(), d_ip, d_ix)
    return out


@pytest.mark.parametrize("fanouts,dep", [([10, 10], False), ([5, 5], False), ([15, 10, 5], False), ([1], False), ([32], False),
                                         ([10, -1], False), ([-1, 10], False), ([10, 10], True), ([5, 10, -1], True)])
@pytest.mark.parametrize("name", ["powerlaw", "community"])
def test_labor_layers_exact(hiplib, graphs, name, fanouts, dep):
    from COALA_GNN.sampler import LaborSampler
    ip, ix, d_ip, d_ix = graphs[name]
    g = LaborSampler([1]).make_graph(d_ip, d_ix)
    n_seeds = 64 if -1 in fanouts else 512
    for seed, step in ((0, 0), (0, 5), (2**64 - 5, 2**64 - 1), (7, 0)):
        seeds = np.random.default_rng(seed % 1000 + step % 1000).permutation(len(ip) - 1)[:n_seeds].astype(np.int64)
        _check_call(LaborSampler(fanouts, seed=seed, edge_ids=True, layer_dependency=dep), g, ip, ix, seeds, step)
    _check_call(LaborSampler(fanouts, seed=3, layer_dependency=dep), g, ip, ix, seeds[: n_seeds // 3], 1)     # without edge ids
    g.close()


# ------------------------------------------------------------------------------------------------ 2. edge shapes
@pytest.fixture(scope="module")
def edge_graph():
    """Degrees 0, 1, k-1, k, k+1, 2k, 200 for k in (1, 5, 32), self-loops, columns that repeat one neighbour, and a hub of 10^6 in-edges
    (above kHubDegree = 4096: counted and compacted by a whole block)."""
    import torch
    ip, ix, special = edge_case_graph([1, 5, 32], n_plain=3000, hub_degree=HUB, seed=7)
    rng = np.random.default_rng(2)
    plain = np.setdiff1d(np.arange(len(ip) - 1), special)
    seeds = np.concatenate([special, rng.choice(plain, 300, replace=False)]).astype(np.int64)
    rng.shuffle(seeds)
    return (ip, ix) + tuple(_to_gpu(torch, ip, ix)) + (seeds,)


@pytest.mark.parametrize("fanouts", [[1], [5], [32], [5, 5], [32, 1], [5, -1]])
def test_labor_on_edge_graph(hiplib, edge_graph, fanouts):
    from COALA_GNN.sampler import LaborSampler
    ip, ix, d_ip, d_ix, seeds = edge_graph
    n = len(ip) - 1
    deg = ip[seeds + 1] - ip[seeds]
    k = fanouts[-1] if fanouts[-1] != -1 else HUB      # the fan-out of the layer sampled from the seeds
    assert (deg == 0).any() and (deg == HUB).any() and (k == HUB or ((deg == k).any() and (deg == k + 1).any()))
    g = LaborSampler([1]).make_graph(d_ip, d_ix)
    for step in (0, 1):
        blocks = _check_call(LaborSampler(fanouts, seed=k, edge_ids=True), g, ip, ix, seeds, step)
        got = np.diff(blocks[-1].indptr.cpu().numpy())
        assert np.array_equal(got[deg <= k], deg[deg <= k]), "a row of at most k in-edges takes them all"
    if -1 in fanouts:   # the restatement of a -1 layer takes node ids of the graph only
        g.close()
        return
    # duplicate seeds (every row of a repeated node is the same row) and out-of-range seeds (empty rows; the ids stay in the list)
    odd = np.concatenate([seeds[:50], seeds[:50], [n + 5, seeds[3], n, 2**40], seeds[50:80]]).astype(np.int64)
    blocks = _check_call(LaborSampler(fanouts, seed=1, edge_ids=True), g, ip, ix, odd, 3)
    lp = blocks[-1].indptr.cpu().numpy()
    assert lp[101] == lp[100] and lp[103] == lp[102] and lp[104] == lp[103]
    assert np.array_equal(np.diff(lp)[:50], np.diff(lp)[50:100])
    g.close()


def test_labor_many_hub_rows_in_one_tile(hiplib, edge_graph):
    """40 rows of the hub in one batch: more hub rows than a block defers in one pass (32), so the rest are counted by their lane
    groups -- the same counts either way, and the insert pass takes them all on whole blocks."""
    from COALA_GNN.sampler import LaborSampler
    ip, ix, d_ip, d_ix, seeds = edge_graph
    hub = len(ip) - 2
    assert ip[hub + 1] - ip[hub] == HUB
    batch = np.concatenate([seeds[:10], np.full(40, hub), seeds[10:20]]).astype(np.int64)
    g = LaborSampler([1]).make_graph(d_ip, d_ix)
    _check_call(LaborSampler([5], seed=2, edge_ids=True), g, ip, ix, batch, 0)
    g.close()


# ------------------------------------------------------------------------------------------------ 3. determinism
def test_labor_is_deterministic_and_steps_differ(hiplib, graphs):
    import torch
    from COALA_GNN.sampler import LaborSampler, NeighborSampler
    ip, ix, d_ip, d_ix = graphs["powerlaw"]
    g = LaborSampler([1]).make_graph(d_ip, d_ix)
    seeds = torch.from_numpy(np.random.default_rng(0).permutation(len(ip) - 1)[:1024]).cuda()
    smp = LaborSampler([10, 10], seed=4, edge_ids=True)
    a = smp.sample(g, seeds, step=7)
    NeighborSampler([5, 5], seed=4).sample(g, seeds[:300], step=7)        # another kind of call on the handle in between
    b = smp.sample(g, seeds, step=7)
    c = smp.sample(g, seeds, step=8)
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x.src_nodes, y.src_nodes) and torch.equal(x.indptr, y.indptr) and torch.equal(x.indices, y.indices)
        assert torch.equal(x.edata["_ID"], y.edata["_ID"]) and torch.equal(x.edata["edge_weights"], y.edata["edge_weights"])
    assert not torch.equal(a[2][-1].indptr, c[2][-1].indptr), "another step must give another sample"
    # the sampler's own step counter advances as NeighborSampler's does
    s2 = LaborSampler([10, 10], seed=4, edge_ids=True)
    s2.step = 7
    d = s2.sample(g, seeds)
    assert s2.step == 8 and torch.equal(d[0], a[0])
    g.close()


# ------------------------------------------------------------------------------------------------ 4. owner bucketing
@pytest.mark.parametrize("G", [4, 64])
@pytest.mark.parametrize("fanouts", [[10, 10], [5]])
def test_labor_owner_bucketing(hiplib, graphs, G, fanouts):
    import torch
    from COALA_GNN.sampler import LaborSampler
    ip, ix, d_ip, d_ix = graphs["powerlaw"]
    g = LaborSampler([1]).make_graph(d_ip, d_ix)
    rev = list(reversed(fanouts))
    for step, n_seeds in ((0, 1024), (1, 333)):
        seeds = np.random.default_rng(step).permutation(len(ip) - 1)[:n_seeds].astype(np.int64)
        ref = reference_layers(ip, ix, seeds, rev, 3, step)
        inp, _, blocks = LaborSampler(fanouts, seed=3, bucket_by_owner=G, edge_ids=True).sample(g, torch.from_numpy(seeds).cuda(), step=step)
        src_r, ind_r, loc_r, eid_r = ref[-1]
        want, sizes, new_of_old = bucketed(src_r, G)
        dst = ref[-2][0] if len(rev) > 1 else seeds
        b0 = blocks[0]
        assert np.array_equal(inp.cpu().numpy(), want) and np.array_equal(b0.src_nodes.cpu().numpy(), want)
        assert b0.owner_counts.cpu().tolist() == b0.owner_counts_host == sizes.tolist()
        assert np.array_equal(b0.dst_in_src.cpu().numpy(), new_of_old[: len(dst)])
        assert np.array_equal(want[b0.dst_in_src.cpu().numpy()], dst)
        assert np.array_equal(b0.indptr.cpu().numpy(), ind_r)
        assert np.array_equal(b0.indices.cpu().numpy(), new_of_old[loc_r])
        assert np.array_equal(b0.edata["_ID"].cpu().numpy(), eid_r)
        assert np.array_equal(b0.dstdata["_ID"].cpu().numpy(), dst)
        for l in range(len(rev) - 1):            # the layers behind the input layer are not bucketed
            b = blocks[len(rev) - 1 - l]
            assert b.dst_in_src is None and np.array_equal(b.src_nodes.cpu().numpy(), ref[l][0])
            assert np.array_equal(b.indices.cpu().numpy(), ref[l][2])
    g.close()


# ------------------------------------------------------------------------------------------------ 5. refusal
def _labor_call(L, g, seeds, fanouts, specs, wait=True):
    """coala_sampler_sample_layers_labor with guard-padded buffers; specs[l] = (src_cap, edge_cap, dst_cap).
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
    n = len(fanouts)
    n_src, n_edges = (C.c_int64 * n)(), (C.c_int64 * n)()
    eid_p = (C.c_void_p * n)(*[b[3].data_ptr() for b in bufs])
    ticket = C.c_int64(-1)
    rc = L.coala_sampler_sample_layers_labor(g._h, seeds.data_ptr(), seeds.numel(), (C.c_int32 * n)(*fanouts), n, 0, 0,
                                             (_capi.SamplerLayer * n)(*lay), eid_p, 0, None, None, None, C.byref(ticket), current_stream())
    if rc == 0 and wait:
        rc = L.coala_sampler_wait_layers(g._h, ticket.value, n_src, n_edges, None)
    torch.cuda.synchronize()
    for (src_cap, edge_cap, dst_cap), (src, nbr, ind, eid) in zip(specs, bufs):
        assert torch.all(src[src_cap:] == -77) and torch.all(nbr[edge_cap:] == -77) and torch.all(eid[edge_cap:] == -77), "write past a capacity"
        assert torch.all(ind[dst_cap + 1:] == -77), "write past indptr_local"
    return rc, bufs, list(n_src), list(n_edges)


def test_labor_refusal_names_the_layer_and_the_handle_stays_usable(hiplib, graphs):
    """The capacities reach the kernels through the C ABI (no oversized launch): a layer whose n_dst + E exceeds its src_cap, or whose E
    exceeds its edge_cap, is refused on the device -- the wait returns COALA_EINVAL with the layer and its item count, nothing is
    written past a capacity, and the same handle then samples exactly."""
    import torch
    from COALA_GNN.sampler import LaborSampler
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    ip, ix, d_ip, d_ix = graphs["powerlaw"]
    g = LaborSampler([1]).make_graph(d_ip, d_ix)
    s = np.random.default_rng(9).permutation(len(ip) - 1)[:100].astype(np.int64)
    d_s = torch.from_numpy(s).cuda()
    (src0, ind0, loc0, eid0), (src1, ind1, loc1, eid1) = reference_layers(ip, ix, s, [5, 5], 0, 0)
    E0, E1 = len(loc0), len(loc1)
    items0, items1 = 100 + E0, len(src0) + E1
    rc, _, _, _ = _labor_call(L, g, d_s, [5], [(items0, E0 - 1, 100)])
    assert rc == _capi.EINVAL and f"layer 0 holds {items0} items" in _capi.last_error() and "edge_cap" in _capi.last_error()
    rc, _, _, _ = _labor_call(L, g, d_s, [5], [(items0 - 1, E0, 100)])
    assert rc == _capi.EINVAL and f"layer 0 holds {items0} items" in _capi.last_error() and "src_cap" in _capi.last_error()
    rc, bufs, n_src, _ = _labor_call(L, g, d_s, [5, 5], [(items0, E0, 100), (items1 - 1, E1, items0)])
    assert rc == _capi.EINVAL and f"layer 1 holds {items1} items" in _capi.last_error() and n_src[0] == len(src0)
    assert np.array_equal(bufs[0][0][: len(src0)].cpu().numpy(), src0), "the layer in front of the refused one is complete"
    # sample_end is this wait: the refusal surfaces there as an error that names the layer
    with pytest.raises(RuntimeError, match="layer 1 holds"):
        _capi.check(rc)
    # exactly enough: accepted, and equal to the reference
    rc, (b0, b1), n_src, n_edges = _labor_call(L, g, d_s, [5, 5], [(items0, E0, 100), (items1, E1, items0)])
    assert rc == 0, _capi.last_error()
    assert n_src == [len(src0), len(src1)] and n_edges == [E0, E1]
    for (src, nbr, ind, eid), (src_r, ind_r, loc_r, eid_r), n_dst in ((b0, (src0, ind0, loc0, eid0), 100), (b1, (src1, ind1, loc1, eid1), len(src0))):
        assert np.array_equal(src[: len(src_r)].cpu().numpy(), src_r) and np.array_equal(ind[: n_dst + 1].cpu().numpy(), ind_r)
        assert np.array_equal(nbr[: len(loc_r)].cpu().numpy(), loc_r) and np.array_equal(eid[: len(eid_r)].cpu().numpy(), eid_r)
    # a null indptr_local is refused before any launch
    lay = (_capi.SamplerLayer * 1)(_capi.SamplerLayer(b0[0].data_ptr(), b0[1].data_ptr(), None, items0, E0))
    rc = L.coala_sampler_sample_layers_labor(g._h, d_s.data_ptr(), 100, (C.c_int32 * 1)(5), 1, 0, 0, lay, None, 0, None, None, None, None, None)
    assert rc == _capi.EINVAL and "null buffer" in _capi.last_error()
    _check_call(LaborSampler([5, 5], seed=1, edge_ids=True), g, ip, ix, s[:30], 2)
    g.close()


# ------------------------------------------------------------------------------------------------ 6. the purpose
def test_labor_fetches_fewer_input_nodes(hiplib, graphs):
    """powerlaw_csc(200000, 30, seed=1), fan-outs [10, 10], batch 1024, 8 batches: on every batch LaborSampler's input-node count is at
    most 0.96 of NeighborSampler's on the same seeds."""
    import torch
    from COALA_GNN.sampler import LaborSampler, NeighborSampler
    ip, ix, d_ip, d_ix = graphs["powerlaw"]
    g = LaborSampler([1]).make_graph(d_ip, d_ix)
    perm = np.random.default_rng(2024).permutation(len(ip) - 1)
    labor, plain = LaborSampler([10, 10], seed=1), NeighborSampler([10, 10], seed=1)
    ratios, picks = [], []
    for b in range(8):
        seeds = torch.from_numpy(perm[b * 1024: (b + 1) * 1024]).cuda()
        in_l, _, bl = labor.sample(g, seeds, step=b)
        in_p, _, _ = plain.sample(g, seeds, step=b)
        ratios.append(in_l.numel() / in_p.numel())
        for blk in bl:
            dst = blk.dstdata["_ID"]
            deg = (d_ip[dst + 1] - d_ip[dst])
            picks.append((blk.indptr.diff()[deg > 10].float().mean().item(), int((deg > 10).sum())))
    print("LABOR / neighbour-sampling input nodes per batch:", " ".join(f"{r:.4f}" for r in ratios))
    print("mean picks per sampled row, per block:", " ".join(f"{m:.3f}" for m, _ in picks))
    assert all(r <= 0.96 for r in ratios), ratios
    g.close()


# ------------------------------------------------------------------------------------------------ 7. consumers
def test_labor_edge_weights_make_the_weighted_sum_the_mean(hiplib, graphs):
    """mean_aggregate(h) against weighted_sum_aggregate(h, edata['edge_weights']), w = fl(1 / cnt).  Both are within their fp32 bounds of
    the exact mean (u = 2^-24): the mean within (cnt + 2) u sum|x_j| / cnt (test_block_ops_gpu.py), the weighted sum within gamma(cnt + 1)
    sum|w x_j| of the exact sum of w x_j (the CSR bound of test_weighted_sum_gpu.py), which is within u sum|x_j| / cnt of the exact mean
    as |w - 1 / cnt| <= u / cnt.  Asserted: |difference| <= (gamma(cnt + 1) + (cnt + 4) u) sum|x_j| / cnt."""
    import torch
    from COALA_GNN.sampler import LaborSampler
    from test_block_ops_gpu import U, _gamma
    ip, ix, d_ip, d_ix = graphs["community"]
    g = LaborSampler([1]).make_graph(d_ip, d_ix)
    seeds = torch.from_numpy(np.random.default_rng(3).permutation(len(ip) - 1)[:1024]).cuda()
    _, _, blocks = LaborSampler([10, 10], seed=2).sample(g, seeds, step=0)
    for b in blocks:
        torch.manual_seed(b.num_src)
        h = torch.randn(b.num_src, 96, device="cuda")
        m = b.mean_aggregate(h).cpu().numpy().astype(np.float64)
        s = b.weighted_sum_aggregate(h, b.edata["edge_weights"]).cpu().numpy().astype(np.float64)
        lp, idx = b.indptr.cpu().numpy(), b.indices.cpu().numpy()
        cnt = np.diff(lp)
        mag = np.add.reduceat(np.abs(h.cpu().numpy().astype(np.float64))[idx], np.minimum(lp[:-1], len(idx) - 1)) * (cnt > 0)[:, None]
        bound = (_gamma(cnt + 1) + (cnt + 4) * U)[:, None] * mag / np.maximum(cnt, 1)[:, None]
        assert np.all(np.abs(m - s) <= bound), float(np.max(np.abs(m - s) - bound))
        assert np.array_equal(b.in_degrees().cpu().numpy(), cnt) and int(b.out_degrees().sum()) == len(idx)
    g.close()


@pytest.mark.parametrize("G", [0, 1])
def test_loader_with_labor_sampler(hiplib, oracle, tmp_path, G):
    """A COALA_GNN_DataLoader epoch with LaborSampler (G = 1: the owner-bucketed input layer): the rows delivered are the rows of the
    input nodes, the blocks are ragged, and a model trains on them."""
    import torch
    from _util import ColorFiles
    from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, SSD_INFO
    from COALA_GNN.harness import SageMean
    from COALA_GNN.sampler import LaborSampler
    from COALA_GNN.synthetic import alloc_pinned_table, block_colors, feature_rows_torch, powerlaw_csc
    torch.manual_seed(0)
    n_nodes, dim, batch, fan = 20000, 64, 64, [5, 5]
    table = alloc_pinned_table(n_nodes, dim, seed=3, device=0)
    indptr, indices = powerlaw_csc(n_nodes, 8.0, seed=1, device="cuda")
    labels = (torch.arange(n_nodes, device="cuda") * 7) % 5
    color, tk, sc, _ = block_colors(n_nodes, nodes_per_color=512)
    files = ColorFiles(tmp_path, color, tk, sc)
    comm = MPI_Comm_Manager(0)
    comm.initialize_nested_process_group("isolated")
    train_ids = torch.randperm(int(0.6 * n_nodes), generator=torch.Generator().manual_seed(0))[:64 * 6]
    nd = Node_Distributor(comm, train_ids, batch, files.color_file, files.topk_file, files.score_file, parsing_method="baseline")
    sampler = LaborSampler(fan, seed=5, bucket_by_owner=G)
    g = sampler.make_graph(indptr, indices, ndata={"labels": labels})
    loader = COALA_GNN_DataLoader(SSD_INFO(1, dim * 4, 1024, 0), nd, g, sampler, batch, dim, fan, 4, "cuda:0", refresh_counter=3,
                                  cache_backend="isolated", sim_buf=table, num_rows=n_nodes, prefetch=1)
    model = SageMean(dim, 32, 5, 2).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    steps = 0
    ip, ix = indptr.cpu().numpy(), indices.cpu().numpy()
    for input_nodes, seeds, blocks, feat in loader:
        assert torch.equal(feat, feature_rows_torch(input_nodes, dim, 3))
        assert all(b.nbr is None for b in blocks) and blocks[-1].num_dst == batch
        assert torch.equal(blocks[-1].dstdata["_ID"], seeds.to(blocks[-1].dstdata["_ID"].device))
        ref = reference_layers(ip, ix, seeds.cpu().numpy(), [5, 5], 5, steps)
        assert np.array_equal(np.sort(input_nodes.cpu().numpy()), np.sort(ref[-1][0]))
        labels_b = blocks[-1].dstdata["labels"].view(-1)
        loss = torch.nn.functional.cross_entropy(model(blocks, feat), labels_b)
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert torch.isfinite(loss)
        steps += 1
    assert steps == 5
    del loader
    table.close()


def test_train_synthetic_with_labor_sampler(hiplib):
    """examples/train_synthetic.py --sampler labor in a child process with its own time limit: a finite loss that went down."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), "--nodes", "60000", "--dim", "64", "--batch_size", "256",
           "--epochs", "1", "--cache_size", "4", "--prefetch", "1", "--fan_out", "10,5", "--sampler", "labor", "--layer_dependency"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    first, last = re.search(r"first loss (\S+)", r.stdout), re.search(r"final loss (\S+)", r.stdout)
    assert first and last and "Test Acc" in r.stdout, r.stdout[-2000:]
    first, last = float(first.group(1)), float(last.group(1))
    print(f"loss {first} -> {last}")
    assert math.isfinite(first) and math.isfinite(last) and last < first
