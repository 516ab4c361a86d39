"""GPU tests of edge-weighted sampling (NeighborSampler(prob=...), coala_sampler_sample_layers_weighted).

Every layer is compared with the numpy restatement of tests/_weighted_ref.py bit for bit (source list, nbr_local).  The only
tolerated difference is a row whose f-th and (f+1)-th restated fp64 keys are within a relative 1e-12 (the device's log1p may round
differently in the last place); such rows are counted and must be almost none.  Inclusion frequencies are checked against exact
successive-sampling probabilities within 5 sigma."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _full_ref import bucketed, full_layer
from _sampler_sweep import TIE, check_weighted_call as _check_call
from _util import csc_from_columns, edge_case_graph
from _weighted_ref import inclusion_probabilities, reference_layers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 8192 * 1024


def _to_gpu(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _patterned_weights(ip, f, seed):
    """Per row, by node id % 7: random in (0, 1] with ~10 % zeros; all zero; exactly f positive among zeros; exactly f + 1 positive;
    one dominant weight (1e30 against 1e-30); denormal weights (1e-40) beside 1.0; all equal."""
    rng = np.random.default_rng(seed)
    deg = np.diff(ip)
    n, E = len(deg), int(ip[-1])
    rows = np.repeat(np.arange(n), deg)
    j = np.arange(E) - ip[rows]
    kind = rows % 7
    w = (1.0 - rng.random(E)).astype(np.float32)
    w[rng.random(E) < 0.1] = 0
    w[kind == 1] = 0
    rank = np.empty(E, dtype=np.int64)                  # a random rank of every edge inside its row
    order = np.lexsort((rng.random(E), rows))
    rank[order] = np.arange(E) - ip[rows[order]]
    w[(kind == 2)] = np.where(rank[kind == 2] < f, 1.0 + rng.random(int((kind == 2).sum())), 0).astype(np.float32)
    w[(kind == 3)] = np.where(rank[kind == 3] < f + 1, 1.0 + rng.random(int((kind == 3).sum())), 0).astype(np.float32)
    w[kind == 4] = np.where(rank[kind == 4] == 0, 1e30, 1e-30).astype(np.float32)
    w[kind == 5] = np.where(j[kind == 5] % 2 == 0, 1e-40, 1.0).astype(np.float32)
    w[kind == 6] = 0.5
    assert np.float32(1e-40) > 0
    return w


# ------------------------------------------------------------------------------------------------ 1. exactness
@pytest.fixture(scope="module")
def hub_graph():
    import torch
    ip, ix, special = edge_case_graph([1, 5, 16, 17, 32], n_plain=3000, hub_degree=1_000_003, seed=9)
    rng = np.random.default_rng(3)
    plain = np.setdiff1d(np.arange(len(ip) - 1), special)
    seeds = np.concatenate([special, rng.choice(plain, 300, replace=False)]).astype(np.int64)
    rng.shuffle(seeds)
    ws = {f"w{f}": _patterned_weights(ip, f, f) for f in (1, 5, 16, 17, 32)}
    d_ip, d_ix = _to_gpu(torch, ip, ix)
    from COALA_GNN.sampler import NeighborSampler
    g = NeighborSampler([1]).make_graph(d_ip, d_ix, edata={k: torch.from_numpy(v).cuda() for k, v in ws.items()})
    yield ip, ix, ws, seeds, g
    g.close()


@pytest.mark.parametrize("f", [1, 5, 16, 17, 32])
def test_weighted_layers_exact_on_edge_cases(hiplib, hub_graph, f):
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, ws, seeds, g = hub_graph
    assert g.max_in_degree == 1_000_003 and (seeds == len(ip) - 2).any()
    deg = np.diff(ip)[seeds]
    assert {0, f, f + 1}.issubset(set(deg.tolist())) and (deg < f).any()
    tol = 0
    for fanouts, seed, step, k in (([f], 0, 0, len(seeds)), ([5, f], 7, 2**64 - 1, len(seeds) // 3), ([f], 2**64 - 5, 2**64 - 2, 1),
                                   ([f], 3, 11, len(seeds))):
        _, t = _check_call(NeighborSampler(fanouts, seed=seed, prob=f"w{f}"), g, ip, ix, ws[f"w{f}"], seeds[:k], step)
        tol += t
    assert tol <= 1


@pytest.mark.parametrize("fanouts", [[5, 5], [15, 10, 5], [32, 1]])
def test_weighted_layers_exact_on_powerlaw(hiplib, fanouts):
    import torch
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import powerlaw_csc
    d_ip, d_ix = powerlaw_csc(200_000, 10.0, seed=4, device="cuda")
    ip, ix = d_ip.cpu().numpy(), d_ix.cpu().numpy()
    w = _patterned_weights(ip, 5, 1)
    g = NeighborSampler([1]).make_graph(d_ip, d_ix, edata={"w": torch.from_numpy(w).cuda()})
    seeds = np.random.default_rng(2).permutation(200_000)[:512].astype(np.int64)
    tol = 0
    for step in (0, 1, 99):
        tol += _check_call(NeighborSampler(fanouts, seed=4, prob="w"), g, ip, ix, w, seeds, step)[1]
    assert tol <= 1
    g.close()


# ------------------------------------------------------------------------------------------------ 2. statistics
def _replicated_graph(row, copies):
    """copies nodes with the same weighted in-edge row; position j of every row holds node j, so a pick names its position"""
    deg = len(row)
    ip = np.arange(copies + 1, dtype=np.int64) * deg
    ix = np.tile(np.arange(deg, dtype=np.int64), copies)
    w = np.tile(np.asarray(row, dtype=np.float32), copies)
    return ip, ix, w


@pytest.mark.parametrize("row,f", [([1, 2, 3, 4, 0, 10], 2), ([1, 2, 3, 4, 0, 10], 3), ([0.5, 0.5, 5, 1e-3, 2, 0], 2), ([1] * 6, 5)])
def test_inclusion_frequencies_match_exact_probabilities(hiplib, row, f):
    """20,000 copies of one weighted row: one call is 20,000 independent draws of that row."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    copies = 20_000
    ip, ix, w = _replicated_graph(row, copies)
    d_ip, d_ix = _to_gpu(torch, ip, ix)
    g = NeighborSampler([1]).make_graph(d_ip, d_ix, edata={"w": torch.from_numpy(w).cuda()})
    seeds = np.arange(copies, dtype=np.int64)
    blocks, tol = _check_call(NeighborSampler([f], seed=21, prob="w"), g, ip, ix, w, seeds, 5)
    assert tol == 0
    b = blocks[0]
    src, loc = b.src_nodes.cpu().numpy(), b.nbr.cpu().numpy()
    j = np.where(loc >= 0, src[np.maximum(loc, 0)], -1)             # the position each pick came from
    hits = np.bincount(j[j >= 0], minlength=len(row)) / copies
    p = inclusion_probabilities(row, f)
    assert np.all(np.abs(hits - p) <= 5 * np.sqrt(p * (1 - p) / copies) + 1e-12), (hits, p)
    g.close()


def test_equal_weights_give_uniform_inclusion_and_flat_hub_deciles(hiplib):
    import torch
    from COALA_GNN.sampler import NeighborSampler
    # 4,000 rows of 1,000 equal weights: every edge is taken with probability f / deg
    copies, deg, f = 4000, 1000, 32
    ip = np.arange(copies + 1, dtype=np.int64) * deg
    ix = np.tile(np.arange(deg, dtype=np.int64), copies)            # position j holds node j: the pick says where it came from
    d_ip, d_ix = _to_gpu(torch, ip, ix)
    g = NeighborSampler([1]).make_graph(d_ip, d_ix, edata={"w": torch.full((copies * deg,), 0.25, device="cuda")})
    _, _, (b,) = NeighborSampler([f], seed=3, prob="w").sample(g, torch.arange(copies, device="cuda"))
    src, loc = b.src_nodes.cpu().numpy(), b.nbr.cpu().numpy()
    assert (loc >= 0).all()
    picks = src[loc]
    assert all(len(set(r)) == f for r in picks[:200].tolist())
    hits = np.bincount(picks.reshape(-1), minlength=deg) / copies
    p = f / deg
    assert np.all(np.abs(hits - p) <= 5 * np.sqrt(p * (1 - p) / copies))
    g.close()
    # four hubs of 10^6 equal-weight in-edges, 40 steps: the deciles of the chosen positions are flat
    H, nh, steps = 1_000_000, 4, 40
    ip = np.arange(nh + 1, dtype=np.int64) * H
    ix = np.tile(np.arange(H, dtype=np.int64), nh)
    d_ip, d_ix = _to_gpu(torch, ip, ix)
    g = NeighborSampler([1]).make_graph(d_ip, d_ix, edata={"w": torch.ones(nh * H, device="cuda")})
    smp = NeighborSampler([f], seed=8, prob="w")
    counts = np.zeros(10)
    for step in range(steps):
        _, _, (b,) = smp.sample(g, torch.arange(nh, device="cuda"), step=step)
        src, loc = b.src_nodes.cpu().numpy(), b.nbr.cpu().numpy()
        assert (loc >= 0).all()
        pos = src[loc]
        assert all(len(set(r)) == f for r in pos.tolist())
        counts += np.bincount(pos.reshape(-1) * 10 // H, minlength=10)
    n = nh * steps * f
    assert np.all(np.abs(counts - n / 10) <= 5 * np.sqrt(n * 0.1 * 0.9)), counts
    g.close()


# ------------------------------------------------------------------------------------------------ 3. invariance
def test_weighted_draw_is_deterministic_and_batch_independent(hiplib, hub_graph):
    import torch
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, ws, seeds, g = hub_graph
    smp = NeighborSampler([16], seed=12, prob="w16")
    d_seeds = torch.from_numpy(seeds).cuda()
    _, _, (a,) = smp.sample(g, d_seeds, step=4)
    _, _, (b,) = smp.sample(g, d_seeds, step=4)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        _, _, (c,) = smp.sample(g, d_seeds, step=4)
    st.synchronize()
    for x in (b, c):
        assert torch.equal(a.src_nodes, x.src_nodes) and torch.equal(a.nbr, x.nbr)

    def rows_of(blk):
        src = blk.src_nodes.cpu().numpy()
        loc = blk.nbr.cpu().numpy()
        return np.where(loc >= 0, src[np.maximum(loc, 0)], -1)

    full = dict(zip(seeds.tolist(), rows_of(a)))
    hub = len(ip) - 2
    rng = np.random.default_rng(6)
    plain = np.setdiff1d(np.arange(len(ip) - 1), seeds)
    for v in seeds[:: max(1, len(seeds) // 25)]:
        alone = rows_of(smp.sample(g, torch.tensor([v], device="cuda"), step=4)[2][0])[0]
        batch = np.concatenate([[v], rng.choice(plain, 999, replace=False)])
        in_batch = rows_of(smp.sample(g, torch.from_numpy(batch).cuda(), step=4)[2][0])[0]
        hubs = np.array([hub, v] if v != hub else [v], dtype=np.int64)
        by_hubs = rows_of(smp.sample(g, torch.from_numpy(hubs).cuda(), step=4)[2][0])[1 if len(hubs) > 1 else 0]
        assert np.array_equal(alone, full[int(v)]) and np.array_equal(in_batch, alone) and np.array_equal(by_hubs, alone), int(v)


def test_unit_weights_with_small_degrees_equal_the_uniform_sampler(hiplib):
    import torch
    from COALA_GNN.sampler import NeighborSampler
    rng = np.random.default_rng(5)
    n = 60_000
    ip, ix = csc_from_columns([rng.integers(0, n, size=rng.integers(0, 9)) for _ in range(n)])
    d_ip, d_ix = _to_gpu(torch, ip, ix)
    g = NeighborSampler([1]).make_graph(d_ip, d_ix, edata={"w": torch.ones(len(ix), device="cuda")})
    seeds = torch.from_numpy(rng.permutation(n)[:3000]).cuda()
    for fan in ([8], [8, 10], [16, 9, 8]):
        for G in (0, 3):
            _, _, bw = NeighborSampler(fan, seed=2, bucket_by_owner=G, prob="w").sample(g, seeds, step=7)
            _, _, bu = NeighborSampler(fan, seed=2, bucket_by_owner=G).sample(g, seeds, step=7)
            for x, y in zip(bw, bu):
                assert torch.equal(x.src_nodes, y.src_nodes) and torch.equal(x.nbr, y.nbr)
    g.close()


# ------------------------------------------------------------------------------------------------ 4. mixed lists, bucketing, limits
@pytest.mark.parametrize("fanouts", [[10, -1], [-1, 5]])
def test_mixed_lists_keep_every_edge_in_full_layers(hiplib, hub_graph, fanouts):
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, ws, seeds, g = hub_graph
    s = seeds[seeds != len(ip) - 2][:300]          # no hub: a full layer of it would be 10^6 edges per layer of the list
    w = ws["w5"]
    assert (w == 0).any()
    blocks, tol = _check_call(NeighborSampler(fanouts, seed=1, prob="w5"), g, ip, ix, w, s, 2)
    assert tol == 0
    full_block = blocks[fanouts.index(-1)]
    dst = full_block.src_nodes.cpu().numpy()[: full_block.num_dst]
    _, ind, loc = full_layer(ip, ix, dst)                            # zero-weight edges included
    assert np.array_equal(full_block.indptr.cpu().numpy(), ind) and np.array_equal(full_block.indices.cpu().numpy(), loc)


@pytest.mark.parametrize("G", [1, 3, 64])
def test_weighted_bucketing(hiplib, hub_graph, G):
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, ws, seeds, g = hub_graph
    for fanouts in ([5], [17, 5]):
        smp = NeighborSampler(fanouts, seed=3, bucket_by_owner=G, prob="w5")
        import torch
        _, _, blocks = smp.sample(g, torch.from_numpy(seeds).cuda(), step=1)
        ref = reference_layers(ip, ix, ws["w5"], seeds, list(reversed(fanouts)), 3, 1)
        src, _, loc, _ = ref[-1]
        want, sizes, new_of_old = bucketed(src, G)
        b0 = blocks[0]
        assert np.array_equal(b0.src_nodes.cpu().numpy(), want)
        assert b0.owner_counts.cpu().tolist() == b0.owner_counts_host == sizes.tolist()
        assert np.array_equal(b0.dst_in_src.cpu().numpy(), new_of_old[: b0.num_dst])
        assert np.array_equal(b0.nbr.cpu().numpy(), np.where(loc >= 0, new_of_old[np.maximum(loc, 0)], -1))


def test_weighted_layer_behind_a_full_layer_item_limit(hiplib):
    """Node 0 has LIMIT - 1 distinct in-neighbours: [-1] from it is exactly LIMIT items; a weighted fixed layer behind it would hold
    2 * LIMIT items and is refused at sample_end, naming layer 1, as for uniform layers.  The handle then samples exactly."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    ip = np.zeros(LIMIT + 1, dtype=np.int64)
    ip[1:] = LIMIT - 1
    ix = np.arange(1, LIMIT, dtype=np.int64)
    d_ip, d_ix = _to_gpu(torch, ip, ix)
    g = NeighborSampler([1]).make_graph(d_ip, d_ix, edata={"w": torch.ones(LIMIT - 1, device="cuda")})
    with pytest.raises(RuntimeError, match=f"layer 1 would hold {2 * LIMIT} items"):
        NeighborSampler([1, -1], prob="w").sample(g, torch.tensor([0], device="cuda"))
    inp, _, (b,) = NeighborSampler([3], seed=1, prob="w").sample(g, torch.tensor([0, 5], device="cuda"))
    got = inp.cpu().numpy()[b.nbr.cpu().numpy()[0]]
    from _weighted_ref import select
    want = select(ip, np.ones(LIMIT - 1, dtype=np.float32), np.array([0, 5]), 3, 1, 0, 0)[0] + 1
    assert np.array_equal(got, want) and (b.nbr.cpu().numpy()[1] == -1).all()
    g.close()


# ------------------------------------------------------------------------------------------------ 5. errors
def test_bad_weights_raise_before_any_launch(hiplib):
    import torch
    from COALA_GNN.sampler import NeighborSampler
    ip, ix = csc_from_columns([[1, 2], [0], [0, 1, 2]])
    d_ip, d_ix = _to_gpu(torch, ip, ix)
    bad = {"neg": [1.0, -1.0, 1.0, 1.0, 1.0, 1.0], "nan": [1.0, float("nan"), 1, 1, 1, 1], "inf": [float("inf"), 1, 1, 1, 1, 1],
           "short": [1.0] * 5}
    g = NeighborSampler([1]).make_graph(d_ip, d_ix, edata={k: torch.tensor(v, device="cuda") for k, v in bad.items()})
    seeds = torch.tensor([0, 2], device="cuda")
    for key in bad:
        smp = NeighborSampler([2], prob=key)
        with pytest.raises(ValueError, match=repr(key)):
            smp.sample(g, seeds)
        assert smp.step == 0
    with pytest.raises(KeyError):
        NeighborSampler([2], prob="absent").sample(g, seeds)
    g.edata["ok"] = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0, 2.0], device="cuda")
    _, _, (b,) = NeighborSampler([2], prob="ok").sample(g, seeds)
    src = b.src_nodes.cpu().numpy()
    loc = b.nbr.cpu().numpy()                                        # node 0: weights (1, 0); node 2: (0, 0, 2)
    assert loc[:, 1].tolist() == [-1, -1] and src[loc[:, 0]].tolist() == [1, 2]
    g.close()


# ------------------------------------------------------------------------------------------------ 6. end to end
def _assert_positive_edges(ip, ix, w, dst, picked):
    """every (dst, picked) pair has a positive-weight occurrence in dst's CSC column"""
    N = len(ip) - 1
    deg = np.diff(ip)
    rows = np.repeat(np.arange(N), deg)
    pos_pairs = np.unique(rows[w > 0] * N + ix[w > 0])
    pairs = np.unique(dst * N + picked)
    at = np.minimum(np.searchsorted(pos_pairs, pairs), len(pos_pairs) - 1)
    assert np.array_equal(pos_pairs[at], pairs), "a weight-0 edge (or a non-edge) appears in a block"


@pytest.mark.parametrize("model_type", ["sage", "gat"])
def test_loader_with_weighted_sampler(hiplib, tmp_path, model_type):
    import torch
    from _util import ColorFiles
    from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, SSD_INFO
    from COALA_GNN.harness import GAT, SageMean
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import alloc_pinned_table, block_colors, feature_rows_torch, powerlaw_csc
    torch.manual_seed(0)
    n_nodes, dim, batch, fan = 20000, 64, 64, [5, 5]
    table = alloc_pinned_table(n_nodes, dim, seed=3, device=0)
    indptr, indices = powerlaw_csc(n_nodes, 8.0, seed=1, device="cuda")
    ip, ix = indptr.cpu().numpy(), indices.cpu().numpy()
    rng = np.random.default_rng(4)
    w = (1.0 - rng.random(len(ix))).astype(np.float32)
    w[rng.random(len(ix)) < 0.3] = 0
    labels = (torch.arange(n_nodes, device="cuda") * 7) % 5
    color, tk, sc, _ = block_colors(n_nodes, nodes_per_color=512)
    files = ColorFiles(tmp_path, color, tk, sc)
    comm = MPI_Comm_Manager(0)
    comm.initialize_nested_process_group("isolated")
    train_ids = torch.randperm(int(0.6 * n_nodes), generator=torch.Generator().manual_seed(0))[:64 * 6]
    nd = Node_Distributor(comm, train_ids, batch, files.color_file, files.topk_file, files.score_file, parsing_method="baseline")
    sampler = NeighborSampler(fan, seed=5, prob="w")
    g = sampler.make_graph(indptr, indices, ndata={"labels": labels}, edata={"w": torch.from_numpy(w).cuda()})
    loader = COALA_GNN_DataLoader(SSD_INFO(1, dim * 4, 1024, 0), nd, g, sampler, batch, dim, fan, 4, "cuda:0", refresh_counter=3,
                                  cache_backend="isolated", sim_buf=table, num_rows=n_nodes, prefetch=1)
    model = (SageMean(dim, 32, 5, 2) if model_type == "sage" else GAT(dim, 16, 5, 2, 2)).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    steps = 0
    for input_nodes, seeds, blocks, feat in loader:
        assert torch.equal(feat, feature_rows_torch(input_nodes, dim, 3))
        for b in blocks:
            src = b.src_nodes.cpu().numpy()
            dst = b.dstdata["_ID"].cpu().numpy()
            loc = b.nbr.cpu().numpy()
            rows, cols = np.nonzero(loc >= 0)
            _assert_positive_edges(ip, ix, w, dst[rows], src[loc[rows, cols]])
        loss = torch.nn.functional.cross_entropy(model(blocks, feat), blocks[-1].dstdata["labels"].view(-1))
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert torch.isfinite(loss)
        steps += 1
    assert steps == 5
    del loader
    table.close()


def test_train_synthetic_with_random_edge_weights(hiplib):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), "--nodes", "60000", "--dim", "64", "--batch_size", "256",
           "--epochs", "1", "--cache_size", "4", "--prefetch", "1", "--fan_out", "10,5", "--edge_weights", "random"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    loss = re.search(r"final loss (\S+)", r.stdout)
    assert loss and math.isfinite(float(loss.group(1))) and "Test Acc" in r.stdout, r.stdout[-2000:]
