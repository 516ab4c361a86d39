"""GPU tests of the trainable node embeddings (COALA_GNN/embedding.py) on the native backend: sparse optimizer steps against the float64
one-step reference (tests/_embedding_ref.py), the line-equals-cold-row invariant behind every step, and a loader epoch in which the
loader's fetch is the embedding lookup (NodeEmbedding.from_manager + attach)."""
import numpy as np
import pytest

from _embedding_ref import check_add, check_adagrad, make_grad
from _util import ColorFiles

pytestmark = pytest.mark.gpu

LR, EPS = 0.05, 1e-10


def _ids_with_pairs(rng, num_rows, n_single, n_twice):
    """Distinct ids, n_twice of them listed twice (the fp32 sum of two gradient rows does not depend on the order), shuffled."""
    ids = rng.choice(num_rows, size=n_single + n_twice, replace=False)
    return rng.permutation(np.concatenate([ids, ids[:n_twice]])).astype(np.int64)


def _reduced(ids, coef, reduce):
    uniq, first, cnt = np.unique(ids, return_index=True, return_counts=True)
    g = coef[first].copy()
    for k in np.flatnonzero(cnt == 2):
        a, b = np.flatnonzero(ids == uniq[k])
        g[k] = coef[a] + coef[b]
    if reduce == "mean":
        g = g / cnt.astype(np.float32)[:, None]
    return uniq, g


@pytest.mark.parametrize("reduce", ["mean", "sum"])
@pytest.mark.parametrize("kind", ["adagrad", "adagrad-pinned-state", "sgd"])
def test_native_steps_match_the_one_step_reference(hiplib, kind, reduce):
    import torch
    from COALA_GNN import NodeEmbedding, SparseAdagrad, SparseSGD
    torch.cuda.set_device(0)
    num_rows, dim = 3000, 64          # 1 MiB of 128-float lines: 2048 of the 3000 rows fit, so lookups both hit and miss
    rng = np.random.default_rng(2)
    torch.manual_seed(1)
    emb = NodeEmbedding(num_rows, dim, cache_mb=1, device="cuda:0", backend="native")
    if kind == "sgd":
        opt = SparseSGD([emb], lr=LR, reduce=reduce)
    else:
        opt = SparseAdagrad([emb], lr=LR, eps=EPS, reduce=reduce, state_device_bytes=0 if kind.endswith("pinned-state") else 1 << 30)
        assert opt.state_of(emb)[0].is_cuda == (kind == "adagrad")
    w_start = emb.weight_host.numpy().copy()
    never = np.ones(num_rows, dtype=bool)
    for step in range(6):
        ids = _ids_with_pairs(rng, num_rows, 700, 150)
        never[ids] = False
        coef = make_grad(rng, (len(ids), dim))
        uniq, g = _reduced(ids, coef, reduce)
        torch.cuda.synchronize()
        w0 = emb.weight_host.numpy().copy()
        s0 = opt.state_of(emb)[0].cpu().numpy().copy() if kind != "sgd" else None
        d_ids = torch.from_numpy(ids).cuda()
        opt.zero_grad()
        rows = emb(d_ids)
        assert rows.is_leaf and rows.requires_grad and rows.detach().cpu().numpy().tobytes() == w0[ids].tobytes()
        (rows * torch.from_numpy(coef).cuda()).sum().backward()
        opt.step()
        torch.cuda.synchronize()
        w1 = emb.weight_host.numpy()
        if kind == "sgd":
            check_add(w1[uniq], w0[uniq], g, -LR, f"{kind} {reduce}, step {step}")
        else:
            check_adagrad(w1[uniq], opt.state_of(emb)[0].cpu().numpy()[uniq], w0[uniq], s0[uniq], g, LR, EPS, f"{kind} {reduce}, step {step}")
        rest = np.ones(num_rows, dtype=bool)
        rest[uniq] = False
        assert w1[rest].tobytes() == w0[rest].tobytes()
        # the invariant: whatever the cache holds of the stepped rows and of a random draw is what the table holds
        back = np.unique(np.concatenate([uniq, rng.choice(num_rows, size=500, replace=False)]))
        assert emb.read(torch.from_numpy(back)).cpu().numpy().tobytes() == emb.weight_host.numpy()[back].tobytes()
    hit, miss, bad = emb._cache.stats()
    assert hit > 0 and miss > 0 and bad == 0
    assert never.any() and emb.weight_host.numpy()[never].tobytes() == w_start[never].tobytes()
    emb.close()


def test_write_dedupes_last_wins_on_the_device(hiplib):
    import torch
    from COALA_GNN import NodeEmbedding
    torch.cuda.set_device(0)
    emb = NodeEmbedding(100, 8, cache_mb=1, device="cuda:0", backend="native", init_func=lambda t: t.zero_())
    emb.read(torch.arange(0, 100, 2))                       # half of the rows are cached
    ids = torch.tensor([7, 3, 7, 9, 3, 7, 8])
    rows = torch.arange(56, dtype=torch.float32).view(7, 8)
    emb.write(ids, rows)
    torch.cuda.synchronize()
    assert torch.equal(emb.weight_host[[7, 3, 9, 8]], rows[[5, 4, 3, 6]])
    assert torch.equal(emb.read(torch.tensor([8, 7, 3, 9])).cpu(), rows[[6, 5, 4, 3]])
    assert float(emb.weight_host.sum()) == float(rows[[5, 4, 3, 6]].sum())
    emb.close()


def test_loader_fetch_is_the_embedding_lookup(hiplib, tmp_path):
    import torch
    from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, NodeEmbedding, SparseAdagrad, SSD_INFO
    from COALA_GNN.harness import SAGE
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import PinnedFeatureTable, block_colors, powerlaw_csc
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    n_nodes, dim, batch, fan = 2000, 128, 64, [5, 5]
    table = PinnedFeatureTable(n_nodes, dim, 0)
    table.cpu_tensor.uniform_(-0.1, 0.1)
    w_start = table.array.copy()
    indptr, indices = powerlaw_csc(n_nodes, 8, seed=1, device="cuda")
    labels = (torch.arange(n_nodes, device="cuda") * 7) % 5
    color, tk, sc, _ = block_colors(n_nodes, nodes_per_color=512)
    files = ColorFiles(tmp_path, color, tk, sc)
    comm = MPI_Comm_Manager(0)
    comm.initialize_nested_process_group("isolated")
    train_ids = torch.randperm(int(0.6 * n_nodes), generator=torch.Generator().manual_seed(0))[:batch * 12]
    nd = Node_Distributor(comm, train_ids, batch, files.color_file, files.topk_file, files.score_file, parsing_method="baseline")
    sampler = NeighborSampler(fan, seed=5)
    g = sampler.make_graph(indptr, indices, ndata={"labels": labels})
    loader = COALA_GNN_DataLoader(SSD_INFO(1, dim * 4, 1024, 0), nd, g, sampler, batch, dim, fan, 1, "cuda:0", refresh_counter=3,
                                  cache_backend="isolated", sim_buf=table, num_rows=n_nodes, prefetch=0)
    emb = NodeEmbedding.from_manager(loader.COALA_GNN_Manager)
    assert (emb.num_rows, emb.dim) == (n_nodes, dim) and emb.weight_host is table.cpu_tensor
    model = SAGE(dim, 32, 5, 2, "mean").cuda()
    dense = torch.optim.Adam(model.parameters(), lr=1e-2)
    sparse = SparseAdagrad([emb], lr=0.05)
    fixed_in, fixed_seeds, fixed_blocks = NeighborSampler(fan, seed=9).sample(g, train_ids[:batch].cuda())
    fixed_labels = fixed_blocks[-1].dstdata["labels"].view(-1)

    def fixed_loss():
        with torch.no_grad():
            return float(torch.nn.functional.cross_entropy(model(fixed_blocks, emb.read(fixed_in)), fixed_labels))

    loss_before = fixed_loss()
    stepped = np.zeros(n_nodes, dtype=bool)
    steps = 0
    for input_nodes, seeds, blocks, feat in loader:
        stepped[input_nodes.cpu().numpy()] = True
        h = emb.attach(input_nodes, feat)
        assert h.is_leaf and h.data_ptr() == feat.data_ptr()
        loss = torch.nn.functional.cross_entropy(model(blocks, h), blocks[-1].dstdata["labels"].view(-1))
        dense.zero_grad()
        loss.backward()
        dense.step()
        sparse.step()
        assert emb.trace == []
        steps += 1
    assert steps == 11
    torch.cuda.synchronize()
    loss_after = fixed_loss()
    print(f"loss on the fixed batch: {loss_before:.4f} -> {loss_after:.4f}")
    assert loss_after < loss_before
    torch.cuda.synchronize()
    everything = torch.arange(n_nodes)
    assert emb.read(everything).cpu().numpy().tobytes() == table.array.tobytes()      # the invariant, over the whole table
    assert (~stepped).any() and stepped.any()
    assert table.array[~stepped].tobytes() == w_start[~stepped].tobytes()             # nodes never sampled keep their rows
    assert not np.array_equal(table.array[stepped], w_start[stepped])
    hit, miss, bad = loader.COALA_GNN_Manager.COALA_GNN_Cache.stats()
    assert hit > 0 and miss > 0 and bad == 0
    with pytest.raises(ValueError, match="isolated"):
        class Other:
            cache_backend, COALA_GNN_Cache = "nccl", loader.COALA_GNN_Manager.COALA_GNN_Cache
        NodeEmbedding.from_manager(Other())
    del loader
    table.close()
