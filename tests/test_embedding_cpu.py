"""CPU tests of the trainable node embeddings (COALA_GNN/embedding.py): the new C symbols, the torch backend of NodeEmbedding under
SparseAdagrad / SparseSGD against nn.Embedding(sparse=True) with torch.optim.Adagrad and against the float64 one-step reference
(tests/_embedding_ref.py), the reduce rules, last-wins writes and the refusals of the Python layer."""
import numpy as np
import pytest
import torch

from _embedding_ref import check_add, check_adagrad, make_grad

LR, EPS = 0.05, 1e-10


def test_write_symbols_resolve_and_the_abi_version_stays(hiplib):
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    for name in ("coala_cache_write_rows", "coala_cache_adagrad_rows"):
        assert name in _capi.SYMBOLS and getattr(L, name) is not None
    assert L.coala_abi_version() == 4
    assert hasattr(hiplib.Isolated_Cache, "write_rows") and hasattr(hiplib.Isolated_Cache, "adagrad_rows")
    if hiplib.native is not None:
        assert hasattr(hiplib.native, "cache_write_rows") and hasattr(hiplib.native, "cache_adagrad_rows")
    # refused before anything touches a device: a null handle
    assert L.coala_cache_write_rows(None, None, 0, None, 0, 1.0, None) == _capi.EINVAL and "null handle" in _capi.last_error()
    assert L.coala_cache_adagrad_rows(None, None, 0, None, None, 0.1, 1e-10, None) == _capi.EINVAL


def _ids_with_pairs(rng, num_rows, n_single, n_twice):
    """Distinct ids, n_twice of them listed twice (the fp32 sum of two gradient rows does not depend on the order), shuffled."""
    ids = rng.choice(num_rows, size=n_single + n_twice, replace=False)
    return rng.permutation(np.concatenate([ids, ids[:n_twice]])).astype(np.int64)


def _reduced(ids, coef):
    """fp32 sum of the rows of coef per distinct id (every id occurs at most twice) -> (uniq, g, counts)."""
    uniq, first, cnt = np.unique(ids, return_index=True, return_counts=True)
    g = coef[first].copy()
    for k in np.flatnonzero(cnt == 2):
        a, b = np.flatnonzero(ids == uniq[k])
        g[k] = coef[a] + coef[b]
    return uniq, g, cnt


def test_torch_backend_tracks_sparse_embedding_under_adagrad(hiplib):
    from COALA_GNN import NodeEmbedding, SparseAdagrad
    num_rows, dim = 500, 24
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    emb = NodeEmbedding(num_rows, dim, device="cpu", backend="torch")
    opt = SparseAdagrad([emb], lr=LR, eps=EPS, reduce="sum")
    ref = torch.nn.Embedding(num_rows, dim, sparse=True)
    with torch.no_grad():
        ref.weight.copy_(emb.weight)
    ropt = torch.optim.Adagrad(ref.parameters(), lr=LR, eps=EPS)
    never = np.ones(num_rows, dtype=bool)
    w_start = emb.weight.numpy().copy()
    for step in range(6):
        ids = _ids_with_pairs(rng, num_rows, 60, 25)
        never[ids] = False
        coef = make_grad(rng, (len(ids), dim))
        uniq, g, _ = _reduced(ids, coef)
        w0, s0 = emb.weight.numpy().copy(), opt.state_of(emb)[0].numpy().copy()
        r0 = ref.weight.detach().numpy().copy()
        rs0 = ropt.state[ref.weight]["sum"].numpy().copy() if ropt.state[ref.weight] else np.zeros_like(r0)
        t_ids, t_coef = torch.from_numpy(ids), torch.from_numpy(coef)
        opt.zero_grad()
        rows = emb(t_ids)
        assert rows.is_leaf and rows.requires_grad and len(emb.trace) == 1
        (rows * t_coef).sum().backward()
        opt.step()
        assert emb.trace == []
        ropt.zero_grad()
        (ref(t_ids) * t_coef).sum().backward()
        ropt.step()
        # each side within the bound of the float64 step from its OWN snapshot
        check_adagrad(emb.weight.numpy()[uniq], opt.state_of(emb)[0].numpy()[uniq], w0[uniq], s0[uniq], g, LR, EPS, f"ours, step {step}")
        check_adagrad(ref.weight.detach().numpy()[uniq], ropt.state[ref.weight]["sum"].numpy()[uniq], r0[uniq], rs0[uniq], g, LR, EPS,
                      f"torch.optim.Adagrad, step {step}")
        rest = np.ones(num_rows, dtype=bool)
        rest[uniq] = False
        assert emb.weight.numpy()[rest].tobytes() == w0[rest].tobytes()
    # ... and so the two stay together: six steps of at most a bound's worth of drift each
    assert np.allclose(emb.weight.numpy(), ref.weight.detach().numpy(), rtol=1e-5, atol=1e-6)
    assert emb.weight.numpy()[never].tobytes() == w_start[never].tobytes() and never.any()


def test_reduce_mean_divides_by_counts_and_sgd_adds(hiplib):
    from COALA_GNN import NodeEmbedding, SparseAdagrad, SparseSGD
    num_rows, dim = 200, 8
    rng = np.random.default_rng(1)
    for reduce in ("mean", "sum"):
        emb = NodeEmbedding(num_rows, dim, device="cpu", backend="torch", init_func=lambda t: t.normal_())
        ids = _ids_with_pairs(rng, num_rows, 30, 20)
        coef = make_grad(rng, (len(ids), dim))
        uniq, g, cnt = _reduced(ids, coef)
        if reduce == "mean":
            g = g / cnt.astype(np.float32)[:, None]
        w0 = emb.weight.numpy().copy()
        sgd = SparseSGD([emb], lr=0.25, reduce=reduce)
        (emb(torch.from_numpy(ids)) * torch.from_numpy(coef)).sum().backward()
        sgd.step()
        check_add(emb.weight.numpy()[uniq], w0[uniq], g, -0.25, f"sgd {reduce}")
        # the same ids looked up in two calls of one step: one trace entry each, reduced together
        ada = SparseAdagrad(emb, lr=LR, reduce=reduce)
        w0, s0 = emb.weight.numpy().copy(), ada.state_of(emb)[0].numpy().copy()
        half = len(ids) // 2
        a, b = emb(torch.from_numpy(ids[:half])), emb(torch.from_numpy(ids[half:]))
        ((a * torch.from_numpy(coef[:half])).sum() + (b * torch.from_numpy(coef[half:])).sum()).backward()
        assert len(emb.trace) == 2
        ada.step()
        check_adagrad(emb.weight.numpy()[uniq], ada.state_of(emb)[0].numpy()[uniq], w0[uniq], s0[uniq], g, LR, 1e-10, f"adagrad {reduce}")


def test_write_is_last_wins_and_read_is_untracked(hiplib):
    from COALA_GNN import NodeEmbedding
    emb = NodeEmbedding(50, 4, device="cpu", backend="torch", init_func=lambda t: torch.zeros_like(t))
    assert float(emb.weight.abs().sum()) == 0.0
    ids = torch.tensor([7, 3, 7, 9, 3, 7])
    rows = torch.arange(24, dtype=torch.float32).view(6, 4)
    emb.write(ids, rows)
    assert torch.equal(emb.read(torch.tensor([7, 3, 9])), rows[[5, 4, 3]])
    assert emb.trace == [] and float(emb.weight.abs().sum()) == float(rows[[5, 4, 3]].sum())
    assert emb.weight_host is emb.weight


def test_python_layer_refusals(hiplib):
    from COALA_GNN import NodeEmbedding, SparseAdagrad, SparseSGD
    with pytest.raises(ValueError, match="backend"):
        NodeEmbedding(10, 4, device="cpu", backend="dgl")
    with pytest.raises(ValueError, match="cuda device"):
        NodeEmbedding(10, 4, device="cpu", backend="native")
    with pytest.raises(ValueError, match="positive"):
        NodeEmbedding(0, 4, device="cpu", backend="torch")
    emb = NodeEmbedding(10, 4, device="cpu", backend="torch")
    with pytest.raises(ValueError, match="shape"):
        emb.write(torch.tensor([1, 2]), torch.zeros(3, 4))
    with pytest.raises(ValueError, match="shape"):
        emb.attach(torch.tensor([1, 2]), torch.zeros(2, 5))
    with pytest.raises(ValueError, match="reduce"):
        SparseAdagrad([emb], lr=0.1, reduce="max")
    with pytest.raises(ValueError, match="lr"):
        SparseSGD([emb], lr=0.0)
    with pytest.raises(TypeError):
        SparseSGD([torch.nn.Embedding(3, 3)], lr=0.1)

    class FakeManager:
        cache_backend, COALA_GNN_Cache, MPI_comm_manager, sim_buf, dim, device = "nccl", None, None, None, 4, "cpu"
    with pytest.raises(ValueError, match="isolated"):
        NodeEmbedding.from_manager(FakeManager())
    opt = SparseSGD([emb], lr=0.1)
    opt.step()                                   # nothing looked up: nothing to do
    leaf = emb.attach(torch.tensor([1, 2]), torch.ones(2, 4))
    assert leaf.requires_grad and len(emb.trace) == 1
    opt.zero_grad()
    assert emb.trace == []
