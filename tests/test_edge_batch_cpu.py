"""CPU tests of the link-prediction pieces: the numpy restatement (_edge_batch_ref) against brute force and its own statistics, the
torch fallbacks (Block.exclude_edges_torch, block_ops.pair_dot_torch) on hand-made blocks, reverse_edge_ids, and the new C symbols.
No kernel is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import _edge_batch_ref as R
from _util import edge_case_graph


@pytest.fixture(scope="module")
def graph():
    ip, ix, _ = edge_case_graph([1, 5, 32], n_plain=200, hub_degree=300, seed=3)
    ip, ix, _ = R.with_zero_runs(ip, ix, runs=(3, 4, 5))
    return ip, ix


def test_endpoints_agree_with_brute_force(graph):
    ip, ix = graph
    E = len(ix)
    assert ip[1] == 0 and ip[-1] == ip[-2] == ip[-6] and np.any(np.diff(ip)[10:-10] == 0)     # degree-0 runs at both ends and inside
    eids = np.arange(E)
    src, dst = R.endpoints(ip, ix, eids)
    assert np.array_equal(dst, R.brute_force_rows(ip)) and np.array_equal(src, ix)
    assert np.all((ip[dst] <= eids) & (eids < ip[dst + 1]))
    src, dst = R.endpoints(ip, ix, [-1, E, 0, E - 1, 2**40])
    assert list(src[[0, 1, 4]]) == [-1] * 3 and list(dst[[0, 1, 4]]) == [-1] * 3
    assert dst[2] == np.flatnonzero(np.diff(ip))[0] and dst[3] == np.flatnonzero(np.diff(ip))[-1]


def test_negative_stream_constant_is_its_own():
    assert R.K_NEG not in R.K_OTHERS and len(set(R.K_OTHERS)) == 3


def test_negatives_range_permutation_steps():
    N = 2501
    eids = np.random.default_rng(0).integers(0, 10**6, size=300)
    a = R.negatives(N, eids, 5, seed=7, step=3)
    assert a.min() >= 0 and a.max() < N
    perm = np.random.default_rng(1).permutation(len(eids))
    assert np.array_equal(R.negatives(N, eids[perm], 5, seed=7, step=3), a[perm])      # a function of (seed, step, e, j) alone
    assert np.array_equal(R.negatives(N, eids[:10], 64, seed=7, step=3)[:, :5], a[:10])  # ... whatever k is
    b = R.negatives(N, eids, 5, seed=7, step=4)
    assert (a != b).mean() > 0.99
    assert (a != R.negatives(N, eids, 5, seed=8, step=3)).mean() > 0.99


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_negatives_chi_square(seed):
    N, n, k = 2501, 4096, 16
    neg = R.negatives(N, np.arange(n) * 3 + seed, k, seed=seed, step=seed + 1).reshape(-1)
    bins = neg * 64 // N
    expected = np.bincount(np.arange(N) * 64 // N, minlength=64) * (len(neg) / N)
    chi2 = float((((np.bincount(bins, minlength=64) - expected) ** 2) / expected).sum())
    print(f"chi-square over 64 bins, {len(neg)} draws: {chi2:.1f} (bound {R.CHI2_63_BOUND})")
    assert chi2 < R.CHI2_63_BOUND


def test_compaction_first_appearance(graph):
    ip, ix = graph
    nodes, local = R.compact([5, 3, 5, -1, 9, 3, 0])
    assert list(nodes) == [5, 3, 9, 0] and list(local) == [0, 1, 0, -1, 2, 1, 3]
    E = len(ix)
    ref = R.edge_batch(ip, ix, [0, E - 1, 7, 7, E, -1], 2, seed=1, step=0)
    assert ref["n_bad"] == 2 and np.all(ref["pos_src"][4:] == -1) and np.all(ref["neg_dst"][4:] == -1)
    assert len(np.unique(ref["seed_nodes"])) == len(ref["seed_nodes"])
    src, dst = R.endpoints(ip, ix, [0, E - 1, 7, 7])
    assert np.array_equal(ref["seed_nodes"][ref["pos_src"][:4]], src) and np.array_equal(ref["seed_nodes"][ref["pos_dst"][:4]], dst)
    assert ref["seed_nodes"][0] == src[0]


# --------------------------------------------------------------------------------------------------------- torch fallbacks
def _fixed_block(hiplib):
    from COALA_GNN.sampler import Block
    nbr = torch.tensor([[1, 2, 3], [4, -1, -1], [0, 5, -1], [-1, -1, -1]], dtype=torch.int32)
    eid = torch.tensor([[10, 11, 12], [20, -1, -1], [30, 31, -1], [-1, -1, -1]], dtype=torch.int64)
    return Block(torch.arange(100, 106), nbr, 4, eid=eid), nbr.numpy(), eid.numpy()


def _ragged_block(hiplib, lazy=False):
    from COALA_GNN.sampler import Block
    indptr = torch.tensor([0, 3, 4, 6, 6], dtype=torch.int64)
    indices = torch.tensor([1, 2, 3, 4, 0, 5], dtype=torch.int32)
    eid = torch.tensor([10, 11, 12, 20, 30, 31], dtype=torch.int64)

    def edge_weights():
        deg = indptr[1:] - indptr[:-1]
        return torch.repeat_interleave(1.0 / deg.to(torch.float32), deg)
    b = Block(torch.arange(100, 106), None, 4, indptr=indptr, indices=indices, eid=eid, edata_lazy={"edge_weights": edge_weights} if lazy else None)
    return b, indptr.numpy(), indices.numpy(), eid.numpy()


@pytest.mark.parametrize("excluded", [[], [11], [10, 11, 12], [20, 31], [5, 13, 999], [10, 12, 20, 30, 31]])
def test_exclude_edges_torch(hiplib, excluded):
    ex = torch.tensor(sorted(excluded), dtype=torch.int64)
    b, nbr, eid = _fixed_block(hiplib)
    got = b.exclude_edges_torch(ex)
    want_n, want_e = R.exclude_fixed(nbr, eid, np.array(excluded, dtype=np.int64))
    assert np.array_equal(got.nbr.numpy(), want_n) and np.array_equal(got.edata["_ID"].numpy(), want_e)
    assert got.src_nodes is b.src_nodes and got.num_dst == 4 and got.nbr.dtype == torch.int32
    valid = got.nbr.numpy() >= 0
    assert not np.any(valid[:, 1:] & ~valid[:, :-1])                      # valid entries first
    if set(excluded).isdisjoint(eid.reshape(-1).tolist()):
        assert np.array_equal(got.nbr.numpy(), nbr)                       # ids that are not in the block change nothing
    if excluded == [10, 11, 12]:
        assert np.all(got.nbr.numpy()[0] == -1)                           # an emptied row
    r, ip, ix, re = _ragged_block(hiplib)
    got = r.exclude_edges_torch(ex)
    wp, wi, we = R.exclude_csr(ip, ix, re, np.array(excluded, dtype=np.int64))
    assert np.array_equal(got.indptr.numpy(), wp) and np.array_equal(got.indices.numpy(), wi) and np.array_equal(got.edata["_ID"].numpy(), we)
    assert got.indices.dtype == torch.int32 and got.indptr.dtype == torch.int64
    h = torch.arange(12.0).view(6, 2)
    assert torch.equal(got.mean_aggregate(h), got.mean_aggregate_torch(h))


def test_exclude_edges_per_edge_data(hiplib):
    from types import SimpleNamespace
    from COALA_GNN.sampler import Block
    r, ip, ix, re = _ragged_block(hiplib, lazy=True)
    got = r.exclude_edges_torch(torch.tensor([11, 20], dtype=torch.int64))
    assert np.allclose(got.edata["edge_weights"].numpy(), [0.5, 0.5, 0.5, 0.5])         # 1 / surviving in-degree: rows of 2, 0, 2, 0
    assert got.edata["edge_weights"].shape == got.indices.shape
    # graph edata is gathered through the new '_ID'
    g = SimpleNamespace(edata={"w": torch.arange(100.0)}, ndata={})
    b = Block(torch.arange(100, 106), torch.tensor([[1, 2, 3]], dtype=torch.int32), 1, eid=torch.tensor([[10, 11, 12]]), edata_graph=g)
    got = b.exclude_edges_torch(torch.tensor([11], dtype=torch.int64))
    assert got.edata["w"].tolist() == [[10.0, 12.0, 0.0]]
    # a materialised entry was made for the old edges: refused
    b.edata["w"]
    with pytest.raises(RuntimeError, match="edata already holds"):
        b.exclude_edges(torch.tensor([11], dtype=torch.int64))
    # no edge ids: refused
    with pytest.raises(ValueError, match="edge ids"):
        Block(torch.arange(3), torch.tensor([[1, 2]], dtype=torch.int32), 1).exclude_edges(torch.tensor([1], dtype=torch.int64))


def test_pair_dot_torch(hiplib):
    from COALA_GNN.block_ops import pair_dot, pair_dot_torch
    rng = np.random.default_rng(0)
    h = torch.from_numpy(rng.standard_normal((7, 5)))
    src, dst = torch.tensor([0, 3, 3, -1, 6, 2]), torch.tensor([1, 3, 3, 2, -1, 6])
    want = np.array([float(h[s] @ h[d]) if s >= 0 and d >= 0 else 0.0 for s, d in zip(src.tolist(), dst.tolist())])
    for fn in (pair_dot, pair_dot_torch):       # on the CPU pair_dot is its fallback
        assert np.allclose(fn(h, src, dst).numpy(), want, rtol=0, atol=1e-14)
    h3 = torch.from_numpy(rng.standard_normal((7, 2, 3))).requires_grad_()
    out = pair_dot(h3, src, dst)
    assert tuple(out.shape) == (6, 2)
    assert np.allclose(out[1].detach().numpy(), (h3[3] * h3[3]).sum(-1).detach().numpy())
    out.sum().backward()
    assert torch.all(h3.grad[4] == 0) and torch.all(h3.grad[5] == 0)                     # unreferenced rows
    assert torch.allclose(h3.grad[0], h3[1].detach()) and torch.allclose(h3.grad[3], 4 * h3[3].detach())
    assert pair_dot(h, src[:0], dst[:0]).shape == (0,)
    with pytest.raises(IndexError):
        pair_dot(h, torch.tensor([7]), torch.tensor([0]))
    with pytest.raises(ValueError):
        pair_dot(h, torch.tensor([1.0]), torch.tensor([0]))


def test_reverse_edge_ids(hiplib):
    from COALA_GNN.sampler import reverse_edge_ids
    ip, ix = R.symmetric_graph(300, 6, seed=2)
    rev = reverse_edge_ids(torch.from_numpy(ip), torch.from_numpy(ix)).numpy()
    dst = R.brute_force_rows(ip)
    assert np.array_equal(ix[rev], dst) and np.array_equal(dst[rev], ix) and np.array_equal(rev[rev], np.arange(len(ix)))
    ip2, ix2 = R.csc_from_columns([[1], [0, 0]])                 # a repeated neighbour
    with pytest.raises(ValueError, match="simple"):
        reverse_edge_ids(torch.from_numpy(ip2), torch.from_numpy(ix2))
    ip3, ix3 = R.csc_from_columns([[1, 2], [0], []])             # 2 -> 0 has no reverse
    with pytest.raises(ValueError, match="symmetric"):
        reverse_edge_ids(torch.from_numpy(ip3), torch.from_numpy(ix3))


def test_wrapper_arguments(hiplib):
    from COALA_GNN import sampler as S
    with pytest.raises(ValueError):
        S.UniformNegativeSampler(65)
    with pytest.raises(ValueError):
        S.EdgePredictionSampler(S.NeighborSampler([5]), exclude="reverse_id")
    with pytest.raises(ValueError):
        S.EdgePredictionSampler(S.RandomWalkNeighborSampler(3, 2, 0.5, 4), exclude="self")
    inner = S.LaborSampler([5, 5], bucket_by_owner=4)
    w = S.as_edge_prediction_sampler(inner, exclude="self", negative_sampler=S.UniformNegativeSampler(5))
    assert inner.edge_ids and w.bucket_by_owner == 4 and w.num_neg == 5 and w.fanouts == [5, 5, 6] and w.stream_safe and w.completes_on_host


def test_symbols_and_abi(hiplib):
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    for name in ("coala_sampler_edge_batch", "coala_sampler_edge_batch_wait", "coala_block_exclude_edges", "coala_block_exclude_edges_csr",
                 "coala_block_pair_dot", "coala_block_pair_dot_backward"):
        assert name in _capi.SYMBOLS and getattr(L, name) is not None
    assert L.coala_abi_version() == 4
    # argument checks that need no device: refused before anything is launched
    assert L.coala_sampler_edge_batch(None, None, 0, 0, 0, 0, None, None, None) == _capi.EINVAL
    assert L.coala_block_pair_dot(0, None, None, None, None, 5, 0, 8, None) == _capi.EINVAL and "pair shape" in _capi.last_error()
    assert L.coala_block_pair_dot(0, None, None, None, None, 0, 1, 8, None) == _capi.OK
    assert L.coala_block_exclude_edges(0, None, None, None, 0, None, None, 4, 33, None) == _capi.EINVAL
    assert L.coala_block_exclude_edges(0, None, None, None, 0, None, None, 4, 5, None) == _capi.EINVAL and "null buffer" in _capi.last_error()
    assert L.coala_block_exclude_edges_csr(0, None, None, None, None, 0, None, None, None, None, 0, None) == _capi.OK
    assert C.sizeof(_capi.EdgeBatchOut) == 32
