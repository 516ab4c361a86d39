"""GPU tests of the edge-batch kernels (coala_sampler_edge_batch / _wait): seed edges -> endpoints, negative pairs and the compacted
seed-node list, bit for bit against the numpy restatement (tests/_edge_batch_ref.py), at the C ABI with sentinel-padded buffers."""
import ctypes as C

import numpy as np
import pytest

import _edge_batch_ref as R

pytestmark = pytest.mark.gpu

PAD = 37            # sentinel entries in front of and behind every output
S64, S32 = -0x0123456789ABCDEF, -0x01234567


@pytest.fixture(scope="module")
def setup(hiplib):
    import torch
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, hub = R.link_graph(n_plain=2000, hub_degree=5000, seed=5)
    deg = np.diff(ip)
    assert deg[hub] == 5000 and deg[0] == 0 and deg[-1] == 0
    g = NeighborSampler([1]).make_graph(torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda())
    rows = R.brute_force_rows(ip)
    E = len(ix)
    behind = np.flatnonzero((deg[1:] > 0) & (deg[:-1] == 0)) + 1             # rows right behind a degree-0 run
    loops = np.flatnonzero(ix == rows)
    key = rows * len(deg) + ix
    uk, first, cnt = np.unique(key, return_index=True, return_counts=True)
    twin = np.flatnonzero(key == uk[np.argmax(cnt)])[:2]                     # two edges with both endpoints in common
    assert len(loops) and cnt.max() >= 2 and len(behind) >= 4
    special = [0, E - 1, ip[hub], ip[hub + 1] - 1, loops[0], twin[0], twin[1], 7, 7]
    for v in list(behind[:3]) + [behind[-1]]:
        special += [ip[v], ip[v + 1] - 1]
    yield torch, g, ip, ix, np.array(special, dtype=np.int64)
    g.close()


def _eids(ip, ix, special, n, seed=0):
    rng = np.random.default_rng(seed)
    e = np.concatenate([special, rng.integers(0, len(ix), size=max(n - len(special), 0))])[:n]
    if n > len(special):
        e[-1] = e[-2]              # a repeated eid among the random ones as well
    return e.astype(np.int64)


def _call(torch, g, eids, k, seed, step):
    """The C ABI on sentinel-padded buffers -> dict as _edge_batch_ref.edge_batch gives it, after checking the padding."""
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    n = len(eids)
    d_e = torch.from_numpy(eids).cuda()
    sizes = (n * (2 + k), n, n, n * k)
    bufs = [torch.full((m + 2 * PAD,), s, dtype=dt, device="cuda")
            for m, dt, s in zip(sizes, (torch.int64, torch.int32, torch.int32, torch.int32), (S64, S32, S32, S32))]
    out = _capi.EdgeBatchOut(*[b.data_ptr() + PAD * b.element_size() for b in bufs])
    ticket = C.c_int64(-1)
    _capi.check(L.coala_sampler_edge_batch(g._h, d_e.data_ptr(), n, k, seed, step, C.byref(out), C.byref(ticket), current_stream()))
    n_nodes, n_bad = C.c_int64(-1), C.c_int64(-1)
    _capi.check(L.coala_sampler_edge_batch_wait(g._h, ticket.value, C.byref(n_nodes), C.byref(n_bad)))
    host = [b.cpu().numpy() for b in bufs]
    for h, m, s in zip(host, sizes, (S64, S32, S32, S32)):
        assert np.all(h[:PAD] == s) and np.all(h[PAD + m:] == s), "a write outside an output's capacity"
    assert np.all(host[0][PAD + n_nodes.value: PAD + sizes[0]] == S64), "seed_nodes written past n_nodes"
    return dict(seed_nodes=host[0][PAD: PAD + n_nodes.value], pos_src=host[1][PAD: PAD + n], pos_dst=host[2][PAD: PAD + n],
                neg_dst=host[3][PAD: PAD + n * k].reshape(n, k), n_bad=n_bad.value)


def _same(got, want):
    for key in ("seed_nodes", "pos_src", "pos_dst", "neg_dst"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert got["n_bad"] == want["n_bad"]


@pytest.mark.parametrize("k", [0, 1, 5, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024])
def test_edge_batch_bitwise(setup, n, k):
    torch, g, ip, ix, special = setup
    eids = _eids(ip, ix, special, n, seed=n + k)
    got = _call(torch, g, eids, k, seed=11, step=3)
    want = R.edge_batch(ip, ix, eids, k, seed=11, step=3)
    _same(got, want)
    assert want["n_bad"] == 0 and len(np.unique(got["seed_nodes"])) == len(got["seed_nodes"])
    _same(_call(torch, g, eids, k, seed=11, step=3), want)                   # the same call twice
    other = _call(torch, g, eids, k, seed=11, step=4)
    _same(other, R.edge_batch(ip, ix, eids, k, seed=11, step=4))
    assert np.array_equal(other["pos_src"], got["pos_src"])                  # the positives do not depend on the step
    if n * k >= 64:
        neg_a, neg_b = got["seed_nodes"][got["neg_dst"]], other["seed_nodes"][other["neg_dst"]]
        assert (neg_a != neg_b).mean() > 0.9                                 # ... the negatives do


def test_bad_edges_raise_and_the_handle_stays_usable(setup):
    torch, g, ip, ix, special = setup
    from COALA_GNN.sampler import edge_batch, edge_batch_wait
    E = len(ix)
    eids = _eids(ip, ix, special, 65, seed=1)
    bad = eids.copy()
    bad[[3, 40]] = [-1, E]
    got = _call(torch, g, bad, 5, seed=2, step=0)
    _same(got, R.edge_batch(ip, ix, bad, 5, seed=2, step=0))
    assert got["n_bad"] == 2 and np.all(got["neg_dst"][[3, 40]] == -1) and got["pos_dst"][40] == -1
    with pytest.raises(IndexError, match="2 of the 65 seed edges"):
        edge_batch_wait(edge_batch(g, torch.from_numpy(bad).cuda(), 5, seed=2, step=0))
    b = edge_batch_wait(edge_batch(g, torch.from_numpy(eids).cuda(), 5, seed=2, step=0))
    want = R.edge_batch(ip, ix, eids, 5, seed=2, step=0)
    assert np.array_equal(b.seed_nodes.cpu().numpy(), want["seed_nodes"]) and np.array_equal(b.neg_dst.cpu().numpy(), want["neg_dst"].reshape(-1))
    assert np.array_equal(b.neg_src.cpu().numpy(), np.repeat(want["pos_src"], 5)) and b.neg_src.dtype == torch.int32
    with pytest.raises(ValueError, match="over the limit"):
        edge_batch(g, torch.zeros(200000, dtype=torch.int64, device="cuda"), 64)
    # a ticket is collected by the call that matches it
    from COALA_GNN_Pybind import _capi
    pend = edge_batch(g, torch.from_numpy(eids).cuda(), 1)
    cnt = (C.c_int64 * 1)()
    assert _capi.load().coala_sampler_wait(g._h, pend[-1], cnt, None) == _capi.EINVAL
    edge_batch_wait(pend)


def test_interleaved_with_node_samples_on_one_handle(setup):
    """Edge batches share the handle's hash table, scan state and count ring with the node samples: a random sequence of both, every
    size transition among them, each edge batch against the restatement and each node sample against a handle that never saw an edge
    batch."""
    torch, g, ip, ix, special = setup
    from COALA_GNN.sampler import LaborSampler, NeighborSampler
    rng = np.random.default_rng(99)
    clean = NeighborSampler([1]).make_graph(g.indptr, g.indices)
    N = len(ip) - 1
    sizes = [1, 1024, 3, 65, 5000, 64, 300, 2, 1500, 63, 4000, 1]
    fans = [[5, 5], [-1, 2], [32], [2, -1], [3, 3, 3]]
    try:
        for i, n in enumerate(sizes):
            k = int(rng.choice([0, 1, 5, 64]))
            m = min(n, 1024)
            eids = _eids(ip, ix, special, m, seed=100 + i)
            _same(_call(torch, g, eids, k, seed=5, step=i), R.edge_batch(ip, ix, eids, k, seed=5, step=i))
            seeds = torch.from_numpy(rng.permutation(N)[:n].astype(np.int64)).cuda()
            cls = LaborSampler if i % 4 == 3 else NeighborSampler
            f = [5, 5] if cls is LaborSampler else fans[i % len(fans)]
            a = cls(f, seed=3, bucket_by_owner=4 if i % 3 == 0 else 0).sample(g, seeds, step=i)
            b = cls(f, seed=3, bucket_by_owner=4 if i % 3 == 0 else 0).sample(clean, seeds, step=i)
            assert torch.equal(a[0], b[0])
            for x, y in zip(a[2], b[2]):
                assert torch.equal(x.src_nodes, y.src_nodes)
                for t, u in ((x.nbr, y.nbr), (x.indptr, y.indptr), (x.indices, y.indices)):
                    assert (t is None) == (u is None) and (t is None or torch.equal(t, u))
    finally:
        clean.close()
