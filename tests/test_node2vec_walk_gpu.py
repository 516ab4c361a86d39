"""GPU tests of the second-order walks (COALA_GNN.sampler.node2vec_random_walk; node2vec_trace in coala_sampler.hip).

The rule is exact integer arithmetic, so the traces are compared bit for bit with the Python-integer restatement of
tests/_node2vec_ref.py (checked on its own, and against the exact node2vec transition probabilities, in test_node2vec_cpu.py).  The
graph is test_sampler_pinsage_gpu.py's: the degree edges, self-loops and repeated neighbours of _util.edge_case_graph, a node whose only
in-neighbour is itself, a 2-cycle, a sink and a node one hop above it, one node of in-degree 5,000 and 2,000 plain nodes -- with every
row sorted by source id, which the near test's binary search needs."""
import numpy as np
import pytest

import _node2vec_ref as R
from _util import csc_from_columns

pytestmark = pytest.mark.gpu

HUB = 5000
# (L, W, p, q): the smallest; the longest walk; the paper's two corners (1/16 acceptance for the far / the return class); 64 walks; p = 1
CASES = [(1, 1, 1, 1), (127, 1, 1, 1), (20, 10, 0.25, 4), (20, 10, 4, 0.25), (5, 64, 0.5, 2), (16, 3, 1, 2)]


@pytest.fixture(scope="module")
def walk_graph(hiplib):
    """-> (indptr, indices, graph on the device, start nodes, named nodes).  Start nodes: every special node, the named ones, duplicates,
    -1 and num_nodes, random plain nodes."""
    import torch
    from COALA_GNN.sampler import CSCGraph
    ip, ix, special, named, n0 = R.edge_graph(HUB)
    n = len(ip) - 1
    rng = np.random.default_rng(8)
    plain = np.setdiff1d(np.arange(n0), special)
    nodes = np.concatenate([special, list(named.values()), rng.choice(plain, 150, replace=False), special[:10], [-1, n, named["own"], n + 7]])
    nodes = nodes.astype(np.int64)
    rng.shuffle(nodes)
    g = CSCGraph(torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda())
    yield ip, ix, g, nodes, named
    g.close()


@pytest.mark.parametrize("L,W,p,q", CASES)
def test_traces_exact(walk_graph, L, W, p, q):
    import torch
    from COALA_GNN.sampler import node2vec_random_walk
    ip, ix, g, nodes, named = walk_graph
    seed, step = (3, 0) if W != 64 else (2**64 - 5, 2**64 - 1)
    got = node2vec_random_walk(g, torch.from_numpy(nodes).cuda(), p, q, L, num_walks=W, seed=seed, step=step)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(nodes), W, L + 1) and got.is_cuda
    want = R.traces(ip, ix, nodes, L, W, R.thresholds(p, q), seed, step)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), f"traces differ at L {L} W {W} p {p} q {q}: {int((got != want).any(-1).sum())} walks"
    at = {name: int(np.flatnonzero(nodes == v)[0]) for name, v in named.items()}
    n = len(ip) - 1
    assert np.all(got[at["own"]] == named["own"]) and np.all(got[at["sink"], :, 1:] == -1) and np.all(got[at["sink"], :, 0] == named["sink"])
    assert np.all(got[at["above"], :, 1] == named["sink"]) and np.all(got[at["above"], :, 2:] == -1)
    assert set(np.unique(got[at["a"]]).tolist()) <= {named["a"], named["b"]}
    assert np.all(got[(nodes < 0) | (nodes >= n)] == -1), "an out-of-range start node gives a row of -1"


def test_cap_path_through_the_c_entry(hiplib):
    """thr_far = 0 and thr_return = 0 on a star (ctypes: the Python wrapper refuses such thresholds): every hop after the first refuses
    256 attempts and takes attempt 255's candidate, as the reference does."""
    import torch
    from COALA_GNN.sampler import CSCGraph
    from COALA_GNN_Pybind import _capi, current_stream
    L_ = _capi.load()
    k = 9
    ip, ix = csc_from_columns([list(range(1, k + 1))] + [[0]] * k)
    g = CSCGraph(torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda())
    try:
        nodes = np.arange(k + 1, dtype=np.int64)
        d_nodes = torch.from_numpy(nodes).cuda()
        for thr in ((0, R.ONE, 0), (R.ONE, R.ONE, 0), (0, 1 << 31, R.ONE)):
            out = torch.full((k + 1, 3, 13), -7, dtype=torch.int64, device="cuda")
            _capi.check(L_.coala_sampler_node2vec_walk(g._h, d_nodes.data_ptr(), k + 1, 3, 12, *thr, 1, 2, out.data_ptr(), current_stream()))
            stats = {}
            want = R.traces(ip, ix, nodes, 12, 3, thr, 1, 2, stats=stats)
            assert np.array_equal(out.cpu().numpy(), want), f"thresholds {thr}"
            if thr[0] == 0 and thr[2] == 0:
                assert stats["capped"] == (k + 1) * 3 * 11
        # thresholds the entry refuses: the largest is not 2^32, or one is above it
        for bad in ((0, 0, 0), (R.ONE - 1, 5, 5), (R.ONE + 1, R.ONE, 0)):
            rc = L_.coala_sampler_node2vec_walk(g._h, d_nodes.data_ptr(), k + 1, 3, 12, *bad, 1, 2, out.data_ptr(), current_stream())
            assert rc == _capi.EINVAL and "thresholds" in _capi.last_error()
    finally:
        g.close()


def test_refusals_leave_the_handle_usable(walk_graph):
    import torch
    from COALA_GNN.sampler import CSCGraph, node2vec_random_walk, sort_csc_by_src
    ip, ix, g, nodes, named = walk_graph
    d_nodes = torch.from_numpy(nodes[:64]).cuda()
    want = R.traces(ip, ix, nodes[:64], 4, 2, R.thresholds(0.5, 2), 9, 1)

    def usable():
        assert np.array_equal(node2vec_random_walk(g, d_nodes, 0.5, 2, 4, num_walks=2, seed=9, step=1).cpu().numpy(), want)

    usable()
    for kwargs in (dict(p=0.2, q=4, walk_length=4), dict(p=1, q=17, walk_length=4), dict(p=1, q=1, walk_length=0), dict(p=1, q=1, walk_length=128),
                   dict(p=1, q=1, walk_length=4, num_walks=65), dict(p=1, q=1, walk_length=4, num_walks=0), dict(p=0, q=1, walk_length=4)):
        with pytest.raises(ValueError):
            node2vec_random_walk(g, d_nodes, **kwargs)
        usable()
    # an unsorted graph: refused at q != 1, walked at p = q = 1 (and at q = 1, p != 1: row prev is never read)
    rng = np.random.default_rng(1)
    ux = np.concatenate([rng.permutation(ix[ip[v]: ip[v + 1]]) for v in range(len(ip) - 1)]).astype(np.int64)
    assert not np.array_equal(ux, ix)
    gu = CSCGraph(torch.from_numpy(ip).cuda(), torch.from_numpy(ux).cuda())
    try:
        for _ in range(2):
            with pytest.raises(ValueError, match="sort_csc_by_src"):
                node2vec_random_walk(gu, d_nodes, 1, 2, 4)
        for p in (1, 0.5):
            got = node2vec_random_walk(gu, d_nodes, p, 1, 6, num_walks=2, seed=4).cpu().numpy()
            assert np.array_equal(got, R.traces(ip, ux, nodes[:64], 6, 2, R.thresholds(p, 1), 4, 0))
        # sort_csc_by_src puts it right: stable, a permutation, and the walks are the sorted graph's
        sx, perm = sort_csc_by_src(gu.indptr, gu.indices)
        assert np.array_equal(sx.cpu().numpy(), ix) and np.array_equal(ux[perm.cpu().numpy()], ix)
        pn = perm.cpu().numpy()
        for v in (named["hub"], 5):
            seg, vals = pn[ip[v]: ip[v + 1]], ix[ip[v]: ip[v + 1]]
            assert np.all((np.diff(seg) > 0) | (np.diff(vals) > 0)), "equal sources keep their CSC order"
    finally:
        gu.close()


def test_walks_do_not_depend_on_the_batch(walk_graph):
    import torch
    from COALA_GNN.sampler import node2vec_random_walk
    ip, ix, g, nodes, named = walk_graph
    rng = np.random.default_rng(2)
    big = rng.integers(0, len(ip) - 1, size=1000).astype(np.int64)
    picks = [0, 17, 500, 999]
    for v in (named["hub"], named["a"]):
        big[picks[1]] = v
        batch = node2vec_random_walk(g, torch.from_numpy(big).cuda(), 0.25, 4, 20, num_walks=10, seed=6, step=3)
        for i in picks:
            alone = node2vec_random_walk(g, torch.from_numpy(big[i: i + 1]).cuda(), 0.25, 4, 20, num_walks=10, seed=6, step=3)
            assert torch.equal(alone[0], batch[i])


@pytest.mark.parametrize("p,q", [(0.25, 4), (4, 0.25), (2, 0.5)])
def test_traces_exact_on_a_symmetric_graph(hiplib, p, q):
    """Planted communities, symmetrised: no walk ends, and all three classes -- return, near (triangles), far -- occur at every hop."""
    import torch
    from COALA_GNN.sampler import CSCGraph, node2vec_random_walk
    from COALA_GNN.synthetic import community_csc, symmetrize_csc
    ip_t, ix_t = symmetrize_csc(*community_csc(600, 8, community=64, seed=3, device="cuda"))
    g = CSCGraph(ip_t, ix_t)
    try:
        ip, ix = ip_t.cpu().numpy(), ix_t.cpu().numpy()
        keep = np.flatnonzero(np.diff(ip) > 0)[:200].astype(np.int64)
        got = node2vec_random_walk(g, torch.from_numpy(keep).cuda(), p, q, 20, num_walks=4, seed=7, step=5).cpu().numpy()
        G = R.Graph(ip, ix)
        want = R.traces(G, None, keep, 20, 4, R.thresholds(p, q), 7, 5)
        assert np.array_equal(got, want) and np.all(got >= 0)
        flat = got.reshape(-1, 21)
        a, b, c = flat[:, :-2].reshape(-1), flat[:, 1:-1].reshape(-1), flat[:, 2:].reshape(-1)
        near = np.array([x in G.row_set(u) for u, x in zip(a.tolist(), c.tolist())])
        assert (c == a).any() and (near & (c != a)).any() and (~near & (c != a)).any(), "a class never occurred"
    finally:
        g.close()
