"""CPU twin of test_item_batch_limits_gpu.py: the numpy-uint64 forms of the walk and edge-batch references (_node2vec_ref.traces_vec,
negatives_vec, walk_batch_vec; _edge_batch_ref.negatives_vec, large_graph) equal the Python-integer forms, which stay the definition, bit
for bit: on the GPU tests' graph of degree edges and on a symmetric graph, at the paper's two corners and p = q = 1, with out-of-range
start nodes, on the attempt-cap path, and under the existing fault injection."""
import numpy as np
import pytest

import _edge_batch_ref as E
import _node2vec_ref as R
from _util import csc_from_columns

# (L, W, p, q): the two corners (1/16 acceptance of the far / of the return class), and the open walk that takes attempt 0
SHAPES = [(20, 3, 0.25, 4), (20, 3, 4, 0.25), (5, 2, 1, 1)]


@pytest.fixture(scope="module")
def graphs():
    ip, ix, special, named, n0 = R.edge_graph(5000)
    n = len(ip) - 1
    rng = np.random.default_rng(21)
    nodes = np.concatenate([special, list(named.values()), rng.integers(0, n0, 120), special[:6], [-1, n, n + 7, -(1 << 40)]]).astype(np.int64)
    rng.shuffle(nodes)
    sp, sx = E.symmetric_graph(3001, 6, seed=4)
    snodes = np.concatenate([rng.integers(0, 3001, 150), [-1, 3001, 5, 5]]).astype(np.int64)
    return {"edge": (ip, ix, nodes, R.Graph(ip, ix)), "symmetric": (sp, sx, snodes, R.Graph(sp, sx))}


@pytest.mark.parametrize("which", ["edge", "symmetric"])
@pytest.mark.parametrize("L,W,p,q", SHAPES)
def test_traces_vec_equals_traces(graphs, which, L, W, p, q):
    ip, ix, nodes, G = graphs[which]
    thr = R.thresholds(p, q)
    want = R.traces(G, None, nodes, L, W, thr, seed=11, step=3)
    got = R.traces_vec(ip, ix, nodes, L, W, thr, seed=11, step=3)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    bad = (nodes < 0) | (nodes >= len(ip) - 1)
    assert bad.sum() >= 2 and np.all(got[bad] == -1)
    assert not np.array_equal(got, R.traces_vec(ip, ix, nodes, L, W, thr, seed=11, step=4)), "the step must matter"
    if which == "symmetric" and L == 20:
        flat = got[~bad].reshape(-1, L + 1)
        a, c = flat[:, :-2].reshape(-1), flat[:, 2:].reshape(-1)
        near = np.array([x in G.row_set(u) for u, x in zip(a.tolist(), c.tolist()) if x >= 0 and u >= 0])
        assert (c == a).any() and near.any() and (~near).any(), "a class never occurred: the near test checks nothing"


def test_cap_path_on_a_star():
    """thr_return = thr_far = 0 on a star, as test_cap_path_through_the_c_entry uses: every hop after the first runs into the attempt
    cap and takes attempt 255's candidate."""
    k = 9
    ip, ix = csc_from_columns([list(range(1, k + 1))] + [[0]] * k)
    nodes = np.arange(k + 1, dtype=np.int64)
    for thr in ((0, R.ONE, 0), (R.ONE, R.ONE, 0), (0, 1 << 31, R.ONE)):
        stats = {}
        want = R.traces(ip, ix, nodes, 12, 3, thr, 1, 2, stats=stats)
        assert np.array_equal(R.traces_vec(ip, ix, nodes, 12, 3, thr, 1, 2), want), f"thresholds {thr}"
        if thr[0] == 0 and thr[2] == 0:
            assert stats["capped"] == (k + 1) * 3 * 11


@pytest.mark.parametrize("which", ["edge", "symmetric"])
def test_swapped_classes_still_disagree(graphs, which):
    """The existing fault injection (return and near thresholds swapped) goes through the vectorised form unchanged, and still differs
    from the unswapped result."""
    ip, ix, nodes, G = graphs[which]
    thr = R.thresholds(0.25, 4)
    swapped = R.traces_vec(ip, ix, nodes, 20, 3, thr, seed=11, step=3, swap_classes=True)
    assert np.array_equal(swapped, R.traces(G, None, nodes, 20, 3, thr, seed=11, step=3, swap_classes=True))
    assert not np.array_equal(swapped, R.traces_vec(ip, ix, nodes, 20, 3, thr, seed=11, step=3))


def test_an_unsorted_row_is_refused():
    ip, ix = csc_from_columns([[2, 1], [0], [0]])
    with pytest.raises(AssertionError, match="sorted"):
        R.traces_vec(ip, ix, np.arange(3), 2, 1, R.thresholds(1, 2), 0, 0)


@pytest.mark.parametrize("which", ["edge", "symmetric"])
@pytest.mark.parametrize("L,W,K", [(6, 3, 1), (4, 2, 16), (2, 1, 0), (1, 64, 1)])
def test_walk_negatives_and_batch(graphs, which, L, W, K):
    ip, ix, nodes, G = graphs[which]
    nodes = nodes[:40].copy()
    nodes[[1, 20]] = [-1, len(ip) - 1]
    N = len(ip) - 1
    want = R.negatives(nodes, N, L, W, K, seed=5, step=7)
    got = R.negatives_vec(nodes, N, L, W, K, seed=5, step=7)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    thr = R.thresholds(0.5, 2)
    a, b = R.walk_batch_vec(ip, ix, nodes, L, W, K, thr, 5, 7), R.walk_batch(ip, ix, nodes, L, W, K, thr, 5, 7)
    for key in ("input_nodes", "pos", "neg", "traces"):
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), key
    assert a["n_bad"] == b["n_bad"] >= 2


@pytest.mark.parametrize("k", [0, 1, 5, 64])
def test_edge_negatives_vec(k):
    ip, ix, hub = E.link_graph(n_plain=2000, hub_degree=5000, seed=5)
    rng = np.random.default_rng(k)
    eids = np.concatenate([[0, len(ix) - 1, -1, len(ix), 7, 7, (1 << 62) + 5], rng.integers(0, len(ix), 2000)]).astype(np.int64)
    N = len(ip) - 1
    for seed, step in ((11, 3), (2**64 - 5, 2**64 - 1)):
        want, got = E.negatives(N, eids, k, seed, step), E.negatives_vec(N, eids, k, seed, step)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    a, b = E.edge_batch(ip, ix, eids, k, 11, 3), E.edge_batch(ip, ix, eids, k, 11, 3, draw=E.negatives_vec)
    for key in ("seed_nodes", "pos_src", "pos_dst", "neg_dst"):
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
    assert a["n_bad"] == b["n_bad"] == 3


def test_large_graph_is_what_the_gpu_tests_assume():
    ip, ix, hub, zeros = E.large_graph(30_011, 6, hub_degree=900, seed=2)
    N = len(ip) - 1
    deg = np.diff(ip)
    assert N == 30_011 and np.all(deg[zeros] == 0) and 900 <= deg[hub] <= 930 and ix.min() >= 0 and ix.max() < N
    assert 0 in zeros and N - 1 in zeros
    key = np.repeat(np.arange(N), deg) * N + ix
    assert np.all(np.diff(key) > 0), "rows sorted by source, no repeated edge"
    assert (deg == 0).sum() < 0.01 * N
