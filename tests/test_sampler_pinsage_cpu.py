"""CPU tests of the random-walk sampler's reference, tests/_pinsage_ref.py (no GPU): the vectorised and the Python-integer forms agree,
and the rule they state has the statistics it should have.  The seed is fixed (SEED below), so every test is deterministic; the bounds
are quantiles chosen before looking at what the rule gives."""
import numpy as np

from _pinsage_ref import compact_fixed, reference_layers, select, threshold, traces, traces_slow, walk_layer
from _util import csc_from_columns, edge_case_graph

SEED = 11


def _cycle_graph(n, deg):
    """Node v has in-neighbours v+1 .. v+deg (mod n): no sinks."""
    return csc_from_columns([[(v + 1 + j) % n for j in range(deg)] for v in range(n)])


def test_threshold_is_the_exact_floor():
    assert threshold(0.0) == 0 and threshold(0.5) == 1 << 52 and threshold(0.25) == 1 << 51
    p = 0.3
    assert threshold(p) == int(np.floor(np.float64(p) * np.float64(2.0**53))) < 1 << 53
    assert threshold(np.nextafter(1.0, 0.0)) == (1 << 53) - 1


def test_vectorised_and_slow_forms_agree():
    ip, ix, special = edge_case_graph([1, 3, 5], n_plain=150, hub_degree=700, seed=4)
    n = len(ip) - 1
    nodes = np.concatenate([special, [-1, n, n + 3, 2**40], np.arange(n - 40, n), special[:5]]).astype(np.int64)
    for T, W, p, seed, step, layer in ((2, 10, 0.5, 0, 0, 0), (1, 1, 0.0, 3, 7, 1), (16, 32, 0.0, 2**64 - 5, 2**64 - 1, 7), (8, 64, 0.25, 5, 1, 2),
                                       (3, 17, 0.9, 1, 2, 3)):
        a = traces(ip, ix, nodes, W, T, threshold(p), seed, step, layer)
        b = traces_slow(ip, ix, nodes, W, T, threshold(p), seed, step, layer)
        assert a.shape == (len(nodes), W, T + 1) and a.dtype == np.int64
        assert np.array_equal(a, b), (T, W, p)
        bad = (nodes < 0) | (nodes >= n)
        assert np.all(a[bad] == -1) and np.all(a[~bad, :, 0] == nodes[~bad, None])
        # once a walk has ended it stays ended, and every hop follows an in-edge
        hops = a[:, :, 1:]
        assert not np.any((hops[:, :, 1:] >= 0) & (hops[:, :, :-1] < 0))
        for i in np.flatnonzero(~bad)[:20]:
            for w in range(W):
                for h in range(T):
                    if a[i, w, 1 + h] >= 0:
                        u = a[i, w, h]
                        assert a[i, w, 1 + h] in ix[ip[u]: ip[u + 1]]


def test_first_hop_is_uniform():
    """A node of in-degree 7, W = 1: the first hop over steps 0..13999 against uniform, chi-square below 22.46 (0.999 quantile, 6 d.o.f.)."""
    ip, ix = csc_from_columns([[1, 2, 3, 4, 5, 6, 7]] + [[0]] * 7)
    hits = np.zeros(8, dtype=np.int64)
    for step in range(14000):
        hits[traces(ip, ix, [0], 1, 1, 0, SEED, step)[0, 0, 1]] += 1
    assert hits[0] == 0 and hits.sum() == 14000
    chi2 = float(((hits[1:] - 2000.0) ** 2 / 2000.0).sum())
    print("first-hop counts", hits[1:].tolist(), "chi-square", chi2)
    assert chi2 < 22.46


def test_termination_rate():
    """termination_prob = 0.3: of 20,000 walks the number ended at hop 1 lies within 4 sqrt(20000 * 0.3 * 0.7) ~ 259 of 6,000."""
    ip, ix = _cycle_graph(5000, 3)
    tr = traces(ip, ix, np.arange(5000), 4, 2, threshold(0.3), SEED, 0)
    assert np.all(tr[:, :, 1] >= 0), "the first hop is never terminated"
    ended = int((tr[:, :, 2] < 0).sum())
    print("ended at hop 1:", ended, "of 20000")
    assert abs(ended - 6000) <= 4 * np.sqrt(20000 * 0.3 * 0.7)


def test_no_termination_gives_full_traces():
    ip, ix = _cycle_graph(300, 4)
    tr = traces(ip, ix, np.arange(300), 5, 16, 0, SEED, 3, layer=1)
    assert np.all(tr >= 0)


def test_traces_do_not_depend_on_the_batch():
    ip, ix, special = edge_case_graph([3], n_plain=100, seed=1)
    n = len(ip) - 1
    full = traces(ip, ix, np.arange(n), 6, 4, threshold(0.4), SEED, 9, layer=2)
    rng = np.random.default_rng(0)
    batch = rng.permutation(n)[:57]
    batch = np.concatenate([batch, batch[:9]])
    sub = traces(ip, ix, batch, 6, 4, threshold(0.4), SEED, 9, layer=2)
    assert np.array_equal(sub, full[batch])
    assert not np.array_equal(full, traces(ip, ix, np.arange(n), 6, 4, threshold(0.4), SEED, 10, layer=2)), "another step, other walks"
    assert not np.array_equal(full, traces(ip, ix, np.arange(n), 6, 4, threshold(0.4), SEED, 9, layer=1)), "another layer, other walks"


def test_selection_order_and_padding():
    tr = np.full((3, 3, 4), -1, dtype=np.int64)
    tr[0, :, 0] = 9
    tr[0, 0, 1:] = [5, 2, 5]
    tr[0, 1, 1:] = [7, 2, -1]
    tr[0, 2, 1:] = [9, 3, 7]          # counts: 5 -> 2, 2 -> 2, 7 -> 2, 9 -> 1 (the start node counts only where it is visited), 3 -> 1
    tr[1, :, 0] = 4
    tr[1, 0, 1:] = [4, 4, 4]          # a self-loop: one distinct node
    nbr, cnt = select(tr, 4)
    assert nbr.tolist() == [[2, 5, 7, 3], [4, -1, -1, -1], [-1, -1, -1, -1]]
    assert cnt.tolist() == [[2, 2, 2, 1], [3, 0, 0, 0], [0, 0, 0, 0]] and cnt.dtype == np.int32
    nbr, cnt = select(tr, 6)
    assert nbr[0].tolist() == [2, 5, 7, 3, 9, -1] and cnt[0].tolist() == [2, 2, 2, 1, 1, 0]
    # on a sampled layer: counts never increase along a row, ids ascend inside a tie, a row's counts sum to at most W T
    ip, ix, special = edge_case_graph([5], n_plain=200, seed=2)
    src, loc, c, g = walk_layer(ip, ix, np.arange(len(ip) - 1), 5, 3, 12, threshold(0.2), SEED, 0, 0)
    assert np.all(c[:, 1:] <= c[:, :-1]) and np.all((c == 0) == (g < 0)) and np.all(c.sum(1) <= 36)
    tie = (c[:, 1:] == c[:, :-1]) & (c[:, 1:] > 0)
    assert np.all(g[:, 1:][tie] > g[:, :-1][tie])
    deg = np.diff(ip)
    assert np.all((g[:, 0] >= 0) == (deg > 0))


def test_compaction_and_layer_lists():
    dst = np.array([8, 3, 8, -1, 50], dtype=np.int64)
    nbr = np.array([[3, 7], [7, -1], [9, 8], [-1, -1], [2, 3]], dtype=np.int64)
    src, loc = compact_fixed(dst, nbr)
    assert src.tolist() == [8, 3, 50, 7, 9, 2]
    assert loc.tolist() == [[1, 3], [3, -1], [4, 0], [-1, -1], [5, 1]] and loc.dtype == np.int32
    ip, ix = _cycle_graph(200, 3)
    seeds = np.arange(0, 200, 7)
    layers = reference_layers(ip, ix, seeds, [3, 2], 2, 10, threshold(0.5), SEED, 1)
    assert np.array_equal(layers[0][0][: len(seeds)], seeds)
    assert layers[1][1].shape == (len(layers[0][0]), 2) and np.array_equal(layers[1][0][: len(layers[0][0])], layers[0][0])
    again = walk_layer(ip, ix, layers[0][0], 2, 2, 10, threshold(0.5), SEED, 1, 1)
    assert all(np.array_equal(a, b) for a, b in zip(again, layers[1]))
