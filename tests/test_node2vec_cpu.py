"""CPU tests of the node2vec pieces: the reference of tests/_node2vec_ref.py against itself and against the exact node2vec transition
probabilities, the attempt cap, the torch fallback of the window loss against the float64 table, and three fault injections that
these checks must catch.

Transition frequencies.  A hop of the rule accepts candidate x (uniform over the row of cur) with probability t_class / 2^32, so the
accepted x has probability proportional to (its multiplicity) * t_class: node2vec's alpha / sum alpha up to the 2^-32 truncation of the
thresholds and the attempt cap ((15/16)^256 ~ 7e-8 per hop at worst), both far below the resolution of this test.  Every (prev, cur)
context seen n times and every next node of exact probability P must show a count within 5 sigma = 5 sqrt(n P (1 - P)) of n P: over
the ~600 cells of the four settings a false alarm has probability ~ 600 * 5.7e-7."""
import math

import numpy as np
import pytest

import _node2vec_ref as R
from _labor_ref import M64, splitmix64_int

SETTINGS = [(0.25, 4.0), (4.0, 0.25), (1.0, 1.0), (0.5, 2.0)]


def small_graph():
    """12 nodes, symmetric, simple: a ring, chords that close triangles and chords that do not, one pendant-like node of degree 2."""
    edges = {(i, (i + 1) % 12) for i in range(12)} | {(0, 2), (2, 4), (4, 6), (1, 7), (3, 9), (5, 11), (0, 6), (8, 10), (2, 9)}
    cols = [[] for _ in range(12)]
    for u, v in edges:
        cols[u].append(v)
        cols[v].append(u)
    ip = np.zeros(13, dtype=np.int64)
    np.cumsum([len(c) for c in cols], out=ip[1:])
    rng = np.random.default_rng(0)
    ix = np.concatenate([rng.permutation(c) for c in cols]).astype(np.int64)      # rows NOT sorted: the reference does not care
    return ip, ix


def worst_sigma(p, q, swap_classes=False, steps=4000):
    """Walks of 3 hops from every node at `steps` steps -> (the worst deviation of a (prev, cur, next) count from its expectation, in
    sigmas; the number of cells)."""
    ip, ix = small_graph()
    G = R.Graph(ip, ix)
    thr = R.thresholds(p, q)
    ctx, cell = {}, {}
    nodes = np.arange(12)
    for step in range(steps):
        tr = R.traces(G, None, nodes, 3, 1, thr, seed=11, step=step, swap_classes=swap_classes)[:, 0]
        for row in tr.tolist():
            for h in (1, 2):
                a, b, c = row[h - 1], row[h], row[h + 1]
                assert c >= 0, "no walk ends on this graph"
                ctx[(a, b)] = ctx.get((a, b), 0) + 1
                cell[(a, b, c)] = cell.get((a, b, c), 0) + 1
    worst, cells = 0.0, 0
    for (a, b), n in ctx.items():
        for c, P in R.transition_probs(G, a, b, p, q).items():
            got = cell.get((a, b, c), 0)
            sd = math.sqrt(n * P * (1.0 - P))
            worst = max(worst, abs(got - n * P) / sd if sd > 0 else (0.0 if got == n * P else math.inf))
            cells += 1
    return worst, cells


# ------------------------------------------------------------------------------------------------ 1. the reference against itself
def test_thresholds():
    assert R.thresholds(1, 1) == (R.ONE, R.ONE, R.ONE)
    assert R.thresholds(0.25, 4) == (R.ONE, R.ONE // 4, R.ONE // 16) and R.thresholds(4, 0.25) == (R.ONE // 16, R.ONE // 4, R.ONE)
    for p in (0.25, 0.5, 1, 2, 4):
        for q in (0.25, 0.5, 1, 2, 4):
            t = R.thresholds(p, q)
            assert max(t) == R.ONE and min(t) >= 1 << 28, "the paper's grid fits the wrapper's 1/16 bound"
    assert min(R.thresholds(0.2, 4)) < 1 << 28


def test_reference_self_consistency():
    ip, ix = small_graph()
    G = R.Graph(ip, ix)
    nodes = np.array([3, 7, 3, -1, 12, 0], dtype=np.int64)
    thr = R.thresholds(0.5, 2)
    tr = R.traces(ip, ix, nodes, 6, 4, thr, seed=5, step=9)
    assert tr.shape == (6, 4, 7) and np.array_equal(tr[0], tr[2]), "a repeated start node has the same walks"
    assert np.all(tr[3] == -1) and np.all(tr[4] == -1) and np.all(tr[[0, 1, 5], :, 0] == nodes[[0, 1, 5], None])
    for row in tr[[0, 1, 5]].reshape(-1, 7).tolist():
        for a, b in zip(row, row[1:]):
            assert b in G.row_set(a), "every hop follows an in-edge"
    assert not np.array_equal(tr, R.traces(ip, ix, nodes, 6, 4, thr, seed=5, step=10)) and not np.array_equal(tr[0, 0], tr[0, 1])
    # hop 0 does not depend on p and q; a walk is a prefix of the longer walk with the same key
    other = R.traces(ip, ix, nodes, 6, 4, R.thresholds(4, 0.25), seed=5, step=9)
    assert np.array_equal(tr[:, :, :2], other[:, :, :2]) and not np.array_equal(tr, other)
    assert np.array_equal(R.traces(ip, ix, nodes, 3, 4, thr, seed=5, step=9), tr[:, :, :4])
    # the batch: start nodes first, every entry addresses its node, column 0 of a negative is its walk's start
    b = R.walk_batch(ip, ix, nodes, 6, 4, 3, thr, seed=5, step=9)
    assert b["n_bad"] == 2 and b["input_nodes"][:3].tolist() == [3, 7, 0] and len(set(b["input_nodes"].tolist())) == len(b["input_nodes"])
    pos, neg = b["pos"], b["neg"]
    assert pos.shape == (24, 7) and neg.shape == (72, 7) and np.array_equal(b["traces"], tr)
    flat = tr.reshape(-1, 7)
    assert np.array_equal(pos >= 0, flat >= 0) and np.array_equal(b["input_nodes"][pos[pos >= 0]], flat[flat >= 0])
    starts = np.repeat(flat[:, 0], 3)
    assert np.array_equal(neg[:, 0] >= 0, starts >= 0) and np.array_equal(b["input_nodes"][neg[starts >= 0, 0]], starts[starts >= 0])
    assert np.all(neg[starts < 0] == -1) and np.all(neg[starts >= 0] >= 0)
    used = np.zeros(len(b["input_nodes"]), dtype=bool)
    used[pos[pos >= 0]] = True
    used[neg[neg >= 0]] = True
    assert used.all(), "input_nodes holds nothing the tables do not address"
    assert R.window_pairs(5, 3) == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (2, 4)] and len(R.window_pairs(21, 10)) == 12 * 9


# ------------------------------------------------------------------------------------------------ 2. transition frequencies
@pytest.mark.parametrize("p,q", SETTINGS)
def test_transition_frequencies(p, q):
    worst, cells = worst_sigma(p, q)
    print(f"p={p} q={q}: worst deviation {worst:.2f} sigma over {cells} cells")
    assert cells >= 150 and worst <= 5.0, f"p={p} q={q}: a (prev, cur, next) frequency is {worst:.2f} sigma from the exact probability"


def test_fault_swapped_classes_is_caught():
    """Return and near thresholds swapped: the frequency check must fail where they differ."""
    worst, _ = worst_sigma(0.25, 4.0, swap_classes=True, steps=1000)
    assert worst > 5.0


# ------------------------------------------------------------------------------------------------ 3. the attempt cap
def test_cap_on_a_star():
    """thr_far = 0 (and thr_return = 0) on a star: at the centre every candidate is the previous leaf or far, at a leaf the only candidate
    leads back: every hop after the first refuses 256 attempts and takes attempt 255's candidate."""
    k = 9
    cols = [list(range(1, k + 1))] + [[0]] * k
    ip = np.zeros(k + 2, dtype=np.int64)
    np.cumsum([len(c) for c in cols], out=ip[1:])
    ix = np.concatenate(cols).astype(np.int64)
    L, stats = 12, {}
    tr = R.traces(ip, ix, np.arange(k + 1), L, 2, (0, R.ONE, 0), seed=1, step=2, stats=stats)
    assert stats["capped"] == (k + 1) * 2 * (L - 1) and np.all(tr >= 0)
    outer = R._outer_key(1, 2)
    for v in range(k + 1):
        for w in range(2):
            kw, row = R.walk_key(outer, v, w), tr[v, w].tolist()
            for h in range(1, L):
                cur = row[h]
                deg = int(ip[cur + 1] - ip[cur])
                want = int(ix[ip[cur] + R.mulhi(splitmix64_int((kw + 2 * (256 * h + 255)) & M64), deg)])
                assert row[h + 1] == want, "the capped hop takes attempt 255's candidate"
    # with the return class open the centre goes back to the leaf it came from, the only candidate that is ever accepted
    back = R.traces(ip, ix, np.arange(1, k + 1), 6, 1, (R.ONE, R.ONE, 0), seed=1, step=2)[:, 0]
    assert np.all(back[:, 1::2] == 0) and np.all(back[:, 2::2] == back[:, :1])


# ------------------------------------------------------------------------------------------------ 4. the torch fallback of the loss
def loss_case(rng, N, D, R_rows, L1, ended=True):
    h = rng.standard_normal((N, D)) * 0.7
    pos = rng.integers(0, N, size=(R_rows, L1))
    neg = rng.integers(0, N, size=(R_rows * 2, L1))
    if ended:
        for r in range(0, R_rows, 3):
            pos[r, rng.integers(1, L1):] = -1       # an ended walk
        neg[1] = -1                                   # the rows of an invalid start node
        pos[1, 1] = pos[1, 0]                         # a node twice inside a window
    return h, pos.astype(np.int64), neg.astype(np.int64)


@pytest.mark.parametrize("D,L1,C", [(1, 2, 2), (16, 21, 10), (33, 21, 21), (8, 9, 2)])
def test_skipgram_loss_torch_against_float64(hiplib, D, L1, C):
    import torch
    from COALA_GNN.block_ops import skipgram_loss, skipgram_loss_torch
    rng = np.random.default_rng(D * 100 + L1)
    h, pos, neg = loss_case(rng, 40, D, 7, L1)
    want, want_g = R.skipgram_loss(h, pos, neg, C)
    for fn in (skipgram_loss_torch, skipgram_loss):     # on the CPU skipgram_loss is its fallback
        for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 2e-5)):
            t = torch.tensor(h, dtype=dtype, requires_grad=True)
            out = fn(t, torch.from_numpy(pos), torch.from_numpy(neg).to(torch.int32), C)
            out.backward()
            assert out.dim() == 0 and out.dtype == dtype
            assert abs(float(out.detach()) - want) <= tol * max(1.0, abs(want))
            assert np.abs(t.grad.numpy().astype(np.float64) - want_g).max() <= tol * max(1.0, np.abs(want_g).max())


def test_skipgram_loss_edges(hiplib):
    import torch
    from COALA_GNN.block_ops import skipgram_loss_torch
    h = torch.randn(5, 4, dtype=torch.float64, requires_grad=True)
    none = torch.full((3, 6), -1)
    out = skipgram_loss_torch(h, none, none[:0], 3)
    out.backward()
    assert float(out.detach()) == 0.0 and float(h.grad.abs().max()) == 0.0, "a mean over no pair is 0"
    # one window, one pair: softplus(-s) + softplus(s) by hand
    h2 = torch.tensor([[1.0, 2.0], [0.5, -1.0]], dtype=torch.float64)
    s = 1.0 * 0.5 - 2.0
    got = float(skipgram_loss_torch(h2, torch.tensor([[0, 1]]), torch.tensor([[0, 1]]), 2))
    assert abs(got - (math.log1p(math.exp(s)) + math.log1p(math.exp(-s)))) < 1e-14
    for bad in (dict(context_size=1), dict(context_size=7)):
        with pytest.raises(ValueError):
            skipgram_loss_torch(h, none, none, **bad)
    with pytest.raises(IndexError):
        skipgram_loss_torch(h, torch.tensor([[0, 5]]), none, 2)
    with pytest.raises(ValueError):
        skipgram_loss_torch(h, torch.tensor([[0.0, 1.0]]), none, 2)


def test_fault_windows_over_ended_walks_is_caught(hiplib):
    """A loss whose windows run over a -1 (read as a row of h) is not the reference's loss: the comparison above would fail."""
    import torch
    from COALA_GNN.block_ops import skipgram_loss_torch
    rng = np.random.default_rng(3)
    h, pos, neg = loss_case(rng, 40, 16, 7, 21)
    good, _ = R.skipgram_loss(h, pos, neg, 10)
    bad, _ = R.skipgram_loss(h, pos, neg, 10, over_ended=True)
    got = float(skipgram_loss_torch(torch.tensor(h), torch.from_numpy(pos), torch.from_numpy(neg), 10))
    assert abs(got - good) <= 1e-12 and abs(got - bad) > 1e-3


def test_fault_dropped_start_column_is_caught():
    """Negatives whose column 0 is drawn like the others, not the walk's start node, differ from the reference's table."""
    nodes = np.arange(12)
    good = R.negatives(nodes, 12, 5, 2, 3, seed=4, step=0)
    bad = R.negatives(nodes, 12, 5, 2, 3, seed=4, step=0, keep_start=False)
    assert np.array_equal(good[:, 1:], bad[:, 1:]) and np.array_equal(good[:, 0], np.repeat(nodes, 6))
    assert (good[:, 0] != bad[:, 0]).mean() > 0.5


def test_new_symbols_and_refusals(hiplib):
    """The C entries exist, and refuse bad arguments before touching the device (no GPU needed: nothing is launched)."""
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    for name in ("coala_sampler_node2vec_walk", "coala_sampler_walk_batch", "coala_sampler_walk_batch_wait", "coala_block_skipgram_loss",
                 "coala_block_skipgram_loss_backward"):
        assert hasattr(L, name)
    assert L.coala_block_skipgram_loss(0, None, None, None, None, 4, 1, 2, 8, -1.0, None) == _capi.EINVAL and "walk table shape" in _capi.last_error()
    assert L.coala_block_skipgram_loss(0, None, None, None, None, 4, 129, 2, 8, -1.0, None) == _capi.EINVAL
    assert L.coala_block_skipgram_loss(0, None, None, None, None, 4, 128, 2, 129, -1.0, None) == _capi.EINVAL   # 128 * 129 > 16384
    assert L.coala_block_skipgram_loss(0, None, None, None, None, 4, 21, 22, 8, -1.0, None) == _capi.EINVAL
    assert L.coala_block_skipgram_loss(0, None, None, None, None, 4, 21, 10, 8, 0.5, None) == _capi.EINVAL
    assert L.coala_block_skipgram_loss(0, None, None, None, None, 0, 21, 10, 8, 1.0, None) == _capi.OK
    assert L.coala_block_skipgram_loss_backward(0, None, None, None, None, 0, 21, 10, 8, 1.0, None) == _capi.OK
    from COALA_GNN.sampler import node2vec_thresholds
    assert node2vec_thresholds(0.25, 4) == R.thresholds(0.25, 4) and node2vec_thresholds(3, 0.7) == R.thresholds(3, 0.7)
    for bad in ((0, 1), (1, -2), (float("nan"), 1), (True, 1)):
        with pytest.raises(ValueError):
            node2vec_thresholds(*bad)
