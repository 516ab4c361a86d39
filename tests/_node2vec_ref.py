"""Python-integer / numpy restatement of the second-order walks, the skip-gram batch and the window loss: the reference of the node2vec
tests (coala_sampler_node2vec_walk, coala_sampler_walk_batch, coala_block_skipgram_loss).

Contract (coala_sampler.hip header).  Thresholds: m = max(1/p, 1, 1/q); thr_return, thr_near, thr_far = int(x / m * 2^32) for x = 1/p, 1,
1/q in float64.  Keys: wkey = sample_key(seed, step, 0, v) ^ 0x1F83D9ABFB41BD6B, walk w uses kw = splitmix64(wkey + w).  Hop h at `cur`,
having come from `prev`: deg(cur) == 0 ends the walk; attempt a = 0, 1, .. uses c = 2 (256 h + a) and the candidate
x = indices[indptr[cur] + mulhi64(splitmix64(kw + c), deg)]; at h = 0 attempt 0 is taken; at h >= 1 the class of x picks t (return:
x == prev; near: x occurs in row prev; far otherwise) and x is taken when (splitmix64(kw + c + 1) >> 32) < t; the first taken attempt
wins, attempt 255's candidate is taken when all 256 fail; a taken x outside [0, N) ends the walk; -1 pads.  The near test goes through a
Python set here: independent of the order inside a row.
Negatives: row (walk, j), column 0 = the start node, column t >= 1 = mulhi64(splitmix64((kw ^ 0x6A09E667F3BCC909) + 128 j + t), N).
Compaction: the distinct ids of [valid start nodes | traces row-major | negatives' columns 1.. row-major] in order of first appearance.
Loss: float64, PyG's Node2Vec.loss with softplus (block_ops.skipgram_loss's docstring)."""
import numpy as np

from _labor_ref import M64, splitmix64_int

STREAM = 0x1F83D9ABFB41BD6B
NEG_STREAM = 0x6A09E667F3BCC909
ATTEMPTS = 256
_GOLD = 0x9E3779B97F4A7C15
_STEP = 0xD1B54A32D192ED03
ONE = 1 << 32


def thresholds(p, q):
    a, b = 1.0 / float(p), 1.0 / float(q)
    m = max(a, 1.0, b)
    return int(a / m * 4294967296.0), int(1.0 / m * 4294967296.0), int(b / m * 4294967296.0)


def _outer_key(seed, step):
    h = splitmix64_int(((seed & M64) ^ _GOLD) & M64)          # layer 0: GOLD * (0 + 1)
    return splitmix64_int((h ^ ((step & M64) * _STEP)) & M64)


def walk_key(outer, v, w):
    wkey = splitmix64_int(outer ^ (v & M64)) ^ STREAM
    return splitmix64_int((wkey + w) & M64)


def mulhi(a, b):
    return (a * b) >> 64


class Graph(object):
    """The CSC as Python lists, and every row as a set (the near test)."""

    def __init__(self, indptr, indices):
        self.ip, self.ix = np.asarray(indptr).tolist(), np.asarray(indices).tolist()
        self.N = len(self.ip) - 1
        self._sets = {}

    def row_set(self, v):
        s = self._sets.get(v)
        if s is None:
            s = self._sets[v] = set(self.ix[self.ip[v]: self.ip[v + 1]])
        return s


def walk(G, kw, v, L, thr, swap_classes=False, stats=None):
    """One walk: -> list of L + 1 ids, -1 once ended.  swap_classes: the fault injection `return and near swapped`.  stats (a dict):
    counts the hops that ran into the attempt cap under 'capped'."""
    t_ret, t_near, t_far = thr
    if swap_classes:
        t_ret, t_near = t_near, t_ret
    out = [v] + [-1] * L
    cur, prev = v, -1
    for h in range(L):
        start = G.ip[cur]
        deg = G.ip[cur + 1] - start
        if deg <= 0:
            break
        x = -1
        took = False
        for a in range(ATTEMPTS):
            c = 2 * (ATTEMPTS * h + a)
            x = G.ix[start + mulhi(splitmix64_int((kw + c) & M64), deg)]
            if h == 0:
                took = True
                break
            t = t_ret if x == prev else (t_near if x in G.row_set(prev) else t_far)
            if (splitmix64_int((kw + c + 1) & M64) >> 32) < t:
                took = True
                break
        if not took and stats is not None:
            stats["capped"] = stats.get("capped", 0) + 1
        if x < 0 or x >= G.N:
            break
        prev, cur = cur, x
        out[h + 1] = cur
    return out


def traces(indptr, indices, nodes, L, W, thr, seed, step, swap_classes=False, stats=None):
    """-> int64 [n, W, L + 1]; an out-of-range start node gives a row of -1."""
    G = indptr if isinstance(indptr, Graph) else Graph(indptr, indices)
    outer = _outer_key(seed, step)
    out = np.full((len(nodes), W, L + 1), -1, dtype=np.int64)
    memo = {}
    for i, v in enumerate(np.asarray(nodes).tolist()):
        if not 0 <= v < G.N:
            continue
        if v not in memo:       # a repeated start node has the same walks
            memo[v] = [walk(G, walk_key(outer, v, w), v, L, thr, swap_classes, stats) for w in range(W)]
        out[i] = memo[v]
    return out


def negatives(nodes, N, L, W, K, seed, step, keep_start=True):
    """-> int64 [n * W * K, L + 1].  keep_start=False: the fault injection `column 0 dropped` (column 0 drawn like the others)."""
    outer = _outer_key(seed, step)
    out = np.full((len(nodes) * W * K, L + 1), -1, dtype=np.int64)
    for i, v in enumerate(np.asarray(nodes).tolist()):
        if not 0 <= v < N:
            continue
        for w in range(W):
            nk = walk_key(outer, v, w) ^ NEG_STREAM
            for j in range(K):
                row = out[(i * W + w) * K + j]
                row[0] = v if keep_start else mulhi(splitmix64_int((nk + 128 * j) & M64), N)
                for t in range(1, L + 1):
                    row[t] = mulhi(splitmix64_int((nk + 128 * j + t) & M64), N)
    return out


def walk_batch(indptr, indices, nodes, L, W, K, thr, seed, step):
    """-> dict(input_nodes int64, pos int32 [n W, L + 1], neg int32 [n W K, L + 1], traces int64 [n, W, L + 1], n_bad)."""
    nodes = np.asarray(nodes, dtype=np.int64)
    N = len(indptr) - 1
    tr = traces(indptr, indices, nodes, L, W, thr, seed, step)
    ng = negatives(nodes, N, L, W, K, seed, step)
    ok = (nodes >= 0) & (nodes < N)
    items = np.concatenate([np.where(ok, nodes, -1), tr.reshape(-1), ng[:, 1:].reshape(-1)])
    keep = items >= 0
    uniq, first = np.unique(items[keep], return_index=True)
    order = np.argsort(first, kind="stable")
    input_nodes = uniq[order]
    local = {int(v): i for i, v in enumerate(input_nodes.tolist())}
    relabel = np.vectorize(lambda x: local[x] if x >= 0 else -1, otypes=[np.int32])
    pos = relabel(tr.reshape(-1, L + 1)) if tr.size else np.zeros((0, L + 1), np.int32)
    neg = relabel(ng) if ng.size else np.zeros((0, L + 1), np.int32)
    return dict(input_nodes=input_nodes, pos=pos, neg=neg, traces=tr, n_bad=int((~ok).sum()))


# ------------------------------------------------------------------------------------------------------------ vectorised forms
# The same rules in numpy uint64 (wrapping arithmetic), for batches of millions of items.  The Python-integer forms above stay the
# definition; test_item_batch_large_cpu.py holds these to them bit for bit.
def _walk_keys_vec(nodes, W, seed, step):
    """kw of every (start node, walk): uint64 [n, W]."""
    from _labor_ref import splitmix64
    v = np.asarray(nodes, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        wkey = splitmix64(np.uint64(_outer_key(seed, step)) ^ v) ^ np.uint64(STREAM)
        return splitmix64(wkey[:, None] + np.arange(W, dtype=np.uint64)[None, :])


def traces_vec(indptr, indices, nodes, L, W, thr, seed, step, swap_classes=False):
    """traces() for every walk at once: per hop, over the walks still alive, an attempt loop over the walks still undecided.  The near
    test is a binary search in the keys row * span + source of the whole CSC, so every row must be sorted by source (what the device
    needs at q != 1 as well)."""
    from _labor_ref import mulhi64, splitmix64
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    nodes = np.asarray(nodes, dtype=np.int64)
    n, N = len(nodes), len(indptr) - 1
    t_ret, t_near, t_far = (np.uint64(t) for t in thr)
    if swap_classes:
        t_ret, t_near = t_near, t_ret
    lo = int(indices.min()) if len(indices) else 0
    span = (int(indices.max()) - lo + 1) if len(indices) else 1
    edge_key = np.repeat(np.arange(N, dtype=np.int64), np.diff(indptr)) * span + (indices - lo)
    assert np.all(np.diff(edge_key) >= 0), "traces_vec needs every row sorted by source"

    def in_row(row, x):                                     # does x occur in row `row`?
        inside = (x >= lo) & (x < lo + span)
        want = row * span + (np.where(inside, x, lo) - lo)
        at = np.minimum(np.searchsorted(edge_key, want), max(len(edge_key) - 1, 0))
        return inside & (edge_key[at] == want) if len(edge_key) else np.zeros(len(x), dtype=bool)

    ok = np.repeat((nodes >= 0) & (nodes < N), W)
    kw = _walk_keys_vec(nodes, W, seed, step).reshape(-1)
    out = np.full((n * W, L + 1), -1, dtype=np.int64)
    cur = np.where(ok, np.repeat(nodes, W), 0)
    out[ok, 0] = cur[ok]
    prev = np.full(n * W, -1, dtype=np.int64)
    alive = ok.copy()
    with np.errstate(over="ignore"):
        for h in range(L):
            idx = np.flatnonzero(alive)
            start = indptr[cur[idx]]
            deg = indptr[cur[idx] + 1] - start
            alive[idx[deg <= 0]] = False
            idx, start, deg = idx[deg > 0], start[deg > 0], deg[deg > 0]
            x = np.full(len(idx), -1, dtype=np.int64)
            und = np.arange(len(idx))                      # the walks of idx that have taken no candidate yet
            for a in range(ATTEMPTS):
                if len(und) == 0:
                    break
                c = np.uint64(2 * (ATTEMPTS * h + a))
                k = kw[idx[und]]
                cand = indices[start[und] + mulhi64(splitmix64(k + c), deg[und].astype(np.uint64)).astype(np.int64)]
                x[und] = cand                              # attempt 255's candidate stays when every attempt fails
                if h == 0:
                    break
                p = prev[idx[und]]
                t = np.where(cand == p, t_ret, np.where(in_row(p, cand), t_near, t_far))
                und = und[~((splitmix64(k + c + np.uint64(1)) >> np.uint64(32)) < t)]
            good = (x >= 0) & (x < N)
            alive[idx[~good]] = False
            g = idx[good]
            prev[g], cur[g] = cur[g], x[good]
            out[g, h + 1] = x[good]
    return out.reshape(n, W, L + 1)


def negatives_vec(nodes, N, L, W, K, seed, step):
    """negatives() (keep_start=True) for every row at once."""
    from _labor_ref import mulhi64, splitmix64
    nodes = np.asarray(nodes, dtype=np.int64)
    n = len(nodes)
    ok = (nodes >= 0) & (nodes < N)
    nk = _walk_keys_vec(nodes, W, seed, step) ^ np.uint64(NEG_STREAM)
    out = np.empty((n, W, K, L + 1), dtype=np.int64)
    with np.errstate(over="ignore"):
        c = (np.uint64(128) * np.arange(K, dtype=np.uint64))[:, None] + np.arange(L + 1, dtype=np.uint64)[None, :]
        out[...] = mulhi64(splitmix64(nk[:, :, None, None] + c[None, None]), np.uint64(N)).astype(np.int64)
    out[..., 0] = nodes[:, None, None]
    out[~ok] = -1
    return out.reshape(n * W * K, L + 1)


def walk_batch_vec(indptr, indices, nodes, L, W, K, thr, seed, step):
    """walk_batch() from traces_vec, negatives_vec and _edge_batch_ref.compact."""
    from _edge_batch_ref import compact
    nodes = np.asarray(nodes, dtype=np.int64)
    n, N = len(nodes), len(indptr) - 1
    tr = traces_vec(indptr, indices, nodes, L, W, thr, seed, step)
    ng = negatives_vec(nodes, N, L, W, K, seed, step)
    ok = (nodes >= 0) & (nodes < N)
    input_nodes, local = compact(np.concatenate([np.where(ok, nodes, -1), tr.reshape(-1), ng[:, 1:].reshape(-1)]))
    local = local.astype(np.int32)
    n_pos = n * W * (L + 1)
    neg = np.empty((n * W * K, L + 1), dtype=np.int32)
    neg[:, 0] = np.repeat(local[:n], W * K)               # column 0: the item of the walk's start node
    neg[:, 1:] = local[n + n_pos:].reshape(n * W * K, L)
    return dict(input_nodes=input_nodes, pos=local[n: n + n_pos].reshape(n * W, L + 1), neg=neg, traces=tr, n_bad=int((~ok).sum()))


# ----------------------------------------------------------------------------------------------------- exact transition probabilities
def transition_probs(G, prev, cur, p, q):
    """node2vec's second-order transition distribution at `cur` having come from `prev`, over the entries of row cur: {next: prob}."""
    row = G.ix[G.ip[cur]: G.ip[cur + 1]]
    wts = [(1.0 / p) if x == prev else (1.0 if x in G.row_set(prev) else 1.0 / q) for x in row]
    tot = sum(wts)
    out = {}
    for x, wt in zip(row, wts):
        out[x] = out.get(x, 0.0) + wt / tot
    return out


# ----------------------------------------------------------------------------------------------------------------- window loss (f64)
def window_pairs(L1, C):
    """[(a, a + j)] for every window start a in 0 .. L1 - C and j in 1 .. C - 1."""
    return [(a, a + j) for a in range(L1 - C + 1) for j in range(1, C)]


def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0, e) / (1.0 + e)


def table_loss(h, rows, C, sign, over_ended=False):
    """-> (mean loss, its gradient w.r.t. h, the number of valid pairs) of one table, in float64.  over_ended: the fault injection
    `windows run over a -1` (a -1 entry read as the last row of h, as a raw gather would)."""
    h = np.asarray(h, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    grad = np.zeros_like(h)
    if rows.shape[0] == 0:
        return 0.0, grad, 0
    pairs = np.array(window_pairs(rows.shape[1], C), dtype=np.int64).reshape(-1, 2)
    s, d = rows[:, pairs[:, 0]].reshape(-1), rows[:, pairs[:, 1]].reshape(-1)
    keep = np.ones_like(s, dtype=bool) if over_ended else (s >= 0) & (d >= 0)
    s, d = s[keep], d[keep]
    n = len(s)
    if n == 0:
        return 0.0, grad, 0
    score = (h[s] * h[d]).sum(-1)
    loss = _softplus(sign * score).sum() / n
    coef = (sign * _sigmoid(sign * score) / n)[:, None]
    np.add.at(grad, s, coef * h[d])
    np.add.at(grad, d, coef * h[s])
    return float(loss), grad, n


def skipgram_loss(h, pos, neg, C, over_ended=False):
    """-> (loss, grad_h) in float64: mean softplus(-s) over pos's valid pairs + mean softplus(s) over neg's."""
    lp, gp, _ = table_loss(h, pos, C, -1.0, over_ended)
    ln, gn, _ = table_loss(h, neg, C, 1.0, over_ended)
    return lp + ln, gp + gn


# ----------------------------------------------------------------------------------------------------------------- the GPU tests' graph
def edge_graph(hub_degree=5000):
    """test_sampler_pinsage_gpu.py's graph with every row sorted by source id: _util.edge_case_graph (degree edges, self-loops, repeated
    neighbours, 2,000 plain nodes, a hub), then a node whose only in-neighbour is itself, a 2-cycle, a sink and a node one hop above it.
    -> (indptr, indices, special nodes, named nodes, the number of nodes before the named ones)."""
    from _util import csc_from_columns, edge_case_graph
    ip, ix, special = edge_case_graph([1, 3, 5, 32], n_plain=2000, hub_degree=hub_degree, seed=5)
    n0 = len(ip) - 1
    cols = [np.sort(ix[ip[v]: ip[v + 1]]) for v in range(n0)]
    own, a, b, sink, above = n0, n0 + 1, n0 + 2, n0 + 3, n0 + 4
    cols += [[own], [b], [a], [], [sink]]
    ip, ix = csc_from_columns(cols)
    named = dict(own=own, a=a, b=b, sink=sink, above=above, hub=n0 - 1)
    assert ip[n0] - ip[n0 - 1] == hub_degree
    return ip, ix, special, named, n0
