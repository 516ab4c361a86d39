"""Plain numpy restatement of a weighted fixed sampler layer (NeighborSampler(prob=...)), the reference of the weighted tests.

Contract (coala_sampler.hip header): destination d (node v) with in-edges at CSC positions indptr[v] + j and fp32 weights w.  With
P = #{w > 0} <= f the row takes those P edges; otherwise the f smallest (key_j, j) over the positive edges, where
    r_j = splitmix64((sample_key(seed, step, layer, v) ^ STREAM) + j),  u_j = (r_j >> 11) * 2^-53,  key_j = -log1p(-u_j) / w_j  (fp64).
The chosen edges are listed in ascending position, then -1.  The block is compacted as every fixed layer: source list = the
destination nodes, then every other neighbour in order of first appearance in the row-major (d, j) scan.  Full layers come from
_full_ref.full_layer (weights unread)."""
import numpy as np

from _full_ref import full_layer

M64 = (1 << 64) - 1
STREAM = 0x6A09E667F3BCC909
_GOLD = 0x9E3779B97F4A7C15


def splitmix64(x):
    """x: uint64 array (wrapping arithmetic)"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=np.uint64) + np.uint64(_GOLD)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def sample_key(seed, step, layer, v):
    """The uniform path's per-row key, for an array of node ids v."""
    h = int(splitmix64(np.uint64((seed ^ ((_GOLD * (layer + 1)) & M64)) & M64)))
    h = int(splitmix64(np.uint64((h ^ ((step * 0xD1B54A32D192ED03) & M64)) & M64)))
    return splitmix64(np.uint64(h) ^ np.asarray(v, dtype=np.int64).astype(np.uint64))


def edge_keys(wkey_per_edge, j, w):
    """fp64 keys of edges (row key already xor'ed with STREAM, position j in the row, fp32 weight); +inf where w == 0 is NOT used:
    the caller drops weight-0 edges before ranking."""
    with np.errstate(over="ignore"):
        r = splitmix64(wkey_per_edge + np.asarray(j, dtype=np.int64).astype(np.uint64))
    u = (r >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    with np.errstate(divide="ignore", over="ignore"):
        return -np.log1p(-u) / np.asarray(w, dtype=np.float32).astype(np.float64)


def select(indptr, w, dst, f, seed, step, layer, num_nodes=None, with_margin=False):
    """-> pos int64[n_dst, f]: chosen positions j (ascending, -1 padded).  with_margin: also the relative gap between the f-th and
    (f+1)-th smallest keys of each row (inf where the row has at most f positive edges), the measure of a near tie."""
    dst = np.asarray(dst, dtype=np.int64)
    n = len(dst)
    N = len(indptr) - 1 if num_nodes is None else num_nodes
    ok = (dst >= 0) & (dst < N)
    v = np.where(ok, dst, 0)
    starts = np.where(ok, indptr[v], 0)
    deg = np.where(ok, indptr[v + 1] - indptr[v], 0)
    E = int(deg.sum())
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    run = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=run[1:])
    j = np.arange(E, dtype=np.int64) - run[rows]
    we = w[starts[rows] + j]
    pos_ok = we > 0
    rows, j, we = rows[pos_ok], j[pos_ok], we[pos_ok]
    wkey = sample_key(seed, step, layer, dst[rows]) ^ np.uint64(STREAM)
    key = edge_keys(wkey, j, we)
    order = np.lexsort((j, key, rows))                  # by row, then key, then position
    rows_s, j_s, key_s = rows[order], j[order], key[order]
    first = np.searchsorted(rows_s, np.arange(n + 1))
    rank = np.arange(len(rows_s)) - first[rows_s]
    keep = rank < f
    out = np.full((n, f), -1, dtype=np.int64)
    rk, jk = rows_s[keep], j_s[keep]
    o2 = np.lexsort((jk, rk))                           # chosen edges by row, then position
    rk, jk = rk[o2], jk[o2]
    slot = np.arange(len(rk)) - np.searchsorted(rk, rk)
    out[rk, slot] = jk
    if not with_margin:
        return out
    margin = np.full(n, np.inf)
    cnt = np.diff(first)
    has = np.nonzero(cnt > f)[0]
    kf, kf1 = key_s[first[has] + f - 1], key_s[first[has] + f]
    with np.errstate(invalid="ignore", divide="ignore"):
        margin[has] = np.where(kf1 > 0, (kf1 - kf) / kf1, 0.0)
    return out, margin


def compact(dst, nbr):
    """Fixed-layer compaction of global neighbours nbr int64[n_dst, f] (-1 padded) -> (src int64[n_src], nbr_local int32[n_dst, f])"""
    dst = np.asarray(dst, dtype=np.int64)
    flat = nbr.reshape(-1)
    valid = flat >= 0
    items = np.concatenate([dst, flat[valid]])
    uniq, first, inv = np.unique(items, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    loc = np.full(flat.shape, -1, dtype=np.int32)
    loc[valid] = rank[inv.reshape(-1)[len(dst):]]
    return uniq[order], loc.reshape(nbr.shape)


def weighted_layer(indptr, indices, w, dst, f, seed, step, layer):
    """-> (src, nbr_local int32[n_dst, f], chosen positions int64[n_dst, f], margins)"""
    dst = np.asarray(dst, dtype=np.int64)
    pos, margin = select(indptr, w, dst, f, seed, step, layer, with_margin=True)
    N = len(indptr) - 1
    ok = (dst >= 0) & (dst < N)
    starts = np.where(ok, indptr[np.where(ok, dst, 0)], 0)
    nbr = np.where(pos >= 0, indices[np.clip(starts[:, None] + pos, 0, max(len(indices) - 1, 0))] if len(indices) else -1, -1)
    src, loc = compact(dst, nbr)
    return src, loc, pos, margin


def reference_layers(indptr, indices, w, seeds, fanouts_reversed, seed, step):
    """Every layer of a weighted list, in sampling order: [(src, indptr_local or None, nbr_local, margins or None), ...]"""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int64)
    dst = np.asarray(seeds, dtype=np.int64)
    out = []
    for layer, f in enumerate(fanouts_reversed):
        if f == -1:
            src, ip, loc = full_layer(indptr, indices, dst)
            out.append((src, ip, loc, None))
        else:
            src, loc, _, margin = weighted_layer(indptr, indices, w, dst, f, seed, step, layer)
            out.append((src, None, loc, margin))
        dst = src
    return out


def inclusion_probabilities(w, f):
    """Exact inclusion probability of every edge under successive sampling (draw f times without replacement, each time with
    probability proportional to the weight among the edges left), by enumeration of the ordered draws.  Rows with at most f positive
    weights take every positive edge."""
    w = np.asarray(w, dtype=np.float64)
    pos = np.nonzero(w > 0)[0]
    p = np.zeros(len(w))
    if len(pos) <= f:
        p[pos] = 1.0
        return p

    def walk(left, prob, depth, taken):
        if depth == f:
            for i in taken:
                p[i] += prob
            return
        tot = w[left].sum()
        for k, i in enumerate(left):
            walk(left[:k] + left[k + 1:], prob * w[i] / tot, depth + 1, taken + [i])

    walk(list(pos), 1.0, 0, [])
    return p
