"""numpy restatement of the link-prediction pieces (tests only): the endpoints of a seed edge, the negative pairs, the compaction of
the item list into seed nodes, and edge exclusion on a block.  All integer arithmetic, so the device is compared bit for bit.  The rules
are those of coala_sampler_edge_batch and coala_block_exclude_edges (include/coala_hip.h).  Importable without a GPU and without torch."""
import numpy as np

from _util import csc_from_columns, edge_case_graph

M64 = (1 << 64) - 1
K_NEG = 0xA54FF53A5F1D36F1          # kNegStream
# the stream constants the sampler already uses (weighted, LABOR, walk): the negatives' must be none of them
K_OTHERS = (0x6A09E667F3BCC909, 0xBB67AE8584CAA73B, 0x3C6EF372FE94F82B)
CHI2_63_BOUND = 131.7               # the 1 - 1e-6 quantile of chi-square(63), Wilson-Hilferty: 63 (1 - 2/567 + 4.7534 sqrt(2/567))^3


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sample_key(seed, step, layer, v):
    h = splitmix64((seed ^ (0x9E3779B97F4A7C15 * (layer + 1))) & M64)
    h = splitmix64(h ^ ((step * 0xD1B54A32D192ED03) & M64))
    return splitmix64(h ^ (v & M64))


def endpoints(indptr, indices, eids):
    """-> (src, dst) int64 [n]; (-1, -1) for an edge outside [0, E).  dst is the row v with indptr[v] <= e < indptr[v+1]."""
    eids = np.asarray(eids, dtype=np.int64)
    ok = (eids >= 0) & (eids < len(indices))
    e = np.where(ok, eids, 0)
    dst = np.searchsorted(indptr, e, side="right") - 1        # the first i with indptr[i] > e, minus one
    src = indices[e] if len(indices) else np.zeros_like(e)
    return np.where(ok, src, -1), np.where(ok, dst, -1)


def negatives(num_nodes, eids, k, seed, step):
    """-> int64 [n, k]: v'_j = mulhi64(splitmix64(nkey + j), N), nkey = sample_key(seed, step, 0, e) ^ K_NEG; -1 for a bad edge is the
    caller's business (edge_batch): here every e gets its draws."""
    out = np.zeros((len(eids), k), dtype=np.int64)
    for i, e in enumerate(np.asarray(eids, dtype=np.int64).tolist()):
        nkey = sample_key(seed & M64, step & M64, 0, e & M64) ^ K_NEG
        for j in range(k):
            out[i, j] = (splitmix64((nkey + j) & M64) * num_nodes) >> 64
    return out


def negatives_vec(num_nodes, eids, k, seed, step):
    """negatives() in numpy uint64 (wrapping arithmetic), for batches of millions of draws; test_item_batch_large_cpu.py holds it to the
    Python-integer form above, which stays the definition."""
    from _labor_ref import mulhi64, splitmix64 as mix
    e = np.asarray(eids, dtype=np.int64).astype(np.uint64)
    h = splitmix64((seed & M64) ^ 0x9E3779B97F4A7C15)                  # sample_key's first two rounds do not depend on e
    h = splitmix64(h ^ (((step & M64) * 0xD1B54A32D192ED03) & M64))
    with np.errstate(over="ignore"):
        nkey = mix(np.uint64(h) ^ e) ^ np.uint64(K_NEG)
        draws = mix(nkey[:, None] + np.arange(k, dtype=np.uint64)[None, :])
    return mulhi64(draws, np.uint64(num_nodes)).astype(np.int64).reshape(len(e), k)


def compact(items):
    """items int64 (-1: none) -> (the distinct ids >= 0 in order of first appearance, every item's index in that list or -1)."""
    items = np.asarray(items, dtype=np.int64)
    valid = items >= 0
    uniq, first, inv = np.unique(items[valid], return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # uniq sorted by first appearance
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    local = np.full(len(items), -1, dtype=np.int64)
    local[valid] = rank[inv]
    return uniq[order], local


def edge_batch(indptr, indices, eids, k, seed, step, draw=negatives):
    """-> dict(seed_nodes int64, pos_src, pos_dst int32 [n], neg_dst int32 [n, k], n_bad).  draw: negatives, or negatives_vec for a
    batch too large for Python integers."""
    eids = np.asarray(eids, dtype=np.int64)
    n, N = len(eids), len(indptr) - 1
    src, dst = endpoints(indptr, indices, eids)
    neg = draw(N, eids, k, seed, step)
    neg[src < 0] = -1
    nodes, local = compact(np.concatenate([src, dst, neg.reshape(-1)]))
    return dict(seed_nodes=nodes, pos_src=local[:n].astype(np.int32), pos_dst=local[n: 2 * n].astype(np.int32),
                neg_dst=local[2 * n:].reshape(n, k).astype(np.int32), n_bad=int((src < 0).sum()))


def exclude_fixed(nbr, eid, excluded):
    """Fixed block (nbr int32 [n_dst, f], eid int64 [n_dst, f], -1 padded) -> (nbr, eid) without the listed edges: survivors at the
    front of the row in their old order, -1 behind them."""
    keep = (nbr >= 0) & ~np.isin(eid, excluded)
    out_n, out_e = np.full_like(nbr, -1), np.full_like(eid, -1)
    for d in range(nbr.shape[0]):
        c = int(keep[d].sum())
        out_n[d, :c], out_e[d, :c] = nbr[d][keep[d]], eid[d][keep[d]]
    return out_n, out_e


def exclude_csr(indptr, indices, eid, excluded):
    """Ragged block -> (indptr, indices, eid) without the listed edges, in their old order."""
    keep = ~np.isin(eid, excluded)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    new = np.zeros(len(indptr), dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=len(indptr) - 1), out=new[1:])
    return new, indices[keep], eid[keep]


def with_zero_runs(indptr, indices, runs=(3, 4, 5)):
    """The same graph with runs of degree-0 nodes put at the start, in the middle and at the end: -> (indptr, indices, new id of every
    old node)."""
    N = len(indptr) - 1
    half = N // 2
    new_id = np.arange(N, dtype=np.int64) + runs[0]
    new_id[half:] += runs[1]
    deg = np.diff(indptr)
    new_deg = np.concatenate([np.zeros(runs[0], np.int64), deg[:half], np.zeros(runs[1], np.int64), deg[half:], np.zeros(runs[2], np.int64)])
    new_indptr = np.zeros(len(new_deg) + 1, dtype=np.int64)
    np.cumsum(new_deg, out=new_indptr[1:])
    return new_indptr, new_id[indices], new_id


def brute_force_rows(indptr):
    """The destination of every CSC position, by walking the rows."""
    rows = np.empty(int(indptr[-1]), dtype=np.int64)
    for v in range(len(indptr) - 1):
        rows[indptr[v]: indptr[v + 1]] = v
    return rows


def link_graph(n_plain=2000, hub_degree=5000, seed=0):
    """The graph of the GPU tests: edge_case_graph's degree classes for the fan-outs 1, 5 and 32, n_plain plain nodes, a hub, and
    degree-0 runs at the start, in the middle and at the end.  -> (indptr, indices, hub node)."""
    ip, ix, special = edge_case_graph([1, 5, 32], n_plain=n_plain, hub_degree=hub_degree, seed=seed)
    ip, ix, new_id = with_zero_runs(ip, ix)
    return ip, ix, int(new_id[special[-1]])


def symmetric_graph(num_nodes, avg_degree, seed=0):
    """A symmetric simple graph (no self-loops, no repeats) in CSC form, rows sorted by source: -> (indptr, indices)."""
    rng = np.random.default_rng(seed)
    m = num_nodes * avg_degree // 2
    u, v = rng.integers(0, num_nodes, size=m), rng.integers(0, num_nodes, size=m)
    u, v = u[u != v], v[u != v]
    key = np.unique(np.concatenate([u * num_nodes + v, v * num_nodes + u]))      # sorted by (dst, src) with dst = key // N
    dst, src = key // num_nodes, key % num_nodes
    indptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=num_nodes), out=indptr[1:])
    return indptr, src.astype(np.int64)


def large_graph(num_nodes=300_007, avg_degree=6, hub_degree=4000, seed=0):
    """The graph of the item-batch limit tests: symmetric_graph, then a few nodes lose every in-edge (the first, the last, three in the
    middle) and one hub gains in-edges up to about hub_degree; rows rebuilt sorted by source.  Large enough that the negatives of a batch
    of millions are mostly distinct.  -> (indptr, indices, hub node, the degree-0 nodes)."""
    ip, ix = symmetric_graph(num_nodes, avg_degree, seed=seed)
    rng = np.random.default_rng(seed + 1)
    zeros = np.array([0, num_nodes // 3, num_nodes // 3 + 1, num_nodes // 2, num_nodes - 1], dtype=np.int64)
    hub = num_nodes // 5
    dst = np.repeat(np.arange(num_nodes, dtype=np.int64), np.diff(ip))
    keep = ~np.isin(dst, zeros)
    extra = rng.choice(num_nodes, size=hub_degree, replace=False).astype(np.int64)
    key = np.unique(np.concatenate([dst[keep] * num_nodes + ix[keep], hub * num_nodes + extra]))     # sorted by (dst, src), no repeats
    indptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // num_nodes, minlength=num_nodes), out=indptr[1:])
    return indptr, (key % num_nodes).astype(np.int64), hub, zeros


__all__ = ["splitmix64", "sample_key", "endpoints", "negatives", "negatives_vec", "compact", "edge_batch", "large_graph", "exclude_fixed", "exclude_csr", "with_zero_runs",
           "brute_force_rows", "link_graph", "symmetric_graph", "csc_from_columns", "K_NEG", "K_OTHERS", "CHI2_63_BOUND"]
