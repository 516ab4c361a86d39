"""Plain numpy / Python-integer restatement of a random-walk sampler layer (RandomWalkNeighborSampler, DGL's PinSAGESampler on a
homogeneous graph) and of random_walk, the reference of the PinSAGE tests.

Contract (coala_sampler.hip header): sampled layer l keeps k = num_neighbors nodes per destination node, found by W = num_random_walks
walks of T = num_traversals hops, with the termination threshold thr = floor(termination_prob * 2^53).  For destination node v (a node
of the graph):
    wkey = sample_key(seed, step, l, v) ^ STREAM
    walk w starts at u = v; hop h = 0 .. T-1, c = 2 (16 w + h):
        h >= 1 and (splitmix64(wkey + c) >> 11) < thr            -> the walk ends
        deg = indptr[u+1] - indptr[u] == 0                        -> the walk ends
        u = indices[indptr[u] + mulhi64(splitmix64(wkey + c + 1), deg)], a recorded visit
count(u) = recorded visits of u over the W walks; the row takes the min(k, distinct) nodes of largest count, a tie to the smaller id,
in that order, then -1; the visit count of a slot is int32, 0 on padding.  An out-of-range destination id gives an empty row.  The
source list is the destination nodes, then every other chosen node in order of first appearance in the row-major slot scan (negative
ids are not listed, a repeated id is listed once: what the hash table of the kernels does).  All in exact integer arithmetic."""
import numpy as np

from _labor_ref import M64, mulhi64, splitmix64, splitmix64_int

STREAM = 0x3C6EF372FE94F82B
_GOLD = 0x9E3779B97F4A7C15
_STEP = 0xD1B54A32D192ED03


def threshold(termination_prob):
    """floor(p * 2^53): the product of a double in [0, 1) and a power of two is exact."""
    return int(float(termination_prob) * 9007199254740992.0)


def _outer_key(seed, step, layer):
    h = splitmix64_int(((seed & M64) ^ (_GOLD * (layer + 1))) & M64)
    return splitmix64_int((h ^ ((step & M64) * _STEP)) & M64)


def walk_keys(seed, step, layer, v):
    """wkey of an array of node ids (uint64)."""
    return splitmix64(np.uint64(_outer_key(seed, step, layer)) ^ np.asarray(v, dtype=np.int64).astype(np.uint64)) ^ np.uint64(STREAM)


def traces(indptr, indices, nodes, W, T, thr, seed, step, layer=0):
    """-> int64 [n, W, T + 1]: [i, w, 0] = nodes[i], then the visits of walk w, -1 once ended; an out-of-range start gives -1 throughout."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    nodes = np.asarray(nodes, dtype=np.int64)
    n, N = len(nodes), len(indptr) - 1
    ok = (nodes >= 0) & (nodes < N)
    out = np.full((n, W, T + 1), -1, dtype=np.int64)
    out[ok, :, 0] = nodes[ok, None]
    wkey = walk_keys(seed, step, layer, np.where(ok, nodes, 0))
    with np.errstate(over="ignore"):
        for w in range(W):
            u = np.where(ok, nodes, 0)
            ended = ~ok
            for h in range(T):
                c = np.uint64(2 * (16 * w + h))
                if h >= 1:
                    ended = ended | ((splitmix64(wkey + c) >> np.uint64(11)) < np.uint64(thr))
                start = indptr[u]
                deg = indptr[u + 1] - start
                ended = ended | (deg == 0)
                off = mulhi64(splitmix64(wkey + c + np.uint64(1)), np.maximum(deg, 1).astype(np.uint64)).astype(np.int64)
                nxt = indices[np.minimum(start + off, len(indices) - 1)] if len(indices) else u
                u = np.where(ended, u, nxt)
                out[:, w, 1 + h] = np.where(ended, -1, u)
    return out


def traces_slow(indptr, indices, nodes, W, T, thr, seed, step, layer=0):
    """The same in Python integers (cross-check of the vectorised form)."""
    ip, ix = np.asarray(indptr).tolist(), np.asarray(indices).tolist()
    N = len(ip) - 1
    outer = _outer_key(seed, step, layer)
    out = np.full((len(nodes), W, T + 1), -1, dtype=np.int64)
    for i, v in enumerate(np.asarray(nodes).tolist()):
        if not 0 <= v < N:
            continue
        wkey = splitmix64_int((outer ^ v) & M64) ^ STREAM
        for w in range(W):
            out[i, w, 0] = v
            u = v
            for h in range(T):
                c = 2 * (16 * w + h)
                if h >= 1 and (splitmix64_int((wkey + c) & M64) >> 11) < thr:
                    break
                deg = ip[u + 1] - ip[u]
                if deg == 0:
                    break
                u = ix[ip[u] + ((splitmix64_int((wkey + c + 1) & M64) * deg) >> 64)]
                out[i, w, 1 + h] = u
    return out


def select(tr, k):
    """Rows from traces [n, W, T + 1]: -> (nbr int64 [n, k], counts int32 [n, k]): count descending, id ascending, -1 / 0 padded."""
    n = tr.shape[0]
    nbr = np.full((n, k), -1, dtype=np.int64)
    cnt = np.zeros((n, k), dtype=np.int32)
    for i in range(n):
        vis = tr[i, :, 1:].reshape(-1)
        ids, c = np.unique(vis[vis >= 0], return_counts=True)
        order = np.lexsort((ids, -c))[:k]
        nbr[i, : len(order)] = ids[order]
        cnt[i, : len(order)] = c[order]
    return nbr, cnt


def compact_fixed(dst, nbr):
    """Source list of a fixed block (dst nodes, then the others in order of first appearance; negative ids left out, repeats once) and
    the local index of every slot (-1 on padding)."""
    dst = np.asarray(dst, dtype=np.int64)
    items = np.concatenate([dst, nbr.reshape(-1)])
    keep = items >= 0
    uniq, first, inv = np.unique(items[keep], return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    loc = np.full(len(items), -1, dtype=np.int64)
    loc[keep] = rank[inv.reshape(-1)]
    return uniq[order], loc[len(dst):].reshape(nbr.shape).astype(np.int32)


def walk_layer(indptr, indices, dst, k, T, W, thr, seed, step, layer):
    """-> (src int64[n_src], nbr_local int32[n_dst, k], counts int32[n_dst, k], nbr int64[n_dst, k])"""
    nbr, cnt = select(traces(indptr, indices, dst, W, T, thr, seed, step, layer), k)
    src, loc = compact_fixed(dst, nbr)
    return src, loc, cnt, nbr


def reference_layers(indptr, indices, seeds, ks_reversed, T, W, thr, seed, step):
    """Every layer of a walk list, in sampling order: [(src, nbr_local, counts, nbr), ...]"""
    dst = np.asarray(seeds, dtype=np.int64)
    out = []
    for layer, k in enumerate(ks_reversed):
        out.append(walk_layer(indptr, indices, dst, k, T, W, thr, seed, step, layer))
        dst = out[-1][0]
    return out
