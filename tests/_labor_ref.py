"""Plain numpy restatement of a LABOR sampler layer (LaborSampler, importance_sampling=0), the reference of the LABOR tests.

Contract (coala_sampler.hip header): sampled layer l with fan-out k; destination d (node v) with in-degree deg and the in-edge at CSC
position e = indptr[v] + j from source t = indices[e].  deg <= k takes every in-edge; otherwise the edge is taken iff
    mulhi64(r_t, deg) < k,   r_t = splitmix64(labor_key(seed, step, l) ^ t),
    labor_key = splitmix64(splitmix64(seed ^ GOLD * (l + 1)) ^ step * 0xD1B54A32D192ED03) ^ STREAM
(layer_dependency: the first round hashes `seed` alone, so every layer has the same key).  All in exact integer arithmetic.  The block
is CSR: taken edges in ascending CSC position inside a row, rows in destination order; the source list is the destination nodes, then
every other taken neighbour in order of first appearance in the row-major scan (the logic of _full_ref.full_layer).  An out-of-range
destination id gives an empty row.  A -1 layer is _full_ref.full_layer."""
import numpy as np

from _full_ref import full_layer

M64 = (1 << 64) - 1
STREAM = 0xBB67AE8584CAA73B
_GOLD = 0x9E3779B97F4A7C15
_STEP = 0xD1B54A32D192ED03
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def splitmix64_int(x):
    """One value, in Python integers."""
    x = (x + _GOLD) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def splitmix64(x):
    """x: uint64 array (wrapping arithmetic)"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=np.uint64) + np.uint64(_GOLD)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def mulhi64(a, b):
    """High 64 bits of the 128-bit product of uint64 arrays, in 32-bit halves (no partial sum overflows 64 bits)."""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    a0, a1 = a & _LOW, a >> _S32
    b0, b1 = b & _LOW, b >> _S32
    lo = a0 * b0
    m1 = a1 * b0 + (lo >> _S32)            # <= (2^32-1)^2 + 2^32 - 1 < 2^64
    m2 = a0 * b1 + (m1 & _LOW)
    return a1 * b1 + (m1 >> _S32) + (m2 >> _S32)


def labor_key(seed, step, layer, layer_dependency=False):
    h = splitmix64_int(seed & M64 if layer_dependency else (seed ^ (_GOLD * (layer + 1))) & M64)
    h = splitmix64_int((h ^ (step * _STEP)) & M64)
    return h ^ STREAM


def source_draws(key, t):
    """r_t of an array of source node ids."""
    return splitmix64(np.uint64(key) ^ np.asarray(t, dtype=np.int64).astype(np.uint64))


def taken_mask(key, t, deg, k):
    """The rule, per edge: t its source node, deg the in-degree of its row."""
    deg = np.asarray(deg, dtype=np.int64)
    return (deg <= k) | (mulhi64(source_draws(key, t), deg.astype(np.uint64)) < np.uint64(k))


def taken_mask_slow(key, t, deg, k):
    """The same in Python integers (cross-check of the vectorised form)."""
    out = np.zeros(len(t), dtype=bool)
    for i, (ti, di) in enumerate(zip(np.asarray(t).tolist(), np.asarray(deg).tolist())):
        r = splitmix64_int((key ^ (ti & M64)) & M64)
        out[i] = di <= k or ((r * di) >> 64) < k
    return out


def compact_ragged(dst, taken_nodes):
    """Source list of a ragged block (dst nodes, then the others in order of first appearance) and the local index of every edge."""
    items = np.concatenate([np.asarray(dst, dtype=np.int64), np.asarray(taken_nodes, dtype=np.int64)])
    uniq, first, inv = np.unique(items, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    return uniq[order], rank[inv.reshape(-1)[len(dst):]].astype(np.int32)


def labor_layer(indptr, indices, dst, k, key):
    """-> (src int64[n_src], indptr_local int64[n_dst + 1], nbr_local int32[E], eid int64[E])"""
    dst = np.asarray(dst, dtype=np.int64)
    n, N = len(dst), len(indptr) - 1
    ok = (dst >= 0) & (dst < N)
    v = np.where(ok, dst, 0)
    starts = np.where(ok, indptr[v], 0)
    deg = np.where(ok, indptr[v + 1] - indptr[v], 0)
    run = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=run[1:])
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    pos = starts[rows] + np.arange(int(run[-1]), dtype=np.int64) - run[rows]
    take = taken_mask(key, indices[pos], deg[rows], k)
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[take], minlength=n), out=ip[1:])
    eid = pos[take]
    src, loc = compact_ragged(dst, indices[eid])
    return src, ip, loc, eid


def reference_layers(indptr, indices, seeds, fanouts_reversed, seed, step, layer_dependency=False):
    """Every layer of a LABOR list, in sampling order: [(src, indptr_local, nbr_local, eid), ...]"""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int64)
    dst = np.asarray(seeds, dtype=np.int64)
    out = []
    for layer, k in enumerate(fanouts_reversed):
        if k == -1:
            src, ip, loc = full_layer(indptr, indices, dst)
            eid = np.repeat(indptr[dst] - ip[:-1], np.diff(ip)) + np.arange(int(ip[-1]), dtype=np.int64)
        else:
            src, ip, loc, eid = labor_layer(indptr, indices, dst, k, labor_key(seed, step, layer, layer_dependency))
        out.append((src, ip, loc, eid))
        dst = src
    return out


def edge_weights(ip):
    """edata['edge_weights'] of a block: 1 / (edges of the row), fp32, per edge."""
    deg = np.diff(ip)
    with np.errstate(divide="ignore"):
        return np.repeat((np.float32(1.0) / deg.astype(np.float32)).astype(np.float32), deg)
