"""Plain numpy restatement of a relation layer (RelNeighborSampler: a fan-out per edge type), the reference of the relation-sampler tests.

Contract (coala_sampler.hip header).  The graph is a CSC with an edge type in [0, R) per edge, non-decreasing inside every row, so the
in-edges of relation r of node v are one segment [s_r, s_r + deg_r) of the row.  Sampled layer l with fan-outs f_0 .. f_{R-1}:
    f_r == 0                  nothing of relation r;
    f_r == -1 or deg_r <= f_r every edge of the segment;
    otherwise                 f_r distinct positions of the segment by Floyd's algorithm: for c = 0 .. f_r - 1, j = deg_r - f_r + c,
                              t = mulhi64(splitmix64(sample_key(seed, step, l, v) + 64 r + c), j + 1), and the pick is t unless an earlier
                              pick equals t, then j.  sample_key is the uniform sampler's per-row key.
The block is CSR: taken edges in ascending CSC position inside a row, rows in destination order; the source list is the destination
nodes, then every other taken neighbour in order of first appearance in the row-major scan (the logic of _full_ref.full_layer).  An
out-of-range destination id gives an empty row.  Everything is exact integer arithmetic."""
import numpy as np

M64 = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15
_STEP = 0xD1B54A32D192ED03
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def splitmix64_int(x):
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
    m1 = a1 * b0 + (lo >> _S32)
    m2 = a0 * b1 + (m1 & _LOW)
    return a1 * b1 + (m1 >> _S32) + (m2 >> _S32)


def sample_key(seed, step, layer, v):
    """The uniform sampler's per-row key, for an array of node ids v."""
    h = splitmix64_int((seed ^ (_GOLD * (layer + 1))) & M64)
    h = splitmix64_int((h ^ (step * _STEP)) & M64)
    return splitmix64(np.uint64(h) ^ np.asarray(v, dtype=np.int64).astype(np.uint64))


def floyd_picks(key, r, deg, f):
    """Rows with deg > f (arrays key uint64, deg int64): -> int64 [n, f] positions relative to the segment's start, in draw order."""
    n = len(deg)
    chosen = np.empty((n, f), dtype=np.int64)
    with np.errstate(over="ignore"):
        for c in range(f):
            j = deg - f + c
            t = mulhi64(splitmix64(key + np.uint64(64 * r + c)), (j + 1).astype(np.uint64)).astype(np.int64)
            dup = (chosen[:, :c] == t[:, None]).any(1)
            chosen[:, c] = np.where(dup, j, t)
    return chosen


def floyd_picks_slow(key, r, deg, f):
    """One row in Python integers (cross-check of the vectorised form)."""
    out = []
    for c in range(f):
        j = deg - f + c
        t = (splitmix64_int((key + 64 * r + c) & M64) * (j + 1)) >> 64
        out.append(j if t in out else t)
    return out


def type_index(indptr, etype, num_rels):
    """row * num_rels + type per edge: non-decreasing over the whole array when the types are sorted inside every row."""
    deg = np.diff(indptr)
    return np.repeat(np.arange(len(deg), dtype=np.int64), deg) * num_rels + np.asarray(etype, dtype=np.int64)


def compact_ragged(dst, taken_nodes):
    """Source list of a ragged block (dst nodes, then the others in order of first appearance) and the local index of every edge."""
    items = np.concatenate([np.asarray(dst, dtype=np.int64), np.asarray(taken_nodes, dtype=np.int64)])
    uniq, first, inv = np.unique(items, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    return uniq[order], rank[inv.reshape(-1)[len(dst):]].astype(np.int32)


def rel_layer(indptr, indices, etype, dst, fan, seed, step, layer, tindex=None):
    """fan: the num_rels fan-outs of the layer.  -> (src int64[n_src], indptr_local int64[n_dst + 1], nbr_local int32[E], eid int64[E])"""
    R = len(fan)
    dst = np.asarray(dst, dtype=np.int64)
    n, N = len(dst), len(indptr) - 1
    if tindex is None:
        tindex = type_index(indptr, etype, R)
    ok = (dst >= 0) & (dst < N)
    v = np.where(ok, dst, 0)
    key = sample_key(seed, step, layer, dst)
    rows_all, eid_all = [], []
    for r, f in enumerate(fan):
        if f == 0:
            continue
        s = np.searchsorted(tindex, v * R + r, side="left")
        deg = np.where(ok, np.searchsorted(tindex, v * R + r + 1, side="left") - s, 0)
        whole = np.nonzero((deg > 0) & ((deg <= f) | (f < 0)))[0]
        if len(whole):
            d = deg[whole]
            run = np.concatenate([[0], np.cumsum(d)])
            rows_all.append(np.repeat(whole, d))
            eid_all.append(np.repeat(s[whole] - run[:-1], d) + np.arange(int(run[-1]), dtype=np.int64))
        drawn = np.nonzero(deg > f)[0] if f > 0 else np.zeros(0, dtype=np.int64)
        if len(drawn):
            picks = floyd_picks(key[drawn], r, deg[drawn], f)
            rows_all.append(np.repeat(drawn, f))
            eid_all.append((s[drawn][:, None] + picks).reshape(-1))
    rows = np.concatenate(rows_all) if rows_all else np.zeros(0, dtype=np.int64)
    eid = np.concatenate(eid_all) if eid_all else np.zeros(0, dtype=np.int64)
    order = np.lexsort((eid, rows))
    rows, eid = rows[order], eid[order]
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ip[1:])
    src, loc = compact_ragged(dst, indices[eid])
    return src, ip, loc, eid


def expand_fanouts(fanouts, num_rels):
    """RelNeighborSampler's fan-out list (model order; an int is applied to every relation) -> per layer a list of num_rels ints."""
    return [[int(x) for x in f] if hasattr(f, "__iter__") else [int(f)] * num_rels for f in fanouts]


def reference_layers(indptr, indices, etype, seeds, rel_fanouts_reversed, seed, step):
    """Every layer of a relation list, in sampling order: [(src, indptr_local, nbr_local, eid), ...]"""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int64)
    R = len(rel_fanouts_reversed[0])
    tindex = type_index(indptr, etype, R)
    dst = np.asarray(seeds, dtype=np.int64)
    out = []
    for layer, fan in enumerate(rel_fanouts_reversed):
        out.append(rel_layer(indptr, indices, etype, dst, fan, seed, step, layer, tindex))
        dst = out[-1][0]
    return out


def sort_by_type(indptr, etype):
    """numpy's statement of sort_csc_by_etype: the stable order by (row, type) -> perm (new position -> old position)."""
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return np.lexsort((np.arange(len(rows)), np.asarray(etype), rows))


def typed_edge_case_graph(fanouts=(1, 5, 32), num_rels=3, n_plain=200, hub_degree=0, seed=0):
    """A typed CSC graph built around the sampler's edges.  For every fan-out f, every degree d in {0, f-1, f, f+1, 2f, 200} and every
    relation r there are three nodes whose relation-r segment has d edges (drawn at random; with the node itself among them; with one
    neighbour in half of them) and whose other relations have 0..3 edges each -- so rows lacking the first, a middle or the last
    relation occur (d = 0, and the small segments), and one node has no in-edge at all.  Then n_plain nodes with 0..4 edges per
    relation, and with hub_degree > 0 a last node whose relation 1 has that many edges beside 2 edges of the last relation and none
    of relation 0.  The types are sorted inside every row by construction.
    -> (indptr, indices, etype int64, special): special = every node above except the plain ones (hub included)."""
    rng = np.random.default_rng(seed)
    degrees = sorted({0, 200} | {d for f in fanouts for d in (f - 1, f, f + 1, 2 * f) if d >= 0})
    n_special = 3 * len(degrees) * num_rels + 1
    n = n_special + n_plain + (1 if hub_degree else 0)
    cols, types = [], []

    def add(per_rel):
        cols.append(np.concatenate(per_rel).astype(np.int64) if per_rel else np.zeros(0, dtype=np.int64))
        types.append(np.repeat(np.arange(len(per_rel)), [len(c) for c in per_rel]))

    for d in degrees:
        for r in range(num_rels):
            for kind in range(3):
                v = len(cols)
                per_rel = [rng.integers(0, n, size=rng.integers(0, 4)) for _ in range(num_rels)]
                seg = rng.integers(0, n, size=d)
                if d and kind == 1:
                    seg[rng.integers(0, d)] = v                        # self-loop
                if d > 1 and kind == 2:
                    seg[rng.permutation(d)[: d // 2 + 1]] = seg[0]     # one neighbour in half the segment
                per_rel[r] = seg
                add(per_rel)
    add([np.zeros(0, dtype=np.int64)] * num_rels)                      # total degree 0
    for _ in range(n_plain):
        add([rng.integers(0, n, size=rng.integers(0, 5)) for _ in range(num_rels)])
    if hub_degree:
        per_rel = [np.zeros(0, dtype=np.int64) for _ in range(num_rels)]
        per_rel[min(1, num_rels - 1)] = rng.integers(0, n, size=hub_degree)
        if num_rels > 2:
            per_rel[num_rels - 1] = rng.integers(0, n, size=2)
        add(per_rel)
    deg = np.array([len(c) for c in cols], dtype=np.int64)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    special = np.arange(n_special, dtype=np.int64)
    if hub_degree:
        special = np.append(special, n - 1)
    return indptr, np.concatenate(cols), np.concatenate(types).astype(np.int64), special
