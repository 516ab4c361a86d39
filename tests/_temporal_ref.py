"""Plain numpy restatement of a temporal layer (TemporalNeighborSampler), the reference of the temporal-sampler tests.

Contract (coala_sampler.hip header).  The graph is a CSC with an int64 timestamp per edge, non-decreasing inside every row.  A destination
item is a pair (v, t), carried as the int64 code slot << node_bits | v: slot indexes slot_time (the distinct query times of the call,
ascending), node_bits is the bit length of num_nodes.  A code that is negative or decodes to slot >= n_slots or v >= num_nodes gives an
empty row.  For a valid pair:
    m                 number of the row's edges with ts < t (inclusive: ts <= t); the eligible edges are the first m of the row;
    m <= f            the m eligible edges in CSC order, then -1;
    uniform, m > f    Floyd: for c = 0 .. f - 1, j = m - f + c, x = mulhi64(splitmix64(key + c), j + 1), the pick is x unless an earlier
                      pick equals x, then j; key = sample_key(seed, step, layer, v) ^ splitmix64(uint64(t) ^ K_TEMPORAL);
    last, m > f       positions m - f .. m - 1.
Slot c of the row holds the code (row's slot) << node_bits | indices[e] and the edge id e.  The source list is the destination codes, then
every other code in order of first appearance in the row-major scan; nbr_local is the index of every slot's code in it, -1 on padding.
Everything is exact integer arithmetic."""
import numpy as np

from _rel_fanout_ref import M64, mulhi64, sample_key, splitmix64, splitmix64_int

K_TEMPORAL = 0xBB67AE8584CAA73B


def node_bits_of(num_nodes):
    return int(num_nodes).bit_length()


def encode(nodes, times, num_nodes):
    """(node, time) pairs -> (codes, slot_time), as the wrapper makes them: slot_time the sorted distinct times, a node outside the graph
    coded with the node field num_nodes."""
    nodes = np.asarray(nodes, dtype=np.int64)
    slot_time, slot = np.unique(np.asarray(times, dtype=np.int64), return_inverse=True)
    field = np.where((nodes >= 0) & (nodes < num_nodes), nodes, num_nodes)
    return (slot.reshape(-1).astype(np.int64) << node_bits_of(num_nodes)) | field, slot_time


def decode(codes, slot_time, num_nodes):
    """codes -> (node field, query time)"""
    bits = node_bits_of(num_nodes)
    codes = np.asarray(codes, dtype=np.int64)
    return codes & ((1 << bits) - 1), slot_time[codes >> bits]


def temporal_key(seed, step, layer, v, t):
    """Per-pair key of the uniform strategy, for arrays v, t."""
    tk = splitmix64(np.asarray(t, dtype=np.int64).astype(np.uint64) ^ np.uint64(K_TEMPORAL))
    return sample_key(seed, step, layer, v) ^ tk


def floyd(key, m, f):
    """Rows with m > f (arrays key uint64, m int64): -> int64 [n, f] positions in draw order (the uniform sampler's loop, deg := m)."""
    chosen = np.empty((len(m), f), dtype=np.int64)
    with np.errstate(over="ignore"):
        for c in range(f):
            j = m - f + c
            x = mulhi64(splitmix64(key + np.uint64(c)), (j + 1).astype(np.uint64)).astype(np.int64)
            dup = (chosen[:, :c] == x[:, None]).any(1)
            chosen[:, c] = np.where(dup, j, x)
    return chosen


def floyd_slow(key, m, f):
    """One row in Python integers (cross-check of the vectorised form)."""
    out = []
    for c in range(f):
        j = m - f + c
        x = (splitmix64_int((int(key) + c) & M64) * (j + 1)) >> 64
        out.append(j if x in out else x)
    return out


def row_index(indptr, ts):
    """A key that is non-decreasing over the whole edge array when the times are sorted inside every row: (row, rank of the time)."""
    deg = np.diff(indptr)
    uniq = np.unique(ts)
    return np.repeat(np.arange(len(deg), dtype=np.int64), deg) * (len(uniq) + 1) + np.searchsorted(uniq, ts), uniq


def eligible(indptr, ts, v, t, inclusive, index=None):
    """m for arrays of valid nodes v and times t: a lower (inclusive: upper) bound of t among the row's timestamps."""
    tindex, uniq = index if index is not None else row_index(indptr, ts)
    # rank of t among the distinct timestamps: edges with ts < t are those of rank < lower bound, ts <= t those of rank < upper bound
    rank = np.searchsorted(uniq, t, side="right" if inclusive else "left")
    return np.searchsorted(tindex, v * (len(uniq) + 1) + rank, side="left") - indptr[v]


def temporal_layer(indptr, indices, ts, codes, slot_time, f, seed, step, layer, strategy="uniform", inclusive=False, index=None):
    """-> (src codes int64[n_src], nbr_local int32[n, f], eid int64[n, f])"""
    N = len(indptr) - 1
    bits = node_bits_of(N)
    codes = np.asarray(codes, dtype=np.int64)
    n = len(codes)
    slot, v = codes >> bits, codes & ((1 << bits) - 1)
    ok = (codes >= 0) & (slot < len(slot_time)) & (v < N)
    vv = np.where(ok, v, 0)
    t = np.where(ok, slot_time[np.where(ok, slot, 0)] if len(slot_time) else 0, 0).astype(np.int64)
    m = np.where(ok, eligible(indptr, ts, vv, t, inclusive, index), 0)
    pos = np.full((n, f), -1, dtype=np.int64)
    small = m <= f
    lane = np.arange(f, dtype=np.int64)[None, :]
    pos[small] = np.where(lane < m[small][:, None], lane, -1)
    big = np.nonzero(~small)[0]
    if len(big):
        if strategy == "last":
            pos[big] = m[big][:, None] - f + lane
        else:
            pos[big] = floyd(temporal_key(seed, step, layer, vv[big], t[big]), m[big], f)
    eid = np.where(pos >= 0, indptr[vv][:, None] + pos, -1)
    taken = np.where(pos >= 0, (slot[:, None] << bits) | indices[np.maximum(eid, 0)], -1)
    items = np.concatenate([codes, taken.reshape(-1)])
    keep = items >= 0
    uniq, first, inv = np.unique(items[keep], return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    local = np.full(len(items), -1, dtype=np.int64)
    local[keep] = rank[inv.reshape(-1)]
    return uniq[order], local[n:].reshape(n, f).astype(np.int32), eid


def reference_layers(indptr, indices, ts, nodes, times, fanouts_reversed, seed, step, strategy="uniform", inclusive=False, index=None):
    """Every layer of a call over the pairs (nodes, times), in sampling order: [(src codes, nbr_local, eid), ...], and slot_time."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int64)
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    if index is None:
        index = row_index(indptr, ts)
    codes, slot_time = encode(nodes, times, len(indptr) - 1)
    out = []
    for layer, f in enumerate(fanouts_reversed):
        out.append(temporal_layer(indptr, indices, ts, codes, slot_time, f, seed, step, layer, strategy, inclusive, index))
        codes = out[-1][0]
    return out, slot_time


def sort_by_time(indptr, ts):
    """numpy's statement of sort_csc_by_time: the stable order by (row, time) -> perm (new position -> old position)."""
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return np.lexsort((np.arange(len(rows)), np.asarray(ts), rows))


def edge_case_graph(f=5, hub_degree=0, n_plain=100, t_max=1000, seed=0):
    """A timed CSC graph around the sampler's edges: rows of degree 0, f, f + 1, 63, 64, 65, a row whose timestamps are all equal, a row
    that holds one neighbour many times, n_plain rows of degree 0..12 and, with hub_degree > 0, a last row of that many edges whose
    timestamps run 0, 0, 1, 1, 2, ... (every value twice).  Times are sorted inside every row.
    -> (indptr, indices, ts, named): named maps 'deg0', 'f', 'f1', '63', '64', '65', 'equal', 'repeat', 'hub' to node ids."""
    rng = np.random.default_rng(seed)
    degs = [("deg0", 0), ("f", f), ("f1", f + 1), ("63", 63), ("64", 64), ("65", 65), ("equal", 40), ("repeat", 40)]
    n = len(degs) + n_plain + (1 if hub_degree else 0)
    cols, times, named = [], [], {}
    for v, (name, d) in enumerate(degs):
        named[name] = v
        c = rng.integers(0, n, size=d)
        t = np.sort(rng.integers(0, t_max, size=d))
        if name == "equal":
            t[:] = t_max // 2
        if name == "repeat":
            c[::2] = 3
        cols.append(c)
        times.append(t)
    for _ in range(n_plain):
        d = int(rng.integers(0, 13))
        cols.append(rng.integers(0, n, size=d))
        times.append(np.sort(rng.integers(0, t_max, size=d)))
    if hub_degree:
        named["hub"] = n - 1
        cols.append(rng.integers(0, n, size=hub_degree))
        times.append(np.arange(hub_degree, dtype=np.int64) // 2)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cols], out=indptr[1:])
    return indptr, np.concatenate(cols).astype(np.int64), np.concatenate(times).astype(np.int64), named
