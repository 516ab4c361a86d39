"""Python-integer restatement of the metapath walks (coala_sampler.hip header), the reference of the metapath tests.  Rows are sorted by
edge type.  Hop h from u uses r = metapath[h % M]: lo / hi = the first positions of u's row whose type is >= r / >= r + 1 (bisect), deg_r
= max(hi - lo, 0); deg_r == 0 ends the walk, else the next node is indices[lo + mulhi64(draw, deg_r)], `draw` the untyped walk's draw of
that hop.  Short walks: _pinsage_ref's keys, counters c = 2 (16 w + h), step draw splitmix64(wkey + c + 1), termination draw
(splitmix64(wkey + c) >> 11) < thr only at h >= M with h % M == 0; a layer makes M * R hops and records those with (h + 1) % M == 0.
Walk batches: _node2vec_ref's keys, step draw splitmix64(kw + 2 (256 h)), no termination, its negatives and compaction."""
import bisect

import numpy as np

import _node2vec_ref as RW
import _pinsage_ref as RP
from _edge_batch_ref import compact
from _labor_ref import M64, splitmix64_int


class TypedGraph(object):
    def __init__(self, indptr, indices, etype):
        self.ip, self.ix, self.et = (np.asarray(a).tolist() for a in (indptr, indices, etype))
        self.N = len(self.ip) - 1

    def step(self, u, r, draw):
        """The node a hop of type r from u reaches with `draw`, or None when the walk ends."""
        lo = bisect.bisect_left(self.et, r, self.ip[u], self.ip[u + 1])
        deg = max(bisect.bisect_left(self.et, r + 1, self.ip[u], self.ip[u + 1]) - lo, 0)
        x = self.ix[lo + RW.mulhi(draw, deg)] if deg else -1
        return x if 0 <= x < self.N else None


def _walks(G, nodes, metapath, T, W, key, stops, draw):
    """-> int64 [n, W, T + 1]: walk w of v has key(v, w), ends before hop h when stops(k, w, h), and steps with draw(k, w, h).  A repeated
    start node has the same walks, one outside the graph rows of -1."""
    out = np.full((len(nodes), W, T + 1), -1, dtype=np.int64)
    memo = {}
    for i, v in enumerate(np.asarray(nodes).tolist()):
        if 0 <= v < G.N and v not in memo:
            memo[v] = np.full((W, T + 1), -1, dtype=np.int64)
            for w in range(W):
                k, u = key(v, w), v
                memo[v][w, 0] = v
                for h in range(T):
                    u = None if stops(k, w, h) else G.step(u, metapath[h % len(metapath)], draw(k, w, h))
                    if u is None:
                        break
                    memo[v][w, h + 1] = u
        if v in memo:
            out[i] = memo[v]
    return out


def traces(G, nodes, metapath, T, W, thr, seed, step, layer=0):
    """random_walk(metapath=): T hops, a multiple of M."""
    outer, M = RP._outer_key(seed, step, layer), len(metapath)
    return _walks(G, nodes, metapath, T, W, lambda v, w: splitmix64_int((outer ^ v) & M64) ^ RP.STREAM,
                  lambda k, w, h: h >= M and h % M == 0 and (splitmix64_int((k + 2 * (16 * w + h)) & M64) >> 11) < thr,
                  lambda k, w, h: splitmix64_int((k + 2 * (16 * w + h) + 1) & M64))


def reference_layers(G, seeds, ks_reversed, metapath, R, W, thr, seed, step):
    """Every layer of a typed walk sampler in sampling order: [(src, nbr_local, counts, nbr), ...] as _pinsage_ref.reference_layers."""
    dst, out, M = np.asarray(seeds, dtype=np.int64), [], len(metapath)
    for layer, k in enumerate(ks_reversed):
        tr = traces(G, dst, metapath, M * R, W, thr, seed, step, layer)
        nbr, cnt = RP.select(tr[:, :, ::M], k)      # columns M, 2M, ..: the hops that complete a repetition (select drops column 0)
        src, loc = RP.compact_fixed(dst, nbr)
        out.append((src, loc, cnt, nbr))
        dst = src
    return out


def walk_batch(G, nodes, metapath, L, W, K, seed, step):
    """walk_batch(metapath=) -> dict(input_nodes, pos int32 [n W, L + 1], neg int32 [n W K, L + 1], traces int64 [n, W, L + 1], n_bad)."""
    nodes = np.asarray(nodes, dtype=np.int64)
    n, outer = len(nodes), RW._outer_key(seed, step)
    tr = _walks(G, nodes, metapath, L, W, lambda v, w: RW.walk_key(outer, v, w), lambda k, w, h: False,
                lambda k, w, h: splitmix64_int((k + 2 * RW.ATTEMPTS * h) & M64))
    ng = RW.negatives_vec(nodes, G.N, L, W, K, seed, step)
    ok = (nodes >= 0) & (nodes < G.N)
    input_nodes, local = compact(np.concatenate([np.where(ok, nodes, -1), tr.reshape(-1), ng[:, 1:].reshape(-1)]))
    local, n_pos = local.astype(np.int32), n * W * (L + 1)
    neg = np.concatenate([np.repeat(local[:n], W * K)[:, None], local[n + n_pos:].reshape(n * W * K, L)], axis=1)
    return dict(input_nodes=input_nodes, pos=local[n: n + n_pos].reshape(n * W, L + 1), neg=neg, traces=tr, n_bad=int((~ok).sum()))
