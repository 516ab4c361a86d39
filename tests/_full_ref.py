"""Plain numpy restatement of a full sampler layer (fan-out -1) and a per-layer reference for mixed fan-out lists (tests only).

A full layer draws nothing: destination d (node v) takes indices[indptr[v]:indptr[v+1]] in CSC order; the source list is the
destination nodes, then every other neighbour in order of first appearance in the row-major (d, edge) scan; the block is CSR
(indptr_local = exclusive scan of the degrees, nbr_local = local source index of each edge).  Fixed layers come from the CPU twin
(orc_sample_layer at their layer index, compacted by orc_compact_block)."""
import os

import numpy as np

THREADS = min(8, os.cpu_count() or 1)


def full_layer(indptr, indices, dst):
    """-> (src int64[n_src], indptr_local int64[n_dst + 1], nbr_local int32[E])"""
    dst = np.asarray(dst, dtype=np.int64)
    n = len(dst)
    starts, deg = indptr[dst], indptr[dst + 1] - indptr[dst]
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=ip[1:])
    E = int(ip[-1])
    pos = np.repeat(starts - ip[:-1], deg) + np.arange(E, dtype=np.int64)
    items = np.concatenate([dst, indices[pos]])
    uniq, first, inv = np.unique(items, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    return uniq[order], ip, rank[inv.reshape(-1)[n:]].astype(np.int32)


def fixed_layer(oracle, indptr, indices, dst, f, seed, step, layer):
    """The twin's layer: -> (src int64[n_src], nbr_local int32[n_dst, f])"""
    O = oracle
    dst = np.ascontiguousarray(dst, dtype=np.int64)
    nbr = np.empty(len(dst) * f, dtype=np.int64)
    O.lib().orc_sample_layer_mt(O._ptr(indptr), O._ptr(indices), len(indptr) - 1, O._ptr(dst), len(dst), int(f), int(seed), int(step),
                                int(layer), O._ptr(nbr), THREADS)
    src = np.empty(len(dst) * (f + 1), dtype=np.int64)
    local = np.empty(len(dst) * f, dtype=np.int32)
    n_src = O.lib().orc_compact_block_mt(O._ptr(dst), len(dst), O._ptr(nbr), int(f), O._ptr(src), O._ptr(local), THREADS)
    return src[:n_src].copy(), local.reshape(len(dst), f)


def reference_layers(oracle, indptr, indices, seeds, fanouts_reversed, seed, step):
    """Every layer of a mixed list, in sampling order: [(src, indptr_local or None, nbr_local), ...]"""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int64)
    dst = np.asarray(seeds, dtype=np.int64)
    out = []
    for layer, f in enumerate(fanouts_reversed):
        if f == -1:
            src, ip, loc = full_layer(indptr, indices, dst)
            out.append((src, ip, loc))
        else:
            src, loc = fixed_layer(oracle, indptr, indices, dst, f, seed, step, layer)
            out.append((src, None, loc))
        dst = src
    return out


def bucketed(ids, G):
    """Stable partition of ids by owner = id % G -> (bucketed ids, bucket sizes, new position of every old index)"""
    owner = ids % G
    perm = np.argsort(owner, kind="stable")
    new_of_old = np.empty(len(ids), dtype=np.int64)
    new_of_old[perm] = np.arange(len(ids))
    return ids[perm], np.bincount(owner, minlength=G), new_of_old

