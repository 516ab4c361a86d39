"""References for the edge ids of sampled blocks (tests only): the CSC position of every neighbour slot.

A full layer's ids are arange(indptr[v], indptr[v + 1]) per destination node; a weighted fixed layer's are indptr[v] + the positions
_weighted_ref.weighted_layer chose; a uniform fixed layer's are recovered from the CPU twin's sampled neighbours on a graph without
repeated edges, where (destination, neighbour) names one position."""
import numpy as np

from _full_ref import fixed_layer
from _weighted_ref import weighted_layer


def full_ids(indptr, dst):
    """int64[E]: the positions of every in-edge of dst[0], dst[1], ... in CSC order"""
    dst = np.asarray(dst, dtype=np.int64)
    deg = indptr[dst + 1] - indptr[dst]
    run = np.zeros(len(dst), dtype=np.int64)
    np.cumsum(deg[:-1], out=run[1:])
    return np.repeat(indptr[dst] - run, deg) + np.arange(int(deg.sum()), dtype=np.int64)


def weighted_ids(indptr, indices, w, dst, f, seed, step, layer):
    """-> (int64[n_dst, f] ids, -1 padded; margins of the rows: see _weighted_ref.select)"""
    dst = np.asarray(dst, dtype=np.int64)
    _, _, pos, margin = weighted_layer(indptr, indices, w, dst, f, seed, step, layer)
    return np.where(pos >= 0, indptr[dst][:, None] + pos, -1), margin


def uniform_ids(oracle, indptr, indices, dst, f, seed, step, layer):
    """int64[n_dst, f] ids of the twin's uniform fixed layer, -1 padded.  Needs a graph without repeated edges."""
    dst = np.asarray(dst, dtype=np.int64)
    N = len(indptr) - 1
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(indptr))
    key = rows * N + indices
    order = np.argsort(key, kind="stable")
    skey = key[order]
    assert len(skey) < 2 or np.all(skey[1:] != skey[:-1]), "uniform_ids needs a graph without repeated edges"
    src, loc = fixed_layer(oracle, indptr, indices, dst, f, seed, step, layer)
    nb = np.where(loc >= 0, src[np.maximum(loc, 0)], -1)
    want = dst[:, None] * N + nb
    at = np.minimum(np.searchsorted(skey, want), max(len(skey) - 1, 0))
    assert np.all((skey[at] == want) | (nb < 0)), "the twin sampled a neighbour that is not in the column"
    return np.where(nb >= 0, order[at], -1)
