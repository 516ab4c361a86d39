"""Shared helpers of the GPU parity tests (tests only)."""
import ctypes as C

import numpy as np


SENTINEL = np.float32(-7.25e33)   # what the padding around a guarded region holds
GUARD = 67                         # floats of sentinel behind every guarded region


def check_guards(flat, off, n):
    """flat: 1-D fp32 numpy array; asserts that everything outside flat[off : off + n] still holds SENTINEL, bit for bit."""
    pad = np.concatenate([flat[:off], flat[off + n:]])
    bad = np.flatnonzero(pad.view(np.int32) != SENTINEL.view(np.int32))
    if len(bad):
        k = int(bad[0])
        where = f"{off - k} floats before" if k < off else f"{k - off} floats after the end of"
        raise AssertionError(f"write outside the region: {len(bad)} padding floats changed, the first {where} the region")


class Guarded:
    """fp32 [rows, dim] region at float offset `off` of a torch buffer padded with SENTINEL: `off` floats before it, GUARD after.
    `fill`: a scalar or an array of the region's shape.  An odd `off` puts the region off 16-byte alignment."""

    def __init__(self, torch, rows, dim, off=0, fill=-2.0, device="cuda"):
        self.off, self.shape, self.n = off, (rows, dim), rows * dim
        self.flat = torch.full((off + self.n + GUARD,), float(SENTINEL), dtype=torch.float32, device=device)
        if np.isscalar(fill):
            self.flat[off: off + self.n] = float(fill)
        else:
            self.flat[off: off + self.n] = torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float32).reshape(-1)).to(device)

    @property
    def ptr(self):
        return self.flat.data_ptr() + 4 * self.off

    def region(self):
        """-> the region as a numpy array, after asserting that the padding around it is unchanged."""
        h = self.flat.cpu().numpy()
        check_guards(h, self.off, self.n)
        return h[self.off: self.off + self.n].reshape(self.shape)


class PinnedTable:
    """fp32 [rows, dim] table in pinned host memory visible to the GPU (the cold tier), filled on the host.
    offset (a number of floats, 0 included): the table starts that far into its allocation (1: off 16-byte alignment), and the
    allocation holds SENTINEL before it and GUARD floats of it after it (guards_intact).  offset=None: the table alone."""

    def __init__(self, P, feat, device=0, offset=None):
        from COALA_GNN_Pybind import _capi
        self._capi = _capi
        L = _capi.load()
        hp, dp = C.c_void_p(), C.c_void_p()
        padded = offset is not None
        offset = offset or 0
        total = feat.size + (offset + GUARD if padded else 0)
        _capi.check(L.coala_pinned_alloc(4 * total, device, C.byref(hp), C.byref(dp)))
        self.host_ptr, self.device_ptr = hp.value, dp.value + 4 * offset
        buf = (C.c_float * total).from_address(self.host_ptr)
        self._flat = np.frombuffer(buf, dtype=np.float32)
        self._flat[...] = SENTINEL
        self.offset = offset
        self.array = self._flat[offset: offset + feat.size].reshape(feat.shape)
        self.array[...] = feat
        self.rows, self.dim = feat.shape

    def guards_intact(self):
        check_guards(self._flat, self.offset, self.rows * self.dim)
        return True

    def data_ptr(self):  # what COALA_GNN_Manager reads from sim_buf
        return self.device_ptr

    def close(self):
        if self.host_ptr:
            self.array = self._flat = None
            self._capi.load().coala_pinned_free(self.host_ptr)
            self.host_ptr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ColorFiles:
    """color.npy / topk.npy / score.npy in a temp dir, shaped like examples/color_info_gen/generate_color_data.py:39-64."""

    def __init__(self, tmpdir, color, topk, score):
        import os
        self.color_file = os.path.join(str(tmpdir), "color.npy")
        self.topk_file = os.path.join(str(tmpdir), "topk.npy")
        self.score_file = os.path.join(str(tmpdir), "score.npy")
        np.save(self.color_file, np.ascontiguousarray(color, dtype=np.int64))
        np.save(self.topk_file, np.ascontiguousarray(topk, dtype=np.int64))
        np.save(self.score_file, np.ascontiguousarray(score, dtype=np.float64))


def synth_colors(num_rows, num_colors, topk=10, seed=0):
    rng = np.random.default_rng(seed)
    color = rng.integers(0, num_colors + 1, size=num_rows).astype(np.int64)  # 0 = uncoloured
    tk = rng.integers(0, num_colors + 1, size=(num_colors, topk)).astype(np.int64)
    sc = rng.random((num_colors, topk))
    return color, tk, sc


def csc_from_columns(columns):
    """int64 CSC (indptr[N+1], indices[E]) from explicit in-neighbour lists: columns[v] holds the in-neighbours of node v in
    CSC order.  Nothing is cleaned up: repeated entries and v itself (a self-loop) stay as given."""
    deg = np.array([len(c) for c in columns], dtype=np.int64)
    indptr = np.zeros(len(columns) + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    parts = [np.asarray(c, dtype=np.int64).reshape(-1) for c in columns if len(c)]
    indices = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return indptr, indices


def edge_case_graph(fanouts, n_plain=200, hub_degree=0, seed=0):
    """A CSC graph built around the sampler's edges, for the fan-outs given.  For every degree in {0, 1, 200} and {f-1, f, f+1, 2f}
    of each f there are three nodes: one with in-neighbours drawn at random, one whose column holds the node itself, one whose
    column repeats a single neighbour in half of its entries.  Then n_plain nodes of in-degree 0..8, and with hub_degree > 0 a last
    node with that many in-edges.  -> (indptr, indices, special): special = every node above except the plain ones (hub included)."""
    rng = np.random.default_rng(seed)
    degrees = sorted({0, 1, 200} | {d for f in fanouts for d in (f - 1, f, f + 1, 2 * f) if d >= 0})
    n_special = 3 * len(degrees)
    n = n_special + n_plain + (1 if hub_degree else 0)
    columns = []
    for d in degrees:
        for kind in range(3):
            v = len(columns)
            col = rng.integers(0, n, size=d)
            if d and kind == 1:
                col[rng.integers(0, d)] = v                        # self-loop
            if d > 1 and kind == 2:
                col[rng.permutation(d)[: d // 2 + 1]] = col[0]     # one neighbour in half the column
            columns.append(col)
    columns += [rng.integers(0, n, size=rng.integers(0, 9)) for _ in range(n_plain)]
    if hub_degree:
        columns.append(rng.integers(0, n, size=hub_degree))
    indptr, indices = csc_from_columns(columns)
    special = np.arange(n_special, dtype=np.int64)
    if hub_degree:
        special = np.append(special, n - 1)
    return indptr, indices, special


def check_block_properties(indptr, indices, dst, f, src, loc):
    """The sampler's published properties of one block, independent of any twin: the destination nodes come first in the source
    list, the source list has no repeats, dst d has min(deg, f) valid entries and they come before the -1 padding, every valid
    entry is an in-neighbour of d, and no node is picked more often than it occurs in d's column (distinct positions)."""
    n = len(dst)
    assert np.array_equal(src[:n], dst), "destination nodes are not first"
    assert len(np.unique(src)) == len(src), "repeated source node"
    deg = indptr[dst + 1] - indptr[dst]
    valid = loc >= 0
    assert np.array_equal(valid.sum(1), np.minimum(deg, f)), "count != min(deg, fanout)"
    assert not np.any(valid[:, 1:] & ~valid[:, :-1]), "-1 padding before a valid entry"
    if not valid.any():
        return
    N = len(indptr) - 1
    rows, cols = np.nonzero(valid)
    picked = src[loc[rows, cols]]
    starts = indptr[dst]
    run = np.zeros(n, dtype=np.int64)
    np.cumsum(deg[:-1], out=run[1:])
    pos = np.repeat(starts - run, deg) + np.arange(int(deg.sum()))
    up, cp = np.unique(dst[rows] * N + picked, return_counts=True)
    uc, cc = np.unique(np.repeat(dst, deg) * N + indices[pos], return_counts=True)
    at = np.minimum(np.searchsorted(uc, up), len(uc) - 1)
    assert np.array_equal(uc[at], up), "a picked node is not in its destination's CSC column"
    assert np.all(cp <= cc[at]), "a node picked more often than its column holds it"
