"""The twin construction of the wide sampler tests (tests only): a CSC graph G with more than 2^32 edges that is never held on the host,
and a small twin T on which the numpy restatements run.

A small graph S (the sweep's graphs: degree edges, self-loops, repeated neighbours, a hub above kHubDegree as its last node) is copied
into G once per boundary B, so that B lies strictly inside the copy's hub row, and once more wholly above the last boundary.  Between
the copies ("live groups") lie filler rows that absorb the slack; every filler entry is one filler node, the sink.  A live row lists
live nodes of its own group only -- node m of S is node live_ids[group][m] of G -- so a sample that starts in a group never leaves it.
T has the same node ids and the same live rows, and every filler row empty.  Every draw of the sampler is keyed by the node id and the
position inside the row, never by the CSC position, so a sample of G from live seeds is the sample of T with every edge id moved by
indptr_G[v] - indptr_T[v] of its row v: to_wide().  tests/test_wide_twin_cpu.py checks exactly that, on a G small enough for numpy.

Importable without a GPU; torch is imported only where a device tensor is made."""
from collections import namedtuple

import numpy as np

import _edge_batch_ref as EB
import _rel_fanout_ref
import _sampler_sweep as S
from _util import edge_case_graph

BOUNDARIES = (2**31, 2**32)         # the wide graph: signed and unsigned 32-bit positions
FILLER_DEGREE = 2**16
SMALL_BOUNDARIES = (2**12, 2**13)   # the same layout scaled down until G fits in numpy
SMALL_FILLER_DEGREE = 64

Small = namedtuple("Small", "graph special")     # graph: _sampler_sweep.Graph; special: the nodes built around the degree edges, the hub last


def small_graph(kind, seed, fanouts=(1, 5, 32), n_plain=3000, hub_degree=S.HUB):
    """S: kind 'hub' (_util.edge_case_graph) or 'typed' (_rel_fanout_ref.typed_edge_case_graph), with weights and per-row sorted edge
    types made the way _sampler_sweep._build_graph makes them -- with the default sizes it IS the sweep's graph."""
    fanouts = list(fanouts)
    if kind == "typed":
        ip, ix, et, special = _rel_fanout_ref.typed_edge_case_graph(fanouts, S.NUM_RELS, n_plain=n_plain, hub_degree=hub_degree, seed=seed)
    else:
        ip, ix, special = edge_case_graph(fanouts, n_plain=n_plain, hub_degree=hub_degree, seed=seed)
    if fanouts == [1, 5, 32] and n_plain == 3000 and hub_degree == S.HUB:
        return Small(S.build_graph((kind, seed)), special)
    rng = np.random.default_rng(500 + seed)
    if kind != "typed":
        et = rng.integers(0, S.NUM_RELS, size=len(ix)).astype(np.int64)
        perm = _rel_fanout_ref.sort_by_type(ip, et)
        ix, et = ix[perm], et[perm]
    w = (1.0 - rng.random(len(ix))).astype(np.float32)
    w[rng.random(len(ix)) < 0.1] = 0
    return Small(S.Graph(ip, ix, et, w, int(np.diff(ip).max())), special)


class Layout(object):
    """Where the rows of G lie.  Holds indptr_G, the twin T and the position maps; G's indices exist only on the device
    (device_graph) or, scaled down, in numpy (wide_numpy).

    Node order: filler run, live group 0, filler run, live group 1, ..., live group len(boundaries), one filler row.  A filler run is
    rows of filler_degree entries and one shorter row for the remainder.  Group i < len(boundaries) starts at
    boundaries[i] - indptr_S[hub] - deg_S(hub) // 2, which puts the boundary in the middle of its hub row (S's last row)."""

    def __init__(self, small, boundaries=BOUNDARIES, filler_degree=FILLER_DEGREE):
        g = small.graph
        ip, ix = np.asarray(g.indptr), np.asarray(g.indices)
        n, e = len(ip) - 1, len(ix)
        hub = n - 1
        hub_start, hub_deg = int(ip[hub]), int(ip[hub + 1] - ip[hub])
        assert hub_deg == np.diff(ip).max() and hub_deg >= 4, "S's last node must be its hub"
        self.small, self.boundaries, self.filler_degree = small, tuple(int(b) for b in boundaries), int(filler_degree)
        self.n_small, self.e_small, self.hub_small = n, e, hub
        deg, live, end = [], [], 0
        self.live_ids, self.group_pos = [], []
        starts = [b - hub_start - hub_deg // 2 for b in self.boundaries] + [None]
        for gs in starts:
            gs = end + filler_degree if gs is None else gs
            gap = gs - end
            assert gap > 0, f"no room for a filler row in front of the live group at {gs}: S has {e} edges, the previous group ends at {end}"
            run = [filler_degree] * (gap // filler_degree) + ([gap % filler_degree] if gap % filler_degree else [])
            deg += run
            live += [False] * len(run)
            self.live_ids.append(len(deg) + np.arange(n, dtype=np.int64))
            self.group_pos.append((gs, gs + e))
            deg += np.diff(ip).tolist()
            live += [True] * n
            end = gs + e
        deg.append(filler_degree)
        live.append(False)
        self.live = np.array(live)
        deg = np.array(deg, dtype=np.int64)
        self.N = len(deg)
        self.indptr = np.zeros(self.N + 1, dtype=np.int64)
        np.cumsum(deg, out=self.indptr[1:])
        self.E = int(self.indptr[-1])
        self.sink = 0                                                # the first filler node
        assert not self.live[self.sink]
        self.indptr_T = np.zeros(self.N + 1, dtype=np.int64)
        np.cumsum(np.where(self.live, deg, 0), out=self.indptr_T[1:])
        self.indices_T = np.concatenate([ids[ix] for ids in self.live_ids])
        k = len(self.live_ids)
        self.weights_T = np.tile(np.asarray(g.weights), k)
        self.etype_T = np.tile(np.asarray(g.etype), k)
        self.shift = self.indptr[:-1] - self.indptr_T[:-1]           # per row: G position - T position
        self.hubs = np.array([int(ids[hub]) for ids in self.live_ids], dtype=np.int64)
        self.max_in_degree = int(deg.max())
        for a in (self.indptr, self.indptr_T, self.indices_T, self.weights_T, self.etype_T, self.shift):
            a.setflags(write=False)

    # ------------------------------------------------------------------------------------------------ the conditions of the method
    def check(self):
        """Every boundary strictly inside a hub row; live rows wholly below the first boundary, wholly between two consecutive ones and
        wholly above the last; E above the last boundary; closure: a live row lists live nodes of its own group only."""
        ip = self.indptr
        assert self.E > self.boundaries[-1]
        for b, h in zip(self.boundaries, self.hubs):
            assert ip[h] < b < ip[h + 1] - 1, (b, int(ip[h]), int(ip[h + 1]))
        rows = np.flatnonzero(self.live & (np.diff(ip) > 0))
        lo, hi = ip[rows], ip[rows + 1]
        edges = (0,) + self.boundaries + (self.E + 1,)
        for a, b in zip(edges[:-1], edges[1:]):
            assert np.any((lo >= a) & (hi <= b)), f"no live row wholly inside [{a}, {b})"
        for g, (ids, (p0, p1)) in enumerate(zip(self.live_ids, self.group_pos)):
            assert ip[ids[0]] == p0 and ip[ids[-1] + 1] == p1 and np.all(self.live[ids])
            t0 = int(self.indptr_T[ids[0]])
            row = self.indices_T[t0: t0 + self.e_small]
            assert row.min() >= ids[0] and row.max() <= ids[-1], f"group {g} is not closed"
        assert int(self.live.sum()) == len(self.live_ids) * self.n_small
        return True

    # ------------------------------------------------------------------------------------------------ position maps
    def _rows(self, indptr, pos):
        return np.searchsorted(indptr, pos, side="right") - 1        # the row v with indptr[v] <= pos < indptr[v + 1]

    def to_wide(self, eid_T):
        """T positions -> G positions (any shape); -1 stays -1."""
        e = np.asarray(eid_T, dtype=np.int64)
        ok = e >= 0
        assert np.all(e[ok] < len(self.indices_T))
        rows = self._rows(self.indptr_T, np.where(ok, e, 0))
        return np.where(ok, e + self.shift[rows], -1)

    def to_twin(self, eid_G):
        """Live G positions -> T positions; -1 stays -1.  A filler position is an error."""
        e = np.asarray(eid_G, dtype=np.int64)
        ok = e >= 0
        assert np.all(e[ok] < self.E)
        rows = self._rows(self.indptr, np.where(ok, e, int(self.group_pos[0][0])))
        assert np.all(self.live[rows]), "a filler position has no twin"
        return np.where(ok, e - self.shift[rows], -1)

    def is_live(self, pos):
        return self.live[self._rows(self.indptr, np.asarray(pos, dtype=np.int64))]

    def indices_at(self, pos):
        """G's entry at any position in [0, E), filler included."""
        pos = np.asarray(pos, dtype=np.int64)
        assert np.all((pos >= 0) & (pos < self.E))
        rows = self._rows(self.indptr, pos)
        at = np.clip(pos - self.shift[rows], 0, len(self.indices_T) - 1)
        return np.where(self.live[rows], self.indices_T[at], self.sink)

    # ------------------------------------------------------------------------------------------------ the graphs
    def twin(self):
        """T as the restatements take it (_sampler_sweep.Graph)."""
        return S.Graph(self.indptr_T, self.indices_T, self.etype_T, self.weights_T, self.max_in_degree)

    def _fill(self, full, chunks, of):
        """of(fill value) -> the array; every live group is one slice assignment."""
        out = full
        t = 0
        for p0, p1 in self.group_pos:
            out[p0:p1] = of(chunks[t: t + self.e_small])
            t += self.e_small
        return out

    def wide_numpy(self):
        """G itself as a _sampler_sweep.Graph: only for a scaled-down layout."""
        assert self.E < 2**24, "G is held on the host only when scaled down"
        ix = self._fill(np.full(self.E, self.sink, dtype=np.int64), self.indices_T, lambda a: a)
        w = self._fill(np.ones(self.E, dtype=np.float32), self.weights_T, lambda a: a)
        et = self._fill(np.zeros(self.E, dtype=np.int64), self.etype_T, lambda a: a)
        return S.Graph(self.indptr, ix, et, w, self.max_in_degree)

    def device_graph(self, weights=False, etype=False):
        """G as a CSCGraph: `indices` is allocated on the device holding the sink id and every live group is copied in by one slice
        assignment.  weights (fp32, filler 1.0) -> edata['w'], etype (int32, filler 0) -> edata['etype'], only when asked for."""
        import torch
        from COALA_GNN.sampler import CSCGraph
        ix = self._fill(torch.full((self.E,), self.sink, dtype=torch.int64, device="cuda"), self.indices_T, self._up(torch.int64))
        edata = {}
        if weights:
            edata["w"] = self.device_weights()
        if etype:
            edata["etype"] = self.device_etype()
        return CSCGraph(torch.from_numpy(self.indptr.copy()).cuda(), ix, edata=edata)

    @staticmethod
    def _up(dtype):
        import torch
        return lambda a: torch.from_numpy(np.array(a)).to(device="cuda", dtype=dtype)     # a copy: the layout's arrays are read-only

    def device_weights(self):
        import torch
        return self._fill(torch.ones(self.E, dtype=torch.float32, device="cuda"), self.weights_T, self._up(torch.float32))

    def device_etype(self):
        import torch
        return self._fill(torch.zeros(self.E, dtype=torch.int32, device="cuda"), self.etype_T, self._up(torch.int32))

    def device_twin(self):
        return S.make_device_graph(self.twin())

    # ------------------------------------------------------------------------------------------------ seeds
    def seeds(self, n=300, rng_seed=0):
        """About n distinct live nodes in a fixed shuffled order: the hub of every group, the first and last live node of every group,
        the special-degree nodes (all of group 0's, every third of the others'), the rest drawn from the live nodes."""
        rng = np.random.default_rng(rng_seed)
        special = np.asarray(self.small.special, dtype=np.int64)
        must = [self.hubs]
        for g, ids in enumerate(self.live_ids):
            must += [ids[[0, -1]], ids[special if g == 0 else special[g::3]]]
        must = np.unique(np.concatenate(must))
        rest = np.setdiff1d(np.flatnonzero(self.live), must)
        extra = rng.permutation(rest)[: max(n - len(must), 0)]
        return rng.permutation(np.concatenate([must, extra])).astype(np.int64)

    # ------------------------------------------------------------------------------------------------ coverage of the boundaries
    def covers(self, eids):
        """Whether a call's edge ids (G positions, any -1 ignored) make the case worth running: for every boundary the straddling hub row
        gives ids on both sides of it (so there are ids above every boundary)."""
        e = np.asarray(eids, dtype=np.int64).reshape(-1)
        for b, h in zip(self.boundaries, self.hubs):
            lo, hi = int(self.indptr[h]), int(self.indptr[h + 1])
            if not (np.any((e >= lo) & (e < b)) and np.any((e >= b) & (e < hi))):
                return False
        return bool(np.any(e >= self.group_pos[-1][0]))

    # ------------------------------------------------------------------------------------------------ edge batches
    def edge_batch_eids(self, rng_seed=0, n_random=200):
        """The seed edges of the wide edge-batch test: B - 1, B, B + 1 of every boundary, the first and last position of every live group,
        E - 1, a filler position below the first boundary and one between the boundaries, a repeated id, n_random live positions."""
        rng = np.random.default_rng(rng_seed)
        e = [b + d for b in self.boundaries for d in (-1, 0, 1)]
        e += [p for p0, p1 in self.group_pos for p in (p0, p1 - 1)]
        e += [self.E - 1, self.filler_degree + 7, self.group_pos[0][1] + self.filler_degree + 3]
        e.append(e[1])
        live_T = rng.integers(0, len(self.indices_T), size=n_random)
        return np.concatenate([np.array(e, dtype=np.int64), self.to_wide(live_T)])

    def edge_batch_ref(self, eids, k, seed, step):
        """_edge_batch_ref.edge_batch on G from the pieces it exports: the endpoints of a live edge on T through to_twin, those of a
        filler edge from indptr_G and indices_at; the negatives from the wide ids, which key the draw; then compact."""
        eids = np.asarray(eids, dtype=np.int64)
        n = len(eids)
        ok = (eids >= 0) & (eids < self.E)
        e = np.where(ok, eids, int(self.group_pos[0][0]))
        live = self.is_live(e) & ok
        src, dst = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        src[live], dst[live] = EB.endpoints(self.indptr_T, self.indices_T, self.to_twin(e[live]))
        fill = ok & ~live
        src[fill], dst[fill] = self.indices_at(e[fill]), self._rows(self.indptr, e[fill])
        neg = EB.negatives(self.N, eids, k, seed, step)
        neg[src < 0] = -1
        nodes, local = EB.compact(np.concatenate([src, dst, neg.reshape(-1)]))
        return dict(seed_nodes=nodes, pos_src=local[:n].astype(np.int32), pos_dst=local[n: 2 * n].astype(np.int32),
                    neg_dst=local[2 * n:].reshape(n, k).astype(np.int32), n_bad=int((src < 0).sum()))


def same_edge_batch(got, want):
    """The comparison of tests/test_edge_batch_gpu.py: every array equal in dtype and value, and the bad-edge count."""
    for key in ("seed_nodes", "pos_src", "pos_dst", "neg_dst"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert got["n_bad"] == want["n_bad"]


def widen(layout, refs):
    """A reference made on T -> the reference of G: the edge ids through to_wide, everything else as it is."""
    return [dict(r, eid=layout.to_wide(r["eid"])) if r.get("eid") is not None else r for r in refs]


def ref_edge_ids(refs):
    e = [r["eid"].reshape(-1) for r in refs if r.get("eid") is not None]
    return np.concatenate(e) if e else np.zeros(0, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------- the calls of the wide GPU file
GRAPH_SEED = 1
N_SEEDS = 300
WALKS = ((2, 10, 0.5), (3, 17, 0.9), (4, 16, 0.0), (1, 1, 0.0))      # the (T, W, p) triples of the sweep


def _call(kind, fanouts, n, **kw):
    d = dict(T=2, W=10, p=0.5, dep=False, seed=7, step=3)
    d.update(kw)
    return S.Call(kind, fanouts, n, "perm", 0, d["seed"], d["step"], 0, kind != "walk", d["dep"], d["T"], d["W"], d["p"], 0)


def wide_calls(n):
    """name -> (graph kind, Call) for n seeds; G = 0 (the tests also run every call with bucket_by_owner = 4 against the same reference).
    A LABOR row takes about 5 of the hub's 5,000 edges and a relation row 1: the steps are ones at which the reference's picks fall on both
    sides of both boundaries, which tests/test_wide_twin_cpu.py asserts for every call."""
    calls = {
        "uniform_5_5": ("hub", _call("uniform", [5, 5], n)),
        "uniform_32": ("hub", _call("uniform", [32], n)),
        "full_2_all": ("hub", _call("full", [2, -1], n)),
        "full_all_2": ("hub", _call("full", [-1, 2], n)),
        "weighted_5_5": ("hub", _call("weighted", [5, 5], n)),
        "labor_5_5": ("hub", _call("labor", [5, 5], n, step=4)),
        "labor_5_5_dep": ("hub", _call("labor", [5, 5], n, dep=True, step=4)),
        "rel": ("typed", _call("rel", [[1, 0, 2], [-1, 1, 2]], n)),
    }
    for T, W, p in WALKS:
        calls[f"walk_T{T}_W{W}"] = ("hub", _call("walk", [3, 2], n, T=T, W=W, p=p))
    return calls


# ---------------------------------------------------------------------------------------------------- a simulated 32-bit wrap
def uniform_layer_by_position(indptr, indices, dst, f, seed, step, layer, wrap=None, wrap_ids=False):
    """One uniform fixed layer from its positions (_sampler_sweep.uniform_ids): -> (src, nbr_local, eid).  wrap: every position is
    reduced mod `wrap` before `indices` is read -- what a kernel does whose `start + pick` lost its 64-bit cast; wrap_ids: the edge id
    it reports is the reduced one as well."""
    import _weighted_ref
    eid = S.uniform_ids(indptr, dst, f, seed, step, layer)
    pos = eid if wrap is None else np.where(eid >= 0, eid % wrap, -1)
    nbr = np.where(pos >= 0, indices[np.maximum(pos, 0)], -1)
    src, loc = _weighted_ref.compact(dst, nbr)
    return src, loc, (pos if wrap_ids else eid)


def edge_batch_by_position(indptr, indices, eids, k, seed, step, wrap=None):
    """_edge_batch_ref.edge_batch with every position reduced mod `wrap` before the row search and the read of `indices`."""
    eids = np.asarray(eids, dtype=np.int64)
    n, N = len(eids), len(indptr) - 1
    ok = (eids >= 0) & (eids < len(indices))
    src, dst = EB.endpoints(indptr, indices, eids if wrap is None else np.where(ok, eids % wrap, eids))
    neg = EB.negatives(N, eids, k, seed, step)
    neg[src < 0] = -1
    nodes, local = EB.compact(np.concatenate([src, dst, neg.reshape(-1)]))
    return dict(seed_nodes=nodes, pos_src=local[:n].astype(np.int32), pos_dst=local[n: 2 * n].astype(np.int32),
                neg_dst=local[2 * n:].reshape(n, k).astype(np.int32), n_bad=int((src < 0).sum()))
