"""CPU tests of temporal neighbour sampling: the numpy restatement (tests/_temporal_ref.py) on its own, the torch helpers, and every
refusal of COALA_GNN.sampler.TemporalNeighborSampler / TemporalEdgePredictionSampler, which all come before any launch."""
import ctypes as C

import numpy as np
import pytest

from _temporal_ref import (decode, edge_case_graph, eligible, encode, floyd, floyd_slow, node_bits_of, reference_layers, sort_by_time,
                           temporal_key, temporal_layer)


@pytest.fixture(scope="module")
def timed():
    """A random timed graph of 3000 nodes, degrees 0..60, timestamps in [0, 500) (so repeated inside a row), sorted per row."""
    rng = np.random.default_rng(11)
    deg = rng.integers(0, 61, size=3000)
    deg[[0, 9, 2999]] = 0
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = rng.integers(0, 3000, size=int(ip[-1])).astype(np.int64)
    ts = rng.integers(0, 500, size=int(ip[-1])).astype(np.int64)
    perm = sort_by_time(ip, ts)
    return ip, ix[perm], ts[perm]


def _pairs(rng, n, n_nodes, t_lo, t_hi):
    """n distinct (node, time) pairs."""
    nodes = rng.choice(n_nodes, size=n, replace=False).astype(np.int64)
    return nodes, rng.integers(t_lo, t_hi, size=n).astype(np.int64)


def test_floyd_vectorised_equals_python_integers():
    rng = np.random.default_rng(0)
    v = rng.integers(0, 1 << 40, size=64)
    t = rng.integers(-5, 1 << 50, size=64)
    for f in (1, 5, 32):
        m = rng.integers(f + 1, 3 * f + 50, size=64).astype(np.int64)
        m[0] = f + 1
        key = temporal_key(7, 3, 1, v, t)
        got = floyd(key, m, f)
        for i in range(64):
            assert got[i].tolist() == floyd_slow(key[i], int(m[i]), f)
            assert len(set(got[i].tolist())) == f and got[i].min() >= 0 and got[i].max() < m[i]


def test_eligible_is_a_bound_of_the_row(timed):
    ip, ix, ts = timed
    rng = np.random.default_rng(1)
    v = rng.integers(0, 3000, size=400)
    t = rng.integers(-3, 504, size=400)
    for inclusive in (False, True):
        m = eligible(ip, ts, v, t, inclusive)
        for i in range(400):
            row = ts[ip[v[i]]: ip[v[i] + 1]]
            assert m[i] == (np.sum(row <= t[i]) if inclusive else np.sum(row < t[i]))


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("strategy", ["uniform", "last"])
@pytest.mark.parametrize("f", [1, 5, 32])
def test_rows_of_the_reference(timed, f, strategy, inclusive):
    """Every picked edge is eligible, slots are valid-first, `last` picks the newest, m <= f takes all, picks are distinct."""
    ip, ix, ts = timed
    rng = np.random.default_rng(2)
    nodes, times = _pairs(rng, 500, 3000, -2, 503)
    (layer,), slot_time = reference_layers(ip, ix, ts, nodes, times, [f], 5, 9, strategy, inclusive)
    src, nbr, eid = layer
    m = eligible(ip, ts, nodes, times, inclusive)
    assert (m == 0).any() and (m <= f).any() and ((m > f).any() or f == 32)
    codes, _ = encode(nodes, times, 3000)
    assert np.array_equal(src[:500], codes)
    for i in range(500):
        lo = ip[nodes[i]]
        k = min(int(m[i]), f)
        assert (eid[i, :k] >= lo).all() and (eid[i, :k] < lo + m[i]).all() and (eid[i, k:] == -1).all(), "eligible, valid first"
        assert (nbr[i, :k] >= 0).all() and (nbr[i, k:] == -1).all()
        assert len(set(eid[i, :k].tolist())) == k
        when = ts[eid[i, :k]]
        assert (when <= times[i]).all() if inclusive else (when < times[i]).all()
        if m[i] <= f:
            assert eid[i, :k].tolist() == list(range(lo, lo + k)), "m <= f takes all, in CSC order"
        elif strategy == "last":
            assert eid[i].tolist() == list(range(lo + m[i] - f, lo + m[i])), "the newest, ascending"
        got_node, got_time = decode(src[nbr[i, :k]], slot_time, 3000)
        assert np.array_equal(got_node, ix[eid[i, :k]]) and (got_time == times[i]).all(), "a neighbour inherits its row's time"
    assert len(np.unique(src)) == len(src)


@pytest.mark.parametrize("strategy", ["uniform", "last"])
def test_a_row_does_not_depend_on_its_batch_or_its_slot(timed, strategy):
    ip, ix, ts = timed
    rng = np.random.default_rng(3)
    nodes, times = _pairs(rng, 300, 3000, 100, 400)
    (batch,), _ = reference_layers(ip, ix, ts, nodes, times, [5], 1, 2, strategy)
    for i in (0, 7, 299):
        (alone,), _ = reference_layers(ip, ix, ts, nodes[i: i + 1], times[i: i + 1], [5], 1, 2, strategy)
        assert np.array_equal(alone[2][0], batch[2][i])
    # other query times in the batch move every slot index (times below all of them are added): the rows keep their edges
    more_n = np.concatenate([np.arange(50, dtype=np.int64), nodes])
    more_t = np.concatenate([np.arange(50, dtype=np.int64) - 60, times])
    (moved,), _ = reference_layers(ip, ix, ts, more_n, more_t, [5], 1, 2, strategy)
    assert np.array_equal(moved[2][50:], batch[2])
    # a permutation of the slot indices: the same pairs under a hand-made, descending time table
    N = 3000
    slot_time, slot = np.unique(times, return_inverse=True)
    flipped = ((len(slot_time) - 1 - slot.reshape(-1)).astype(np.int64) << node_bits_of(N)) | nodes
    _, _, eid = temporal_layer(ip, ix, ts, flipped, slot_time[::-1].copy(), 5, 1, 2, 0, strategy)
    assert np.array_equal(eid, batch[2])


def test_bad_codes_give_empty_rows(timed):
    ip, ix, ts = timed
    bits = node_bits_of(3000)
    slot_time = np.array([100, 200], dtype=np.int64)
    codes = np.array([-1, -(1 << 62), (2 << bits) | 5, (1 << bits) | 3000, (1 << bits) | 4095, (1 << bits) | 5], dtype=np.int64)
    src, nbr, eid = temporal_layer(ip, ix, ts, codes, slot_time, 4, 0, 0, 0)
    assert (eid[:5] == -1).all() and (nbr[:5] == -1).all() and (eid[5] >= 0).any()
    assert src[:4].tolist() == codes[2:].tolist(), "a negative code is not inserted; any other is, decoded or not"


def test_uniformity_of_the_reference():
    """One row, m = 20 eligible edges of 30, f = 5, 4000 steps: every eligible edge's count is Binomial(4000, 1/4), demanded within
    5 sigma = 5 sqrt(750) ~ 137 of 1000; the ineligible tail is never taken."""
    ip = np.array([0, 30], dtype=np.int64)
    ix = np.zeros(30, dtype=np.int64)
    ts = np.arange(30, dtype=np.int64) * 10
    steps = 4000
    counts = np.zeros(30, dtype=np.int64)
    key = np.concatenate([temporal_key(42, s, 0, np.array([0]), np.array([200])) for s in range(steps)])
    picks = floyd(key, np.full(steps, 20, dtype=np.int64), 5)
    # the same through the layer for a few steps: the vectorised shortcut above is the rule
    for s in (0, 1, 3999):
        _, _, eid = temporal_layer(ip, ix, ts, np.array([0]), np.array([200], dtype=np.int64), 5, 42, s, 0)
        assert eid[0].tolist() == picks[s].tolist()
    np.add.at(counts, picks.reshape(-1), 1)
    assert counts[20:].sum() == 0 and counts.sum() == 5 * steps
    assert np.all(np.abs(counts[:20] - 1000) <= 5 * np.sqrt(750)), counts[:20]


def test_edge_case_graph_has_the_shapes():
    ip, ix, ts, named = edge_case_graph(f=5, hub_degree=1001)
    deg = np.diff(ip)
    assert [int(deg[named[k]]) for k in ("deg0", "f", "f1", "63", "64", "65")] == [0, 5, 6, 63, 64, 65] and deg[named["hub"]] == 1001
    row = slice(ip[named["equal"]], ip[named["equal"] + 1])
    assert len(set(ts[row].tolist())) == 1
    assert np.sum(ix[ip[named["repeat"]]: ip[named["repeat"] + 1]] == 3) >= 20
    assert np.array_equal(sort_by_time(ip, ts), np.arange(len(ts))), "sorted inside every row"


# ------------------------------------------------------------------------------------------------ helpers and refusals
def test_sort_csc_by_time_against_numpy():
    import torch
    from COALA_GNN.sampler import check_time_sorted, sort_csc_by_time
    rng = np.random.default_rng(3)
    deg = rng.integers(0, 9, size=500)
    deg[[0, 17, 499]] = 0
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = rng.integers(0, 500, size=int(ip[-1])).astype(np.int64)
    ts = rng.integers(-4, 4, size=len(ix)).astype(np.int64)
    for dtype in (torch.int64, torch.int32):
        s_ix, s_ts, perm = sort_csc_by_time(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(ts).to(dtype))
        want = sort_by_time(ip, ts)
        assert perm.dtype == torch.int64 and np.array_equal(perm.numpy(), want), "stable by (row, time)"
        assert s_ts.dtype == dtype and np.array_equal(s_ix.numpy(), ix[want]) and np.array_equal(s_ts.numpy(), ts[want])
        check_time_sorted(torch.from_numpy(ip), s_ts)
    with pytest.raises(ValueError, match="shape"):
        sort_csc_by_time(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(ts[:-1]))
    with pytest.raises(ValueError, match="integer"):
        sort_csc_by_time(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(ts).double())


def test_unsorted_times_raise():
    import torch
    from COALA_GNN.sampler import check_time_sorted
    ip = torch.tensor([0, 3, 3, 5, 8])
    ok = torch.tensor([0, 1, 1, 0, 2, -5, 1, 2])                   # the time may fall where a row starts
    check_time_sorted(ip, ok)
    check_time_sorted(torch.tensor([0, 0, 0]), torch.zeros(0, dtype=torch.int64))
    for bad in ([0, 2, 1, 0, 2, 1, 1, 2], [0, 1, 2, 2, 0, 1, 1, 2], [0, 1, 2, 0, 2, 1, 2, 1]):   # a fall inside the first, a middle, the last row
        with pytest.raises(ValueError, match="sort_csc_by_time"):
            check_time_sorted(ip, torch.tensor(bad), "when")
    with pytest.raises(ValueError, match="shape"):
        check_time_sorted(ip, ok[:-1])
    with pytest.raises(ValueError, match="integer"):
        check_time_sorted(ip, ok.float())


def test_synthetic_edge_times():
    import torch
    from COALA_GNN.sampler import check_time_sorted
    from COALA_GNN.synthetic import edge_times
    ip = torch.tensor([0, 40, 40, 45, 300])
    a, b = edge_times(ip, seed=1, t_max=50), edge_times(ip, seed=1, t_max=50)
    assert a.dtype == torch.int64 and a.shape == (300,) and torch.equal(a, b) and not torch.equal(a, edge_times(ip, seed=2, t_max=50))
    assert int(a.min()) >= 0 and int(a.max()) < 50
    check_time_sorted(ip, a)


def _host_graph(ip, ts, num_nodes=None, ndata=None):
    """A CSCGraph without its device handle: everything TemporalNeighborSampler reads of a graph before its first launch."""
    import torch
    from COALA_GNN.sampler import CSCGraph
    g = CSCGraph.__new__(CSCGraph)
    g.indptr, g.indices = ip, torch.zeros(int(ip[-1]), dtype=torch.int64)
    g.num_nodes, g.num_edges, g.device = (ip.numel() - 1 if num_nodes is None else num_nodes), int(ip[-1]), torch.device("cpu")
    g.ndata, g.edata = dict(ndata or {}), {"ts": ts}
    g._weights, g._etypes, g._etimes, g._max_in_degree = {}, {}, {}, None
    return g


def test_every_refusal_comes_before_any_launch(hiplib):
    import torch
    from COALA_GNN.sampler import (EdgePredictionSampler, NeighborSampler, TemporalEdgePredictionSampler, TemporalNeighborSampler,
                                   UniformNegativeSampler, pair_code_bits)
    s = TemporalNeighborSampler([5, 10], seed=3)
    assert isinstance(s, NeighborSampler) and s.fanouts == [5, 10] and s.time == "ts" and s.strategy == "uniform" and not s.inclusive
    assert s.edge_ids and s.seed_time is None and s.bucket_by_owner == 0 and s.stream_safe and s.completes_on_host and s.step == 0
    assert TemporalNeighborSampler([5], time="when", strategy="last", inclusive=True, seed_time="t", edge_ids=False).strategy == "last"
    with pytest.raises(ValueError, match="fan-out -1"):
        TemporalNeighborSampler([5, -1])
    for f in (0, 33):
        with pytest.raises(ValueError, match="fan-out"):
            TemporalNeighborSampler([f])
    with pytest.raises(ValueError, match="prob"):
        TemporalNeighborSampler([5], prob="w")
    with pytest.raises(ValueError, match="bucket_by_owner"):
        TemporalNeighborSampler([5], bucket_by_owner=4)
    with pytest.raises(ValueError, match="node timestamps"):
        TemporalNeighborSampler([5], node_time="t")
    with pytest.raises(ValueError, match="strategy"):
        TemporalNeighborSampler([5], strategy="recent")
    ip = torch.tensor([0, 3, 3, 5, 8])
    good = torch.tensor([0, 1, 1, 0, 2, -5, 1, 2])
    seeds = torch.tensor([0, 2])
    for bad, match in ((torch.tensor([0, 2, 1, 0, 2, 1, 1, 2]), "sort_csc_by_time"), (good.double(), "floating-point"), (good[:-1], "shape")):
        with pytest.raises(ValueError, match=match):
            s.sample_begin(_host_graph(ip, bad), seeds, seed_times=torch.tensor([1, 1]))
    with pytest.raises(KeyError, match="when"):
        TemporalNeighborSampler([5], time="when").sample_begin(_host_graph(ip, good), seeds, seed_times=torch.tensor([1, 1]))
    with pytest.raises(ValueError, match="seed_times"):
        s.sample_begin(_host_graph(ip, good), seeds)                                             # no times anywhere
    with pytest.raises(ValueError, match="floating-point"):
        s.sample_begin(_host_graph(ip, good), seeds, seed_times=torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match="one per seed"):
        s.sample_begin(_host_graph(ip, good), seeds, seed_times=torch.tensor([1, 2, 3]))
    with pytest.raises(KeyError, match="'t'"):
        TemporalNeighborSampler([5], seed_time="t").sample_begin(_host_graph(ip, good), seeds)
    # code overflow: 61 bits of node field leave one bit of slot, so two distinct times fit and three do not
    big = _host_graph(ip, good, num_nodes=(1 << 61) - 1)
    assert pair_code_bits((1 << 61) - 1, 2) == 61 and pair_code_bits(4, 1) == 3 and pair_code_bits(3, 1) == 2
    with pytest.raises(ValueError, match="62"):
        pair_code_bits((1 << 61) - 1, 3)
    with pytest.raises(ValueError, match="distinct query times"):
        s.sample_begin(big, torch.tensor([0, 1, 2]), seed_times=torch.tensor([5, 6, 7]))
    assert s.step == 0, "a refused call does not advance the step"
    # the wrappers
    with pytest.raises(ValueError, match="inclusive"):
        TemporalEdgePredictionSampler(TemporalNeighborSampler([5], inclusive=True))
    with pytest.raises(ValueError, match="TemporalNeighborSampler"):
        TemporalEdgePredictionSampler(NeighborSampler([5]))
    with pytest.raises(ValueError, match="TemporalEdgePredictionSampler"):
        EdgePredictionSampler(s)
    w = TemporalEdgePredictionSampler(s, negative_sampler=UniformNegativeSampler(3))
    assert w.fanouts == [5, 10, 4] and w.num_neg == 3 and w.bucket_by_owner == 0 and w.stream_safe and w.completes_on_host
    for name in ("sample", "sample_begin", "sample_end", "make_graph"):
        assert callable(getattr(w, name))


def test_temporal_symbol_is_exported_and_the_abi_version_stays(hiplib):
    from COALA_GNN_Pybind import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "coala_sampler_sample_layers_temporal") and "coala_sampler_sample_layers_temporal" in _capi.SYMBOLS
    assert _capi.load().coala_abi_version() == 4


def test_temporal_entry_refuses_bad_arguments_before_any_device_call(hiplib):
    """The argument checks that need no handle: they come first, so they can be seen without a GPU."""
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    lay = (_capi.SamplerLayer * 1)(_capi.SamplerLayer(None, None, None, 0, 0))
    fan = (C.c_int32 * 1)(5)

    def call(fan=fan, lay=lay, ts=1, slot_time=1, n_slots=1, strategy=0):
        return L.coala_sampler_sample_layers_temporal(None, None, 0, fan, 1, 0, 0, lay, ts, slot_time, n_slots, strategy, 0, None, None, None,
                                                      None, None)
    assert call(ts=None) == _capi.EINVAL and "edge_ts" in _capi.last_error()
    assert call(slot_time=None) == _capi.EINVAL and "slot_time" in _capi.last_error()
    assert call(n_slots=-1) == _capi.EINVAL and "slot_time" in _capi.last_error()
    for strategy in (-1, 2):
        assert call(strategy=strategy) == _capi.EINVAL and "strategy" in _capi.last_error()
    for bad in (-1, 0, 33):
        assert call(fan=(C.c_int32 * 1)(bad)) == _capi.EINVAL and f"fan-out {bad}" in _capi.last_error()
    ragged = (_capi.SamplerLayer * 1)(_capi.SamplerLayer(None, None, 1, 0, 0))
    assert call(lay=ragged) == _capi.EINVAL and "indptr_local" in _capi.last_error()
    assert call(fan=None) == _capi.EINVAL and "null" in _capi.last_error()
    assert call() == _capi.EINVAL and "null" in _capi.last_error()      # valid arguments: the null handle is what is left
