"""CPU tests of edge-weighted sampling (NeighborSampler(prob=...)): the numpy restatement of tests/_weighted_ref.py against exact
successive-sampling inclusion probabilities and the P <= f / weight-0 rules, the new C entry's export and its argument checks, and the
Python weight validation.  No kernel is launched here."""
import ctypes as C
import math

import numpy as np
import pytest

from _weighted_ref import inclusion_probabilities, select, sample_key, splitmix64


def _replicated(row, copies):
    """A CSC graph of `copies` nodes, each with the same in-edge weights `row` -> (indptr, w)"""
    deg = len(row)
    indptr = np.arange(copies + 1, dtype=np.int64) * deg
    return indptr, np.tile(np.asarray(row, dtype=np.float32), copies)


@pytest.mark.parametrize("row,f", [([1, 2, 3, 4, 0, 10], 2), ([1, 2, 3, 4, 0, 10], 3), ([0.5, 0.5, 5, 1e-3, 2, 0], 2),
                                   ([1, 1, 1, 1, 1, 1], 3), ([7, 0, 0, 1, 1, 0], 2)])
def test_restatement_inclusion_matches_enumeration(row, f):
    copies = 20000
    indptr, w = _replicated(row, copies)
    pos = select(indptr, w, np.arange(copies), f, seed=11, step=3, layer=1)
    hits = np.zeros(len(row))
    valid = pos >= 0
    np.add.at(hits, pos[valid], 1)
    freq = hits / copies
    p = inclusion_probabilities(row, f)
    assert abs(p.sum() - min(f, int(np.count_nonzero(row)))) < 1e-12
    sigma = np.sqrt(p * (1 - p) / copies)
    assert np.all(np.abs(freq - p) <= 5 * sigma + 1e-12), (freq, p)
    assert np.all(valid.sum(1) == min(f, int(np.count_nonzero(row))))


def test_enumeration_against_closed_forms():
    assert np.allclose(inclusion_probabilities([1, 3], 1), [0.25, 0.75])
    # two of three: P(not a) = w_b/W * w_c/(W - w_b) + w_c/W * w_b/(W - w_c)
    w = [1.0, 2.0, 5.0]
    W = sum(w)
    p_not_a = w[1] / W * w[2] / (W - w[1]) + w[2] / W * w[1] / (W - w[2])
    assert math.isclose(inclusion_probabilities(w, 2)[0], 1 - p_not_a)
    assert np.array_equal(inclusion_probabilities([0, 2, 0, 3], 2), [0, 1, 0, 1])


def test_positive_count_at_most_f_and_weight_zero_rules():
    f = 4
    rows = [[0, 0, 0, 0, 0],                     # every weight 0: an empty row
            [0, 3, 0, 1e-40, 0, 0, 2, 0],        # P = 3 <= f: exactly those, in CSC order (a denormal weight is positive)
            [1, 1, 1, 1],                        # deg = f
            [0] * 50 + [1] * 4 + [0] * 50,       # exactly f positive among many zeros
            [0] * 50 + [1] * 5 + [0] * 50,       # f + 1 positive: one of them is left out
            [1e30] + [1e-30] * 40,               # one dominant weight
            []]                                  # degree 0
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    w = np.concatenate([np.asarray(r, dtype=np.float32) for r in rows])
    for step in range(20):
        pos = select(indptr, w, np.arange(len(rows)), f, seed=5, step=step, layer=0)
        assert np.all(pos[0] == -1) and np.all(pos[6] == -1)
        assert pos[1].tolist() == [1, 3, 6, -1]
        assert pos[2].tolist() == [0, 1, 2, 3]
        assert pos[3].tolist() == [50, 51, 52, 53]
        assert np.all((pos[4] >= 50) & (pos[4] < 55)) and np.all(np.diff(pos[4]) > 0)
        assert pos[5][0] == 0 and np.all(np.diff(pos[5]) > 0)
        for d, r in enumerate(rows):
            chosen = pos[d][pos[d] >= 0]
            assert np.all(np.asarray(r, dtype=np.float32)[chosen] > 0), "a weight-0 edge was chosen"
    # an out-of-range destination id gives an empty row
    assert np.all(select(indptr, w, np.array([len(rows), -3]), f, 0, 0, 0) == -1)


def test_draws_depend_on_the_row_only():
    """A row's draw depends on (seed, step, layer, v, j): the same node gives the same positions whatever else is in the batch."""
    rng = np.random.default_rng(0)
    n = 3000
    deg = rng.integers(0, 60, size=n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    w = rng.random(int(indptr[-1])).astype(np.float32)
    w[rng.random(len(w)) < 0.2] = 0
    all_rows = select(indptr, w, np.arange(n), 7, 9, 2, 1)
    some = rng.permutation(n)[:400]
    assert np.array_equal(select(indptr, w, some, 7, 9, 2, 1), all_rows[some])
    assert not np.array_equal(select(indptr, w, np.arange(n), 7, 9, 2, 0), all_rows)   # another layer key, another draw


def test_stream_differs_from_uniform_key():
    v = np.arange(5)
    k = sample_key(1, 2, 0, v)
    assert k.dtype == np.uint64 and len(set(k.tolist())) == 5
    assert int(splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF     # splitmix64's published first output for state 0


def test_weighted_symbol_is_exported(hiplib):
    from COALA_GNN_Pybind import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "coala_sampler_sample_layers_weighted")
    assert "coala_sampler_sample_layers_weighted" in _capi.SYMBOLS
    assert _capi.load().coala_abi_version() == 4


def test_weighted_entry_fails_loudly_without_a_gpu(hiplib):
    """Bad arguments are refused before any device call; and without a GPU no sampler handle can exist, so no weighted call can run."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    fan = (C.c_int32 * 1)(5)
    lay = (_capi.SamplerLayer * 1)(_capi.SamplerLayer(None, None, None, 0, 0))
    w = (C.c_float * 4)()
    rc = L.coala_sampler_sample_layers_weighted(None, None, 0, fan, 1, 0, 0, lay, None, None, None, None, None, None)
    assert rc == _capi.EINVAL and "edge_weights" in _capi.last_error()
    rc = L.coala_sampler_sample_layers_weighted(None, None, 0, fan, 1, 0, 0, lay, C.cast(w, C.c_void_p), None, None, None, None, None)
    assert rc == _capi.EINVAL and "null" in _capi.last_error()
    if not torch.cuda.is_available():
        ip = np.zeros(2, dtype=np.int64)
        h = C.c_void_p()
        with pytest.raises(RuntimeError, match="libcoala_hip"):
            _capi.check(L.coala_sampler_create(0, ip.ctypes.data, ip.ctypes.data, 1, 0, C.byref(h)))


def _host_graph(num_edges, edata):
    """A CSCGraph shell on the host (no sampler handle): enough for edge_weights(), which runs before any launch."""
    import torch
    from COALA_GNN.sampler import CSCGraph
    g = CSCGraph.__new__(CSCGraph)
    g.num_edges, g.device, g.edata, g._weights, g._h = num_edges, torch.device("cpu"), dict(edata), {}, None
    return g


def test_weight_validation(hiplib):
    import torch
    from COALA_GNN.sampler import NeighborSampler
    assert NeighborSampler([5, -1], prob="w").prob == "w" and NeighborSampler([5]).prob is None
    good = torch.tensor([0.0, 1.0, 2.5, 0.0], dtype=torch.float64)
    g = _host_graph(4, {"w": good, "ints": torch.tensor([0, 1, 2, 3]),
                        "neg": torch.tensor([1.0, -0.5, 1.0, 1.0]), "nan": torch.tensor([1.0, float("nan"), 1.0, 1.0]),
                        "inf": torch.tensor([1.0, float("inf"), 1.0, 1.0]), "big": torch.tensor([1e300, 1.0, 1.0, 1.0], dtype=torch.float64),
                        "short": torch.ones(3), "2d": torch.ones(4, 1)})
    w = g.edge_weights("w")
    assert w.dtype == torch.float32 and w.is_contiguous() and w.tolist() == [0.0, 1.0, 2.5, 0.0]
    assert g.edge_weights("w") is w                                   # validated once, cached
    assert g.edge_weights("ints").tolist() == [0.0, 1.0, 2.0, 3.0]
    for key in ("neg", "nan", "inf", "big", "short", "2d"):
        with pytest.raises(ValueError, match=repr(key)):
            g.edge_weights(key)
    with pytest.raises(KeyError, match="missing"):
        g.edge_weights("missing")
    good[1] = -1.0                                                    # modified in place: validated again
    with pytest.raises(ValueError, match="'w'"):
        g.edge_weights("w")
    g.edata["w"] = torch.ones(4)                                      # replaced
    assert g.edge_weights("w").tolist() == [1.0] * 4
