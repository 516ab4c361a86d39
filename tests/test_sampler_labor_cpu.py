"""The LABOR restatement (tests/_labor_ref.py, the reference of test_sampler_labor_gpu.py) checked on its own, without a GPU: the
rule's properties on a power-law graph, the expected row length, the 32-bit-halves mulhi64 against Python integers, and the
argument checks of COALA_GNN.sampler.LaborSampler."""
import ctypes as C

import numpy as np
import pytest

from _full_ref import full_layer
from _labor_ref import (M64, compact_ragged, edge_weights, labor_key, labor_layer, mulhi64, reference_layers, source_draws, splitmix64,
                        splitmix64_int, taken_mask, taken_mask_slow)


@pytest.fixture(scope="module")
def powerlaw():
    from COALA_GNN.synthetic import powerlaw_csc
    ip, ix = powerlaw_csc(200_000, 30, seed=1, device="cpu")
    return np.ascontiguousarray(ip.numpy()), np.ascontiguousarray(ix.numpy())


def _rows(ip, ix, dst, k, key):
    """Per destination: (degree, the taken source nodes as an array)."""
    src, lp, loc, eid = labor_layer(ip, ix, dst, k, key)
    return ip[dst + 1] - ip[dst], [ix[eid[lp[d]: lp[d + 1]]] for d in range(len(dst))], (src, lp, loc, eid)


def test_mulhi64_halves_against_python_integers():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 1 << 64, size=10_000, dtype=np.uint64)
    b = rng.integers(0, 1 << 64, size=10_000, dtype=np.uint64)
    b[:3000] = rng.integers(1, 1 << 22, size=3000)                          # degrees of real graphs
    b[3000:5000] = (1 << 32) + rng.integers(-1000, 1000, size=2000)         # degrees near 2^32: both halves of b in play
    a[:8] = [0, 1, M64, M64, 1 << 32, (1 << 32) - 1, M64 - 1, 1 << 63]
    b[:8] = [M64, M64, M64, 1, 1 << 32, (1 << 32) + 1, 2, 2]
    got = mulhi64(a, b)
    want = np.array([(int(x) * int(y)) >> 64 for x, y in zip(a.tolist(), b.tolist())], dtype=np.uint64)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert np.array_equal(splitmix64(a[:100]), np.array([splitmix64_int(int(x)) for x in a[:100]], dtype=np.uint64))
    assert splitmix64_int(0) == 0xE220A8397B1DCDAF                           # splitmix64's published first output for state 0


def test_vectorised_rule_equals_python_integers(powerlaw):
    ip, ix = powerlaw
    rng = np.random.default_rng(1)
    t = rng.integers(0, len(ip) - 1, size=5000)
    deg = np.concatenate([rng.integers(1, 80, size=4000), rng.integers(1, 1 << 40, size=1000)])
    for k in (1, 5, 32):
        key = labor_key(3, 7, 1)
        assert np.array_equal(taken_mask(key, t, deg, k), taken_mask_slow(key, t, deg, k))


def test_rule_properties_on_powerlaw(powerlaw):
    ip, ix = powerlaw
    dst = np.random.default_rng(2).permutation(len(ip) - 1)[:4096].astype(np.int64)
    k = 10
    key = labor_key(5, 3, 0)
    deg, rows, (src, lp, loc, eid) = _rows(ip, ix, dst, k, key)
    assert (deg <= k).any() and (deg > k).any()
    # rows with deg <= k are complete, in CSC order
    for d in np.nonzero(deg <= k)[0]:
        assert np.array_equal(rows[d], ix[ip[dst[d]]: ip[dst[d] + 1]])
    # edge ids ascend inside a row and belong to it; repeated edges are taken or left together
    for d in range(len(dst)):
        e = eid[lp[d]: lp[d + 1]]
        assert np.all(np.diff(e) > 0) and np.all((e >= ip[dst[d]]) & (e < ip[dst[d] + 1]))
        col = ix[ip[dst[d]]: ip[dst[d] + 1]]
        assert np.array_equal(np.isin(col, rows[d]).nonzero()[0] + ip[dst[d]], e)
    # two destinations of equal degree agree on every source they share; the test is monotone in the degree: a source taken at
    # degree d is taken at every smaller degree of the layer
    lowest_left = {}     # source -> smallest degree at which it was left out
    highest_taken = {}   # source -> largest degree at which it was taken
    for d in range(len(dst)):
        col = ix[ip[dst[d]]: ip[dst[d] + 1]]
        took = set(rows[d].tolist())
        for t in set(col.tolist()):
            if t in took:
                highest_taken[t] = max(highest_taken.get(t, 0), int(deg[d]))
            else:
                lowest_left[t] = min(lowest_left.get(t, 1 << 62), int(deg[d]))
    shared = set(lowest_left) & set(highest_taken)
    assert len(shared) > 100, "the batch must share sources between rows for this check to mean anything"
    assert all(highest_taken[t] < lowest_left[t] for t in shared)
    # the block: dst nodes first, no repeats, local indices point at the taken nodes; first appearance as in _full_ref.full_layer
    assert np.array_equal(src[: len(dst)], dst) and len(np.unique(src)) == len(src)
    assert np.array_equal(src[loc], ix[eid])
    assert np.array_equal(edge_weights(lp), np.repeat(1 / np.diff(lp).astype(np.float32), np.diff(lp)).astype(np.float32))
    # ... checked by filtering the graph to the taken edges and taking the full layer of that graph
    keep = np.zeros(len(ix), dtype=bool)
    keep[eid] = True
    ip_f = np.concatenate([[0], np.cumsum(keep)])[ip]
    src_f, lp_f, loc_f = full_layer(ip_f, ix[keep], dst)
    assert np.array_equal(src_f, src) and np.array_equal(lp_f, lp) and np.array_equal(loc_f, loc)


def test_out_of_range_destination_and_duplicates(powerlaw):
    ip, ix = powerlaw
    n = len(ip) - 1
    dst = np.array([5, n + 3, 5, -2, 9], dtype=np.int64)
    src, lp, loc, eid = labor_layer(ip, ix, dst, 3, labor_key(0, 0, 0))
    assert lp[2] == lp[1] and lp[4] == lp[3], "an out-of-range destination id gives an empty row"
    assert np.array_equal(loc[lp[0]: lp[1]], loc[lp[2]: lp[3]]), "a repeated destination repeats its row"


def test_layer_dependency_shares_the_draws():
    t = np.arange(1000)
    same = [source_draws(labor_key(4, 9, l, layer_dependency=True), t) for l in (0, 1)]
    diff = [source_draws(labor_key(4, 9, l, layer_dependency=False), t) for l in (0, 1)]
    assert np.array_equal(same[0], same[1])
    assert not np.any(diff[0] == diff[1])
    assert not np.any(same[0] == diff[0])
    assert labor_key(4, 9, 0) != labor_key(4, 10, 0) != labor_key(5, 9, 0)


def test_labor_stream_is_its_own():
    """labor_key is the two outer rounds of the uniform path's sample_key xor a constant: never the key of a uniform or weighted row."""
    from _weighted_ref import STREAM as WEIGHTED, sample_key
    from _labor_ref import STREAM
    assert STREAM != WEIGHTED
    v = np.arange(100)
    r = source_draws(labor_key(1, 2, 0), v)
    assert not np.any(r == sample_key(1, 2, 0, v)) and not np.any(r == sample_key(1, 2, 0, v) ^ np.uint64(WEIGHTED))


@pytest.mark.parametrize("k", [1, 5, 10, 32])
def test_mean_picks_per_sampled_row(powerlaw, k):
    """Rows with deg > k hold k neighbours in expectation: the mean over >= 10^5 such rows lies within 2 % of k.
    The rows are those of 32 calls (steps 0..31, 4096 rows with deg > k each, 131,072 in all), not of one: the draws of one call are
    shared by its rows -- that is the method -- so a single call's mean moves with the draw of its most popular sources (one node of
    this graph is the source of 1.7 % of all edges, and one call's mean was seen 4 % off), however many rows it has.  Over
    independent calls these deviations average out as 1 / sqrt(calls)."""
    ip, ix = powerlaw
    deg_all = ip[1:] - ip[:-1]
    pool = np.nonzero(deg_all > k)[0].astype(np.int64)
    rng = np.random.default_rng(k)
    picks = rows = 0
    for step in range(32):
        dst = rng.choice(pool, 4096, replace=False)
        _, lp, _, _ = labor_layer(ip, ix, dst, k, labor_key(11, step, 0))
        picks += int(lp[-1])
        rows += len(dst)
    mean = picks / rows
    print(f"k={k}: mean picks per sampled row {mean:.4f} ({mean / k:.4f} k) over {rows} rows of 32 calls")
    assert rows >= 100_000 and abs(mean / k - 1) <= 0.02


def test_reference_layers_chain(powerlaw):
    ip, ix = powerlaw
    seeds = np.arange(100, 400, dtype=np.int64)
    ref = reference_layers(ip, ix, seeds, [5, -1, 3], 1, 2)
    dst = seeds
    for l, (src, lp, loc, eid) in enumerate(ref):
        assert np.array_equal(src[: len(dst)], dst) and len(lp) == len(dst) + 1 and len(loc) == len(eid) == lp[-1]
        assert np.array_equal(src[loc], ix[eid])
        dst = src
    assert np.array_equal(np.diff(ref[1][1]), ip[ref[0][0] + 1] - ip[ref[0][0]]), "the -1 layer keeps every in-edge"


def test_labor_symbol_is_exported(hiplib):
    from COALA_GNN_Pybind import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "coala_sampler_sample_layers_labor")
    assert "coala_sampler_sample_layers_labor" in _capi.SYMBOLS


def test_labor_entry_refuses_bad_arguments_before_any_device_call(hiplib):
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    lay = (_capi.SamplerLayer * 1)(_capi.SamplerLayer(None, None, None, 0, 0))
    rc = L.coala_sampler_sample_layers_labor(None, None, 0, (C.c_int32 * 1)(5), 1, 0, 0, lay, None, 0, None, None, None, None, None)
    assert rc == _capi.EINVAL and "null" in _capi.last_error()


def test_argument_validation(hiplib):
    from COALA_GNN.sampler import LaborSampler, NeighborSampler
    s = LaborSampler([10, -1, 5], seed=3, bucket_by_owner=4, edge_ids=True, layer_dependency=True)
    assert isinstance(s, NeighborSampler) and s.fanouts == [10, -1, 5] and s.layer_dependency and s.step == 0
    assert s.stream_safe and s.completes_on_host and s.bucket_by_owner == 4 and s.edge_ids
    for name in ("sample", "sample_begin", "sample_end", "make_graph"):
        assert callable(getattr(s, name))
    assert not LaborSampler([5]).layer_dependency
    with pytest.raises(ValueError, match="prob"):
        LaborSampler([5], prob="w")
    with pytest.raises(ValueError, match="importance_sampling"):
        LaborSampler([5], importance_sampling=1)
    for f in (0, 33):
        with pytest.raises(ValueError, match="fan-out"):
            LaborSampler([5, f])
    with pytest.raises(ValueError, match="bucket_by_owner"):
        LaborSampler([5], bucket_by_owner=65)
