"""CPU tests of the full-layer feature (fan-out -1): NeighborSampler's fan-out validation, the Manager's request-buffer bound, and the
numpy restatement of a full layer (tests/_full_ref.py, the reference of test_sampler_full_gpu.py) pinned to the CPU twin: on a graph
whose degrees are all <= f, a fixed layer of fan-out f takes every in-edge, so the twin's dense block minus its -1 padding is the
full layer."""
import numpy as np
import pytest

from _full_ref import full_layer
from _util import csc_from_columns, edge_case_graph


@pytest.mark.parametrize("fanouts", [[-1], [-1, -1], [5, -1], [-1, 5], [32, -1, 1], [1, 32, 16]])
def test_neighbor_sampler_accepts_full_and_fixed_fanouts(hiplib, fanouts):
    from COALA_GNN.sampler import NeighborSampler
    assert NeighborSampler(fanouts).fanouts == fanouts


@pytest.mark.parametrize("fanouts", [[0], [-2], [33], [5, 0], [-1, -3], [10, 64]])
def test_neighbor_sampler_rejects_bad_fanouts(hiplib, fanouts):
    from COALA_GNN.sampler import NeighborSampler
    with pytest.raises(ValueError, match="fan-out"):
        NeighborSampler(fanouts)


def test_manager_request_buffer_bound(hiplib):
    from COALA_GNN.COALA_GNN_Manager import request_buffer_rows
    assert request_buffer_rows(1024, [5, 5]) == 1024 * 36                   # today's value: batch * prod(f + 1)
    assert request_buffer_rows(1000, [10, 15, 5], num_rows=7) == 1000 * 11 * 16 * 6
    assert request_buffer_rows(1024, ["5", "10"]) == 1024 * 66
    assert request_buffer_rows(1024, [-1]) == 8_388_608                      # the sampler's item limit
    assert request_buffer_rows(1024, [5, -1], num_rows=200_000) == 200_000   # no more than the table's rows
    assert request_buffer_rows(1024, [-1, -1], num_rows=10**9) == 8_388_608
    assert request_buffer_rows(64, [-1, 5], num_rows=100) == 100


def _twin_dense(oracle, indptr, indices, dst, f):
    O = oracle
    dst = np.ascontiguousarray(dst, dtype=np.int64)
    nbr = np.empty(len(dst) * f, dtype=np.int64)
    O.lib().orc_sample_layer(O._ptr(indptr), O._ptr(indices), len(indptr) - 1, O._ptr(dst), len(dst), f, 3, 4, 0, O._ptr(nbr))
    src = np.empty(len(dst) * (f + 1), dtype=np.int64)
    local = np.empty(len(dst) * f, dtype=np.int32)
    n_src = O.lib().orc_compact_block(O._ptr(dst), len(dst), O._ptr(nbr), f, O._ptr(src), O._ptr(local))
    return src[:n_src], local.reshape(len(dst), f)


@pytest.mark.parametrize("case", ["edge", "random", "empty_rows"])
def test_full_layer_restatement_matches_twin_on_small_degrees(oracle, case):
    rng = np.random.default_rng(len(case))
    if case == "edge":           # degrees 0, 1, f-1, f, self-loops, repeated neighbours (edge_case_graph without its 2f / 200 rows)
        ip, ix, special = edge_case_graph([8], n_plain=500, seed=3)
        deg = ip[1:] - ip[:-1]
        dst = np.concatenate([special[deg[special] <= 8], np.arange(len(special), len(special) + 200)])
        f = 8
    elif case == "random":
        n = 5000
        ip, ix = csc_from_columns([rng.integers(0, n, size=rng.integers(0, 13)) for _ in range(n)])
        dst = rng.permutation(n)[:700]
        f = 12
    else:                        # every destination has degree 0: no edges at all
        ip, ix = csc_from_columns([[] for _ in range(50)] + [[1, 2]])
        dst = np.arange(50)
        f = 1
    ip, ix = ip.astype(np.int64), ix.astype(np.int64)
    assert (ip[dst + 1] - ip[dst]).max() <= f
    src_t, loc_t = _twin_dense(oracle, ip, ix, dst, f)
    src, ind, loc = full_layer(ip, ix, dst)
    assert np.array_equal(src, src_t)
    valid = loc_t >= 0
    assert not np.any(valid[:, 1:] & ~valid[:, :-1])
    assert np.array_equal(np.diff(ind), valid.sum(1))
    assert np.array_equal(loc, loc_t[valid])            # row-major: the dense rows with their -1 padding removed
    assert ind[0] == 0 and ind[-1] == len(loc) and loc.dtype == np.int32
