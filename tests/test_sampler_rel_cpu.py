"""The relation-layer restatement (tests/_rel_fanout_ref.py, the reference of test_sampler_rel_gpu.py) checked on its own, without a
GPU: the rule's row counts, its two pinned consequences (all -1 is the full layer; one relation holds the uniform sampler's edges),
the inclusion frequency of a drawn edge, and the host side of COALA_GNN.sampler: sort_csc_by_etype, check_etype_sorted and the
argument checks of RelNeighborSampler."""
import ctypes as C

import numpy as np
import pytest

from _full_ref import full_layer
from _rel_fanout_ref import (M64, expand_fanouts, floyd_picks, floyd_picks_slow, reference_layers, rel_layer, sample_key, sort_by_type,
                             typed_edge_case_graph)


@pytest.fixture(scope="module")
def powerlaw():
    """powerlaw_csc(200000, 30) typed by the source node (id % 3) and sorted with numpy."""
    from COALA_GNN.synthetic import powerlaw_csc
    ip, ix = powerlaw_csc(200_000, 30, seed=1, device="cpu")
    ip, ix = np.ascontiguousarray(ip.numpy()), np.ascontiguousarray(ix.numpy())
    perm = sort_by_type(ip, ix % 3)
    return ip, ix[perm], (ix % 3)[perm]


def _check_rows(ip, ix, et, dst, fan, layer):
    """Every row holds min(deg_r, f_r) edges of relation r (all for -1, none for 0), distinct, ascending, inside its column."""
    src, lp, loc, eid = layer
    N = len(ip) - 1
    assert len(lp) == len(dst) + 1 and lp[0] == 0 and lp[-1] == len(loc) == len(eid)
    assert len(np.unique(src)) == len(src) and np.array_equal(src[loc], ix[eid])
    if len(np.unique(dst)) == len(dst):                          # a repeated destination is listed once, where it first stands
        assert np.array_equal(src[: len(dst)], dst)
    for d, v in enumerate(dst):
        e = eid[lp[d]: lp[d + 1]]
        if not 0 <= v < N:
            assert len(e) == 0
            continue
        assert np.all(np.diff(e) > 0) and np.all((e >= ip[v]) & (e < ip[v + 1]))
        col = et[ip[v]: ip[v + 1]]
        for r, f in enumerate(fan):
            deg_r = int((col == r).sum())
            want = 0 if f == 0 else deg_r if f < 0 else min(deg_r, f)
            assert int((et[e] == r).sum()) == want, (v, r, f, deg_r)


def test_floyd_vectorised_equals_python_integers():
    rng = np.random.default_rng(0)
    key = rng.integers(0, 1 << 64, size=300, dtype=np.uint64)
    key[:2] = [M64, M64 - 70]                                    # the counter 64 r + c wraps
    for r, f in ((0, 1), (1, 5), (63, 32)):
        deg = rng.integers(f + 1, 4 * f + 3, size=300).astype(np.int64)
        deg[:5] = [f + 1, f + 1, 1_000_003, 1 << 40, f + 2]
        got = floyd_picks(key, r, deg, f)
        for i in range(300):
            assert got[i].tolist() == floyd_picks_slow(int(key[i]), r, int(deg[i]), f)
        assert np.all((got >= 0) & (got < deg[:, None]))
        assert all(len(set(row)) == f for row in got.tolist())


@pytest.mark.parametrize("fan", [[10, 3, 1], [5, 5, 5], [32, 32, 32], [1, 0, -1], [0, 0, 7], [-1, 2, 0]])
def test_row_counts(powerlaw, fan):
    ip, ix, et = powerlaw
    dst = np.random.default_rng(1).permutation(len(ip) - 1)[:300].astype(np.int64)
    _check_rows(ip, ix, et, dst, fan, rel_layer(ip, ix, et, dst, fan, 3, 4, 0))
    g_ip, g_ix, g_et, special = typed_edge_case_graph(seed=5)
    dst = np.concatenate([special, [len(g_ip) + 3, -2, special[4]]]).astype(np.int64)
    layer = rel_layer(g_ip, g_ix, g_et, dst, fan, 1, 2, 1)
    _check_rows(g_ip, g_ix, g_et, dst, fan, layer)
    lp = layer[1]
    assert np.array_equal(layer[3][lp[-2]: lp[-1]], layer[3][lp[4]: lp[5]]), "a repeated destination repeats its row"


def test_edge_case_graph_has_the_shapes():
    ip, ix, et, special = typed_edge_case_graph(hub_degree=5000, seed=2)
    rows = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    per = np.zeros((len(ip) - 1, 3), dtype=np.int64)
    np.add.at(per, (rows, et), 1)
    assert np.all(np.diff(et)[np.diff(rows) == 0] >= 0), "types are sorted inside every row"
    for f in (1, 5, 32):
        for r in range(3):
            assert {0, f - 1, f, f + 1, 2 * f, 200} <= set(per[special, r].tolist())
    for lacking in ([0], [1], [2], [0, 1, 2]):
        others = [r for r in range(3) if r not in lacking]
        assert np.any(np.all(per[special][:, lacking] == 0, 1) & np.all(per[special][:, others] > 0, 1))
    assert per[-1].tolist() == [0, 5000, 2] and special[-1] == len(ip) - 2
    assert np.any(ix == rows), "self-loops"


def test_all_minus_one_is_the_full_layer(powerlaw):
    ip, ix, et = powerlaw
    seeds = np.arange(50, 150, dtype=np.int64)
    ref = reference_layers(ip, ix, et, seeds, [[-1, -1, -1], [-1, -1, -1]], 5, 6)
    dst = seeds
    for src, lp, loc, eid in ref:
        f_src, f_lp, f_loc = full_layer(ip, ix, dst)
        assert np.array_equal(src, f_src) and np.array_equal(lp, f_lp) and np.array_equal(loc, f_loc)
        assert np.array_equal(eid, np.repeat(ip[dst] - f_lp[:-1], np.diff(f_lp)) + np.arange(len(eid)))
        dst = src


@pytest.mark.parametrize("fanouts", [[1], [5], [32], [5, 5]])
def test_one_relation_holds_the_uniform_samplers_edges(oracle, powerlaw, fanouts):
    """num_rels == 1: every row holds the neighbours the CPU twin of NeighborSampler draws at the same seed and step (the twin lists
    them in draw order and knows neighbours, not positions: compared as sorted lists per row), and so the same source set."""
    ip, ix, _ = powerlaw
    et = np.zeros(len(ix), dtype=np.int64)
    seeds = np.random.default_rng(2).permutation(len(ip) - 1)[:400].astype(np.int64)
    rev = list(reversed(fanouts))
    for seed, step in ((0, 0), (7, 3), (2**64 - 5, 2**64 - 1)):
        twin = oracle.sample_blocks(ip, ix, seeds, rev, seed, step)
        ref = reference_layers(ip, ix, et, seeds, [[f] for f in rev], seed, step)
        t_dst = r_dst = seeds   # behind the first layer the two list the same destination nodes in another order: rows go by node
        for (t_src, _, t_nbr), (src, lp, loc, eid) in zip(twin, ref):
            assert np.array_equal(np.sort(t_src), np.sort(src))
            got = np.full(t_nbr.shape, -1, dtype=np.int64)
            cols = np.arange(len(eid)) - np.repeat(lp[:-1], np.diff(lp))
            got[np.repeat(np.arange(len(lp) - 1), np.diff(lp)), cols] = ix[eid]
            assert np.array_equal(np.sort(got, 1)[np.argsort(r_dst)], np.sort(t_nbr, 1)[np.argsort(t_dst)]), f"seed {seed} step {step}"
            t_dst, r_dst = t_src, src


def test_inclusion_frequency_and_independent_streams():
    """One row with 10 edges of relation 0 (f = 3) beside 7 edges of relation 1 (f = 2), over 20,000 steps: every edge of relation 0 is
    taken with frequency within 5 sigma of 0.3 (sigma = sqrt(0.3 * 0.7 / 20000) = 0.0032: bound 0.0162), every edge of relation 1 within
    5 sigma of 2 / 7 (sigma = 0.0032: bound 0.0160) in the same run, and the two relations' picks are uncorrelated."""
    steps = 20_000
    ip = np.array([0, 17], dtype=np.int64)
    ix = np.zeros(17, dtype=np.int64)
    et = np.array([0] * 10 + [1] * 7, dtype=np.int64)
    keys = np.concatenate([sample_key(9, s, 0, [0]) for s in range(steps)])
    p0 = floyd_picks(keys, 0, np.full(steps, 10), 3)
    p1 = floyd_picks(keys, 1, np.full(steps, 7), 2)
    for s in (0, 1, 19_999):                                    # the vectorised draws are those of the layer
        _, lp, _, eid = rel_layer(ip, ix, et, [0], [3, 2], 9, s, 0)
        assert eid.tolist() == sorted(p0[s].tolist()) + sorted((10 + p1[s]).tolist())
    f0 = np.bincount(p0.reshape(-1), minlength=10) / steps
    f1 = np.bincount(p1.reshape(-1), minlength=7) / steps
    print("relation 0:", np.round(f0, 4), "relation 1:", np.round(f1, 4))
    assert np.all(np.abs(f0 - 0.3) <= 5 * np.sqrt(0.3 * 0.7 / steps))
    assert np.all(np.abs(f1 - 2 / 7) <= 5 * np.sqrt((2 / 7) * (5 / 7) / steps))
    # independence: P(edge a of relation 0 and edge b of relation 1) = 0.3 * 2 / 7 within 5 sigma, for every pair
    in0 = np.zeros((steps, 10), dtype=bool)
    in0[np.arange(steps)[:, None], p0] = True
    in1 = np.zeros((steps, 7), dtype=bool)
    in1[np.arange(steps)[:, None], p1] = True
    joint = (in0[:, :, None] & in1[:, None, :]).mean(0)
    p = 0.3 * 2 / 7
    assert np.all(np.abs(joint - p) <= 5 * np.sqrt(p * (1 - p) / steps)), np.abs(joint - p).max()


def test_sort_csc_by_etype_against_numpy():
    import torch
    from COALA_GNN.sampler import check_etype_sorted, sort_csc_by_etype
    rng = np.random.default_rng(3)
    deg = rng.integers(0, 9, size=500)
    deg[[0, 17, 499]] = 0
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = rng.integers(0, 500, size=int(ip[-1])).astype(np.int64)
    et = rng.integers(0, 5, size=len(ix)).astype(np.int64)
    w = rng.random(len(ix))
    for dtype in (torch.int64, torch.int32, torch.uint8):
        s_ix, s_et, perm = sort_csc_by_etype(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(et).to(dtype))
        want = sort_by_type(ip, et)
        assert perm.dtype == torch.int64 and np.array_equal(perm.numpy(), want), "stable by (row, type)"
        assert s_et.dtype == dtype and np.array_equal(s_ix.numpy(), ix[want]) and np.array_equal(s_et.numpy(), et[want])
        check_etype_sorted(torch.from_numpy(ip), s_et, 5)
    back = np.empty_like(w)
    back[perm.numpy()] = w[perm.numpy()]                         # other edata travels with perm, and comes back through it
    assert np.array_equal(back, w) and np.array_equal(np.sort(perm.numpy()), np.arange(len(ix)))
    with pytest.raises(ValueError, match="shape"):
        sort_csc_by_etype(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(et[:-1]))
    with pytest.raises(ValueError, match="integer"):
        sort_csc_by_etype(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(w))


def test_unsorted_types_raise():
    import torch
    from COALA_GNN.sampler import check_etype_sorted
    ip = torch.tensor([0, 3, 3, 5, 8])
    ok = torch.tensor([0, 1, 2, 0, 2, 1, 1, 2])                   # the type may fall where a row starts
    check_etype_sorted(ip, ok, 3)
    check_etype_sorted(torch.tensor([0, 0, 0]), torch.zeros(0, dtype=torch.int64), 1)
    for bad in ([0, 2, 1, 0, 2, 1, 1, 2], [0, 1, 2, 2, 0, 1, 1, 2], [0, 1, 2, 0, 2, 1, 2, 1]):   # a fall inside the first, a middle, the last row
        with pytest.raises(ValueError, match="sort_csc_by_etype"):
            check_etype_sorted(ip, torch.tensor(bad), 3)
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        check_etype_sorted(ip, ok, 2)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        check_etype_sorted(ip, torch.tensor([-1, 1, 2, 0, 2, 1, 1, 2]), 3)
    with pytest.raises(ValueError, match="shape"):
        check_etype_sorted(ip, ok[:-1], 3)
    with pytest.raises(ValueError, match="integer"):
        check_etype_sorted(ip, ok.float(), 3)


def test_rel_symbol_is_exported(hiplib):
    from COALA_GNN_Pybind import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "coala_sampler_sample_layers_rel") and "coala_sampler_sample_layers_rel" in _capi.SYMBOLS


def test_rel_entry_refuses_bad_arguments_before_any_device_call(hiplib):
    """The argument checks that need no handle: they come first, so they can be seen without a GPU."""
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    lay = (_capi.SamplerLayer * 1)(_capi.SamplerLayer(None, None, None, 0, 0))
    fan = (C.c_int32 * 2)(5, 5)

    def call(fan, num_rels, etype=1):
        return L.coala_sampler_sample_layers_rel(None, None, 0, fan, num_rels, 1, 0, 0, lay, etype, None, None, None, None, None, None)
    assert call(fan, 2, None) == _capi.EINVAL and "etype" in _capi.last_error()
    for num_rels in (0, 65, -1):
        assert call(fan, num_rels) == _capi.EINVAL and "num_rels" in _capi.last_error()
    for bad in (-2, 33):
        assert call((C.c_int32 * 2)(5, bad), 2) == _capi.EINVAL and f"fan-out {bad}" in _capi.last_error()
    assert call((C.c_int32 * 2)(0, 0), 2) == _capi.EINVAL and "fan-out 0" in _capi.last_error()
    assert call(None, 2) == _capi.EINVAL and "null" in _capi.last_error()
    assert call(fan, 2) == _capi.EINVAL and "null" in _capi.last_error()      # valid fan-outs: the null handle is what is left


def test_argument_validation(hiplib):
    from COALA_GNN.sampler import NeighborSampler, RelNeighborSampler
    s = RelNeighborSampler([[10, 3, 0, -1], 5, (1, 2, 3, 4)], 4, etype="t", seed=3, bucket_by_owner=4)
    assert isinstance(s, NeighborSampler) and s.rel_fanouts == [[10, 3, 0, -1], [5, 5, 5, 5], [1, 2, 3, 4]] and s.fanouts == [-1, 20, 10]
    assert s.rel_fanouts == expand_fanouts([[10, 3, 0, -1], 5, (1, 2, 3, 4)], 4)
    assert s.num_rels == 4 and s.etype == "t" and s.edge_ids and s.step == 0 and s.stream_safe and s.completes_on_host and s.bucket_by_owner == 4
    assert not RelNeighborSampler([5], 1, edge_ids=False).edge_ids and RelNeighborSampler([5], 1).etype == "etype"
    for name in ("sample", "sample_begin", "sample_end", "make_graph"):
        assert callable(getattr(s, name))
    with pytest.raises(ValueError, match="prob"):
        RelNeighborSampler([5], 2, prob="w")
    for num_rels in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="num_rels"):
            RelNeighborSampler([5], num_rels)
    for f in (-2, 33, [5, 33], [-2, 1]):
        with pytest.raises(ValueError, match="fan-out"):
            RelNeighborSampler([5, f], 2)
    with pytest.raises(ValueError, match="one per relation"):
        RelNeighborSampler([[5, 5, 5]], 2)
    for f in (0, [0, 0]):
        with pytest.raises(ValueError, match="at least one relation"):
            RelNeighborSampler([f], 2)
    with pytest.raises(ValueError, match="layers"):
        RelNeighborSampler([], 2)
    with pytest.raises(ValueError, match="bucket_by_owner"):
        RelNeighborSampler([5], 2, bucket_by_owner=65)
