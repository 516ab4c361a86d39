"""The twin construction of the wide sampler tests (tests/_wide.py), checked on the CPU.

The wide GPU file compares a graph of more than 2^32 edges with restatements run on a small twin T.  That argument is tested here, on the
same layout scaled down to boundaries 2^12 and 2^13 (and a smaller S, so that two hub rows fit between them), where G itself fits in
numpy: for one call of every kind and for the edge batch the restatement run on G equals the restatement run on T moved through
to_wide().  Then: the layout conditions at the real boundaries (indptr only), the checker raising on a simulated 32-bit wrap, and the
rules the GPU file leans on -- no near tie in a weighted reference, and every reference reaching both sides of every boundary."""
import types

import numpy as np
import pytest

import _edge_batch_ref as EB
import _sampler_sweep as S
import _wide as W


@pytest.fixture(scope="module")
def scaled():
    """kind -> (Layout at the scaled-down boundaries, G in numpy, T, seeds)"""
    out = {}
    for kind, kw in (("hub", dict(n_plain=200, hub_degree=1000)), ("typed", dict(fanouts=(1, 5), n_plain=100, hub_degree=500))):
        lay = W.Layout(W.small_graph(kind, W.GRAPH_SEED, **kw), W.SMALL_BOUNDARIES, W.SMALL_FILLER_DEGREE)
        lay.check()
        out[kind] = (lay, lay.wide_numpy(), lay.twin(), lay.seeds(120, rng_seed=3))
    return out


@pytest.fixture(scope="module")
def real():
    """kind -> (Layout at 2^31 and 2^32, seeds): indptr and T only."""
    return {kind: (lay, lay.seeds(W.N_SEEDS)) for kind, lay in ((k, W.Layout(W.small_graph(k, W.GRAPH_SEED))) for k in ("hub", "typed"))}


def _same_refs(on_G, on_T, where):
    assert len(on_G) == len(on_T)
    for l, (a, b) in enumerate(zip(on_G, on_T)):
        assert set(a) == set(b), where
        for key in a:
            x, y = a[key], b[key]
            assert (x is None) == (y is None), f"{key}, layer {l}: {where}"
            if x is not None:
                assert x.dtype == y.dtype and x.shape == y.shape, f"{key}, layer {l}: {where}"
                same = np.array_equal(x.view(np.int32), y.view(np.int32)) if x.dtype == np.float32 else np.array_equal(x, y, equal_nan=True)
                assert same, f"{key} differs, layer {l}: {where}"


@pytest.mark.parametrize("name", sorted(W.wide_calls(1)))
def test_restatement_on_G_equals_twin_through_to_wide(scaled, oracle, name):
    kind, call = W.wide_calls(0)[name]
    lay, G, T, seeds = scaled[kind]
    call = call._replace(n_seeds=len(seeds))
    assert len(np.unique(seeds)) == len(seeds) and np.all(lay.live[seeds])
    on_G = S.reference(call, G, oracle, seeds)
    on_T = W.widen(lay, S.reference(call, T, oracle, seeds))
    _same_refs(on_G, on_T, f"{name}: {call}")
    if call.edge_ids:
        e = W.ref_edge_ids(on_G)
        assert all(np.any((e >= a) & (e < b)) for a, b in zip((0,) + lay.boundaries, lay.boundaries + (lay.E,))), "a range of positions is never taken"
    for r in on_G:        # closure: nothing leaves the live groups
        assert np.all(lay.live[r["src"]])


def test_scaled_down_layout_and_position_maps(scaled):
    for kind, (lay, G, T, seeds) in scaled.items():
        assert lay.E == len(G.indices) and len(T.indices) == 3 * lay.e_small
        pos = np.arange(lay.E)
        assert np.array_equal(lay.indices_at(pos), G.indices)
        live = lay.is_live(pos)
        assert live.sum() == len(T.indices) and np.all(G.indices[~live] == lay.sink) and np.all(G.weights[~live] == 1) and np.all(G.etype[~live] == 0)
        t = np.arange(len(T.indices))
        assert np.array_equal(lay.to_wide(t), pos[live]) and np.array_equal(lay.to_twin(pos[live]), t)
        assert np.array_equal(G.indices[lay.to_wide(t)], T.indices) and np.array_equal(G.weights[lay.to_wide(t)], T.weights)
        assert np.array_equal(lay.to_wide(np.array([[-1, 0]])), [[-1, lay.group_pos[0][0]]])
        with pytest.raises(AssertionError):
            lay.to_twin(np.array([0]))
        # the seeds: every hub, the ends of every group, the degree classes
        assert np.all(np.isin(lay.hubs, seeds)) and all(ids[0] in seeds and ids[-1] in seeds for ids in lay.live_ids)
        deg = np.diff(lay.indptr)[seeds]
        assert {0, 1, 4, 5, 6, 10}.issubset(set(deg.tolist()))


@pytest.mark.parametrize("k", [0, 5, 64])
def test_edge_batch_on_G_equals_twin(scaled, k):
    lay, G, T, _ = scaled["hub"]
    eids = lay.edge_batch_eids(rng_seed=k)
    live = lay.is_live(eids)
    assert (~live).sum() == 3 and eids[12] == lay.E - 1 and not live[13] and not live[14] and eids[13] < lay.boundaries[0] < eids[14] < lay.boundaries[1]
    want = EB.edge_batch(G.indptr, G.indices, eids, k, seed=11, step=3)
    W.same_edge_batch(lay.edge_batch_ref(eids, k, seed=11, step=3), want)
    assert want["n_bad"] == 0
    bad = eids.copy()
    bad[[3, 40]] = [-1, lay.E]
    got = lay.edge_batch_ref(bad, k, seed=2, step=0)
    W.same_edge_batch(got, EB.edge_batch(G.indptr, G.indices, bad, k, seed=2, step=0))
    assert got["n_bad"] == 2


def test_layout_conditions_at_the_real_boundaries(real):
    for kind, (lay, seeds) in real.items():
        assert lay.boundaries == (2**31, 2**32) and lay.check()
        assert 2**32 < lay.E < 2**32 + 2**20 and lay.N < 2**17 and lay.max_in_degree == W.FILLER_DEGREE
        assert len(lay.indices_T) == 3 * lay.e_small and lay.small.graph is S.build_graph((kind, W.GRAPH_SEED))
        ip = lay.indptr
        for b, h in zip(lay.boundaries, lay.hubs):
            assert ip[h + 1] - ip[h] >= S.HUB and ip[h] < b - 2000 and b + 2000 < ip[h + 1]
        assert ip[lay.live_ids[2][0]] > 2**32
        assert 290 <= len(seeds) <= 360 and len(np.unique(seeds)) == len(seeds) and np.all(lay.live[seeds])
        assert np.all(np.isin(lay.hubs, seeds)) and all(ids[0] in seeds and ids[-1] in seeds for ids in lay.live_ids)
        assert np.all(np.isin(lay.live_ids[0][lay.small.special], seeds))
        eids = lay.edge_batch_eids()
        assert np.array_equal(eids[:6], [2**31 - 1, 2**31, 2**31 + 1, 2**32 - 1, 2**32, 2**32 + 1]) and np.all(lay.is_live(eids[:12]))
        assert (~lay.is_live(eids)).sum() == 3 and eids[13] < 2**31 < eids[14] < 2**32 and eids[15] == eids[1]
        assert np.array_equal(lay.to_wide(lay.to_twin(eids[:12])), eids[:12])


def test_weighted_references_have_no_near_tie_and_every_reference_reaches_both_sides(real, oracle):
    """What the GPU file assumes of its references, settled here from the references alone: _sampler_sweep's rule for weighted calls
    (the smallest margin is at least 1e-9, so the GPU file tolerates no row), and edge ids on both sides of both boundaries."""
    for name, (kind, call) in W.wide_calls(0).items():
        lay, seeds = real[kind]
        call = call._replace(n_seeds=len(seeds))
        ref = W.widen(lay, S.reference(call, lay.twin(), oracle, seeds))
        if call.kind == "weighted":
            assert np.isfinite(S.smallest_margin(ref)) and S.smallest_margin(ref) >= 1e-9, name
        if call.edge_ids:
            e = W.ref_edge_ids(ref)
            assert lay.covers(e) and np.any(e > 2**32) and np.any((e > 2**31) & (e < 2**32)) and np.any((e >= 0) & (e < 2**31)), name
        assert max(S.layer_items(call, ref)) <= S.ITEM_CAP, name


# ---------------------------------------------------------------------------------------------------- the checker rejects a wrap
def _fake_block(src, loc, eid, n_dst):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return types.SimpleNamespace(src_nodes=t(src), nbr=t(loc), indptr=None, indices=None, dst_in_src=None, num_dst=n_dst, edata={"_ID": t(eid)})


def test_checker_rejects_a_simulated_32_bit_wrap(scaled, oracle):
    """A uniform layer and an edge batch recomputed on the scaled-down G with every position reduced mod the lower boundary: what a
    kernel computes whose position arithmetic lost its 64-bit cast.  check_call and the edge-batch comparison must raise; the same
    recomputation without the wrap must pass (so it is the wrap they reject)."""
    lay, G, T, seeds = scaled["hub"]
    call = W._call("uniform", [5], len(seeds))
    ref = W.widen(lay, S.reference(call, T, oracle, seeds))
    src, loc, eid = W.uniform_layer_by_position(G.indptr, G.indices, seeds, 5, call.seed, call.step, 0)
    S.check_call(call, [_fake_block(src, loc, eid, len(seeds))], ref)
    B = lay.boundaries[0]
    for wrap_ids in (False, True):
        src, loc, eid = W.uniform_layer_by_position(G.indptr, G.indices, seeds, 5, call.seed, call.step, 0, wrap=B, wrap_ids=wrap_ids)
        with pytest.raises(AssertionError):
            S.check_call(call, [_fake_block(src, loc, eid, len(seeds))], ref)
    # a wrap that only the edge ids show: the reads are right, the reported id is reduced
    src, loc, eid = W.uniform_layer_by_position(G.indptr, G.indices, seeds, 5, call.seed, call.step, 0)
    with pytest.raises(AssertionError, match="edge ids differ"):
        S.check_call(call, [_fake_block(src, loc, np.where(eid >= 0, eid % B, -1), len(seeds))], ref)
    eids = lay.edge_batch_eids()
    want = lay.edge_batch_ref(eids, 5, seed=11, step=3)
    W.same_edge_batch(W.edge_batch_by_position(G.indptr, G.indices, eids, 5, 11, 3), want)
    with pytest.raises(AssertionError):
        W.same_edge_batch(W.edge_batch_by_position(G.indptr, G.indices, eids, 5, 11, 3, wrap=B), want)
