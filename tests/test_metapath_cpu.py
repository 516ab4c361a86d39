"""CPU tests of the metapath walks: the refusals that need no GPU, synthetic.bipartite_csc, and the uniformity of a hop of the
restatement (tests/_metapath_ref.py) inside one type's segment of a row."""
import ctypes as C

import numpy as np
import pytest

import _metapath_ref as MP

ONE = 1 << 32


def _path(*types):
    return (C.c_int32 * max(len(types), 1))(*types), len(types)


def _entries(hiplib):
    """The three typed entry points with a null handle: call(path, etype, num_rels, length or traversals, thresholds)."""
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    lay, fan = (_capi.SamplerLayer * 1)(_capi.SamplerLayer(None, None, None, 0, 0)), (C.c_int32 * 1)(3)
    return _capi, dict(
        trace=lambda p, et=1, R=2, n=2, thr=None: L.coala_sampler_random_walk_metapath(None, None, 0, 1, n, 0, 0, 0, 0, et, R, *p, None, None),
        layers=lambda p, et=1, R=2, n=2, thr=None: L.coala_sampler_sample_layers_walk_metapath(
            None, None, 0, fan, 1, 0, 0, lay, C.byref(_capi.SamplerWalk(n, 4, 0)), et, R, *p, None, None, None, None, None, None),
        batch=lambda p, et=1, R=2, n=2, thr=(ONE, ONE, ONE): L.coala_sampler_walk_batch_metapath(None, None, 0, 1, n, *thr, 1, 0, 0, et, R, *p, None, None,
                                                                                                 None))


@pytest.mark.parametrize("entry", ["trace", "layers", "batch"])
def test_entry_points_refuse_bad_arguments_before_any_device_call(hiplib, entry):
    _capi, calls = _entries(hiplib)
    call = calls[entry]
    for args, word in ((dict(p=_path(0, 1), et=None), "etype"), (dict(p=(None, 2)), "metapath"), (dict(p=_path()), "1..16"), (dict(p=_path(*[0] * 17)), "1..16"),
                       (dict(p=_path(0, 2)), "outside [0, 2)"), (dict(p=_path(-1)), "outside [0, 2)"), (dict(p=_path(0, 1)), "null"),   # valid: the null handle is left
                       {"trace": (dict(p=_path(0, 1, 0), n=4), "multiple"), "layers": (dict(p=_path(0, 1, 0), n=6), "16 hops"),
                        "batch": (dict(p=_path(0, 1), n=128), "walk_length 128")}[entry],
                       {"trace": (dict(p=_path(0, 1), n=18), "length 18"), "layers": (dict(p=_path(0), n=17), "num_traversals 17"),
                        "batch": (dict(p=_path(0, 1), thr=(ONE >> 1, ONE, ONE)), "first-order")}[entry]):
        assert call(**args) == _capi.EINVAL and word in _capi.last_error(), (args, _capi.last_error())


def test_python_arguments(hiplib):
    from COALA_GNN import MetaPath2Vec, Node2Vec
    from COALA_GNN.sampler import PinSAGESampler, RandomWalkNeighborSampler, random_walk, walk_batch
    s = PinSAGESampler([3, 2], 2, 0.5, 10, [0, 1], etype="t", seed=4)
    assert isinstance(s, RandomWalkNeighborSampler) and s.metapath == [0, 1] and s.etype == "t" and s.fanouts == [3, 2] and s.num_traversals == 2
    assert RandomWalkNeighborSampler(3, 2, 0.5, 10).metapath is None and RandomWalkNeighborSampler(3, 16, 0.0, 4, metapath=(0,)).metapath == [0]
    for bad in ([], [0] * 17, [0, -1], [0, 1.0], [True], 3, "01"):
        for make in (lambda: RandomWalkNeighborSampler(3, 1, 0.5, 10, metapath=bad), lambda: random_walk(None, None, metapath=bad)):
            with pytest.raises(ValueError, match="metapath"):
                make()
    for make, word in ((lambda: PinSAGESampler(3, 2, 0.5, 10, [0]), "at least two"), (lambda: RandomWalkNeighborSampler(3, 6, 0.5, 10, metapath=[0, 1, 0]), "16 hops"),
                       (lambda: RandomWalkNeighborSampler(3, 2, 0.5, 10, metapath=[0, 1], prob="w"), "prob"), (lambda: random_walk(None, None, length=3, metapath=[0, 1]), "multiple"),
                       (lambda: walk_batch(None, None, q=2, metapath=[0, 1]), "q=2"), (lambda: walk_batch(None, None, p=0.5, metapath=[0, 1]), "p=0.5"),
                       (lambda: Node2Vec(None, 8, 4, 2, q=2.0, metapath=[0, 1]), "q=2.0"), (lambda: MetaPath2Vec(None, 8, None, 4, 2), "needs a metapath")):
        with pytest.raises(ValueError, match=word):
            make()


def test_bipartite_csc_is_sorted_and_bipartite(hiplib):
    import torch
    from COALA_GNN.sampler import check_etype_sorted
    from COALA_GNN.synthetic import bipartite_csc
    ip, ix, et = bipartite_csc(40, 60, 4, seed=3)
    check_etype_sorted(ip, et, 2)
    assert ip.dtype == ix.dtype == torch.int64 and ip.numel() == 101 and ix.numel() == et.numel() == 480 == int(ip[-1])
    rows = torch.repeat_interleave(torch.arange(100), ip[1:] - ip[:-1])
    user = rows < 40
    assert bool((ix[user] >= 40).all()) and bool((et[user] == 1).all())       # a user's in-edges come from items: item -> user
    assert bool((ix[~user] < 40).all()) and bool((et[~user] == 0).all()) and bool((ip[41:] - ip[40:-1] == 4).all())
    assert set(zip(rows[user].tolist(), ix[user].tolist())) == set(zip(ix[~user].tolist(), rows[~user].tolist())), "every edge has its reverse"
    assert all(torch.equal(a, b) for a, b in zip(bipartite_csc(40, 60, 4, seed=3), (ip, ix, et)))


def test_a_hop_is_uniform_inside_its_segment():
    """Node 0's row: 3 edges of type 0, 7 of type 1, 2 of type 2.  20,480 first hops of type 1 (64 walks at 320 steps, seed 5): every one
    lands in the segment, and each of its 7 edges is taken n / 7 times within 5 sigma (the fixed seed's largest deviation is 0.7 sigma)."""
    G = MP.TypedGraph([0, 12] + [12] * 12, list(range(1, 13)), [0] * 3 + [1] * 7 + [2] * 2)
    n, counts = 320 * 64, np.zeros(13, dtype=np.int64)
    for step in range(320):
        counts += np.bincount(MP.traces(G, [0], [1], 1, 64, 0, seed=5, step=step)[0, :, 1], minlength=13)
    assert n >= 20_000 and counts[4:11].sum() == n, "a hop left its type's segment"
    assert np.all(np.abs(counts[4:11] - n / 7) <= 5 * np.sqrt(n * (1 / 7) * (6 / 7))), counts[4:11]
