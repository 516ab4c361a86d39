"""GPU tests of edge exclusion on sampled blocks (Block.exclude_edges, coala_block_exclude_edges[_csr]) and of the wrapper that applies
it (EdgePredictionSampler(exclude=...)): bit for bit against the numpy restatement (tests/_edge_batch_ref.py) applied to the same seed
and step sampled without exclusion."""
import numpy as np
import pytest

import _edge_batch_ref as R
from _rel_fanout_ref import sort_by_type

pytestmark = pytest.mark.gpu

NUM_RELS = 3
U = 2.0 ** -24


@pytest.fixture(scope="module")
def setup(hiplib):
    import torch
    from COALA_GNN.sampler import NeighborSampler
    ip, ix, hub = R.link_graph(n_plain=2000, hub_degree=5000, seed=8)
    rng = np.random.default_rng(8)
    et = rng.integers(0, NUM_RELS, size=len(ix)).astype(np.int64)
    perm = sort_by_type(ip, et)
    ix, et = ix[perm], et[perm]
    w = rng.random(len(ix)).astype(np.float32)
    g = NeighborSampler([1]).make_graph(torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda(),
                                        edata={"etype": torch.from_numpy(et).cuda(), "w": torch.from_numpy(w).cuda()})
    yield torch, g, ip, ix, et, w, hub
    g.close()


def _samplers(G):
    from COALA_GNN.sampler import LaborSampler, NeighborSampler, RelNeighborSampler
    return {
        "nbr_3_5": lambda: NeighborSampler([3, 5], seed=4, bucket_by_owner=G, edge_ids=True),
        "nbr_32": lambda: NeighborSampler([32], seed=4, bucket_by_owner=G, edge_ids=True),
        "nbr_full_5": lambda: NeighborSampler([-1, 5], seed=4, bucket_by_owner=G, edge_ids=True),
        "labor_5_5": lambda: LaborSampler([5, 5], seed=4, bucket_by_owner=G, edge_ids=True),
        "rel": lambda: RelNeighborSampler([[2, 0, 3], [-1, 1, 2]], NUM_RELS, seed=4, bucket_by_owner=G),
    }


def _np(t):
    return None if t is None else t.cpu().numpy()


def _check_against_reference(got, plain, excluded):
    """got: the excluded block; plain: the same block sampled without exclusion; excluded: sorted int64 numpy."""
    assert np.array_equal(_np(got.src_nodes), _np(plain.src_nodes)) and got.num_dst == plain.num_dst
    for a, b in ((got.dst_in_src, plain.dst_in_src), (got.owner_counts, plain.owner_counts)):
        assert (a is None) == (b is None) and (a is None or np.array_equal(_np(a), _np(b)))
    eid = _np(plain.edata["_ID"])
    if plain.nbr is not None:
        want_n, want_e = R.exclude_fixed(_np(plain.nbr), eid, excluded)
        assert got.nbr.dtype == plain.nbr.dtype and np.array_equal(_np(got.nbr), want_n)
        assert np.array_equal(_np(got.edata["_ID"]), want_e)
        return int((want_n >= 0).sum()), int((_np(plain.nbr) >= 0).sum())
    wp, wi, we = R.exclude_csr(_np(plain.indptr), _np(plain.indices), eid, excluded)
    assert got.nbr is None and got.indices.dtype == plain.indices.dtype and got.indptr.dtype == plain.indptr.dtype
    assert np.array_equal(_np(got.indptr), wp) and np.array_equal(_np(got.indices), wi) and np.array_equal(_np(got.edata["_ID"]), we)
    return len(wi), len(eid)


def _parity(torch, b):
    """Every native aggregate on block b against its _torch form in float64 (the tolerance of tests/_dispatch_parity.py)."""
    rng = np.random.default_rng(b.num_src)
    dev = b.src_nodes.device
    slots = b.indices if b.nbr is None else b.nbr
    h = torch.from_numpy(rng.standard_normal((b.num_src, 12)).astype(np.float32)).to(dev)
    w = torch.from_numpy((0.1 + rng.random(tuple(slots.shape))).astype(np.float32)).to(dev)
    et = b.edata["etype"]
    assert et.shape == slots.shape
    feat = torch.from_numpy(rng.standard_normal((b.num_src, 2, 6)).astype(np.float32)).to(dev)
    el = torch.from_numpy(rng.standard_normal((b.num_src, 2)).astype(np.float32)).to(dev)
    er = torch.from_numpy(rng.standard_normal((b.num_dst, 2)).astype(np.float32)).to(dev)
    q = torch.from_numpy(rng.standard_normal((b.num_dst, 2, 6)).astype(np.float32)).to(dev)
    el3 = torch.from_numpy(rng.standard_normal((b.num_src, NUM_RELS, 2)).astype(np.float32)).to(dev)
    er3 = torch.from_numpy(rng.standard_normal((b.num_dst, NUM_RELS, 2)).astype(np.float32)).to(dev)
    feat4 = torch.from_numpy(rng.standard_normal((b.num_src, NUM_RELS, 2, 6)).astype(np.float32)).to(dev)
    d = lambda t: t.double()
    ops = {
        "mean": (lambda: b.mean_aggregate(h), lambda c: b.mean_aggregate_torch(c(h))),
        "weighted_sum": (lambda: b.weighted_sum_aggregate(h, w), lambda c: b.weighted_sum_aggregate_torch(c(h), c(w))),
        "max": (lambda: b.max_aggregate(h), lambda c: b.max_aggregate_torch(c(h))),
        "rel_sum": (lambda: b.rel_sum_aggregate(h, et, NUM_RELS, w), lambda c: b.rel_sum_aggregate_torch(c(h), et, NUM_RELS, c(w))),
        "gat": (lambda: b.gat_aggregate(el, er, feat), lambda c: b.gat_aggregate_torch(c(el), c(er), c(feat))),
        "gatv2": (lambda: b.gatv2_aggregate(feat, q, feat[0]), lambda c: b.gatv2_aggregate_torch(c(feat), c(q), c(feat[0]))),
        "rel_gat": (lambda: b.rel_gat_aggregate(el3, er3, feat4, et, NUM_RELS), lambda c: b.rel_gat_aggregate_torch(c(el3), c(er3), c(feat4), et, NUM_RELS)),
        "dot_gat": (lambda: b.dot_gat_aggregate(q, feat, feat), lambda c: b.dot_gat_aggregate_torch(c(q), c(feat), c(feat))),
    }
    for name, (native, torch_form) in ops.items():
        got, want, low = native(), torch_form(d), torch_form(lambda t: t)
        assert tuple(got.shape) == tuple(want.shape), name
        e = float((low.double() - want).abs().max()) if want.numel() else 0.0
        tol = max(4.0 * e, 8.0 * U * float(want.abs().max()) if want.numel() else 0.0)
        err = float((got.double() - want).abs().max()) if want.numel() else 0.0
        assert err <= tol, f"{name}: error {err:.3e} above {tol:.3e}"


@pytest.mark.parametrize("G", [0, 4])
@pytest.mark.parametrize("kind", ["nbr_3_5", "nbr_32", "nbr_full_5", "labor_5_5", "rel"])
def test_wrapper_equals_plain_sample_then_mask(setup, kind, G):
    torch, g, ip, ix, et, w, hub = setup
    from COALA_GNN.sampler import EdgePredictionSampler, UniformNegativeSampler
    rng = np.random.default_rng(3)
    eids = np.concatenate([[0, len(ix) - 1, ip[hub], ip[hub] + 1], rng.integers(0, len(ix), size=252)]).astype(np.int64)
    wrapped = EdgePredictionSampler(_samplers(G)[kind](), exclude="self", negative_sampler=UniformNegativeSampler(2))
    input_nodes, batch, blocks = wrapped.sample(g, torch.from_numpy(eids).cuda(), step=6)
    want = R.edge_batch(ip, ix, eids, 2, seed=4, step=6)
    assert np.array_equal(_np(batch.seed_nodes), want["seed_nodes"]) and np.array_equal(_np(batch.pos_dst), want["pos_dst"])
    p_in, p_seeds, p_blocks = _samplers(G)[kind]().sample(g, batch.seed_nodes, step=6)
    assert torch.equal(input_nodes, p_in) and input_nodes is blocks[0].src_nodes and len(blocks) == len(p_blocks)
    assert torch.equal(blocks[-1].dstdata["_ID"], batch.seed_nodes)
    excluded = np.unique(eids)
    removed = 0
    for got, plain in zip(blocks, p_blocks):
        left, before = _check_against_reference(got, plain, excluded)
        removed += before - left
        assert not np.isin(_np(got.edata["_ID"]), excluded).any()
        eid = got.edata["_ID"]
        assert torch.equal(got.edata["w"], torch.where(eid >= 0, g.edata["w"][eid.clamp_min(0)], 0.0))     # graph edata through the new ids
        if kind == "labor_5_5":
            deg = np.diff(_np(got.indptr))
            assert np.array_equal(_np(got.edata["edge_weights"]), np.repeat((1.0 / deg[deg > 0].astype(np.float32)), deg[deg > 0]))
        _parity(torch, got)
    assert removed > 0, "the seed edges were in no block: the case checks nothing"


@pytest.mark.parametrize("kind", ["nbr_32", "nbr_full_5", "labor_5_5"])
def test_exclusion_lists(setup, kind):
    """Block.exclude_edges with lists of 0, 1 and 2048 ids, a list of foreign ids only, and a row that loses every slot; native against
    the restatement and against exclude_edges_torch."""
    torch, g, ip, ix, et, w, hub = setup
    rng = np.random.default_rng(5)
    N = len(ip) - 1
    seeds = np.concatenate([[hub], np.setdiff1d(rng.permutation(N)[:700], [hub])]).astype(np.int64)
    make = _samplers(0)[kind]
    sample = lambda: make().sample(g, torch.from_numpy(seeds).cuda(), step=2)[2]
    plain = sample()
    for layer in range(len(plain)):
        eid = _np(plain[layer].edata["_ID"])
        present = np.unique(eid[eid >= 0])
        foreign = np.setdiff1d(np.arange(len(ix)), present)
        hub_row = eid[0] if plain[layer].nbr is not None else eid[: int(plain[layer].indptr[1])]
        lists = {"empty": np.zeros(0, np.int64), "one": present[len(present) // 2:][:1], "foreign": foreign[:: max(len(foreign) // 500, 1)],
                 "row": np.unique(hub_row[hub_row >= 0]),
                 "2048": np.unique(np.concatenate([rng.choice(present, min(1500, len(present)), replace=False), rng.choice(foreign, 548, replace=False)]))}
        if layer == len(plain) - 1:
            assert len(lists["row"]) >= 32 if kind == "nbr_32" else len(lists["row"]) > 0
        for name, ex in lists.items():
            ex_t = torch.from_numpy(np.ascontiguousarray(ex, dtype=np.int64)).cuda()
            got = plain[layer].exclude_edges(ex_t)
            left, before = _check_against_reference(got, plain[layer], ex)
            via_torch = plain[layer].exclude_edges_torch(ex_t)
            _check_against_reference(via_torch, plain[layer], ex)
            if name in ("empty", "foreign"):
                assert left == before
            if name == "row" and layer == len(plain) - 1:
                assert int(got.in_degrees()[0]) == 0, "the hub row keeps an edge"
                if got.nbr is not None:
                    assert got.nbr.shape[1] == (32 if kind == "nbr_32" else 5)
                    assert bool((got.nbr[0] == -1).all()) and bool((got.edata["_ID"][0] == -1).all())     # a row that lost every slot
    b = sample()[0]
    b.edata["w"]
    with pytest.raises(RuntimeError):
        b.exclude_edges(torch.zeros(1, dtype=torch.int64, device="cuda"))


def test_blocks_without_edge_ids_are_refused(setup):
    torch, g, ip, ix, et, w, hub = setup
    from COALA_GNN.sampler import NeighborSampler, RandomWalkNeighborSampler
    seeds = torch.arange(10, 40, device="cuda")
    for s in (NeighborSampler([3]), RandomWalkNeighborSampler(3, 2, 0.5, 4)):
        with pytest.raises(ValueError, match="edge ids"):
            s.sample(g, seeds)[2][0].exclude_edges(torch.zeros(1, dtype=torch.int64, device="cuda"))
