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


# ------------------------------------------------------------------------------------------- the kernels past one pass of their grid
# Hand-made blocks at the C ABI, with more rows than the largest grid has lane groups (exclude_edges_kernel: 32 lanes per row, 65,536
# rows a pass; exclude_edges_csr_kernel: a wave per row, 32,768 rows a pass), sentinel guards around every output.
PAD = 37
S64, S32 = -0x0123456789ABCDEF, -0x01234567


def _padded(torch, m, dtype, fill):
    buf = torch.full((m + 2 * PAD,), fill, dtype=dtype, device="cuda")
    return buf, buf.data_ptr() + PAD * buf.element_size()


def _inside(buf, m, fill):
    """The output's m entries, after checking the guards around them."""
    assert bool((buf[:PAD] == fill).all()) and bool((buf[PAD + m:] == fill).all()), "a write outside an output's capacity"
    return buf[PAD: PAD + m].cpu().numpy()


def _exclusion_lists(rng, eid_rows, all_ids, one):
    """Sorted lists of 0, 1 (the id `one`) and 2,048 ids; the long one holds every id of the given rows (they lose every slot)."""
    rows = np.unique(np.concatenate([e[e >= 0] for e in eid_rows]))
    assert 0 < len(rows) < 1500
    rest = np.setdiff1d(all_ids, rows)
    long = np.unique(np.concatenate([rows, rng.choice(rest, 2048 - len(rows), replace=False)]))
    assert len(long) == 2048
    return {"empty": np.zeros(0, np.int64), "one": np.array([one], dtype=np.int64), "2048": long}


@pytest.mark.parametrize("fanout", [5, 32])
def test_fixed_kernel_past_one_grid_pass(hiplib, fanout):
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    n_dst = 70_001
    assert n_dst * 32 > 8192 * 256
    rng = np.random.default_rng(fanout)
    nbr = rng.integers(0, 1 << 20, size=(n_dst, fanout)).astype(np.int32)
    nbr[rng.random((n_dst, fanout)) < 0.2] = -1                      # -1 anywhere in a row
    nbr[[5, 65_540]] = -1                                            # rows without a slot
    nbr[[0, 65_535, 65_536, 65_537, n_dst - 1], 0] = 7               # ... and the rows the long list empties have one for sure
    eid = rng.permutation(2 * n_dst * fanout)[: n_dst * fanout].reshape(n_dst, fanout).astype(np.int64)
    eid[nbr < 0] = -1
    emptied = [0, 65_535, 65_536, 65_537, n_dst - 1]                 # around the first row of the second pass, and the last row
    lists = _exclusion_lists(rng, [eid[r] for r in emptied], eid[eid >= 0], one=eid[-1][nbr[-1] >= 0][0])
    d_nbr, d_eid = torch.from_numpy(nbr).cuda(), torch.from_numpy(eid).cuda()
    for name, ex in lists.items():
        d_ex = torch.from_numpy(ex).cuda()
        out_n, p_n = _padded(torch, n_dst * fanout, torch.int32, S32)
        out_e, p_e = _padded(torch, n_dst * fanout, torch.int64, S64)
        _capi.check(L.coala_block_exclude_edges(0, d_nbr.data_ptr(), d_eid.data_ptr(), d_ex.data_ptr() if len(ex) else None, len(ex), p_n, p_e,
                                                n_dst, fanout, current_stream()))
        got_n = _inside(out_n, n_dst * fanout, S32).reshape(n_dst, fanout)
        got_e = _inside(out_e, n_dst * fanout, S64).reshape(n_dst, fanout)
        keep = (nbr >= 0) & ~np.isin(eid, ex)
        order = np.argsort(~keep, axis=1, kind="stable")            # survivors first, in their old order
        want_n = np.take_along_axis(np.where(keep, nbr, -1), order, axis=1)
        want_e = np.take_along_axis(np.where(keep, eid, -1), order, axis=1)
        ends = np.r_[0:1500, n_dst - 1500: n_dst]                    # ... which is exclude_fixed, row by row
        ref_n, ref_e = R.exclude_fixed(nbr[ends], eid[ends], ex)
        assert np.array_equal(want_n[ends], ref_n) and np.array_equal(want_e[ends], ref_e)
        assert got_n.dtype == want_n.dtype and np.array_equal(got_n, want_n), name
        assert np.array_equal(got_e, want_e), name
        if name == "2048":
            assert np.all(got_n[emptied] == -1) and np.all(got_e[emptied] == -1) and (nbr[emptied] >= 0).any(axis=1).all()
        if name == "one":
            assert (got_n[-1] >= 0).sum() == (nbr[-1] >= 0).sum() - 1
        if name == "empty":
            assert (got_n >= 0).sum() == (nbr >= 0).sum()


def test_csr_kernel_past_one_grid_pass(hiplib):
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    n_dst, wide = 40_003, 33_000
    assert n_dst * 64 > 8192 * 256 and wide > 32_768
    rng = np.random.default_rng(40)
    deg = rng.integers(0, 131, size=n_dst)
    deg[[0, 1, 2]], deg[wide], deg[-1] = [0, 130, 64], 3000, 65       # the degrees 0 .. 130 and one row of a few thousand, in the second pass
    indptr = np.zeros(n_dst + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    E = int(indptr[-1])
    indices = rng.integers(0, 1 << 20, size=E).astype(np.int32)
    eid = rng.permutation(2 * E)[:E].astype(np.int64)
    rows = np.repeat(np.arange(n_dst), deg)
    emptied = [1, 32_768, n_dst - 1]
    lists = _exclusion_lists(rng, [eid[indptr[r]: indptr[r + 1]] for r in emptied] + [eid[indptr[wide]: indptr[wide] + 700]], eid, one=eid[-1])
    d_ip, d_ix, d_eid = torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda(), torch.from_numpy(eid).cuda()
    for name, ex in lists.items():
        d_ex = torch.from_numpy(ex).cuda()
        ex_ptr = d_ex.data_ptr() if len(ex) else None
        counts, p_c = _padded(torch, n_dst, torch.int64, S64)
        _capi.check(L.coala_block_exclude_edges_csr(0, d_ip.data_ptr(), d_ix.data_ptr(), d_eid.data_ptr(), ex_ptr, len(ex), p_c, None, None, None,
                                                    n_dst, current_stream()))
        got_c = _inside(counts, n_dst, S64)
        keep = ~np.isin(eid, ex)
        assert np.array_equal(got_c, np.bincount(rows[keep], minlength=n_dst)), name
        new_ip = np.zeros(n_dst + 1, dtype=np.int64)                  # the host scan between the two passes
        np.cumsum(got_c, out=new_ip[1:])
        left = int(new_ip[-1])
        d_new = torch.from_numpy(new_ip).cuda()
        out_x, p_x = _padded(torch, left, torch.int32, S32)
        out_e, p_e = _padded(torch, left, torch.int64, S64)
        _capi.check(L.coala_block_exclude_edges_csr(0, d_ip.data_ptr(), d_ix.data_ptr(), d_eid.data_ptr(), ex_ptr, len(ex), None, d_new.data_ptr(),
                                                    p_x, p_e, n_dst, current_stream()))
        want_ip, want_x, want_e = R.exclude_csr(indptr, indices, eid, ex)
        assert np.array_equal(new_ip, want_ip) and left == int(keep.sum())
        got_x, got_e = _inside(out_x, left, S32), _inside(out_e, left, S64)
        assert got_x.dtype == want_x.dtype and np.array_equal(got_x, want_x) and np.array_equal(got_e, want_e), name
        if name == "2048":
            assert np.all(got_c[emptied] == 0) and got_c[wide] == 2300
        if name == "one":
            assert left == E - 1 and got_c[-1] == 64
        if name == "empty":
            assert left == E
