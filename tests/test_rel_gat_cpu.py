"""CPU tests of relation-typed attention's surface: Block.rel_gat_aggregate_torch (the fallback and reference of the native kernels)
against GAT's own reference applied relation by relation, the dense and the packed form against each other, RelGATConv and RelSAGEConv
against sums of per-relation GATConv / SAGEConv modules, the argument checks, and one training step of harness.RGAT and harness.RSAGE.

The rule (include/coala_hip.h, coala_block_rel_gat_aggregate): the softmax of GAT runs over the edges of one (destination, relation)
at a time and the relations' results are summed, so the result is the sum over r of gat_aggregate on a copy of the block that keeps
only the edges of type r: the other slots set to -1 in the fixed form, the CSR row filtered in the ragged form.  A slot whose type is
outside [0, R) is in no copy."""
import types

import numpy as np
import pytest

R, H, D = 5, 2, 3   # relation 3 is used by no edge

# a fixed block: padding in front of, between and behind valid slots; row 2 is empty; types out of range (-1, R, 1000); repeated sources
FIXED_NBR = np.array([[0, 1, 2, 3], [-1, 4, -1, 4], [-1, -1, -1, -1], [5, 5, 5, -1], [6, 0, 1, 2], [3, -1, -1, -1]], dtype=np.int32)
FIXED_TYPE = np.array([[0, 1, 0, 2], [77, 4, -5, 4], [0, 1, 2, 4], [-1, R, 1000, 0], [2, 2, 2, 2], [1, 9, 9, 9]], dtype=np.int64)
# a ragged block: rows of 0, 1 and 7 edges, a -1 entry inside a row, interleaved types
RAGGED_ROWS = [[], [2], [0, 1, 2, 3, 4, 5, 6], [], [6, -1, 6], [1, 0]]
RAGGED_TYPE = [[], [4], [0, 1, 0, -1, R, 1000, 1], [], [1, 0, 1], [2, 2]]
N_SRC = 7


def _fixed(torch, nbr):
    from COALA_GNN.sampler import Block
    return Block(torch.arange(N_SRC), torch.from_numpy(np.ascontiguousarray(nbr)), len(nbr))


def _ragged(torch, rows):
    from COALA_GNN.sampler import Block
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    idx = np.array([s for r in rows for s in r], dtype=np.int32)
    return Block(torch.arange(N_SRC), None, len(rows), indptr=torch.from_numpy(indptr), indices=torch.from_numpy(idx))


def _cases(torch):
    """-> [(name, block, etype tensor, [the block restricted to relation r, r < R])]"""
    fixed = _fixed(torch, FIXED_NBR)
    fixed_r = [_fixed(torch, np.where(FIXED_TYPE == r, FIXED_NBR, -1).astype(np.int32)) for r in range(R)]
    ragged = _ragged(torch, RAGGED_ROWS)
    ragged_r = [_ragged(torch, [[s for s, t in zip(row, ts) if t == r] for row, ts in zip(RAGGED_ROWS, RAGGED_TYPE)]) for r in range(R)]
    rt = torch.tensor([t for ts in RAGGED_TYPE for t in ts], dtype=torch.int64)
    return [("fixed", fixed, torch.from_numpy(FIXED_TYPE), fixed_r), ("ragged", ragged, rt, ragged_r)]


def _inputs(torch, n_dst, seed=0):
    g = torch.Generator().manual_seed(seed)
    el = torch.randn(N_SRC, R, H, generator=g, dtype=torch.float64).requires_grad_(True)
    er = torch.randn(n_dst, R, H, generator=g, dtype=torch.float64).requires_grad_(True)
    feat = torch.randn(N_SRC, R, H, D, generator=g, dtype=torch.float64).requires_grad_(True)
    cot = torch.randn(n_dst, H, D, generator=g, dtype=torch.float64)
    return el, er, feat, cot


def _grads(torch, out, cot, leaves):
    return torch.autograd.grad((out * cot).sum(), leaves)


def _close(torch, got, want, tol=1e-12):
    assert got.shape == want.shape and got.numel()
    assert float((got.detach() - want.detach()).abs().max()) <= tol


def test_fallback_equals_gat_per_relation():
    import torch
    for name, b, etype, by_rel in _cases(torch):
        el, er, feat, cot = _inputs(torch, b.num_dst)
        for dt in (torch.int64, torch.int32):
            got = b.rel_gat_aggregate_torch(el, er, feat, etype.to(dt), R, negative_slope=0.3)
            assert got.shape == (b.num_dst, H, D) and got.dtype == torch.float64
            want = sum(br.gat_aggregate_torch(el[:, r], er[:, r], feat[:, r], 0.3) for r, br in enumerate(by_rel))
            _close(torch, got, want)
            g_el, g_er, g_feat = _grads(torch, got, cot, (el, er, feat))
            for g, w in zip((g_el, g_er, g_feat), _grads(torch, want, cot, (el, er, feat))):
                _close(torch, g, w)
        assert torch.equal(b.rel_gat_aggregate(el, er, feat, etype, R, negative_slope=0.3), got), "a CPU tensor goes through the fallback"
        empty = [d for d in range(b.num_dst) if not any(br.in_degrees()[d] for br in by_rel)]
        assert empty and bool((got[empty] == 0).all()), "a row without a valid edge is exactly zero"
        assert int(by_rel[3].in_degrees().sum()) == 0, "relation 3 is absent from the whole block"
        # the relation absent everywhere receives no gradient
        assert bool((g_el[:, 3] == 0).all()) and bool((g_er[:, 3] == 0).all()) and bool((g_feat[:, 3] == 0).all())


def test_dense_and_packed_forms_agree():
    import torch
    for name, b, etype, _ in _cases(torch):
        el, er, feat, cot = _inputs(torch, b.num_dst, seed=1)
        _, src = b._slots()
        t = etype.reshape(-1)
        rows = torch.where((src >= 0) & (t >= 0) & (t < R), src * R + t, -1).view(etype.shape)
        dense = b.rel_gat_aggregate_torch(el, er, feat, etype, R)
        packed = b.rel_gat_aggregate_torch(el.reshape(-1, H), er, feat.reshape(-1, H, D), etype, R, rows=rows)
        assert torch.equal(dense, packed), name
        for g, w in zip(_grads(torch, dense, cot, (el, er, feat)), _grads(torch, packed, cot, (el, er, feat))):
            _close(torch, g, w, 0.0)
        # the packed form reads any row the caller names: a permuted table with the permuted rows gives the same result
        perm = torch.randperm(N_SRC * R, generator=torch.Generator().manual_seed(2))
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(perm.numel())
        rows_p = torch.where(rows >= 0, inv[rows.clamp_min(0)], -1)
        again = b.rel_gat_aggregate(el.reshape(-1, H)[perm], er, feat.reshape(-1, H, D)[perm], etype.to(torch.int32), R, rows=rows_p.to(torch.int32))
        _close(torch, again, dense)


def _typed_convs(torch, make, seed):
    torch.manual_seed(seed)
    convs = [make().double() for _ in range(R)]
    with torch.no_grad():
        for c in convs:
            c.bias.normal_()
    return convs


def test_relgatconv_equals_the_sum_of_gatconvs():
    import torch
    from COALA_GNN.nn import GATConv, RelGATConv
    in_feats = 4

    def make():
        c = GATConv(in_feats, D, H, negative_slope=0.25)
        with torch.no_grad():
            c.fc_dst.weight.copy_(c.fc_src.weight)
        return c

    for name, b, etype, by_rel in _cases(torch):
        convs = _typed_convs(torch, make, 3)
        layer = RelGATConv.from_gatconvs(convs)
        assert [tuple(p.shape) for p in (layer.fc_weight, layer.attn_l, layer.attn_r, layer.bias)] == \
            [(R, H * D, in_feats), (R, H, D), (R, H, D), (R, H * D)]
        h = torch.randn(N_SRC, in_feats, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).requires_grad_(True)
        cot = torch.randn(b.num_dst, H, D, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
        got = layer(b, (h, b.dst_rows(h)), etype)
        want = sum(c(br, (h, br.dst_rows(h))) for c, br in zip(convs, by_rel))
        assert got.shape == (b.num_dst, H, D)
        _close(torch, got, want)
        params = [p for c in convs for p in (c.fc_src.weight, c.fc_dst.weight, c.attn_l, c.attn_r, c.bias)]
        g_got = _grads(torch, got, cot, (h, layer.fc_weight, layer.attn_l, layer.attn_r, layer.bias))
        g_want = _grads(torch, want, cot, [h] + params)
        _close(torch, g_got[0], g_want[0])
        for r in range(R):
            gs, gd, gl, gr, gb = g_want[1 + 5 * r: 6 + 5 * r]
            _close(torch, g_got[1][r], gs + gd)
            _close(torch, g_got[2][r], gl[0])
            _close(torch, g_got[3][r], gr[0])
            _close(torch, g_got[4][r], gb)
    convs[0].fc_dst.weight.data.add_(1.0)
    with pytest.raises(ValueError, match="same weights"):
        RelGATConv.from_gatconvs(convs)
    fresh = RelGATConv(in_feats, D, H, R)
    assert bool((fresh.bias == 0).all()) and all(float(fresh.attn_l[r].detach().abs().sum()) > 0 for r in range(R))
    assert set(dict(fresh.named_parameters())) == {"fc_weight", "attn_l", "attn_r", "bias"}


def test_relsageconv_equals_the_sum_of_sageconvs():
    import torch
    from COALA_GNN.nn import RelSAGEConv, SAGEConv
    for in_feats, out_feats in ((4, 6), (6, 4)):   # SAGEConv projects before the aggregation when in > out: the same mathematics
        for name, b, etype, by_rel in _cases(torch):
            convs = _typed_convs(torch, lambda: SAGEConv(in_feats, out_feats, "gcn"), 6)
            layer = RelSAGEConv(in_feats, out_feats, R).double()
            assert tuple(layer.fc_neigh_weight.shape) == (R, out_feats, in_feats) and tuple(layer.bias.shape) == (R, out_feats)
            with torch.no_grad():
                for r, c in enumerate(convs):
                    layer.fc_neigh_weight[r] = c.fc_neigh.weight
                    layer.bias[r] = c.bias
            h = torch.randn(N_SRC, in_feats, dtype=torch.float64, generator=torch.Generator().manual_seed(7)).requires_grad_(True)
            cot = torch.randn(b.num_dst, out_feats, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
            got = layer(b, (h, b.dst_rows(h)), etype)
            want = sum(c(br, (h, br.dst_rows(h))) for c, br in zip(convs, by_rel))
            _close(torch, got, want)
            _close(torch, layer(b, h, etype), want)
            g_got = _grads(torch, got, cot, (h, layer.fc_neigh_weight, layer.bias))
            g_want = _grads(torch, want, cot, [h] + [p for c in convs for p in (c.fc_neigh.weight, c.bias)])
            _close(torch, g_got[0], g_want[0])
            for r in range(R):
                _close(torch, g_got[1][r], g_want[1 + 2 * r])
                _close(torch, g_got[2][r], g_want[2 + 2 * r])


def test_argument_errors():
    import torch
    from COALA_GNN.nn import RelGATConv, RelSAGEConv
    for name, b, etype, _ in _cases(torch):
        el, er, feat, _ = _inputs(torch, b.num_dst)
        rows = torch.zeros(etype.shape, dtype=torch.int64)
        for fn in (b.rel_gat_aggregate, b.rel_gat_aggregate_torch):
            with pytest.raises(ValueError, match="integer tensor"):
                fn(el, er, feat, etype.double(), R)
            with pytest.raises(ValueError, match="one per neighbour slot"):
                fn(el, er, feat, etype.reshape(-1)[:-1], R)
            for bad in (0, 65, True, 2.0):
                with pytest.raises(ValueError, match="1..64 relations"):
                    fn(el, er, feat, etype, bad)
            with pytest.raises(ValueError, match="this block takes"):
                fn(el[:, :-1], er, feat, etype, R)                                   # el does not match feat
            with pytest.raises(ValueError, match="this block takes"):
                fn(el, er[:-1], feat, etype, R)                                      # er is not [num_dst, R, H]
            with pytest.raises(ValueError, match="this block takes"):
                fn(el, er, feat[:-1], etype, R)                                      # the dense form needs num_src rows
            with pytest.raises(ValueError, match="this block takes"):
                fn(el, er, feat, etype, R, rows=rows)                                # the packed form takes [P, H] and [P, H, D]
            with pytest.raises(ValueError, match="this block takes"):
                fn(el.reshape(-1, H), er, feat.reshape(-1, H, D), etype, R)          # ... and the dense form does not
            with pytest.raises(ValueError, match="rows must be an integer tensor"):
                fn(el.reshape(-1, H), er, feat.reshape(-1, H, D), etype, R, rows=rows.double())
            with pytest.raises(ValueError, match="rows of shape"):
                fn(el.reshape(-1, H), er, feat.reshape(-1, H, D), etype, R, rows=rows.reshape(-1)[:-1])
    for bad in (0, 65, True, 2.0):
        with pytest.raises(ValueError, match="1..64 relations"):
            RelGATConv(4, D, H, bad)
        with pytest.raises(ValueError, match="1..64 relations"):
            RelSAGEConv(4, 4, bad)


def _typed_blocks(torch):
    """Two hand-made layers with edge ids into a small graph's edata: an input block (ragged) and an output block (fixed)."""
    from COALA_GNN.sampler import Block
    graph = types.SimpleNamespace(edata={"etype": torch.arange(40) % 3}, ndata={})
    b0 = _ragged(torch, RAGGED_ROWS)
    b0 = Block(b0.src_nodes, None, b0.num_dst, indptr=b0.indptr, indices=b0.indices, eid=torch.arange(b0.indices.numel()) * 2,
               edata_graph=graph)
    nbr = torch.tensor([[0, 5, -1], [2, 2, 1], [-1, -1, -1]], dtype=torch.int32)
    eid = torch.where(nbr >= 0, torch.arange(9).view(3, 3) + 20, -1)
    b1 = Block(torch.arange(6), nbr, 3, eid=eid, edata_graph=graph)
    return [b0, b1]


@pytest.mark.parametrize("model_name", ["RGAT", "RSAGE"])
def test_models_train_one_step_on_cpu(model_name):
    import torch
    from COALA_GNN import harness
    torch.manual_seed(0)
    blocks = _typed_blocks(torch)
    kw = {"n_heads": 2} if model_name == "RGAT" else {}
    model = getattr(harness, model_name)(5, 8, 4, 2, 3, **kw)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    x = torch.randn(N_SRC, 5)
    labels = torch.tensor([0, 3, 1])
    model.train()
    out = model(blocks, x)
    assert out.shape == (3, 4)
    loss = torch.nn.functional.cross_entropy(out, labels)
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert any(float(p.grad.abs().sum()) > 0 for p in model.layers[0].parameters())
    before = [p.detach().clone() for p in model.parameters()]
    opt.step()
    assert any(not torch.equal(a, p) for a, p in zip(before, model.parameters()))
    from COALA_GNN.sampler import Block
    bare = [Block(b.src_nodes, b.nbr, b.num_dst, indptr=b.indptr, indices=b.indices) for b in blocks]
    with pytest.raises(ValueError, match=f"{model_name} needs the edge ids of its blocks"):
        model(bare, x)
    if model_name == "RGAT":
        with pytest.raises(ValueError, match="multiple of n_heads"):
            harness.RGAT(5, 9, 4, 2, 3, n_heads=2)
