"""CPU tests of the relation-typed sum's surface: Block.rel_sum_aggregate_torch (the fallback and reference of the native kernels) and
Block.rel_in_degrees against plain numpy loops that restate the rule; RelGraphConv's parameter names, shapes and formula; the
argument checks.

The rule (include/coala_hip.h, coala_block_rel_sum): out[d, r, :] = the sum, in slot order, of w_j x[s_j, :] over the valid slots j of
row d whose type is r.  A padding slot's type and weight are never used; a valid slot whose type is outside [0, R) adds nothing; a
relation absent from a row, and a row without a valid slot, give zeros."""
import numpy as np
import pytest


def ref_rel_sum(rows, types, w, x, R):
    """The rule as a loop.  rows[d]: the source of every slot of row d in slot order (-1: padding); types[d], w[d]: the slots' types
    and weights (w None: 1).  -> [n_dst, R, dim] in x's dtype."""
    out = np.zeros((len(rows), R, x.shape[1]), dtype=x.dtype)
    for d, srcs in enumerate(rows):
        for k, s in enumerate(srcs):
            t = int(types[d][k])
            if s < 0 or not 0 <= t < R:
                continue
            out[d, t] += x[s] * (x.dtype.type(1) if w is None else x.dtype.type(w[d][k]))
    return out


def ref_rel_degrees(rows, types, R):
    cnt = np.zeros((len(rows), R), dtype=np.int64)
    for d, srcs in enumerate(rows):
        for k, s in enumerate(srcs):
            if s >= 0 and 0 <= int(types[d][k]) < R:
                cnt[d, int(types[d][k])] += 1
    return cnt


R = 5   # relation 3 is used by no edge

# a fixed block: padding in front of, between and behind valid slots; row 2 is empty; types out of range (-1, R, 1000); a padding slot
# with a wild type and a NaN weight
FIXED_NBR = np.array([[0, 1, 2, 3], [-1, 4, -1, 4], [-1, -1, -1, -1], [5, 5, 5, -1], [6, 0, 1, 2], [3, -1, -1, -1]], dtype=np.int32)
FIXED_TYPE = np.array([[0, 1, 0, 2], [77, 4, -5, 4], [0, 1, 2, 4], [-1, R, 1000, 0], [2, 2, 2, 2], [1, 9, 9, 9]], dtype=np.int64)
# a ragged block: rows of 0, 1 and 7 edges, a -1 entry inside a row
RAGGED_ROWS = [[], [2], [0, 1, 2, 3, 4, 5, 6], [], [6, -1, 6], [1, 0]]
RAGGED_TYPE = [[], [4], [0, 1, 0, -1, R, 1000, 2], [], [1, 0, 1], [2, 2]]


def _blocks(torch):
    from COALA_GNN.sampler import Block
    rng = np.random.default_rng(0)
    n_src = 7
    fw = rng.integers(-3, 4, size=FIXED_NBR.shape).astype(np.float64)
    fw[1, 0] = np.nan                                             # a padding slot's weight is never used
    fixed = Block(torch.arange(n_src), torch.from_numpy(FIXED_NBR), len(FIXED_NBR))
    indptr = np.zeros(len(RAGGED_ROWS) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in RAGGED_ROWS], out=indptr[1:])
    idx = np.array([s for r in RAGGED_ROWS for s in r], dtype=np.int32)
    rt = np.array([t for r in RAGGED_TYPE for t in r], dtype=np.int64)
    rw = rng.integers(-3, 4, size=len(idx)).astype(np.float64)
    rw[np.flatnonzero(idx < 0)] = np.nan
    ragged = Block(torch.arange(n_src), None, len(RAGGED_ROWS), indptr=torch.from_numpy(indptr), indices=torch.from_numpy(idx))
    x = rng.integers(-4, 5, size=(n_src, 3)).astype(np.float64)
    w_rows = [list(rw[indptr[d]: indptr[d + 1]]) for d in range(len(RAGGED_ROWS))]
    return [("fixed", fixed, FIXED_NBR.tolist(), FIXED_TYPE.tolist(), fw.tolist(), FIXED_TYPE, fw),
            ("ragged", ragged, RAGGED_ROWS, RAGGED_TYPE, w_rows, rt, rw)], x


@pytest.mark.parametrize("weights", [True, False])
def test_fallback_equals_the_numpy_loop(weights):
    """float64 on small integers: every sum is exact, so the comparison is for equality."""
    import torch
    cases, x = _blocks(torch)
    for name, b, rows, types, w_rows, t_arr, w_arr in cases:
        want = ref_rel_sum(rows, types, w_rows if weights else None, x, R)
        for dt in (torch.int64, torch.int32, torch.int16):
            got = b.rel_sum_aggregate_torch(torch.from_numpy(x), torch.from_numpy(t_arr).to(dt), R, torch.from_numpy(w_arr) if weights else None)
            assert got.shape == (b.num_dst, R, 3) and got.dtype == torch.float64
            assert np.array_equal(got.numpy(), want), f"{name} {dt}"
        # a CPU tensor goes through the fallback
        got = b.rel_sum_aggregate(torch.from_numpy(x), torch.from_numpy(t_arr), R, torch.from_numpy(w_arr) if weights else None)
        assert np.array_equal(got.numpy(), want), name
        assert np.all(want[:, 3] == 0) and np.any(want[:, 0] != 0), "relation 3 is absent everywhere, relation 0 is not"
        assert not np.isnan(want).any()


def test_rel_in_degrees_against_a_loop():
    import torch
    cases, _ = _blocks(torch)
    for name, b, rows, types, _, t_arr, _ in cases:
        got = b.rel_in_degrees(torch.from_numpy(t_arr), R)
        assert got.dtype == torch.int64 and tuple(got.shape) == (b.num_dst, R)
        assert np.array_equal(got.numpy(), ref_rel_degrees(rows, types, R)), name


def test_gradcheck_of_the_fallback():
    import torch
    cases, x = _blocks(torch)
    rng = np.random.default_rng(1)
    for name, b, _, _, _, t_arr, w_arr in cases:
        h = torch.from_numpy(x + rng.standard_normal(x.shape)).requires_grad_(True)
        w = torch.from_numpy(np.nan_to_num(w_arr) + 0.5).requires_grad_(True)
        t = torch.from_numpy(t_arr)
        assert torch.autograd.gradcheck(lambda h_, w_: b.rel_sum_aggregate_torch(h_, t, R, w_), (h, w)), name
        assert torch.autograd.gradcheck(lambda h_: b.rel_sum_aggregate_torch(h_, t, R), (h,)), name


def test_argument_errors():
    import torch
    from COALA_GNN.nn import RelGraphConv
    cases, x = _blocks(torch)
    h = torch.from_numpy(x)
    for name, b, _, _, _, t_arr, w_arr in cases:
        t = torch.from_numpy(t_arr)
        for bad in (0, 65, -1):
            with pytest.raises(ValueError, match="1..64"):
                b.rel_sum_aggregate(h, t, bad)
            with pytest.raises(ValueError, match="1..64"):
                b.rel_sum_aggregate_torch(h, t, bad)
            with pytest.raises(ValueError, match="1..64"):
                b.rel_in_degrees(t, bad)
        with pytest.raises(ValueError, match="one per neighbour slot"):
            b.rel_sum_aggregate(h, t.reshape(-1)[:-1], R)
        with pytest.raises(ValueError, match="one per neighbour slot"):
            b.rel_sum_aggregate_torch(h, t, R, torch.from_numpy(w_arr).reshape(-1)[:-1])
        with pytest.raises(ValueError, match="integer"):
            b.rel_sum_aggregate(h, t.double(), R)
        b.rel_sum_aggregate(h, t, 64)
    with pytest.raises(ValueError, match="not provided"):
        RelGraphConv(4, 3, 2, regularizer="bdd")
    for bad in (0, 65):
        with pytest.raises(ValueError, match="1..64"):
            RelGraphConv(4, 3, bad)
    with pytest.raises(ValueError):
        RelGraphConv(4, 3, 2, regularizer="other")


def test_relgraphconv_parameter_names_and_shapes():
    import torch
    from COALA_GNN.nn import RelGraphConv
    sd = RelGraphConv(6, 4, 3, layer_norm=True).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"linear_r.W": (3, 6, 4), "h_bias": (4,), "loop_weight": (6, 4),
                                                          "layer_norm_weight.weight": (4,), "layer_norm_weight.bias": (4,)}
    sd = RelGraphConv(6, 4, 3, regularizer="basis", num_bases=2).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"linear_r.W": (2, 6, 4), "linear_r.coeff": (3, 2), "h_bias": (4,),
                                                          "loop_weight": (6, 4)}
    sd = RelGraphConv(6, 4, 3, regularizer="basis", bias=False, self_loop=False).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"linear_r.W": (3, 6, 4), "linear_r.coeff": (3, 3)}
    assert torch.all(RelGraphConv(6, 4, 3).h_bias == 0)


def test_relgraphconv_formula():
    """Against sum_j norm_j x[s_j] @ W[t_j] written edge by edge in numpy, with every later stage of the layer; 'basis' with coeff = I
    equals None with the same W; num_rels = 1 without norm and self-loop is the weighted sum with unit weights, times W[0], + h_bias."""
    import torch
    from COALA_GNN.nn import RelGraphConv
    cases, x = _blocks(torch)
    torch.manual_seed(0)
    for name, b, rows, types, _, t_arr, _ in cases:
        h = torch.from_numpy(x)
        t = torch.from_numpy(t_arr)
        plain = RelGraphConv(3, 4, R, activation=torch.tanh, layer_norm=True).double()
        with torch.no_grad():
            plain.h_bias.uniform_(-1, 1)
            plain.layer_norm_weight.weight.uniform_(0.5, 2)
        norm = torch.rand(t.shape, dtype=torch.float64) + 0.5
        W = plain.linear_r.W.detach().numpy()
        agg = np.zeros((b.num_dst, 4))
        for d, srcs in enumerate(rows):
            for k, s in enumerate(srcs):
                tt = int(types[d][k])
                if s >= 0 and 0 <= tt < R:
                    agg[d] += float(norm.reshape(-1)[sum(len(r) for r in rows[:d]) + k]) * (x[s] @ W[tt])
        a = torch.from_numpy(agg)
        want = torch.nn.functional.layer_norm(a, (4,), plain.layer_norm_weight.weight, plain.layer_norm_weight.bias) + plain.h_bias
        want = torch.tanh(want + h[: b.num_dst] @ plain.loop_weight)
        got = plain(b, h, t, norm)
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), name
        assert torch.equal(plain(b, (h, h[: b.num_dst]), t, norm.unsqueeze(-1) if norm.dim() == 1 else norm), got), name
        # 'basis' with coeff = I
        basis = RelGraphConv(3, 4, R, regularizer="basis", activation=torch.tanh, layer_norm=True).double()
        sd = dict(plain.state_dict())
        sd["linear_r.coeff"] = torch.eye(R, dtype=torch.float64)
        basis.load_state_dict(sd)
        assert torch.allclose(basis(b, h, t, norm), got, rtol=1e-13, atol=1e-13), name
        # one relation
        one = RelGraphConv(3, 4, 1, self_loop=False).double()
        with torch.no_grad():
            one.h_bias.uniform_(-1, 1)
        slots = b.indices if b.nbr is None else b.nbr
        ws = b.weighted_sum_aggregate_torch(h, torch.ones(slots.shape, dtype=torch.float64))
        assert torch.equal(one(b, h, torch.zeros_like(t)), ws @ one.linear_r.W[0] + one.h_bias), name


def test_rgcn_model_and_synthetic_edge_types():
    import torch
    from COALA_GNN.harness import RGCN
    from COALA_GNN.sampler import Block
    from COALA_GNN.synthetic import edge_types_by_source
    idx = torch.tensor([0, 5, 9, 12, 3, 7], dtype=torch.int64)
    t = edge_types_by_source(idx, 4)
    assert t.dtype == torch.int64 and t.tolist() == [0, 1, 1, 0, 3, 3]
    model = RGCN(3, 8, 2, 1, 4).double()
    assert sorted(model.state_dict()) == ["layers.0.h_bias", "layers.0.linear_r.W", "layers.0.loop_weight"]
    b = Block(torch.arange(7), torch.from_numpy(FIXED_NBR), len(FIXED_NBR))
    with pytest.raises(ValueError, match="edge_ids=True"):
        model([b], torch.zeros(7, 3, dtype=torch.float64))
    # a block with edge ids: every message is divided by the number of the row's edges of its relation
    eid = torch.arange(FIXED_NBR.size).view(FIXED_NBR.shape)
    eid[torch.from_numpy(FIXED_NBR) < 0] = -1

    class G:
        ndata = {}
        edata = {"etype": torch.from_numpy(np.clip(FIXED_TYPE, 0, 3)).reshape(-1)}
    b = Block(torch.arange(7), torch.from_numpy(FIXED_NBR), len(FIXED_NBR), eid=eid, edata_graph=G())
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((7, 3)))
    model.eval()
    got = model([b], x)
    et = b.edata["etype"]
    cnt = ref_rel_degrees(FIXED_NBR.tolist(), et.tolist(), 4)
    L = model.layers[0]
    want = x[: b.num_dst] @ L.loop_weight + L.h_bias
    for d in range(b.num_dst):
        for k in range(FIXED_NBR.shape[1]):
            if FIXED_NBR[d, k] >= 0:
                r = int(et[d, k])
                want[d] = want[d] + x[FIXED_NBR[d, k]] @ L.linear_r.W[r] / cnt[d, r]
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
