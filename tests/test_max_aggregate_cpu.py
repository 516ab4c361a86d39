"""CPU tests of the max aggregation surface: Block.max_aggregate_torch (the fallback and reference of the native kernels) against a
plain numpy loop that restates the rule, bit for bit in value and argmax; where its gradient goes on ties; SAGEConv('pool') and
GINConv against hand-written float64 layers, with DGL's parameter names and shapes; the new C entry points.

The rule (include/coala_hip.h, coala_block_max_aggregate): over the valid slots of a row in slot order the running maximum starts from
the first one, and a later slot replaces it when its value is greater, or is NaN while the maximum is not.  Ties, +-0 included, keep
the first slot; a NaN propagates with the argmax at the first NaN; a row without a valid slot gives 0 and argmax -1."""
import numpy as np
import pytest


def ref_max(rows_of, x, w_of=None):
    """The rule as a loop.  rows_of[d]: the source of every valid slot of row d, in slot order; w_of[d] (optional): their weights.
    -> (out [n_dst, dim] in x's dtype, arg int32 [n_dst, dim])"""
    n_dst, dim = len(rows_of), x.shape[1]
    out = np.zeros((n_dst, dim), dtype=x.dtype)
    arg = np.full((n_dst, dim), -1, dtype=np.int32)
    for d, srcs in enumerate(rows_of):
        for k, s in enumerate(srcs):
            v = x[s] if w_of is None else x[s] * x.dtype.type(w_of[d][k])
            if k == 0:
                out[d], arg[d] = v, s
                continue
            with np.errstate(invalid="ignore"):
                take = (v > out[d]) | (np.isnan(v) & ~np.isnan(out[d]))
            out[d][take] = v[take]
            arg[d][take] = s
    return out, arg


def tie_fraction(rows_of, x):
    """Fraction of the (row, column) pairs whose maximum is reached by more than one slot."""
    ties = 0
    for srcs in rows_of:
        if len(srcs) > 1:
            v = x[np.asarray(srcs)]
            top = np.where(np.isnan(v), -np.inf, v).max(0)
            ties += int(((v == top).sum(0) > 1).sum())
    return ties / (len(rows_of) * x.shape[1])


def make_values(rng, kind, n_src, dim, dtype=np.float32):
    """'normal': distinct values; 'ties': the integers -2..2; 'special': those with +-0, +-inf and NaN entries among them."""
    if kind == "normal":
        return rng.standard_normal((n_src, dim)).astype(dtype)
    x = rng.integers(-2, 3, size=(n_src, dim)).astype(dtype)
    if kind == "special":
        r = rng.random((n_src, dim))
        x[r < 0.10] = -0.0
        x[(r >= 0.10) & (r < 0.16)] = np.inf
        x[(r >= 0.16) & (r < 0.30)] = -np.inf
        x[(r >= 0.30) & (r < 0.33)] = np.nan
        x[n_src - 1] = -np.inf                     # whole rows of one special value
        x[n_src - 2] = np.nan
        x[n_src - 3] = -0.0
        x[n_src - 4] = 0.0
    return x


def fixed_case(rng, n_dst=60, f=16, n_src=50):
    nbr = rng.integers(0, n_src, size=(n_dst, f)).astype(np.int32)
    nbr[rng.random((n_dst, f)) < 0.25] = -1                # -1 anywhere in a row
    nbr[3] = -1                                            # a row without a valid edge
    nbr[4, :] = 2                                          # one source repeated over a whole row
    nbr[5, 1] = nbr[5, 0] = 7                              # a source twice
    nbr[6, :] = -1
    nbr[6, f - 1] = n_src - 1                              # one valid slot, the last: a row of -inf in the 'special' values
    nbr[7, 0], nbr[7, 1:] = -1, n_src - 1                  # only -inf, after a padding slot
    nbr[8, : min(f, 4)] = [n_src - 3, n_src - 4, n_src - 3, n_src - 4][: min(f, 4)]   # -0, +0, -0, +0 first
    nbr[9, : min(f, 4)] = [n_src - 4, n_src - 3, n_src - 2, n_src - 2][: min(f, 4)]   # +0, -0, NaN, NaN
    return nbr, [[int(s) for s in r if s >= 0] for r in nbr]


def ragged_case(rng, n_dst=40, n_src=50, long_row=150):
    deg = rng.integers(0, 30, size=n_dst)
    deg[[0, 7]] = 0                                        # rows without an edge
    deg[9] = long_row                                      # longer than one 64-edge chunk
    deg[3] = 6
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rng.integers(0, n_src, size=int(indptr[-1])).astype(np.int32)
    indices[indptr[3]: indptr[4]] = 5                      # repeated sources
    indices[indptr[9] + 70] = n_src - 2                    # the NaN row of the 'special' values, in the long row's second chunk
    return indptr, indices, [[int(s) for s in indices[indptr[d]: indptr[d + 1]]] for d in range(n_dst)]


def fixed_block(torch, nbr, n_src, device="cpu"):
    from COALA_GNN.sampler import Block
    return Block(torch.arange(n_src, device=device), torch.from_numpy(nbr).to(device), nbr.shape[0])


def ragged_block(torch, indptr, indices, n_src, device="cpu"):
    from COALA_GNN.sampler import Block
    return Block(torch.arange(n_src, device=device), None, len(indptr) - 1, indptr=torch.from_numpy(indptr).to(device),
                 indices=torch.from_numpy(indices).to(device))


def _case(torch, rng, form, n_src=50):
    if form == "fixed":
        nbr, rows_of = fixed_case(rng, n_src=n_src)
        return fixed_block(torch, nbr, n_src), rows_of, nbr.shape
    indptr, indices, rows_of = ragged_case(rng, n_src=n_src)
    return ragged_block(torch, indptr, indices, n_src), rows_of, indices.shape


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["normal", "ties", "special"])
@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_max_aggregate_torch_follows_the_rule_bit_for_bit(hiplib, form, kind, dtype):
    import torch
    rng = np.random.default_rng(1)
    b, rows_of, _ = _case(torch, rng, form)
    x = make_values(rng, kind, 50, 9, dtype)
    want, want_arg = ref_max(rows_of, x)
    got, arg = b.max_aggregate_torch(torch.from_numpy(x), return_arg=True)
    assert same_bits(got.numpy(), want), "values differ from the rule"
    assert arg.dtype == torch.int32 and np.array_equal(arg.numpy(), want_arg), "argmax differs from the rule"
    assert same_bits(b.max_aggregate_torch(torch.from_numpy(x)).numpy(), want)
    assert same_bits(b.max_aggregate(torch.from_numpy(x)).numpy(), want), "CPU rows must take the torch path"
    empty = [d for d, r in enumerate(rows_of) if not r]
    assert empty and np.all(want_arg[empty] == -1) and same_bits(want[empty], np.zeros((len(empty), 9), dtype))
    if kind == "ties":
        assert tie_fraction(rows_of, x) > 0.5, "the tie-heavy inputs do not tie"
    if kind == "special":
        assert np.isnan(want).any() and np.isneginf(want).any() and np.signbit(want[want == 0]).any()


@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_weighted_max_in_torch(hiplib, form):
    """u_mul_e then max: the messages are h_src[s_j] * w_j, one weight per neighbour slot."""
    import torch
    rng = np.random.default_rng(2)
    b, rows_of, slots = _case(torch, rng, form)
    x = make_values(rng, "normal", 50, 6)
    w = rng.standard_normal(slots).astype(np.float32)
    w[rng.random(slots) < 0.1] = 0
    valid = (b.indices if b.nbr is None else b.nbr).numpy() >= 0
    if form == "fixed":
        w_of = [list(w[d][valid[d]]) for d in range(len(rows_of))]
    else:
        ip = b.indptr.numpy()
        w_of = [list(w[ip[d]: ip[d + 1]]) for d in range(len(rows_of))]
    want, want_arg = ref_max(rows_of, x, w_of)
    got, arg = b.max_aggregate_torch(torch.from_numpy(x), torch.from_numpy(w), return_arg=True)
    assert same_bits(got.numpy(), want) and np.array_equal(arg.numpy(), want_arg)


@pytest.mark.parametrize("kind", ["ties", "special"])
@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_gradient_goes_to_the_first_winner_only(hiplib, form, kind):
    """grad_src[arg[d, c], c] += grad_out[d, c]; integer gradients, so every sum is exact and the comparison is too."""
    import torch
    rng = np.random.default_rng(3)
    b, rows_of, _ = _case(torch, rng, form)
    x = make_values(rng, kind, 50, 9, np.float64)
    go = rng.integers(-8, 9, size=(len(rows_of), 9)).astype(np.float64)
    _, arg = ref_max(rows_of, x)
    want = np.zeros_like(x)
    for d, c in zip(*np.nonzero(arg >= 0)):
        want[arg[d, c], c] += go[d, c]
    h = torch.from_numpy(x).requires_grad_(True)
    (b.max_aggregate_torch(h) * torch.from_numpy(go)).sum().backward()
    assert np.array_equal(h.grad.numpy(), want)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_max_aggregate_torch_gradcheck(hiplib, form, weighted):
    """float64, values without ties (a source twice in a row still ties with itself: both slots are the same input)."""
    import torch
    rng = np.random.default_rng(4)
    if form == "fixed":
        nbr, _ = fixed_case(rng, n_dst=12, f=5, n_src=10)
        b, slots = fixed_block(torch, nbr, 10), nbr.shape
    else:
        indptr, indices, _ = ragged_case(rng, n_dst=12, n_src=10, long_row=70)
        b, slots = ragged_block(torch, indptr, indices, 10), indices.shape
    h = torch.from_numpy(rng.standard_normal((10, 3))).requires_grad_(True)
    if not weighted:
        assert torch.autograd.gradcheck(b.max_aggregate_torch, (h,))
    else:
        w = torch.from_numpy(rng.uniform(0.5, 1.5, size=slots) * rng.choice([-1.0, 1.0], size=slots)).requires_grad_(True)
        assert torch.autograd.gradcheck(b.max_aggregate_torch, (h, w))


def _weights_of(b, rows_of, w):
    if b.nbr is not None:
        valid = b.nbr.numpy() >= 0
        return [list(w[d][valid[d]]) for d in range(len(rows_of))]
    ip = b.indptr.numpy()
    return [list(w[ip[d]: ip[d + 1]]) for d in range(len(rows_of))]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_sageconv_pool_matches_float64(hiplib, form, weighted):
    import torch
    from COALA_GNN.nn import SAGEConv
    rng = np.random.default_rng(5)
    b, rows_of, slots = _case(torch, rng, form, n_src=70)
    n_dst, fin, fout = b.num_dst, 9, 4
    conv = SAGEConv(fin, fout, "pool").double()
    with torch.no_grad():
        conv.bias.copy_(torch.from_numpy(rng.standard_normal(fout)))
    x = rng.standard_normal((70, fin))
    w = rng.standard_normal(slots) if weighted else None
    got = conv(b, (torch.from_numpy(x), torch.from_numpy(x[:n_dst])), edge_weight=None if w is None else torch.from_numpy(w))
    sd = {k: v.numpy() for k, v in conv.state_dict().items()}
    pooled = np.maximum(x @ sd["fc_pool.weight"].T + sd["fc_pool.bias"], 0)
    neigh, _ = ref_max(rows_of, pooled, None if w is None else _weights_of(b, rows_of, w))
    ref = x[:n_dst] @ sd["fc_self.weight"].T + neigh @ sd["fc_neigh.weight"].T + sd["bias"]
    np.testing.assert_allclose(got.detach().numpy(), ref, rtol=1e-10, atol=1e-10)
    # without h_dst the destination rows are the first rows of h_src
    np.testing.assert_allclose(conv(b, torch.from_numpy(x), edge_weight=None if w is None else torch.from_numpy(w)).detach().numpy(), ref,
                               rtol=1e-10, atol=1e-10)


def test_sageconv_pool_parameters_follow_dgl(hiplib):
    import torch
    from COALA_GNN.nn import SAGEConv
    m = SAGEConv((12, 10), 6, "pool")
    want = {"fc_pool.weight": (12, 12), "fc_pool.bias": (12,), "fc_self.weight": (6, 10), "fc_neigh.weight": (6, 12), "bias": (6,)}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    torch.manual_seed(0)
    theirs = {k: torch.randn(s) for k, s in want.items()}          # a checkpoint with DGL's names and shapes
    m.load_state_dict(theirs, strict=True)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in theirs.items())
    assert torch.all(SAGEConv(5, 3, "pool").bias == 0)
    assert {k for k, _ in SAGEConv(5, 3, "pool", bias=False).named_parameters()} == {"fc_pool.weight", "fc_pool.bias", "fc_self.weight",
                                                                                     "fc_neigh.weight"}
    with pytest.raises(ValueError):
        SAGEConv(5, 3, "lstm")
    for agg in ("mean", "gcn"):                                     # the other aggregators get no fc_pool
        assert not any(k.startswith("fc_pool") for k in SAGEConv(5, 3, agg).state_dict())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("learn_eps", [False, True])
@pytest.mark.parametrize("agg", ["sum", "max", "mean"])
@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_ginconv_matches_float64(hiplib, form, agg, learn_eps, weighted):
    import torch
    from COALA_GNN.nn import GINConv
    rng = np.random.default_rng(6)
    b, rows_of, slots = _case(torch, rng, form, n_src=70)
    n_dst, fin, fout = b.num_dst, 7, 4
    lin = torch.nn.Linear(fin, fout).double()
    conv = GINConv(lin, agg, init_eps=0.25, learn_eps=learn_eps, activation=torch.tanh).double()
    assert conv.eps.dtype == torch.float64 and isinstance(conv.eps, torch.nn.Parameter) == learn_eps
    x = rng.standard_normal((70, fin))
    w = rng.standard_normal(slots) if weighted else None
    got = conv(b, (torch.from_numpy(x), torch.from_numpy(x[:n_dst])), edge_weight=None if w is None else torch.from_numpy(w))
    w_of = _weights_of(b, rows_of, w) if weighted else [[1.0] * len(r) for r in rows_of]
    if agg == "max":
        neigh, _ = ref_max(rows_of, x, w_of if weighted else None)
    else:
        neigh = np.zeros((n_dst, fin))
        for d, r in enumerate(rows_of):
            for s, ws in zip(r, w_of[d]):
                neigh[d] += x[s] * ws
            if agg == "mean":
                neigh[d] /= max(len(r), 1)
    ref = np.tanh((1.25 * x[:n_dst] + neigh) @ lin.weight.detach().numpy().T + lin.bias.detach().numpy())
    np.testing.assert_allclose(got.detach().numpy(), ref, rtol=1e-10, atol=1e-10)
    if learn_eps:                                                   # d out / d eps = h_dst, through apply_func and the activation
        got.sum().backward()
        assert conv.eps.grad is not None and conv.eps.grad.shape == (1,)


def test_ginconv_parameters_follow_dgl(hiplib):
    import torch
    from COALA_GNN.nn import GINConv
    m = GINConv(torch.nn.Linear(5, 3), "max", init_eps=0.5)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {"eps": (1,), "apply_func.weight": (3, 5), "apply_func.bias": (3,)}
    assert "eps" not in dict(m.named_parameters()) and float(m.eps) == 0.5
    m2 = GINConv(torch.nn.Linear(5, 3), "sum", learn_eps=True)
    assert "eps" in dict(m2.named_parameters()) and float(m2.eps.detach()) == 0.0
    theirs = {"eps": torch.tensor([0.75]), "apply_func.weight": torch.randn(3, 5), "apply_func.bias": torch.randn(3)}
    for mod in (m, m2):
        mod.load_state_dict(theirs, strict=True)
        assert float(mod.eps.detach()) == 0.75
    assert {k: tuple(v.shape) for k, v in GINConv().state_dict().items()} == {"eps": (1,)}     # no apply_func: the aggregate alone
    with pytest.raises(ValueError):
        GINConv(None, "lstm")


def test_ginconv_sum_is_an_exact_slot_order_sum(hiplib):
    """Integer rows: the unit-weight sum is exact in fp32, which mean * in_deg is not for a degree such as 3."""
    import torch
    from COALA_GNN.nn import GINConv
    rng = np.random.default_rng(7)
    b, rows_of, _ = _case(torch, rng, "fixed", n_src=70)
    x = rng.integers(-50, 50, size=(70, 8)).astype(np.float32)
    got = GINConv(None, "sum", init_eps=1)(b, torch.from_numpy(x)).numpy()
    ref = 2 * x[: b.num_dst] + np.stack([x[r].sum(0) if r else np.zeros(8, np.float32) for r in rows_of])
    assert np.array_equal(got, ref.astype(np.float32))


def test_models_build_and_run_on_cpu_blocks(hiplib):
    """SAGE('pool') and GIN of the harness: output shapes of 2-layer models on CPU blocks (the fallback path), and gradients for every
    parameter."""
    import torch
    from COALA_GNN.harness import GIN, SAGE
    rng = np.random.default_rng(8)
    nbr1 = rng.integers(-1, 30, size=(12, 5)).astype(np.int32)
    nbr2 = rng.integers(-1, 12, size=(4, 5)).astype(np.int32)
    blocks = [fixed_block(torch, nbr1, 30), fixed_block(torch, nbr2, 12)]
    x = torch.randn(30, 8)
    models = [SAGE(8, 6, 5, 2, aggregator_type="pool")] + [GIN(8, 6, 5, 2, aggregator_type=a, learn_eps=a == "max") for a in ("sum", "max", "mean")]
    for model in models:
        out = model(blocks, x)
        assert out.shape == (4, 5)
        out.sum().backward()
        assert all(p.grad is not None for p in model.parameters())


def test_new_symbols_resolve_and_the_abi_version_stays(hiplib):
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    for name in ("coala_block_max_aggregate", "coala_block_max_aggregate_csr", "coala_block_max_aggregate_backward"):
        assert name in _capi.SYMBOLS and getattr(L, name) is not None
    assert L.coala_abi_version() == 4
