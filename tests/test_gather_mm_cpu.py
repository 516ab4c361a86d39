"""CPU tests of the typed linear step: the C symbols and their shape checks, gather_mm_torch (the fallback of block_ops.gather_mm and
its reference) against a float64 loop, and nn.TypedLinear's parameters."""
import numpy as np
import pytest


def test_symbols_and_shape_checks(hiplib):
    from COALA_GNN_Pybind import _capi
    L, nil = _capi.load(), (None,) * 7
    for name in ("coala_block_gather_mm_plan_work", "coala_block_gather_mm_plan", "coala_block_gather_mm", "coala_block_gather_mm_backward_w"):
        assert name in _capi.SYMBOLS and hasattr(L, name)
    assert L.coala_block_gather_mm_plan_work(257, 3) == 2 * 4 and L.coala_block_gather_mm_plan_work(0, 3) == 0
    for T, K, N in ((0, 8, 8), (65, 8, 8), (4, 0, 8), (4, 8, 0)):
        assert L.coala_block_gather_mm(0, *nil, 5, T, K, N, 0, None) == _capi.EINVAL and "typed product shape" in _capi.last_error()
        assert L.coala_block_gather_mm_backward_w(0, *nil, 5, T, K, N, None) == _capi.EINVAL
        assert T not in (0, 65) or L.coala_block_gather_mm_plan(0, None, None, 5, T, None, None, None, None) == _capi.EINVAL
    assert L.coala_block_gather_mm_plan(0, None, None, 0, 4, None, None, None, None) == _capi.OK
    assert L.coala_block_gather_mm(0, *nil, 0, 4, 8, 8, 1, None) == _capi.OK and L.coala_block_gather_mm_backward_w(0, *nil, 0, 4, 8, 8, None) == _capi.OK
    assert L.coala_block_gather_mm(0, *nil, 5, 4, 8, 8, 0, None) == _capi.EINVAL and "null buffer" in _capi.last_error()


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("use_rows", [False, True])
def test_gather_mm_torch(hiplib, use_rows, transposed):
    import torch
    from COALA_GNN.block_ops import gather_mm, gather_mm_torch
    rng = np.random.default_rng(2 * use_rows + transposed)
    n, T, K, N = 30, 3, 5, 4
    M = 50 if use_rows else n
    x, W = rng.standard_normal((n, K)), rng.standard_normal((T, N, K) if transposed else (T, K, N))
    types, g = rng.integers(-1, T + 1, size=M), rng.standard_normal((M, N))
    rows = rng.integers(-1, n - 3, size=M) if use_rows else None
    want, gx, gw = np.zeros((M, N)), np.zeros_like(x), np.zeros_like(W)
    for i in range(M):
        a = i if rows is None else rows[i]
        if 0 <= types[i] < T and a >= 0:
            Wt = W[types[i]].T if transposed else W[types[i]]
            want[i], gx[a] = x[a] @ Wt, gx[a] + Wt @ g[i]
            gw[types[i]] += np.outer(g[i], x[a]) if transposed else np.outer(x[a], g[i])
    for fn in (gather_mm, gather_mm_torch):               # on the CPU gather_mm is its fallback
        xt, Wt_ = torch.from_numpy(x).requires_grad_(), torch.from_numpy(W).requires_grad_()
        y = fn(xt, Wt_, torch.from_numpy(types), None if rows is None else torch.from_numpy(rows), transposed=transposed)
        y.backward(torch.from_numpy(g))
        assert all(np.abs(got.numpy() - ref).max() <= 1e-12 for got, ref in ((y.detach(), want), (xt.grad, gx), (Wt_.grad, gw)))
        assert np.all(y.detach().numpy()[(types < 0) | (types >= T)] == 0)
    empty = torch.zeros(0, dtype=torch.int64)
    assert gather_mm(torch.from_numpy(x), torch.from_numpy(W), empty, empty, transposed=transposed).shape == (0, N)
    with pytest.raises(IndexError):
        gather_mm(torch.from_numpy(x), torch.from_numpy(W), torch.tensor([0]), torch.tensor([n]), transposed=transposed)
    with pytest.raises(ValueError):
        gather_mm(torch.from_numpy(x), torch.from_numpy(W), torch.tensor([0.5] * n), transposed=transposed)


def test_typed_linear_module(hiplib):
    import torch
    from COALA_GNN.nn import TypedLinear
    m = TypedLinear(6, 4, 3)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {"W": (3, 6, 4)} and float(m.W.detach().abs().max()) <= 6 ** -0.5
    x, t = torch.randn(7, 6), torch.tensor([2, 0, 1, 1, 0, 2, 3])
    y = m(x, t, sorted_by_type=True)
    assert torch.allclose(y[:6], torch.einsum("ni,nio->no", x[:6], m.W[t[:6]]), atol=1e-6) and torch.all(y[6] == 0)
    for kw in ({"regularizer": "basis"}, {"num_bases": 2}):
        with pytest.raises(ValueError):
            TypedLinear(6, 4, 3, **kw)
