"""CPU tests of SparseAdam and RowWiseAdagrad (COALA_GNN/embedding.py): the new C symbols, the torch backend against the float64 one-step
references (tests/_optim_ref.py), the references themselves against torch.optim.SparseAdam and against DGL-KE's four lines, the refusals
of the Python layer and the state placement."""
import numpy as np
import pytest
import torch

from _optim_ref import (check_adam, check_rowwise_adagrad, make_grad, naive_bc2_misses, rowwise_additions, rowwise_additions_torch,
                        rowwise_adagrad_ref)

LR, EPS = 0.05, 1e-8


def test_optimizer_symbols_resolve_and_the_abi_version_stays(hiplib):
    import ctypes as C
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    for name in ("coala_cache_adam_rows", "coala_cache_rowwise_adagrad_rows"):
        assert name in _capi.SYMBOLS and getattr(L, name) is not None
    assert L.coala_abi_version() == 4
    assert hasattr(hiplib.Isolated_Cache, "adam_rows") and hasattr(hiplib.Isolated_Cache, "rowwise_adagrad_rows")
    if hiplib.native is not None:
        assert hasattr(hiplib.native, "cache_adam_rows") and hasattr(hiplib.native, "cache_rowwise_adagrad_rows")
    # refused before anything touches a device: a null handle (whatever else is wrong with the call)
    assert L.coala_cache_adam_rows(None, None, 0, None, None, None, None, 0, 0.1, 0.9, 0.999, 1e-8, None) == _capi.EINVAL
    assert "null handle" in _capi.last_error()
    assert L.coala_cache_adam_rows(None, None, 0, None, None, None, None, 1, 0.1, 1.5, 0.999, 1e-8, None) == _capi.EINVAL
    assert "null handle" in _capi.last_error()
    assert L.coala_cache_rowwise_adagrad_rows(None, None, 0, None, None, 0.1, 1e-10, None) == _capi.EINVAL
    assert "null handle" in _capi.last_error()
    assert _capi.SYMBOLS["coala_cache_adam_rows"][1][7] is C.c_int64          # step


def _ids_with_pairs(rng, num_rows, n_single, n_twice):
    ids = rng.choice(num_rows, size=n_single + n_twice, replace=False)
    return rng.permutation(np.concatenate([ids, ids[:n_twice]])).astype(np.int64)


def _reduced(ids, coef, reduce):
    """fp32 sum of the rows of coef per distinct id (every id occurs at most twice; the sum of two does not depend on the order)."""
    uniq, first, cnt = np.unique(ids, return_index=True, return_counts=True)
    g = coef[first].copy()
    for k in np.flatnonzero(cnt == 2):
        a, b = np.flatnonzero(ids == uniq[k])
        g[k] = coef[a] + coef[b]
    if reduce == "mean":
        g = g / cnt.astype(np.float32)[:, None]
    return uniq, g


def _backward(emb, ids, coef):
    rows = emb(torch.from_numpy(ids))
    (rows * torch.from_numpy(coef)).sum().backward()


@pytest.mark.parametrize("reduce", ["mean", "sum"])
@pytest.mark.parametrize("mode", ["row", "global"])
def test_torch_backend_adam_matches_the_reference(hiplib, mode, reduce):
    from COALA_GNN import NodeEmbedding, SparseAdam
    num_rows, dim = 400, 24
    rng = np.random.default_rng(3)
    torch.manual_seed(0)
    emb = NodeEmbedding(num_rows, dim, device="cpu", backend="torch")
    opt = SparseAdam([emb], lr=LR, betas=(0.9, 0.999), eps=EPS, reduce=reduce, step=mode)
    late = np.arange(num_rows - 40, num_rows)                  # rows that sit out the first step: their own t lags the global count
    for step in range(1, 5):
        pool = num_rows - 40 if step == 1 else num_rows
        ids = _ids_with_pairs(rng, pool, 80, 30)
        if step > 1:
            ids = np.unique(np.concatenate([ids, late[:10]]))
        coef = make_grad(rng, (len(ids), dim))
        uniq, g = _reduced(ids, coef, reduce)
        m, v, steps = opt.state_of(emb)[:3]
        w0, m0, v0, t0 = emb.weight.numpy().copy(), m.numpy().copy(), v.numpy().copy(), steps.numpy().copy()
        opt.zero_grad()
        _backward(emb, ids, coef)
        opt.step()
        assert emb.trace == [] and opt.steps == step
        t = t0[uniq] + 1 if mode == "row" else step
        check_adam(emb.weight.numpy()[uniq], m.numpy()[uniq], v.numpy()[uniq], w0[uniq], m0[uniq], v0[uniq], t, g, LR, 0.9, 0.999, EPS,
                   f"torch backend, step={mode} {reduce}, step {step}")
        rest = np.ones(num_rows, dtype=bool)
        rest[uniq] = False
        for a, b in ((emb.weight.numpy(), w0), (m.numpy(), m0), (v.numpy(), v0), (steps.numpy(), t0)):
            assert a[rest].tobytes() == b[rest].tobytes()
        if mode == "row":
            assert np.array_equal(steps.numpy()[uniq], t0[uniq] + 1)
        else:
            assert not steps.numpy().any()                     # the global count never touches the vector
    if mode == "row":
        assert int(opt.state_of(emb)[2][late[:10]].max()) == 3 < opt.steps


def test_torch_backend_adam_counter_saturates(hiplib):
    from COALA_GNN import NodeEmbedding, SparseAdam
    emb = NodeEmbedding(10, 4, device="cpu", backend="torch")
    opt = SparseAdam(emb, lr=LR)
    steps = opt.state_of(emb)[2]
    steps[3] = 2 ** 31 - 1
    w0 = emb.weight.numpy().copy()
    _backward(emb, np.array([3, 4]), np.ones((2, 4), dtype=np.float32))
    opt.step()
    assert steps.tolist()[3:5] == [2 ** 31 - 1, 1]
    z = np.zeros((2, 4), dtype=np.float32)
    check_adam(emb.weight.numpy()[3:5], *(s.numpy()[3:5] for s in opt.state_of(emb)[:2]), w0[3:5], z, z, [2 ** 31 - 1, 1], np.ones((2, 4)),
               LR, 0.9, 0.999, 1e-8, "saturated counter")


@pytest.mark.parametrize("reduce", ["mean", "sum"])
@pytest.mark.parametrize("dim", [1, 24, 64])
def test_torch_backend_rowwise_adagrad_matches_the_reference(hiplib, dim, reduce):
    from COALA_GNN import NodeEmbedding, RowWiseAdagrad
    num_rows = 300
    rng = np.random.default_rng(dim)
    emb = NodeEmbedding(num_rows, dim, device="cpu", backend="torch")
    opt = RowWiseAdagrad([emb], lr=LR, eps=1e-10, reduce=reduce)
    assert opt.state_of(emb)[0].shape == (num_rows,) and opt.state_of(emb)[0].dtype == torch.float32
    for step in range(3):
        ids = _ids_with_pairs(rng, num_rows, 60, 25)
        coef = make_grad(rng, (len(ids), dim))
        uniq, g = _reduced(ids, coef, reduce)
        w0, s0 = emb.weight.numpy().copy(), opt.state_of(emb)[0].numpy().copy()
        opt.zero_grad()
        _backward(emb, ids, coef)
        opt.step()
        check_rowwise_adagrad(emb.weight.numpy()[uniq], opt.state_of(emb)[0].numpy()[uniq], w0[uniq], s0[uniq], g, LR, 1e-10,
                              rowwise_additions_torch(dim), f"torch backend, dim {dim} {reduce}, step {step}")
        rest = np.ones(num_rows, dtype=bool)
        rest[uniq] = False
        assert emb.weight.numpy()[rest].tobytes() == w0[rest].tobytes() and opt.state_of(emb)[0].numpy()[rest].tobytes() == s0[rest].tobytes()


def test_the_adam_reference_states_torch_sparse_adam(hiplib):
    """torch.optim.SparseAdam on nn.Embedding(sparse=True), three steps, each within TWICE the bound of adam_ref at the global step from
    its own snapshot (torch rounds sqrt(v) / sqrt(bc2) differently, and forms exp_avg in fp32 without carrying the product's error).
    torch takes lr and the betas as Python doubles in its bias corrections and as fp32 in its tensor ops; the C ABI, and so the
    reference, knows only their fp32 values.  The scalars here are exact in fp32 (1 - 2^-3, 1 - 2^-10, 2^-4), so both mean the same
    numbers -- with 0.999 the two readings of beta2 differ by 1.3e-5 of bc2 at step 1, a thousand bounds.
    eps = 2^-100, below half an ulp of every sqrt(v) here (torch refuses 0): torch.optim.SparseAdam adds eps to sqrt(v) BEFORE the division by sqrt(bc2) (lr sqrt(bc2) / bc1 * m / (sqrt(v) + eps)),
    DGL's SparseAdam and torch.optim.Adam after it (sqrt(v / bc2) + eps, the rule of the C ABI); the two are the same rule up to
    rounding only where eps does not count, and differ by eps (1 / sqrt(bc2) - 1) in the denominator otherwise -- 30 eps at step 1."""
    num_rows, dim = 60, 8
    lr, b1, b2, eps = 2.0 ** -4, 1 - 2.0 ** -3, 1 - 2.0 ** -10, 2.0 ** -100
    rng = np.random.default_rng(5)
    torch.manual_seed(0)
    ref = torch.nn.Embedding(num_rows, dim, sparse=True)
    ropt = torch.optim.SparseAdam(list(ref.parameters()), lr=lr, betas=(b1, b2), eps=eps)
    for step in range(1, 4):
        ids = _ids_with_pairs(rng, num_rows, 20, 8)
        coef = make_grad(rng, (len(ids), dim))
        uniq, g = _reduced(ids, coef, "sum")
        st = ropt.state[ref.weight]
        w0 = ref.weight.detach().numpy().copy()
        m0 = st["exp_avg"].numpy().copy() if st else np.zeros_like(w0)
        v0 = st["exp_avg_sq"].numpy().copy() if st else np.zeros_like(w0)
        ropt.zero_grad()
        (ref(torch.from_numpy(ids)) * torch.from_numpy(coef)).sum().backward()
        ropt.step()
        st = ropt.state[ref.weight]
        check_adam(ref.weight.detach().numpy()[uniq], st["exp_avg"].numpy()[uniq], st["exp_avg_sq"].numpy()[uniq], w0[uniq], m0[uniq],
                   v0[uniq], step, g, lr, b1, b2, eps, f"torch.optim.SparseAdam, step {step}", scale=2.0)


def test_the_rowwise_reference_states_dglke(hiplib):
    """DGL-KE's row-wise Adagrad, its four lines transcribed to numpy in fp32: grad_sum = mean(g * g, 1); state_sum.index_add_(ids,
    grad_sum); std = sqrt(state_sum[ids]) + eps; emb.index_add_(ids, -lr * g / std)."""
    rng = np.random.default_rng(6)
    dim, n = 16, 40
    ids = rng.choice(100, size=n, replace=False)
    w = rng.uniform(-1, 1, size=(100, dim)).astype(np.float32)
    state = np.abs(rng.normal(size=100)).astype(np.float32)
    g = make_grad(rng, (n, dim))
    w0, s0 = w.copy(), state.copy()
    lr, eps = np.float32(LR), np.float32(1e-10)
    grad_sum = (g * g).mean(axis=1, dtype=np.float32)
    np.add.at(state, ids, grad_sum)
    std = np.sqrt(state[ids]) + eps
    np.add.at(w, ids, (-lr * g / std[:, None]).astype(np.float32))
    # numpy sums 16 floats pairwise in blocks of 8: at most 8 additions on a path
    check_rowwise_adagrad(w[ids], state[ids], w0[ids], s0[ids], g, LR, 1e-10, 8, "DGL-KE's four lines")
    ref, s, _ = rowwise_adagrad_ref(w0[ids], s0[ids], g, LR, 1e-10)
    assert np.allclose(w[ids], ref, rtol=1e-5, atol=1e-7) and np.allclose(state[ids], s, rtol=1e-6)


def test_the_naive_bias_correction_is_what_the_first_steps_tell_apart(hiplib):
    """1 - float32(beta2) ** t in fp32 against -expm1(t ln beta2).  At t = 1 the fp32 form is exact relative to the fp32 beta2 the ABI
    receives (1 - beta2 is a Sterbenz subtraction), so a t = 1 case alone cannot tell the two apart; from t = 2 on the fp32 form is
    outside the rows bound at beta2 = 0.999 and 0.9999.  The GPU tests therefore run fresh rows at t = 1 AND rows at their second step."""
    for beta2 in (0.999, 0.9999):
        assert not naive_bc2_misses(beta2, 1)
        assert naive_bc2_misses(beta2, 2)


def test_additions_on_the_longest_path(hiplib):
    # (dim, 16-byte path) -> A, by the kernel's geometry: 128-float line = 32 lanes x 1 vfloat4 or 64 lanes x 2 floats; 1024 = 64 x 4 x 4 or 64 x 16
    assert [rowwise_additions(d, v) for d, v in ((128, True), (100, True), (99, False), (1, False), (1024, True), (1024, False), (256, True))] == \
        [3 + 5, 3 + 5, 1 + 6, 1 + 6, 15 + 6, 15 + 6, 3 + 6]


def test_validation_errors(hiplib):
    from COALA_GNN import NodeEmbedding, RowWiseAdagrad, SparseAdam
    emb = NodeEmbedding(10, 4, device="cpu", backend="torch")
    for betas in ((1.0, 0.999), (0.9, -0.1), (0.9,), "ab", (0.9, 1.5)):
        with pytest.raises(ValueError, match="betas"):
            SparseAdam([emb], lr=0.1, betas=betas)
    with pytest.raises(ValueError, match="step"):
        SparseAdam([emb], lr=0.1, step="lazy")
    with pytest.raises(ValueError, match="reduce"):
        SparseAdam([emb], lr=0.1, reduce="max")
    with pytest.raises(ValueError, match="lr"):
        SparseAdam([emb], lr=0.0)
    with pytest.raises(ValueError, match="eps"):
        SparseAdam([emb], lr=0.1, eps=-1.0)
    with pytest.raises(ValueError, match="reduce"):
        RowWiseAdagrad([emb], lr=0.1, reduce="max")
    with pytest.raises(ValueError, match="lr"):
        RowWiseAdagrad([emb], lr=-1.0)
    with pytest.raises(ValueError, match="eps"):
        RowWiseAdagrad([emb], lr=0.1, eps=-1e-3)
    with pytest.raises(TypeError):
        SparseAdam([torch.nn.Embedding(3, 3)], lr=0.1)
    with pytest.raises(TypeError):
        SparseAdam([emb], lr=0.1, amsgrad=True)                 # out of scope: not in the signature
    SparseAdam([emb], lr=0.1, betas=(0.0, 0.0)).step()          # nothing looked up: nothing to do
    RowWiseAdagrad(emb, lr=0.1).step()


def test_state_placement_arithmetic(hiplib):
    """m, v and the step vector go to HBM when num_rows * (2 * dim + 1) * 4 bytes fit state_device_bytes; the torch backend keeps
    them on its own device whatever the budget."""
    from COALA_GNN import NodeEmbedding, RowWiseAdagrad, SparseAdam
    emb = NodeEmbedding(100, 8, device="cpu", backend="torch")
    opt = SparseAdam([emb], lr=0.1, state_device_bytes=0)
    assert opt.state_bytes(emb) == 100 * 17 * 4
    m, v, steps, m_ptr, v_ptr = opt.state_of(emb)
    assert m.shape == v.shape == (100, 8) and m.dtype == v.dtype == torch.float32 and not m.any() and not v.any()
    assert steps.shape == (100,) and steps.dtype == torch.int32 and not steps.any()
    assert (m_ptr, v_ptr) == (m.data_ptr(), v.data_ptr()) and m_ptr != v_ptr
    assert opt.state_of(emb)[0] is m                            # made once
    t, ptr = RowWiseAdagrad([emb], lr=0.1).state_of(emb)
    assert t.shape == (100,) and ptr == t.data_ptr()

    class Native:                                               # what state_of reads of a native embedding
        backend, num_rows, dim, device = "native", 1000, 32, torch.device("cpu")
    fits = SparseAdam([emb], lr=0.1, state_device_bytes=1000 * 65 * 4)
    assert fits.state_bytes(Native) == 1000 * 65 * 4
    assert fits.state_of(Native)[0].shape == (1000, 32)         # exactly fits: plain tensors on the device
