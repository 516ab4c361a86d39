"""GPU tests of the scaled dot-product attention kernels (coala_block_dot_gat_aggregate[_csr][_backward] in coala_block_ops.hip)
against float64.

Called through the C ABI on hand-made blocks: fixed rows with -1 anywhere, destinations without an edge, repeated rows, fan-outs 1..32;
CSR rows of degree 0 to past one 64-slot chunk and a hub of 4,097 edges (65 chunks); heads 1..16; D in {1, 3, 16, 64, 65, 128}; the
16-byte path and the scalar path (D % 4 != 0, or buffers one float off 16-byte alignment); n_dst 0, 1 and 100,003, past the grid cap;
scores up to +-1e3; k and v tables whose row count differs from the block's source count.  Every output is followed by sentinel guard
words, and every input is checked untouched.

Tolerances.  Every bound is the first-order roundoff bound derived in tests/_dot_gat_ref.py's docstring from the kernels' summation
orders -- the score's D-term dot (lane scan and LDS adds) and its scale, 3 ulp for exp and log, one rescale per chunk of the online
softmax, the slot-order sum of grad_q, atomics in any order for grad_k and grad_v.  Every element of every output is compared.  The CPU
twin (tests/test_dot_gat_cpu.py) shows that an fp32 evaluation in the kernels' order lies inside these bounds and that three wrong
kernels would not."""
import numpy as np
import pytest

import _dot_gat_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e33)
GUARD = 67


def _device(torch, arr, off, fill=None):
    flat = torch.full((off + arr.size + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    if fill is None:
        flat[off: off + arr.size] = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)).cuda()
    else:
        flat[off: off + arr.size] = fill
    return flat, flat.data_ptr() + 4 * off


def _region(flat, off, shape):
    h = flat.cpu().numpy()
    n = int(np.prod(shape))
    pad = np.concatenate([h[:off], h[off + n:]])
    assert np.array_equal(pad.view(np.int32), np.full(pad.shape, SENTINEL).view(np.int32)), "write outside the output region"
    return h[off: off + n].reshape(shape)


def _run(torch, L, form, graph, n_dst, P, q, k, v, g, scale, off, want=(True, True, True)):
    """Forward and backward through the C ABI, every float buffer at float offset `off`, sentinels around every output and filling the
    outputs that are written whole.  want: which of grad_q, grad_k, grad_v are asked for (a null pointer otherwise).
    -> dict of out, lse, gq, gk, gv."""
    from COALA_GNN_Pybind import _capi, current_stream
    H, D = k.shape[1], k.shape[2]
    ins = dict(q=q, k=k, v=v, g=g)
    bufs = {n: _device(torch, a, off) for n, a in ins.items()}
    o_buf, o = _device(torch, np.empty((n_dst, H, D), np.float32), off, fill=float(SENTINEL))
    s_buf, lse = _device(torch, np.empty((n_dst, H), np.float32), off, fill=float(SENTINEL))
    gq_buf, gq = _device(torch, np.empty((n_dst, H, D), np.float32), off, fill=float(SENTINEL))
    gk_buf, gk = _device(torch, np.empty((P, H, D), np.float32), off, fill=0.0)
    gv_buf, gv = _device(torch, np.empty((P, H, D), np.float32), off, fill=0.0)
    p = {n: b[1] for n, b in bufs.items()}
    st = current_stream()
    grads = (gq if want[0] else None, gk if want[1] else None, gv if want[2] else None)
    if form == "fixed":
        dn = torch.from_numpy(graph).cuda()
        f = graph.shape[1]
        _capi.check(L.coala_block_dot_gat_aggregate(0, dn.data_ptr(), p["q"], p["k"], p["v"], o, lse, n_dst, f, H, D, float(scale), st))
        _capi.check(L.coala_block_dot_gat_aggregate_backward(0, dn.data_ptr(), p["q"], p["k"], p["v"], o, lse, p["g"], *grads, n_dst, f, H, D,
                                                             float(scale), st))
    else:
        indptr, rows = graph
        dp = torch.from_numpy(indptr).cuda()
        di = torch.from_numpy(np.append(rows, np.int32(-1))).cuda()   # one word past the edges: a block without edges has a buffer
        _capi.check(L.coala_block_dot_gat_aggregate_csr(0, dp.data_ptr(), di.data_ptr(), p["q"], p["k"], p["v"], o, lse, n_dst, H, D,
                                                        float(scale), st))
        _capi.check(L.coala_block_dot_gat_aggregate_csr_backward(0, dp.data_ptr(), di.data_ptr(), p["q"], p["k"], p["v"], o, lse, p["g"], *grads,
                                                                 n_dst, H, D, float(scale), st))
    torch.cuda.synchronize()
    res = dict(out=_region(o_buf, off, (n_dst, H, D)), lse=_region(s_buf, off, (n_dst, H)), gq=_region(gq_buf, off, (n_dst, H, D)),
               gk=_region(gk_buf, off, (P, H, D)), gv=_region(gv_buf, off, (P, H, D)))
    for n, a in ins.items():                                                       # inputs untouched
        assert np.array_equal(_region(bufs[n][0], off, a.shape), a)
    return res


def _fixed_case(torch, L, n_dst, f, H, D, off, big, log=None):
    row, P, (q, k, v, g), scale, (dst, rows, nc) = R.small_case((n_dst, f, H, D, off, big))
    got = _run(torch, L, "fixed", row, n_dst, P, q, k, v, g, scale, off)
    R.check_all(got, R.reference(dst, rows, n_dst, P, nc, q, k, v, g, scale), log)
    assert np.all(got["gk"][P - 7:] == 0.0) and np.all(got["gv"][P - 7:] == 0.0), "an unreferenced row has a gradient"


LARGE_CASES = [(0, 4, 2, 8, 0, False), (1, 1, 1, 1, 1, False), (1, 5, 2, 4, 0, False), (100_003, 9, 1, 4, 0, False)]


@pytest.mark.parametrize("n_dst,f,H,D,off,big", R.SMALL_CASES + LARGE_CASES)
def test_dot_gat_fixed_against_float64(hiplib, n_dst, f, H, D, off, big):
    import torch
    from COALA_GNN_Pybind import _capi
    _fixed_case(torch, _capi.load(), n_dst, f, H, D, off, big, log=print)


@pytest.mark.parametrize("n_dst,f,H,D,off,big", R.SMALL_CASES + [(0, 1, 1, 4, 0, False), (1, 3, 2, 4, 1, False)])
def test_dot_gat_csr_against_float64(hiplib, n_dst, f, H, D, off, big):
    """Degrees 0..2f, 5 % of the rows at 65..200 edges (two to four chunks: the online rescale, grad_q added to across chunks), row 0
    empty."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(n_dst * 5 + f * 31 + H * 3 + D + off)
    P = max(64, min(5000, n_dst // 4))
    indptr, rows = R.csr_rows(rng, n_dst, f, P)
    q, k, v, g = R.make_inputs(rng, P, n_dst, H, D, big)
    scale = R.scale_of(D)
    got = _run(torch, L, "csr", (indptr, rows), n_dst, P, q, k, v, g, scale, off)
    dst, rr, nc = R.edges_csr(indptr, rows)
    R.check_all(got, R.reference(dst, rr, n_dst, P, nc, q, k, v, g, scale), log=print)


@pytest.mark.parametrize("big", [False, True])
def test_dot_gat_csr_hub_against_float64(hiplib, big):
    """One row of 4,097 edges (65 chunks of the online softmax; grad_q added to chunk after chunk) between small rows, some of its
    slots -1."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(99 + big)
    P, H, D = 700, 2, 6
    deg = rng.integers(0, 9, size=41)
    deg[20] = 4097
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    rows = rng.integers(0, P, size=int(indptr[-1])).astype(np.int32)
    rows[rng.random(rows.shape) < 0.02] = -1
    q, k, v, g = R.make_inputs(rng, P, len(deg), H, D, big)
    scale = R.scale_of(D)
    got = _run(torch, L, "csr", (indptr, rows), len(deg), P, q, k, v, g, scale, 0)
    dst, rr, nc = R.edges_csr(indptr, rows)
    R.check_all(got, R.reference(dst, rr, len(deg), P, nc, q, k, v, g, scale), log=print)


@pytest.mark.parametrize("f,H,D,off,big", [(5, 4, 16, 0, False), (32, 2, 65, 1, True), (17, 8, 3, 0, True), (1, 16, 128, 1, False)])
def test_dot_gat_fixed_and_csr_give_identical_bits(hiplib, f, H, D, off, big):
    """Fixed rows whose valid entries come first (the sampler's layout) against the same rows in CSR form, and each against a second
    run of itself: out, lse and grad_q bit for bit."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(f * 11 + H + D + off)
    n_dst, P = (2000, 700) if H * D <= 512 else (300, 100)
    deg = rng.integers(0, f + 1, size=n_dst)
    deg[:3] = [0, f, 1]
    row = np.full((n_dst, f), -1, np.int32)
    for d in range(n_dst):
        row[d, :deg[d]] = rng.integers(0, P, size=deg[d])
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    rows = row[row >= 0].astype(np.int32)
    q, k, v, g = R.make_inputs(rng, P, n_dst, H, D, big)
    scale = R.scale_of(D)
    a = _run(torch, L, "fixed", row, n_dst, P, q, k, v, g, scale, off)
    a2 = _run(torch, L, "fixed", row, n_dst, P, q, k, v, g, scale, off)
    b = _run(torch, L, "csr", (indptr, rows), n_dst, P, q, k, v, g, scale, off)
    for n in ("out", "lse", "gq"):
        assert np.array_equal(a[n].view(np.int32), b[n].view(np.int32)), f"{n} differs between the fixed and the CSR kernels"
        assert np.array_equal(a[n].view(np.int32), a2[n].view(np.int32)), f"{n} differs between two launches"
    assert np.all(np.isneginf(a["lse"][deg == 0])) and np.isfinite(a["lse"][deg > 0]).all()


@pytest.mark.parametrize("form", ["fixed", "csr"])
def test_dot_gat_null_gradients_are_not_written(hiplib, form):
    """Each of the three gradient pointers null in turn (and in pairs): grad_q keeps the bits of the full call, grad_k and grad_v stay
    inside the bounds, and the buffer behind a null stays as it was."""
    import itertools
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(23)
    n_dst, P, H, D = 500, 200, 4, 16
    scale = R.scale_of(D)
    if form == "fixed":
        graph = R.fixed_rows(rng, n_dst, 7, P)
        dst, rr, nc = R.edges_fixed(graph)
    else:
        graph = R.csr_rows(rng, n_dst, 6, P)
        dst, rr, nc = R.edges_csr(*graph)
    q, k, v, g = R.make_inputs(rng, P, n_dst, H, D, False)
    ref = R.reference(dst, rr, n_dst, P, nc, q, k, v, g, scale)
    full = _run(torch, L, form, graph, n_dst, P, q, k, v, g, scale, 0)
    R.check_all(full, ref)
    for want in itertools.product([False, True], repeat=3):
        got = _run(torch, L, form, graph, n_dst, P, q, k, v, g, scale, 0, want=want)
        for on, n, untouched in zip(want, R.GRADS, (float(SENTINEL), 0.0, 0.0)):
            if not on:
                assert np.all(got[n] == np.float32(untouched)), f"{n} was written through a null pointer's buffer"
            elif n == "gq":
                assert np.array_equal(got["gq"].view(np.int32), full["gq"].view(np.int32))
            else:
                R.check(n, got[n], ref[n])


def test_dot_gat_refuses_bad_shapes(hiplib):
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    st = current_stream()
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    i64 = torch.zeros(65, dtype=torch.int64, device="cuda")
    a = torch.zeros(4096, device="cuda")
    b = torch.full((4096,), float(SENTINEL), device="cuda")
    A, B, N, P = a.data_ptr(), b.data_ptr(), i32.data_ptr(), i64.data_ptr()
    for n, f, H, D in ((1, 0, 2, 4), (1, 33, 2, 4), (1, 4, 0, 4), (1, 4, 17, 4), (1, 4, 2, 0), (-1, 4, 2, 4), (0, 33, 2, 4)):
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_dot_gat_aggregate(0, N, A, A, A, B, B, n, f, H, D, 0.5, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_dot_gat_aggregate_backward(0, N, A, A, A, A, A, A, B, B, B, n, f, H, D, 0.5, st))
    for n, H, D in ((1, 0, 4), (1, 17, 4), (1, 2, 0), (-1, 2, 4)):
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_dot_gat_aggregate_csr(0, P, N, A, A, A, B, B, n, H, D, 0.5, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_dot_gat_aggregate_csr_backward(0, P, N, A, A, A, A, A, A, B, B, B, n, H, D, 0.5, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_dot_gat_aggregate(0, N, A, None, A, B, B, 1, 4, 2, 4, 0.5, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_dot_gat_aggregate(0, None, A, A, A, B, B, 1, 4, 2, 4, 0.5, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_dot_gat_aggregate_backward(0, N, A, A, A, A, None, A, B, B, B, 1, 4, 2, 4, 0.5, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_dot_gat_aggregate_csr(0, None, N, A, A, A, B, B, 1, 2, 4, 0.5, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_dot_gat_aggregate_csr_backward(0, P, None, A, A, A, A, A, A, B, B, B, 1, 2, 4, 0.5, st))
    # n_dst == 0 is fine before any pointer is looked at; so is a backward nobody wants anything from
    _capi.check(L.coala_block_dot_gat_aggregate(0, None, None, None, None, None, None, 0, 4, 2, 4, 0.5, st))
    _capi.check(L.coala_block_dot_gat_aggregate_csr_backward(0, None, None, None, None, None, None, None, None, None, None, None, 0, 2, 4, 0.5, st))
    _capi.check(L.coala_block_dot_gat_aggregate_backward(0, N, A, A, A, A, A, A, None, None, None, 1, 4, 2, 4, 0.5, st))
    torch.cuda.synchronize()
    assert torch.all(b == float(SENTINEL))
