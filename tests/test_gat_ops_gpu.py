"""GPU tests of the GAT attention kernels (coala_block_gat_aggregate[_csr][_backward] in coala_block_ops.hip) against float64.

Called through the C ABI on hand-made blocks: fixed rows with -1 anywhere, rows without a valid edge, repeated sources, fan-outs
1..32; CSR rows of degree 0 to past one 64-edge chunk and a hub of 1,000,003 in-edges; heads 1, 2, 4, 8; D in {1, 3, 16, 64, 65,
128, 256}; the 16-byte path and the scalar path (D % 4 != 0, or buffers one float off 16-byte alignment); n_dst up to 100,003, past
the 32,768 waves of the grid; scores up to +-1e3.  Every output is followed by sentinel guard words.

Bounds.  First order in u = 2^-24 (fp32 unit roundoff), gamma(n) = n u / (1 - n u); each bound is multiplied by 1.01 for the
second-order terms (every relative term below stays under 1e-2) and gets an absolute 2^-100 times the magnitude it scales, for
weights that underflow.  exp and log are taken to be within 3 ulp (the OpenCL full-profile limit, which the device library meets):
a relative error of at most 6u for exp, an absolute error of at most 6u |log l| for log.  Per row d and head h, with k valid edges,
nc 64-edge chunks (1 for a fixed row), z_j = el + er, x_j = e_j - max e:
  weights   the computed exp(e_j - m) carries a relative error eta <= u (2 max|z| + 2 max|x| + 6 nc): 2u|z| from el + er and the slope
            product, u|x| from the subtraction, 6u from exp, and per rescale of the online softmax (at most nc - 1) 6u plus the
            rounding of m_old - m_new, whose sum telescopes to at most max|x|.  A factor common to every weight of the row (the max,
            a rescale) cancels in the normalisation.
  forward   |out - ref| <= (2 eta + gamma(k + nc) + gamma(6 + 2 nc) + 2u) sum_j a_j |feat_j|: the weights enter numerator and
            denominator; the numerator sums k products and is rescaled at most nc - 1 times; the denominator is a 6-level tree per
            chunk plus nc sequential adds and nc - 1 rescales; then 1 / l and the product.  A row without a valid edge is exactly 0.
  backward  a_j = exp(e_j - lse) has relative error eta_b <= eta + gamma(6 + 2 nc) + u (4 max|z| + |m| + 8 log k + max|x| + 6)
            (the weight and sum errors of lse, log, the roundings of m + log l and of e_j - lse, exp, the perturbed scores).  A dot
            product of a head's D floats is summed in at most P = ceil(D / 64) + 8 levels (product, 6-step lane scan, one LDS add per
            64-float pass): gamma(P) sum |g f|.  <g, out> also carries out's forward bound.  t_j = a_j (dot_j - <g, out>) k_j:
            |dt_j| <= k_j (a_j (d dot_j + d <g, out>) + |a_j (dot_j - <g, out>)| (eta_b + 3u)).
            grad_feat[s]: sum over its K_s contributions of a_j g, atomics in any order: (eta_b + u + gamma(K_s)) sum a_j |g|.
            grad_el[s]: sum |dt_j| + gamma(K_s) sum |t_j|.  grad_er[d]: sum |dt_j| + gamma(6 + nc) sum |t_j|.
  lse       m + log l, the output the backward reads: eta from the weights, gamma(6 + 2 nc) from l's sum, 6u log k from log, u (|m| + log k)
            from the addition and one more u: eta + gamma(6 + 2 nc) + u (|m| + 8 log k + 1), the form of tests/_dot_gat_ref.py.  -inf on a
            row without a valid edge."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = np.float32(-7.25e33)
GUARD = 67
SLOPE = np.float32(0.2)


def _gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


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


def reference(rows, srcs, n_dst, n_src, nc, el, er, feat, g, slope=SLOPE):
    """float64 values and bounds (module docstring).  rows / srcs: the valid edges (int64), in row order; nc: chunks per row."""
    import torch
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
    H, D = feat.shape[1], feat.shape[2]
    r, s = torch.from_numpy(rows), torch.from_numpy(srcs)
    el64, er64, f64, g64 = T(el), T(er), T(feat), T(g)
    sl = float(slope)
    z = el64[s] + er64[r]
    e = torch.where(z > 0, z, z * sl)
    kf = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, sl))
    rh = r.unsqueeze(1).expand(-1, H)
    m = torch.full((n_dst, H), float("-inf"), dtype=torch.float64).scatter_reduce(0, rh, e, "amax")
    x = e - m[r]
    p = torch.exp(x)
    l = torch.zeros((n_dst, H), dtype=torch.float64).index_add_(0, r, p)
    a = p / l[r]
    fs = f64[s]
    out = torch.zeros((n_dst, H, D), dtype=torch.float64).index_add_(0, r, a.unsqueeze(-1) * fs)
    absout = torch.zeros_like(out).index_add_(0, r, a.unsqueeze(-1) * fs.abs())
    absf = torch.zeros_like(out).index_add_(0, r, fs.abs())
    k = torch.bincount(r, minlength=n_dst).to(torch.float64).unsqueeze(1)
    ncr = torch.from_numpy(np.asarray(nc, dtype=np.float64)).unsqueeze(1)
    zero = torch.zeros((n_dst, H), dtype=torch.float64)
    maxz = zero.scatter_reduce(0, rh, z.abs(), "amax")
    maxx = zero.scatter_reduce(0, rh, x.abs(), "amax")
    g_ = lambda n: torch.from_numpy(_gamma(n.numpy()))    # noqa: E731
    eta = U * (2 * maxz + 2 * maxx + 6 * ncr)
    b_out = 1.01 * ((2 * eta + g_(k + ncr) + g_(6 + 2 * ncr) + 2 * U).unsqueeze(-1) * absout + 2.0 ** -100 * absf)
    mm = torch.where(torch.isfinite(m), m, zero)
    logk = torch.log(k.clamp_min(1))
    lse = torch.where(k > 0, mm + torch.log(l.clamp_min(1e-300)), torch.full_like(l, float("-inf")))
    b_lse = 1.01 * (eta + g_(6 + 2 * ncr) + U * (mm.abs() + 8 * logk + 1)) + 2.0 ** -100
    # backward
    eta_b = eta + g_(6 + 2 * ncr) + U * (4 * maxz + mm.abs() + 8 * torch.log(k.clamp_min(1)) + maxx + 6)
    P = -(-D // 64) + 8
    gE = g64[r]
    dot = (gE * fs).sum(-1)
    absdot = (gE * fs).abs().sum(-1)
    dout = (g64 * out).sum(-1)
    ddout = float(_gamma(P)) * (g64 * out).abs().sum(-1) + (g64.abs() * b_out).sum(-1)
    t = a * (dot - dout[r]) * kf
    dt = kf * (a * (float(_gamma(P)) * absdot + ddout[r]) + (a * (dot - dout[r])).abs() * (eta_b[r] + 3 * U))
    Ks = torch.bincount(s, minlength=n_src).to(torch.float64)
    gKs = g_(Ks)[s].unsqueeze(1)
    gf = torch.zeros((n_src, H, D), dtype=torch.float64).index_add_(0, s, a.unsqueeze(-1) * gE)
    b_gf = 1.01 * torch.zeros_like(gf).index_add_(0, s, ((eta_b[r] + U + gKs) * a).unsqueeze(-1) * gE.abs()
                                                  + 2.0 ** -100 * gE.abs())
    gel = torch.zeros((n_src, H), dtype=torch.float64).index_add_(0, s, t)
    b_el = 1.01 * torch.zeros_like(gel).index_add_(0, s, dt + gKs * t.abs()) + 2.0 ** -100
    ger = zero.clone().index_add_(0, r, t)
    b_er = 1.01 * zero.clone().index_add_(0, r, dt + g_(6 + ncr)[r] * t.abs()) + 2.0 ** -100
    return dict(out=(out.numpy(), b_out.numpy()), gf=(gf.numpy(), b_gf.numpy()), gel=(gel.numpy(), b_el.numpy()),
                ger=(ger.numpy(), b_er.numpy()), lse=(lse.numpy(), b_lse.numpy()), empty=(k.squeeze(1) == 0).numpy())


def _check(name, got, ref_bound):
    ref, bound = ref_bound
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bound)
    if err.size:
        print(f"{name}: largest error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} elements past the bound; at {i}: got {got[i]!r} want {ref[i]!r} bound {bound[i]!r}")


def _inputs(rng, n_src, n_dst, H, D, big):
    el = rng.standard_normal((n_src, H)).astype(np.float32)
    er = rng.standard_normal((n_dst, H)).astype(np.float32)
    if big:
        el *= np.float32(1e3)
        er *= np.float32(1e3)
    feat = rng.standard_normal((n_src, H, D)).astype(np.float32)
    g = rng.standard_normal((n_dst, H, D)).astype(np.float32)
    return el, er, feat, g


def _fixed_nbr(rng, n_dst, f, n_src):
    nbr = rng.integers(0, n_src, size=(n_dst, f)).astype(np.int32)
    nbr[rng.random((n_dst, f)) < 0.25] = -1
    rep = rng.random(n_dst) < 0.15
    nbr[rep, f - 1] = nbr[rep, 0]
    if n_dst:
        nbr[rng.random(n_dst) < 0.05] = -1
        nbr[0] = -1
    return nbr


def _run(torch, L, form, graph, n_dst, n_src, el, er, feat, g, off):
    """Forward and backward through the C ABI, every float buffer at float offset `off`, sentinels around every output."""
    from COALA_GNN_Pybind import _capi, current_stream
    H, D = feat.shape[1], feat.shape[2]
    bufs = {k: _device(torch, v, off) for k, v in dict(el=el, er=er, feat=feat, g=g).items()}
    o_buf, o = _device(torch, np.empty((n_dst, H, D), np.float32), off, fill=float(SENTINEL))
    s_buf, lse = _device(torch, np.empty((n_dst, H), np.float32), off, fill=float(SENTINEL))
    gf_buf, gf = _device(torch, np.empty((n_src, H, D), np.float32), off, fill=0.0)
    gl_buf, gl = _device(torch, np.empty((n_src, H), np.float32), off, fill=0.0)
    ge_buf, ge = _device(torch, np.empty((n_dst, H), np.float32), off, fill=float(SENTINEL))
    p = {k: v[1] for k, v in bufs.items()}
    st = current_stream()
    if form == "fixed":
        nbr = graph
        dn = torch.from_numpy(nbr).cuda()
        f = nbr.shape[1]
        _capi.check(L.coala_block_gat_aggregate(0, dn.data_ptr(), p["el"], p["er"], p["feat"], o, lse, n_dst, f, H, D, float(SLOPE), st))
        _capi.check(L.coala_block_gat_aggregate_backward(0, dn.data_ptr(), p["el"], p["er"], p["feat"], o, lse, p["g"], gf, gl, ge, n_dst, f,
                                                         H, D, float(SLOPE), st))
    else:
        indptr, indices = graph
        dp = torch.from_numpy(indptr).cuda()
        di = torch.from_numpy(np.append(indices, np.int32(-1))).cuda()   # one word past the edges: a block without edges has a buffer
        _capi.check(L.coala_block_gat_aggregate_csr(0, dp.data_ptr(), di.data_ptr(), p["el"], p["er"], p["feat"], o, lse, n_dst, H, D,
                                                    float(SLOPE), st))
        _capi.check(L.coala_block_gat_aggregate_csr_backward(0, dp.data_ptr(), di.data_ptr(), p["el"], p["er"], p["feat"], o, lse, p["g"], gf,
                                                             gl, ge, n_dst, H, D, float(SLOPE), st))
    torch.cuda.synchronize()
    res = dict(out=_region(o_buf, off, (n_dst, H, D)), lse=_region(s_buf, off, (n_dst, H)), gf=_region(gf_buf, off, (n_src, H, D)),
               gel=_region(gl_buf, off, (n_src, H)), ger=_region(ge_buf, off, (n_dst, H)))
    for k, v in dict(el=el, er=er, feat=feat, g=g).items():                       # inputs untouched
        assert np.array_equal(_region(bufs[k][0], off, v.shape), v)
    return res


def _edges_fixed(nbr):
    rows, cols = np.nonzero(nbr >= 0)
    return rows.astype(np.int64), nbr[rows, cols].astype(np.int64), np.ones(nbr.shape[0])


def _edges_csr(indptr, indices):
    deg = np.diff(indptr)
    return np.repeat(np.arange(len(deg)), deg).astype(np.int64), indices.astype(np.int64), -(-deg // 64)


def _check_all(got, ref):
    for k in ("out", "gf", "gel", "ger"):
        _check(k, got[k], ref[k])
    if "lse" in got:                                                # the direct calls' output; autograd hands none out
        full = ~ref["empty"]
        _check("lse", got["lse"][full], (ref["lse"][0][full], ref["lse"][1][full]))
        assert np.all(np.isneginf(got["lse"][ref["empty"]])), "lse of a row without a valid edge is not -inf"
    assert np.all(got["out"][ref["empty"]] == 0.0), "a row without a valid edge is not exactly 0"
    assert np.isfinite(got["out"]).all() and np.isfinite(got["gf"]).all() and np.isfinite(got["gel"]).all() and np.isfinite(got["ger"]).all()


DIMS = [1, 3, 16, 64, 65, 128, 256]
HEADS = [1, 2, 4, 8]
FANS = [1, 2, 3, 5, 7, 8, 15, 16, 17, 24, 31, 32]
CASES = [(300 if H * D <= 512 else 90, FANS[(i * 4 + j) % len(FANS)], H, D, (i + j) % 2, (i + j) % 3 == 0)
         for i, D in enumerate(DIMS) for j, H in enumerate(HEADS)]
CASES += [(100_003, 32, 1, 3, 0, False), (100_003, 9, 1, 4, 1, True), (32_769, 31, 4, 16, 0, False), (0, 4, 2, 8, 0, False),
          (1, 1, 1, 1, 1, False), (2, 32, 8, 4, 0, True)]


@pytest.mark.parametrize("n_dst,f,H,D,off,big", CASES)
def test_gat_fixed_against_float64(hiplib, n_dst, f, H, D, off, big):
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(n_dst * 7 + f * 131 + H * 17 + D + off)
    n_src = max(64, min(5000, n_dst // 4))
    nbr = _fixed_nbr(rng, n_dst, f, n_src - 7)       # the last 7 sources are never referenced
    el, er, feat, g = _inputs(rng, n_src, n_dst, H, D, big)
    got = _run(torch, L, "fixed", nbr, n_dst, n_src, el, er, feat, g, off)
    rows, srcs, nc = _edges_fixed(nbr)
    ref = reference(rows, srcs, n_dst, n_src, nc, el, er, feat, g)
    _check_all(got, ref)
    assert np.all(got["gf"][n_src - 7:] == 0.0) and np.all(got["gel"][n_src - 7:] == 0.0)


CSR_CASES = [(n, f, H, D, off, big) for (n, f, H, D, off, big) in CASES if 0 < n <= 300]
CSR_CASES += [(100_003, 12, 1, 3, 1, False), (0, 1, 1, 4, 0, False)]


@pytest.mark.parametrize("n_dst,f,H,D,off,big", CSR_CASES)
def test_gat_csr_against_float64(hiplib, n_dst, f, H, D, off, big):
    """Degrees 0..2f, some rows of 65..200 edges (two to four chunks, the online rescale)."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(n_dst * 5 + f * 31 + H * 3 + D + off)
    n_src = max(64, min(5000, n_dst // 4))
    deg = rng.integers(0, 2 * f + 1, size=n_dst)
    if n_dst:
        deg[rng.random(n_dst) < 0.05] = rng.integers(65, 200)
        deg[0] = 0
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rng.integers(0, n_src, size=int(indptr[-1])).astype(np.int32)
    el, er, feat, g = _inputs(rng, n_src, n_dst, H, D, big)
    got = _run(torch, L, "csr", (indptr, indices), n_dst, n_src, el, er, feat, g, off)
    _check_all(got, reference(*_edges_csr(indptr, indices)[:2], n_dst, n_src, _edges_csr(indptr, indices)[2], el, er, feat, g))


@pytest.mark.parametrize("big", [False, True])
def test_gat_csr_hub_against_float64(hiplib, big):
    """One row of 1,000,003 in-edges (15,626 chunks of the online softmax) between small rows, at H * D = 4."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(99 + big)
    n_src, H, D = 3000, 2, 2
    deg = rng.integers(0, 9, size=41)
    deg[20] = 1_000_003
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rng.integers(0, n_src, size=int(indptr[-1])).astype(np.int32)
    el, er, feat, g = _inputs(rng, n_src, len(deg), H, D, big)
    got = _run(torch, L, "csr", (indptr, indices), len(deg), n_src, el, er, feat, g, 0)
    rows, srcs, nc = _edges_csr(indptr, indices)
    _check_all(got, reference(rows, srcs, len(deg), n_src, nc, el, er, feat, g))


@pytest.mark.parametrize("f,H,D,off,big", [(5, 4, 16, 0, False), (32, 2, 65, 1, True), (17, 8, 3, 0, True), (1, 1, 64, 1, False)])
def test_gat_fixed_and_csr_give_identical_bits(hiplib, f, H, D, off, big):
    """Fixed rows whose valid entries come first (the sampler's layout) against the same rows in CSR form: out, lse and grad_er bit
    for bit."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(f * 11 + H + D + off)
    n_dst, n_src = 2000, 700
    deg = rng.integers(0, f + 1, size=n_dst)
    deg[:3] = [0, f, 1]
    nbr = np.full((n_dst, f), -1, np.int32)
    for d in range(n_dst):
        nbr[d, :deg[d]] = rng.integers(0, n_src, size=deg[d])
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = nbr[nbr >= 0].astype(np.int32)
    el, er, feat, g = _inputs(rng, n_src, n_dst, H, D, big)
    a = _run(torch, L, "fixed", nbr, n_dst, n_src, el, er, feat, g, off)
    b = _run(torch, L, "csr", (indptr, indices), n_dst, n_src, el, er, feat, g, off)
    for k in ("out", "lse", "ger"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{k} differs between the fixed and the CSR kernels"


def test_gat_refuses_bad_shapes(hiplib):
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    st = current_stream()
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    i64 = torch.zeros(65, dtype=torch.int64, device="cuda")
    a = torch.zeros(4096, device="cuda")
    b = torch.full((4096,), float(SENTINEL), device="cuda")
    A, B = a.data_ptr(), b.data_ptr()
    fixed_bad = ((1, 0, 2, 4), (1, 33, 2, 4), (1, 4, 0, 4), (1, 4, 17, 4), (1, 4, 2, 0), (-1, 4, 2, 4), (0, 33, 2, 4))
    for n, f, H, D in fixed_bad:
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_gat_aggregate(0, i32.data_ptr(), A, A, A, B, B, n, f, H, D, 0.2, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_gat_aggregate_backward(0, i32.data_ptr(), A, A, A, A, A, A, B, B, B, n, f, H, D, 0.2, st))
    for n, H, D in ((1, 0, 4), (1, 17, 4), (1, 2, 0), (-1, 2, 4)):
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_gat_aggregate_csr(0, i64.data_ptr(), i32.data_ptr(), A, A, A, B, B, n, H, D, 0.2, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_gat_aggregate_csr_backward(0, i64.data_ptr(), i32.data_ptr(), A, A, A, A, A, A, B, B, B, n, H, D, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_gat_aggregate(0, i32.data_ptr(), A, None, A, B, B, 1, 4, 2, 4, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_gat_aggregate_backward(0, i32.data_ptr(), A, A, A, A, A, A, B, None, B, 1, 4, 2, 4, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_gat_aggregate_csr(0, None, i32.data_ptr(), A, A, A, B, B, 1, 2, 4, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_gat_aggregate_csr_backward(0, i64.data_ptr(), None, A, A, A, A, A, A, B, B, B, 1, 2, 4, 0.2, st))
    torch.cuda.synchronize()
    assert torch.all(b == float(SENTINEL))


@pytest.mark.parametrize("form", ["fixed", "csr"])
def test_block_gat_aggregate_autograd_matches_direct_calls(hiplib, form):
    """Block.gat_aggregate with autograd: the forward and grad_er bit for bit equal to the direct kernel calls, and every
    gradient (grad_feat, grad_el: float atomics in any order) within the float64 bounds."""
    import torch
    from COALA_GNN.sampler import Block
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(5 if form == "fixed" else 6)
    n_dst, n_src, H, D = 1500, 600, 4, 32
    el, er, feat, g = _inputs(rng, n_src, n_dst, H, D, False)
    if form == "fixed":
        graph = _fixed_nbr(rng, n_dst, 10, n_src)
        b = Block(torch.arange(n_src, device="cuda"), torch.from_numpy(graph).cuda(), n_dst)
        rows, srcs, nc = _edges_fixed(graph)
    else:
        deg = rng.integers(0, 90, size=n_dst)
        indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        graph = (indptr, rng.integers(0, n_src, size=int(indptr[-1])).astype(np.int32))
        b = Block(torch.arange(n_src, device="cuda"), None, n_dst, indptr=torch.from_numpy(graph[0]).cuda(),
                  indices=torch.from_numpy(graph[1]).cuda())
        rows, srcs, nc = _edges_csr(*graph)
    t = [torch.from_numpy(x).cuda().requires_grad_(True) for x in (el, er, feat)]
    out = b.gat_aggregate(*t, negative_slope=float(SLOPE))
    (out * torch.from_numpy(g).cuda()).sum().backward()
    direct = _run(torch, L, form, graph, n_dst, n_src, el, er, feat, g, 0)
    assert np.array_equal(out.detach().cpu().numpy().view(np.int32), direct["out"].view(np.int32))
    assert np.array_equal(t[1].grad.cpu().numpy().view(np.int32), direct["ger"].view(np.int32))
    got = dict(out=out.detach().cpu().numpy(), gf=t[2].grad.cpu().numpy(), gel=t[0].grad.cpu().numpy(), ger=t[1].grad.cpu().numpy())
    _check_all(got, reference(rows, srcs, n_dst, n_src, nc, el, er, feat, g))


@pytest.mark.parametrize("fanouts", [[5, 5], [-1, -1]])
def test_sampled_blocks_native_agrees_with_fallback(hiplib, fanouts):
    """Blocks from the sampler ([5, 5] fixed, [-1, -1] ragged): native forward and backward against the float64 fallback
    (Block.gat_aggregate_torch on CPU float64 tensors), within the bounds."""
    import torch
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import powerlaw_csc
    indptr, indices = powerlaw_csc(20000, 8.0, seed=3, device="cuda")
    sampler = NeighborSampler(fanouts, seed=1)
    g = sampler.make_graph(indptr, indices)
    _, _, blocks = sampler.sample(g, torch.randperm(20000, device="cuda")[:256])
    rng = np.random.default_rng(len(fanouts) + fanouts[0])
    H, D = 4, 16
    for b in blocks:
        el, er, feat, gr = _inputs(rng, b.num_src, b.num_dst, H, D, False)
        t = [torch.from_numpy(x).cuda().requires_grad_(True) for x in (el, er, feat)]
        out = b.gat_aggregate(*t)
        (out * torch.from_numpy(gr).cuda()).sum().backward()
        t64 = [torch.from_numpy(x.astype(np.float64)).requires_grad_(True) for x in (el, er, feat)]
        cpu = type(b)(b.src_nodes.cpu(), None if b.nbr is None else b.nbr.cpu(), b.num_dst,
                      indptr=None if b.indptr is None else b.indptr.cpu(), indices=None if b.indices is None else b.indices.cpu())
        ref_out = cpu.gat_aggregate_torch(*t64, negative_slope=float(SLOPE))
        (ref_out * torch.from_numpy(gr.astype(np.float64))).sum().backward()
        if b.nbr is None:
            rows, srcs, nc = _edges_csr(b.indptr.cpu().numpy(), b.indices.cpu().numpy())
        else:
            rows, srcs, nc = _edges_fixed(b.nbr.cpu().numpy())
        ref = reference(rows, srcs, b.num_dst, b.num_src, nc, el, er, feat, gr)
        assert np.allclose(ref_out.detach().numpy(), ref["out"][0], rtol=1e-12, atol=1e-12)       # the fallback is the reference
        assert np.allclose(t64[2].grad.numpy(), ref["gf"][0], rtol=1e-10, atol=1e-10)
        got = dict(out=out.detach().cpu().numpy(), gf=t[2].grad.cpu().numpy(), gel=t[0].grad.cpu().numpy(), ger=t[1].grad.cpu().numpy())
        _check_all(got, ref)
