"""GPU tests of the relation-typed GAT attention kernels (coala_block_rel_gat_aggregate[_csr][_backward] in coala_block_ops.hip)
against float64.

Called through the C ABI on hand-made blocks: n_dst 1, 5, 257; fan-outs 1, 7, 32 with -1 anywhere; CSR rows of degree 0, 1, 63, 64,
65 and 200; heads 1, 4, 16; D in {1, 3, 64, 65}, the 16-byte path and the scalar path (D % 4 != 0, or buffers one float off 16-byte
alignment); 1, 3, 16 and 64 relations with R * H <= 256; rows whose types are sorted, as RelNeighborSampler gives them, and rows whose
types are interleaved; a row whose 64 slots are 64 different relations; a relation present only in a row's second chunk; rows without
a valid edge; types outside [0, R); scores up to +-1e3.  Every output is followed by sentinel guard words.

Bounds.  First order in u = 2^-24 (fp32 unit roundoff), gamma(n) = n u / (1 - n u); each bound is multiplied by 1.01 for the
second-order terms (every relative term below stays under 1e-2) and gets an absolute 2^-100 times the magnitude it scales, for
weights that underflow.  exp and log are taken to be within 3 ulp (a relative error of at most 6u for exp, an absolute error of at
most 6u |log l| for log), 1 / l within 3u.  A group is the k edges of one (destination d, relation r), per head; its row has K valid
edges of any relation in nc 64-slot chunks (1 for a fixed row); z_j = el + er, x_j = e_j - max e over the group.
  scores    e_j carries an absolute error of 2u |z_j|: el + er, then the slope product.
  forward   the kernel's first pass keeps the group's max m and sum l online: a term of l is exp(e - m_chunk), rescaled by
            exp(m_old - m_new) at most nc - 1 times -- a relative error of u (2 max|z| + max|x| + 7 nc) (the roundings of the
            differences telescope to max|x|; 6u per exp and u per product) -- summed by a 6-level tree per chunk and one add per
            chunk: gamma(6 + nc).  The second pass takes a_j = exp(e_j - m) (1 / l): u (2 max|z| + max|x| + 6) for the numerator,
            3u + u for the reciprocal and the product.  The error of m itself is common to numerator and denominator and cancels.
            out sums the K products a_j feat_j of the whole row in slot order, one product and one add each (or one fma):
            gamma(K + 1).  So  |out - ref| <= sum_j c_j a_j |feat_j|,  c_j = u (4 max|z| + 2 max|x| + 7 nc + 10) + gamma(6 + nc) +
            gamma(K + 1)  with its group's maxima.  A row without a valid edge is exactly 0.
  lse       m + log l: 2u max|z| (the scores) + the relative error of l + 6u log k + u |lse|.
  backward  a_j = exp(e_j - lse) has relative error eta_b <= u (4 max|z| + 2 max|x| + 7 nc + |m| + 8 log k + 6) + gamma(6 + nc) (the
            score, lse's errors above with |lse| <= |m| + log k, the rounding of e_j - lse, exp).  A dot product of a head's D floats is
            summed in at most P = ceil(D / 64) + 8 levels (product, 6-step lane scan, one LDS add per 64-float pass): d dot_j =
            gamma(P) sum |g f|.  G = sum over the group of a_j dot_j is a product, a 6-level tree per chunk and an add per chunk:
            dG <= sum_j a_j d dot_j + (eta_b + u + gamma(6 + nc)) sum_j |a_j dot_j|.  t_j = a_j (dot_j - G) k_j:
            |dt_j| <= k_j (a_j (d dot_j + dG) + |a_j (dot_j - G)| (eta_b + 3u)).  (The kernel subtracts G / S, S = sum of the group's
            a_j: that removes the part of eta_b common to the group from dG, and is held to the bound as derived without it.)
            grad_feat[p]: sum over its K_p contributions of a_j g, atomics in any order: (eta_b + u + gamma(K_p)) sum a_j |g|.
            grad_el[p]: sum |dt_j| + gamma(K_p) sum |t_j|.  grad_er[d, r]: sum |dt_j| + gamma(6 + nc) sum |t_j|."""
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


def reference(dst, row, typ, n_dst, P, R, nc, el, er, feat, g, slope=SLOPE):
    """float64 values and bounds (module docstring).  dst / row / typ: the valid edges with a type in range (int64), in slot order; nc:
    chunks per destination row."""
    import torch
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
    H, D = feat.shape[1], feat.shape[2]
    d, s, key = torch.from_numpy(dst), torch.from_numpy(row), torch.from_numpy(dst * R + typ)
    el64, er64, f64, g64 = T(el), T(er).reshape(n_dst * R, H), T(feat), T(g)
    sl = float(slope)
    z = el64[s] + er64[key]
    e = torch.where(z > 0, z, z * sl)
    kf = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, sl))
    kh = key.unsqueeze(1).expand(-1, H)
    zero = torch.zeros((n_dst * R, H), dtype=torch.float64)
    m = torch.full((n_dst * R, H), float("-inf"), dtype=torch.float64).scatter_reduce(0, kh, e, "amax")
    x = e - m[key]
    p = torch.exp(x)
    l = zero.clone().index_add_(0, key, p)
    a = p / l[key]
    lse = m + torch.log(l)
    fs = f64[s]
    out = torch.zeros((n_dst, H, D), dtype=torch.float64).index_add_(0, d, a.unsqueeze(-1) * fs)
    k = torch.bincount(key, minlength=n_dst * R).to(torch.float64).unsqueeze(1)
    K = torch.bincount(d, minlength=n_dst).to(torch.float64)
    ncr = torch.from_numpy(np.asarray(nc, dtype=np.float64))
    ncg = ncr.repeat_interleave(R).unsqueeze(1)                                  # per group
    maxz = zero.scatter_reduce(0, kh, z.abs(), "amax")
    maxx = zero.scatter_reduce(0, kh, x.abs(), "amax")
    g_ = lambda n: torch.from_numpy(_gamma(n.numpy()))    # noqa: E731
    cf = U * (4 * maxz + 2 * maxx + 7 * ncg + 10) + g_(6 + ncg) + g_(K + 1).repeat_interleave(R).unsqueeze(1)
    absf = torch.zeros_like(out).index_add_(0, d, fs.abs())
    b_out = 1.01 * (torch.zeros_like(out).index_add_(0, d, (cf[key] * a).unsqueeze(-1) * fs.abs()) + 2.0 ** -100 * absf)
    logk = torch.log(k.clamp_min(1))
    mm = torch.where(torch.isfinite(m), m, zero)
    b_lse = 1.01 * (U * (4 * maxz + maxx + 7 * ncg + 6 * logk + mm.abs() + logk) + g_(6 + ncg)) + 2.0 ** -100
    # backward
    eta_b = U * (4 * maxz + 2 * maxx + 7 * ncg + mm.abs() + 8 * logk + 6) + g_(6 + ncg)
    Pl = float(_gamma(-(-D // 64) + 8))
    gE = g64[d]
    dot = (gE * fs).sum(-1)
    ddot = Pl * (gE * fs).abs().sum(-1)
    G = zero.clone().index_add_(0, key, a * dot)
    dG = zero.clone().index_add_(0, key, a * ddot + (eta_b[key] + U + g_(6 + ncg)[key]) * (a * dot).abs())
    t = a * (dot - G[key]) * kf
    dt = kf * (a * (ddot + dG[key]) + (a * (dot - G[key])).abs() * (eta_b[key] + 3 * U))
    Ks = torch.bincount(s, minlength=P).to(torch.float64)
    gKs = g_(Ks)[s].unsqueeze(1)
    gf = torch.zeros((P, H, D), dtype=torch.float64).index_add_(0, s, a.unsqueeze(-1) * gE)
    b_gf = 1.01 * torch.zeros_like(gf).index_add_(0, s, ((eta_b[key] + U + gKs) * a).unsqueeze(-1) * gE.abs() + 2.0 ** -100 * gE.abs())
    gel = torch.zeros((P, H), dtype=torch.float64).index_add_(0, s, t)
    b_el = 1.01 * torch.zeros_like(gel).index_add_(0, s, dt + gKs * t.abs()) + 2.0 ** -100
    ger = zero.clone().index_add_(0, key, t)
    b_er = 1.01 * zero.clone().index_add_(0, key, dt + g_(6 + ncg)[key] * t.abs()) + 2.0 ** -100
    shape = (n_dst, R, H)
    return dict(out=(out.numpy(), b_out.numpy()), gf=(gf.numpy(), b_gf.numpy()), gel=(gel.numpy(), b_el.numpy()),
                ger=(ger.view(shape).numpy(), b_er.view(shape).numpy()), lse=(lse.view(shape).numpy(), b_lse.view(shape).numpy()),
                empty=(K == 0).numpy(), absent=(k.view(n_dst, R) == 0).numpy())


def _check(name, got, ref_bound, where=None):
    ref, bound = ref_bound
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bound)
    if where is not None:
        bad &= where
    print(f"{name}: largest error / bound {np.nanmax(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0)):.3f}")
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} elements past the bound; at {i}: got {got[i]!r} want {ref[i]!r} bound {bound[i]!r}")


def _check_all(got, ref):
    for k in ("out", "gf", "gel", "ger"):
        _check(k, got[k], ref[k])
    present = ~ref["absent"][:, :, None] & np.ones(got["lse"].shape, bool)
    _check("lse", got["lse"], ref["lse"], present)
    assert np.all(np.isneginf(got["lse"][~present])), "lse is -inf where (d, r) has no edge"
    assert np.all(got["ger"][~present] == 0.0), "grad_er is 0 where (d, r) has no edge"
    assert np.all(got["out"][ref["empty"]] == 0.0), "a row without a valid edge is not exactly 0"
    assert all(np.isfinite(got[k]).all() for k in ("out", "gf", "gel", "ger"))


def _inputs(rng, P, n_dst, R, H, D, big):
    el = rng.standard_normal((P, H)).astype(np.float32)
    er = rng.standard_normal((n_dst, R, H)).astype(np.float32)
    if big:
        el *= np.float32(1e3)
        er *= np.float32(1e3)
    feat = rng.standard_normal((P, H, D)).astype(np.float32)
    g = rng.standard_normal((n_dst, H, D)).astype(np.float32)
    return el, er, feat, g


def _types(rng, shape, R, srt):
    """Random types, ~6% of them outside [0, R); srt: non-decreasing along the last axis, as RelNeighborSampler's rows are."""
    t = rng.integers(0, R, size=shape).astype(np.int32)
    if srt:
        t = np.sort(t, axis=-1)
    wild = rng.random(shape) < 0.06
    t[wild] = rng.choice(np.array([-1, R, 1000, -(2 ** 31)], dtype=np.int32), size=int(wild.sum()))
    return t


def _fixed_graph(rng, n_dst, f, P, R, srt):
    row = rng.integers(0, P, size=(n_dst, f)).astype(np.int32)
    row[rng.random((n_dst, f)) < 0.25] = -1
    rep = rng.random(n_dst) < 0.15
    row[rep, f - 1] = row[rep, 0]
    row[rng.random(n_dst) < 0.05] = -1
    if n_dst > 1:
        row[1] = -1
    return row, _types(rng, (n_dst, f), R, srt)


def _csr_graph(rng, degs, P, R, srt):
    indptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    row = rng.integers(0, P, size=int(indptr[-1])).astype(np.int32)
    row[rng.random(row.shape) < 0.05] = -1
    typ = np.concatenate([_types(rng, (int(d),), R, srt) for d in degs] + [np.zeros(0, np.int32)]).astype(np.int32)
    return indptr, row, typ


def _edges(form, graph, R):
    """-> (dst, row, typ) of the valid edges with a type in range, in slot order, and the chunks per row"""
    if form == "fixed":
        row, typ = graph
        dst = np.repeat(np.arange(row.shape[0]), row.shape[1])
        nc = np.ones(row.shape[0])
    else:
        indptr, row, typ = graph
        deg = np.diff(indptr)
        dst = np.repeat(np.arange(len(deg)), deg)
        nc = np.maximum(-(-deg // 64), 1)
    row, typ = row.reshape(-1).astype(np.int64), typ.reshape(-1).astype(np.int64)
    keep = (row >= 0) & (typ >= 0) & (typ < R)
    return dst[keep].astype(np.int64), row[keep], typ[keep], nc


def _run(torch, L, form, graph, n_dst, P, R, el, er, feat, g, off):
    """Forward and backward through the C ABI, every float buffer at float offset `off`, sentinels around every output."""
    from COALA_GNN_Pybind import _capi, current_stream
    H, D = feat.shape[1], feat.shape[2]
    ins = dict(el=el, er=er, feat=feat, g=g)
    bufs = {k: _device(torch, v, off) for k, v in ins.items()}
    o_buf, o = _device(torch, np.empty((n_dst, H, D), np.float32), off, fill=float(SENTINEL))
    s_buf, lse = _device(torch, np.empty((n_dst, R, H), np.float32), off, fill=float(SENTINEL))
    gf_buf, gf = _device(torch, np.empty((P, H, D), np.float32), off, fill=0.0)
    gl_buf, gl = _device(torch, np.empty((P, H), np.float32), off, fill=0.0)
    ge_buf, ge = _device(torch, np.empty((n_dst, R, H), np.float32), off, fill=float(SENTINEL))
    p = {k: v[1] for k, v in bufs.items()}
    st = current_stream()
    pad = lambda a: torch.from_numpy(np.append(a.reshape(-1), np.int32(-1))).cuda()   # noqa: E731  (a block without slots has a buffer)
    if form == "fixed":
        dr, dt = pad(graph[0]), pad(graph[1])
        f = graph[0].shape[1]
        _capi.check(L.coala_block_rel_gat_aggregate(0, dr.data_ptr(), dt.data_ptr(), p["el"], p["er"], p["feat"], o, lse, n_dst, f, R, H, D,
                                                    float(SLOPE), st))
        _capi.check(L.coala_block_rel_gat_aggregate_backward(0, dr.data_ptr(), dt.data_ptr(), p["el"], p["er"], p["feat"], lse, p["g"], gf, gl, ge,
                                                             n_dst, f, R, H, D, float(SLOPE), st))
    else:
        dp, dr, dt = torch.from_numpy(graph[0]).cuda(), pad(graph[1]), pad(graph[2])
        _capi.check(L.coala_block_rel_gat_aggregate_csr(0, dp.data_ptr(), dr.data_ptr(), dt.data_ptr(), p["el"], p["er"], p["feat"], o, lse,
                                                        n_dst, R, H, D, float(SLOPE), st))
        _capi.check(L.coala_block_rel_gat_aggregate_csr_backward(0, dp.data_ptr(), dr.data_ptr(), dt.data_ptr(), p["el"], p["er"], p["feat"], lse,
                                                                 p["g"], gf, gl, ge, n_dst, R, H, D, float(SLOPE), st))
    torch.cuda.synchronize()
    res = dict(out=_region(o_buf, off, (n_dst, H, D)), lse=_region(s_buf, off, (n_dst, R, H)), gf=_region(gf_buf, off, (P, H, D)),
               gel=_region(gl_buf, off, (P, H)), ger=_region(ge_buf, off, (n_dst, R, H)))
    for k, v in ins.items():                                                      # inputs untouched
        assert np.array_equal(_region(bufs[k][0], off, v.shape), v)
    return res


def _against_float64(torch, form, graph, n_dst, P, R, H, D, off, big, rng):
    from COALA_GNN_Pybind import _capi
    el, er, feat, g = _inputs(rng, P, n_dst, R, H, D, big)
    got = _run(torch, _capi.load(), form, graph, n_dst, P, R, el, er, feat, g, off)
    dst, row, typ, nc = _edges(form, graph, R)
    ref = reference(dst, row, typ, n_dst, P, R, nc, el, er, feat, g)
    _check_all(got, ref)
    assert np.all(got["gf"][P - 7:] == 0.0) and np.all(got["gel"][P - 7:] == 0.0)   # the last 7 table rows are never referenced
    return got


# n_dst, fan-out, H, D, R, float offset, big scores, sorted types
FIXED = [(1, 1, 1, 1, 1, 0, False, True), (5, 7, 4, 3, 3, 1, True, False), (257, 32, 16, 64, 16, 0, False, True),
         (257, 7, 4, 65, 64, 1, True, False), (5, 32, 1, 64, 64, 0, False, False), (257, 1, 4, 1, 3, 0, True, True),
         (5, 32, 4, 64, 3, 1, False, True)]


@pytest.mark.parametrize("n_dst,f,H,D,R,off,big,srt", FIXED)
def test_rel_gat_fixed_against_float64(hiplib, n_dst, f, H, D, R, off, big, srt):
    import torch
    rng = np.random.default_rng(n_dst * 7 + f * 131 + H * 17 + D + R * 3 + off)
    P = 71
    _against_float64(torch, "fixed", _fixed_graph(rng, n_dst, f, P - 7, R, srt), n_dst, P, R, H, D, off, big, rng)


DEGS = [0, 1, 63, 64, 65, 200]
# n_dst, H, D, R, float offset, big scores, sorted types
CSR = [(257, 4, 3, 3, 0, False, True), (257, 4, 1, 64, 1, True, False), (5, 16, 64, 16, 0, False, False), (5, 1, 65, 64, 1, True, True),
       (6, 4, 64, 1, 1, False, True), (1, 1, 65, 1, 0, True, False)]


@pytest.mark.parametrize("n_dst,H,D,R,off,big,srt", CSR)
def test_rel_gat_csr_against_float64(hiplib, n_dst, H, D, R, off, big, srt):
    """Rows of degree 0, 1, 63, 64, 65 and 200 in turn (one row: 200)."""
    import torch
    rng = np.random.default_rng(n_dst * 5 + H * 3 + D + R * 11 + off)
    degs = [200] if n_dst == 1 else [DEGS[i % len(DEGS)] for i in range(n_dst)]
    P = 71
    _against_float64(torch, "csr", _csr_graph(rng, degs, P - 7, R, srt), n_dst, P, R, H, D, off, big, rng)


@pytest.mark.parametrize("big", [False, True])
def test_rel_gat_csr_chunk_corner_rows(hiplib, big):
    """R = 64, H = 4: a row whose 64 slots are 64 different relations; a row of 130 slots where relation 5 appears only in the second
    chunk and relation 9 only in the third; a row of 64 slots of one relation; a row whose every slot is padding or out of range."""
    import torch
    rng = np.random.default_rng(40 + big)
    R, H, D, P = 64, 4, 3, 71
    t1 = rng.integers(10, 20, size=130).astype(np.int32)
    t1[70], t1[100], t1[129] = 5, 5, 9
    types = [rng.permutation(64).astype(np.int32), t1, np.full(64, 63, np.int32), np.array([-1, R, 1000, 3], np.int32), np.zeros(0, np.int32)]
    degs = [len(t) for t in types]
    indptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    row = rng.integers(0, P - 7, size=int(indptr[-1])).astype(np.int32)
    row[indptr[3] + 3] = -1
    got = _against_float64(torch, "csr", (indptr, row, np.concatenate(types)), len(degs), P, R, H, D, 0, big, rng)
    assert np.isfinite(got["lse"][0]).all() and np.isfinite(got["lse"][1, [5, 9]]).all() and np.all(np.isneginf(got["lse"][3:]))


@pytest.mark.parametrize("f,H,D,R,off,big,srt", [(5, 4, 16, 3, 0, False, True), (32, 2, 65, 64, 1, True, False), (7, 16, 3, 16, 0, True, False),
                                                 (1, 1, 64, 1, 1, False, True)])
def test_rel_gat_fixed_and_csr_give_identical_bits(hiplib, f, H, D, R, off, big, srt):
    """Fixed rows whose valid entries come first (the sampler's layout) against the same rows in CSR form -- out, lse and grad_er bit for
    bit -- and a second call of each against the first."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(f * 11 + H + D + off)
    n_dst, P = 300, 64
    deg = rng.integers(0, f + 1, size=n_dst)
    deg[:3] = [0, f, 1]
    row = np.full((n_dst, f), -1, np.int32)
    for d in range(n_dst):
        row[d, :deg[d]] = rng.integers(0, P, size=deg[d])
    typ = _types(rng, (n_dst, f), R, srt)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    valid = row >= 0
    el, er, feat, g = _inputs(rng, P, n_dst, R, H, D, big)
    a = _run(torch, L, "fixed", (row, typ), n_dst, P, R, el, er, feat, g, off)
    b = _run(torch, L, "csr", (indptr, row[valid], typ[valid]), n_dst, P, R, el, er, feat, g, off)
    a2 = _run(torch, L, "fixed", (row, typ), n_dst, P, R, el, er, feat, g, off)
    b2 = _run(torch, L, "csr", (indptr, row[valid], typ[valid]), n_dst, P, R, el, er, feat, g, off)
    for k in ("out", "lse", "ger"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{k} differs between the fixed and the CSR kernels"
        assert np.array_equal(a[k].view(np.int32), a2[k].view(np.int32)), f"{k} differs between two calls (fixed)"
        assert np.array_equal(b[k].view(np.int32), b2[k].view(np.int32)), f"{k} differs between two calls (CSR)"


def test_rel_gat_long_rows_are_reproducible(hiplib):
    """Rows of several chunks, interleaved types: out, lse and grad_er bit for bit from call to call."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(77)
    R, H, D, P = 16, 4, 16, 64
    graph = _csr_graph(rng, [200, 65, 0, 129, 64], P, R, False)
    el, er, feat, g = _inputs(rng, P, 5, R, H, D, False)
    a = _run(torch, L, "csr", graph, 5, P, R, el, er, feat, g, 0)
    b = _run(torch, L, "csr", graph, 5, P, R, el, er, feat, g, 0)
    for k in ("out", "lse", "ger"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def test_rel_gat_refuses_bad_shapes(hiplib):
    """Shapes outside the native limits get an error code, not a launch; n_dst == 0 succeeds and reads no pointer."""
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    st = current_stream()
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    i64 = torch.zeros(65, dtype=torch.int64, device="cuda")
    a = torch.zeros(4096, device="cuda")
    b = torch.full((4096,), float(SENTINEL), device="cuda")
    A, B, I, P = a.data_ptr(), b.data_ptr(), i32.data_ptr(), i64.data_ptr()
    # n_dst, fan-out, R, H, D
    bad = ((1, 0, 2, 2, 4), (1, 33, 2, 2, 4), (1, 4, 0, 2, 4), (1, 4, 65, 2, 4), (1, 4, 2, 0, 4), (1, 4, 2, 17, 4), (1, 4, 2, 2, 0),
           (-1, 4, 2, 2, 4), (1, 4, 17, 16, 4), (1, 4, 64, 5, 4), (0, 33, 2, 2, 4), (0, 4, 33, 8, 4))
    for n, f, R, H, D in bad:
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_rel_gat_aggregate(0, I, I, A, A, A, B, B, n, f, R, H, D, 0.2, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_rel_gat_aggregate_backward(0, I, I, A, A, A, A, A, B, B, B, n, f, R, H, D, 0.2, st))
        if 1 <= f <= 32:
            with pytest.raises(RuntimeError, match="bad block shape"):
                _capi.check(L.coala_block_rel_gat_aggregate_csr(0, P, I, I, A, A, A, B, B, n, R, H, D, 0.2, st))
            with pytest.raises(RuntimeError, match="bad block shape"):
                _capi.check(L.coala_block_rel_gat_aggregate_csr_backward(0, P, I, I, A, A, A, A, A, B, B, B, n, R, H, D, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_rel_gat_aggregate(0, I, None, A, A, A, B, B, 1, 4, 2, 2, 4, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_rel_gat_aggregate_backward(0, I, I, A, A, A, None, A, B, B, B, 1, 4, 2, 2, 4, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_rel_gat_aggregate_csr(0, None, I, I, A, A, A, B, B, 1, 2, 2, 4, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_rel_gat_aggregate_csr_backward(0, P, I, I, A, A, A, A, A, B, B, None, 1, 2, 2, 4, 0.2, st))
    _capi.check(L.coala_block_rel_gat_aggregate(0, None, None, None, None, None, None, None, 0, 4, 2, 2, 4, 0.2, st))
    _capi.check(L.coala_block_rel_gat_aggregate_backward(0, None, None, None, None, None, None, None, None, None, None, 0, 4, 2, 2, 4, 0.2, st))
    _capi.check(L.coala_block_rel_gat_aggregate_csr(0, None, None, None, None, None, None, None, None, 0, 2, 2, 4, 0.2, st))
    _capi.check(L.coala_block_rel_gat_aggregate_csr_backward(0, None, None, None, None, None, None, None, None, None, None, None, 0, 2, 2, 4,
                                                             0.2, st))
    torch.cuda.synchronize()
    assert torch.all(b == float(SENTINEL))


def _block(torch, form, graph, n_src, device="cuda"):
    from COALA_GNN.sampler import Block
    src = torch.arange(n_src, device=device)
    if form == "fixed":
        return Block(src, torch.from_numpy(graph[0]).to(device), graph[0].shape[0])
    return Block(src, None, len(graph[0]) - 1, indptr=torch.from_numpy(graph[0]).to(device), indices=torch.from_numpy(graph[1]).to(device))


@pytest.mark.parametrize("form", ["fixed", "csr"])
@pytest.mark.parametrize("packed", [False, True])
def test_block_rel_gat_aggregate_autograd_matches_direct_calls(hiplib, form, packed):
    """Block.rel_gat_aggregate with autograd, in the dense form (row = src * R + etype formed by the wrapper) and the packed form: out and
    grad_er bit for bit equal to the direct kernel calls, every gradient within the float64 bounds."""
    import torch
    from COALA_GNN.block_ops import _RelGatAggregate, _RelGatAggregateCSR
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(5 + (form == "csr") + 2 * packed)
    n_dst, n_src, R, H, D = 200, 40, 3, 4, 8
    P = n_src * R
    graph = _fixed_graph(rng, n_dst, 10, n_src, R, True) if form == "fixed" else _csr_graph(rng, rng.integers(0, 90, size=n_dst), n_src, R, False)
    src, typ = graph[-2], graph[-1]
    rows = np.where((src >= 0) & (typ >= 0) & (typ < R), src.astype(np.int64) * R + typ, -1).astype(np.int32)
    b = _block(torch, form, graph, n_src)
    el, er, feat, g = _inputs(rng, P, n_dst, R, H, D, False)
    t = [torch.from_numpy(x).cuda().requires_grad_(True) for x in (el, er, feat)]
    etype = torch.from_numpy(typ.astype(np.int64)).cuda()
    if packed:
        out = b.rel_gat_aggregate(t[0], t[1], t[2], etype, R, rows=torch.from_numpy(rows.astype(np.int64)).cuda(), negative_slope=float(SLOPE))
    else:
        out = b.rel_gat_aggregate(t[0].view(n_src, R, H), t[1], t[2].view(n_src, R, H, D), etype, R, negative_slope=float(SLOPE))
    assert out.grad_fn.name() == (_RelGatAggregateCSR if form == "csr" else _RelGatAggregate).__name__ + "Backward", "the native path ran"
    (out * torch.from_numpy(g).cuda()).sum().backward()
    dgraph = (rows, typ) if form == "fixed" else (graph[0], rows, typ)
    direct = _run(torch, L, form, dgraph, n_dst, P, R, el, er, feat, g, 0)
    assert np.array_equal(out.detach().cpu().numpy().view(np.int32), direct["out"].view(np.int32))
    assert np.array_equal(t[1].grad.cpu().numpy().view(np.int32), direct["ger"].view(np.int32))
    dst, row, ty, nc = _edges(form, dgraph, R)
    ref = reference(dst, row, ty, n_dst, P, R, nc, el, er, feat, g)
    for k, v in dict(out=out.detach(), gf=t[2].grad, gel=t[0].grad, ger=t[1].grad).items():
        _check(k, v.cpu().numpy(), ref[k])


# what takes the fallback, and what the native kernels: dtype, H, R, fan-out, device of the block
PARITY = [("native", np.float32, 4, 3, 7), ("fp64", np.float64, 4, 3, 7), ("heads17", np.float32, 17, 3, 7), ("rh260", np.float32, 13, 20, 7),
          ("fanout33", np.float32, 4, 3, 33), ("rh256", np.float32, 4, 64, 7)]


@pytest.mark.parametrize("form", ["fixed", "csr"])
@pytest.mark.parametrize("name,dtype,H,R,f", PARITY)
def test_dispatch_parity(hiplib, form, name, dtype, H, R, f):
    """Any input, native or fallback, has the shape and the values of rel_gat_aggregate_torch in float64 on the CPU.  Tolerance, as for
    the other ops' dispatch parity: E = the largest difference between the reference in the input's dtype and in float64; the result is
    within 4 E, and never asked to be closer than 8 u times the reference's largest magnitude."""
    import torch
    rng = np.random.default_rng(len(name) + H + R + f + (form == "csr"))
    n_dst, n_src, D = 37, 30, 6
    fixed = _fixed_graph(rng, n_dst, f, n_src, R, False)
    valid = fixed[0] >= 0
    graph = fixed if form == "fixed" else (np.concatenate([[0], np.cumsum(valid.sum(1))]).astype(np.int64), fixed[0][valid], fixed[1][valid])
    el = torch.from_numpy(rng.standard_normal((n_src, R, H)).astype(dtype))
    er = torch.from_numpy(rng.standard_normal((n_dst, R, H)).astype(dtype))
    feat = torch.from_numpy(rng.standard_normal((n_src, R, H, D)).astype(dtype))
    etype = torch.from_numpy(graph[-1].astype(np.int64))
    got = _block(torch, form, graph, n_src).rel_gat_aggregate(el.cuda(), er.cuda(), feat.cuda(), etype.cuda(), R)
    native = name in ("native", "rh256") or (name == "fanout33" and form == "csr")   # a ragged block has no fan-out limit
    host = _block(torch, form, graph, n_src, "cpu")
    want = host.rel_gat_aggregate_torch(el.double(), er.double(), feat.double(), etype, R)
    low = host.rel_gat_aggregate_torch(el, er, feat, etype, R).double()
    assert tuple(got.shape) == tuple(want.shape) == (n_dst, H, D) and got.dtype == el.dtype and got.is_cuda
    e = float((low - want).abs().max())
    unit = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
    tol = max(4.0 * e, 8.0 * unit * float(want.abs().max()))
    err = float((got.double().cpu() - want).abs().max())
    print(f"{name}-{form}: error {err:.3e} E {e:.3e} bound {tol:.3e} (native: {native})")
    assert err <= tol
    # which path ran: with a gradient asked for, the native path leaves its autograd function's name
    out = _block(torch, form, graph, n_src).rel_gat_aggregate(el.cuda().requires_grad_(True), er.cuda(), feat.cuda(), etype.cuda(), R)
    assert ("RelGatAggregate" in out.grad_fn.name()) == native


def test_packed_rows_past_the_table_are_refused(hiplib):
    """A row index at or past P raises before anything is launched, as the torch path's gather does."""
    import torch
    rng = np.random.default_rng(3)
    n_dst, n_src, R, H, D, P = 9, 12, 3, 2, 4, 20
    graph = _fixed_graph(rng, n_dst, 5, n_src, R, False)
    b = _block(torch, "fixed", graph, n_src)
    rows = torch.from_numpy(np.where(graph[0] >= 0, graph[0].astype(np.int64), -1)).cuda()
    rows[0, 0] = P
    el, er, feat = torch.zeros(P, H, device="cuda"), torch.zeros(n_dst, R, H, device="cuda"), torch.zeros(P, H, D, device="cuda")
    etype = torch.zeros(graph[1].shape, dtype=torch.int64, device="cuda")
    with pytest.raises(IndexError, match="rows holds 20"):
        b.rel_gat_aggregate(el, er, feat, etype, R, rows=rows)
    rows[0, 0] = P - 1
    assert tuple(b.rel_gat_aggregate(el, er, feat, etype, R, rows=rows).shape) == (n_dst, H, D)
