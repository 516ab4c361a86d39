"""float64 reference and roundoff bounds of the scaled dot-product attention block op (coala_block_dot_gat_aggregate[_csr][_backward]),
shared by the GPU tests and their CPU twin (tests only).

The op, for dst d, head h and the slots j of d with row_j >= 0 (the row of k / v the slot reads):
  e_j = scale <q[d, h], k[row_j, h]>;  a_j = softmax_j e_j;  out[d, h] = sum_j a_j v[row_j, h];  lse[d, h] = log sum_j exp e_j
  t_j = a_j (<g, v_j> - <g, out>)
  grad_v[row_j, h, c] += a_j g_c;  grad_k[row_j, h, c] += scale t_j q_c;  grad_q[d, h, c] = scale sum_j t_j k[row_j, h, c]

Bounds.  u = 2^-24 (fp32 unit roundoff), gamma(n) = n u / (1 - n u).  As in tests/_gatv2_ref.py the bounds are first order in the
roundings of sums and products and exact (expm1) in the errors that pass through exp; each is multiplied by 1.01 for the second-order
terms and gets an absolute 2^-100 times the magnitude it scales, for weights that underflow.  exp and log are taken to be within 3 ulp:
a relative error of at most 6u for exp, an absolute error of at most 6u |log l| for log.  Per row d and head h with k valid edges and nc
64-slot chunks (1 for a fixed row), P = ceil(D / 64) + 8:
  score     a term q_c k_c is one rounded product.  A head's D terms are added by a 6-step lane scan per 64-float pass and one LDS add
            per pass the head touches (at most ceil(D / 64) + 1); the finished sum is multiplied by scale, one more rounding: at most
            P + 1 levels, so |e~_j - e_j| <= de_j = |scale| gamma(P + 1) sum_c |q_c k_c|.
  weights   the computed exp(e~_j - m~) is exp(e_j - m~) times a factor within exp(+-eta), eta = max_j de_j + u (2 max|x| + 6 nc),
            x_j = e_j - max e: the score error, u|x| from the subtraction, 6u from exp, and per rescale of the online softmax (at most
            nc - 1) 6u plus the rounding of m_old - m_new, whose sum telescopes to at most max|x|.  exp(-m~) is common to the row.
  forward   a~_j / a_j lies within exp(+-2 eta), so
            |out - ref| <= (expm1(2 eta) + gamma(k + nc) + gamma(6 + 2 nc) + 2u) sum_j a_j |v_j|: the numerator sums k products and is
            rescaled at most nc - 1 times; the denominator is a 6-level tree per chunk plus nc sequential adds and nc - 1 rescales; then
            1 / l and the product.  A row without an edge is exactly 0.
  backward  a_j = exp(e~_j - lse~) with the scores computed again (de_j once more).  lse~ = m~ + log l~ carries eta + gamma(6 + 2 nc)
            from l~, 6u log k from log, u (|m| + log k) from the addition; the subtraction adds u (max|x| + log k) and exp 6u:
            a~_j / a_j within exp(+-eta_b), eta_b = eta + max_j de_j + gamma(6 + 2 nc) + u (|m| + 8 log k + max|x| + 6); r = expm1(eta_b).
            A dot product of a head's D floats has at most P levels: gamma(P) sum |g v|.  <g, out> also carries out's forward bound.
            |dt_j| <= (1 + r) a_j (d dot_j + d <g, out>) + |t_j| (r + 3u).
            grad_v[p]: K_p contributions a_j g_c (one more rounding each), added by atomics in any order:
              sum_j a_j |g_c| (r + 2u + gamma(K_p)).
            grad_k[p]: K_p contributions scale t_j q_c (two more roundings), atomics in any order:
              sum_j |scale q_c| (|dt_j| + |t_j| (3u + gamma(K_p))).
            grad_q[d]: the k terms t_j k_jc added in slot order in a register (an fma each), then per chunk one product with scale and,
              after the first chunk, one addition to what is stored: sum_j |scale k_jc| (|dt_j| + |t_j| (2u + gamma(k + 2 nc))).

`fault` makes the float64 values wrong in one of three ways a kernel could be, for the test that the bounds tell right from wrong:
'no_scale' drops the scale from grad_k and grad_q, 'k_for_v' sums k in place of v in out, 'no_gout' drops -<g, out> from t_j."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -100

DIMS = [1, 3, 16, 64, 65, 128]
HEADS = [1, 2, 4, 8, 16]
FANS = [1, 2, 5, 8, 17, 31, 32]
# (n_dst, fan-out, H, D, float offset of every buffer, big scores): every D, H and fan-out appears, at both offsets; plus (16, 128)
SMALL_CASES = [(300 if HEADS[i % 5] * DIMS[i % 6] <= 512 else 90, FANS[i % 7], HEADS[i % 5], DIMS[i % 6], (i // 2) % 2, i % 3 == 0) for i in range(12)]
SMALL_CASES += [(90, 5, 16, 128, 0, False)]


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def scale_of(D):
    """The tests' scale: not 1 at any D, so that a dropped scale shows."""
    return np.float32(0.75 / np.sqrt(D))


def make_inputs(rng, P, n_dst, H, D, big):
    """fp32 q [n_dst, H, D], k, v [P, H, D], grad_out; big: q and k scaled so that the scores reach +-1e3."""
    q = rng.standard_normal((n_dst, H, D)).astype(np.float32)
    k = rng.standard_normal((P, H, D)).astype(np.float32)
    if big:
        q *= np.float32(20.0)
        k *= np.float32(20.0)
    v = rng.standard_normal((P, H, D)).astype(np.float32)
    g = rng.standard_normal((n_dst, H, D)).astype(np.float32)
    return q, k, v, g


def fixed_rows(rng, n_dst, f, P):
    """-1 anywhere in a row, repeated rows, destinations without an edge (row 0 among them, unless it is the only one)."""
    row = rng.integers(0, P, size=(n_dst, f)).astype(np.int32)
    row[rng.random((n_dst, f)) < 0.25] = -1
    rep = rng.random(n_dst) < 0.15
    row[rep, f - 1] = row[rep, 0]
    if n_dst:
        row[rng.random(n_dst) < 0.05] = -1
    if n_dst > 1:
        row[0] = -1
    return row


def csr_rows(rng, n_dst, f, P):
    """Degrees 0..2f, 5 % of the rows at 65..200 edges, row 0 empty (unless it is the only one)."""
    deg = rng.integers(0, 2 * f + 1, size=n_dst)
    if n_dst:
        deg[rng.random(n_dst) < 0.05] = rng.integers(65, 200)
    if n_dst > 1:
        deg[0] = 0
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return indptr, rng.integers(0, P, size=int(indptr[-1])).astype(np.int32)


def edges_fixed(row):
    d, c = np.nonzero(row >= 0)
    return d.astype(np.int64), row[d, c].astype(np.int64), np.ones(row.shape[0])


def edges_csr(indptr, rows):
    deg = np.diff(indptr)
    d = np.repeat(np.arange(len(deg)), deg).astype(np.int64)
    valid = rows >= 0
    return d[valid], rows[valid].astype(np.int64), -(-deg // 64)


def small_case(case):
    """A fixed case of the small table: -> (row [n_dst, f], P, (q, k, v, g), scale, (dst, rows, nc)).  The last 7 rows of k / v are
    never referenced."""
    n_dst, f, H, D, off, big = case
    rng = np.random.default_rng(n_dst * 7 + f * 131 + H * 17 + D + off)
    P = max(64, min(5000, n_dst // 4))
    row = fixed_rows(rng, n_dst, f, P - 7)
    return row, P, make_inputs(rng, P, n_dst, H, D, big), scale_of(D), edges_fixed(row)


def reference(dst, rows, n_dst, P, nc, q, k, v, g, scale, fault=None):
    """float64 values and bounds (module docstring): dict name -> (value, bound) for out, lse, gq, gk, gv, and 'empty', the destinations
    without an edge.  dst / rows: the valid edges (int64), in slot order; nc: chunks per destination."""
    import torch
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
    g_ = lambda n: torch.from_numpy(gamma(n.numpy()))    # noqa: E731
    H, D = k.shape[1], k.shape[2]
    r, s = torch.from_numpy(dst), torch.from_numpy(rows)
    Q, K, V, G = T(q), T(k), T(v), T(g)
    sc = float(scale)
    Pl = -(-D // 64) + 8
    kE, vE, qE, gE = K[s], V[s], Q[r], G[r]                           # [E, H, D]
    e = sc * (qE * kE).sum(-1)                                       # [E, H]
    de = abs(sc) * float(gamma(Pl + 1)) * (qE * kE).abs().sum(-1)
    rh = r.unsqueeze(1).expand(-1, H)
    m = torch.full((n_dst, H), float("-inf"), dtype=torch.float64).scatter_reduce(0, rh, e, "amax")
    x = e - m[r]
    p = torch.exp(x)
    l = torch.zeros((n_dst, H), dtype=torch.float64).index_add_(0, r, p)
    a = p / l[r]
    summed = kE if fault == "k_for_v" else vE
    out = torch.zeros((n_dst, H, D), dtype=torch.float64).index_add_(0, r, a.unsqueeze(-1) * summed)
    absout = torch.zeros_like(out).index_add_(0, r, a.unsqueeze(-1) * vE.abs())
    absv = torch.zeros_like(out).index_add_(0, r, vE.abs())
    kcnt = torch.bincount(r, minlength=n_dst).to(torch.float64)
    kk = kcnt.unsqueeze(1)
    ncr = torch.from_numpy(np.asarray(nc, dtype=np.float64)).unsqueeze(1)
    zero = torch.zeros((n_dst, H), dtype=torch.float64)
    maxx = zero.scatter_reduce(0, rh, x.abs(), "amax")
    emax = zero.scatter_reduce(0, rh, de, "amax")
    eta = emax + U * (2 * maxx + 6 * ncr)
    b_out = 1.01 * ((torch.expm1(2 * eta) + g_(kk + ncr) + g_(6 + 2 * ncr) + 2 * U).unsqueeze(-1) * absout + TINY * absv)
    mm = torch.where(torch.isfinite(m), m, zero)
    logk = torch.log(kk.clamp_min(1))
    lse = torch.where(kk > 0, mm + torch.log(l.clamp_min(1e-300)), torch.full_like(l, float("-inf")))
    b_lse = 1.01 * (eta + g_(6 + 2 * ncr) + U * (mm.abs() + 8 * logk + 1)) + TINY
    # backward (the correct out, whatever the fault did to the forward)
    out_t = torch.zeros((n_dst, H, D), dtype=torch.float64).index_add_(0, r, a.unsqueeze(-1) * vE)
    eta_b = eta + emax + g_(6 + 2 * ncr) + U * (mm.abs() + 8 * logk + maxx + 6)
    rb = torch.expm1(eta_b)[r]                                      # [E, H]
    dot = (gE * vE).sum(-1)
    absdot = (gE * vE).abs().sum(-1)
    dout = (G * out_t).sum(-1)
    ddout = float(gamma(Pl)) * (G * out_t).abs().sum(-1) + (G.abs() * b_out).sum(-1)
    t = a * (dot - (0 if fault == "no_gout" else dout[r]))
    t_abs = (a * (dot - dout[r])).abs()
    dt = (1 + rb) * a * (float(gamma(Pl)) * absdot + ddout[r]) + t_abs * (rb + 3 * U)
    Ks = torch.bincount(s, minlength=P).to(torch.float64)
    gKs = g_(Ks)[s].unsqueeze(1)                                    # [E, 1]
    sg = 1.0 if fault == "no_scale" else sc
    gv = torch.zeros((P, H, D), dtype=torch.float64).index_add_(0, s, a.unsqueeze(-1) * gE)
    b_gv = 1.01 * torch.zeros_like(gv).index_add_(0, s, (a * (rb + 2 * U + gKs)).unsqueeze(-1) * gE.abs() + TINY * gE.abs())
    gk = torch.zeros((P, H, D), dtype=torch.float64).index_add_(0, s, sg * t.unsqueeze(-1) * qE)
    b_gk = 1.01 * torch.zeros_like(gk).index_add_(0, s, abs(sc) * qE.abs() * (dt + t_abs * (3 * U + gKs)).unsqueeze(-1) + TINY * qE.abs())
    gq = torch.zeros((n_dst, H, D), dtype=torch.float64).index_add_(0, r, sg * t.unsqueeze(-1) * kE)
    b_gq = 1.01 * torch.zeros_like(gq).index_add_(0, r, abs(sc) * kE.abs() * (dt + t_abs * (2 * U + g_(kk + 2 * ncr)[r])).unsqueeze(-1)
                                                  + TINY * kE.abs())
    return dict(out=(out.numpy(), b_out.numpy()), lse=(lse.numpy(), b_lse.numpy()), gq=(gq.numpy(), b_gq.numpy()),
                gk=(gk.numpy(), b_gk.numpy()), gv=(gv.numpy(), b_gv.numpy()), empty=(kcnt == 0).numpy())


GRADS = ("gq", "gk", "gv")


def outside(got, ref_bound):
    """Number of elements past the bound."""
    ref, bound = ref_bound
    return int((~(np.abs(np.asarray(got, dtype=np.float64) - ref) <= bound)).sum())


def check(name, got, ref_bound, log=None):
    ref, bound = ref_bound
    got = np.asarray(got, dtype=np.float64)
    same_inf = np.isinf(ref) & (got == ref)                         # lse of a destination without an edge: -inf on both sides
    err = np.where(same_inf, 0.0, np.abs(got - np.where(same_inf, 0.0, ref)))
    if log is not None and err.size:
        i = np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)
        log(f"{name}: largest error / bound {err[i] / max(bound[i], 1e-300):.3f} (error {err[i]:.3e}, bound {bound[i]:.3e})")
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} elements past the bound; at {i}: got {got[i]!r} want {ref[i]!r} bound {bound[i]!r}")


def check_all(got, ref, log=None, names=("out", "lse") + GRADS):
    for n in names:
        check(n, got[n], ref[n], log)
    assert np.all(got["out"][ref["empty"]] == 0.0), "a destination without an edge is not exactly 0"
    assert np.all(np.isneginf(got["lse"][ref["empty"]])), "lse of a destination without an edge is not -inf"
    if "gq" in names:
        assert np.all(got["gq"][ref["empty"]] == 0.0), "grad_q of a destination without an edge is not exactly 0"
    assert all(np.isfinite(got[n]).all() for n in names if n != "lse")


def _segment_sums(x, D):
    """head_segment_add's order in fp32: x [N, H * D] -> [N, H], every 64-float pass scanned by a 6-step segmented inclusive scan, the
    last lane of each head's segment in the pass added to the head's sum, pass after pass."""
    N, hd = x.shape
    H = hd // D
    acc = np.zeros((N, H), np.float32)
    lane = np.arange(64)
    for c0 in range(0, hd, 64):
        c = c0 + lane
        inside = c < hd
        h = np.where(inside, c // D, 0)
        start = np.where(inside, np.maximum(h * D - c0, 0), hd - c0)
        xs = np.zeros((N, 64), np.float32)
        xs[:, : min(64, hd - c0)] = x[:, c0: c0 + 64]
        o = 1
        while o < 64:
            y = np.zeros_like(xs)
            y[:, o:] = xs[:, :-o]
            xs = np.where((lane - o >= start)[None, :], xs + y, xs).astype(np.float32)
            o <<= 1
        for ln in np.nonzero(inside & ((lane == 63) | (c + 1 == hd) | ((c + 1) % D == 0)))[0]:
            acc[:, h[ln]] += xs[:, ln]
    return acc


def _butterfly(x, op):
    """wave_sum / wave_max over the last axis (64 lanes) in the kernel's xor order, fp32."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = op(x, x[..., lane ^ o]).astype(np.float32)
    return x[..., 0]


def kernel_order_fp32(row, q, k, v, g, scale):
    """The fixed-form kernels restated in numpy fp32, in their summation orders (a row is one chunk of 64 lanes; the atomics in
    np.add.at's order): -> dict of out, lse, gq, gk, gv."""
    n_dst, f = row.shape
    P, H, D = k.shape
    hd = H * D
    f32 = np.float32
    scale = f32(scale)
    valid = row >= 0
    rc = np.where(valid, row, 0)
    qf, kf, vf, gf = (a.reshape(a.shape[0], hd) for a in (q, k, v, g))
    dots = np.zeros((n_dst, 64, H), f32)
    gdots = np.zeros((n_dst, 64, H), f32)
    for j in range(f):
        dots[:, j] = _segment_sums(qf * kf[rc[:, j]], D)
        gdots[:, j] = _segment_sums(gf * vf[rc[:, j]], D)
    val = np.zeros((n_dst, 64), bool)
    val[:, :f] = valid
    e = np.where(val[..., None], scale * dots, f32(-np.inf)).astype(f32)              # [n_dst, 64, H]
    m = _butterfly(np.moveaxis(e, 1, -1), np.maximum)                                # [n_dst, H]
    with np.errstate(invalid="ignore"):
        p = np.where(val[..., None], np.exp(e - m[:, None, :], dtype=f32), f32(0)).astype(f32)
    l = _butterfly(np.moveaxis(p, 1, -1), np.add)
    out = np.zeros((n_dst, H, D), f32)
    for j in range(f):
        out += np.where(valid[:, j, None, None], p[:, j, :, None] * v[rc[:, j]], f32(0)).astype(f32)
    inv = np.where(l > 0, f32(1) / np.where(l > 0, l, f32(1)), f32(0)).astype(f32)
    out = (out * inv[..., None]).astype(f32)
    with np.errstate(divide="ignore"):
        lse = np.where(l > 0, m + np.log(np.where(l > 0, l, f32(1)), dtype=f32), f32(-np.inf)).astype(f32)
    gout = _segment_sums(gf * out.reshape(n_dst, hd), D)                              # [n_dst, H]
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.where(val[..., None], np.exp(scale * dots - lse[:, None, :], dtype=f32), f32(0)).astype(f32)
    t = (a * (gdots - gout[:, None, :])).astype(f32)
    t = np.where(val[..., None], t, f32(0)).astype(f32)
    gq = np.zeros((n_dst, H, D), f32)
    gk = np.zeros((P, H, D), f32)
    gv = np.zeros((P, H, D), f32)
    for j in range(f):
        sel = valid[:, j]
        gq += np.where(sel[:, None, None], t[:, j, :, None] * k[rc[:, j]], f32(0)).astype(f32)
        np.add.at(gv, row[sel, j], (a[sel, j, :, None] * g[sel]).astype(f32))
        np.add.at(gk, row[sel, j], ((scale * t[sel, j, :, None]).astype(f32) * q[sel]).astype(f32))
    gq = (scale * gq).astype(f32)
    return dict(out=out, lse=lse, gq=gq, gk=gk, gv=gv)


PARITY_INPUTS = ("3d", "colslice", "transposed", "fp64", "fp16", "fanout33", "nbr_slice", "heads17")


def parity_check(device, form, inp, packed=False, log=print):
    """tests/_dispatch_parity.py's check for Block.dot_gat_aggregate (its OPS tuple is closed): whatever path the input takes, the
    result has the shape, the dtype and the values of dot_gat_aggregate_torch in float64 on the CPU, under that file's tolerance rule."""
    import torch
    import _dispatch_parity as DP
    rng = np.random.default_rng(700 + DP.FORMS.index(form) * 10 + PARITY_INPUTS.index(inp) + 100 * packed)
    f = 33 if inp == "fanout33" else 7
    H, D = (17 if inp == "heads17" else DP.H), DP.D
    nbr = rng.integers(0, DP.N_SRC, size=(DP.N_DST, f)).astype(np.int32)
    nbr[rng.random((DP.N_DST, f)) < 0.25] = -1
    nbr[3] = -1                                                  # a destination without an in-edge
    nbr[5] = np.arange(f)                                        # a full row
    dtype = {"fp64": torch.float64, "fp16": torch.float16}.get(inp, torch.float32)
    if inp == "colslice":
        base = torch.from_numpy(rng.standard_normal((2, DP.N_SRC, H, D + 2)).astype(np.float32))
        view = lambda t: t[..., 1: 1 + D]   # noqa: E731
    elif inp == "transposed":
        base = torch.from_numpy(rng.standard_normal((2, H, DP.N_SRC, D)).astype(np.float32))
        view = lambda t: t.transpose(1, 2)   # noqa: E731
    else:
        base = torch.from_numpy(rng.standard_normal((2, DP.N_SRC, H, D)).astype(np.float32)).to(dtype)
        view = lambda t: t                   # noqa: E731
    q = torch.from_numpy(rng.standard_normal((DP.N_DST, H, D)).astype(np.float32)).to(dtype)

    def call(block, suffix, dev, dt):
        kv = view(base.to(dev)) if dt is None else view(base).to(dt).to(dev)
        qq = q.to(dev) if dt is None else q.to(dt).to(dev)
        rows = None
        if packed:                                                # the block's own slots, as an int64 rows tensor
            rows = (block.indices if block.nbr is None else block.nbr).to(torch.int64).clone()
        return getattr(block, "dot_gat_aggregate" + suffix)(qq, kv[0], kv[1], rows)

    got = call(DP._block(device, form, nbr, inp == "nbr_slice"), "", device, None)
    host = DP._block("cpu", form, nbr, False)
    want = call(host, "_torch", "cpu", torch.float64)
    try:
        low = call(host, "_torch", "cpu", dtype).double()
    except RuntimeError:       # an op the CPU does not have in this dtype (fp16): the floor alone then bounds the error
        low = None
    assert tuple(got.shape) == tuple(want.shape), f"shape {tuple(got.shape)}, the reference gives {tuple(want.shape)}"
    assert got.dtype == dtype
    e = float((low - want).abs().max()) if low is not None else 0.0
    tol = max(4.0 * e, 8.0 * DP.UNIT[dtype] * float(want.abs().max()))
    err = float((got.detach().double().cpu() - want).abs().max())
    log(f"dot_gat-{form}-{inp}: error {err:.3e} E {e:.3e} bound {tol:.3e}")
    assert err <= tol, f"error {err:.3e} above {tol:.3e}"
