"""float64 reference and roundoff bounds of the GATv2 block op (coala_block_gatv2_aggregate[_csr][_backward]), shared by the GPU tests
and their CPU twin (tests only).

The op, for dst d, head h and the valid in-edges j of d (source s_j), slope = negative_slope:
  z_jc = feat_src[s_j, h, c] + feat_dst[d, h, c];  e_j = sum_c attn[h, c] lrelu(z_jc);  a_j = softmax_j e_j;  out[d, h] = sum_j a_j feat_src[s_j, h]
  t_j = a_j (<g, feat_src_j> - <g, out>);  k_jc = z_jc > 0 ? 1 : slope
  grad_src[s_j, h, c] += a_j g_c + t_j attn_c k_jc;  grad_dst[d, h, c] = sum_j t_j attn_c k_jc;  grad_attn[h, c] = sum_d sum_j t_j lrelu(z_jc)

Bounds.  u = 2^-24 (fp32 unit roundoff), gamma(n) = n u / (1 - n u).  The bounds are first order in the roundings of sums and products
and exact (expm1) in the errors that pass through exp, which are not small when the scores are large; each is multiplied by 1.01 for
the remaining second-order terms and gets an absolute 2^-100 times the magnitude it scales, for weights that underflow.  exp and log are
taken to be within 3 ulp (the OpenCL full-profile limit, which the device library meets): a relative error of at most 6u for exp, an
absolute error of at most 6u |log l| for log.  Per row d and head h with k valid edges and nc 64-edge chunks (1 for a fixed row):
  kink      z_jc is one fp32 addition of two fp32 numbers: correctly rounded, so its sign (and whether it is zero) is that of the exact
            sum, which float64 also gives.  The kernel and the reference are always on the same side of the kink: no element is excluded.
  score     a term attn_c lrelu(z_jc) carries three roundings (the sum, the slope product, the attn product).  A head's D terms are added
            by a 6-step lane scan per 64-float pass and one LDS add per pass the head touches (at most ceil(D / 64) + 1): with the
            term's own roundings at most P + 2 levels, P = ceil(D / 64) + 8, so |e~_j - e_j| <= de_j = gamma(P + 2) sum_c |attn_c lrelu(z_jc)|.
  weights   the computed exp(e~_j - m~) is exp(e_j - m~) times a factor within exp(+-eta), eta = max_j de_j + u (2 max|x| + 6 nc),
            x_j = e_j - max e: the score error, u|x| from the subtraction, 6u from exp, and per rescale of the online softmax (at most
            nc - 1) 6u plus the rounding of m_old - m_new, whose sum telescopes to at most max|x|.  exp(-m~) is common to the row.
  forward   a~_j / a_j lies within exp(+-2 eta) (numerator and denominator), so
            |out - ref| <= (expm1(2 eta) + gamma(k + nc) + gamma(6 + 2 nc) + 2u) sum_j a_j |feat_src_j|: the numerator sums k products
            and is rescaled at most nc - 1 times; the denominator is a 6-level tree per chunk plus nc sequential adds and nc - 1 rescales;
            then 1 / l and the product.  A row without a valid edge is exactly 0.
  lse       m~ + log l~, the output the backward reads: eta + gamma(6 + 2 nc) + u (|m| + 8 log k + 1), the form of tests/_dot_gat_ref.py
            (the weights, l's sum, 6u log k from log, u (|m| + log k) from the addition and one more u).  -inf on a row without a valid edge.
  backward  a_j = exp(e~_j - lse~) with the scores computed again (de_j once more).  lse~ = m~ + log l~ carries eta + gamma(6 + 2 nc)
            from l~, 6u log k from log, u (|m| + log k) from the addition; the subtraction e~_j - lse~ adds u (max|x| + log k) and exp 6u:
            a~_j / a_j within exp(+-eta_b), eta_b = eta + max_j de_j + gamma(6 + 2 nc) + u (|m| + 8 log k + max|x| + 6); r = expm1(eta_b).
            A dot product of a head's D floats has at most P levels: gamma(P) sum |g f|.  <g, out> also carries out's forward bound.
            |dt_j| <= (1 + r) a_j (d dot_j + d <g, out>) + |t_j| (r + 3u).
            grad_src[s]: K_s contributions a_j g_c + t_j attn_c k_jc, each with three more roundings, added by atomics in any order:
              sum_j a_j |g_c| (r + 3u + gamma(K_s)) + k_jc |attn_c| (|dt_j| + |t_j| (3u + gamma(K_s))).
            grad_dst[d]: the k terms t_j attn_c k_jc added in slot order, once more per chunk: sum_j k_jc |attn_c| (|dt_j| + |t_j| (2u + gamma(k + nc))).
            grad_attn: a term t_j lrelu(z_jc) has three more roundings.  Wave w adds the terms of its rows (row d belongs to wave
              d mod W; W = 4 parts for H D <= 1024, parts above) edge by edge and chunk by chunk, a chain of at most
              L = max_w sum_{d in w} (k_d + nc_d) additions; three more add the waves of a block, and the caller's sum of the `parts`
              partial rows at most parts, in any order: sum |dt_j lrelu(z_jc)| + (3u + gamma(L + 3 + parts)) sum |t_j lrelu(z_jc)|.

`fault` makes the float64 values wrong in one of three ways a kernel could be, for the test that the bounds tell right from wrong:
'v1' applies attn before the leaky_relu (e_j = lrelu(sum_c attn_c z_jc), GAT's score), 'no_t' drops t_j attn_c k_jc from grad_src, 'kink'
takes k_jc on the wrong side of 0."""
import numpy as np

U = 2.0 ** -24
SLOPE = np.float32(0.2)
TINY = 2.0 ** -100

DIMS = [1, 3, 16, 64, 65, 128]
HEADS = [1, 2, 4, 8, 16]
FANS = [1, 2, 5, 8, 17, 31, 32]
# (n_dst, fan-out, H, D, float offset of every buffer, big scores): every D, H and fan-out appears, at both offsets; H * D = 1024 is the
# longest row whose grad_attn sums stay in registers, and (16, 128) takes the other backward kernel
SMALL_CASES = [(300 if HEADS[i % 5] * DIMS[i % 6] <= 512 else 90, FANS[i % 7], HEADS[i % 5], DIMS[i % 6], (i // 2) % 2, i % 3 == 0) for i in range(12)]
SMALL_CASES += [(90, 5, 16, 128, 0, False)]


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def default_parts(n_dst):
    """The autograd wrapper's choice (block_ops._gatv2_parts), restated."""
    return max(1, min(-(-n_dst // 4), 1024))


def make_inputs(rng, n_src, n_dst, H, D, big):
    """fp32 feat_src, feat_dst, attn [H, D], grad_out; big: rows scaled so that the scores reach +-1e3."""
    fs = rng.standard_normal((n_src, H, D)).astype(np.float32)
    fd = rng.standard_normal((n_dst, H, D)).astype(np.float32)
    if big:
        scale = np.float32(400.0 / np.sqrt(D))
        fs *= scale
        fd *= scale
    attn = rng.standard_normal((H, D)).astype(np.float32)
    attn[0, 0] = -abs(attn[0, 0])      # with every attn >= 0 and D = 1 the score would be GAT's: attn lrelu(z) = lrelu(attn z)
    g = rng.standard_normal((n_dst, H, D)).astype(np.float32)
    return fs, fd, attn, g


def fixed_nbr(rng, n_dst, f, n_src):
    """-1 anywhere in a row, repeated sources, rows without a valid edge (row 0 among them)."""
    nbr = rng.integers(0, n_src, size=(n_dst, f)).astype(np.int32)
    nbr[rng.random((n_dst, f)) < 0.25] = -1
    rep = rng.random(n_dst) < 0.15
    nbr[rep, f - 1] = nbr[rep, 0]
    if n_dst:
        nbr[rng.random(n_dst) < 0.05] = -1
        nbr[0] = -1
    return nbr


def edges_fixed(nbr):
    rows, cols = np.nonzero(nbr >= 0)
    return rows.astype(np.int64), nbr[rows, cols].astype(np.int64), np.ones(nbr.shape[0])


def edges_csr(indptr, indices):
    deg = np.diff(indptr)
    rows = np.repeat(np.arange(len(deg)), deg).astype(np.int64)
    valid = indices >= 0
    return rows[valid], indices[valid].astype(np.int64), -(-deg // 64)


def reference(rows, srcs, n_dst, n_src, nc, fs, fd, attn, g, parts, slope=SLOPE, fault=None, wave_rows=None):
    """float64 values and bounds (module docstring): dict name -> (value, bound) for out, gs (grad_src), gd (grad_dst), ga (grad_attn),
    and 'empty', the rows without a valid edge.  rows / srcs: the valid edges (int64), in row order; nc: chunks per row; parts: rows of
    the grad_attn partials buffer.  wave_rows: the row numbers the kernel deals to its waves, when the n_dst rows given here are a
    subset of a larger block whose other rows add exact zeros to grad_attn (default: 0 .. n_dst - 1)."""
    import torch
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
    g_ = lambda n: torch.from_numpy(gamma(n.numpy()))    # noqa: E731
    H, D = fs.shape[1], fs.shape[2]
    r, s = torch.from_numpy(rows), torch.from_numpy(srcs)
    F, Fd, A, G = T(fs), T(fd), T(attn).reshape(1, H, D), T(g)
    sl = float(slope)
    P = -(-D // 64) + 8
    fE = F[s]                                                       # [E, H, D]
    z = fE + Fd[r]
    pos = z > 0
    lz = torch.where(pos, z, z * sl)
    kf = torch.where(pos, torch.ones_like(z), torch.full_like(z, sl))
    if fault == "kink":
        kf = torch.where(pos, torch.full_like(z, sl), torch.ones_like(z))
    e = (A * lz).sum(-1)                                            # [E, H]
    de = float(gamma(P + 2)) * (A * lz).abs().sum(-1)
    if fault == "v1":
        lin = (A * z).sum(-1)
        e = torch.where(lin > 0, lin, lin * sl)
    rh = r.unsqueeze(1).expand(-1, H)
    m = torch.full((n_dst, H), float("-inf"), dtype=torch.float64).scatter_reduce(0, rh, e, "amax")
    x = e - m[r]
    p = torch.exp(x)
    l = torch.zeros((n_dst, H), dtype=torch.float64).index_add_(0, r, p)
    a = p / l[r]
    out = torch.zeros((n_dst, H, D), dtype=torch.float64).index_add_(0, r, a.unsqueeze(-1) * fE)
    absout = torch.zeros_like(out).index_add_(0, r, a.unsqueeze(-1) * fE.abs())
    absf = torch.zeros_like(out).index_add_(0, r, fE.abs())
    kcnt = torch.bincount(r, minlength=n_dst).to(torch.float64)
    k = kcnt.unsqueeze(1)
    ncr = torch.from_numpy(np.asarray(nc, dtype=np.float64)).unsqueeze(1)
    zero = torch.zeros((n_dst, H), dtype=torch.float64)
    maxx = zero.scatter_reduce(0, rh, x.abs(), "amax")
    emax = zero.scatter_reduce(0, rh, de, "amax")
    eta = emax + U * (2 * maxx + 6 * ncr)
    b_out = 1.01 * ((torch.expm1(2 * eta) + g_(k + ncr) + g_(6 + 2 * ncr) + 2 * U).unsqueeze(-1) * absout + TINY * absf)
    mm = torch.where(torch.isfinite(m), m, zero)
    logk = torch.log(k.clamp_min(1))
    lse = torch.where(k > 0, mm + torch.log(l.clamp_min(1e-300)), torch.full_like(l, float("-inf")))
    b_lse = 1.01 * (eta + g_(6 + 2 * ncr) + U * (mm.abs() + 8 * logk + 1)) + TINY
    # backward
    eta_b = eta + emax + g_(6 + 2 * ncr) + U * (mm.abs() + 8 * logk + maxx + 6)
    rb = torch.expm1(eta_b)[r]                                      # [E, H]
    gE = G[r]
    dot = (gE * fE).sum(-1)
    absdot = (gE * fE).abs().sum(-1)
    dout = (G * out).sum(-1)
    ddout = float(gamma(P)) * (G * out).abs().sum(-1) + (G.abs() * b_out).sum(-1)
    t = a * (dot - dout[r])
    dt = (1 + rb) * a * (float(gamma(P)) * absdot + ddout[r]) + t.abs() * (rb + 3 * U)
    Ks = torch.bincount(s, minlength=n_src).to(torch.float64)
    gKs = g_(Ks)[s].unsqueeze(1)                                    # [E, 1]
    ak = A.abs() * kf                                               # [E, H, D]
    via_t = t.unsqueeze(-1) * A * kf
    gs = torch.zeros((n_src, H, D), dtype=torch.float64).index_add_(0, s, a.unsqueeze(-1) * gE + (0 if fault == "no_t" else via_t))
    b_gs = 1.01 * torch.zeros_like(gs).index_add_(0, s, (a * (rb + 3 * U + gKs)).unsqueeze(-1) * gE.abs()
                                                  + ak * (dt + t.abs() * (3 * U + gKs)).unsqueeze(-1) + TINY * (gE.abs() + A.abs()))
    gd = torch.zeros((n_dst, H, D), dtype=torch.float64).index_add_(0, r, via_t)
    b_gd = 1.01 * torch.zeros_like(gd).index_add_(0, r, ak * (dt + t.abs() * (2 * U + g_(k + ncr)[r])).unsqueeze(-1)) + TINY * A.abs()
    ga = (t.unsqueeze(-1) * lz).sum(0)
    waves = parts * (4 if H * D <= 1024 else 1)
    chain = np.bincount((np.arange(n_dst) if wave_rows is None else np.asarray(wave_rows, dtype=np.int64)) % waves, weights=kcnt.numpy() + np.asarray(nc, dtype=np.float64), minlength=1).max() if n_dst else 0.0
    b_ga = 1.01 * ((dt.unsqueeze(-1) * lz.abs()).sum(0) + (3 * U + float(gamma(chain + 3 + parts))) * (t.abs().unsqueeze(-1) * lz.abs()).sum(0)) + TINY
    return dict(out=(out.numpy(), b_out.numpy()), gs=(gs.numpy(), b_gs.numpy()), gd=(gd.numpy(), b_gd.numpy()), ga=(ga.numpy(), b_ga.numpy()),
                lse=(lse.numpy(), b_lse.numpy()), empty=(kcnt == 0).numpy())


def outside(got, ref_bound):
    """Number of elements past the bound."""
    ref, bound = ref_bound
    return int((~(np.abs(np.asarray(got, dtype=np.float64) - ref) <= bound)).sum())


def check(name, got, ref_bound, log=None):
    ref, bound = ref_bound
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    if log is not None and err.size:
        i = np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)
        log(f"{name}: largest error / bound {err[i] / max(bound[i], 1e-300):.3f} (error {err[i]:.3e}, bound {bound[i]:.3e})")
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} elements past the bound; at {i}: got {got[i]!r} want {ref[i]!r} bound {bound[i]!r}")


def check_all(got, ref, log=None):
    for k in ("out", "gs", "gd", "ga"):
        check(k, got[k], ref[k], log)
    if "lse" in got:                                                # the kernels' output; the torch fallback keeps none
        full = ~ref["empty"]
        check("lse", got["lse"][full], (ref["lse"][0][full], ref["lse"][1][full]), log)
        assert np.all(np.isneginf(got["lse"][ref["empty"]])), "lse of a row without a valid edge is not -inf"
    assert np.all(got["out"][ref["empty"]] == 0.0), "a row without a valid edge is not exactly 0"
    assert np.all(got["gd"][ref["empty"]] == 0.0), "grad_dst of a row without a valid edge is not exactly 0"
    assert all(np.isfinite(got[k]).all() for k in ("out", "gs", "gd", "ga"))


PARITY_INPUTS = ("3d", "colslice", "transposed", "fp64", "fp16", "fanout33", "nbr_slice", "heads17")


def parity_check(device, form, inp, log=print):
    """tests/_dispatch_parity.py's check for Block.gatv2_aggregate (its OPS tuple is closed): whatever path the input takes, the
    result has the shape, the dtype and the values of gatv2_aggregate_torch in float64 on the CPU, under that file's tolerance rule."""
    import torch
    import _dispatch_parity as DP
    rng = np.random.default_rng(500 + DP.FORMS.index(form) * 10 + PARITY_INPUTS.index(inp))
    f = 33 if inp == "fanout33" else 7
    H, D = (17 if inp == "heads17" else DP.H), DP.D
    nbr = rng.integers(0, DP.N_SRC, size=(DP.N_DST, f)).astype(np.int32)
    nbr[rng.random((DP.N_DST, f)) < 0.25] = -1
    nbr[3] = -1                                                  # a destination without an in-edge
    nbr[5] = np.arange(f)                                        # a full row
    dtype = {"fp64": torch.float64, "fp16": torch.float16}.get(inp, torch.float32)
    if inp == "colslice":
        base = torch.from_numpy(rng.standard_normal((DP.N_SRC, H, D + 2)).astype(np.float32))
        view = lambda t: t[:, :, 1: 1 + D]   # noqa: E731
    elif inp == "transposed":
        base = torch.from_numpy(rng.standard_normal((H, DP.N_SRC, D)).astype(np.float32))
        view = lambda t: t.transpose(0, 1)   # noqa: E731
    else:
        base = torch.from_numpy(rng.standard_normal((DP.N_SRC, H, D)).astype(np.float32)).to(dtype)
        view = lambda t: t                   # noqa: E731
    fd = torch.from_numpy(rng.standard_normal((DP.N_DST, H, D)).astype(np.float32)).to(dtype)
    attn = torch.from_numpy(rng.standard_normal((1, H, D)).astype(np.float32)).to(dtype)

    def call(block, suffix, dev, dt):
        h = view(base.to(dev)) if dt is None else view(base).to(dt).to(dev)
        cast = (lambda t: t.to(dev)) if dt is None else (lambda t: t.to(dt).to(dev))
        return getattr(block, "gatv2_aggregate" + suffix)(h, cast(fd), cast(attn) if suffix == "" else cast(attn)[0])

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
    log(f"gatv2-{form}-{inp}: error {err:.3e} E {e:.3e} bound {tol:.3e}")
    assert err <= tol, f"error {err:.3e} above {tol:.3e}"
