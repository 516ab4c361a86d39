"""float64 one-step references of Adam and row-wise Adagrad on table rows (tests only), in the style of tests/_embedding_ref.py, with the
bounds the tests hold the fp32 code to.  Every reference starts from the fp32 bytes the call sees and takes every scalar as f32(x).

Rows, both ops      |got - ref| <= 2^-23 |ref| + K * 2^-24 |upd|
Adam m, v           |got - ref| <= 2 * 2^-23 (|beta x| + |(1 - beta) y|)        (the two products and the sum; y = g or g^2)
row-wise state      |got - ref| <= (A + 3) * 2^-24 s

K counts the fp32 roundings on upd's path, each perturbing upd by at most 2^-24 of itself; the final subtraction row - upd rounds once
more, relative to the result (the 2^-23 |ref| term has room for it).

Adam, upd = lr (m / bc1) / (sqrt(v / bc2) + eps), computed as (step_size * m) / (sqrt(v) * rsbc2 + eps):
  numerator    m = fma(beta1, m0, p) + e with p + e == (1 - beta1) g exactly: the fma and the sum                           2
               (m0 is signed and the two terms of m can cancel, so every rounding here has to be relative to m itself: a rounded
               product (1 - beta1) g would leave an error relative to the product, amplified without bound relative to upd)
               step_size = lr / bc1, one rounding from double to fp32 (bc1 = -expm1(t ln beta1) in double)                   1
               step_size * m                                                                                                1
  denominator  v = fma(beta2, v0, (1 - beta2) * (g * g)): 1 - beta2, g * g, the product, the fma -- 4 on v, all terms
               positive; sqrt halves them                                                                                   2
               sqrt                                                                                                         1
               rsbc2 = 1 / sqrt(bc2), one rounding from double to fp32                                                      1
               fma(sqrt(v), rsbc2, eps): one rounding of a sum of positive terms                                            1
  the division                                                                                                              1
  total 10; K_ADAM = 12 leaves two for the products of the (1 + d) factors and the double-precision error of expm1 / log.
  (The torch backend rounds m once from a float64 sum and v once more -- product and sum apart: 9.5.)

Row-wise Adagrad, upd_k = g_k * lr / (sqrt(s) + eps), s = s0 + (1 / dim) sum g^2:
  s carries A + 3 roundings (below); sqrt halves them                                                             (A + 3) / 2
  sqrt, + eps, lr / ( ), and the product with g_k (none in the kernel: it is inside the final fma)                          4
  K_ROWWISE(A) = ceil((A + 3) / 2) + 4, which is 16 at the largest A of the kernel, 21.

A, the additions on the longest path from one g_k^2 to the total, in the kernel's summation order (write_rows_kernel in
coala_cache.hip): a lane adds the squares of its own VPL * VEC floats in load order, one fma each -- the first square is rounded by
its fma with 0, every later fma rounds the square and the sum together -- so a lane's partial sum carries VPL * VEC roundings,
VPL * VEC - 1 of them additions; the xor butterfly over the row's LPR lanes adds log2(LPR) more.  With UNITS = line / VEC accesses per
line, LPR = min(UNITS, 64), VPL = UNITS / LPR:  A = VPL * VEC - 1 + log2(LPR)  (rowwise_additions).  The "+ 3": the first square's own
rounding, the division of the total by dim, and the sum with s0.  All terms are positive, so the bound is relative to s.
The torch backend sums pairwise over the row padded to a power of two: A = ceil(log2 dim).

Inputs stay away from denormals: make_grad / make_state of _embedding_ref; Adam's m is a make_state magnitude with a random sign."""
import numpy as np

from _embedding_ref import U23, U24, f32, make_grad, make_state  # noqa: F401  (make_grad / make_state re-exported for the tests)

K_ADAM = 12
PRIOR_STEPS = np.array([0, 1, 9, 999, 10 ** 6], dtype=np.int32)
INT32_MAX = 2 ** 31 - 1


def make_signed_state(rng, shape):
    return (make_state(rng, shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def make_steps(rng, n):
    return rng.choice(PRIOR_STEPS, size=n).astype(np.int32)


def _f64(*arrays):
    return tuple(np.asarray(a, dtype=np.float32).astype(np.float64) for a in arrays)


def bias_corrections(t, beta):
    """1 - beta^t as -expm1(t ln beta), float64, beta as its fp32 value (beta = 0: 1)."""
    b = f32(beta)
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return -np.expm1(t * np.log(np.float64(b)))


def adam_ref(rows32, m32, v32, t, grad32, lr, beta1, beta2, eps):
    """-> (new rows, new m, new v, upd), float64.  t: the step count AFTER the increment, a scalar or one per row."""
    r, m0, v0, g = _f64(rows32, m32, v32, grad32)
    b1, b2 = f32(beta1), f32(beta2)
    m = b1 * m0 + (1.0 - b1) * g
    v = b2 * v0 + (1.0 - b2) * g * g
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), (r.shape[0],))
    bc1, bc2 = bias_corrections(t, beta1)[:, None], bias_corrections(t, beta2)[:, None]
    upd = f32(lr) * (m / bc1) / (np.sqrt(v / bc2) + f32(eps))
    return r - upd, m, v, upd


def check_adam(got_rows, got_m, got_v, rows32, m32, v32, t, grad32, lr, beta1, beta2, eps, what="", scale=1.0):
    """scale: 2 where the issue allows twice the bound (torch.optim.SparseAdam)."""
    ref, m, v, upd = adam_ref(rows32, m32, v32, t, grad32, lr, beta1, beta2, eps)
    _, m0, v0, g = _f64(rows32, m32, v32, grad32)
    b1, b2 = f32(beta1), f32(beta2)
    err = np.abs(np.asarray(got_rows, dtype=np.float64) - ref)
    bound = scale * (U23 * np.abs(ref) + K_ADAM * U24 * np.abs(upd))
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: Adam rows at {ratio:.3f} of their bound")
    assert np.all(err <= bound), f"{what}: Adam row off by {ratio:.3f} of its bound"
    for name, got, want, bnd in (("m", got_m, m, 2 * U23 * (np.abs(b1 * m0) + np.abs((1.0 - b1) * g))),
                                 ("v", got_v, v, 2 * U23 * (np.abs(b2 * v0) + np.abs((1.0 - b2) * g * g)))):
        e = np.abs(np.asarray(got, dtype=np.float64) - want)
        bnd = scale * bnd
        assert np.all(e <= bnd), f"{what}: Adam {name} off by {float((e / np.maximum(bnd, 1e-300)).max()):.3f} of its bound"


def rowwise_adagrad_ref(rows32, s_row32, grad32, lr, eps):
    """-> (new rows, new row state, upd), float64."""
    r, s0, g = _f64(rows32, s_row32, grad32)
    s = s0 + (g * g).sum(axis=1) / g.shape[1]
    upd = f32(lr) * g / (np.sqrt(s) + f32(eps))[:, None]
    return r - upd, s, upd


def rowwise_additions(dim, vec4):
    """A of the kernel for rows of `dim` floats on the 16-byte (vec4) or 4-byte path."""
    line = max(128, 1 << (int(dim) - 1).bit_length())
    vec = 4 if vec4 else 1
    units = line // vec
    lpr = min(units, 64)
    return (units // lpr) * vec - 1 + lpr.bit_length() - 1


def rowwise_additions_torch(dim):
    return (int(dim) - 1).bit_length()


def k_rowwise(A):
    return (A + 3 + 1) // 2 + 4


def check_rowwise_adagrad(got_rows, got_s, rows32, s_row32, grad32, lr, eps, A, what=""):
    ref, s, upd = rowwise_adagrad_ref(rows32, s_row32, grad32, lr, eps)
    K = k_rowwise(A)
    assert K <= 16
    serr = np.abs(np.asarray(got_s, dtype=np.float64) - s)
    sb = (A + 3) * U24 * s
    sratio = float((serr / np.maximum(sb, 1e-300)).max()) if serr.size else 0.0
    err = np.abs(np.asarray(got_rows, dtype=np.float64) - ref)
    bound = U23 * np.abs(ref) + K * U24 * np.abs(upd)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: row-wise state at {sratio:.3f}, rows at {ratio:.3f} of their bounds (A={A}, K={K})")
    assert np.all(serr <= sb), f"{what}: row-wise Adagrad state off by {sratio:.3f} of its bound"
    assert np.all(err <= bound), f"{what}: row-wise Adagrad row off by {ratio:.3f} of its bound"


def naive_bc2_misses(beta2, t, lr=0.05, eps=1e-8):
    """True when 1 - float32(beta2) ** t, the bias correction formed in fp32 without expm1, puts step t of a fresh row (m = v = 0)
    outside the rows bound on its own.  At t = 1 it never does: float32(beta2) ** 1 is beta2 and 1 - beta2 is exact in fp32 for
    beta2 >= 0.5 (Sterbenz), so against a reference that takes beta2 as its fp32 value the form is exact there; the digits go from
    t = 2 on, where beta2 ** t is rounded at 2^-24 and 1 - beta2 ** t is ~ t * 1e-4 (1e-3): 5e-5 (7e-6) of bc2 at t = 2."""
    g = np.array([[0.37, -2.5, 1e-3, 40.0]], dtype=np.float32)
    z = np.zeros_like(g)
    ref, m, v, upd = adam_ref(z, z, z, t, g, lr, 0.9, beta2, eps)
    bc2_naive = np.float64(np.float32(1.0) - np.float32(beta2) ** np.float32(t))
    bc1 = bias_corrections(t, 0.9)
    upd_naive = f32(lr) * (m / bc1) / (np.sqrt(v / bc2_naive) + f32(eps))
    return bool(np.any(np.abs(upd_naive - upd) > U23 * np.abs(ref) + K_ADAM * U24 * np.abs(upd)))
