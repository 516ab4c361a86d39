"""float64 one-step references of the write-through row updates (tests only), with the bounds the tests hold the fp32 code to.

Every reference works from the fp32 bytes the call itself sees -- the table rows, the state rows, the gradient, and lr / eps / alpha
as the fp32 values the C ABI receives -- so a test that snapshots table and state before every call never accumulates rounding across
steps.  The bounds allow one rounding per fp32 operation of the update:

  Adagrad row    |got - ref| <= 2^-23 |ref| + 8 * 2^-24 |upd|,   upd = lr g / (sqrt(s) + eps)
                 (g*g, the sum s, sqrt, + eps, lr*g and the division perturb upd by at most a few 2^-24 each, sqrt halving what s
                  carries; the final subtraction rounds once more, relative to the result)
  Adagrad state  |s_got - s_ref| <= 2^-23 s_ref                  (one product and one sum, or one fma)
  mode 1 (add)   |got - ref| <= 2^-23 (|alpha src| + |ref|)      (one fma, or a product and a sum)

Inputs are to stay away from denormals: |g| in [1e-4, 1e2], state 0 or in [1e-6, 1e3]."""
import numpy as np

U23 = 2.0 ** -23
U24 = 2.0 ** -24


def f32(x):
    """The fp32 value a scalar argument crosses the C ABI as, in float64."""
    return float(np.float32(x))


def adagrad_ref(rows32, state32, grad32, lr, eps):
    """-> (new rows, new state, upd), float64, from fp32 inputs."""
    r, s0, g = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (rows32, state32, grad32))
    s = s0 + g * g
    upd = f32(lr) * g / (np.sqrt(s) + f32(eps))
    return r - upd, s, upd


def check_adagrad(got_rows, got_state, rows32, state32, grad32, lr, eps, what=""):
    ref, s, upd = adagrad_ref(rows32, state32, grad32, lr, eps)
    err = np.abs(np.asarray(got_rows, dtype=np.float64) - ref)
    bound = U23 * np.abs(ref) + 8 * U24 * np.abs(upd)
    assert np.all(err <= bound), f"{what}: Adagrad row off by {float((err / np.maximum(bound, 1e-300)).max()):.3f} of its bound"
    serr = np.abs(np.asarray(got_state, dtype=np.float64) - s)
    assert np.all(serr <= U23 * s), f"{what}: Adagrad state off by {float((serr / np.maximum(U23 * s, 1e-300)).max()):.3f} of its bound"


def add_ref(rows32, src32, alpha):
    r, x = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (rows32, src32))
    return r + f32(alpha) * x, f32(alpha) * x


def check_add(got_rows, rows32, src32, alpha, what=""):
    ref, ax = add_ref(rows32, src32, alpha)
    err = np.abs(np.asarray(got_rows, dtype=np.float64) - ref)
    bound = U23 * (np.abs(ax) + np.abs(ref))
    assert np.all(err <= bound), f"{what}: added row off by {float((err / np.maximum(bound, 1e-300)).max()):.3f} of its bound"


def make_grad(rng, shape):
    """|g| log-uniform in [1e-4, 1e2], random sign, fp32."""
    mag = np.exp(rng.uniform(np.log(1e-4), np.log(1e2), size=shape))
    return (mag * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def make_state(rng, shape):
    """0 (a row never stepped) in about a third of the entries, else log-uniform in [1e-6, 1e3], fp32."""
    s = np.exp(rng.uniform(np.log(1e-6), np.log(1e3), size=shape))
    s[rng.random(size=shape) < 0.33] = 0.0
    return s.astype(np.float32)
