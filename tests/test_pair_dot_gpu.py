"""GPU tests of the pair scores (coala_block_pair_dot / _backward, block_ops.pair_dot): out[p, hd] = <h[src_p, hd], h[dst_p, hd]>.

At the C ABI on Guarded buffers with h one float off 16-byte alignment, against float64 with the bounds of test_weighted_sum_gpu.py:
forward |err| <= gamma(D + 1) sum |h_u h_v| (D products, each rounded once at most, and D - 1 additions); grad_h |err| <= gamma(m + 1)
sum |terms|, m the number of pair endpoints that land on the row (one rounded product per term, m - 1 additions of the atomics in any
order).  Rows that no pair references get a gradient of exactly 0, pairs with a -1 index score exactly 0 and add nothing."""
import numpy as np
import pytest

from _util import Guarded
from test_block_ops_gpu import _gamma

pytestmark = pytest.mark.gpu

N = 400
UNREFERENCED = 10     # the last rows of h: no pair names them


def _pairs(rng, P):
    top = N - UNREFERENCED
    src, dst = rng.integers(0, top, size=P).astype(np.int32), rng.integers(0, top, size=P).astype(np.int32)
    if P >= 65:
        src[5], dst[5] = 9, 9                                  # u == v
        src[6:9], dst[6:9] = 11, 12                            # a repeated pair
        src[10], dst[11], src[12], dst[12] = -1, -1, -1, -1    # pairs without a score
    if P >= 6144:
        dst[1000:1300] = 17                                    # one row 300 times
        src[1300:1400] = 3                                     # ... and a scaled row 100 times
    return src, dst


def _reference(h, src, dst, g):
    """float64: (out [P, H], its magnitude, grad_h [N, H, D], its magnitude, endpoints per row)"""
    ok = (src >= 0) & (dst >= 0)
    a, b = np.where(ok, src, 0), np.where(ok, dst, 0)
    hd = h.astype(np.float64)
    prod = hd[a] * hd[b] * ok[:, None, None]
    grad, mag, m = np.zeros_like(hd), np.zeros_like(hd), np.zeros(N, dtype=np.int64)
    ga, gb = g[:, :, None] * hd[b] * ok[:, None, None], g[:, :, None] * hd[a] * ok[:, None, None]
    for rows, t in ((a, ga), (b, gb)):
        np.add.at(grad, rows, t)
        np.add.at(mag, rows, np.abs(t))
        np.add.at(m, rows[ok], 1)
    return prod.sum(-1), np.abs(prod).sum(-1), grad, mag, m


def _check_case(torch, L, rng, d_h, h, src, dst, D, H):
    """One forward and one backward call at the C ABI over the given pairs, held to the bounds of the module docstring; -> endpoints per
    row of h."""
    from COALA_GNN_Pybind import _capi, current_stream
    heads, P = H or 1, len(src)
    g = rng.standard_normal((P, heads)).astype(np.float32)
    d_s, d_d = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    d_out = Guarded(torch, P, heads, off=3)
    d_g = Guarded(torch, P, heads, off=1, fill=g) if P else Guarded(torch, 0, heads)
    d_gh = Guarded(torch, N, heads * D, off=1, fill=0.0)
    _capi.check(L.coala_block_pair_dot(0, d_h.ptr, d_s.data_ptr(), d_d.data_ptr(), d_out.ptr, P, heads, D, current_stream()))
    _capi.check(L.coala_block_pair_dot_backward(0, d_h.ptr, d_s.data_ptr(), d_d.data_ptr(), d_g.ptr, d_gh.ptr, P, heads, D, current_stream()))
    torch.cuda.synchronize()
    out, gh = d_out.region().astype(np.float64), d_gh.region().reshape(N, heads, D)
    d_h.region()                                            # the input's padding too
    ref, mag, gref, gmag, m = _reference(h, src, dst, g.astype(np.float64))
    err = np.abs(out - ref)
    bound = _gamma(D + 1) * mag
    print(f"D={D} H={H} P={P}: forward worst err/bound {float((err / np.maximum(bound, 1e-300)).max()) if P else 0:.3f}")
    assert np.all(err <= bound)
    none = (src < 0) | (dst < 0)
    assert np.all(out[none] == 0)
    gerr = np.abs(gh.astype(np.float64) - gref)
    gbound = _gamma(m + 1)[:, None, None] * gmag
    print(f"D={D} H={H} P={P}: grad_h worst err/bound {float((gerr / np.maximum(gbound, 1e-300)).max()):.3f}")
    assert np.all(gerr <= gbound)
    assert np.all(gh[m == 0] == 0) and np.all(m[N - UNREFERENCED:] == 0)
    if P:                                                   # bitwise reproducible forward
        d_out2 = Guarded(torch, P, heads, off=0)
        _capi.check(L.coala_block_pair_dot(0, d_h.ptr, d_s.data_ptr(), d_d.data_ptr(), d_out2.ptr, P, heads, D, current_stream()))
        assert d_out2.region().tobytes() == d_out.region().tobytes()
    return m


def _table(torch, rng, D, heads):
    h = rng.standard_normal((N, heads, D)).astype(np.float32)
    h[[3, 50, 51]] *= np.float32(1e6)
    d_h = Guarded(torch, N, heads * D, off=1, fill=h.reshape(N, -1))
    assert d_h.ptr % 16 == 4
    return h, d_h


@pytest.mark.parametrize("H", [None, 1, 4])
@pytest.mark.parametrize("D", [1, 3, 64, 100, 128, 257])
def test_pair_dot_abi(hiplib, D, H):
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    heads = H or 1
    rng = np.random.default_rng(1000 * D + heads)
    h, d_h = _table(torch, rng, D, heads)
    for P in (0, 1, 65, 6144):
        src, dst = _pairs(rng, P)
        m = _check_case(torch, L, rng, d_h, h, src, dst, D, H)
        if P >= 6144:
            assert m[17] >= 300 and m[3] >= 100


GRID_THREADS = 8192 * 256      # the largest grid of the pair kernels (coala_block_ops.hip: pair_dot_launch)


def _pairs_past_the_grid(rng, P, heads, GS):
    """_pairs' specials scaled to P pairs: one row named 3,000 times, and the pairs without a score placed behind unit GRID_THREADS / GS,
    where only the second pass of the grid-stride loop meets them."""
    src, dst = _pairs(rng, P)
    first_pass = GRID_THREADS // GS // heads                # pairs the first pass covers
    assert P > first_pass + 8
    dst[P - 3100: P - 100] = 17                             # one row 3,000 times, most of it in the second pass
    src[P - 100: P - 40] = 3                                # ... and a scaled row
    src[first_pass + 1], dst[first_pass + 2] = -1, -1
    src[P - 5], dst[P - 3], src[P - 1], dst[P - 1] = -1, -1, -1, -1
    return src, dst


@pytest.mark.parametrize("D,H,P,GS", [(64, 1, 40_000, 64), (24, 1, 70_001, 32), (3, 4, 35_003, 16)])
def test_pair_dot_past_one_grid_pass(hiplib, D, H, P, GS):
    """More (pair, head) units than lane groups in the largest grid, for each group size: the units of the second pass of the
    grid-stride loop, forward and backward, on the same reference and bounds."""
    import torch
    from COALA_GNN_Pybind import _capi
    assert P * H * GS > GRID_THREADS and GS == (16 if D <= 16 else 32 if D <= 32 else 64)
    rng = np.random.default_rng(P)
    h, d_h = _table(torch, rng, D, H)
    src, dst = _pairs_past_the_grid(rng, P, H, GS)
    m = _check_case(torch, _capi.load(), rng, d_h, h, src, dst, D, H)
    assert m[17] >= 2990 and m[3] >= 60 and ((src < 0) | (dst < 0))[GRID_THREADS // GS // H:].sum() >= 5


INPUTS = ("native", "colslice", "int64", "fp64", "fp16", "cpu_index")


@pytest.mark.parametrize("H", [None, 4])
@pytest.mark.parametrize("inp", INPUTS)
def test_pair_dot_dispatch_parity(hiplib, inp, H, monkeypatch):
    """Whatever path an input takes -- the kernels or pair_dot_torch -- the result has the shape, dtype and values of pair_dot_torch in
    float64 on the CPU, and so has the gradient (the tolerance of tests/_dispatch_parity.py)."""
    import torch
    from COALA_GNN import block_ops
    from _dispatch_parity import UNIT
    D, P = 24, 500
    rng = np.random.default_rng(INPUTS.index(inp) * 10 + (H or 0))
    shape = (N, D) if H is None else (N, H, D)
    dtype = {"fp64": torch.float64, "fp16": torch.float16}.get(inp, torch.float32)
    base = torch.from_numpy(rng.standard_normal(shape[:-1] + (D + 8,)).astype(np.float32)).to(dtype)
    view = (lambda t: t[..., 3: 3 + D]) if inp == "colslice" else (lambda t: t[..., :D].contiguous())
    src, dst = (torch.from_numpy(a.astype(np.int64 if inp == "int64" else np.int32)) for a in _pairs(rng, P))
    calls = []
    real = block_ops._PairDot.apply
    monkeypatch.setattr(block_ops._PairDot, "apply", staticmethod(lambda *a: calls.append(1) or real(*a)))
    h = view(base.cuda()).requires_grad_()
    idx_dev = "cpu" if inp == "cpu_index" else "cuda"
    got = block_ops.pair_dot(h, src.to(idx_dev), dst.to(idx_dev))
    assert bool(calls) == (inp in ("native", "colslice", "int64")), "the wrong path ran"
    w = torch.from_numpy(rng.standard_normal(tuple(got.shape)).astype(np.float32))
    (got * w.cuda().to(dtype)).sum().backward()
    h64 = view(base).double().requires_grad_()
    want = block_ops.pair_dot_torch(h64, src, dst)
    (want * w.double()).sum().backward()
    hlow = view(base).clone().requires_grad_()
    try:
        low = block_ops.pair_dot_torch(hlow, src, dst)
        (low * w.to(dtype)).sum().backward()
        low, glow = low.detach().double(), hlow.grad.double()
    except RuntimeError:
        low = glow = None
    assert tuple(got.shape) == tuple(want.shape) == ((P,) if H is None else (P, H)) and got.dtype == dtype
    for name, a, b, lo in (("out", got.detach(), want.detach(), low), ("grad_h", h.grad, h64.grad, glow)):
        e = float((lo - b).abs().max()) if lo is not None else 0.0
        tol = max(4.0 * e, 8.0 * UNIT[dtype] * float(b.abs().max()))
        err = float((a.double().cpu() - b).abs().max())
        print(f"{inp} H={H} {name}: error {err:.3e} E {e:.3e} bound {tol:.3e}")
        assert err <= tol
    with pytest.raises(IndexError):
        block_ops.pair_dot(h.detach(), torch.tensor([N], device="cuda"), torch.tensor([0], device="cuda"))
