"""GPU tests of the block op (coala_block_mean_aggregate[_backward] in coala_block_ops.hip) against a float64 reference.

Called directly through the C ABI with hand-made int32 neighbour arrays: -1 anywhere in a row, rows without any valid entry, a
source repeated within a row, fan-outs 1..32, dims that take the 16-byte path (dim % 4 == 0, aligned buffers), the scalar path
with more than 64 units per row, and the scalar path forced at dim % 4 == 0 by buffers one float off 16-byte alignment; n_dst up
to 100,003, past the 32,768 waves of the grid.  Inputs are signed normal values with a few rows scaled by 1e6, so sums cancel.

Bounds (u = 2^-24, unit roundoff of fp32; gamma(n) = n u / (1 - n u)):
  forward   out[d] = fl(fl(x_1 + ... + x_cnt) * fl(1/cnt)): cnt - 1 roundings in the sum (the first addition to 0 is exact), one in
            1/cnt, one in the product, so |got - ref| <= gamma(cnt + 1) * sum|x_j| / cnt <= (cnt + 2) u sum|x_j| / cnt for cnt <= 32;
            a row without a valid entry is exactly 0.
  backward  grad_src[s] = sum over its k contributions of fl(g[d] * fl(1/cnt[d])), added by atomics in any order: two roundings per
            term and k - 1 in the sum, so |got - ref| <= gamma(k + 1) * sum|g[d] / cnt[d]|; a source nobody references stays 0.
Everything outside the n_dst x dim (n_src x dim) region keeps its sentinel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = np.float32(-7.25e33)
GUARD = 67                      # floats of sentinel behind every output region


def _gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def _inputs(rng, n_dst, f, n_src, dim):
    """Neighbour array (int32 [n_dst, f]) with -1 anywhere, all--1 rows and repeated sources; the last 7 sources are never
    referenced.  Signed fp32 rows [n_src, dim] and output gradients [n_dst, dim], a few rows of each scaled by 1e6."""
    nbr = rng.integers(0, n_src - 7, size=(n_dst, f)).astype(np.int32)
    nbr[rng.random((n_dst, f)) < 0.25] = -1
    rep = rng.random(n_dst) < 0.15
    nbr[rep, 0] = rng.integers(0, n_src - 7, size=int(rep.sum()))
    nbr[rep, f - 1] = nbr[rep, 0]                          # the same source twice in the row (f = 1: the entry itself)
    if n_dst:
        nbr[rng.random(n_dst) < 0.05] = -1                 # rows without any valid neighbour
        nbr[0] = -1
    x = rng.standard_normal((n_src, dim)).astype(np.float32)
    x[rng.random(n_src) < 0.03] *= np.float32(1e6)
    go = rng.standard_normal((n_dst, dim)).astype(np.float32)
    go[rng.random(n_dst) < 0.03] *= np.float32(1e6)
    return nbr, x, go


def _device(torch, arr, off, fill=None):
    """arr's values (or `fill`) at float offset `off` of a buffer padded with the sentinel before and GUARD floats after."""
    flat = torch.full((off + arr.size + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    if fill is None:
        flat[off: off + arr.size] = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).cuda()
    else:
        flat[off: off + arr.size] = fill
    return flat, flat.data_ptr() + 4 * off


def _region(flat, off, shape):
    """-> the region as a numpy array; asserts that the padding around it still holds the sentinel, bit for bit."""
    h = flat.cpu().numpy()
    n = int(np.prod(shape))
    pad = np.concatenate([h[:off], h[off + n:]])
    assert np.array_equal(pad.view(np.int32), np.full(pad.shape, SENTINEL).view(np.int32)), "write outside the output region"
    return h[off: off + n].reshape(shape)


def _check_forward(nbr, x, got):
    valid = nbr >= 0
    cnt = valid.sum(1)
    x64 = x.astype(np.float64)
    step = max(1, (1 << 22) // max(1, nbr.shape[1] * x.shape[1]))
    for lo in range(0, len(nbr), step):                    # [rows, f, dim] float64 in slices of ~32 MB
        v = valid[lo: lo + step]
        terms = x64[np.where(v, nbr[lo: lo + step], 0)] * v[..., None]
        c = np.maximum(cnt[lo: lo + step], 1)[:, None].astype(np.float64)
        ref = terms.sum(1) / c
        bound = (cnt[lo: lo + step] + 2)[:, None] * U * np.abs(terms).sum(1) / c + 1e-30
        err = np.abs(got[lo: lo + step].astype(np.float64) - ref)
        bad = ~(err <= bound)
        if bad.any():
            r, c = np.argwhere(bad)[0]
            raise AssertionError(f"forward: {bad.sum()} elements past the bound; row {lo + r} (cnt {cnt[lo + r]}) col {c}: "
                                 f"got {got[lo + r, c]!r} want {ref[r, c]!r} bound {bound[r, c]!r}, row {nbr[lo + r].tolist()}")
    assert np.all(got[cnt == 0] == 0.0), "forward: a row without valid neighbours is not exactly 0"


def _check_backward(nbr, go, n_src, got):
    import torch
    valid = nbr >= 0
    cnt = valid.sum(1)
    rows, cols = np.nonzero(valid)
    src = torch.from_numpy(nbr[rows, cols].astype(np.int64))
    k = np.bincount(nbr[rows, cols], minlength=n_src)
    ref = torch.zeros((n_src, go.shape[1]), dtype=torch.float64)
    mag = torch.zeros_like(ref)
    step = max(1, (1 << 22) // go.shape[1])
    for lo in range(0, len(rows), step):
        r = rows[lo: lo + step]
        t = torch.from_numpy(go[r].astype(np.float64) / cnt[r][:, None])
        ref.index_add_(0, src[lo: lo + step], t)
        mag.index_add_(0, src[lo: lo + step], t.abs())
    bound = _gamma(k + 1)[:, None] * mag.numpy()
    err = np.abs(got.astype(np.float64) - ref.numpy())
    bad = ~(err <= bound)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError(f"backward: {bad.sum()} elements past the bound; source row {r} (k {k[r]}) col {c}: got {got[r, c]!r} "
                             f"want {ref[r, c].item()!r} bound {bound[r, c]!r}")
    assert np.all(got[k == 0] == 0.0), "backward: a source nobody references is not exactly 0"


DIMS = [1, 3, 4, 63, 64, 65, 129, 257, 1000, 1024, 2048]
FANS = [1, 15, 16, 31, 32]
CASES = [(517, FANS[(i + off) % 5], dim, off) for i, dim in enumerate(DIMS) for off in (0, 1)]
CASES += [(0, 16, 64, 0), (1, 32, 4, 1), (2, 1, 3, 0), (32_768, 15, 4, 0), (32_769, 31, 65, 1), (100_003, 32, 4, 0),
          (100_003, 16, 3, 1), (100_003, 1, 256, 0), (100_003, 31, 64, 1)]


@pytest.mark.parametrize("n_dst,f,dim,off", CASES)
def test_mean_aggregate_against_float64(hiplib, n_dst, f, dim, off):
    """Forward and backward through the C ABI; off = 1 puts every float buffer one float off 16-byte alignment (scalar path)."""
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    rng = np.random.default_rng(n_dst * 131 + f * 7 + dim + off)
    n_src = max(64, min(5000, n_dst // 4))
    nbr, x, go = _inputs(rng, n_dst, f, n_src, dim)
    d_nbr = torch.from_numpy(nbr).cuda()
    h_buf, h_ptr = _device(torch, x, off)
    out_buf, out_ptr = _device(torch, np.empty((n_dst, dim), np.float32), off, fill=float(SENTINEL))
    _capi.check(L.coala_block_mean_aggregate(0, d_nbr.data_ptr(), h_ptr, out_ptr, n_dst, f, dim, current_stream()))
    _check_forward(nbr, x, _region(out_buf, off, (n_dst, dim)))
    g_buf, g_ptr = _device(torch, go, off)
    gs_buf, gs_ptr = _device(torch, np.empty((n_src, dim), np.float32), off, fill=0.0)   # the caller zeroes grad_src
    _capi.check(L.coala_block_mean_aggregate_backward(0, d_nbr.data_ptr(), g_ptr, gs_ptr, n_dst, f, dim, current_stream()))
    _check_backward(nbr, go, n_src, _region(gs_buf, off, (n_src, dim)))
    assert np.array_equal(_region(h_buf, off, (n_src, dim)), x) and np.array_equal(_region(g_buf, off, (n_dst, dim)), go)


@pytest.mark.parametrize("f,dim", [(32, 1024), (16, 65), (1, 3), (31, 4), (15, 129)])
def test_block_mean_aggregate_autograd_against_float64(hiplib, f, dim):
    """Block.mean_aggregate with autograd on hand-made blocks: the forward and the gradient of sum(out * w) (which is w / cnt
    scattered to the sources) within the same bounds."""
    import torch
    from COALA_GNN.sampler import Block
    rng = np.random.default_rng(f * 1000 + dim)
    n_dst, n_src = 3001, 800
    nbr, x, w = _inputs(rng, n_dst, f, n_src, dim)
    b = Block(torch.arange(n_src, device="cuda"), torch.from_numpy(nbr).cuda(), n_dst)
    h = torch.from_numpy(x).cuda().requires_grad_(True)
    out = b.mean_aggregate(h)
    _check_forward(nbr, x, out.detach().cpu().numpy())
    (out * torch.from_numpy(w).cuda()).sum().backward()
    _check_backward(nbr, w, n_src, h.grad.cpu().numpy())


def test_mean_aggregate_refuses_bad_shapes(hiplib):
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    nbr = torch.zeros(64, dtype=torch.int32, device="cuda")
    a = torch.zeros(64 * 4, device="cuda")
    b = torch.full((64 * 4,), float(SENTINEL), device="cuda")
    for fn in (L.coala_block_mean_aggregate, L.coala_block_mean_aggregate_backward):
        for n_dst, f, dim in ((1, 0, 4), (1, 33, 4), (1, 4, 0), (-1, 4, 4), (0, 33, 4)):
            with pytest.raises(RuntimeError, match="bad block shape"):
                _capi.check(fn(0, nbr.data_ptr(), a.data_ptr(), b.data_ptr(), n_dst, f, dim, current_stream()))
    torch.cuda.synchronize()
    assert torch.all(b == float(SENTINEL))
