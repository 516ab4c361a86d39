"""GPU tests of the weighted sum aggregation (coala_block_weighted_sum[_backward][_csr] in coala_block_ops.hip,
Block.weighted_sum_aggregate) against a float64 reference.

Bounds, as in test_block_ops_gpu.py (u = 2^-24, gamma(n) = n u / (1 - n u), imported from there):
  forward   out[d, c] = sum of cnt terms w_j x[s_j, c], added in slot order with one fma (or a product and an addition) each: a term
            passes at most cnt roundings, so |got - ref| <= gamma(cnt) sum|w_j x_j|; gamma(cnt + 1) is asserted, the form of that
            file's backward bound.  A row without a valid entry is exactly 0.
  grad_src  grad_src[s, c] = sum over the k edges landing on s of fl(w_j g[d, c]), added by atomics in any order: one rounding per
            product and at most k - 1 in the sum, |got - ref| <= gamma(k + 1) sum|w_j g|; a source nobody references stays 0.
  grad_w    grad_w[d, j] = <g[d, :], x[s_j, :]>, dim terms: a lane adds its share with fmas (at most ceil(dim / 64) roundings, four
            times that on the 16-byte path) and a butterfly over 64 lanes adds at most 6 more, additions of an exact 0 being exact: a
            term passes at most dim + 1 roundings for every dim, so |got - ref| <= gamma(dim + 1) sum|g_c x_c|; 0 on a padding slot.
Everything outside an output region keeps its sentinel."""
import numpy as np
import pytest

from _util import Guarded
from test_block_ops_gpu import U, _gamma

pytestmark = pytest.mark.gpu


def _dense_inputs(rng, n_dst, f, n_src, dim):
    """nbr int32 [n_dst, f] with -1 anywhere, rows without a valid entry and repeated sources (the last 7 sources unreferenced);
    signed weights with zeros; signed rows and output gradients, a few rows of each scaled by 1e6 so that sums cancel."""
    nbr = rng.integers(0, n_src - 7, size=(n_dst, f)).astype(np.int32)
    nbr[rng.random((n_dst, f)) < 0.25] = -1
    rep = rng.random(n_dst) < 0.15
    nbr[rep, 0] = rng.integers(0, n_src - 7, size=int(rep.sum()))
    nbr[rep, f - 1] = nbr[rep, 0]
    nbr[rng.random(n_dst) < 0.05] = -1
    nbr[0] = -1
    w = rng.standard_normal((n_dst, f)).astype(np.float32)
    w[rng.random((n_dst, f)) < 0.1] = 0
    x = rng.standard_normal((n_src, dim)).astype(np.float32)
    x[rng.random(n_src) < 0.03] *= np.float32(1e6)
    go = rng.standard_normal((n_dst, dim)).astype(np.float32)
    go[rng.random(n_dst) < 0.03] *= np.float32(1e6)
    return nbr, w, x, go


def _edge_list(nbr=None, indptr=None, idx=None):
    """(row, slot in the flat weight array, source) of every valid edge of either block form"""
    if nbr is not None:
        rows, cols = np.nonzero(nbr >= 0)
        return rows, rows * nbr.shape[1] + cols, nbr[rows, cols].astype(np.int64)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    keep = idx >= 0
    return rows[keep], np.flatnonzero(keep), idx[keep].astype(np.int64)


def _check(rows, slots, srcs, w, x, go, n_dst, got_out, got_gs, got_gw, what):
    """All three outputs against float64, element by element, within the bounds of the module docstring.  Each got_* may be None."""
    import torch
    dim, n_src = x.shape[1], x.shape[0]
    wf = w.reshape(-1).astype(np.float64)
    t_rows, t_src = torch.from_numpy(rows), torch.from_numpy(srcs)
    cnt = np.bincount(rows, minlength=n_dst)
    k = np.bincount(srcs, minlength=n_src)
    step = max(1, (1 << 21) // dim)
    ref_o, mag_o = torch.zeros((n_dst, dim), dtype=torch.float64), torch.zeros((n_dst, dim), dtype=torch.float64)
    ref_s, mag_s = torch.zeros((n_src, dim), dtype=torch.float64), torch.zeros((n_src, dim), dtype=torch.float64)
    ref_w, mag_w = np.zeros(w.size), np.zeros(w.size)
    for lo in range(0, len(rows), step):
        sl = slice(lo, lo + step)
        xs, gs, ws = x[srcs[sl]].astype(np.float64), go[rows[sl]].astype(np.float64), wf[slots[sl]][:, None]
        t = torch.from_numpy(ws * xs)
        ref_o.index_add_(0, t_rows[sl], t), mag_o.index_add_(0, t_rows[sl], t.abs())
        t = torch.from_numpy(ws * gs)
        ref_s.index_add_(0, t_src[sl], t), mag_s.index_add_(0, t_src[sl], t.abs())
        ref_w[slots[sl]], mag_w[slots[sl]] = (gs * xs).sum(1), np.abs(gs * xs).sum(1)
    for name, got, ref, bound, zero in (("forward", got_out, ref_o.numpy(), _gamma(cnt + 1)[:, None] * mag_o.numpy(), cnt == 0),
                                        ("grad_src", got_gs, ref_s.numpy(), _gamma(k + 1)[:, None] * mag_s.numpy(), k == 0),
                                        ("grad_w", got_gw, ref_w, _gamma(dim + 1) * mag_w, mag_w == 0)):
        if got is None:
            continue
        got = got.reshape(ref.shape)
        err = np.abs(got.astype(np.float64) - ref)
        bad = ~(err <= bound + 1e-30)
        if bad.any():
            at = tuple(np.argwhere(bad)[0])
            raise AssertionError(f"{what} {name}: {bad.sum()} elements past the bound; at {at}: got {got[at]!r} want {ref[at]!r} "
                                 f"bound {bound[at]!r}")
        if name != "grad_w":
            assert np.all(got[zero] == 0.0), f"{what} {name}: a row nothing is added to is not exactly 0"
    if got_gw is not None:
        pad = np.ones(w.size, dtype=bool)
        pad[slots] = False
        assert np.all(got_gw.reshape(-1)[pad] == 0.0), f"{what}: grad_w of a padding slot is not 0"


def _run_dense(L, torch, nbr, w, x, go, off, want_src=True, want_w=True):
    from COALA_GNN_Pybind import _capi, current_stream
    n_dst, f = nbr.shape
    n_src, dim = x.shape
    d_nbr = torch.from_numpy(nbr).cuda()
    gw_, gx, gg = Guarded(torch, n_dst, f, off, w), Guarded(torch, n_src, dim, off, x), Guarded(torch, n_dst, dim, off, go)
    out, gs, gwo = Guarded(torch, n_dst, dim, off), Guarded(torch, n_src, dim, off, 0.0), Guarded(torch, n_dst, f, off)
    _capi.check(L.coala_block_weighted_sum(0, d_nbr.data_ptr(), gw_.ptr, gx.ptr, out.ptr, n_dst, f, dim, current_stream()))
    _capi.check(L.coala_block_weighted_sum_backward(0, d_nbr.data_ptr(), gw_.ptr, gx.ptr, gg.ptr, gs.ptr if want_src else None,
                                                    gwo.ptr if want_w else None, n_dst, f, dim, current_stream()))
    torch.cuda.synchronize()
    assert np.array_equal(gw_.region(), w) and np.array_equal(gx.region(), x) and np.array_equal(gg.region(), go), "an input changed"
    return out.region(), gs.region(), gwo.region()


def _run_csr(L, torch, indptr, idx, w, x, go, off):
    from COALA_GNN_Pybind import _capi, current_stream
    n_dst, E = len(indptr) - 1, len(idx)
    n_src, dim = x.shape
    d_ip, d_idx = torch.from_numpy(indptr).cuda(), torch.from_numpy(idx).cuda()
    gw_, gx, gg = Guarded(torch, 1, E, off, w), Guarded(torch, n_src, dim, off, x), Guarded(torch, n_dst, dim, off, go)
    out, gs, gwo = Guarded(torch, n_dst, dim, off), Guarded(torch, n_src, dim, off, 0.0), Guarded(torch, 1, E, off)
    _capi.check(L.coala_block_weighted_sum_csr(0, d_ip.data_ptr(), d_idx.data_ptr(), gw_.ptr, gx.ptr, out.ptr, n_dst, dim, current_stream()))
    _capi.check(L.coala_block_weighted_sum_csr_backward(0, d_ip.data_ptr(), d_idx.data_ptr(), gw_.ptr, gx.ptr, gg.ptr, gs.ptr, gwo.ptr, n_dst, dim,
                                                        current_stream()))
    torch.cuda.synchronize()
    return out.region(), gs.region(), gwo.region().reshape(-1)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dim", [1, 100, 128, 1024])
@pytest.mark.parametrize("f", [1, 5, 32])
def test_weighted_sum_dense_against_float64(hiplib, f, dim, off):
    """Through the C ABI; off = 1 puts every float buffer one float off 16-byte alignment (the scalar path at dim % 4 == 0)."""
    import torch
    from COALA_GNN_Pybind import _capi
    rng = np.random.default_rng(f * 4099 + dim * 3 + off)
    n_dst, n_src = 2053, 400
    nbr, w, x, go = _dense_inputs(rng, n_dst, f, n_src, dim)
    out, gs, gw = _run_dense(_capi.load(), torch, nbr, w, x, go, off)
    _check(*_edge_list(nbr=nbr), w, x, go, n_dst, out, gs, gw, f"dense f={f} dim={dim} off={off}")


def _csr_inputs(rng, n_dst, n_src, dim, long_row):
    deg = rng.integers(0, 40, size=n_dst)
    deg[rng.random(n_dst) < 0.1] = 0
    deg[n_dst // 2] = long_row
    indptr = np.zeros(n_dst + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    E = int(indptr[-1])
    idx = rng.integers(0, n_src - 7, size=E).astype(np.int32)
    w = rng.standard_normal(E).astype(np.float32)
    w[rng.random(E) < 0.1] = 0
    x = rng.standard_normal((n_src, dim)).astype(np.float32)
    x[rng.random(n_src) < 0.03] *= np.float32(1e6)
    go = rng.standard_normal((n_dst, dim)).astype(np.float32)
    go[rng.random(n_dst) < 0.03] *= np.float32(1e6)
    return indptr, idx, w, x, go


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dim", [1, 100, 128, 1024])
def test_weighted_sum_ragged_against_float64(hiplib, dim, off):
    """A ragged block with empty rows and one row of 3001 edges (47 chunks of 64, the last one partial)."""
    import torch
    from COALA_GNN_Pybind import _capi
    rng = np.random.default_rng(dim * 7 + off)
    n_dst, n_src = 301, 500
    indptr, idx, w, x, go = _csr_inputs(rng, n_dst, n_src, dim, 3001)
    out, gs, gw = _run_csr(_capi.load(), torch, indptr, idx, w, x, go, off)
    _check(*_edge_list(indptr=indptr, idx=idx), w, x, go, n_dst, out, gs, gw, f"ragged dim={dim} off={off}")


@pytest.mark.parametrize("f,dim,off", [(5, 128, 0), (32, 100, 0), (1, 1, 0), (32, 1024, 1), (17, 64, 0)])
def test_dense_and_ragged_forms_give_the_same_bits(hiplib, f, dim, off):
    """The same rows in both forms (the ragged one drops the -1 slots): forward and grad_w equal bit for bit."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(f + dim)
    n_dst, n_src = 1031, 300
    nbr, w, x, go = _dense_inputs(rng, n_dst, f, n_src, dim)
    valid = nbr >= 0
    indptr = np.zeros(n_dst + 1, dtype=np.int64)
    np.cumsum(valid.sum(1), out=indptr[1:])
    a_out, _, a_gw = _run_dense(L, torch, nbr, w, x, go, off)
    b_out, _, b_gw = _run_csr(L, torch, indptr, nbr[valid], w[valid], x, go, off)
    assert np.array_equal(a_out.view(np.int32), b_out.view(np.int32)), "forward differs between the dense and the ragged form"
    assert np.array_equal(a_gw[valid].view(np.int32), b_gw.view(np.int32)), "grad_w differs between the dense and the ragged form"


@pytest.mark.parametrize("f,dim", [(5, 128), (32, 100), (1, 64)])
def test_unit_weights_equal_mean_times_degree_and_no_grad_w_unless_asked(hiplib, f, dim):
    """Block API with autograd.  Weights of 1: the weighted sum S and the mean M of the same row satisfy |S - M cnt| <=
    (gamma(cnt + 1) + (cnt + 2) u + 2 u) sum|x_j| -- S's bound, cnt times the mean's bound ((cnt + 2) u sum|x_j| / cnt,
    test_block_ops_gpu.py) and the rounding of the product M * cnt, on |M| cnt <= (1 + (cnt + 2) u) sum|x_j|.  The weights do not
    require a gradient here: none is made, and grad_src is still within its bound."""
    import torch
    from COALA_GNN.sampler import Block
    rng = np.random.default_rng(f * 31 + dim)
    n_dst, n_src = 1500, 400
    nbr, _, x, go = _dense_inputs(rng, n_dst, f, n_src, dim)
    b = Block(torch.arange(n_src, device="cuda"), torch.from_numpy(nbr).cuda(), n_dst)
    h = torch.from_numpy(x).cuda().requires_grad_(True)
    ones = torch.ones(n_dst, f, device="cuda")
    s = b.weighted_sum_aggregate(h, ones)
    m = b.mean_aggregate(h.detach())
    cnt = (nbr >= 0).sum(1)
    mag = (np.abs(x.astype(np.float64))[np.maximum(nbr, 0)] * (nbr >= 0)[..., None]).sum(1)
    bound = (_gamma(cnt + 1) + (cnt + 4) * U)[:, None] * mag + 1e-30
    md = (m * torch.from_numpy(cnt).cuda().to(torch.float32).unsqueeze(-1)).cpu().numpy().astype(np.float64)
    assert np.all(np.abs(s.detach().cpu().numpy().astype(np.float64) - md) <= bound)
    (s * torch.from_numpy(go).cuda()).sum().backward()
    assert ones.grad is None
    rows, slots, srcs = _edge_list(nbr=nbr)
    _check(rows, slots, srcs, np.ones((n_dst, f), np.float32), x, go, n_dst, s.detach().cpu().numpy(), h.grad.cpu().numpy(), None, "unit weights")
    # both gradients through autograd, and the weight's alone
    w = torch.randn(n_dst, f, device="cuda", requires_grad=True)
    h2 = torch.from_numpy(x).cuda().requires_grad_(True)
    (b.weighted_sum_aggregate(h2, w) * torch.from_numpy(go).cuda()).sum().backward()
    _check(rows, slots, srcs, w.detach().cpu().numpy(), x, go, n_dst, None, h2.grad.cpu().numpy(), w.grad.cpu().numpy(), "autograd")
    w2 = w.detach().clone().requires_grad_(True)
    (b.weighted_sum_aggregate(h2.detach(), w2) * torch.from_numpy(go).cuda()).sum().backward()
    assert torch.equal(w2.grad, w.grad), "grad_w changes when grad_src is not asked for"


def test_native_op_agrees_with_the_torch_fallback(hiplib):
    """Both block forms: the native forward and gradients against weighted_sum_aggregate_torch in float64 on the CPU."""
    import torch
    from COALA_GNN.sampler import Block
    rng = np.random.default_rng(3)
    n_dst, n_src, f, dim = 700, 250, 9, 36
    nbr, w, x, go = _dense_inputs(rng, n_dst, f, n_src, dim)
    indptr, idx, wc, _, _ = _csr_inputs(rng, n_dst, n_src, dim, 200)
    for kw, wv in ((dict(nbr=torch.from_numpy(nbr)), w), (dict(nbr=None, indptr=torch.from_numpy(indptr), indices=torch.from_numpy(idx)), wc)):
        cpu = Block(torch.arange(n_src), kw.pop("nbr"), n_dst, **kw)
        gpu = Block(torch.arange(n_src, device="cuda"), None if cpu.nbr is None else cpu.nbr.cuda(), n_dst,
                    **{k: v.cuda() for k, v in kw.items()})
        h64, w64 = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(wv).double().requires_grad_(True)
        ref = cpu.weighted_sum_aggregate(h64, w64)
        (ref * torch.from_numpy(go).double()).sum().backward()
        h, wt = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(wv).cuda().requires_grad_(True)
        out = gpu.weighted_sum_aggregate(h, wt)
        (out * torch.from_numpy(go).cuda()).sum().backward()
        rows, slots, srcs = _edge_list(nbr=nbr) if cpu.nbr is not None else _edge_list(indptr=indptr, idx=idx)
        _check(rows, slots, srcs, wv, x, go, n_dst, out.detach().cpu().numpy(), h.grad.cpu().numpy(), wt.grad.cpu().numpy(), "native")
        # the fallback itself is the float64 reference of _check, to float64 rounding
        _check(rows, slots, srcs, wv, x, go, n_dst, ref.detach().numpy(), h64.grad.numpy(), w64.grad.numpy(), "fallback")


def test_weighted_sum_refuses_bad_shapes(hiplib):
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    from _util import SENTINEL
    L = _capi.load()
    nbr = torch.zeros(64, dtype=torch.int32, device="cuda")
    ip = torch.zeros(65, dtype=torch.int64, device="cuda")
    a = torch.zeros(64 * 4, device="cuda")
    b = torch.full((64 * 4,), float(SENTINEL), device="cuda")
    st = current_stream()
    for n_dst, f, dim in ((1, 0, 4), (1, 33, 4), (1, 4, 0), (-1, 4, 4), (0, 33, 4)):
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_weighted_sum(0, nbr.data_ptr(), a.data_ptr(), a.data_ptr(), b.data_ptr(), n_dst, f, dim, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_weighted_sum_backward(0, nbr.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), b.data_ptr(), b.data_ptr(),
                                                            n_dst, f, dim, st))
    for n_dst, dim in ((1, 0), (-1, 4)):
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_weighted_sum_csr(0, ip.data_ptr(), nbr.data_ptr(), a.data_ptr(), a.data_ptr(), b.data_ptr(), n_dst, dim, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_weighted_sum_csr_backward(0, ip.data_ptr(), nbr.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(),
                                                                b.data_ptr(), b.data_ptr(), n_dst, dim, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_weighted_sum(0, nbr.data_ptr(), None, a.data_ptr(), b.data_ptr(), 4, 4, 4, st))
    from COALA_GNN.sampler import Block
    blk = Block(torch.arange(8, device="cuda"), torch.zeros((4, 3), dtype=torch.int32, device="cuda"), 4)
    with pytest.raises(ValueError, match="one per neighbour slot"):
        blk.weighted_sum_aggregate(torch.zeros(8, 4, device="cuda"), torch.zeros(4, 2, device="cuda"))
    torch.cuda.synchronize()
    assert torch.all(b == float(SENTINEL))
