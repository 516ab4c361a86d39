"""GPU tests of the typed linear step (coala_block_gather_mm*, block_ops.gather_mm, nn.TypedLinear):
y[i] = x[rows[i]] @ op(W[types[i]]).  At the C ABI on Guarded buffers one float off 16-byte alignment, against float64 numpy, u = 2^-24:
forward |err| <= gamma(in + 1) sum |x w| (a chain of fused multiply-adds in any order); grad_W |err| <= gamma(m_t + 1) sum |x g|, m_t the
rows of the type; grad_x |err| <= gamma(out + c) sum |g w|, c the rows that name the source.  Exact: zeros for rows that send nothing,
for sources no row names and types no row has, the padding; the forward's bits when it runs twice, when the list is permuted and when
the other rows change; the plan against a stable numpy sort."""
import copy

import numpy as np
import pytest

from _util import Guarded
from test_block_ops_gpu import _gamma

pytestmark = pytest.mark.gpu
N = 400               # rows of x when rows= is given; the last 10 are named by no entry


def _types(rng, sizes, T, n_bad=4):
    """A shuffled type list with sizes[t] rows of type t, plus n_bad rows each of the types -1 and T."""
    return rng.permutation(np.concatenate([np.full(c, ty) for ty, c in enumerate(sizes)] + [np.full(n_bad, -1), np.full(n_bad, T)]).astype(np.int32))


def _rows(rng, M):
    r = rng.integers(0, N - 10, size=M).astype(np.int32)
    if M > 320:
        r[rng.permutation(M)[:300]] = 17          # one source about 300 times
        r[[5, 77, 200]] = -1
    return r


def _reference(x, W, types, rows, transposed, g):
    """float64: y, its magnitude, grad_x, its magnitude, rows per source, grad_W (in W's layout), its magnitude, rows per type, who sends"""
    T = W.shape[0]
    Wm = (W.transpose(0, 2, 1) if transposed else W).astype(np.float64)
    ok = (types >= 0) & (types < T) & (True if rows is None else rows >= 0)
    a = np.where(ok, np.arange(len(types)) if rows is None else rows, 0)
    xa, Wt, gk = x.astype(np.float64)[a] * ok[:, None], Wm[np.where(ok, types, 0)], g.astype(np.float64) * ok[:, None]
    y, ymag = np.einsum("mi,mio->mo", xa, Wt), np.einsum("mi,mio->mo", np.abs(xa), np.abs(Wt))
    gx, gxmag, c = np.zeros(x.shape), np.zeros(x.shape), np.zeros(x.shape[0], dtype=np.int64)
    np.add.at(gx, a, np.einsum("mo,mio->mi", gk, Wt))
    np.add.at(gxmag, a, np.einsum("mo,mio->mi", np.abs(gk), np.abs(Wt)))
    np.add.at(c, a[ok], 1)
    gw, gwmag, mt = np.zeros(Wm.shape), np.zeros(Wm.shape), np.bincount(types[ok], minlength=T)
    np.add.at(gw, types[ok], xa[ok][:, :, None] * gk[ok][:, None, :])
    np.add.at(gwmag, types[ok], np.abs(xa[ok][:, :, None] * gk[ok][:, None, :]))
    back = (lambda v: v.transpose(0, 2, 1)) if transposed else (lambda v: v)
    return y, ymag, gx, gxmag, c, back(gw), back(gwmag), mt, ok


def _launch(torch, L, d_x, d_W, types, rows, transposed, T, K, Nout, off, g=None):
    """plan + forward (+ both backward kernels with g) at the C ABI -> [y, order, seg(, grad_x, grad_W)] as numpy, padding checked"""
    from COALA_GNN_Pybind import _capi, current_stream
    M, st = len(types), current_stream()
    d_t, d_r = torch.from_numpy(types).cuda(), None if rows is None else torch.from_numpy(rows).cuda()
    rp = None if rows is None else d_r.data_ptr()
    order, seg = torch.full((M,), -9, dtype=torch.int32, device="cuda"), torch.full((T + 1,), -9, dtype=torch.int32, device="cuda")
    work = torch.empty(max(L.coala_block_gather_mm_plan_work(M, T), 1), dtype=torch.int32, device="cuda")
    d_y = Guarded(torch, M, Nout, off=off)
    _capi.check(L.coala_block_gather_mm_plan(0, d_t.data_ptr(), rp, M, T, order.data_ptr(), seg.data_ptr(), work.data_ptr(), st))
    _capi.check(L.coala_block_gather_mm(0, d_x.ptr, d_W.ptr, order.data_ptr(), seg.data_ptr(), rp, None, d_y.ptr, M, T, K, Nout, int(transposed), st))
    out = [d_y.region().copy(), order.cpu().numpy(), seg.cpu().numpy()]
    if g is not None:   # grad_x without rows is stored, not added: its buffer starts as garbage
        d_g, d_gw = Guarded(torch, M, Nout, off=off, fill=g), Guarded(torch, *d_W.shape, off=off, fill=0.0)
        d_gx = Guarded(torch, d_x.shape[0], K, off=off, fill=0.0 if rows is not None else -2.0)
        _capi.check(L.coala_block_gather_mm(0, d_g.ptr, d_W.ptr, order.data_ptr(), seg.data_ptr(), None, rp, d_gx.ptr, M, T, Nout, K, int(not transposed), st))
        p, q = ((d_g.ptr, None, Nout), (d_x.ptr, rp, K)) if transposed else ((d_x.ptr, rp, K), (d_g.ptr, None, Nout))
        _capi.check(L.coala_block_gather_mm_backward_w(0, p[0], p[1], q[0], q[1], order.data_ptr(), seg.data_ptr(), d_gw.ptr, M, T, p[2], q[2], st))
        out += [d_gx.region().copy(), d_gw.region().copy()]
        d_g.region()
    d_x.region(), d_W.region()                             # the inputs' padding too
    return out


def _check(torch, L, rng, T, K, Nout, types, use_rows, transposed, off=1):
    """One list through every kernel, held to the module docstring."""
    M = len(types)
    n_x = N if use_rows else M
    rows = _rows(rng, M) if use_rows else None
    x = rng.standard_normal((n_x, K)).astype(np.float32)
    x[[i for i in (3, 50, 51) if i < n_x]] *= np.float32(1e6)
    W = rng.standard_normal((T, Nout, K) if transposed else (T, K, Nout)).astype(np.float32)
    g = rng.standard_normal((M, Nout)).astype(np.float32)
    d_x, d_W = Guarded(torch, n_x, K, off=off, fill=x), Guarded(torch, T * W.shape[1], W.shape[2], off=off, fill=W.reshape(-1, W.shape[2]))
    y, order, seg, gx, gw = _launch(torch, L, d_x, d_W, types, rows, transposed, T, K, Nout, off, g)
    ry, rymag, rgx, rgxmag, c, rgw, rgwmag, mt, ok = _reference(x, W, types, rows, transposed, g)
    for name, got, ref, bound in (("forward", y, ry, _gamma(K + 1) * rymag), ("grad_x", gx, rgx, _gamma(Nout + c)[:, None] * rgxmag),
                                  ("grad_W", gw.reshape(W.shape), rgw, _gamma(mt + 1)[:, None, None] * rgwmag)):
        err = np.abs(got.astype(np.float64) - ref)
        print(f"in={K} out={Nout} T={T} M={M} rows={use_rows} transposed={transposed}: {name} worst err/bound "
              f"{float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0:.3f}")
        assert np.all(err <= bound), name
    assert np.all(y[~ok] == 0) and np.all(gx[c == 0] == 0) and np.all(gw.reshape(W.shape)[mt == 0] == 0)
    if M == 0:                                             # nothing is launched: order and seg are not written
        return
    key = np.where(ok, types, T)
    assert order.tobytes() == np.argsort(key, kind="stable").astype(np.int32).tobytes()
    assert seg.tobytes() == np.concatenate([[0], np.cumsum(np.bincount(key, minlength=T + 1)[:T])]).astype(np.int32).tobytes()
    # the same bits: run twice; and the first half of the entries, after the list is permuted and the other entries' types and values change
    assert _launch(torch, L, d_x, d_W, types, rows, transposed, T, K, Nout, off)[0].tobytes() == y.tobytes()
    perm, keep = rng.permutation(M), np.arange(M) < M // 2
    t2, x2 = np.where(keep, types, rng.integers(0, T, size=M)).astype(np.int32)[perm], x.copy()
    if use_rows:
        r2 = np.where(keep, rows, rng.integers(0, N, size=M)).astype(np.int32)[perm]
    else:                                                  # without rows entry i reads x[i]: permute x with the list
        x2[~keep] = rng.standard_normal((int((~keep).sum()), K)).astype(np.float32)
        x2, r2 = x2[perm], None
    y2 = _launch(torch, L, Guarded(torch, n_x, K, off=off, fill=x2), d_W, t2, r2, transposed, T, K, Nout, off)[0]
    assert y2[np.argsort(perm)][keep].tobytes() == y[keep].tobytes()


@pytest.mark.parametrize("T", [1, 3, 64])
@pytest.mark.parametrize("K,Nout", [(1, 1), (3, 65), (16, 64), (33, 130), (100, 31)])
def test_gather_mm_abi(hiplib, K, Nout, T):
    import torch
    from COALA_GNN_Pybind import _capi
    L, rng = _capi.load(), np.random.default_rng(10000 * K + 100 * Nout + T)
    sizes = {1: [450], 3: [63, 65, 330]}.get(T) or [0, 1, 63, 64, 65, 200] + list(rng.integers(0, 6, size=T - 6))
    types = _types(rng, sizes, T)
    for use_rows, transposed in ((False, False), (False, True), (True, False), (True, True)):
        _check(torch, L, rng, T, K, Nout, types, use_rows, transposed)
    _check(torch, L, rng, T, K, Nout, types[:0], True, False)
    _check(torch, L, rng, T, K, Nout, np.zeros(1, dtype=np.int32), False, True)


@pytest.mark.parametrize("T,sizes,n_bad", [(1, [65], 0), (4, [254, 1, 1, 1], 0), (64, [64 * 64 + 1 - 63] + [1] * 63, 0),
                                           (4, [1, 65, 1, 129], 1), (2, [1, 2049], 0)])
def test_gather_mm_launch_bound_corner(hiplib, T, sizes, n_bad):
    """Lists that need every tile of the launch bound: M = 64 T + 1 with one row per type and one long segment; every segment, the
    tail included, one row past a multiple of 64 (the forward's M / 64 + T + 1 tiles); and one row past grad_W's 2048-row chunk.
    16-byte aligned buffers and sizes: the vector-load instantiations."""
    import torch
    from COALA_GNN_Pybind import _capi
    rng = np.random.default_rng(T)
    for transposed in (False, True):
        _check(torch, _capi.load(), rng, T, 16, 8, _types(rng, sizes, T, n_bad), False, transposed, off=0)


def _spy(monkeypatch):
    """-> the list that grows by one with every call of the native autograd function"""
    from COALA_GNN import block_ops
    calls, real = [], block_ops._GatherMM.apply
    monkeypatch.setattr(block_ops._GatherMM, "apply", staticmethod(lambda *a: calls.append(1) or real(*a)))
    return calls


def _parity(tag, names, got, want, low, unit):
    """tests/_dispatch_parity.py's rule per tensor: within 4 E (E = |low - want|, low the reference in the input's dtype on the CPU, None
    where the CPU lacks the op) and never asked to be closer than 8 u max |want|."""
    for name, a, b, lo in zip(names, got, want, low):
        tol = max(4.0 * (float((lo.double() - b).abs().max()) if lo is not None else 0.0), 8.0 * unit * float(b.abs().max()))
        err = float((a.double().cpu() - b).abs().max())
        print(f"{tag} {name}: error {err:.3e} bound {tol:.3e}")
        assert a.shape == b.shape and err <= tol, name


INPUTS = ("native", "colslice", "int64", "fp64", "fp16", "cpu_index", "T65")


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("inp", INPUTS)
def test_gather_mm_dispatch_parity(hiplib, inp, transposed, monkeypatch):
    """Whatever path an input takes -- the kernels or gather_mm_torch -- the result and both gradients have the shape, dtype and values
    of gather_mm_torch in float64 on the CPU.  Every source is named about 1.3 times and none often: E is the error of ONE summation
    order in fp32, which says nothing about a 300-term sum of float atomics in another order (that one measured 1.17e-04 against
    4 E = 1.03e-04 in one run and passed in the next); the source named 300 times is held to its gamma bound in test_gather_mm_abi."""
    import torch
    from COALA_GNN import block_ops
    from _dispatch_parity import UNIT
    K, Nout, T = 24, 20, 65 if inp == "T65" else 5
    rng = np.random.default_rng(INPUTS.index(inp) * 2 + transposed)
    dtype = {"fp64": torch.float64, "fp16": torch.float16}.get(inp, torch.float32)
    base = torch.from_numpy(rng.standard_normal((N, K + 8)).astype(np.float32)).to(dtype)
    view = (lambda t: t[:, 3: 3 + K]) if inp == "colslice" else (lambda t: t[:, :K].contiguous())
    W0 = torch.from_numpy(rng.standard_normal((T, Nout, K) if transposed else (T, K, Nout)).astype(np.float32)).to(dtype)
    idt = np.int64 if inp == "int64" else np.int32
    types = torch.from_numpy(_types(rng, [500 // T] * T, T).astype(idt))
    rows = torch.from_numpy(np.where(rng.random(len(types)) < 0.01, -1, rng.integers(0, N - 10, size=len(types))).astype(idt))
    w = torch.from_numpy(rng.standard_normal((len(types), Nout)).astype(np.float32))
    calls = _spy(monkeypatch)

    def run(fn, x, W, idx_dev, dt):
        x, W = x.detach().requires_grad_(), W.detach().requires_grad_()
        out = fn(x, W, types.to(idx_dev), rows.to(idx_dev), transposed=transposed)
        (out * w.to(device=x.device, dtype=dt)).sum().backward()
        return out.detach(), x.grad, W.grad

    got = run(block_ops.gather_mm, view(base.cuda()), W0.cuda(), "cpu" if inp == "cpu_index" else "cuda", dtype)
    assert bool(calls) == (inp in ("native", "colslice", "int64")), "the wrong path ran"
    assert tuple(got[0].shape) == (len(types), Nout) and got[0].dtype == dtype
    want = run(block_ops.gather_mm_torch, view(base).double(), W0.double(), "cpu", torch.float64)
    try:
        low = run(block_ops.gather_mm_torch, view(base), W0, "cpu", dtype)
    except RuntimeError:
        low = (None,) * 3
    _parity(f"{inp} transposed={transposed}", ("out", "grad_x", "grad_W"), got, want, low, UNIT[dtype])
    with pytest.raises(IndexError):
        block_ops.gather_mm(got[1], got[2], torch.tensor([0], device="cuda"), torch.tensor([N], device="cuda"), transposed=transposed)


def test_typed_linear_on_gather_mm(hiplib, monkeypatch):
    """nn.TypedLinear on unsorted types with two out of range: output and W's gradient against the same module in float64 on the CPU (E
    from the module in fp32 on the CPU); the native op ran."""
    import torch
    from COALA_GNN import nn
    from _dispatch_parity import UNIT
    rng = np.random.default_rng(3)
    x, ntype = torch.from_numpy(rng.standard_normal((150, 12)).astype(np.float32)), torch.from_numpy(rng.integers(0, 3, size=150))
    ntype[[7, 99]] = torch.tensor([-1, 3])
    torch.manual_seed(5)
    mod = nn.TypedLinear(12, 16, 3)

    def run(dev, dt):
        m = copy.deepcopy(mod).to(device=dev, dtype=dt)
        out = m(x.to(device=dev, dtype=dt), ntype.to(dev))
        (out * torch.linspace(-1, 1, out.numel(), device=dev, dtype=dt).view(out.shape)).sum().backward()
        return out.detach().cpu(), m.W.grad.cpu()

    calls = _spy(monkeypatch)
    got = run("cuda", torch.float32)
    assert len(calls) == 1, "the native gather_mm did not run"
    assert torch.all(got[0][[7, 99]] == 0)
    _parity("TypedLinear", ("out", "W.grad"), got, run("cpu", torch.float64), run("cpu", torch.float32), UNIT[torch.float32])
