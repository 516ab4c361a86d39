"""GPU tests of the LSTM aggregation (coala_block_lstm_aggregate*, Block.lstm_aggregate, nn.LSTMSAGEConv) against the float64 step loop
of _lstm_ref.py, at the C ABI on Guarded buffers one float off 16-byte alignment and through Block.

Bound, per tensor (out, grad_xg, grad_w_hh): the native result's max-norm distance from the float64 reference is at most twice the
distance of Block.lstm_aggregate_torch run in fp32 on the GPU on the same inputs -- the two differ in summation order and nothing else
that rounds (an a-priori bound through k steps of sigmoid and tanh is not derivable).  Both distances are printed.
Exact: zeros for empty rows and no gradient for sources nobody names; the same bits on the fixed and the ragged form, when the forward
runs twice and when the other rows of the tile change; the padding around every buffer."""
import copy
import functools

import numpy as np
import pytest

from _lstm_ref import lstm_ref, valid_rows
from _util import Guarded

pytestmark = pytest.mark.gpu
SPARE = 5                      # sources at the end of xg that no row names
# (H, n_dst, fan-out), every value of the issue once; "hub": a row of 40 edges between empty ones, ragged only
CASES = [(32, 1, 32), (64, 31, 2), (96, 33, 5), (128, 70, 32), (256, 33, 1), (256, 3, "hub"), (32, 70, 5)]


@functools.lru_cache(maxsize=None)
def _case(H, n_dst, fan):
    """-> nbr (None for the hub case), the rows' valid sources, xg, w_hh, grad_out, the float64 reference (computed once)"""
    rng = np.random.default_rng(1000 * H + 10 * n_dst + (99 if fan == "hub" else fan))
    n_src = 3 * n_dst + SPARE
    if fan == "hub":
        nbr, rows = None, [[], [int(s) for s in rng.integers(0, n_src - SPARE, size=40)], []]
    else:
        nbr = rng.integers(0, n_src - SPARE, size=(n_dst, fan)).astype(np.int32)
        nbr[rng.random(nbr.shape) < 0.3] = -1                   # unlike degrees inside a tile, a -1 anywhere in a row
        nbr[6::7] = -1                                          # empty rows
        if n_dst > 1:
            nbr[1] = nbr[1, 0] = 2                              # a full row that repeats one source
        if fan >= 5 and n_dst > 2:
            nbr[2, :3] = [4, -1, 4]                             # a -1 in the middle, the same source on both sides
        rows = valid_rows(nbr)
    xg = rng.standard_normal((n_src, 4 * H)).astype(np.float32)
    w = (rng.standard_normal((4 * H, H)) / np.sqrt(H)).astype(np.float32)
    go = rng.standard_normal((n_dst, H)).astype(np.float32)
    return nbr, rows, xg, w, go, lstm_ref(rows, xg, w, go)


def _index(torch, nbr, rows):
    """-> (the ABI's name suffixes, the index tensors, what follows n_dst, S) of the fixed form (nbr given) or the ragged form"""
    if nbr is not None:
        return ("", ""), (torch.from_numpy(nbr).cuda(),), (nbr.shape[1],), nbr.size
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.array([s for r in rows for s in r], dtype=np.int32)
    return ("_csr", "_csr"), (torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda()), (), len(indices)


def _abi(torch, nbr, rows, xg, w, go=None, off=1):
    """forward (and, with go, backward and the caller's GEMM) at the C ABI -> out(, grad_xg, grad_w_hh) as numpy, padding checked"""
    from COALA_GNN.block_ops import lstm_grad_w_hh
    from COALA_GNN_Pybind import _capi, current_stream
    L, st, H, n_dst = _capi.load(), current_stream(), w.shape[1], len(rows)
    (fs, bs), idx, fan, S = _index(torch, nbr, rows)
    d_xg, d_w, d_out = Guarded(torch, *xg.shape, off=off, fill=xg), Guarded(torch, *w.shape, off=off, fill=w), Guarded(torch, n_dst, H, off=off)
    d_gates, d_cell = (Guarded(torch, S, 4 * H, off=off), Guarded(torch, S, H, off=off)) if go is not None else (None, None)
    _capi.check(getattr(L, "coala_block_lstm_aggregate" + fs)(0, *[t.data_ptr() for t in idx], d_xg.ptr, d_w.ptr, d_out.ptr, d_gates and d_gates.ptr,
                                                              d_cell and d_cell.ptr, n_dst, *fan, H, st))
    res = [d_out.region().copy()]
    if go is not None:
        d_go, d_hp, d_gx = Guarded(torch, n_dst, H, off=off, fill=go), Guarded(torch, S, H, off=off), Guarded(torch, *xg.shape, off=off, fill=0.0)
        _capi.check(getattr(L, "coala_block_lstm_aggregate_backward" + bs)(0, *[t.data_ptr() for t in idx], d_w.ptr, d_go.ptr, d_gates.ptr,
                                                                           d_cell.ptr, d_hp.ptr, d_gx.ptr, n_dst, *fan, H, st))
        dz, hp = (torch.from_numpy(g.region().copy()).cuda() for g in (d_gates, d_hp))
        res += [d_gx.region().copy(), lstm_grad_w_hh(dz, hp).cpu().numpy()]
        d_cell.region(), d_go.region()
    d_xg.region(), d_w.region()
    return res


def _through_block(torch, nbr, rows, xg, w, go, fn="lstm_aggregate"):
    from COALA_GNN.sampler import Block
    _, idx, _, _ = _index(torch, nbr, rows)
    src = torch.arange(xg.shape[0], device="cuda")
    block = Block(src, idx[0], len(rows)) if nbr is not None else Block(src, None, len(rows), indptr=idx[0], indices=idx[1])
    t_xg, t_w = torch.from_numpy(xg).cuda().requires_grad_(), torch.from_numpy(w).cuda().requires_grad_()
    out = getattr(block, fn)(t_xg, t_w)
    (out * torch.from_numpy(go).cuda()).sum().backward()
    return [t.detach().cpu().numpy() for t in (out, t_xg.grad, t_w.grad)]


@pytest.mark.parametrize("H,n_dst,fan", CASES)
def test_lstm_aggregate(hiplib, H, n_dst, fan):
    import torch
    nbr, rows, xg, w, go, want = _case(H, n_dst, fan)
    low = _through_block(torch, None, rows, xg, w, go, "lstm_aggregate_torch")
    outs = []
    for form in ([None] if nbr is None else [nbr, None]):       # the fixed form, and the ragged form of the same rows
        for how, got in (("abi", _abi(torch, form, rows, xg, w, go)), ("block", _through_block(torch, form, rows, xg, w, go))):
            for name, a, lo, ref in zip(("out", "grad_xg", "grad_w_hh"), got, low, want):
                err, e = float(np.abs(a - ref).max()), float(np.abs(lo - ref).max())
                print(f"H={H} n_dst={n_dst} fan={fan} {'fixed' if form is not None else 'ragged'} {how} {name}: native {err:.3e} torch fp32 {e:.3e}")
                assert a.shape == ref.shape and err <= 2.0 * e, name
            assert not got[0][[d for d, r in enumerate(rows) if not r]].any() and not got[1][-SPARE:].any()
            outs.append(got[0])
    assert all(o.tobytes() == outs[0].tobytes() for o in outs), "fixed / ragged / ABI / Block / second run: the forward's bits differ"
    if nbr is not None and n_dst > 1:                           # the other rows of every tile change: the kept rows keep their bits
        other = nbr.copy()
        other[1::2] = np.roll(nbr[1::2], 1, axis=1)[::-1]
        assert _abi(torch, other, valid_rows(other), xg, w)[0][::2].tobytes() == outs[0][::2].tobytes()


def test_lstm_aggregate_large_gates(hiplib):
    import torch                                                # gate pre-activations of magnitude 30: no NaN or Inf in any result
    nbr, rows, xg, w, go, _ = _case(64, 31, 2)
    for got in (_abi(torch, nbr, rows, 30 * np.sign(xg), w, go), _through_block(torch, nbr, rows, 30 * np.sign(xg), 30 * w, go)):
        assert all(np.isfinite(t).all() for t in got)


@pytest.mark.parametrize("H", [48, 512])
def test_lstm_aggregate_outside_native_range(hiplib, H, monkeypatch):
    """COALA_EINVAL at the ABI, nothing launched; Block.lstm_aggregate serves the width through its fallback."""
    import torch
    from COALA_GNN import block_ops
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    t = torch.zeros(8, dtype=torch.int32, device="cuda")
    p = t.data_ptr()
    assert L.coala_block_lstm_aggregate(0, p, p, p, p, None, None, 2, 4, H, None) == _capi.EINVAL and "hidden size" in _capi.last_error()
    assert L.coala_block_lstm_aggregate_backward_csr(0, p, p, p, p, p, p, None, None, 2, H, None) == _capi.EINVAL
    assert L.coala_block_lstm_aggregate(0, p, p, p, p, None, None, 2, 33, 64, None) == _capi.EINVAL and "fan-out" in _capi.last_error()
    assert L.coala_block_lstm_aggregate(0, p, None, p, p, None, None, 2, 4, 64, None) == _capi.EINVAL and "null" in _capi.last_error()
    monkeypatch.setattr(block_ops._LSTMAggregate, "apply", None)               # the native path would raise
    rng = np.random.default_rng(H)
    nbr = rng.integers(-1, 9, size=(4, 3)).astype(np.int32)
    xg, w, go = (rng.standard_normal(s).astype(np.float32) / 8 for s in ((9, 4 * H), (4 * H, H), (4, H)))
    for got, ref in zip(_through_block(torch, nbr, valid_rows(nbr), xg, w, go), lstm_ref(valid_rows(nbr), xg, w, go)):
        assert got.shape == ref.shape and np.allclose(got, ref, rtol=1e-4, atol=1e-5)


def test_lstm_sage_conv_step(hiplib):
    """A state_dict with DGL's names and shapes loads with strict=True; logits and every parameter's gradient of one step against the
    same layer in float64 on the CPU (its fallback), by tests/_dispatch_parity.py's rule: within 4 E, E the distance of the layer in
    fp32 on the CPU from float64, and never asked to be closer than 8 u times the reference's largest magnitude."""
    import torch
    from COALA_GNN.nn import LSTMSAGEConv
    from COALA_GNN.sampler import Block
    nbr, rows, *_ = _case(64, 31, 2)
    g = torch.Generator().manual_seed(3)
    sd = {k: torch.randn(s, generator=g) / 8 for k, s in (("lstm.weight_ih_l0", (256, 64)), ("lstm.weight_hh_l0", (256, 64)), ("lstm.bias_ih_l0", (256,)),
                                                           ("lstm.bias_hh_l0", (256,)), ("fc_self.weight", (7, 64)), ("fc_neigh.weight", (7, 64)), ("bias", (7,)))}
    layer = LSTMSAGEConv(64, 7)
    layer.load_state_dict(sd, strict=True)
    x = torch.randn(3 * 31 + SPARE, 64, generator=g)

    def run(dev, dt):
        m = copy.deepcopy(layer).to(device=dev, dtype=dt)
        out = m(Block(torch.arange(x.shape[0], device=dev), torch.from_numpy(nbr).to(dev), 31), x.to(device=dev, dtype=dt))
        (out * torch.linspace(-1, 1, out.numel(), device=dev, dtype=dt).view(out.shape)).sum().backward()
        return [out.detach().cpu().double()] + [p.grad.cpu().double() for p in m.parameters()]

    for name, a, lo, ref in zip(["logits"] + [n for n, _ in layer.named_parameters()], run("cuda", torch.float32), run("cpu", torch.float32), run("cpu", torch.float64)):
        err, tol = float((a - ref).abs().max()), max(4 * float((lo - ref).abs().max()), 8 * 2.0 ** -24 * float(ref.abs().max()))
        print(f"LSTMSAGEConv {name}: error {err:.3e} bound {tol:.3e}")
        assert err <= tol, name
