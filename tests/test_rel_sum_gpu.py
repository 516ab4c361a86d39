"""GPU tests of the relation-typed sum (coala_block_rel_sum[_backward][_csr] in coala_block_ops.hip, Block.rel_sum_aggregate,
nn.RelGraphConv, harness.RGCN).

The forward is compared twice.  Bit for bit, relation by relation, with coala_block_weighted_sum given the weights w * [etype == r]:
the contract says both add the same terms in the same order with one fma each, and a term of weight 0 leaves a finite accumulator as
it is.  And, independently of that kernel, against a float64 sum within the bounds of test_weighted_sum_gpu.py (u = 2^-24,
gamma(n) = n u / (1 - n u), from test_block_ops_gpu.py):
  forward   out[d, r, c] = sum of the cnt_r terms w_j x[s_j, c] of relation r, in slot order, one fma each: |got - ref| <=
            gamma(cnt_r + 1) sum|w_j x_j|.  A relation absent from a row, and a row without an edge, are exactly 0 -- the buffers are
            filled with another value before the call, so this proves that the output is written whole.
  grad_src  grad_src[s, c] = sum over the k edges (with a type in range) landing on s of fl(w_j g[d, t_j, c]), atomics in any order:
            |got - ref| <= gamma(k + 1) sum|w_j g|; a source nobody references stays exactly 0.
  grad_w    grad_w[slot j] = <g[d, t_j, :], x[s_j, :]>, dim terms through per-lane fmas and a butterfly: |got - ref| <=
            gamma(dim + 1) sum|g_c x_c|; exactly 0 on a padding slot and on a type outside [0, R).
Everything outside an output region keeps its sentinel."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _util import SENTINEL, ColorFiles, Guarded
from test_block_ops_gpu import _gamma
from test_max_aggregate_gpu import _csr
from test_weighted_sum_gpu import _dense_inputs

pytestmark = pytest.mark.gpu

DIMS = [1, 3, 64, 100, 128, 301, 1024]
R_DIM = [(R, dim) for R in (1, 3, 8) for dim in DIMS] + [(64, dim) for dim in (1, 3, 100)]
FILL = np.float32(-2.0)   # what Guarded puts into a region: an output that is not written keeps it


def _types(rng, shape, R):
    """int32 types, uniform in [0, R); about 5 % out of range (-1, R, 2^30); relation 1 is used by no edge when R >= 3"""
    t = rng.integers(0, R, size=shape).astype(np.int32)
    if R >= 3:
        t[t == 1] = 0
    bad = rng.random(shape) < 0.05
    t[bad] = rng.choice(np.array([-1, R, 1 << 30], dtype=np.int32), size=int(bad.sum()))
    return t


def _edges(nbr=None, indptr=None, idx=None):
    """(row, flat slot, source) of every valid slot of either block form"""
    if nbr is not None:
        rows, cols = np.nonzero(nbr >= 0)
        return rows, rows * nbr.shape[1] + cols, nbr[rows, cols].astype(np.int64)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    keep = idx >= 0
    return rows[keep], np.flatnonzero(keep), idx[keep].astype(np.int64)


def _check(torch, rows, slots, srcs, t, w, x, go, n_dst, R, got_out, got_gs, got_gw, what):
    """The outputs against float64 (computed on the GPU), element by element, within the bounds of the module docstring.  t, w: flat,
    one per slot (w None: 1); go [n_dst, R * dim]; each got_* may be None."""
    dim, n_src = x.shape[1], x.shape[0]
    tt = t.reshape(-1)[slots].astype(np.int64)
    ok = (tt >= 0) & (tt < R)
    n_slots = t.size
    rows, slots, srcs, tt = rows[ok], slots[ok], srcs[ok], tt[ok]
    dev = "cuda"
    seg = torch.from_numpy(rows * R + tt).to(dev)
    t_src = torch.from_numpy(srcs).to(dev)
    wf = torch.ones(len(slots), dtype=torch.float64, device=dev) if w is None else torch.from_numpy(w.reshape(-1)[slots].astype(np.float64)).to(dev)
    x64, g64 = torch.from_numpy(x).to(dev).double(), torch.from_numpy(go).to(dev).double().view(n_dst * R, dim)
    cnt = np.bincount(rows * R + tt, minlength=n_dst * R)
    k = np.bincount(srcs, minlength=n_src)
    ref_o, mag_o = (torch.zeros((n_dst * R, dim), dtype=torch.float64, device=dev) for _ in range(2))
    ref_s, mag_s = (torch.zeros((n_src, dim), dtype=torch.float64, device=dev) for _ in range(2))
    ref_w, mag_w = (torch.zeros(n_slots, dtype=torch.float64, device=dev) for _ in range(2))
    t_slots = torch.from_numpy(slots).to(dev)
    step = max(1, (1 << 22) // dim)
    for lo in range(0, len(rows), step):
        sl = slice(lo, lo + step)
        xs, gs, ws = x64[t_src[sl]], g64[seg[sl]], wf[sl, None]
        ref_o.index_add_(0, seg[sl], ws * xs), mag_o.index_add_(0, seg[sl], (ws * xs).abs())
        ref_s.index_add_(0, t_src[sl], ws * gs), mag_s.index_add_(0, t_src[sl], (ws * gs).abs())
        ref_w[t_slots[sl]], mag_w[t_slots[sl]] = (gs * xs).sum(1), (gs * xs).abs().sum(1)
    for name, got, ref, bound, zero in (("forward", got_out, ref_o, _gamma(cnt + 1)[:, None] * mag_o.cpu().numpy(), cnt == 0),
                                        ("grad_src", got_gs, ref_s, _gamma(k + 1)[:, None] * mag_s.cpu().numpy(), k == 0),
                                        ("grad_w", got_gw, ref_w, _gamma(dim + 1) * mag_w.cpu().numpy(), None)):
        if got is None:
            continue
        ref = ref.cpu().numpy()
        got = got.reshape(ref.shape)
        err = np.abs(got.astype(np.float64) - ref)
        bad = ~(err <= bound + 1e-30)
        with np.errstate(divide="ignore", invalid="ignore"):
            print(f"{what} {name}: largest err / bound {np.nanmax(np.where(bound > 0, err / bound, 0.0)):.3f}")
        if bad.any():
            at = tuple(np.argwhere(bad)[0])
            raise AssertionError(f"{what} {name}: {bad.sum()} elements past the bound; at {at}: got {got[at]!r} want {ref[at]!r} bound {bound[at]!r}")
        if zero is not None:
            assert np.all(got[zero].view(np.int32) == 0), f"{what} {name}: a row nothing is added to is not exactly +0"
    if got_gw is not None:
        dead = np.ones(n_slots, dtype=bool)
        dead[slots] = False
        assert np.all(got_gw.reshape(-1)[dead] == 0.0), f"{what}: grad_w of a padding slot or of a type out of range is not 0"
    return cnt.reshape(n_dst, R)


class _Case:
    """One block in either form with its device copies; runs the entry points into guarded buffers."""

    def __init__(self, torch, x, t, w, off, R, nbr=None, indptr=None, idx=None):
        from COALA_GNN_Pybind import _capi, current_stream
        self.torch, self.capi, self.st, self.L = torch, _capi, current_stream, _capi.load()
        self.x, self.t, self.w, self.off, self.R = x, t, w, off, R
        self.nbr, self.indptr, self.idx = nbr, indptr, idx
        self.n_src, self.dim = x.shape
        self.n_dst = nbr.shape[0] if nbr is not None else len(indptr) - 1
        self.slot_shape = nbr.shape if nbr is not None else (1, len(idx))
        self.d_t = torch.from_numpy(t).cuda()
        self.gx = Guarded(torch, self.n_src, self.dim, off, x)
        self.gw = Guarded(torch, *self.slot_shape, off, w) if w is not None else None
        if nbr is not None:
            self.d_nbr = torch.from_numpy(nbr).cuda()
            self.head = (self.d_nbr.data_ptr(),)
            self.tail = (self.n_dst, nbr.shape[1])
        else:
            self.d_ip, self.d_idx = torch.from_numpy(indptr).cuda(), torch.from_numpy(idx).cuda()
            self.head = (self.d_ip.data_ptr(), self.d_idx.data_ptr())
            self.tail = (self.n_dst,)
        self.sfx = "" if nbr is not None else "_csr"

    def edges(self):
        return _edges(self.nbr, self.indptr, self.idx)

    def inputs_unchanged(self):
        assert np.array_equal(self.gx.region(), self.x), "h_src changed"
        assert np.array_equal(self.d_t.cpu().numpy(), self.t), "etype changed"
        if self.gw is not None:
            assert self.gw.region().tobytes() == np.ascontiguousarray(self.w, np.float32).tobytes(), "w changed"

    def forward(self, w="own", fill=-2.0):
        """-> out [n_dst, R * dim]; w: 'own', None (a null pointer) or an array; fill: what the output region holds before the call"""
        torch = self.torch
        gw = self.gw if isinstance(w, str) else (Guarded(torch, *self.slot_shape, self.off, w) if w is not None else None)
        out = Guarded(torch, self.n_dst, self.R * self.dim, self.off, fill)
        fn = getattr(self.L, "coala_block_rel_sum" + self.sfx)
        self.capi.check(fn(0, *self.head, self.d_t.data_ptr(), gw.ptr if gw is not None else None, self.gx.ptr, out.ptr, *self.tail, self.R,
                           self.dim, self.st()))
        torch.cuda.synchronize()
        return out.region()

    def weighted_sum(self, w):
        """coala_block_weighted_sum[_csr] on the same block with the weights w -> [n_dst, dim]"""
        torch = self.torch
        gw, out = Guarded(torch, *self.slot_shape, self.off, w), Guarded(torch, self.n_dst, self.dim, self.off)
        fn = getattr(self.L, "coala_block_weighted_sum" + self.sfx)
        self.capi.check(fn(0, *self.head, gw.ptr, self.gx.ptr, out.ptr, *self.tail, self.dim, self.st()))
        torch.cuda.synchronize()
        return out.region()

    def backward(self, go, want_src=True, want_w=True):
        """-> (grad_src [n_src, dim], grad_w flat); an output that is not wanted is passed as null and must keep its fill"""
        torch = self.torch
        gg = Guarded(torch, self.n_dst, self.R * self.dim, self.off, go)
        gs, gwo = Guarded(torch, self.n_src, self.dim, self.off, 0.0), Guarded(torch, *self.slot_shape, self.off)
        fn = getattr(self.L, "coala_block_rel_sum" + self.sfx + "_backward")
        self.capi.check(fn(0, *self.head, self.d_t.data_ptr(), self.gw.ptr if self.gw is not None else None, self.gx.ptr, gg.ptr,
                           gs.ptr if want_src else None, gwo.ptr if want_w else None, *self.tail, self.R, self.dim, self.st()))
        torch.cuda.synchronize()
        assert np.array_equal(gg.region(), go), "grad_out changed"
        a, b = gs.region(), gwo.region().reshape(-1)
        if not want_src:
            assert np.all(a == 0.0), "grad_src = null, and something was added"
        if not want_w:
            assert np.all(b == FILL), "grad_w = null, and something was stored"
        return a, b

    def weighted_sum_grad_w(self, go):
        torch = self.torch
        gg, gwo = Guarded(torch, self.n_dst, self.dim, self.off, go), Guarded(torch, *self.slot_shape, self.off)
        w = self.gw if self.gw is not None else Guarded(torch, *self.slot_shape, self.off, 1.0)
        fn = getattr(self.L, "coala_block_weighted_sum" + self.sfx + "_backward")
        self.capi.check(fn(0, *self.head, w.ptr, self.gx.ptr, gg.ptr, None, gwo.ptr, *self.tail, self.dim, self.st()))
        torch.cuda.synchronize()
        return gwo.region().reshape(-1)


def _check_forward(torch, case, what):
    """Every check of the forward on one block; -> (out, the count of every (row, relation))"""
    R, dim, n_dst = case.R, case.dim, case.n_dst
    out = case.forward()
    case.inputs_unchanged()
    o3 = out.reshape(n_dst, R, dim)
    t_slots = case.t.reshape(case.slot_shape)
    for r in range(R):
        want = case.weighted_sum(case.w.reshape(case.slot_shape) * (t_slots == r))
        bad = o3[:, r].view(np.int32) != want.view(np.int32)
        assert not bad.any(), f"{what}: relation {r} differs from the weighted sum with w * [etype == {r}] at {tuple(np.argwhere(bad)[0])}"
    rows, slots, srcs = case.edges()
    go = np.zeros((n_dst, R * dim), dtype=np.float32)
    cnt = _check(torch, rows, slots, srcs, case.t, case.w, case.x, go, n_dst, R, out, None, None, what)
    # written whole: an element the kernel leaves alone keeps what the region held before the call, so it differs between two calls
    # into regions filled with different values (a sum can be -2.0, the first fill, by itself: that alone says nothing)
    again = case.forward(fill=3.5)
    same = out.view(np.int32) == again.view(np.int32)
    print(f"{what}: {int((o3 == FILL).sum())} elements equal the first fill, {int((~same).sum())} differ between the two fills")
    assert same.all(), f"{what}: a part of the output was not written, first at {tuple(np.argwhere(~same)[0])}"
    return out, cnt


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("R,dim", R_DIM)
@pytest.mark.parametrize("f", [1, 5, 16, 32])
def test_rel_sum_dense(hiplib, f, R, dim, off):
    """Fixed blocks through the C ABI; off = 1 puts every float buffer one float off 16-byte alignment (the scalar path at
    dim % 4 == 0).  Row 3 holds a single type; relation 1 is used by no edge (R >= 3); row 0 and others have no edge."""
    import torch
    rng = np.random.default_rng(f * 4099 + dim * 3 + off + R * 77)
    n_dst, n_src = 1031, 200
    nbr, w, x, _ = _dense_inputs(rng, n_dst, f, n_src, dim)
    nbr[3] = rng.integers(0, n_src - 7, size=f)
    t = _types(rng, (n_dst, f), R)
    t[3] = R - 1
    case = _Case(torch, x, t, w, off, R, nbr=nbr)
    out, cnt = _check_forward(torch, case, f"dense f={f} R={R} dim={dim} off={off}")
    assert cnt[3, R - 1] == f and cnt[3].sum() == f and cnt[0].sum() == 0
    if R >= 3:
        assert cnt[:, 1].sum() == 0 and np.all(out.reshape(n_dst, R, dim)[:, 1].view(np.int32) == 0)
    assert nbr.max() < n_src - 7
    # w = null is w = ones, bit for bit
    a, b = case.forward(w=None), case.forward(w=np.ones((n_dst, f), np.float32))
    assert a.tobytes() == b.tobytes(), "w = null differs from w = ones"


def _ragged_case(torch, rng, R, dim, off, n_dst=301, n_src=500):
    indptr, idx = _csr(rng, n_dst, n_src)
    E = len(idx)
    t = _types(rng, E, R)
    w = rng.standard_normal(E).astype(np.float32)
    w[rng.random(E) < 0.1] = 0
    x = rng.standard_normal((n_src, dim)).astype(np.float32)
    x[rng.random(n_src) < 0.03] *= np.float32(1e6)
    late = None
    if R >= 2:   # relation R - 1 appears in the 3001-edge row only in its last, partial chunk (edges 2944 .. 3000)
        late = n_dst // 2
        row = t[indptr[late]: indptr[late + 1]]
        row[row == R - 1] = 0
        row[2990] = R - 1
    return _Case(torch, x, t, w, off, R, indptr=indptr, idx=idx), late


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("R,dim", R_DIM)
def test_rel_sum_ragged(hiplib, R, dim, off):
    """A ragged block with empty rows, a row of 150 edges (3 chunks of 64) and one of 3001 (47 chunks, the last one partial)."""
    import torch
    rng = np.random.default_rng(dim * 7 + off + R * 131)
    case, late = _ragged_case(torch, rng, R, dim, off)
    out, cnt = _check_forward(torch, case, f"ragged R={R} dim={dim} off={off}")
    assert cnt[0].sum() == 0
    if late is not None:
        assert cnt[late, R - 1] == 1
    a, b = case.forward(w=None), case.forward(w=np.ones(len(case.idx), np.float32))
    assert a.tobytes() == b.tobytes(), "w = null differs from w = ones"


def _as_ragged(nbr, *per_slot):
    valid = nbr >= 0
    indptr = np.zeros(nbr.shape[0] + 1, dtype=np.int64)
    np.cumsum(valid.sum(1), out=indptr[1:])
    return (indptr, nbr[valid]) + tuple(a[valid] for a in per_slot)


@pytest.mark.parametrize("f,R,dim,off", [(5, 4, 128, 0), (32, 8, 100, 0), (1, 1, 1, 0), (32, 3, 1024, 1), (17, 64, 64, 0), (16, 2, 301, 0)])
def test_dense_and_ragged_forms_give_the_same_bits(hiplib, f, R, dim, off):
    """The same rows in both forms (the ragged one drops the -1 slots): forward and grad_w equal bit for bit."""
    import torch
    rng = np.random.default_rng(f + dim + R)
    n_dst, n_src = 1031, 300
    nbr, w, x, _ = _dense_inputs(rng, n_dst, f, n_src, dim)
    t = _types(rng, (n_dst, f), R)
    go = rng.standard_normal((n_dst, R * dim)).astype(np.float32)
    indptr, idx, tr, wr = _as_ragged(nbr, t, w)
    a, b = _Case(torch, x, t, w, off, R, nbr=nbr), _Case(torch, x, tr, wr, off, R, indptr=indptr, idx=idx)
    assert a.forward().tobytes() == b.forward().tobytes(), "forward differs between the dense and the ragged form"
    _, a_gw = a.backward(go)
    _, b_gw = b.backward(go)
    assert a_gw.reshape(n_dst, f)[nbr >= 0].tobytes() == b_gw.tobytes(), "grad_w differs between the dense and the ragged form"


def test_rel_sum_more_rows_than_waves(hiplib):
    """40000 rows: more than the 32768 waves of the largest grid, so some waves take a second row."""
    import torch
    rng = np.random.default_rng(9)
    nbr, w, x, _ = _dense_inputs(rng, 40000, 5, 300, 12)
    case = _Case(torch, x, _types(rng, (40000, 5), 3), w, 0, 3, nbr=nbr)
    _check_forward(torch, case, "40000 rows")


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("R", [1, 8])
@pytest.mark.parametrize("dim", [1, 3, 100, 128, 301, 1024])
def test_rel_sum_backward(hiplib, dim, R, off):
    """Both gradients through the C ABI on a fixed block and on the same rows in the ragged form; each output null in turn; with
    R = 1 and every type 0, grad_w has the bits of coala_block_weighted_sum_backward's."""
    import torch
    rng = np.random.default_rng(dim * 5 + off + R)
    n_dst, n_src, f = 1031, 200, 7
    nbr, w, x, _ = _dense_inputs(rng, n_dst, f, n_src, dim)
    t = _types(rng, (n_dst, f), R)
    go = rng.standard_normal((n_dst, R * dim)).astype(np.float32)
    go[rng.random(n_dst) < 0.03] *= np.float32(1e6)
    what = f"backward dim={dim} R={R} off={off}"
    case = _Case(torch, x, t, w, off, R, nbr=nbr)
    gs, gw = case.backward(go)
    case.inputs_unchanged()
    rows, slots, srcs = case.edges()
    _check(torch, rows, slots, srcs, t, w, x, go, n_dst, R, None, gs, gw, what)
    assert np.all(gs[n_src - 7:] == 0.0)
    gs2, _ = case.backward(go, want_w=False)
    _check(torch, rows, slots, srcs, t, w, x, go, n_dst, R, None, gs2, None, what + " grad_w = null")
    _, gw2 = case.backward(go, want_src=False)
    assert gw2.tobytes() == gw.tobytes(), "grad_w changes when grad_src is not asked for"
    # the ragged form of the same rows
    indptr, idx, tr, wr = _as_ragged(nbr, t, w)
    rag = _Case(torch, x, tr, wr, off, R, indptr=indptr, idx=idx)
    rs, rw = rag.backward(go)
    _check(torch, *rag.edges(), tr, wr, x, go, n_dst, R, None, rs, rw, what + " ragged")
    assert gw.reshape(n_dst, f)[nbr >= 0].tobytes() == rw.tobytes(), "grad_w differs between the two forms"
    # w = null: unit weights
    unit = _Case(torch, x, t, None, off, R, nbr=nbr)
    us, uw = unit.backward(go)
    _check(torch, rows, slots, srcs, t, None, x, go, n_dst, R, None, us, uw, what + " w = null")
    assert uw.tobytes() == gw.tobytes(), "grad_w depends on w"
    if R == 1:
        for c in (_Case(torch, x, np.zeros_like(t), w, off, 1, nbr=nbr), _Case(torch, x, np.zeros_like(tr), wr, off, 1, indptr=indptr, idx=idx)):
            _, mine = c.backward(go, want_src=False)
            assert mine.tobytes() == c.weighted_sum_grad_w(go).tobytes(), "R = 1: grad_w differs from the weighted sum backward's"


def test_rel_sum_refuses_bad_shapes(hiplib):
    """Return codes only: nothing is launched, and the output buffers keep their sentinel."""
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    from COALA_GNN.sampler import Block
    L = _capi.load()
    nbr = torch.zeros(64, dtype=torch.int32, device="cuda")
    ip = torch.zeros(65, dtype=torch.int64, device="cuda")
    a = torch.zeros(64 * 4, device="cuda")
    b = torch.full((64 * 4,), float(SENTINEL), device="cuda")
    st = current_stream()
    n, i, A, B = nbr.data_ptr(), ip.data_ptr(), a.data_ptr(), b.data_ptr()
    for n_dst, f, R, dim in ((1, 0, 2, 4), (1, 33, 2, 4), (1, 4, 2, 0), (-1, 4, 2, 4), (0, 33, 2, 4), (1, 4, 0, 4), (1, 4, 65, 4), (0, 4, 65, 4),
                             (1, 4, -1, 4)):
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_rel_sum(0, n, n, A, A, B, n_dst, f, R, dim, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_rel_sum_backward(0, n, n, A, A, A, B, B, n_dst, f, R, dim, st))
    for n_dst, R, dim in ((1, 2, 0), (-1, 2, 4), (1, 0, 4), (1, 65, 4)):
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_rel_sum_csr(0, i, n, n, A, A, B, n_dst, R, dim, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_rel_sum_csr_backward(0, i, n, n, A, A, A, B, B, n_dst, R, dim, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_rel_sum(0, n, None, A, A, B, 4, 4, 2, 4, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_rel_sum(0, n, n, None, None, B, 4, 4, 2, 4, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_rel_sum_csr(0, None, n, n, A, A, B, 4, 2, 4, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_rel_sum_backward(0, n, n, A, None, A, B, B, 4, 4, 2, 4, st))   # grad_w wanted, and no h_src
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_rel_sum_csr_backward(0, i, n, n, A, A, None, B, B, 4, 2, 4, st))
    # n_dst == 0 is fine and launches nothing
    _capi.check(L.coala_block_rel_sum(0, n, n, A, A, B, 0, 4, 2, 4, st))
    _capi.check(L.coala_block_rel_sum_csr(0, i, n, n, A, A, B, 0, 2, 4, st))
    _capi.check(L.coala_block_rel_sum_backward(0, n, n, A, A, A, B, B, 0, 4, 2, 4, st))
    _capi.check(L.coala_block_rel_sum_csr_backward(0, i, n, n, A, A, A, B, B, 0, 2, 4, st))
    blk = Block(torch.arange(8, device="cuda"), torch.zeros((4, 3), dtype=torch.int32, device="cuda"), 4)
    h = torch.zeros(8, 4, device="cuda")
    with pytest.raises(ValueError, match="one per neighbour slot"):
        blk.rel_sum_aggregate(h, torch.zeros(4, 2, dtype=torch.int64, device="cuda"), 2)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="1..64"):
            blk.rel_sum_aggregate(h, torch.zeros(4, 3, dtype=torch.int64, device="cuda"), bad)
    torch.cuda.synchronize()
    assert torch.all(b == float(SENTINEL))


def _sampled_blocks(torch, R):
    from COALA_GNN.sampler import LaborSampler, NeighborSampler
    from COALA_GNN.synthetic import edge_types_by_source, powerlaw_csc
    indptr, indices = powerlaw_csc(30000, 12.0, seed=2, device="cuda")
    etype = edge_types_by_source(indices, R)
    seeds = torch.randperm(30000, generator=torch.Generator().manual_seed(1))[:512].cuda()
    out = []
    for name, smp in (("neighbor 10,5", NeighborSampler([10, 5], seed=3, edge_ids=True)), ("neighbor 5,-1", NeighborSampler([5, -1], seed=3, edge_ids=True)),
                      ("labor 5,5", LaborSampler([5, 5], seed=3, edge_ids=True))):
        g = smp.make_graph(indptr, indices, edata={"etype": etype})
        _, _, blocks = smp.sample(g, seeds)
        out += [(f"{name} layer {i}", b) for i, b in enumerate(blocks)]
    return out


@pytest.mark.parametrize("dim", [128, 50])
def test_block_rel_sum_aggregate_through_autograd_on_sampled_blocks(hiplib, dim):
    """Block.rel_sum_aggregate(h, block.edata['etype'], 4, w) on the blocks of NeighborSampler([10, 5]), NeighborSampler([5, -1]) (a
    ragged block) and LaborSampler([5, 5]), all with edge ids: the forward and both gradients are within the bounds of the module
    docstring of a float64 sum, and so are those of the fallback run in float64 (to float64 rounding)."""
    import torch
    R = 4
    rng = np.random.default_rng(dim)
    forms = set()
    for name, b in _sampled_blocks(torch, R):
        forms.add(b.nbr is None)
        et = b.edata["etype"]
        slots_t = b.indices if b.nbr is None else b.nbr
        assert et.dtype == torch.int64 and et.shape == slots_t.shape
        src = b.src_nodes[slots_t.clamp_min(0).long()]
        assert torch.equal(et[slots_t >= 0], (src % R)[slots_t >= 0]), f"{name}: edata['etype'] is not the type of the sampled edge"
        x = rng.standard_normal((b.num_src, dim)).astype(np.float32)
        wv = rng.standard_normal(tuple(slots_t.shape)).astype(np.float32)
        go = rng.standard_normal((b.num_dst, R * dim)).astype(np.float32)
        h, w = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(wv).cuda().requires_grad_(True)
        out = b.rel_sum_aggregate(h, et, R, w)
        assert out.shape == (b.num_dst, R, dim) and out.grad_fn is not None and "RelSum" in type(out.grad_fn).__name__, f"{name}: not the native op"
        (out * torch.from_numpy(go).cuda().view_as(out)).sum().backward()
        h64, w64 = torch.from_numpy(x).cuda().double().requires_grad_(True), torch.from_numpy(wv).cuda().double().requires_grad_(True)
        ref = b.rel_sum_aggregate_torch(h64, et, R, w64)
        (ref * torch.from_numpy(go).cuda().double().view_as(ref)).sum().backward()
        if b.nbr is not None:
            rows, slots, srcs = _edges(nbr=b.nbr.cpu().numpy())
        else:
            rows, slots, srcs = _edges(indptr=b.indptr.cpu().numpy(), idx=b.indices.cpu().numpy())
        tn = et.cpu().numpy().astype(np.int32)
        _check(torch, rows, slots, srcs, tn, wv, x, go, b.num_dst, R, out.detach().cpu().numpy(), h.grad.cpu().numpy(), w.grad.cpu().numpy(), name)
        _check(torch, rows, slots, srcs, tn, wv, x, go, b.num_dst, R, ref.detach().cpu().numpy(), h64.grad.cpu().numpy(), w64.grad.cpu().numpy(),
               name + " (fallback)")
        # unit weights: no grad_w is made, and a forward alone needs no gradient
        h2 = torch.from_numpy(x).cuda().requires_grad_(True)
        o2 = b.rel_sum_aggregate(h2, et.to(torch.int32), R)
        (o2 * torch.from_numpy(go).cuda().view_as(o2)).sum().backward()
        _check(torch, rows, slots, srcs, tn, None, x, go, b.num_dst, R, o2.detach().cpu().numpy(), h2.grad.cpu().numpy(), None, name + " w = None")
    assert forms == {False, True}


def test_relgraphconv_against_float64(hiplib):
    """One RelGraphConv layer, 128 -> 32, R = 4, 'basis' with 2 bases, without bias and self-loop, on a sampled block with
    norm = 1 / c_{d,r}, against the same formula in float64.

    The bound.  out[d, o] = sum over (r, i) of A[d, r, i] V[r, i, o], K = R * in terms, with A the aggregate and V_r = c_r0 W_0 + c_r1 W_1.
    A[d, r, i] is a sum of at most f terms norm_j x[s_j, i] with one fma each: a term passes at most f roundings,
    |A^ - A| <= gamma(f) sum_j |norm_j x_j| =: gamma(f) a.  V^ is two products and an addition (or a product and an fma): a term passes
    at most 2 roundings, |V^ - V| <= gamma(2) (|c_r0 W_0| + |c_r1 W_1|) =: gamma(2) v.  The GEMM adds K products in some order, with or
    without fmas: a term passes at most K roundings.  With (1 + gamma(a)) (1 + gamma(b)) <= 1 + gamma(a + b):
        |out^ - out| <= gamma(K + f + 2) sum over (r, i) of a[d, r, i] v[r, i, o],      n = R * in + f + 2."""
    import torch
    from COALA_GNN.nn import RelGraphConv
    torch.manual_seed(0)
    R, fin, fout = 4, 128, 32
    name, b = _sampled_blocks(torch, R)[0]
    assert b.nbr is not None
    f = b.nbr.shape[1]
    layer = RelGraphConv(fin, fout, R, regularizer="basis", num_bases=2, bias=False, self_loop=False).cuda()
    et = b.edata["etype"]
    cnt = b.rel_in_degrees(et, R)
    rows = torch.arange(b.num_dst, device="cuda").unsqueeze(1).expand_as(et)
    norm = (1.0 / cnt[rows, et].clamp_min(1)).float()
    h = torch.randn(b.num_src, fin, device="cuda")
    with torch.no_grad():
        got = layer(b, h, et, norm.unsqueeze(-1))
        c, W = layer.linear_r.coeff.double(), layer.linear_r.W.double()
        V = torch.einsum("rb,bio->rio", c, W)
        v = torch.einsum("rb,bio->rio", c.abs(), W.abs())
        A = b.rel_sum_aggregate_torch(h.double(), et, R, norm.double())
        a = b.rel_sum_aggregate_torch(h.double().abs(), et, R, norm.double())
        want = A.reshape(b.num_dst, R * fin) @ V.reshape(R * fin, fout)
        mag = a.reshape(b.num_dst, R * fin) @ v.reshape(R * fin, fout)
    err = (got.double() - want).abs()
    bound = float(_gamma(R * fin + f + 2)) * mag
    print(f"RelGraphConv: largest err / bound {(err / bound.clamp_min(1e-300)).max().item():.4f}")
    assert got.shape == (b.num_dst, fout) and bool((err <= bound + 1e-30).all())
    assert bool((want.abs().sum(1) > 0).any())


def test_rgcn_trains_through_the_loader(hiplib, oracle, tmp_path, monkeypatch):
    """The loop of test_max_aggregate_gpu.py::test_models_on_max_aggregation_train_through_the_loader (2 epochs of 11 steps, batch 64,
    fan-out 5,5, prefetching loader) with harness.RGCN on 4 relations.  Every layer call reaches the native op on the GPU and the
    fallback is never entered.  The labels are a function of a node's own first five feature columns, which reach the output through
    both layers' loop_weight, so the loss comes down."""
    import torch
    from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, SSD_INFO
    from COALA_GNN.harness import RGCN
    from COALA_GNN.sampler import Block, NeighborSampler
    from COALA_GNN.synthetic import alloc_pinned_table, block_colors, edge_types_by_source, feature_rows_torch, powerlaw_csc
    torch.manual_seed(0)
    n_nodes, dim, batch, fan, n_cls, R = 20000, 128, 64, [5, 5], 5, 4
    table = alloc_pinned_table(n_nodes, dim, seed=3, device=0)
    indptr, indices = powerlaw_csc(n_nodes, 8.0, seed=1, device="cuda")
    labels = feature_rows_torch(torch.arange(n_nodes, device="cuda"), dim, 3)[:, :n_cls].argmax(1)
    color, tk, sc, ncol = block_colors(n_nodes, nodes_per_color=512)
    files = ColorFiles(tmp_path, color, tk, sc)
    comm = MPI_Comm_Manager(0)
    comm.initialize_nested_process_group("isolated")
    train_ids = torch.randperm(int(0.6 * n_nodes), generator=torch.Generator().manual_seed(0))[:64 * 12]
    nd = Node_Distributor(comm, train_ids, batch, files.color_file, files.topk_file, files.score_file, parsing_method="baseline")
    sampler = NeighborSampler(fan, seed=5, edge_ids=True)
    g = sampler.make_graph(indptr, indices, ndata={"labels": labels}, edata={"etype": edge_types_by_source(indices, R)})
    loader = COALA_GNN_DataLoader(SSD_INFO(1, dim * 4, 1024, 0), nd, g, sampler, batch, dim, fan, 4, "cuda:0", refresh_counter=3,
                                  cache_backend="isolated", sim_buf=table, num_rows=n_nodes, prefetch=1)
    model = RGCN(dim, 64, n_cls, len(fan), R).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    native_calls, fallback_calls, losses = [], [], []
    native, fallback = Block.rel_sum_aggregate, Block.rel_sum_aggregate_torch
    monkeypatch.setattr(Block, "rel_sum_aggregate", lambda self, h, *a, **k: (native_calls.append(h.is_cuda), native(self, h, *a, **k))[1])
    monkeypatch.setattr(Block, "rel_sum_aggregate_torch", lambda self, *a, **k: (fallback_calls.append(1), fallback(self, *a, **k))[1])
    for epoch in range(2):
        for input_nodes, seeds, blocks, feat in loader:
            batch_labels = blocks[-1].dstdata["labels"].view(-1)
            loss = torch.nn.functional.cross_entropy(model(blocks, feat), batch_labels)
            opt.zero_grad(); loss.backward(); opt.step()
            losses.append(loss.item())
    print("losses:", " ".join(f"{x:.4f}" for x in losses))
    assert len(native_calls) == 2 * 22 and all(native_calls) and not fallback_calls, "a layer did not reach the native op on the GPU"
    assert len(losses) == 22 and all(math.isfinite(x) for x in losses)
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5, losses
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    for layer in model.layers:
        for r in range(R):
            assert bool((layer.linear_r.W.grad[r] != 0).any()), f"relation {r} got no gradient"
    del loader
    table.close()


@pytest.mark.parametrize("extra", [["--model_type", "rgcn", "--num_rels", "4"],
                                   ["--model_type", "rgcn", "--rgcn_regularizer", "basis", "--num_bases", "2", "--sampler", "labor",
                                    "--eval_fan_out=-1,-1"]])
def test_example_training_script_runs_rgcn(extra):
    """examples/train_synthetic.py --model_type rgcn, in a fresh process, at the size of
    test_max_aggregate_gpu.py::test_example_training_script_runs_pool_and_gin, for one epoch."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "train_synthetic.py"), "--nodes", "60000", "--dim", "64",
                          "--batch_size", "256", "--epochs", "1", "--cache_size", "4", "--prefetch", "1"] + extra,
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    loss = re.search(r"final loss (\S+)", out.stdout)
    assert loss and math.isfinite(float(loss.group(1))), out.stdout[-2000:]
    assert "Test Acc" in out.stdout
