"""Dispatch parity of Block.*_aggregate, shared by the CPU twin and the GPU test (tests only): whatever path an input takes -- a
native kernel or the torch fallback -- the result has the shape and the values of the *_aggregate_torch reference evaluated in float64
on the CPU.  Every input here is valid for the fallback.

Tolerance, as for the whole-model tests: E = the largest difference between the reference evaluated in the input's dtype on the CPU
and in float64; the result is within 4 E, and never asked to be closer than 8 u times the reference's largest magnitude, u the unit
roundoff of the input's dtype (2^-24 fp32, 2^-11 fp16, 2^-53 fp64)."""
import numpy as np
import torch

from COALA_GNN.sampler import Block

OPS = ("mean", "weighted_sum", "max", "rel_sum", "gat")
FORMS = ("fixed", "ragged")
INPUTS = ("3d", "colslice", "transposed", "fp64", "fp16", "fanout33", "nbr_slice")
N_SRC, N_DST, DIM, H, D, RELS = 90, 37, 10, 2, 6, 3
UNIT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.float64: 2.0 ** -53}


def _block(device, form, nbr, slice_slots):
    """A block over the -1 padded nbr array; slice_slots: the slot array is a non-contiguous view (a column slice of a wider array
    for the fixed form, every other element of a longer one for the ragged form)."""
    src = torch.arange(N_SRC, device=device)
    if form == "fixed":
        t = torch.from_numpy(nbr)
        if slice_slots:
            wide = torch.full((nbr.shape[0], nbr.shape[1] + 5), -1, dtype=torch.int32)
            wide[:, 2: 2 + nbr.shape[1]] = t
            t = wide.to(device)[:, 2: 2 + nbr.shape[1]]
            assert not t.is_contiguous()
        return Block(src, t.to(device), N_DST)
    valid = nbr >= 0
    indptr = np.zeros(N_DST + 1, dtype=np.int64)
    np.cumsum(valid.sum(1), out=indptr[1:])
    idx = torch.from_numpy(nbr[valid])
    if slice_slots:
        wide = torch.zeros(2 * len(idx), dtype=torch.int32)
        wide[::2] = idx
        idx = wide.to(device)[::2]
        assert not idx.is_contiguous()
    return Block(src, None, N_DST, indptr=torch.from_numpy(indptr).to(device), indices=idx.to(device))


def case(device, op, form, inp):
    """-> (got, want float64 CPU tensor, want evaluated in the input dtype on the CPU or None, input dtype)"""
    rng = np.random.default_rng(OPS.index(op) * 100 + FORMS.index(form) * 10 + INPUTS.index(inp))
    f = 33 if inp == "fanout33" else 7
    nbr = rng.integers(0, N_SRC, size=(N_DST, f)).astype(np.int32)
    nbr[rng.random((N_DST, f)) < 0.25] = -1
    nbr[3] = -1                                                  # a destination without an in-edge
    nbr[5] = np.arange(f)                                        # a full row
    dtype = {"fp64": torch.float64, "fp16": torch.float16}.get(inp, torch.float32)
    gat = op == "gat"
    if inp == "colslice":
        base = torch.from_numpy(rng.standard_normal((N_SRC, H, D + 2) if gat else (N_SRC, DIM + 10)).astype(np.float32))
        view = (lambda t: t[:, :, 1: 1 + D]) if gat else (lambda t: t[:, 3: 3 + DIM])
    elif inp == "transposed":
        base = torch.from_numpy(rng.standard_normal((H, N_SRC, D) if gat else (DIM, N_SRC)).astype(np.float32))
        view = (lambda t: t.transpose(0, 1)) if gat else (lambda t: t.t())
    else:
        base = torch.from_numpy(rng.standard_normal((N_SRC, H, D) if gat or inp == "3d" else (N_SRC, DIM)).astype(np.float32)).to(dtype)
        view = lambda t: t
    if inp in ("colslice", "transposed"):
        assert not view(base).is_contiguous()
    slots = nbr if form == "fixed" else nbr[nbr >= 0]
    w = torch.from_numpy((0.1 + rng.random(slots.shape)).astype(np.float32))
    etype = torch.from_numpy(rng.integers(0, RELS, size=slots.shape).astype(np.int64))
    el = torch.from_numpy(rng.standard_normal((N_SRC, H)).astype(np.float32)).to(dtype)
    er = torch.from_numpy(rng.standard_normal((N_DST, H)).astype(np.float32)).to(dtype)

    def call(block, fn_suffix, dev, dt):
        h = view(base.to(dev)) if dt is None else view(base).to(dt).to(dev)
        cast = (lambda t: t.to(dev)) if dt is None else (lambda t: t.to(dt).to(dev))
        if op == "mean":
            return getattr(block, "mean_aggregate" + fn_suffix)(h)
        if op == "weighted_sum":
            return getattr(block, "weighted_sum_aggregate" + fn_suffix)(h, w.to(dev) if dt is None else cast(w))
        if op == "max":
            return getattr(block, "max_aggregate" + fn_suffix)(h)
        if op == "rel_sum":
            return getattr(block, "rel_sum_aggregate" + fn_suffix)(h, etype.to(dev), RELS, w.to(dev) if dt is None else cast(w))
        return getattr(block, "gat_aggregate" + fn_suffix)(cast(el), cast(er), h)

    got = call(_block(device, form, nbr, inp == "nbr_slice"), "", device, None)
    host = _block("cpu", form, nbr, False)
    want = call(host, "_torch", "cpu", torch.float64)
    try:
        low = call(host, "_torch", "cpu", dtype).double()
    except RuntimeError:       # an op the CPU does not have in this dtype (fp16): the floor alone then bounds the error
        low = None
    return got, want, low, dtype


def check(device, op, form, inp, log=print):
    got, want, low, dtype = case(device, op, form, inp)
    assert tuple(got.shape) == tuple(want.shape), f"shape {tuple(got.shape)}, the reference gives {tuple(want.shape)}"
    assert got.dtype == dtype
    e = float((low - want).abs().max()) if low is not None else 0.0
    tol = max(4.0 * e, 8.0 * UNIT[dtype] * float(want.abs().max()))
    err = float((got.detach().double().cpu() - want).abs().max())
    log(f"{op}-{form}-{inp}: error {err:.3e} E {e:.3e} bound {tol:.3e}")
    assert err <= tol, f"error {err:.3e} above {tol:.3e}"
