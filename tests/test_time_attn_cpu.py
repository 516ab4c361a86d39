"""CPU tests of temporal attention: Block.time_attn_aggregate_torch (the factorised fallback) and TGATConv against the float64 per-edge
restatement in tests/_time_attn_ref.py -- outputs and every gradient, omega and phase included."""
import numpy as np
import pytest
import torch

import _time_attn_ref as R


def _block(nbr, n_src):
    from COALA_GNN.sampler import Block
    return Block(torch.arange(n_src), nbr, nbr.shape[0])


@pytest.mark.parametrize("n_dst,fan,H,D,T", [(1, 1, 1, 1, 1), (9, 5, 3, 4, 7), (0, 4, 2, 8, 4)])
def test_factorised_fallback_is_the_per_edge_form(hiplib, n_dst, fan, H, D, T):
    rng = np.random.default_rng(1)
    n_src = 12
    nbr = torch.from_numpy(R.block_rows(rng, n_dst, fan, n_src))
    dt = torch.from_numpy(rng.integers(0, 5000, size=(n_dst, fan)))
    shapes = dict(q=(n_dst, H, D), k=(n_src, H, D), v=(n_src, H, D), qt=(n_dst, H, T), omega=(T,), phase=(T,))
    a = {n: torch.from_numpy(rng.standard_normal(s)).requires_grad_() for n, s in shapes.items()}
    b = {n: t.detach().clone().requires_grad_() for n, t in a.items()}
    got = _block(nbr, n_src).time_attn_aggregate(a["q"], a["k"], a["v"], a["qt"], dt, a["omega"], a["phase"])
    want = R.op_ref(nbr, b["q"], b["k"], b["v"], b["qt"], dt, b["omega"], b["phase"])
    go = [torch.from_numpy(rng.standard_normal(tuple(t.shape))) for t in want]
    torch.autograd.backward(got, go)
    torch.autograd.backward(want, go)
    for name, g, w in [("out", got[0], want[0]), ("tagg", got[1], want[1])] + [(n, a[n].grad, b[n].grad) for n in shapes]:
        torch.testing.assert_close(g, w, rtol=1e-11, atol=1e-11, msg=lambda m, name=name: f"{name}: {m}")
    if n_dst >= 3:
        assert not got[0][1].any() and not got[1][1].any() and not a["q"].grad[1].any() and not a["qt"].grad[1].any()


def test_tgatconv_is_the_per_edge_layer(hiplib):
    from COALA_GNN.nn import TGATConv, TimeEncode
    rng = np.random.default_rng(2)
    n_dst, fan, n_src, F = 8, 5, 11, 6
    nbr = torch.from_numpy(R.block_rows(rng, n_dst, fan, n_src))
    dt = torch.from_numpy(rng.integers(0, 1 << 20, size=(n_dst, fan)))
    torch.manual_seed(0)
    conv = TGATConv(F, 12, 3, 10, time_scale=1e-3).double()
    enc = TimeEncode(10)
    assert torch.equal(enc.omega.detach(), 1.0 / 10.0 ** torch.linspace(0, 9, 10)) and not enc.phase.detach().any()
    assert torch.equal(enc(torch.tensor([0, 3])), torch.cos(torch.tensor([[0.0], [3.0]]) * enc.omega))
    with torch.no_grad():
        conv.time_encoder.phase.add_(torch.from_numpy(rng.standard_normal(10)))   # off its initial value, where d/d phase of cos is 0 at dt = 0
    h = torch.from_numpy(rng.standard_normal((n_src, F))).requires_grad_()
    go = torch.from_numpy(rng.standard_normal((n_dst, 12)))
    grads = []
    for run in ("layer", "ref"):
        conv.zero_grad()
        h.grad = None
        y = conv(_block(nbr, n_src), (h, h[:n_dst]), dt) if run == "layer" else R.layer_ref(conv, nbr, h, h[:n_dst], dt)
        y.backward(go)
        grads.append([y.detach()] + [h.grad.clone()] + [p.grad.clone() for p in conv.parameters()])
    names = ["out", "h"] + [n for n, _ in conv.named_parameters()]
    for name, g, w in zip(names, *grads):
        assert w.abs().max() > 0, name
        torch.testing.assert_close(g, w, rtol=1e-10, atol=1e-12, msg=lambda m, name=name: f"{name}: {m}")
