"""CPU tests of Block.lstm_aggregate_torch (the fallback and, in float64, the reference of the native kernels): against the numpy step loop
on both block forms, against torch.nn.LSTM on full rows (which pins the gate order i, f, g, o and the bias sum); LSTMSAGEConv's names."""
import numpy as np
import pytest
import torch

from _lstm_ref import lstm_ref, valid_rows

H, N_SRC = 6, 20


def _blocks(nbr):
    from COALA_GNN.sampler import Block
    src, rows = torch.arange(N_SRC), valid_rows(nbr)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = torch.tensor([s for r in rows for s in r], dtype=torch.int32)
    return Block(src, torch.from_numpy(nbr), len(nbr)), Block(src, None, len(nbr), indptr=torch.from_numpy(indptr), indices=indices)


@pytest.mark.parametrize("form", [0, 1])
def test_lstm_aggregate_torch_against_numpy(hiplib, form):
    rng = np.random.default_rng(form)
    nbr = rng.integers(0, N_SRC - 3, size=(9, 5)).astype(np.int32)
    nbr[rng.random(nbr.shape) < 0.3] = -1
    nbr[2], nbr[4], nbr[6] = -1, [3, -1, 3, -1, 7], [-1, -1, -1, -1, 1]    # empty; a repeat around a hole; one late slot
    xg, w = rng.standard_normal((N_SRC, 4 * H)), rng.standard_normal((4 * H, H))
    go = rng.standard_normal((9, H))
    want = lstm_ref(valid_rows(nbr), xg, w, go)
    block = _blocks(nbr)[form]
    for fn in (block.lstm_aggregate_torch, block.lstm_aggregate):            # on the CPU lstm_aggregate is its fallback
        t_xg, t_w = torch.from_numpy(xg).requires_grad_(), torch.from_numpy(w).requires_grad_()
        out = fn(t_xg, t_w)
        (out * torch.from_numpy(go)).sum().backward()
        for got, ref in zip((out.detach(), t_xg.grad, t_w.grad), want):
            assert got.dtype == torch.float64 and np.allclose(got.numpy(), ref, rtol=1e-12, atol=1e-13)
        assert torch.all(out[2] == 0) and torch.all(t_xg.grad[N_SRC - 3:] == 0)


def test_lstm_aggregate_torch_against_nn_lstm(hiplib):
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(H, H, batch_first=True).double()
    x = torch.randn(N_SRC, H, dtype=torch.float64)
    nbr = torch.randint(0, N_SRC, (7, 4), dtype=torch.int32)
    want = lstm(x[nbr.long()])[1][0][0]                                      # h_n of the [7, 4, H] mailbox
    xg = x @ lstm.weight_ih_l0.t() + lstm.bias_ih_l0 + lstm.bias_hh_l0
    got = _blocks(nbr.numpy())[0].lstm_aggregate_torch(xg, lstm.weight_hh_l0)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-13)


def test_lstm_sage_conv_names(hiplib):
    from COALA_GNN.nn import LSTMSAGEConv
    shapes = {k: tuple(v.shape) for k, v in LSTMSAGEConv((8, 5), 3).state_dict().items()}
    assert shapes == {"lstm.weight_ih_l0": (32, 8), "lstm.weight_hh_l0": (32, 8), "lstm.bias_ih_l0": (32,), "lstm.bias_hh_l0": (32,),
                      "fc_self.weight": (3, 5), "fc_neigh.weight": (3, 8), "bias": (3,)}
