"""Checks of GraphConv / SAGEConv with edge_weight= against a dense-adjacency float64 computation, shared by the CPU twin (torch
fallback of Block.weighted_sum_aggregate) and the GPU test (native kernels).  Tests only.

Reference, for a block with count adjacency C[d, s] (how many valid slots of row d hold source s) and weighted adjacency
A[d, s] (the sum of their weights), in_deg = C.sum(1), out_deg = C.sum(0):
    GraphConv        D_in^-1/2 A D_out^-1/2 X W + b            (degrees clamped to 1; DGL: unweighted degrees with edge_weight)
    SAGEConv 'mean'  X_dst Ws^T + (A X / max(in_deg, 1)) Wn^T + b
    SAGEConv 'gcn'   ((A X + X_dst) / (in_deg + 1)) Wn^T + b
Bound: every output element is a sum of at most n = in_feats * (fan-out + 1) + 1 products of inputs, computed in fp32 in some order
with a few more roundings for the degree factors; an element is within (n + 8) u of the same sum taken over absolute values
(u = 2^-24).  In float64 the same holds with u = 2^-53."""
import numpy as np
import torch

from COALA_GNN.nn import GraphConv, SAGEConv
from COALA_GNN.sampler import Block


def small_block(device, f=6, n_dst=12, n_src=40, seed=0, ragged=False):
    rng = np.random.default_rng(seed)
    nbr = rng.integers(0, n_src, size=(n_dst, f)).astype(np.int32)
    nbr[rng.random((n_dst, f)) < 0.3] = -1
    nbr[1] = -1                                            # a destination without an in-edge
    nbr[2, :2] = 7                                         # a repeated edge
    w = (rng.random((n_dst, f)) + 0.1).astype(np.float32)
    if ragged:
        valid = nbr >= 0
        indptr = np.zeros(n_dst + 1, dtype=np.int64)
        np.cumsum(valid.sum(1), out=indptr[1:])
        b = Block(torch.arange(n_src, device=device), None, n_dst, indptr=torch.from_numpy(indptr).to(device),
                  indices=torch.from_numpy(nbr[valid]).to(device))
        return b, nbr, w, torch.from_numpy(w[valid]).to(device)
    return Block(torch.arange(n_src, device=device), torch.from_numpy(nbr).to(device), n_dst), nbr, w, torch.from_numpy(w).to(device)


def adjacency(nbr, w, n_src):
    A, Cn = np.zeros((len(nbr), n_src)), np.zeros((len(nbr), n_src))
    for d, j in zip(*np.nonzero(nbr >= 0)):
        A[d, nbr[d, j]] += float(w[d, j])
        Cn[d, nbr[d, j]] += 1.0
    return A, Cn


def _p(t):
    return t.detach().cpu().double().numpy()


def check_layers(device, dtype, in_feats, out_feats, ragged):
    u = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    torch.manual_seed(in_feats * 100 + out_feats)
    b, nbr, w, d_w = small_block(device, ragged=ragged)
    d_w = d_w.to(dtype)
    n_dst, f = nbr.shape
    n_src = b.num_src
    X = torch.randn(n_src, in_feats, dtype=dtype, device=device)
    A, Cn = adjacency(nbr, w, n_src)
    in_deg, out_deg = Cn.sum(1), Cn.sum(0)
    x = _p(X)
    k = (in_feats * (f + 1) + 1 + 8) * u

    conv = GraphConv(in_feats, out_feats).to(device=device, dtype=dtype)
    torch.nn.init.normal_(conv.bias)
    got = _p(conv(b, (X, X[:n_dst]), edge_weight=d_w))
    W, bias = _p(conv.weight), _p(conv.bias)
    norm = (np.maximum(in_deg, 1) ** -0.5)[:, None] * A * (np.maximum(out_deg, 1) ** -0.5)[None, :]
    ref, mag = norm @ x @ W + bias, np.abs(norm) @ np.abs(x) @ np.abs(W) + np.abs(bias)
    assert np.all(np.abs(got - ref) <= k * mag), f"GraphConv(edge_weight): max error {np.abs(got - ref).max()} bound {(k * mag).min()}"
    assert np.array_equal(got[1], bias), "a destination without an in-edge must get the bias alone"

    for agg in ("mean", "gcn"):
        conv = SAGEConv(in_feats, out_feats, agg).to(device=device, dtype=dtype)
        torch.nn.init.normal_(conv.bias)
        Wn, bias = _p(conv.fc_neigh.weight), _p(conv.bias)
        for weight, adj in ((d_w, A), (None, Cn)):
            got = _p(conv(b, X, edge_weight=weight))
            if agg == "mean":
                Ws = _p(conv.fc_self.weight)
                nrm = adj / np.maximum(in_deg, 1)[:, None]
                ref = x[:n_dst] @ Ws.T + nrm @ x @ Wn.T + bias
                mag = np.abs(x[:n_dst]) @ np.abs(Ws.T) + np.abs(nrm) @ np.abs(x) @ np.abs(Wn.T) + np.abs(bias)
            else:
                nrm = 1.0 / (in_deg + 1)[:, None]
                ref = ((adj @ x + x[:n_dst]) * nrm) @ Wn.T + bias
                mag = ((np.abs(adj) @ np.abs(x) + np.abs(x[:n_dst])) * nrm) @ np.abs(Wn.T) + np.abs(bias)
            assert np.all(np.abs(got - ref) <= k * mag), f"SAGEConv({agg}, weighted={weight is not None}): max error {np.abs(got - ref).max()}"


def check_unweighted_graphconv_unchanged(device, ragged):
    """edge_weight=None: the bits of the layer as it was before edge weights existed (its forward restated here)."""
    torch.manual_seed(1)
    b, nbr, _, _ = small_block(device, ragged=ragged)
    for in_feats, out_feats in ((20, 8), (8, 20)):
        conv = GraphConv(in_feats, out_feats, activation=torch.relu).to(device)
        X = torch.randn(b.num_src, in_feats, device=device)
        out_deg = b.out_degrees().to(device=device, dtype=X.dtype).clamp_min(1)
        in_deg = b.in_degrees().to(device=device, dtype=X.dtype).clamp_min(1)
        h = X * out_deg.pow(-0.5).unsqueeze(-1)
        if in_feats > out_feats:
            h = h @ conv.weight
        rst = b.mean_aggregate(h) * in_deg.sqrt().unsqueeze(-1)
        if in_feats <= out_feats:
            rst = rst @ conv.weight
        want = torch.relu(rst + conv.bias)
        assert torch.equal(conv(b, (X, X[: b.num_dst])), want) and torch.equal(conv(b, X, edge_weight=None), want)


def check_sageconv_state_dict():
    for agg, keys in (("mean", ["fc_self.weight", "fc_neigh.weight", "bias"]), ("gcn", ["fc_neigh.weight", "bias"])):
        conv = SAGEConv(10, 4, agg)
        assert sorted(conv.state_dict()) == sorted(keys)
        sd = {k: torch.randn(4, 10) if k.endswith("weight") else torch.randn(4) for k in keys}   # DGL's names and shapes
        conv.load_state_dict(sd, strict=True)
        assert all(torch.equal(conv.state_dict()[k], v) for k, v in sd.items())
    import pytest
    with pytest.raises(ValueError):
        SAGEConv(10, 4, "lstm")
