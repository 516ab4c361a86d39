"""CPU tests of the GAT / GCN surface: Block.gat_aggregate_torch (the fallback and reference of the native kernels) against a
float64 restatement of the attention formulas, its gradients (gradcheck), GATConv and GraphConv against hand-written float64
layers, the block degree methods, and GATConv's DGL parameter names and shapes."""
import numpy as np
import pytest

SLOPE = 0.2


def _ref_gat(rows_of, el, er, feat, slope=SLOPE):
    """float64 restatement: rows_of[d] lists the source of every valid in-edge of d, in order."""
    n_dst, H, D = len(rows_of), feat.shape[1], feat.shape[2]
    out = np.zeros((n_dst, H, D))
    for d, srcs in enumerate(rows_of):
        if not srcs:
            continue
        s = np.asarray(srcs)
        z = el[s] + er[d]                                   # [k, H]
        e = np.where(z > 0, z, z * slope)
        a = np.exp(e - e.max(0))
        a /= a.sum(0)
        out[d] = np.einsum("kh,khd->hd", a, feat[s])
    return out


def _fixed_case(rng, n_dst=40, f=7, n_src=30, H=3, D=5, big=False):
    nbr = rng.integers(0, n_src, size=(n_dst, f)).astype(np.int32)
    nbr[rng.random((n_dst, f)) < 0.3] = -1                 # -1 anywhere in a row
    nbr[3] = -1                                            # a row without a valid edge
    nbr[4, :] = nbr[4, 0] if nbr[4, 0] >= 0 else 2         # one source repeated over a whole row
    nbr[5, 1] = nbr[5, 0] = 7                              # a source twice
    el = rng.standard_normal((n_src, H))
    er = rng.standard_normal((n_dst, H))
    if big:                                                # scores up to +-1e3
        el *= 1e3
        er *= 1e3
    feat = rng.standard_normal((n_src, H, D))
    rows_of = [[int(s) for s in r if s >= 0] for r in nbr]
    return nbr, el, er, feat, rows_of


def _ragged_case(rng, n_dst=25, n_src=40, H=2, D=4, big=False):
    deg = rng.integers(0, 12, size=n_dst)
    deg[[0, 7]] = 0                                        # rows without an edge
    deg[9] = 150                                           # longer than one 64-edge chunk
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rng.integers(0, n_src, size=int(indptr[-1])).astype(np.int32)
    indices[indptr[3]: indptr[4]] = 5                      # repeated sources
    el = rng.standard_normal((n_src, H)) * (1e3 if big else 1.0)
    er = rng.standard_normal((n_dst, H)) * (1e3 if big else 1.0)
    feat = rng.standard_normal((n_src, H, D))
    rows_of = [[int(s) for s in indices[indptr[d]: indptr[d + 1]]] for d in range(n_dst)]
    return indptr, indices, el, er, feat, rows_of


def _fixed_block(torch, nbr, n_src):
    from COALA_GNN.sampler import Block
    return Block(torch.arange(n_src), torch.from_numpy(nbr), nbr.shape[0])


def _ragged_block(torch, indptr, indices, n_src):
    from COALA_GNN.sampler import Block
    return Block(torch.arange(n_src), None, len(indptr) - 1, indptr=torch.from_numpy(indptr), indices=torch.from_numpy(indices))


@pytest.mark.parametrize("big", [False, True])
def test_gat_aggregate_torch_fixed_matches_float64(hiplib, big):
    import torch
    rng = np.random.default_rng(1 + big)
    nbr, el, er, feat, rows_of = _fixed_case(rng, big=big)
    b = _fixed_block(torch, nbr, el.shape[0])
    got = b.gat_aggregate_torch(torch.from_numpy(el), torch.from_numpy(er), torch.from_numpy(feat), SLOPE).numpy()
    ref = _ref_gat(rows_of, el, er, feat)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    assert np.all(got[3] == 0.0) and np.isfinite(got).all()


@pytest.mark.parametrize("big", [False, True])
def test_gat_aggregate_torch_ragged_matches_float64(hiplib, big):
    import torch
    rng = np.random.default_rng(3 + big)
    indptr, indices, el, er, feat, rows_of = _ragged_case(rng, big=big)
    b = _ragged_block(torch, indptr, indices, el.shape[0])
    got = b.gat_aggregate_torch(torch.from_numpy(el), torch.from_numpy(er), torch.from_numpy(feat), SLOPE).numpy()
    np.testing.assert_allclose(got, _ref_gat(rows_of, el, er, feat), rtol=1e-12, atol=1e-12)
    assert np.all(got[[0, 7]] == 0.0) and np.isfinite(got).all()


def test_gat_aggregate_dispatches_cpu_tensors_to_torch(hiplib):
    import torch
    rng = np.random.default_rng(5)
    nbr, el, er, feat, rows_of = _fixed_case(rng, H=2, D=3)
    b = _fixed_block(torch, nbr, el.shape[0])
    t = [torch.from_numpy(x).float() for x in (el, er, feat)]
    got = b.gat_aggregate(*t).numpy()
    np.testing.assert_allclose(got, _ref_gat(rows_of, el, er, feat), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_gat_aggregate_torch_gradcheck(hiplib, form):
    import torch
    rng = np.random.default_rng(7)
    if form == "fixed":
        nbr, el, er, feat, _ = _fixed_case(rng, n_dst=9, f=4, n_src=8, H=2, D=3)
        b = _fixed_block(torch, nbr, el.shape[0])
    else:
        indptr, indices, el, er, feat, _ = _ragged_case(rng, n_dst=12, n_src=10, H=2, D=3)
        b = _ragged_block(torch, indptr, indices, el.shape[0])
    args = [torch.from_numpy(x).requires_grad_(True) for x in (el, er, feat)]
    assert torch.autograd.gradcheck(lambda a, c, f: b.gat_aggregate_torch(a, c, f, SLOPE), args)


def test_block_degrees_and_counts(hiplib):
    import torch
    rng = np.random.default_rng(11)
    nbr, _, _, _, _ = _fixed_case(rng)
    b = _fixed_block(torch, nbr, 30)
    assert b.num_dst_nodes() == 40 and b.num_src_nodes() == 30
    v = nbr[nbr >= 0]
    np.testing.assert_array_equal(b.in_degrees().numpy(), (nbr >= 0).sum(1))
    np.testing.assert_array_equal(b.out_degrees().numpy(), np.bincount(v, minlength=30))
    indptr, indices, _, _, _, _ = _ragged_case(rng)
    r = _ragged_block(torch, indptr, indices, 40)
    assert r.num_dst_nodes() == 25 and r.num_src_nodes() == 40
    np.testing.assert_array_equal(r.in_degrees().numpy(), np.diff(indptr))
    np.testing.assert_array_equal(r.out_degrees().numpy(), np.bincount(indices, minlength=40))


def test_gatconv_parameters_follow_dgl(hiplib):
    from COALA_GNN.nn import GATConv
    m = GATConv((12, 10), 6, 4)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == {"fc_src.weight": (24, 12), "fc_dst.weight": (24, 10), "attn_l": (1, 4, 6), "attn_r": (1, 4, 6), "bias": (24,)}


@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_gatconv_matches_float64(hiplib, form):
    import torch
    from COALA_GNN.nn import GATConv
    rng = np.random.default_rng(13)
    if form == "fixed":
        nbr, _, _, _, rows_of = _fixed_case(rng, n_dst=40, n_src=60)
        b = _fixed_block(torch, nbr, 60)
    else:
        indptr, indices, _, _, _, rows_of = _ragged_case(rng, n_src=60)
        b = _ragged_block(torch, indptr, indices, 60)
    n_dst, H, D, F = b.num_dst, 3, 4, 9
    conv = GATConv((F, F), D, H).double()
    with torch.no_grad():
        conv.bias.copy_(torch.from_numpy(rng.standard_normal(H * D)))
    x = rng.standard_normal((60, F))
    got = conv(b, (torch.from_numpy(x), torch.from_numpy(x[:n_dst]))).detach().numpy()
    sd = {k: v.numpy() for k, v in conv.state_dict().items()}
    fs = (x @ sd["fc_src.weight"].T).reshape(60, H, D)
    fd = (x[:n_dst] @ sd["fc_dst.weight"].T).reshape(n_dst, H, D)
    el = (fs * sd["attn_l"]).sum(-1)
    er = (fd * sd["attn_r"]).sum(-1)
    ref = _ref_gat(rows_of, el, er, fs) + sd["bias"].reshape(1, H, D)
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-10)
    empty = [d for d, r in enumerate(rows_of) if not r]
    assert empty and np.all(got[empty] == sd["bias"].reshape(1, H, D))   # zero in-degree: exactly the bias


@pytest.mark.parametrize("form,fin,fout", [("fixed", 9, 4), ("fixed", 4, 9), ("ragged", 9, 4), ("ragged", 4, 9)])
def test_graphconv_matches_float64(hiplib, form, fin, fout):
    import torch
    from COALA_GNN.nn import GraphConv
    rng = np.random.default_rng(17 + fin)
    if form == "fixed":
        nbr, _, _, _, rows_of = _fixed_case(rng, n_dst=40, n_src=60)
        b = _fixed_block(torch, nbr, 60)
    else:
        indptr, indices, _, _, _, rows_of = _ragged_case(rng, n_src=60)
        b = _ragged_block(torch, indptr, indices, 60)
    conv = GraphConv(fin, fout).double()
    with torch.no_grad():
        conv.bias.copy_(torch.from_numpy(rng.standard_normal(fout)))
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == {"weight": (fin, fout), "bias": (fout,)}
    x = rng.standard_normal((60, fin))
    got = conv(b, (torch.from_numpy(x), torch.from_numpy(x[: b.num_dst]))).detach().numpy()
    W, bias = conv.weight.detach().numpy(), conv.bias.detach().numpy()
    out_deg = np.zeros(60)
    for r in rows_of:
        for s in r:
            out_deg[s] += 1
    ref = np.zeros((len(rows_of), fout))
    for d, r in enumerate(rows_of):
        acc = np.zeros(fin)
        for s in r:
            acc += x[s] / np.sqrt(max(out_deg[s], 1))
        ref[d] = acc / np.sqrt(max(len(r), 1)) @ W + bias
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-10)
    empty = [d for d, r in enumerate(rows_of) if not r]
    assert empty and np.all(got[empty] == bias)


def test_models_build_and_run_on_cpu_blocks(hiplib):
    """GAT and GCN of the harness: output shapes of a 2-layer model on CPU blocks (the fallback path), log-probabilities for GAT."""
    import torch
    from COALA_GNN.harness import GAT, GCN
    rng = np.random.default_rng(19)
    nbr1 = rng.integers(-1, 30, size=(12, 5)).astype(np.int32)     # layer 1: 12 dst among 30 src
    nbr2 = rng.integers(-1, 12, size=(4, 5)).astype(np.int32)      # layer 2: 4 dst among 12 src
    blocks = [_fixed_block(torch, nbr1, 30), _fixed_block(torch, nbr2, 12)]
    x = torch.randn(30, 8)
    out = GAT(8, 6, 5, 2, 4)(blocks, x)
    assert out.shape == (4, 5) and torch.allclose(out.exp().sum(1), torch.ones(4), atol=1e-5)
    assert GCN(8, 6, 5, 2)(blocks, x).shape == (4, 5)
