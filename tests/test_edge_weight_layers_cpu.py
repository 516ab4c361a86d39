"""CPU twin of test_edge_weight_layers_gpu.py: GraphConv / SAGEConv with edge_weight= on the torch fallback of
Block.weighted_sum_aggregate, in float64, against the dense-adjacency computation of tests/_edge_weight_layers.py; and the fallback
itself: its gradients by torch.autograd.gradcheck, its values against an explicit loop, the C entry points' argument checks (made
before anything touches a device)."""
import numpy as np
import pytest

from _edge_weight_layers import check_layers, check_sageconv_state_dict, check_unweighted_graphconv_unchanged, small_block


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("in_feats,out_feats", [(20, 8), (8, 20)])
def test_layers_with_edge_weight_against_dense_adjacency(hiplib, in_feats, out_feats, ragged):
    import torch
    check_layers("cpu", torch.float64, in_feats, out_feats, ragged)


@pytest.mark.parametrize("ragged", [False, True])
def test_graphconv_without_edge_weight_is_unchanged(hiplib, ragged):
    check_unweighted_graphconv_unchanged("cpu", ragged)


def test_sageconv_loads_dgl_state_dict(hiplib):
    check_sageconv_state_dict()


@pytest.mark.parametrize("ragged", [False, True])
def test_fallback_values_and_gradcheck(hiplib, ragged):
    import torch
    b, nbr, w, d_w = small_block("cpu", ragged=ragged)
    torch.manual_seed(0)
    h = torch.randn(b.num_src, 5, dtype=torch.float64, requires_grad=True)
    wt = d_w.double().requires_grad_(True)
    out = b.weighted_sum_aggregate(h, wt)          # CPU tensors: the fallback
    assert torch.equal(out, b.weighted_sum_aggregate_torch(h, wt))
    want = np.zeros((b.num_dst, 5))
    for d in range(b.num_dst):
        for j in range(nbr.shape[1]):
            if nbr[d, j] >= 0:
                want[d] += float(w[d, j]) * h.detach().numpy()[nbr[d, j]]
    assert np.allclose(out.detach().numpy(), want, rtol=0, atol=1e-12) and np.all(out.detach().numpy()[1] == 0)
    assert torch.autograd.gradcheck(b.weighted_sum_aggregate_torch, (h, wt))
    if not ragged:                                  # the weight of a padding slot is not read: no gradient reaches it
        out.sum().backward()
        assert torch.all(wt.grad[torch.from_numpy(nbr < 0)] == 0)
    with pytest.raises(ValueError, match="one per neighbour slot"):
        b.weighted_sum_aggregate(h, wt.reshape(-1)[:-1])


def test_block_edata_defaults_and_sampler_option(hiplib):
    import torch
    from COALA_GNN import sampler as S
    assert S.EID == "_ID" and "EID" in S.__all__
    b = S.Block(torch.arange(4), torch.zeros((2, 2), dtype=torch.int32), 2)
    assert b.edata == {} and S.NeighborSampler([5, 5]).edge_ids is False and S.NeighborSampler([5], edge_ids=True).edge_ids is True
    eid = torch.tensor([[3, -1], [0, 2]])
    b = S.Block(torch.arange(4), torch.tensor([[1, -1], [0, 2]], dtype=torch.int32), 2, eid=eid)
    assert list(b.edata) == ["_ID"] and any(t is eid for t in b.tensors())


def test_weighted_sum_entry_points_refuse_bad_shapes_without_a_device(hiplib):
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    for n_dst, f, dim in ((1, 0, 4), (1, 33, 4), (1, 4, 0), (-1, 4, 4), (0, 33, 4)):
        assert L.coala_block_weighted_sum(0, None, None, None, None, n_dst, f, dim, None) == _capi.EINVAL
        assert "bad block shape" in _capi.last_error()
        assert L.coala_block_weighted_sum_backward(0, None, None, None, None, None, None, n_dst, f, dim, None) == _capi.EINVAL
    for n_dst, dim in ((1, 0), (-1, 4)):
        assert L.coala_block_weighted_sum_csr(0, None, None, None, None, None, n_dst, dim, None) == _capi.EINVAL
        assert L.coala_block_weighted_sum_csr_backward(0, None, None, None, None, None, None, None, n_dst, dim, None) == _capi.EINVAL
    assert L.coala_block_weighted_sum(0, None, None, None, None, 4, 4, 4, None) == _capi.EINVAL and "null buffer" in _capi.last_error()
    assert L.coala_block_weighted_sum(0, None, None, None, None, 0, 4, 4, None) == _capi.OK
    lay = (_capi.SamplerLayer * 1)()
    import ctypes as C
    assert L.coala_sampler_sample_layers_edge_ids(None, None, 0, (C.c_int32 * 1)(5), 1, 0, 0, lay, None, None, None, None, None, None,
                                                  None) == _capi.EINVAL
    assert L.coala_abi_version() == 4
