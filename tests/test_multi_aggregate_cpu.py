"""CPU tests of the multi-statistic aggregation: Block.multi_aggregate_torch against a Python loop over the rows, the refusals of
Block.multi_aggregate and PNAConv, the C symbols, PNAConv's parameter names, and PNAConv's split of M into a per-source and a
per-destination term against the per-edge restatement of _pna_ref.py (float64, the torch path)."""
import math

import numpy as np
import pytest
import torch

from _pna_ref import pna_reference

ALL = ("sum", "mean", "max", "min", "var", "std")
NBR = np.array([[3, -1, 5, 3], [-1, -1, -1, -1], [7, 7, 7, 7], [0, 1, 2, -1], [6, -1, -1, -1]], dtype=np.int32)


def hand_block(form):
    from COALA_GNN.sampler import Block
    src = torch.arange(8)
    if form == "fixed":
        return Block(src, torch.from_numpy(NBR), len(NBR))
    indptr = np.concatenate([[0], np.cumsum((NBR >= 0).sum(1))]).astype(np.int64)
    return Block(src, None, len(NBR), indptr=torch.from_numpy(indptr), indices=torch.from_numpy(NBR[NBR >= 0]))


@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_fallback_matches_a_loop_over_the_rows(hiplib, form):
    h = torch.from_numpy(np.random.default_rng(0).standard_normal((8, 3))) + 100.0
    eps = 1e-5
    got = hand_block(form).multi_aggregate(h, ALL[::-1], eps)         # float64 on the CPU: the torch path
    assert got.shape == (len(NBR), 6, 3) and got.dtype == torch.float64
    for d, row in enumerate(NBR):
        x = h[[int(s) for s in row if s >= 0]]
        for a, name in enumerate(ALL[::-1]):
            if len(x) == 0:
                want = torch.zeros(3, dtype=torch.float64)
            else:
                var = ((x - x.mean(0)) ** 2).mean(0)
                want = {"sum": x.sum(0), "mean": x.mean(0), "max": x.amax(0), "min": x.amin(0), "var": var, "std": (var + eps).sqrt()}[name]
            assert torch.allclose(got[d, a], want, rtol=1e-13, atol=0), (d, name)
    assert torch.equal(got[2, 1], torch.zeros(3, dtype=torch.float64)) and torch.equal(got[4, 1], got[2, 1])   # var of equal values, of one value


def test_refusals(hiplib):
    from COALA_GNN.nn import PNAConv
    blk, h = hand_block("fixed"), torch.zeros(8, 3)
    for bad in (("mean", "median"), ("mean", "mean"), (), ("moment3",)):
        with pytest.raises(ValueError):
            blk.multi_aggregate(h, bad)
        with pytest.raises(ValueError):
            blk.multi_aggregate_torch(h, bad)
    with pytest.raises(ValueError, match="moment"):
        PNAConv(8, 8, ["mean", "moment3"], ["identity"], 1.0)
    with pytest.raises(ValueError, match="edge"):
        PNAConv(8, 8, ["mean"], ["identity"], 1.0, edge_feat_size=4)
    with pytest.raises(ValueError):
        PNAConv(8, 8, ["mean"], ["squash"], 1.0)


def test_c_symbols(hiplib):
    from COALA_GNN_Pybind import _capi
    for name in ("coala_block_multi_aggregate", "coala_block_multi_aggregate_csr", "coala_block_multi_aggregate_backward",
                 "coala_block_multi_aggregate_backward_csr"):
        assert name in _capi.SYMBOLS and getattr(_capi.load(), name) is not None


def test_pnaconv_state_dict_names(hiplib):
    from COALA_GNN.nn import PNAConv
    names = set(PNAConv(8, 8, ["mean", "std"], ["identity", "attenuation"], 1.5, num_towers=2).state_dict())
    want = {f"towers.{t}.{m}.{p}" for t in (0, 1) for m in ("M", "U", "batchnorm") for p in ("weight", "bias")}
    want |= {f"towers.{t}.batchnorm.{b}" for t in (0, 1) for b in ("running_mean", "running_var", "num_batches_tracked")}
    assert names == want | {"mixing_layer.0.weight", "mixing_layer.0.bias"}


@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_pnaconv_equals_the_per_edge_layer(hiplib, form):
    from COALA_GNN.nn import PNAConv, pna_delta
    torch.manual_seed(1)
    layer = PNAConv(6, 6, ALL, ["identity", "amplification", "attenuation"], 0.9, num_towers=2).double()
    blk = hand_block(form)
    h = torch.randn(8, 6, dtype=torch.float64)
    got, want = layer(blk, (h, h[:5])).detach(), pna_reference(layer, blk, h, h[:5]).detach()
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    indptr = torch.tensor([0, 1, 3, 7])
    assert math.isclose(pna_delta(type("G", (), {"indptr": indptr})), float(np.log([2.0, 3.0, 5.0]).mean()), rel_tol=1e-12)
