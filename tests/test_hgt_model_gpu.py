"""harness.HGT (2 layers, T = 3, R = 4) and harness.DotGAT (2 layers) on really sampled blocks, fp32 on the native kernels, against the
float64 global-id reference of tests/_hgt_global_ref.py, which never sees a local index (tests/test_dot_gat_cpu.py proves it against
the models in float64 and against the naive per-edge layer, and shows that it catches a softmax per relation).

The graph is the small one of tests/_model_cases.graph().  Samplers: NeighborSampler(edge_ids=True) at [5, 5] and [5, -1], one
owner-bucketed input layer (bucket_by_owner=3), and RelNeighborSampler on the graph sorted by edge type; seeds in batches of 64, 128
and 256 that hold the hub (300 in-edges: five chunks of the online softmax), the node without in-edges, the self-loop and the
repeated edge.  The blocks are decoded into (dst, src, eid) triples in global ids; logits, every parameter gradient and grad_X
(feat.grad scattered by input_nodes) are compared.  Every layer must have gone through the native autograd Function (the fallback counts
as failure).

Tolerance, the rule of tests/test_models_global_gpu.py: for each array E32 = the largest difference between the reference's own
float32 and float64 evaluations; the kernel path is within FACTOR * E32, and never asked to be closer than 8 * 2^-24 times the array's
largest magnitude.  FACTOR = 4, that file's.  error / E32 is printed per case and array.  T, R >= 2: no parameter is a one-element array.

Measured on the MI355X, error / E32, the largest over a model's cases and arrays whose error is above the floor: dotgat 1.07 (ns5F;
0.93 on ns55, the floor is the bound on the bucketed and the relation-sampled case); hgt 2.70 on ns55, 3.33 on ns55-b3
(layers.0.residual_w), and, layers.1.skip aside, 3.58 on ns5F (layers.1.rel_pri) and 2.31 on rel.  FACTOR stays 4 for all of them.

One array needs more: layers.1.skip, the gradient of the last layer's skip gates, [T] = 3 elements -- 4.13 on ns5F (error 1.3e-06, E32
3.2e-07) and 4.59 on rel (1.9e-06, 4.0e-07); 2.3 and below on the other two cases and for layers.0.skip everywhere.  Its factor is 8,
the next power of two.  The op is no project kernel: element t is autograd's fp32 reduction of sigmoid'(skip[t]) * (y - residual) *
grad_out over every destination of type t and every column, products of both signs.  As with the one-element arrays of
tests/test_models_global_gpu.py, E32 of a three-element array is the largest of three draws of the rounding error of a cancelling sum,
not the stable scale that a maximum over hundreds of elements is, and the floor (8 * 2^-24 of the magnitude after the cancellation)
does not help it; the kernel path's error is of the same size as in the cases that pass."""
import numpy as np
import pytest

import _global_ref as GR
import _hgt_global_ref as HG
import _hgt_model_cases as HC
import _model_cases as MC

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FACTORS = {"layers.1.skip": 8.0}   # measured 4.59 at the most (see above): the next power of two

# (id, sampler, fan-outs in model order, bucket_by_owner, seeds in the batch)
CASES = [("ns55", "ns", [5, 5], 0, 64), ("ns5F", "ns", [5, -1], 0, 128), ("ns55-b3", "ns", [5, 5], 3, 256),
         ("rel", "rel", [[2, 3, 1], [-1, 2, 0]], 0, 128)]


class _Spy(object):
    def __init__(self, fn, name, log):
        self.fn, self.name, self.log = fn, name, log

    def apply(self, *args):
        self.log.append(self.name)
        return self.fn.apply(*args)


@pytest.fixture
def paths(monkeypatch):
    from COALA_GNN import sampler as S
    native, fallback = [], []
    for name in ("_DotGatAggregate", "_DotGatAggregateCSR"):
        monkeypatch.setattr(S, name, _Spy(getattr(S, name), name, native))
    real = S.Block.dot_gat_aggregate_torch
    monkeypatch.setattr(S.Block, "dot_gat_aggregate_torch", lambda self, *a, **k: (fallback.append("dot_gat"), real(self, *a, **k))[1])
    return native, fallback


def _seeds(n):
    rng = np.random.default_rng(n)
    special = [MC.HUB, MC.ZERO, MC.LOOP, MC.MULTI]
    others = [v for v in rng.permutation(MC.N) if v not in special][: n - len(special)]
    return np.array(special + others, dtype=np.int64)


@pytest.mark.parametrize("kind", ["hgt", "dotgat"])
@pytest.mark.parametrize("cid,cls,fanouts,G,n_seeds", CASES, ids=[c[0] for c in CASES])
def test_hgt_and_dotgat_on_sampled_blocks_against_global_reference(hiplib, paths, kind, cid, cls, fanouts, G, n_seeds):
    import torch
    from COALA_GNN.sampler import NeighborSampler, RelNeighborSampler, sort_csc_by_etype
    native, fallback = paths
    g = MC.graph()
    indptr, indices, etype = (torch.from_numpy(a).cuda() for a in (g.indptr, g.indices, g.etype))
    if cls == "rel":
        indices, etype, _ = sort_csc_by_etype(indptr, indices, etype)
        sampler = RelNeighborSampler(fanouts, MC.NRELS, seed=MC.SAMPLER_SEED, bucket_by_owner=G)
    else:
        sampler = NeighborSampler(fanouts, seed=MC.SAMPLER_SEED, bucket_by_owner=G, edge_ids=True)
    dg = sampler.make_graph(indptr, indices, edata={"etype": etype})
    seeds = _seeds(n_seeds)
    try:
        input_nodes, _, blocks = sampler.sample(dg, torch.from_numpy(seeds).cuda(), step=0)
        assert torch.equal(input_nodes, blocks[0].src_nodes)
        if G:
            assert blocks[0].dst_in_src is not None
        layers = [GR.decode(b) for b in blocks]
        idx = indices.cpu().numpy()
        for lay in layers:                                         # the integer part: every triple is an in-edge of the graph
            d, s, e = lay.tri[:, 0], lay.tri[:, 1], lay.tri[:, 2]
            assert np.all((e >= g.indptr[d]) & (e < g.indptr[d + 1])) and np.all(idx[e] == s)
        assert np.array_equal(layers[-1].dst, seeds)
        Cmat = np.random.default_rng(7000 + n_seeds).standard_normal((n_seeds, MC.NCLS)).astype(np.float32)
        model = HC.make_model(kind)
        args = (kind, MC.params_of(model), layers, g.X, Cmat, seeds)
        kw = dict(heads=HC.HEADS, ntype=HC.ntype(), etype=etype.cpu().numpy())
        ref64 = HG.run(*args, torch.float64, **kw)
        ref32 = HG.run(*args, torch.float32, **kw)
        got = HC.run(model.cuda(), blocks, torch.from_numpy(g.X).cuda(), torch.from_numpy(Cmat).cuda())
        assert native == ["_DotGatAggregate" + ("CSR" if b.nbr is None else "") for b in blocks], f"native Functions that ran: {native}"
        assert not fallback, f"torch fallbacks that ran: {fallback}"
        worst = HG.compare(got, ref64, ref32, FACTOR, f"{cid}-{kind}", factors=FACTORS if kind == "hgt" else None)
        print(f"{cid}-{kind}: largest error / E32 above the floor {worst:.2f}")
    finally:
        dg.close()
