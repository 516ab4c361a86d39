"""GPU test of harness.RGAT and harness.RSAGE on sampled blocks: the models on the native kernels (fp32, GPU) against the same modules
run on CPU float64 copies of the blocks, where every block op takes its torch path.

Setup: powerlaw_csc with 3000 nodes and 4 relations (the source's id modulo 4), every node's in-edges sorted by type; one 64-seed batch
from NeighborSampler([5, 5], edge_ids=True), from RelNeighborSampler([[3, 2, 0, -1], [2, 2, 2, 2]], 4) -- ragged blocks, the input
layer's fourth relation keeping every edge -- and from the owner-bucketed form of the first (bucket_by_owner=3).  Compared: the logits, every
parameter's gradient and the gradient of the input features, for the loss (logits * C).sum() with a fixed random C.

Tolerance, measured rather than guessed: E = the largest difference, per compared tensor, between the fp32 torch path and the float64
torch path on the same blocks -- what fp32 arithmetic alone costs this model, whatever the kernel.  The native path must stay within
MULT * max(E, 8 u max|reference|), u = 2^-24 (the floor keeps a tensor that both torch paths happen to get exactly from asking for
zero error).  MULT = 4, the multiple the dispatch-parity tests of the other block ops use: the native kernels sum in another order
than torch's index_add (a tree per chunk, atomics in the backward), which moves an fp32 result by a small multiple of its own
rounding error, not more.  MULT was fixed before the first run.  Measured on the MI355X, the largest native error / max(E, floor) over
the compared tensors (the test prints every figure): RGAT ns55 2.51 (layers.0.attn_r: error 2.3e-06, E 9.2e-07), ns55-b3 2.51; RSAGE
ns55 1.46 (layers.0.fc_neigh_weight: error 1.1e-05, E 4.0e-06, floor 7.3e-06), ns55-b3 1.46; on the RelNeighborSampler batch RGAT 1.15
and RSAGE 0.94."""
import functools
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, RELS, IN, HID, NCLS, HEADS, NSEEDS, MULT = 3000, 4, 20, 16, 5, 4, 64, 4.0
SAMPLERS = ("ns55", "rel", "ns55-b3")


@functools.lru_cache(None)
def _graph():
    import torch
    from COALA_GNN.sampler import sort_csc_by_etype
    from COALA_GNN.synthetic import edge_types_by_source, powerlaw_csc
    indptr, indices = powerlaw_csc(N, 8.0, seed=4, device="cuda")
    indices, etype, _ = sort_csc_by_etype(indptr, indices, edge_types_by_source(indices, RELS))
    g = torch.Generator().manual_seed(0)
    X = torch.randn(N, IN, generator=g)
    labels = torch.randint(0, NCLS, (N,), generator=g)
    seeds = torch.randperm(N, generator=g)[:NSEEDS]
    C = torch.randn(NSEEDS, NCLS, generator=g)
    return indptr, indices, etype, X, labels, seeds, C


@functools.lru_cache(None)
def _blocks(name):
    """-> (the sampled blocks on the GPU, their CPU copies with the graph's edge types behind their edge ids)"""
    from COALA_GNN.sampler import Block, NeighborSampler, RelNeighborSampler
    indptr, indices, etype, _, labels, seeds, _ = _graph()
    if name == "rel":
        sampler = RelNeighborSampler([[3, 2, 0, -1], [2, 2, 2, 2]], RELS, seed=3)
    else:
        sampler = NeighborSampler([5, 5], seed=3, edge_ids=True, bucket_by_owner=3 if name.endswith("b3") else 0)
    g = sampler.make_graph(indptr, indices, ndata={"labels": labels.cuda()}, edata={"etype": etype})
    _, _, blocks = sampler.sample(g, seeds.cuda())
    host = types.SimpleNamespace(edata={"etype": etype.cpu()}, ndata={})
    cpu = lambda t: None if t is None else t.cpu()   # noqa: E731
    copies = [Block(b.src_nodes.cpu(), cpu(b.nbr), b.num_dst, dst_in_src=cpu(b.dst_in_src), dst_nodes=b.dstdata["_ID"].cpu(),
                    indptr=cpu(b.indptr), indices=cpu(b.indices), eid=b.edata["_ID"].cpu(), edata_graph=host) for b in blocks]
    return blocks, copies


def _model(kind, dtype, device):
    import torch
    from COALA_GNN import harness
    torch.manual_seed(7)
    if kind == "RGAT":
        m = harness.RGAT(IN, HID, NCLS, 2, RELS, n_heads=HEADS, dropout=0.0)
    else:
        m = harness.RSAGE(IN, HID, NCLS, 2, RELS, dropout=0.0)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("bias"):
                p.normal_(0.0, 0.3)      # zero at initialisation: drawn so that none of them is invisible
    return m.to(device=device, dtype=dtype)


def _run(kind, blocks, dtype, device):
    """forward, (logits * C).sum().backward() -> {name: float64 array}: 'logits', 'grad_X' ([N, in], scattered by input node) and every
    parameter's gradient"""
    import torch
    _, _, _, X, _, _, C = _graph()
    model = _model(kind, dtype, device)
    input_nodes = blocks[0].src_nodes.to(device)
    feat = X.to(device=device, dtype=dtype)[input_nodes].clone().requires_grad_(True)
    logits = model(blocks, feat)
    (logits * C.to(device=device, dtype=dtype)).sum().backward()
    out = {"logits": logits, "grad_X": torch.zeros((N, IN), dtype=dtype, device=device).index_add(0, input_nodes, feat.grad)}
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        out[k] = p.grad
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", SAMPLERS)
@pytest.mark.parametrize("kind", ["RGAT", "RSAGE"])
def test_native_model_within_the_fp32_spread(hiplib, kind, name):
    import torch
    from COALA_GNN.block_ops import _RelGatAggregate, _RelGatAggregateCSR, _RelSum, _RelSumCSR
    blocks, copies = _blocks(name)
    assert blocks[0].num_dst == blocks[1].num_src and blocks[1].num_dst == NSEEDS
    if name == "rel":
        assert blocks[0].nbr is None, "RelNeighborSampler's layers are ragged"
    if name.endswith("b3"):
        assert blocks[0].dst_in_src is not None
    # the native kernels do run on these blocks: the layer's message step leaves its autograd function
    _, _, _, X, _, _, _ = _graph()
    layer = _model(kind, torch.float32, "cuda").layers[0]
    h = X.cuda()[blocks[0].src_nodes].requires_grad_(True)
    names, seen = set(), set()
    todo = [layer(blocks[0], (h, blocks[0].dst_rows(h)), blocks[0].edata["etype"]).grad_fn]
    while todo:
        fn = todo.pop()
        if fn is not None and fn not in seen:
            seen.add(fn)
            names.add(type(fn).__name__)
            todo += [nf for nf, _ in fn.next_functions]
    want = (_RelGatAggregate, _RelGatAggregateCSR) if kind == "RGAT" else (_RelSum, _RelSumCSR)
    assert want[blocks[0].nbr is None].__name__ + "Backward" in names, sorted(names)

    native = _run(kind, blocks, torch.float32, "cuda")
    low = _run(kind, copies, torch.float32, "cpu")
    ref = _run(kind, copies, torch.float64, "cpu")
    assert set(native) == set(ref) and len(ref) >= 6
    worst = 0.0
    for k in sorted(ref):
        assert native[k].shape == ref[k].shape and np.isfinite(native[k]).all()
        E = float(np.abs(low[k] - ref[k]).max())
        floor = 8.0 * 2.0 ** -24 * float(np.abs(ref[k]).max())
        err = float(np.abs(native[k] - ref[k]).max())
        print(f"{kind}-{name} {k}: native error {err:.3e} fp32 spread E {E:.3e} floor {floor:.3e} ratio {err / max(E, floor):.2f}")
        worst = max(worst, err / max(E, floor))
        assert float(np.abs(ref[k]).max()) > 0, f"{k} is zero in the reference: nothing is compared"
        assert err <= MULT * max(E, floor), f"{k}: native error {err:.3e} above {MULT} x max(E {E:.3e}, floor {floor:.3e})"
    print(f"{kind}-{name}: largest native error / max(E, floor) {worst:.2f}")
