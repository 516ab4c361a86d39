"""GPU tests of the edge-feature attention kernels (coala_block_edge_attn_aggregate[_csr][_backward]) through Block.edge_attn_aggregate and
autograd, and of TransformerConv / harness.GraphTransformer on sampled blocks, against Block.edge_attn_aggregate_torch in float64 on the CPU.

The bound, per tensor (tests/_dispatch_parity.py, tests/test_time_attn_gpu.py): E is the largest distance of the fp32 CPU fallback from
the float64 result; every element of the native result lies within 2 E of it, and is never asked to be closer than 8 * 2^-24 * max|reference|.
Gradients are those of (out * g1).sum() + (eagg * g2).sum().  -s prints the distances."""
import numpy as np
import pytest
import torch

from test_edge_attn_cpu import make_block

pytestmark = pytest.mark.gpu

NAMES = ("q", "k", "v", "qe", "efeat")
SAME_BITS = ("out", "eagg", "grad_q", "grad_qe")
RAGGED = [(0, 1, 63, 64, 65, 130)[i % 6] for i in range(37)]
# (row lengths, (H, D, F), eids dtype or None for the slot form, tensors one float off a 16-byte boundary)
CASES = [([1] * 9, (1, 1, 1), None, False), ([7] * 9, (3, 5, 3), torch.int64, False), ([33] * 9, (16, 8, 65), torch.int32, False),
         ([64] * 9, (4, 130, 128), None, False), ([65] * 9, (3, 5, 3), torch.int64, True), ([130] * 9, (16, 8, 65), None, True),
         (RAGGED, (3, 5, 3), torch.int32, False), (RAGGED, (4, 130, 128), torch.int64, True), (RAGGED, (16, 8, 65), None, False),
         ([3] * 8200, (2, 4, 4), torch.int64, False)]   # the grid holds 2048 blocks of four rows: 8200 rows need a second pass
M = 50


def _rows(lens, seed):
    """Row 0 is full, row 1 has no edge, every other slot is -1 with probability 1/4, wherever it stands."""
    rng = np.random.default_rng(seed)
    rows = [np.where(rng.random(n) < 0.25, -1, rng.integers(0, len(lens) + 3, n)) for n in lens]
    full = 0 if lens[0] else int(np.argmax(lens))
    rows[full] = np.abs(rows[full])
    rows[1][:] = -1
    return [r.tolist() for r in rows]


def _inputs(rows, ragged, H, D, F, eid_dtype, seed):
    """-> ({name: float64 CPU tensor}, eids, (g1, g2)) for the block of `rows`; ids repeat inside a row and across rows."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).double()
    n_dst, n_src, fan = len(rows), max(max(max(x, default=0) for x in rows), len(rows) - 1) + 1, max(len(x) for x in rows)
    slots = (sum(len(x) for x in rows),) if ragged else (n_dst, fan)
    eids = torch.randint(0, M, slots, generator=g).to(eid_dtype) if eid_dtype else None
    x = dict(q=r(n_dst, H, D), k=r(n_src, H, D), v=r(n_src, H, D), qe=r(n_dst, H, F), efeat=r(M, F) if eid_dtype else r(*slots, F))
    return x, eids, (r(n_dst, H, D), r(n_dst, H, F))


def _run(fn, x, eids, go, dtype, device, offset=False):
    """fn(q, k, v, qe, efeat, eids) -> (out, eagg) on copies of x, and its backward -> every result, float64 on the CPU."""
    def place(t):
        buf = torch.empty(t.numel() + 1, dtype=dtype, device=device)
        return buf[1:].view(t.shape).copy_(t) if offset else t.to(device=device, dtype=dtype, copy=True)
    a = {n: place(t).requires_grad_() for n, t in x.items()}
    out = fn(*(a[n] for n in NAMES), None if eids is None else eids.to(device))
    torch.autograd.backward(out, [g.to(device=device, dtype=dtype) for g in go])
    res = {"out": out[0], "eagg": out[1], **{"grad_" + n: a[n].grad for n in NAMES}}
    return {n: t.detach().double().cpu() for n, t in res.items()}, type(out[0].grad_fn).__name__


def _hold(ref, low, nat, tag):
    for n, want in ref.items():
        dist = float((low[n] - want).abs().max()) if want.numel() else 0.0
        err = float((nat[n] - want).abs().max()) if want.numel() else 0.0
        bound = max(2.0 * dist, 8 * 2.0 ** -24 * float(want.abs().max()))
        print(f"{tag} {n:10s}: fallback fp32 distance {dist:.3e} | native {err:.3e} | bound {bound:.3e}")
        assert err <= bound, f"{tag} {n}: native {err:.3e} from float64, the bound is {bound:.3e}"


@pytest.mark.parametrize("lens, hdf, eid_dtype, offset", CASES, ids=lambda v: str(v[:2]) + str(len(v)) if isinstance(v, list) else str(v))
def test_native_against_float64(hiplib, lens, hdf, eid_dtype, offset):
    ragged = lens is RAGGED
    rows = _rows(lens, seed=sum(hdf))
    x, eids, go = _inputs(rows, ragged, *hdf, eid_dtype, seed=len(lens))
    cpu, gpu = make_block(rows, ragged), make_block(rows, ragged, "cuda")
    ref, _ = _run(cpu.edge_attn_aggregate_torch, x, eids, go, torch.float64, "cpu")
    low, _ = _run(cpu.edge_attn_aggregate_torch, x, eids, go, torch.float32, "cpu")
    nat, ran = _run(gpu.edge_attn_aggregate, x, eids, go, torch.float32, "cuda", offset)
    assert ran.startswith("_EdgeAttnAggregate"), f"the native kernel did not run: {ran}"
    _hold(ref, low, nat, f"{lens[:2]} {hdf}")
    assert not nat["out"][1].any() and not nat["eagg"][1].any() and not nat["grad_q"][1].any() and not nat["grad_qe"][1].any()   # no edge
    again, _ = _run(gpu.edge_attn_aggregate, x, eids, go, torch.float32, "cuda", offset)
    for n in SAME_BITS + (() if eid_dtype else ("grad_efeat",)):   # a second run gives the same bits
        assert torch.equal(again[n], nat[n]), n
    if ragged:   # the same block in fixed form, fan-out 130 and -1 padded: the same bits
        fixed, fan = make_block(rows, False, "cuda"), max(lens)
        pad = lambda t: torch.stack([torch.cat([p, p.new_zeros((fan - len(p),) + p.shape[1:])]) for p in t.split(lens)])
        xf = dict(x) if eid_dtype else dict(x, efeat=pad(x["efeat"]))
        got, ran = _run(fixed.edge_attn_aggregate, xf, None if eids is None else pad(eids), go, torch.float32, "cuda", offset)
        assert ran == "_EdgeAttnAggregateBackward"
        for n in SAME_BITS:
            assert torch.equal(got[n], nat[n]), n


@pytest.fixture(scope="module")
def sampled(hiplib):
    """A fixed block of fan-out 5 and the ragged block of a full layer, 64 seeds on a small power-law graph, with edge features."""
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import powerlaw_csc
    indptr, indices = powerlaw_csc(2000, 8, seed=1)
    smp = NeighborSampler([5, -1], seed=3, edge_ids=True)
    g = smp.make_graph(indptr, indices)
    seeds = torch.randperm(2000, generator=torch.Generator().manual_seed(4))[:64].cuda()
    _, _, blocks = smp.sample(g, seeds)
    gen = torch.Generator().manual_seed(5)
    return blocks, torch.randn(blocks[0].num_src, 16, generator=gen), torch.randn(indices.numel(), 8, generator=gen)


@pytest.mark.parametrize("layer", [0, 1], ids=["fan-out 5", "full layer"])
def test_transformer_conv_on_a_sampled_block(sampled, layer):
    """Against the layer on the torch twin in float64 with the same parameters: output and every gradient, held as the op is."""
    from COALA_GNN.nn import TransformerConv
    from COALA_GNN.sampler import Block
    b, efeat = sampled[0][layer], sampled[2]
    x = sampled[1][: b.num_src]
    assert (b.nbr is None) == bool(layer)
    torch.manual_seed(6)
    conv = TransformerConv(16, 8, 3, edge_dim=8, beta=True)
    go = torch.randn(b.num_dst, 24, generator=torch.Generator().manual_seed(7))
    res, ran = {}, None
    for run in ("ref", "low", "nat"):
        dev, dtype = ("cuda", torch.float32) if run == "nat" else ("cpu", torch.float64 if run == "ref" else torch.float32)
        c = TransformerConv(16, 8, 3, edge_dim=8, beta=True)
        c.load_state_dict(conv.state_dict())
        c = c.to(device=dev, dtype=dtype)
        mv = lambda t: None if t is None else t.to(dev)
        blk = Block(mv(b.src_nodes), mv(b.nbr), b.num_dst, indptr=mv(b.indptr), indices=mv(b.indices), eid=mv(b.edata["_ID"]))
        if run != "nat":
            blk.edge_attn_aggregate = blk.edge_attn_aggregate_torch
        h, e = (t.to(device=dev, dtype=dtype, copy=True).requires_grad_() for t in (x, efeat))
        y = c(blk, h, e)
        y.backward(go.to(y))
        res[run] = {n: t.detach().double().cpu() for n, t in [("out", y), ("grad_h", h.grad), ("grad_e", e.grad)] + [(n, p.grad) for n, p in c.named_parameters()]}
    _hold(res["ref"], res["low"], res["nat"], "TransformerConv")


def test_graph_transformer_trains(sampled):
    from COALA_GNN.harness import GraphTransformer
    blocks, x, efeat = sampled
    torch.manual_seed(8)
    model = GraphTransformer(16, 8, 5, 2, 2, edge_dim=8).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    labels, x, efeat = (blocks[-1].dstdata["_ID"] % 5).cuda(), x.cuda(), efeat.cuda()
    losses = []
    for _ in range(20):
        loss = torch.nn.functional.nll_loss(model(blocks, x, efeat), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert np.isfinite(losses).all() and losses[-1] < losses[0] and model.layers[0].lin_edge.weight.grad.abs().max() > 0, losses
