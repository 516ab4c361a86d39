"""harness.GATv2 on sampled blocks, native path against float64: 2 layers, 2 heads, hidden 8, 5 classes, feature dim 12, on blocks from
NeighborSampler([5, 5]), NeighborSampler([-1, -1]), LaborSampler([5, 5]) and the owner-bucketed NeighborSampler([5, 5], bucket_by_owner=4),
with and without share_weights.  The logits, every parameter gradient and the gradient of the feature table from the GPU (fp32, the
native kernels) are compared with the same model in float64 on CPU copies of the same blocks (the *_torch fallbacks).

Tolerance, the rule of tests/_dispatch_parity.py: E = the largest difference between the reference evaluated in fp32 on the CPU and in
float64; an array is within 4 E, and never asked to be closer than 8 u times the reference's largest magnitude, u = 2^-24.

And three training steps of the model examples/train_synthetic.py builds for --model_type gatv2, on a 2,000-node synthetic graph: finite
loss that does not grow."""
import copy
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N_NODES, N_SEEDS, DIM, HIDDEN, CLASSES, HEADS = 20000, 256, 12, 8, 5, 2
_BLOCKS = {}


def _sampled(torch, name):
    """(input_nodes, blocks on the GPU), sampled once per sampler and left unchanged."""
    if name not in _BLOCKS:
        from COALA_GNN.sampler import LaborSampler, NeighborSampler
        from COALA_GNN.synthetic import powerlaw_csc
        indptr, indices = powerlaw_csc(N_NODES, 8.0, seed=3, device="cuda")
        s = {"neighbor55": lambda: NeighborSampler([5, 5], seed=1), "full": lambda: NeighborSampler([-1, -1], seed=1),
             "labor55": lambda: LaborSampler([5, 5], seed=1), "bucketed55": lambda: NeighborSampler([5, 5], seed=1, bucket_by_owner=4)}[name]()
        g = s.make_graph(indptr, indices)
        seeds = torch.randperm(N_NODES, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))[:N_SEEDS]
        input_nodes, _, blocks = s.sample(g, seeds)
        _BLOCKS[name] = (input_nodes, blocks)
    return _BLOCKS[name]


def _cpu_block(b):
    cpu = lambda t: None if t is None else t.cpu()   # noqa: E731
    return type(b)(b.src_nodes.cpu(), cpu(b.nbr), b.num_dst, dst_in_src=cpu(b.dst_in_src), indptr=cpu(b.indptr), indices=cpu(b.indices))


def _evaluate(torch, model, blocks, table, input_nodes, weight):
    """-> dict of the logits, every parameter gradient and the table gradient, as float64 numpy arrays"""
    table = table.clone().requires_grad_(True)
    model.zero_grad()
    logits = model(blocks, table[input_nodes])
    (logits * weight).sum().backward()
    res = {"logits": logits, "table.grad": table.grad}
    res.update({n + ".grad": p.grad for n, p in model.named_parameters()})
    return {k: v.detach().double().cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("sampler", ["neighbor55", "full", "labor55", "bucketed55"])
def test_gatv2_model_native_against_float64(hiplib, sampler, share):
    import torch
    from COALA_GNN import block_ops
    from COALA_GNN.harness import GATv2
    input_nodes, blocks = _sampled(torch, sampler)
    if sampler == "bucketed55":
        assert blocks[0].dst_in_src is not None
    torch.manual_seed(11 + share)
    ref64 = GATv2(DIM, HIDDEN, CLASSES, 2, HEADS, share_weights=share).double()
    rng = np.random.default_rng(3)
    table = torch.from_numpy(rng.standard_normal((N_NODES, DIM)).astype(np.float32))
    weight = torch.from_numpy(rng.standard_normal((blocks[-1].num_dst, CLASSES)).astype(np.float32))
    host = [_cpu_block(b) for b in blocks]
    want = _evaluate(torch, ref64, host, table.double(), input_nodes.cpu(), weight.double())
    low = _evaluate(torch, copy.deepcopy(ref64).float(), host, table, input_nodes.cpu(), weight)
    calls = []
    native = copy.deepcopy(ref64).float().cuda()
    orig = {c: getattr(block_ops, c).apply for c in ("_Gatv2Aggregate", "_Gatv2AggregateCSR")}
    try:                                               # the GPU run goes through the native Function, once per layer
        for c, fn in orig.items():
            setattr(getattr(block_ops, c), "apply", staticmethod(lambda *a, _c=c, _f=fn: (calls.append(_c), _f(*a))[1]))
        got = _evaluate(torch, native, blocks, table.cuda(), input_nodes, weight.cuda())
    finally:
        for c in orig:
            delattr(getattr(block_ops, c), "apply")    # back to the inherited classmethod
    assert calls == ["_Gatv2AggregateCSR" if b.nbr is None else "_Gatv2Aggregate" for b in blocks], calls   # LABOR's blocks are ragged too
    assert set(got) == set(want) and len(want) == (2 + (3 if share else 5) * 2)
    for k in sorted(want):
        e = float(np.abs(low[k] - want[k]).max())
        tol = max(4.0 * e, 8.0 * U * float(np.abs(want[k]).max()))
        err = float(np.abs(got[k] - want[k]).max())
        print(f"{sampler} share={share} {k}: error {err:.3e} E {e:.3e} bound {tol:.3e}")
        assert got[k].shape == want[k].shape and err <= tol, f"{k}: error {err:.3e} above {tol:.3e}"


@pytest.mark.parametrize("share", [False, True])
def test_gatv2_three_training_steps(hiplib, share):
    """The model of examples/train_synthetic.py --model_type gatv2 [--share_weights]: three SGD steps on one minibatch of a 2,000-node
    synthetic graph; the loss is finite and does not grow."""
    import torch
    from COALA_GNN.harness import GATv2
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import powerlaw_csc
    n, dim, classes = 2000, 16, 4
    indptr, indices = powerlaw_csc(n, 8.0, seed=5, device="cuda")
    sampler = NeighborSampler([5, 5], seed=2)
    g = sampler.make_graph(indptr, indices)
    gen = torch.Generator(device="cuda").manual_seed(1)
    feat = torch.randn(n, dim, device="cuda", generator=gen)
    labels = torch.randint(0, classes, (n,), device="cuda", generator=gen)
    input_nodes, seeds, blocks = sampler.sample(g, torch.arange(0, 512, device="cuda"), step=0)
    torch.manual_seed(3)
    model = GATv2(dim, 8, classes, 2, 4, share).cuda()
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    loss_fn = torch.nn.CrossEntropyLoss()              # the example's loss, on the model's log-probabilities
    losses = []
    for _ in range(4):
        loss = loss_fn(model(blocks, feat[input_nodes]), labels[seeds])
        losses.append(loss.item())
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(losses)
    assert all(math.isfinite(x) for x in losses)
    assert all(b <= a for a, b in zip(losses, losses[1:])), losses
