"""GPU tests of the PinSAGE model layer on blocks sampled by random walks: COALA_GNN.nn.WeightedSAGEConv against its formula written in
plain torch, and harness.PinSAGE in a short training run.

Tolerance of the layer test, the rule of test_models_global_gpu.py for fp32 models: for each array (the output, the gradient of every
parameter and of the source rows) E32 = the largest difference between the formula's own float32 and float64 evaluations on the CPU;
the layer on the native kernel is within FACTOR * E32 of the float64 evaluation, and never asked to be closer than 8 * 2^-24 times the
array's largest magnitude.  The float64 evaluation must stay clear of the formula's discontinuities (relu at 0, a zero norm): the
smallest pre-activation magnitude is asserted to be above TAU, far above fp32 rounding at these magnitudes."""
import numpy as np
import pytest

import _model_cases as MC

pytestmark = pytest.mark.gpu

FACTOR = 4.0
TAU = 1e-5
IN, HID, OUT = MC.IN, 16, 12


def _formula(p, nbr, w, h_src, n_dst):
    """WeightedSAGEConv in plain torch, in the dtype of its inputs: -> (out, the pre-activations)."""
    import torch
    valid = (nbr >= 0).to(h_src.dtype)
    idx = nbr.clamp_min(0).to(torch.int64)
    pre_q = h_src @ p["Q.weight"].t() + p["Q.bias"]
    ww = w * valid
    n = (torch.relu(pre_q)[idx] * ww.unsqueeze(-1)).sum(1) / ww.sum(1).clamp_min(1).unsqueeze(1)
    pre_z = torch.cat([n, h_src[:n_dst]], 1) @ p["W.weight"].t() + p["W.bias"]
    z = torch.relu(pre_z)
    norm = z.norm(2, 1, keepdim=True)
    return z / torch.where(norm == 0, torch.ones_like(norm), norm), (pre_q, pre_z, norm)


def _evaluate(params, nbr, w, x, cmat, dtype):
    import torch
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    h = x.to(dtype).clone().requires_grad_(True)
    out, pre = _formula(p, nbr, w.to(dtype), h, nbr.shape[0])
    (out * cmat.to(dtype)).sum().backward()
    res = {"out": out, "grad_h": h.grad}
    res.update({"grad_" + k: v.grad for k, v in p.items()})
    return {k: v.detach().double().numpy() for k, v in res.items()}, pre


@pytest.fixture(scope="module")
def walk_blocks(hiplib):
    import torch
    from COALA_GNN.sampler import RandomWalkNeighborSampler
    g = MC.graph()
    smp = RandomWalkNeighborSampler([5, 5], 2, 0.5, 10, seed=MC.SAMPLER_SEED)
    dg = smp.make_graph(torch.from_numpy(g.indptr).cuda(), torch.from_numpy(g.indices).cuda(), ndata={"labels": torch.from_numpy(g.labels).cuda()})
    _, _, blocks = smp.sample(dg, torch.from_numpy(g.seeds).cuda(), step=0)
    yield g, blocks
    dg.close()


@pytest.mark.parametrize("layer", [0, 1])
def test_weighted_sage_conv_against_the_formula(walk_blocks, layer):
    import torch
    from COALA_GNN.nn import WeightedSAGEConv
    g, blocks = walk_blocks
    b = blocks[layer]
    assert b.nbr is not None and b.nbr.shape[1] == 5
    torch.manual_seed(40 + layer)
    conv = WeightedSAGEConv(IN, HID, OUT)
    with torch.no_grad():
        for prm in conv.parameters():
            if prm.dim() == 1:
                prm.normal_(0.0, 0.3)          # the biases are zero at initialisation: make them visible
    params = dict(conv.named_parameters())
    nbr, w = b.nbr.cpu(), b.edata["weights"].cpu()
    assert (nbr < 0).any() and (w.sum(1) == 0).any() and (w.sum(1) > 1).any(), "the block must hold padding, an empty row and real counts"
    x = torch.from_numpy(g.X)[b.src_nodes.cpu()]
    cmat = torch.from_numpy(np.random.default_rng(7 + layer).standard_normal((b.num_dst, OUT)).astype(np.float32))
    ref, pre = _evaluate(params, nbr, w, x, cmat, torch.float64)
    f32, _ = _evaluate(params, nbr, w, x, cmat, torch.float32)
    pre_q, pre_z, norm = pre
    gap = min(float(pre_q.detach().abs().min()), float(pre_z.detach().abs().min()))
    print(f"layer {layer}: kink gap {gap:.3e}, rows of zero norm {int((norm == 0).sum())}")
    assert gap >= TAU, "the inputs sit on a gradient discontinuity: choose another seed"
    conv = conv.cuda()
    h = x.cuda().requires_grad_(True)
    out = conv(b, (h, b.dst_rows(h)), b.edata["weights"])
    (out * cmat.cuda()).sum().backward()
    got = {"out": out, "grad_h": h.grad}
    got.update({"grad_" + k: v.grad for k, v in conv.named_parameters()})
    assert set(got) == set(ref)
    for k in sorted(ref):
        e32 = float(np.abs(f32[k] - ref[k]).max())
        err = float(np.abs(got[k].detach().double().cpu().numpy() - ref[k]).max())
        bound = max(FACTOR * e32, 8 * 2.0**-24 * float(np.abs(ref[k]).max()))
        print(f"layer {layer} {k}: error {err:.3e} E32 {e32:.3e} ratio {err / max(e32, 1e-300):.2f} bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
    norms = out.detach().norm(2, 1)
    assert torch.all((norms - 1).abs() < 1e-5) or torch.all(((norms - 1).abs() < 1e-5) | (norms == 0))


def test_pinsage_trains(walk_blocks):
    """Three optimiser steps of harness.PinSAGE on one sampled batch of the synthetic graph lower its loss."""
    import torch
    from COALA_GNN.harness import PinSAGE
    g, blocks = walk_blocks
    torch.manual_seed(0)
    model = PinSAGE(IN, HID, MC.NCLS, len(blocks)).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    feat = torch.from_numpy(g.X).cuda()[blocks[0].src_nodes]
    labels = blocks[-1].dstdata["labels"].view(-1)
    losses = []
    for _ in range(4):
        loss = torch.nn.functional.cross_entropy(model(blocks, feat), labels)
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[3] < losses[0]
    with pytest.raises(ValueError, match="RandomWalkNeighborSampler"):
        from COALA_GNN.sampler import Block
        model([Block(b.src_nodes, b.nbr, b.num_dst) for b in blocks], feat)
