"""GPU tests of the multi-statistic aggregation (coala_block_multi_aggregate[_csr] and its backward in coala_block_ops.hip,
Block.multi_aggregate, PNAConv, harness.PNA).

Values and gradients against Block.multi_aggregate_torch in float64 on the CPU by the rule of _dispatch_parity.py: within 4 E, E the
error of the torch path in fp32 on the CPU, with a floor of 8 * 2^-24 times the reference's largest magnitude -- per plane, and for
grad_src under a random grad_out.  What the kernel promises bit for bit is compared bit for bit."""
import copy
import math

import numpy as np
import pytest

from _pna_ref import pna_reference

pytestmark = pytest.mark.gpu

ALL = ("sum", "mean", "max", "min", "var", "std")
SETS = [ALL, ("std",), ("max", "min"), ("mean",), ("std", "sum", "min", "mean")]
N_SRC = 50


def within(got, want, low, what):
    e = float((low.detach().double() - want.detach()).abs().max())
    tol = max(4.0 * e, 8.0 * 2.0 ** -24 * float(want.detach().abs().max()))
    err = float((got.detach().double().cpu() - want.detach()).abs().max())
    print(f"{what}: error {err:.3e} E {e:.3e} bound {tol:.3e}")
    assert err <= tol, f"{what}: error {err:.3e} above {tol:.3e}"


def make_blocks(rng, form, f=7, n_dst=9, lengths=(0, 1, 63, 64, 65, 130)):
    """-> (the block on the GPU, its twin on the CPU).  fixed: fan-out f, row 0 all -1, a -1 in the middle of row 1, a full row 2;
    ragged: rows of `lengths`."""
    import torch
    from COALA_GNN.sampler import Block
    src = torch.arange(N_SRC)
    if form == "fixed":
        nbr = rng.integers(0, N_SRC, size=(n_dst, f)).astype(np.int32)
        nbr[rng.random((n_dst, f)) < 0.2] = -1
        nbr[0], nbr[1, f // 2], nbr[2] = -1, -1, rng.integers(0, N_SRC, size=f)
        t = torch.from_numpy(nbr)
        return Block(src.cuda(), t.cuda(), n_dst), Block(src, t, n_dst)
    indptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))
    idx = torch.from_numpy(rng.integers(0, N_SRC, size=int(indptr[-1])).astype(np.int32))
    return Block(src.cuda(), None, len(lengths), indptr=indptr.cuda(), indices=idx.cuda()), Block(src, None, len(lengths), indptr=indptr, indices=idx)


def check(rng, gpu, cpu, h, aggs, eps=1e-5):
    """Every plane and grad_src of the native path against the float64 reference; -> the native output."""
    import torch
    go = rng.standard_normal((cpu.num_dst, len(aggs), h.shape[1])).astype(np.float32)
    res = []
    for blk, dev, dt, fn in ((gpu, "cuda", torch.float32, "multi_aggregate"), (cpu, "cpu", torch.float64, "multi_aggregate_torch"),
                             (cpu, "cpu", torch.float32, "multi_aggregate_torch")):
        x = torch.from_numpy(h).to(device=dev, dtype=dt).requires_grad_(True)
        out = getattr(blk, fn)(x, aggs, eps)
        (out * torch.from_numpy(go).to(device=dev, dtype=dt)).sum().backward()
        res.append((out, x.grad))
    (got, g_got), (want, g_want), (low, g_low) = res
    assert type(got.grad_fn).__name__ == ("_MultiAggregateCSRBackward" if gpu.nbr is None else "_MultiAggregateBackward")
    assert got.shape == want.shape
    for a, name in enumerate(aggs):
        within(got[:, a], want[:, a], low[:, a], f"{'/'.join(aggs)} plane {name}")
    within(g_got, g_want, g_low, f"{'/'.join(aggs)} grad_src")
    return got.detach()


@pytest.mark.parametrize("dim", [1, 7, 4, 260])   # the scalar path, misaligned rows, one float4 unit, a second pass of 64 lanes
@pytest.mark.parametrize("form,f", [("fixed", 1), ("fixed", 7), ("fixed", 32), ("ragged", 0)])
def test_values_and_gradients(hiplib, form, f, dim):
    rng = np.random.default_rng(1000 * f + dim)
    gpu, cpu = make_blocks(rng, form, f)
    h = rng.standard_normal((N_SRC, dim)).astype(np.float32)
    for aggs in SETS:
        check(rng, gpu, cpu, h, aggs)


@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_variance_far_from_zero_and_repeated_sources(hiplib, form):
    """A table of mean 1000 and spread 1: E[x^2] - E[x]^2 in fp32 is off by about 1000^2 * 2^-24 = 0.06 and cannot meet the bound,
    the shifted moments do.  Then rows that repeat one source among equal values: max and min send their gradient to one slot."""
    rng = np.random.default_rng(5)
    gpu, cpu = make_blocks(rng, form)
    h = (1000.0 + rng.standard_normal((N_SRC, 7))).astype(np.float32)
    check(rng, gpu, cpu, h, ALL)
    h[:] = h[0]
    check(rng, gpu, cpu, h, ("max", "min", "mean"))


@pytest.mark.parametrize("dim", [4, 7])
def test_exact_planes(hiplib, dim):
    """mean, max and min have the bits of the single-statistic ops; a row both forms express gives the same bits in both; rows of one
    neighbour and of equal values give var == 0 and std == sqrt(eps) exactly, with a finite gradient; NaN and inf follow the max rule."""
    import torch
    from COALA_GNN.sampler import Block
    rng = np.random.default_rng(dim)
    eps = torch.tensor(1e-5, dtype=torch.float32)
    nbr = np.sort(rng.integers(-1, N_SRC - 4, size=(40, 9)).astype(np.int32), 1)[:, ::-1].copy()      # the -1 trail: CSR can say it
    nbr[0], nbr[1, 0], nbr[1, 1:], nbr[2] = -1, 3, -1, N_SRC - 1                                                    # no, one, nine equal neighbours
    h = rng.standard_normal((N_SRC, dim)).astype(np.float32)
    h[N_SRC - 4:N_SRC - 1] = [[np.nan], [np.inf], [-np.inf]]
    nbr[3, :4], nbr[4, :3], nbr[5, :2] = [5, N_SRC - 4, 6, N_SRC - 4], [N_SRC - 3, 7, N_SRC - 2], N_SRC - 2
    src, t = torch.arange(N_SRC).cuda(), torch.from_numpy(nbr).cuda()
    indptr = torch.from_numpy(np.concatenate([[0], np.cumsum((nbr >= 0).sum(1))]).astype(np.int64)).cuda()
    fixed, ragged = Block(src, t, 40), Block(src, None, 40, indptr=indptr, indices=t[t >= 0].contiguous())
    x = torch.from_numpy(h).cuda().requires_grad_(True)
    out = fixed.multi_aggregate(x, ALL, float(eps))
    bits = lambda v: v.detach().contiguous().view(torch.int32)
    assert torch.equal(bits(out), bits(ragged.multi_aggregate(x, ALL, float(eps)))), "the two block forms differ"
    assert torch.equal(bits(out[:, 1]), bits(fixed.mean_aggregate(x)))
    assert torch.equal(bits(out[:, 2]), bits(fixed.max_aggregate(x)))
    no_nan = (torch.arange(40).cuda() != 3) & (torch.arange(40).cuda() != 0)                          # -NaN, and -0 of the row without an edge
    assert torch.equal(bits(out[no_nan, 3]), bits(-fixed.max_aggregate(-x)[no_nan]))
    assert torch.isnan(out[3, 2:4]).all() and (out[4, 2] == math.inf).all() and (out[4, 3] == -math.inf).all()
    assert torch.equal(out[0], torch.zeros_like(out[0])), "a row without an edge is not all zeros"
    assert (out[1:3, 4] == 0).all() and (out[1:3, 5] == eps.sqrt().item()).all()
    clean = torch.from_numpy(np.nan_to_num(h, nan=1.0, posinf=2.0, neginf=-2.0)).cuda().requires_grad_(True)
    (g,) = torch.autograd.grad(fixed.multi_aggregate(clean, ALL, float(eps)).sum(), clean)
    assert torch.isfinite(g).all(), "a gradient through var == 0 is not finite"


def test_past_one_grid_pass(hiplib):
    """40,000 rows: the grid is capped at 8192 blocks of 4 waves, so 7,232 waves take a second row."""
    rng = np.random.default_rng(9)
    gpu, cpu = make_blocks(rng, "fixed", f=3, n_dst=40000)
    check(rng, gpu, cpu, rng.standard_normal((N_SRC, 4)).astype(np.float32), ("mean", "max", "min", "std"))


@pytest.mark.parametrize("fan", [[5, 5], [5, -1]])
def test_pnaconv_on_sampled_blocks(hiplib, fan):
    """PNAConv (two towers, every aggregator and scaler) on both layers of a sampled minibatch against the float64 per-edge
    restatement of _pna_ref.py: the output and every parameter's gradient, and the native path by its autograd class."""
    import torch
    from COALA_GNN.nn import PNAConv, pna_delta
    from COALA_GNN.sampler import Block, NeighborSampler
    from COALA_GNN.synthetic import powerlaw_csc
    indptr, indices = powerlaw_csc(3000, 6.0, seed=2, device="cuda")
    smp = NeighborSampler(fan, seed=3)
    g = smp.make_graph(indptr, indices)
    blocks = smp.sample(g, torch.arange(100, 124).cuda())[2]
    torch.manual_seed(0)
    for blk in blocks:
        layer = PNAConv(8, 8, ALL, ["identity", "amplification", "attenuation"], pna_delta(g), num_towers=2)
        host = Block(blk.src_nodes.cpu(), None if blk.nbr is None else blk.nbr.cpu(), blk.num_dst,
                     indptr=None if blk.nbr is not None else blk.indptr.cpu(), indices=None if blk.nbr is not None else blk.indices.cpu())
        h = torch.randn(blk.num_src, 8)
        res = []
        for mod, b, x, fn in ((copy.deepcopy(layer).cuda(), blk, h.cuda(), None), (copy.deepcopy(layer).double(), host, h.double(), pna_reference),
                              (layer, host, h, None)):
            out = mod(b, (x, x[:b.num_dst])) if fn is None else fn(mod, b, x, x[:b.num_dst])
            mod.zero_grad()
            out.square().sum().backward()
            res.append((out, mod))
        (got, m_got), (want, m_want), (low, m_low) = res
        native = type(blk.multi_aggregate(h.cuda().requires_grad_(True), ALL).grad_fn).__name__
        assert native == ("_MultiAggregateCSRBackward" if blk.nbr is None else "_MultiAggregateBackward")
        within(got, want, low, "PNAConv output")
        for (name, p), q, r in zip(m_got.named_parameters(), m_want.parameters(), m_low.parameters()):
            within(p.grad, q.grad, r.grad, f"PNAConv grad {name}")


def test_pna_model_trains(hiplib):
    import torch
    from COALA_GNN.harness import PNA
    from COALA_GNN.nn import pna_delta
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import feature_rows_torch, powerlaw_csc
    indptr, indices = powerlaw_csc(5000, 8.0, seed=1, device="cuda")
    smp = NeighborSampler([5, 5], seed=5)
    g = smp.make_graph(indptr, indices)
    torch.manual_seed(0)
    model = PNA(32, 16, 4, 2, delta=pna_delta(g), num_towers=2).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses = []
    for step in range(20):
        input_nodes, seeds, blocks = smp.sample(g, torch.arange(64 * step, 64 * step + 64).cuda())
        feat = feature_rows_torch(input_nodes, 32, 3)
        loss = torch.nn.functional.cross_entropy(model(blocks, feat), feat[:64, :4].argmax(1))
        opt.zero_grad(); loss.backward(); opt.step()
        losses.append(loss.item())
    print("losses:", " ".join(f"{x:.4f}" for x in losses))
    assert len(losses) == 20 and all(math.isfinite(x) for x in losses)
