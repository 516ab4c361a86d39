"""GPU tests of the temporal attention kernels (coala_block_time_attn_aggregate[_backward]) through Block.time_attn_aggregate and
autograd, and of TGATConv / harness.TGAT on sampled temporal blocks, against the float64 per-edge restatement (tests/_time_attn_ref.py).

Tolerance, the convention of tests/test_skipgram_loss_gpu.py: for every output and gradient the distance of the fp32 fallback
Block.time_attn_aggregate_torch from the float64 reference is measured on the same inputs (its largest element), and every element of
the native result must lie within twice that distance -- the fallback does the same arithmetic in another order -- plus 4 fp32 ulps of
the element's reference magnitude (what is left where the fallback is exact: a row of one edge).  -s prints the distances."""
import types

import numpy as np
import pytest
import torch

import _time_attn_ref as R

pytestmark = pytest.mark.gpu

NAMES = ("q", "k", "v", "qt", "omega", "phase")
EPS = float(np.finfo(np.float32).eps)
CASES = [(1, 1, 1, 1, 1), (7, 5, 3, 40, 65), (5, 32, 16, 4, 128), (3, 64, 2, 5, 64), (4100, 3, 1, 4, 2), (0, 4, 2, 8, 4)]


def _inputs(n_dst, fan, H, D, T, seed=0, dt_max=1000, unit_omega=False):
    """-> (nbr, dt int64, {name: float64 CPU tensor}, (g_out, g_tagg)) on n_dst + 3 source nodes."""
    rng, n_src = np.random.default_rng(seed), n_dst + 3
    nbr = torch.from_numpy(R.block_rows(rng, n_dst, fan, n_src))
    dt = torch.from_numpy(rng.integers(0, dt_max, size=(n_dst, fan)))
    shapes = dict(q=(n_dst, H, D), k=(n_src, H, D), v=(n_src, H, D), qt=(n_dst, H, T), omega=(T,), phase=(T,))
    x = {n: torch.from_numpy(rng.standard_normal(s)).float().double() for n, s in shapes.items()}
    if unit_omega:
        x["omega"].fill_(1.0)
    go = tuple(torch.from_numpy(rng.standard_normal(s)).float().double() for s in ((n_dst, H, D), (n_dst, H, T)))
    return nbr, dt, x, go


def _run(fn, x, go, dtype=None, device=None):
    """fn(q, k, v, qt, omega, phase) -> (out, tagg) on copies of x, and its backward -> every result, float64 on the CPU."""
    a = {n: t.to(device=device, dtype=dtype, copy=True).requires_grad_() for n, t in x.items()}
    out = fn(*(a[n] for n in NAMES))
    torch.autograd.backward(out, [g.to(device=device, dtype=dtype) for g in go])
    res = {"out": out[0], "tagg": out[1], **{"grad_" + n: a[n].grad for n in NAMES}}
    return {n: t.detach().double().cpu() for n, t in res.items()}


def _three(nbr, dt, x, go):
    """The float64 reference, the fp32 fallback and the native path on the same inputs."""
    from COALA_GNN.sampler import Block
    blk = Block(torch.arange(x["k"].shape[0]).cuda(), nbr.cuda(), nbr.shape[0])
    ref = _run(lambda q, k, v, qt, om, ph: R.op_ref(nbr, q, k, v, qt, dt, om, ph), x, go)
    low = _run(lambda q, k, v, qt, om, ph: blk.time_attn_aggregate_torch(q, k, v, qt, dt.cuda(), om, ph), x, go, torch.float32, "cuda")
    nat = _run(lambda q, k, v, qt, om, ph: blk.time_attn_aggregate(q, k, v, qt, dt.cuda(), om, ph), x, go, torch.float32, "cuda")
    return blk, ref, low, nat


def _hold(ref, low, nat, tag):
    for n, want in ref.items():
        dist = float((low[n] - want).abs().max()) if want.numel() else 0.0
        err = (nat[n] - want).abs()
        print(f"{tag} {n:10s}: fallback fp32 distance {dist:.3e} | native {float(err.max()) if err.numel() else 0.0:.3e}")
        assert (err <= 2.0 * dist + 4 * EPS * want.abs()).all(), f"{tag} {n}: native {float(err.max()):.3e} from float64, the fallback {dist:.3e}"


@pytest.fixture
def native_only(monkeypatch):
    """-> a list that grows by one with every call of the native autograd Function."""
    from COALA_GNN import sampler as S
    calls, real = [], S._TimeAttnAggregate
    monkeypatch.setattr(S, "_TimeAttnAggregate", types.SimpleNamespace(apply=lambda *a: (calls.append(1), real.apply(*a))[1]))
    return calls


@pytest.mark.parametrize("case", CASES + [(6, 9, 2, 8, 16, "large arguments")], ids=str)
def test_native_against_float64(hiplib, native_only, case):
    """The last case has omega = 1 and integer dt up to 1e4, arguments a fast cosine loses."""
    large = len(case) == 6
    nbr, dt, x, go = _inputs(*case[:5], seed=len(CASES) + case[0], dt_max=10000 if large else 1000, unit_omega=large)
    blk, ref, low, nat = _three(nbr, dt, x, go)
    assert len(native_only) == 1, "the native kernel did not run"
    _hold(ref, low, nat, str(case))
    again = _run(lambda q, k, v, qt, om, ph: blk.time_attn_aggregate(q, k, v, qt, dt.cuda(), om, ph), x, go, torch.float32, "cuda")
    for n in ("out", "tagg", "grad_q", "grad_qt", "grad_omega", "grad_phase"):   # a second run gives the same bits
        assert torch.equal(again[n], nat[n]), n
    if case[0] >= 3:   # row 1 has no edge: zeros out, and no gradient in
        assert not nat["out"][1].any() and not nat["tagg"][1].any() and not nat["grad_q"][1].any() and not nat["grad_qt"][1].any()


def test_constant_encoding_sums_to_one(hiplib, native_only):
    """T = 1, omega = 0, phase = 0: phi = 1, so tagg is the sum of the row's weights: 1 within a few ulp, exactly 0 on a row without an edge."""
    nbr, dt, x, go = _inputs(40, 17, 4, 8, 1, seed=3)
    x["omega"].zero_(), x["phase"].zero_()
    _, _, _, nat = _three(nbr, dt, x, go)
    empty = (nbr < 0).all(1)
    assert empty.any() and not nat["tagg"][empty].any() and float((nat["tagg"][~empty] - 1.0).abs().max()) <= 4 * EPS


def test_dispatch_parity(hiplib, native_only):
    """A ragged block, float64 inputs and T = 129 take the fallback: its shapes and values."""
    from COALA_GNN.sampler import Block
    nbr, dt, x, go = _inputs(6, 4, 2, 8, 129, seed=5)
    blk = Block(torch.arange(9).cuda(), nbr.cuda(), 6)
    csr = Block(torch.arange(9).cuda(), None, 6, indptr=torch.arange(0, 25, 4).cuda(), indices=nbr.reshape(-1).clamp_min(0).cuda())
    x64, go64 = {n: (t[..., :8] if n in ("qt", "omega", "phase") else t) for n, t in x.items()}, (go[0], go[1][..., :8])
    for b, xs, gs, dtype, d in [(blk, x, go, torch.float32, dt), (blk, x64, go64, torch.float64, dt), (csr, x64, go64, torch.float32, dt.reshape(-1))]:
        got = _run(lambda *a: b.time_attn_aggregate(a[0], a[1], a[2], a[3], d.cuda(), a[4], a[5]), xs, gs, dtype, "cuda")
        want = _run(lambda *a: b.time_attn_aggregate_torch(a[0], a[1], a[2], a[3], d.cuda(), a[4], a[5]), xs, gs, dtype, "cuda")
        for n in want:
            assert got[n].shape == want[n].shape
            torch.testing.assert_close(got[n], want[n], rtol=1e-5, atol=1e-5, msg=lambda m, n=n: f"{n}: {m}")   # index_add's atomics reorder sums
    assert not native_only, "a case outside the native bounds reached the kernel"


@pytest.fixture(scope="module")
def sampled(hiplib):
    """Two temporal blocks (fan-out 5, 5) of 64 seeds on a small power-law graph, and features for their input nodes."""
    from COALA_GNN.sampler import TemporalNeighborSampler, sort_csc_by_time
    from COALA_GNN.synthetic import powerlaw_csc
    indptr, indices = powerlaw_csc(2000, 8, seed=1)
    ts = torch.randint(0, 1 << 20, (indices.numel(),), generator=torch.Generator().manual_seed(2)).cuda()
    indices, ts, _ = sort_csc_by_time(indptr, indices, ts)
    smp = TemporalNeighborSampler([5, 5], seed=3)
    g = smp.make_graph(indptr, indices, edata={"ts": ts})
    seeds = torch.randperm(2000, generator=torch.Generator().manual_seed(4))[:64].cuda()
    _, _, blocks = smp.sample(g, seeds, seed_times=torch.full((64,), 1 << 19).cuda())
    x = torch.randn(blocks[0].num_src, 16, generator=torch.Generator().manual_seed(5))
    return blocks, x


def test_tgatconv_on_a_sampled_block(sampled, native_only):
    """Against the per-edge float64 layer with the same parameters: output and every gradient, held as the op is."""
    from COALA_GNN.nn import TGATConv
    from COALA_GNN.sampler import Block
    b, x = sampled[0][0], sampled[1]
    nbr, dt = b.nbr.cpu(), b.edata["dt"].cpu()
    torch.manual_seed(6)
    conv = TGATConv(16, 24, 3, 20, time_scale=1e-3)
    go = torch.randn(b.num_dst, 24, generator=torch.Generator().manual_seed(7))
    res = {}
    for run in ("ref", "low", "nat"):
        c = TGATConv(16, 24, 3, 20, time_scale=1e-3)
        c.load_state_dict(conv.state_dict())
        c = c.double() if run == "ref" else c.cuda()
        h = (x.double() if run == "ref" else x.cuda()).requires_grad_()
        blk = Block(b.src_nodes, b.nbr, b.num_dst)
        if run == "low":
            blk.time_attn_aggregate = blk.time_attn_aggregate_torch
        y = R.layer_ref(c, nbr, h, h[: b.num_dst], dt) if run == "ref" else c(blk, h, b.edata["dt"])
        y.backward(go.to(y))
        res[run] = {n: t.detach().double().cpu() for n, t in [("out", y), ("grad_h", h.grad)] + [(n, p.grad) for n, p in c.named_parameters()]}
    assert len(native_only) == 1
    _hold(res["ref"], res["low"], res["nat"], "TGATConv")


def test_tgat_trains(sampled, native_only):
    from COALA_GNN.harness import TGAT
    blocks, x = sampled
    torch.manual_seed(8)
    model = TGAT(16, 32, 5, num_layers=2, num_heads=2, time_dim=12, time_scale=1e-3).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    labels = (blocks[-1].dstdata["_ID"] % 5).cuda()
    losses = []
    for _ in range(20):
        loss = torch.nn.functional.cross_entropy(model(blocks, x.cuda()), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert len(native_only) == 40 and losses[-1] < losses[0] and model.layers[0].time_encoder.omega.grad.abs().max() > 0, losses
