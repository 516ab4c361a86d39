"""A time-decay model on really sampled temporal blocks against a float64 restatement over (node, time) pairs.

Two layers of a linear propagation, no activation and therefore no kinks:
    h(v, t) = W_self x_v + W_nb * sum_e exp(-lambda dt_e) x_src(e) / sum_e exp(-lambda dt_e),      dt_e = t - ts[e],
once more on top, the sums over the edges TemporalNeighborSampler([5, 5]) took for the pair (v, t); a pair without an edge aggregates 0.
The product path runs on the blocks through Block.weighted_sum_aggregate with block.edata['dt']; the restatement recurses over
(node, time) pairs from the edge lists of tests/_temporal_ref.py and never sees a local index.  Tolerance: the project's own rule
(_global_ref.Evaluation.tolerance): 4 x the error of the same restatement evaluated in float32 against float64."""
import types

import numpy as np
import pytest

import _global_ref as R
from _temporal_ref import decode, reference_layers

pytestmark = pytest.mark.gpu

N, IN, HID, OUT = 3000, 16, 12, 8
LAMBDA = 0.004
SEED, STEP = 9, 2


def _restate(dtype, X, W, ip, ix, ts, ref, slot_time, nodes, times):
    """h2 of every seed pair in `dtype`, by recursion over (node, time) pairs."""
    edges = []                                   # per sampled layer: (node, time) -> the edge ids its row took
    dst_codes = ref[0][0][: len(nodes)]
    for src, _, eid in ref:
        dn, dt = decode(dst_codes, slot_time, N)
        edges.append({(int(v), int(t)): row[row >= 0] for v, t, row in zip(dn, dt, eid)})
        dst_codes = src
    X = X.astype(dtype)
    (Ws1, Wn1), (Ws2, Wn2) = [(a.astype(dtype), b.astype(dtype)) for a, b in W]
    lam = dtype(LAMBDA)

    def aggregate(e, t, rows):
        w = np.exp(-lam * (t - ts[e]).astype(dtype))
        return (w[:, None] * rows).sum(0, dtype=dtype) / w.sum(dtype=dtype)

    memo = {}

    def h1(u, t):
        if (u, t) not in memo:
            e = edges[1][(u, t)]
            agg = aggregate(e, t, X[ix[e]]) if len(e) else np.zeros(IN, dtype=dtype)
            memo[(u, t)] = Ws1 @ X[u] + Wn1 @ agg
        return memo[(u, t)]

    out = np.zeros((len(nodes), OUT), dtype=dtype)
    for i, (v, t) in enumerate(zip(nodes.tolist(), times.tolist())):
        e = edges[0][(v, t)]
        agg = aggregate(e, t, np.stack([h1(int(u), t) for u in ix[e]])) if len(e) else np.zeros(HID, dtype=dtype)
        out[i] = Ws2 @ h1(v, t) + Wn2 @ agg
    return out


@pytest.mark.parametrize("strategy", ["uniform", "last"])
def test_time_decay_model_against_pair_reference(hiplib, strategy):
    import torch
    from COALA_GNN.sampler import TemporalNeighborSampler
    from COALA_GNN.synthetic import edge_times, powerlaw_csc
    d_ip, d_ix = powerlaw_csc(N, 12, seed=2, device="cuda")
    d_ts = edge_times(d_ip, seed=3, t_max=1000)
    g = TemporalNeighborSampler.make_graph(d_ip, d_ix, edata={"ts": d_ts})
    ip, ix, ts = d_ip.cpu().numpy(), d_ix.cpu().numpy(), d_ts.cpu().numpy()
    rng = np.random.default_rng(4)
    X = rng.standard_normal((N, IN)).astype(np.float32)
    W = [(rng.standard_normal((HID, IN)).astype(np.float32) / 4, rng.standard_normal((HID, IN)).astype(np.float32) / 4),
         (rng.standard_normal((OUT, HID)).astype(np.float32) / 4, rng.standard_normal((OUT, HID)).astype(np.float32) / 4)]
    nodes = rng.permutation(N)[:256].astype(np.int64)
    times = rng.integers(100, 1100, size=256).astype(np.int64)
    smp = TemporalNeighborSampler([5, 5], strategy=strategy, seed=SEED)
    input_nodes, _, blocks = smp.sample(g, torch.from_numpy(nodes).cuda(), step=STEP, seed_times=torch.from_numpy(times).cuda())
    # ---- the product path: fp32, the native weighted-sum kernel on the sampled blocks
    h = torch.from_numpy(X).cuda()[input_nodes]
    for b, (Ws, Wn) in zip(blocks, W):
        w = torch.exp(-LAMBDA * b.edata["dt"].to(torch.float32)) * (b.nbr >= 0)
        agg = b.weighted_sum_aggregate(h, w.contiguous()) / w.sum(1, keepdim=True).clamp_min(1e-30)
        h = b.dst_rows(h) @ torch.from_numpy(Ws).cuda().T + agg @ torch.from_numpy(Wn).cuda().T
    got = h.cpu().numpy()
    # ---- the restatement, in global (node, time) pairs
    ref, slot_time = reference_layers(ip, ix, ts, nodes, times, [5, 5], SEED, STEP, strategy)
    r64 = _restate(np.float64, X, W, ip, ix, ts, ref, slot_time, nodes, times)
    r32 = _restate(np.float32, X, W, ip, ix, ts, ref, slot_time, nodes, times)
    holder = types.SimpleNamespace(ref=types.SimpleNamespace(arrays=lambda: {"out": r64}), ref32=types.SimpleNamespace(arrays=lambda: {"out": r32}))
    tol, e32 = R.Evaluation.tolerance(holder, "out")
    err = float(np.abs(got - r64).max())
    print(f"{strategy}: error {err:.3e} E32 {e32:.3e} ratio {err / e32:.2f} bound {tol:.3e} largest |out| {np.abs(r64).max():.3e}")
    assert (np.abs(r64).sum(1) > 0).all() and e32 > 0
    assert err <= tol, f"off by {err:.3e} (bound {tol:.3e})"
    g.close()
