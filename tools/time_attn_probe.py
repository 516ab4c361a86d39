"""Temporal attention aggregation, the native kernels against Block.time_attn_aggregate_torch, with dot-product attention's figures
beside them to show what the time part costs (development tool).

powerlaw_csc(200000, 30) with sorted synthetic timestamps, 1024 seeds queried at the middle of the time range, TemporalNeighborSampler
with fan-outs 10,10 and 20,20: the input and the output block of each.  Shapes (H, D, T) = (2, 64, 128) and (4, 128, 100).  For time
native, time torch and dot native: forward, and forward + backward (gradients for q, k, v, qt, omega and phase; q, k, v for dot), HIP
events around one call, median of --iters, the three paths taking turns inside every iteration so that what else runs on the machine
hits them alike; and torch.cuda.max_memory_allocated of one forward + backward above what was allocated before it.  The last line
states the condition the native path is held to: on the input blocks, at both shapes, native forward + backward is not slower than the
fallback.
  python tools/time_attn_probe.py [--iters 20]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "coala-gnn_amd"))
import torch  # noqa: E402

from COALA_GNN.sampler import TemporalNeighborSampler  # noqa: E402
from COALA_GNN.synthetic import edge_times, powerlaw_csc  # noqa: E402


def medians_ms(fns, iters):
    """Median HIP-event time of every fn, one call of each per iteration, in turn."""
    for _ in range(3):
        for fn in fns:
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for _ in fns]
    for i in range(iters):
        for fn, e in zip(fns, ev):
            e[i][0].record()
            fn()
            e[i][1].record()
    torch.cuda.synchronize()
    return [sorted(a.elapsed_time(b) for a, b in e)[iters // 2] for e in ev]


def peak_mb(step):
    """Peak allocation of one step above the allocation it starts from, MB."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def probe(tag, b, H, D, T, iters):
    gen = torch.Generator(device="cuda").manual_seed(0)
    E = int((b.nbr >= 0).sum())
    mk = lambda *s: torch.randn(*s, device="cuda", generator=gen).requires_grad_(True)   # noqa: E731
    q, k, v, qt = mk(b.num_dst, H, D), mk(b.num_src, H, D), mk(b.num_src, H, D), mk(b.num_dst, H, T)
    omega = (1.0 / 10.0 ** torch.linspace(0, 9, T, device="cuda")).requires_grad_(True)
    phase = torch.zeros(T, device="cuda", requires_grad=True)
    dt = b.edata["dt"].float()
    g, gt = torch.randn(b.num_dst, H, D, device="cuda", generator=gen), torch.randn(b.num_dst, H, T, device="cuda", generator=gen)
    time_args, dot_args = (q, k, v, qt, omega, phase), (q, k, v)
    ops = [("time native", lambda: b.time_attn_aggregate(q, k, v, qt, dt, omega, phase), time_args),
           ("time torch", lambda: b.time_attn_aggregate_torch(q, k, v, qt, dt, omega, phase), time_args),
           ("dot native", lambda: (b.dot_gat_aggregate(q, k, v, validate=False), gt), dot_args)]

    def stepper(op, args):
        def step():
            for t in args:
                t.grad = None
            out, tagg = op()
            ((out * g).sum() + (tagg * gt).sum()).backward()
        return step
    steps = [stepper(op, args) for _, op, args in ops]
    print(f"{tag}: n_dst {b.num_dst}, n_src {b.num_src}, fan-out {b.nbr.shape[1]}, edges {E}, H {H}, D {D}, T {T}; [E, T] fp32 is "
          f"{E * T * 4 / 1e6:.1f} MB, [E, H, D] {E * H * D * 4 / 1e6:.1f} MB, [E, H, T] {E * H * T * 4 / 1e6:.1f} MB", flush=True)
    with torch.no_grad():
        fwd = medians_ms([op for _, op, _ in ops], iters)
    fb = medians_ms(steps, iters)
    res = {}
    for (name, _, args), f, t, step in zip(ops, fwd, fb, steps):
        for x in args:
            x.grad = None
        res[name] = (f, t, peak_mb(step))
        print(f"  {name:11s} fwd {f:8.3f} ms   fwd+bwd {t:8.3f} ms   peak memory of fwd+bwd {res[name][2]:8.1f} MB", flush=True)
    n, t, d = res["time native"], res["time torch"], res["dot native"]
    print(f"  time native against torch: fwd {t[0] / n[0]:.2f}x, fwd+bwd {t[1] / n[1]:.2f}x, peak memory {t[2] - n[2]:.1f} MB lower; against dot "
          f"native: fwd {n[0] / d[0]:.2f}x the time, fwd+bwd {n[1] / d[1]:.2f}x", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=200_000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    indptr, indices = powerlaw_csc(args.rows, 30.0, seed=0, device="cuda")
    ts = edge_times(indptr, seed=1)
    seeds = torch.randperm(args.rows, device="cuda")[:1024]
    verdicts = []
    for fan in ([10, 10], [20, 20]):
        s = TemporalNeighborSampler(fan)
        g = s.make_graph(indptr, indices, edata={"ts": ts})
        _, _, blocks = s.sample(g, seeds, seed_times=torch.full((1024,), 1 << 19, device="cuda"))
        for H, D, T in ((2, 64, 128), (4, 128, 100)):
            for layer, name in enumerate(("input", "output")):
                r = probe(f"fan-out {fan} {name} block", blocks[layer], H, D, T, args.iters)
                if layer == 0:
                    verdicts.append((fan, (H, D, T), r["time native"][1], r["time torch"][1]))
        g.close()
    ok = all(n <= t for _, _, n, t in verdicts)
    for fan, shape, n, t in verdicts:
        print(f"condition, fan-out {fan} input block, (H, D, T) = {shape}: native fwd+bwd {n:.3f} <= torch {t:.3f} ms: {'holds' if n <= t else 'FAILS'}")
    print(f"condition (median against median, every input block): {'holds' if ok else 'FAILS'}", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
