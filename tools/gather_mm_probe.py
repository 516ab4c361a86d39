"""block_ops.gather_mm (typed linear on the fp32 matrix units) against gather_mm_torch, with torch's dense x @ W[0] as the yardstick of the
matrix pipeline (development tool).

powerlaw_csc(200000, 30), 1024 seeds; M = the input nodes of the batch at fan-out 5,5 and at 10,10; T = 1 / 4 / 8 / 64 uniformly drawn
types; (in, out) = (128, 512), (512, 512), (1024, 512).  Per shape: forward, and forward + backward (both gradients), of gather_mm and
of gather_mm_torch, and the dense product; at (512, 512) also the form RelGATConv's projection would use, rows= with every source named
twice on average and W transposed (grad_x through float atomics).  HIP events around every call, median of --iters [min .. max], the
variants taking turns in one process over two rounds whose samples are pooled; achieved FLOP/s = 2 M in out over the forward's median.
Before a shape is timed the native result and both gradients are compared with the fallback's on the same inputs: the largest
difference over the fallback's largest magnitude, which must stay below 1e-4 (fp32 sums of up to M terms in another order).  Each
(fan-out, T) runs in a child process under a time limit of its own; the first one that fails ends the run.
Not timed: HGTConv / RelGATConv or whole model steps -- no layer but nn.TypedLinear runs on the op.
  python tools/gather_mm_probe.py [--iters 15] [--limit 240]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "coala-gnn_amd"))

FANOUTS = ([5, 5], [10, 10])
TYPES = (1, 4, 8, 64)
SHAPES = ((128, 512), (512, 512), (1024, 512))


def samples_us(fn, iters):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


def take_turns(variants, iters):
    """-> {name: (median, min, max)} in us"""
    pool = {name: [] for name, _ in variants}
    for _ in range(2):
        for name, fn in variants:
            pool[name] += samples_us(fn, iters)
    return {name: (sorted(v)[len(v) // 2], min(v), max(v)) for name, v in pool.items()}


def shape(M, T, K, N, iters, packed):
    """packed: x has M // 2 rows, rows= names them at random, W is stored [T, out, in]."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(M // 2 if packed else M, K, device="cuda", generator=gen).requires_grad_(True)
    W = (torch.randn((T, N, K) if packed else (T, K, N), device="cuda", generator=gen) / K ** 0.5).requires_grad_(True)
    types = torch.randint(0, T, (M,), device="cuda", generator=gen, dtype=torch.int32)
    rows = torch.randint(0, x.shape[0], (M,), device="cuda", generator=gen, dtype=torch.int32) if packed else None
    g = torch.randn(M, N, device="cuda", generator=gen)

    def fwd(fn):
        with torch.no_grad():
            return fn(x, W, types, rows, transposed=packed, validate=False)

    def both(fn):
        x.grad = W.grad = None
        y = fn(x, W, types, rows, transposed=packed, validate=False)
        y.backward(g)
        return y.detach(), x.grad, W.grad

    worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(both(gather_mm), both(gather_mm_torch)))
    variants = [("fwd native", lambda: fwd(gather_mm)), ("fwd torch", lambda: fwd(gather_mm_torch)), ("fwd+bwd native", lambda: both(gather_mm)),
                ("fwd+bwd torch", lambda: both(gather_mm_torch))]
    if not packed:
        variants.append(("dense x @ W[0]", lambda: x.detach() @ W.detach()[0]))
    res = take_turns(variants, iters)
    flop = 2.0 * M * K * N
    print(f"M={M} T={T} in={K} out={N}{' rows= transposed' if packed else ''}: native against torch, largest relative difference {worst:.1e}")
    for name, (med, lo, hi) in res.items():
        rate = f"  {flop / med / 1e6:6.1f} TFLOP/s" if name in ("fwd native", "dense x @ W[0]") else ""
        print(f"  {name:15s} {med:8.0f} us [{lo:.0f} .. {hi:.0f}]{rate}")
    n, t = res["fwd+bwd native"][0], res["fwd+bwd torch"][0]
    print(f"  fwd+bwd native / torch {n / t:.2f}" + ("" if T < 4 or n <= t else "   CONDITION FAILS (T >= 4: not slower than gather_mm_torch)"), flush=True)
    return worst < 1e-4


def case(fanout, T, iters):
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import powerlaw_csc
    torch.cuda.set_device(0)
    n_nodes = 200000
    indptr, indices = powerlaw_csc(n_nodes, 30.0, seed=0, device="cuda")
    s = NeighborSampler(fanout)
    graph = s.make_graph(indptr, indices)
    M = int(s.sample(graph, torch.randperm(n_nodes, generator=torch.Generator().manual_seed(0))[:1024].cuda())[0].numel())
    graph.close()
    print(f"fan-out {fanout}: {M} input nodes", flush=True)
    ok = True
    for K, N in SHAPES:
        ok &= shape(M, T, K, N, iters, False)
        if (K, N) == (512, 512):
            ok &= shape(M, T, K, N, iters, True)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--limit", type=int, default=240, help="seconds for one (fan-out, T)")
    ap.add_argument("--case", type=int, nargs=2, metavar=("FANOUT", "T"), help="run one (fan-out, T) in this process")
    args = ap.parse_args()
    if args.case:
        return case(FANOUTS[args.case[0]], args.case[1], args.iters)
    for f in range(len(FANOUTS)):
        for T in TYPES:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--case", str(f), str(T)], timeout=args.limit).returncode
            if rc:
                print(f"fan-out {FANOUTS[f]} T={T} ended with {rc}: stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    if "--case" in sys.argv:
        import torch  # noqa: E402
        from COALA_GNN.block_ops import gather_mm, gather_mm_torch  # noqa: E402
    sys.exit(main())
