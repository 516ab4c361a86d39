"""Block.lstm_aggregate (native, coala_lstm.hip) against Block.lstm_aggregate_torch and against what a user ran before it existed: gather
the mailbox [num_dst, k, H] and run torch.nn.LSTM on it (profiles/r29_lstm_aggregate.txt).

powerlaw_csc(200000, 30), one batch of 1024 seeds at fan-out 5,5 and 10,10, the input and the output block of each, H = 128 and 256.
Per shape: forward, and forward + backward (gradients for the per-node features and every weight), of the three paths; HIP-event
medians of 20 (two turns of 10 per variant, the variants alternating in one process), min and max beside them; the peak allocation of
one forward + backward of each; and the three results compared at every timed shape (the mailbox path reads a padding slot as source
row 0, for timing only: it is compared on the rows without padding).  All three paths start from the node features x and include the
input projection: once per source node on the native and the fallback path, once per edge inside nn.LSTM.

Condition: native forward + backward on the 5,5 input block at H = 128 takes no longer than gather + nn.LSTM.
Not measured: ragged (fan-out -1) batches, a training epoch.

  python tools/lstm_aggregate_probe.py [--iters 10]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "coala-gnn_amd"))

import torch  # noqa: E402

from COALA_GNN.sampler import NeighborSampler  # noqa: E402
from COALA_GNN.synthetic import powerlaw_csc  # noqa: E402


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


def shape(tag, blk, H, iters):
    gen = torch.Generator(device="cuda").manual_seed(0)
    lstm = torch.nn.LSTM(H, H, batch_first=True).cuda()
    x = torch.randn(blk.num_src, H, device="cuda", generator=gen).requires_grad_(True)
    go = torch.randn(blk.num_dst, H, device="cuda", generator=gen)
    mail = blk.nbr.clamp_min(0).long()
    full = (blk.nbr >= 0).all(1)

    def block_path(fn):
        return lambda: fn(torch.addmm(lstm.bias_ih_l0 + lstm.bias_hh_l0, x, lstm.weight_ih_l0.t()), lstm.weight_hh_l0)

    paths = {"native": block_path(blk.lstm_aggregate), "torch": block_path(blk.lstm_aggregate_torch), "gather+nn.LSTM": lambda: lstm(x[mail])[1][0][0]}

    def fwd(f):
        def run():
            with torch.no_grad():
                return f()
        return run

    def both(f):
        def run():
            x.grad = None
            lstm.zero_grad(set_to_none=True)
            out = f()
            (out * go).sum().backward()
            return out.detach(), x.grad, lstm.weight_hh_l0.grad
        return run

    print(f"{tag} H={H}: {blk.num_dst} dst, {blk.num_src} src, {int((blk.nbr >= 0).sum())} edges in {blk.nbr.numel()} slots, {int(full.sum())} rows without padding", flush=True)
    ref = both(paths["native"])()
    for name in ("torch", "gather+nn.LSTM"):
        got = both(paths[name])()
        rows = slice(None) if name == "torch" else full
        print(f"  native against {name}: out {float((got[0][rows] - ref[0][rows]).abs().max()):.2e}" +
              (f", grad_x {float((got[1] - ref[1]).abs().max()):.2e}, grad_w_hh {float((got[2] - ref[2]).abs().max()):.2e}" if name == "torch" else ""), flush=True)
    for name, f in paths.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        both(f)()
        torch.cuda.synchronize()
        print(f"  peak allocation of forward + backward, {name}: {(torch.cuda.max_memory_allocated() - base) / 2**20:.1f} MiB", flush=True)
    med = take_turns([(f"{kind} {name}", wrap(f)) for kind, wrap in (("fwd", fwd), ("fwd+bwd", both)) for name, f in paths.items()], iters)
    for name, (m, lo, hi) in med.items():
        print(f"  {name:28s} median {m:9.1f} us  (min {lo:9.1f}, max {hi:9.1f})", flush=True)
    n, lib = med["fwd+bwd native"][0], med["fwd+bwd gather+nn.LSTM"][0]
    print(f"  fwd+bwd native / gather+nn.LSTM {n / lib:.2f}, native / torch {n / med['fwd+bwd torch'][0]:.2f}" +
          ("   NATIVE IS SLOWER THAN THE LIBRARY PATH" if n > lib else ""), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="samples per variant and turn (two turns)")
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0), "torch", torch.__version__, flush=True)
    ip, ix = powerlaw_csc(200000, 30, seed=0)
    seeds = torch.randperm(200000, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))[:1024]
    for fan in ([5, 5], [10, 10]):
        smp = NeighborSampler(fan, seed=1)
        _, _, blocks = smp.sample(smp.make_graph(ip, ix), seeds)
        for tag, blk in (("input", blocks[0]), ("output", blocks[-1])):
            for H in (128, 256):
                shape(f"fan-out {fan[0]},{fan[1]} {tag} block", blk, H, args.iters)
