#!/usr/bin/env python3
"""What a sparse embedding update costs through the write-through cache (profiles/r17_embedding_update.txt).

powerlaw_csc(200000, 30); the ids are the input nodes of a 1024-seed batch at fan-out 5,5 and at 10,10; dim 128 and 1024; pinned table,
64 MB cache, warmed by one read of the ids; Adagrad state in HBM and in pinned host memory.  Timed, HIP events around each call, median
of 20 (us):
  adagrad_rows                      the fused native step
  write_rows assign / add
  composed                          read_feature -> torch Adagrad math on the rows -> write_rows(assign): the measure for condition 1
                                    (adagrad_rows no slower than it at every shape), not the code under test
  hipMemcpy D2H                     a pinned device-to-host copy of the rows' bytes in the same process: the host link's write rate
and, with no threshold, the write's delivered host-link rate (4 dim bytes per row written, hits need no read) as a share of that copy."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import torch  # noqa: E402
import COALA_GNN_Pybind as P  # noqa: E402
from COALA_GNN.sampler import NeighborSampler  # noqa: E402
from COALA_GNN.synthetic import PinnedFeatureTable, powerlaw_csc  # noqa: E402

torch.cuda.set_device(0)
N, B, REPS, CACHE_MB, LR, EPS = 200_000, 1024, 20, 64, 0.05, 1e-10
ip, ix = powerlaw_csc(N, 30.0, seed=0, device="cuda")


def timed(fn, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(REPS):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        z.record()
        z.synchronize()
        out.append(a.elapsed_time(z) * 1e3)
    return statistics.median(out), min(out), max(out)


def line(name, t, extra=""):
    print(f"  {name:44s} {t[0]:9.1f}  [{t[1]:.1f} .. {t[2]:.1f}]{extra}")
    return t[0]


print(f"graph powerlaw_csc({N}, 30), {B} seeds, {CACHE_MB} MB cache over a pinned table; us, median of {REPS} event-timed calls [min .. max]")
worst = 0.0
for fan in ([5, 5], [10, 10]):
    s = NeighborSampler(fan, seed=1)
    g = s.make_graph(ip, ix)
    ids = s.sample(g, torch.randperm(N, generator=torch.Generator().manual_seed(0))[:B].cuda())[0].contiguous()
    n = ids.numel()
    for dim in (128, 1024):
        table = PinnedFeatureTable(N, dim, 0)
        table.cpu_tensor.uniform_(-1.0, 1.0)
        ctrl = P.SSD_GNN_SSD_Controllers(1, dim * 4, 1024, 0, 0, dim, True)
        cache = P.Isolated_Cache(ctrl, None, 0, 1, CACHE_MB, table.device_ptr, num_rows=N, sync=False)
        rows = torch.empty((n, dim), dtype=torch.float32, device="cuda")
        grad = torch.randn((n, dim), device="cuda") * 0.1
        cache.read_feature(rows.data_ptr(), ids.data_ptr(), n)      # warm: what fits of the batch is cached, as behind a loader's fetch
        cache.stats(reset=True)
        cache.read_feature(rows.data_ptr(), ids.data_ptr(), n)
        hit, miss, _ = cache.stats(reset=True)
        mb = n * dim * 4 / 1e6
        print(f"fan-out {fan}, dim {dim}: {n} rows = {mb:.1f} MB per direction; {hit} of them cached")
        host_buf = torch.empty((n, dim), dtype=torch.float32).pin_memory()
        t_copy = line("hipMemcpy D2H, pinned, same bytes", timed(lambda: host_buf.copy_(rows, non_blocking=True)))
        copy_rate = mb * 1e6 / (t_copy * 1e-6) / 1e9
        print(f"  {'':44s} -> {copy_rate:.1f} GB/s")
        t_as = line("write_rows assign", timed(lambda: cache.write_rows(ids.data_ptr(), n, grad.data_ptr(), "assign")))
        print(f"  {'':44s} -> {mb * 1e-3 / (t_as * 1e-6):.1f} GB/s to the host = {100 * mb * 1e-3 / (t_as * 1e-6) / copy_rate:.0f} % of the copy's rate")
        t_add = line("write_rows add", timed(lambda: cache.write_rows(ids.data_ptr(), n, grad.data_ptr(), "add", -LR)))
        print(f"  {'':44s} -> {mb * 1e-3 / (t_add * 1e-6):.1f} GB/s to the host = {100 * mb * 1e-3 / (t_add * 1e-6) / copy_rate:.0f} % of the copy's rate")
        for where in ("HBM", "pinned host"):
            if where == "HBM":
                state, keep = torch.zeros((N, dim), dtype=torch.float32, device="cuda"), None
                state_ptr = state.data_ptr()
            else:
                keep = PinnedFeatureTable(N, dim, 0)
                keep.cpu_tensor.zero_()
                state, state_ptr = None, keep.device_ptr
            t_ada = line(f"adagrad_rows, state in {where}",
                         timed(lambda: cache.adagrad_rows(ids.data_ptr(), n, grad.data_ptr(), state_ptr, LR, EPS)))
            print(f"  {'':44s} -> {mb * 1e-3 / (t_ada * 1e-6):.1f} GB/s of rows to the host = {100 * mb * 1e-3 / (t_ada * 1e-6) / copy_rate:.0f} % of the copy's rate")
            if where == "HBM":
                def composed():
                    cache.read_feature(rows.data_ptr(), ids.data_ptr(), n)
                    st = state[ids] + grad * grad
                    state[ids] = st
                    new = rows - LR * grad / (st.sqrt() + EPS)
                    cache.write_rows(ids.data_ptr(), n, new.data_ptr(), "assign")
                t_cmp = line("composed: read, torch Adagrad, assign (HBM)", timed(composed))
                ratio = t_ada / t_cmp
                worst = max(worst, ratio)
                print(f"  {'':44s} adagrad_rows / composed = {ratio:.2f}  (condition 1: <= 1)")
            if keep is not None:
                keep.close()
        cache.close()
        table.close()
print(f"condition 1 (adagrad_rows no slower than the composed path at every shape): worst ratio {worst:.2f} -> {'holds' if worst <= 1.0 else 'FAILS'}")
print("not measured: the step inside a training loop beside the next fetch; an HBM table; misaligned (scalar-path) tables; dims other than 128 and 1024")
