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
and, with no threshold, the write's delivered host-link rate (4 dim bytes per row written, hits need no read) as a share of that copy.

--optimizers (profiles/r19_embedding_optimizers.txt): the same shapes, the variants ALTERNATING inside every one of the 20 rounds --
adagrad_rows with its state in HBM (the yardstick) and in pinned host memory, adam_rows (per-row steps, state in HBM), the composed Adam
path (read_feature -> torch Adam on the fetched rows and the gathered state -> write_rows assign), rowwise_adagrad_rows -- and three
conditions: adam_rows no slower than the composed path; rowwise_adagrad_rows within 10 % of adagrad_rows (HBM); a RowWiseAdagrad step
faster than a SparseAdagrad step whose state does not fit the device budget (whole optimizer steps on a NodeEmbedding, trace reduction
included)."""
import math
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


def timed_alternating(variants, warm=3):
    """variants: [(name, fn)].  Every round runs each variant once, in order, each between its own pair of events -> {name: (median, min, max)}"""
    for _ in range(warm):
        for _, fn in variants:
            fn()
    out = {name: [] for name, _ in variants}
    for _ in range(REPS):
        for name, fn in variants:
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            z.record()
            z.synchronize()
            out[name].append(a.elapsed_time(z) * 1e3)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in out.items()}


def optimizers():
    from COALA_GNN import NodeEmbedding, RowWiseAdagrad, SparseAdagrad
    B1, B2, AEPS = 0.9, 0.999, 1e-8
    print(f"graph powerlaw_csc({N}, 30), {B} seeds, {CACHE_MB} MB cache over a pinned table; us, median of {REPS} event-timed calls [min .. max], "
          "the variants of a shape alternating inside every round")
    worst1 = worst2 = worst3 = 0.0
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
            cache.read_feature(rows.data_ptr(), ids.data_ptr(), n)
            cache.stats(reset=True)
            cache.read_feature(rows.data_ptr(), ids.data_ptr(), n)
            hit, miss, _ = cache.stats(reset=True)
            mb = n * dim * 4 / 1e6
            print(f"fan-out {fan}, dim {dim}: {n} rows = {mb:.1f} MB per direction; {hit} of them cached")
            ada = torch.zeros((N, dim), dtype=torch.float32, device="cuda")
            ada_pin = PinnedFeatureTable(N, dim, 0)
            ada_pin.cpu_tensor.zero_()
            m, v = (torch.zeros((N, dim), dtype=torch.float32, device="cuda") for _ in range(2))
            cm, cv = (torch.zeros((N, dim), dtype=torch.float32, device="cuda") for _ in range(2))
            steps = torch.zeros(N, dtype=torch.int32, device="cuda")
            row_state = torch.zeros(N, dtype=torch.float32, device="cuda")
            host_buf = torch.empty((n, dim), dtype=torch.float32).pin_memory()
            count = [0]

            def composed_adam():
                count[0] += 1
                t = count[0]
                cache.read_feature(rows.data_ptr(), ids.data_ptr(), n)
                mn = cm[ids].mul_(B1).add_(grad, alpha=1.0 - B1)
                vn = cv[ids].mul_(B2).addcmul_(grad, grad, value=1.0 - B2)
                cm[ids] = mn
                cv[ids] = vn
                bc1, bc2 = -math.expm1(t * math.log(B1)), -math.expm1(t * math.log(B2))
                new = rows - (LR / bc1) * mn / (vn.sqrt() / math.sqrt(bc2) + AEPS)
                cache.write_rows(ids.data_ptr(), n, new.data_ptr(), "assign")

            res = timed_alternating([
                ("hipMemcpy D2H, pinned, same bytes", lambda: host_buf.copy_(rows, non_blocking=True)),
                ("adagrad_rows, state in HBM (yardstick)", lambda: cache.adagrad_rows(ids.data_ptr(), n, grad.data_ptr(), ada.data_ptr(), LR, EPS)),
                ("adagrad_rows, state in pinned host", lambda: cache.adagrad_rows(ids.data_ptr(), n, grad.data_ptr(), ada_pin.device_ptr, LR, EPS)),
                ("adam_rows, per-row steps, state in HBM", lambda: cache.adam_rows(ids.data_ptr(), n, grad.data_ptr(), m.data_ptr(), v.data_ptr(), LR,
                                                                                    (B1, B2), AEPS, row_step_ptr=steps.data_ptr())),
                ("composed: read, torch Adam, assign (HBM)", composed_adam),
                ("rowwise_adagrad_rows", lambda: cache.rowwise_adagrad_rows(ids.data_ptr(), n, grad.data_ptr(), row_state.data_ptr(), LR, EPS)),
            ])
            copy_rate = mb * 1e6 / (res["hipMemcpy D2H, pinned, same bytes"][0] * 1e-6) / 1e9
            for name, t in res.items():
                rate = mb * 1e-3 / (t[0] * 1e-6)
                line(name, t, "" if name.startswith("composed") else f"   {rate:5.1f} GB/s of rows to the host = {100 * rate / copy_rate:3.0f} % of the copy's rate")
            r1 = res["adam_rows, per-row steps, state in HBM"][0] / res["composed: read, torch Adam, assign (HBM)"][0]
            r2 = res["rowwise_adagrad_rows"][0] / res["adagrad_rows, state in HBM (yardstick)"][0]
            worst1, worst2 = max(worst1, r1), max(worst2, r2)
            print(f"  adam_rows / composed = {r1:.2f} (condition 1: <= 1);  rowwise_adagrad_rows / adagrad_rows (HBM) = {r2:.2f} (condition 2: <= 1.10)")
            ada_pin.close()
            cache.close()
            table.close()
            del ada, m, v, cm, cv
            torch.cuda.empty_cache()
            if dim == 128:
                # condition 3, by hand: whole optimizer steps (trace reduction included) on a NodeEmbedding of the same table size whose
                # element-wise Adagrad state is not given room on the device
                embs = [NodeEmbedding(N, dim, cache_mb=CACHE_MB, device="cuda:0") for _ in range(2)]
                opts = [SparseAdagrad([embs[0]], lr=LR, state_device_bytes=0), RowWiseAdagrad([embs[1]], lr=LR)]
                assert not opts[0].state_of(embs[0])[0].is_cuda

                def opt_step(k):
                    embs[k].attach(ids, rows).grad = grad
                    opts[k].step()
                res = timed_alternating([("SparseAdagrad.step(), state in pinned host", lambda: opt_step(0)), ("RowWiseAdagrad.step()", lambda: opt_step(1))])
                for name, t in res.items():
                    line(name, t)
                r3 = res["RowWiseAdagrad.step()"][0] / res["SparseAdagrad.step(), state in pinned host"][0]
                worst3 = max(worst3, r3)
                print(f"  RowWiseAdagrad.step() / SparseAdagrad.step() with pinned state = {r3:.2f} (condition 3: < 1)")
                for e in embs:
                    e.close()
    print(f"condition 1 (adam_rows no slower than the composed path at every shape): worst ratio {worst1:.2f} -> {'holds' if worst1 <= 1.0 else 'FAILS'}")
    print(f"condition 2 (rowwise_adagrad_rows within 10 % of adagrad_rows with HBM state): worst ratio {worst2:.2f} -> {'holds' if worst2 <= 1.10 else 'FAILS'}")
    print(f"condition 3 (a RowWiseAdagrad step faster than a SparseAdagrad step with pinned state, dim 128): worst ratio {worst3:.2f} -> {'holds' if worst3 < 1.0 else 'FAILS'}")
    print("not measured: the step inside a training loop beside the next fetch; an HBM table; misaligned (scalar-path) tables; dims other than 128 and 1024; "
          "Adam with its state in pinned host memory; step='global'; condition 3 at dim 1024")


if "--optimizers" in sys.argv:
    optimizers()
    sys.exit(0)

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
