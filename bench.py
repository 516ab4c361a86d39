#!/usr/bin/env python3
"""bench.py -- feature-gather throughput of the MI355X feature-cache path on the IGB-medium GraphSAGE workload.

  python bench.py --gpus N --steps K --warmup W          (N>1: launched by torch.distributed.run, one rank per GPU)

A "step" is one minibatch of the hot path: the sampled input-node ids (already resident in HBM) go through
COALA_GNN_Manager.fetch_feature -> libcoala_hip.so (probe + hit gather, deterministic miss ranking, cold fill from the
pinned-host table; for N>1 the owner-partitioned cache with RCCL all-to-all-v) and come back as the fp32 [n, 1024]
feature tensor in HBM.  Workload at N=1 = BASELINE.json configs[1]: IGB-medium shape (10,000,000 x 1024 fp32 cold table
in pinned host memory), GraphSAGE fan-out 5,5, batch 1024, isolated 4 GiB cache.  N>1 keeps the same per-GPU work
(weak scaling) with the cache sharded by id % N.  Synthetic data: no datasets on the box.

Prints ONE JSON line (rank 0) with metric/value/... plus "roofline" (probe+gather kernel: HIP events attached to every one of its
launches in the timed region, on the stream it is launched on -- the kernel's own begin/end timestamps, which is also what
rocprofv3 reports), "roofline_cold_fill" and, at N>1, "exchange" (both from the same timed region).

A plain run does only what that line needs: set-up, warm-up, the timed steps, --dump-outputs.  --full adds everything that takes
runs of its own after the timed region: the all-hit leg of the probe+gather kernel ("roofline_allhit"), the box's device-to-device
blit rate, "cpu_baseline" (the C oracle, one host core, bounded sample, and the CPU gather / sampler sweeps), the end-to-end epoch
leg, the fan-out 10,10 leg and the colour-affinity leg.
"""
import argparse
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "coala-gnn_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

T_PROCESS_START = time.time()
# Every watchdog deadline of a run is cut off at T_PROCESS_START + this many seconds, so that a hang ends with the JSON line (with an
# "error" field) and a non-zero exit code BEFORE a driver's own limit kills the job silently (its limit: 600 s).  --time-budget S or
# COALA_BENCH_BUDGET_S overrides; extra legs that would not fit into what is left are skipped and say so in the line.
DEFAULT_BUDGET_S = 420.0


def _argv_value(flag, default=None):
    """`--flag V` / `--flag=V` from sys.argv without argparse (the launcher decision is taken before anything heavy is imported)."""
    for i, a in enumerate(sys.argv[1:], 1):
        if a == flag and i + 1 < len(sys.argv):
            return sys.argv[i + 1]
        if a.startswith(flag + "="):
            return a.split("=", 1)[1]
    return default


def _budget_s():
    try:
        return float(_argv_value("--time-budget") or os.environ.get("COALA_BENCH_BUDGET_S") or DEFAULT_BUDGET_S)
    except ValueError:
        return DEFAULT_BUDGET_S


def launch_ranks(n):
    """`python3 bench.py --gpus N` without a launcher around it: start the N ranks as CHILD processes -- one per GPU, as the reference's
    launchers do (examples/4GB_script.sh:28-37, examples/sbatch_ssd_gnn_train.py:249-250) -- relay rank 0's JSON line, return the worst
    exit code.  This process never imports torch and never touches the GPU; nothing is re-executed.  The children get what
    torch.distributed.run would give them (RANK / LOCAL_RANK / WORLD_SIZE / LOCAL_WORLD_SIZE / MASTER_ADDR / MASTER_PORT)."""
    import signal
    import socket
    import subprocess
    import threading
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    budget = _budget_s()
    cpus = len(os.sched_getaffinity(0))
    base = dict(os.environ, WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                COALA_BENCH_T0=repr(T_PROCESS_START), COALA_BENCH_BUDGET_S=repr(budget), COALA_BENCH_LAUNCHER_PID=str(os.getpid()))
    base.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    base.setdefault("OMP_NUM_THREADS", str(max(1, min(16, cpus // n))))   # (torch.distributed.run would say 1)
    cmd = [sys.executable, os.path.abspath(__file__), *sys.argv[1:]]
    kids = []
    for r in range(n):
        env = dict(base, RANK=str(r), LOCAL_RANK=str(r), GROUP_RANK="0")
        # rank 0's stdout comes back through a pipe (the line is relayed and remembered); the other ranks' stdout goes to stderr
        kids.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else sys.stderr, text=(r == 0), start_new_session=True))
    seen = {"line": False}

    def relay():
        for ln in kids[0].stdout:
            if ln.startswith("{"):
                seen["line"] = True
            sys.stdout.write(ln)
            sys.stdout.flush()
    t = threading.Thread(target=relay, daemon=True)
    t.start()

    def stop_all(sig, *_):
        for k in kids:
            if k.poll() is None:
                try:
                    os.killpg(k.pid, sig)          # the rank and whatever it started (its own session: start_new_session)
                except OSError:
                    pass
    for sg in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP):   # a launcher that is told to stop takes its ranks with it
        signal.signal(sg, lambda s_, f_: (stop_all(signal.SIGTERM), time.sleep(2.0), stop_all(signal.SIGKILL), os._exit(128 + s_)))
    # The ranks police themselves (RankGuard: every deadline inside the budget).  This loop is the second line: once one rank has left,
    # the others get 20 s to follow (they see the failure flag / the missing store), and nobody outlives budget + 45 s.
    hard_end = T_PROCESS_START + budget + 45.0
    first_exit = None
    why = None
    while any(k.poll() is None for k in kids):
        now = time.time()
        if first_exit is None and any(k.poll() is not None for k in kids):
            first_exit = now
        if first_exit is not None and now - first_exit > 20.0 and any(k.poll() not in (None, 0) for k in kids):
            why = "a rank exited with an error and the others did not follow within 20 s"
        elif first_exit is not None and now - first_exit > 120.0:
            why = "a rank has finished and the others did not within 120 s"
        elif now > hard_end:
            why = f"the ranks were still running {budget + 45.0:.0f} s after the start (time budget {budget:.0f} s)"
        if why:
            stop_all(signal.SIGTERM)
            time.sleep(3.0)
            stop_all(signal.SIGKILL)
            break
        time.sleep(0.2)
    codes = [k.wait() for k in kids]
    t.join(timeout=5.0)
    worst = next((c for c in codes if c != 0), 0)
    if why and worst == 0:
        worst = 5
    if not seen["line"]:   # no rank got as far as printing: the line still appears, with what is known
        print(json.dumps({"metric": "feature-gather GB/s", "value": None, "unit": "GB/s", "n_gpus": n,
                          "error": why or f"the ranks exited with codes {codes} before rank 0 printed its line"}), flush=True)
        worst = worst or 5
    print(f"[bench] launcher: rank exit codes {codes}" + (f"; {why}" if why else ""), file=sys.stderr, flush=True)
    return worst


if __name__ == "__main__" and "WORLD_SIZE" not in os.environ and "SLURM_NTASKS" not in os.environ:
    try:
        _n_req = int(_argv_value("--gpus", "1"))
    except ValueError:
        _n_req = 1
    if _n_req > 1:
        sys.exit(launch_ranks(_n_req))


def _bind_numa():
    """Before the HIP runtime exists (its helper threads inherit the mask) and before anything is pinned: run this rank on the NUMA
    node of its GPU, so that its shard of the cold tier is allocated next to the link that reads it (COALA_GNN/numa.py; COALA_NUMA=off
    leaves the process where the launcher put it).  numa.py is loaded by path: importing the package would import torch first."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("coala_numa", os.path.join(PKG, "COALA_GNN", "numa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    dev = 0 if os.environ.get("COALA_BENCH_SINGLE_DEVICE") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
    try:
        return mod, mod.bind_to_device_node(dev)
    except Exception as e:  # noqa: BLE001 -- placement is an optimisation: never the reason a run does not start
        return mod, {"applied": False, "why": repr(e)}


ORIG_AFFINITY = os.sched_getaffinity(0)   # before the binding: what an "all cores" CPU baseline may use (run_cpu_baseline)
_NUMA, NUMA_INFO = _bind_numa()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)
HBM_COPY_GBS = 6290.0  # the same guide's measured streaming-copy rate: what a read+write kernel can actually reach


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", type=int, default=10_000_000, help="nodes of the synthetic graph / rows of the table")
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--fanout", type=str, default="5,5")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--cache-mb", type=int, default=4096)
    ap.add_argument("--avg-degree", type=float, default=12.0)
    ap.add_argument("--counts-ahead", dest="counts_ahead", action="store_true", default=True,
                    help="N>1, native exchange, sampler-bucketed ids (the default there): the count exchange of minibatch s+1 is issued (side "
                         "stream) before the fetch of minibatch s, which then runs without its host synchronisation (coala_comm_counts_begin)")
    ap.add_argument("--no-counts-ahead", dest="counts_ahead", action="store_false",
                    help="N>1: every fetch exchanges its own counts and reads them back synchronously (one host wait per minibatch)")
    ap.add_argument("--rounds", type=int, default=0, help="N>1: row-exchange rounds per fetch (1..8); default: measured during the warm-up")
    ap.add_argument("--no-tune-rounds", action="store_true", help="N>1: keep the default number of exchange rounds (2) instead of measuring")
    ap.add_argument("--prewarm", type=int, default=400, help="untimed minibatches that bring the cache to steady state")
    ap.add_argument("--backend", type=str, default=None, help="isolated | nccl | nvshmem (default: isolated at N=1, nccl otherwise)")
    ap.add_argument("--mode", type=str, default="minibatch", choices=["minibatch", "allhit", "allmiss"],
                    help="minibatch: sampler-produced ids (the metric). allhit/allmiss: kernel micro-benchmarks on unique uniform ids")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also run the extra legs (all-hit kernel leg, box blit rate, CPU baselines, epoch, fan-out "
                         "10,10, colour affinity); the --no-* switches below and their sizes apply to them.  Off: the headline line only")
    ap.add_argument("--cpu-baseline-batches", type=int, default=120)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-allhit", action="store_true", help="skip the extra all-hit leg of the probe+gather kernel")
    ap.add_argument("--allhit-launches", type=int, default=100)
    ap.add_argument("--epoch-steps", type=int, default=-1,
                    help="end-to-end leg (loader + GraphSAGE step): -1 = one FULL epoch per mode (measured, not extrapolated), "
                         "k > 0 = k steps extrapolated to an epoch, 0 = skip")
    ap.add_argument("--epoch-prefetch", "--epoch-prefetch-multi", dest="epoch_prefetch", action="store_true", default=False,
                    help="after the default loader's epoch leg also run the leg with COALA_GNN_DataLoader(prefetch=2) (a producer thread).  "
                         "OFF by default.  At N = 1 the two are level (8.9 s either way, profiles/r04_fetch_stream_packets.txt): the default "
                         "loader already keeps fetch and sampler one and two steps ahead on their own streams from ONE host thread, so the "
                         "line reports that one.  At N > 1 the producer thread would issue the exchange's RCCL collectives while the consumer "
                         "thread issues DDP's all-reduce on torch's communicator -- two communicators driven from two host threads with no "
                         "cross-rank launch order, which RCCL documents as a deadlock risk and which has never run on two physical GPUs")
    ap.add_argument("--ddp", action="store_true",
                    help="epoch leg at N > 1: wrap the harness model in torch's DistributedDataParallel (the reference's script does, "
                         "examples/sbatch_ssd_gnn_train.py:112) instead of averaging the gradients with one all-reduce of a flat buffer per step; "
                         "DDP costs this 1.6 ms step another 1.0 ms of host time (profiles/r04_ddp_overhead.txt)")
    ap.add_argument("--epoch-timeout", type=float, default=150.0,
                    help="seconds after which an epoch leg is abandoned (never later than the run's --time-budget): the JSON line is printed "
                         "with an error field and every rank exits with code 3")
    ap.add_argument("--exchange", type=str, default=None, choices=["torch", "native"],
                    help="N>1: the fused native RCCL call (default whenever the cache group is an RCCL group) or the same sequence "
                         "driven from Python over torch.distributed")
    ap.add_argument("--no-color-affinity-leg", action="store_true",
                    help="N=1: skip the extra leg that measures colour-affinity seed routing against baseline striping with two domains on this GPU "
                         "(tools/color_affinity_probe.py, a child process)")
    ap.add_argument("--affinity-nodes", type=int, default=2_000_000,
                    help="N >= 2: nodes of the community graph of the colour-affinity leg (2 domains x N/2 ranks on the ranks of this job); 0 = skip")
    ap.add_argument("--affinity-cache-mb", type=int, default=800, help="N >= 2: cache per DOMAIN in the colour-affinity leg (~10 %% of its table)")
    ap.add_argument("--affinity-steps", type=int, default=300, help="N >= 2: steps per mode in the colour-affinity leg (0 = one epoch)")
    ap.add_argument("--no-fanout-leg", action="store_true", help="skip the extra fan-out 10,10 leg (BASELINE.json configs[2] batch shape)")
    ap.add_argument("--cold-tier", type=str, default="host", choices=["host", "shm", "hbm"],
                    help="host: pinned host memory (hipHostMalloc), zero-copy over PCIe (the workload BASELINE.json names). shm: the "
                         "reference's own kind -- ONE POSIX shm segment per machine, mapped and hipHostRegister'ed by every rank through "
                         "Shared_UVA_Tensor_Manager (shared_UVA.cuh:60-100); whole table, not owner-partitioned. hbm: the whole table "
                         "resident in this GPU's 288 GB HBM (not the headline configuration; MI355X placement data point)")
    ap.add_argument("--shm-attach", type=str, default=None,
                    help="--cold-tier shm: map an EXISTING segment of this name as a non-creator (second mapping of a table another process "
                         "created and filled: tools/shm_two_process_probe.py) instead of creating one")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time-budget", type=float, default=None,
                    help=f"seconds, counted from the start of the launcher: every watchdog deadline is cut off there, and extra legs that would "
                         f"not fit are skipped (default {DEFAULT_BUDGET_S:.0f}, or COALA_BENCH_BUDGET_S): a hang ends with the line + a non-zero code "
                         f"before a driver's 600 s limit")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, rank 0 writes what its last timed step delivered as DIR/<name>.npy (see dump_outputs): "
                         "with the same arguments the inputs are the same from run to run, so two builds can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_LIMIT_BYTES = 64_000_000


def dump_outputs(out_dir, batch, feat, seed=0):
    """What fetch_feature returned in the last timed step, as .npy files under out_dir, DUMP_LIMIT_BYTES at most in all:
    input_nodes and seeds (float64: node ids are exact below 2^53) and features (float32 [rows, dim]).  When the whole feature
    tensor does not fit, a fixed seeded sample of its rows is written instead, in ascending order, and feature_rows (float64)
    holds their positions in the delivered tensor.  -> {name: shape} of the files written."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"input_nodes": batch[0].detach().cpu().numpy().astype(np.float64)}
    if len(batch) > 1 and torch.is_tensor(batch[1]):
        arrays["seeds"] = batch[1].detach().cpu().numpy().astype(np.float64)
    n, dim = feat.shape
    left = DUMP_LIMIT_BYTES - 4096 - sum(a.nbytes for a in arrays.values())   # (4096: room for the files' .npy headers)
    if n * dim * 4 <= left:
        arrays["features"] = feat.detach().cpu().numpy()
    else:
        keep = left // (dim * 4 + 8)     # a sampled row costs its float32 values and its float64 position
        rows = np.sort(np.random.default_rng(seed).choice(n, size=keep, replace=False))
        arrays["features"] = feat[torch.from_numpy(rows).to(feat.device)].cpu().numpy()
        arrays["feature_rows"] = rows.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def _maybe_stall(where, rank):
    """Test hook COALA_BENCH_INJECT_STALL="rank:where": that rank stops making progress at that point (the other ranks then block in
    their next collective): what a first-contact hang of a transport looks like from outside."""
    if os.environ.get("COALA_BENCH_INJECT_STALL", "") == f"{rank}:{where}":
        print(f"[bench] rank {rank}: injected stall at '{where}' (COALA_BENCH_INJECT_STALL)", file=sys.stderr, flush=True)
        while True:
            time.sleep(1.0)


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench] {msg}", file=sys.stderr, flush=True)


class RankGuard(object):
    """Keeps a hang or a rank-local failure VISIBLE.  A rank that fails raises a flag in the torch.distributed store and
    exits non-zero; a monitor thread on every rank polls the flag and a deadline, and when either fires rank 0 prints the JSON
    line (with an "error" field and whatever is finished) and every rank leaves with a non-zero code -- ranks blocked inside a
    collective included.  Nothing is restarted or re-executed: the process just ends, and the launcher reports failure.
    Every deadline is cut off at the run's time budget (counted from the start of the launcher, or of this process when there is
    none): however the legs' individual limits add up, the job has printed its line and left before a driver's own limit."""
    KEY = "coala_bench_failed"

    def __init__(self, rank, world, budget_s=None):
        import threading
        self.rank, self.world = rank, world
        self.line = None          # rank 0: the JSON line as far as it is known
        self.partial = None       # dict of the leg in progress (shown under "epoch" on failure)
        self.deadline, self.what = None, ""
        self.printed = False      # set once rank 0 has printed the finished line
        self.t0 = float(os.environ.get("COALA_BENCH_T0", T_PROCESS_START))
        self.budget_s = float(budget_s if budget_s is not None else _budget_s())
        self.hard_end = self.t0 + self.budget_s
        self.launcher_pid = int(os.environ.get("COALA_BENCH_LAUNCHER_PID", "0"))
        # an OWN client connection to the job's rendezvous store: the default store's client is one socket behind one mutex, and
        # a main thread blocked in it (new_group waiting for a rank that has failed) would block this monitor too
        self.store = None
        self._stop = threading.Event()
        self._failing = False
        self._t = threading.Thread(target=self._watch, daemon=True)   # at N = 1 too: the deadline holds for a single rank as well
        self._t.start()

    def attach_store(self):
        """Once the process group exists (the guard itself is armed before: the rendezvous can hang too)."""
        if self.store is None and self.world > 1 and dist.is_initialized():
            import datetime
            self.store = dist.TCPStore(os.environ.get("MASTER_ADDR", "127.0.0.1"), int(os.environ.get("MASTER_PORT", "29500")),
                                       is_master=False, wait_for_workers=False, timeout=datetime.timedelta(seconds=30))

    def remaining(self):
        """Seconds of the time budget that are left."""
        return self.hard_end - time.time()

    def arm(self, seconds, what):
        self.what = what
        self.deadline = min(time.time() + seconds, self.hard_end)

    def disarm(self):
        self.deadline = None

    def close(self):
        self._stop.set()

    def _leave(self, msg, code):
        if self.printed:          # the line is out and complete: what hangs now is the teardown, not the measurement
            print(f"[bench] rank {self.rank}: {msg} -- after the line was printed; leaving", file=sys.stderr, flush=True)
            os._exit(0)
        if self.rank != 0:
            time.sleep(2.0)       # rank 0 prints the line first: the launcher tears every rank down as soon as one has exited
        if self.rank == 0:
            line = dict(self.line) if self.line is not None else {"metric": "feature-gather GB/s", "value": None, "n_gpus": self.world}
            line["error"] = msg
            if self.partial is not None:
                line["epoch"] = dict(self.partial, error=msg)
            print(json.dumps(line), flush=True)
        print(f"[bench] rank {self.rank}: leaving with code {code}: {msg}", file=sys.stderr, flush=True)
        os._exit(code)

    def _watch(self):
        while not self._stop.wait(0.5):
            if self._failing:
                return            # fail() on the main thread does the leaving
            if self.store is not None:
                try:
                    if self.store.check([self.KEY]):
                        self._leave("a rank failed: " + self.store.get(self.KEY).decode(errors="replace"), 4)
                except Exception:  # noqa: BLE001 -- the store went away with rank 0: nothing left to wait for
                    self._leave("the rendezvous store is gone (rank 0 left)", 4)
            if self.launcher_pid and os.getppid() != self.launcher_pid:
                self._leave("the launcher process is gone", 4)
            if self.deadline is not None and time.time() > self.deadline:
                cut = " (the run's time budget of %.0f s)" % self.budget_s if self.deadline >= self.hard_end - 1e-3 else ""
                self._leave(f"{self.what} abandoned by the watchdog (no completion within its time limit{cut})", 3)

    def fail(self, exc):
        """Called by the rank that caught an exception: tell the others, then leave non-zero."""
        msg = f"rank {self.rank}: {exc!r}"
        self._failing = True
        if self.store is not None and self.rank != 0:
            try:
                self.store.set(self.KEY, msg)
            except Exception:  # noqa: BLE001
                pass
        self._leave(msg, 4)


def main():
    args = parse_args()
    fanout = [int(f) for f in args.fanout.split(",")]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:   # (`python3 bench.py --gpus N` with no WORLD_SIZE never gets here: launch_ranks() above starts the N ranks)
        raise SystemExit(f"WORLD_SIZE={world} does not match --gpus {args.gpus}")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # Test hook for the one-GPU development box: every rank drives GPU 0 and the exchange runs over gloo with host staging
    # (RCCL cannot place two ranks on one device).  Never set by the driver; numbers from such a run are not a measurement.
    single_dev = os.environ.get("COALA_BENCH_SINGLE_DEVICE") == "1"
    dev_index = 0 if single_dev else local_rank
    torch.cuda.set_device(dev_index)
    device = f"cuda:{dev_index}"
    if single_dev:
        os.environ["COALA_CACHE_GROUP_BACKEND"] = "gloo"

    import __graft_entry__ as entry
    bm = entry._load_build_module()
    if local_rank == 0:
        bm.build_lib()          # no-op when the in-tree library is up to date (the usual case: it travels with the snapshot)
    else:                       # the other ranks of the node wait for it instead of loading a missing / stale library
        t_wait = time.time()
        while bm.needs_build() and time.time() - t_wait < 900:
            time.sleep(1.0)
    from COALA_GNN import MPI_Comm_Manager
    from COALA_GNN.COALA_GNN_Manager import COALA_GNN_Manager
    from COALA_GNN.synthetic import PinnedFeatureTable, feature_rows_torch, fill_table, fill_table_partition, powerlaw_csc
    from COALA_GNN.sampler import NeighborSampler

    backend = args.backend or ("isolated" if world == 1 else "nccl")
    # N = 1 with a distributed backend = the dress rehearsal of the multi-GPU run on one GPU: a torch.distributed world of ONE rank with
    # RCCL for GPU tensors (DDP's all-reduce in the epoch leg goes through torch's RCCL communicator), the fused native exchange on its
    # OWN one-rank RCCL communicator, sampler-bucketed ids, the count exchange issued ahead -- every code path of N > 1 except bytes on
    # a link.  (The driver's GPU tests run it: RCCL start-up and the coexistence of the two communicators are exercised on every round.)
    rehearsal = world == 1 and backend in ("nccl", "nvshmem") and not single_dev
    if rehearsal:
        import socket
        if "MASTER_PORT" not in os.environ:
            sk = socket.socket()
            sk.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
            sk.close()
        dist.init_process_group("cpu:gloo,cuda:nccl", rank=0, world_size=1)
        if args.exchange is None:
            args.exchange = "native"
        os.environ["COALA_EXCHANGE"] = args.exchange      # the managers of the later legs (loader, fan-out 10,10) follow
    args.rehearsal = rehearsal
    guard = RankGuard(rank, world, args.time_budget)
    guard.arm(180.0, "process-group set-up")
    comm = MPI_Comm_Manager(0, backend="gloo" if single_dev else None)   # one machine: every rank in domain 0
    comm.device_index = dev_index
    comm.initialize_nested_process_group(backend)
    guard.attach_store()
    guard.arm(300.0, "cold tier + graph set-up")
    try:
        _main_body(args, fanout, world, rank, local_rank, single_dev, dev_index, device, backend, comm, guard)
    except SystemExit:
        raise
    except BaseException as e:  # noqa: BLE001
        if world == 1:
            raise
        import traceback
        traceback.print_exc()
        guard.fail(e)
    finally:
        guard.close()


def _main_body(args, fanout, world, rank, local_rank, single_dev, dev_index, device, backend, comm, guard):
    from COALA_GNN.COALA_GNN_Manager import COALA_GNN_Manager
    from COALA_GNN.synthetic import PinnedFeatureTable, feature_rows_torch, fill_table, fill_table_partition, powerlaw_csc
    from COALA_GNN.sampler import NeighborSampler

    # ---------------------------------------------------------------- cold tier: fp32 [rows, dim] in pinned host memory
    t0 = time.time()
    nbytes = args.rows * args.dim * 4
    cold_partitioned = False
    rows_scale = 1.0
    if args.cold_tier == "hbm":
        class _HbmTable:  # same duck type as PinnedFeatureTable for COALA_GNN_Manager (data_ptr)
            def __init__(self, rows, dim, stride=1, first=0):  # row k holds node id k*stride + first
                self.t = torch.empty((rows, dim), dtype=torch.float32, device=device)
                for lo in range(0, rows, 1 << 20):
                    hi = min(rows, lo + (1 << 20))
                    feature_rows_torch(torch.arange(lo, hi, device=device) * stride + first, dim, args.seed, out=self.t[lo:hi])
                self.array = None

            def data_ptr(self):
                return self.t.data_ptr()

            def close(self):
                self.t = None
        if world > 1 and backend != "isolated":  # every owner keeps its shard of the table in its own HBM
            table = _HbmTable((args.rows + world - 1) // world, args.dim, world, comm.local_rank)
            cold_partitioned = True
            nbytes = ((args.rows + world - 1) // world) * args.dim * 4
        else:
            table = _HbmTable(args.rows, args.dim)
        host_array = None
    elif args.cold_tier == "shm":
        # the reference-API cold tier: what a user following INTEGRATION.md hands to `sim_buf`
        from COALA_GNN import Shared_UVA_Tensor_Manager

        class _ShmTable:
            def __init__(self, rows, dim):
                t_reg = time.perf_counter()
                if args.shm_attach:   # a second mapping of somebody else's segment: the non-creator's path of SharedUVAManager
                    class _Peer:      # (the topology object of a rank that is not local rank 0; no barrier: the creator is long done)
                        node_id, local_rank, device_index = 0, 1, dev_index
                        local_comm = type("C", (), {"Barrier": staticmethod(lambda: None)})()
                    self.mgr = Shared_UVA_Tensor_Manager(_Peer(), args.shm_attach, rows * dim * 4)
                else:
                    self.mgr = Shared_UVA_Tensor_Manager(comm, f"/coala_bench_feat_{os.environ.get('MASTER_PORT', '0')}", rows * dim * 4)
                self.register_s = time.perf_counter() - t_reg
                self.array = self.mgr.get_host_array(np.float32, (rows, dim))
                self.cpu_tensor = torch.from_numpy(self.array)
                self.alias = self.mgr.get_tensor(torch.float32, device, (rows, dim))
                self.device_ptr, self.host_ptr = self.mgr.device_ptr, self.mgr.host_ptr

            def data_ptr(self):
                return self.device_ptr

            def close(self):
                self.alias = self.cpu_tensor = self.array = None
                self.mgr.cleanup()
        table = _ShmTable(args.rows, args.dim)
        log(f"shm segment of {nbytes / 1e9:.2f} GB created/mapped + hipHostRegister'ed in {table.register_s:.2f}s")
        if comm.local_rank == 0 and not args.shm_attach:   # local rank 0 writes the table through its device alias (write_np_array_gpu's way, Shared_Tensor.py:164-179)
            for lo in range(0, args.rows, 1 << 18):
                hi = min(args.rows, lo + (1 << 18))
                feature_rows_torch(torch.arange(lo, hi, dtype=torch.int64, device=device), args.dim, args.seed, out=table.alias[lo:hi])
            torch.cuda.synchronize()
        comm.local_comm.Barrier()
        host_array = table.array
    elif world == 1 or backend == "isolated":
        # the whole table, private to this rank (an isolated cache may read any row).  If the host cannot pin that much
        # memory, the node count is scaled down and the factor reported.
        table = None
        want_rows = args.rows
        while table is None:
            try:
                table = PinnedFeatureTable(args.rows, args.dim, dev_index)
            except RuntimeError as e:
                if args.rows <= 1_000_000:
                    raise
                log(f"pinning {args.rows * args.dim * 4 / 1e9:.1f} GB failed ({e}); halving the node count")
                args.rows //= 2
        rows_scale = args.rows / want_rows
        nbytes = args.rows * args.dim * 4
        fill_table(table.cpu_tensor, args.seed, device=device)
        host_array = table.array
    else:
        # owner-partitioned cold tier: rank r pins only the rows it owns (id % world == r), next to its own PCIe link.
        # (The reference maps ONE shared copy into every GPU: shared_UVA.cuh:42-100, available here as
        # Shared_UVA_Tensor_Manager; an owner of the partitioned cache never reads another owner's rows.)
        local_rows = (args.rows + world - 1) // world
        table = PinnedFeatureTable(local_rows, args.dim, dev_index)
        fill_table_partition(table.cpu_tensor, args.seed, comm.local_rank, world, device=device)
        host_array = None
        cold_partitioned = True
        nbytes = local_rows * args.dim * 4
    sim_ptr_owner = table
    log(f"cold table {nbytes / 1e9:.2f} GB pinned + filled in {time.time() - t0:.1f}s")
    # where this rank's cold tier really is: the node the kernel reports for its first and its middle page (move_pages query), next to
    # the GPU's node and what the binding did
    numa_me = dict(NUMA_INFO)
    hp = getattr(table, "host_ptr", None)
    if hp:
        numa_me["cold_tier_node_first_page"] = _NUMA.node_of_memory(hp)
        numa_me["cold_tier_node_middle_page"] = _NUMA.node_of_memory(hp + nbytes // 2)
    if world > 1:
        numa_all = [None] * world
        dist.all_gather_object(numa_all, numa_me, group=comm.local_gloo_gather)
    else:
        numa_all = [numa_me]

    # ---------------------------------------------------------------- graph + train ids
    t0 = time.time()
    indptr, indices = powerlaw_csc(args.rows, args.avg_degree, seed=args.seed, device=device)
    n_train = int(0.6 * args.rows)                # examples/ssd_gnn_dataloader.py:550-559
    g = torch.Generator().manual_seed(0)
    train_ids = torch.randperm(n_train, generator=g)
    steps_per_epoch = n_train // (args.batch * world) - 1  # COALA_GNN_DataLoader.py:141
    # N>1 over the native exchange: the sampler delivers the input nodes already bucketed by owner, so the fetch needs no routing
    # pass and no un-permute (rows are received in place)
    bucket = world if ((world > 1 or args.rehearsal) and backend != "isolated") else 0
    sampler = NeighborSampler(fanout, seed=args.seed, bucket_by_owner=bucket)
    graph = sampler.make_graph(indptr, indices)
    log(f"graph {args.rows} nodes / {indices.numel()} edges built in {time.time() - t0:.1f}s")

    def make_manager(exchange):
        return COALA_GNN_Manager(node_distributor=None, num_ssds=1, page_size=args.dim * 4, num_elems=1024, ssd_read_offset=0,
                                 cache_size=args.cache_mb, batch_size=args.batch, fan_out=fanout, dim=args.dim,
                                 MPI_comm_manager=comm, device=device, cache_backend=backend, sim_buf=sim_ptr_owner,
                                 num_rows=args.rows, profile=True, cold_partitioned=cold_partitioned, exchange=exchange)

    def first_fetch_is_exact(mgr, smp):
        """One minibatch through the path, compared bit for bit with the table's formula (untimed)."""
        lo = rank * args.batch
        b = smp.sample(graph, train_ids[lo: lo + args.batch].to(device), step=10**9)
        got = mgr.fetch_feature(b)[-1]
        torch.cuda.synchronize()
        return bool(torch.equal(got, feature_rows_torch(b[0], args.dim, args.seed)))

    # Test hook COALA_BENCH_INJECT_EXCHANGE_FAIL="<rank>": that rank reports its first minibatch over the FIRST exchange as wrong (the
    # exchange itself has run, on real objects), so that the fall-back below is executed: every rank drops its manager -- a native
    # exchange's communicator is destroyed -- and continues over the torch transport, and the line says so.
    inject_xfail = os.environ.get("COALA_BENCH_INJECT_EXCHANGE_FAIL", "") == str(rank)
    multi = world > 1 or args.rehearsal        # a one-rank rehearsal walks the same fall-back (its RCCL communicators are real)

    # N>1: the fused native exchange over RCCL has never seen two physical GPUs before the driver's run.  If it raises or delivers a
    # wrong row on ANY rank, every rank falls back to the torch.distributed transport (same sequence, driven from Python) with
    # sampler-order ids, and the line says so.  (A hang cannot be recovered in-process: the RankGuard ends the job non-zero.)
    exchange_note = None
    manager = None
    guard.arm(180.0, "communicator set-up + first minibatch over the exchange")
    _maybe_stall("first_fetch", rank)
    try:
        manager = make_manager(args.exchange)
        ok = first_fetch_is_exact(manager, sampler) if (multi and args.mode == "minibatch") else True
        err = None if ok else "the first minibatch differs from the table"
        if ok and inject_xfail:
            ok, err = False, "injected (COALA_BENCH_INJECT_EXCHANGE_FAIL)"
    except Exception as e:  # noqa: BLE001
        if not multi:
            raise
        ok, err = False, repr(e)
    if multi:
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
        if world > 1:
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=comm.local_gloo_gather)   # a CPU group: usable whatever state RCCL is in
        if int(flag[0]) == 0:
            kind = getattr(manager, "exchange_kind", args.exchange or "native")
            log(f"exchange '{kind}' failed its first-minibatch check on at least one rank ({err}): falling back to the torch transport")
            injected = os.environ.get("COALA_BENCH_INJECT_EXCHANGE_FAIL") is not None
            if kind == "torch" and not injected:
                raise RuntimeError(f"parity self-check failed with the torch transport on rank {rank}: {err}")
            exchange_note = f"torch (fallback: the {kind} exchange failed its first-minibatch check on at least one rank" + (f": {err})" if err else ")")
            if manager is not None and getattr(manager, "exchange", None) is not None and hasattr(manager.exchange, "close"):
                manager.exchange.close()               # a native exchange: its RCCL communicator goes now, not at some later collection
            manager = None
            bucket = 0
            os.environ["COALA_EXCHANGE"] = "torch"     # the managers of the later legs (epoch, fan-out 10,10) follow
            args.exchange = "torch"
            sampler = NeighborSampler(fanout, seed=args.seed)
            manager = make_manager("torch")
            if not first_fetch_is_exact(manager, sampler):
                raise RuntimeError(f"parity self-check failed on rank {rank} with the torch transport as well")
    guard.arm(300.0, "prewarm + timed region")
    cache = manager.COALA_GNN_Cache
    max_rows = manager.max_sample_size
    manager.sync_on_return = False  # stream-ordered fetches: the timed region is bracketed by synchronisations below
    manager.timing_stride = 0       # nobody reads this manager's aggregation timer: no event pair around the fetches (two packets per step on the stream)

    total_steps = args.prewarm + args.warmup + args.steps

    def seeds_for(step):  # rank r takes the r-th batch of the global batch (COALA_GNN_DataLoader.py:72-73)
        lo = ((step % max(steps_per_epoch, 1)) * world + rank) * args.batch
        return train_ids[lo: lo + args.batch].to(device)

    def ids_for(step):  # -> the loader's batch tuple (input_nodes, seeds, blocks); the micro-benchmark modes carry ids only
        if args.mode == "minibatch":
            return sampler.sample(graph, seeds_for(step))
        gen = torch.Generator(device=device).manual_seed(1000 * step + rank if args.mode == "allmiss" else rank)
        return (torch.randperm(args.rows, generator=gen, device=device)[:max_rows],)

    # ---------------------------------------------------------------- untimed: bring the cache to its steady state
    t0 = time.time()
    for s in range(args.prewarm):
        manager.fetch_feature(ids_for(s))
    torch.cuda.synchronize()
    log(f"prewarm {args.prewarm} minibatches in {time.time() - t0:.1f}s")
    # N>1: how many rounds the row exchange is cut into (cold fill of slice k+1 beside the rows of slice k) is decided by
    # measurement on the machine at hand, untimed, on minibatches of their own; every rank ends with the same setting
    rounds_probe = None
    if world > 1 and manager.exchange is not None and hasattr(manager.exchange, "rounds"):
        if args.rounds:
            manager.exchange.rounds = args.rounds
            rounds_probe = {"chosen": args.rounds, "how": "--rounds"}
        elif args.mode == "minibatch" and not args.no_tune_rounds:
            t0 = time.time()
            tune = [ids_for(total_steps + s) for s in range(72)]
            best, probe = manager.tune_exchange_rounds(tune, candidates=(1, 2, 4))
            del tune
            rounds_probe = {"chosen": best, "how": "measured: 24 minibatches per setting in alternating blocks of 8, slowest rank", "ms_per_fetch": probe}
            log(f"exchange rounds: {probe} -> {best} ({time.time() - t0:.1f}s)")
        else:
            rounds_probe = {"chosen": manager.exchange.rounds, "how": "default"}
        os.environ["COALA_EXCHANGE_ROUNDS"] = str(rounds_probe["chosen"])   # the managers of the later legs follow
    batches = [ids_for(args.prewarm + s) for s in range(args.warmup + args.steps)]  # resident in HBM before timing
    torch.cuda.synchronize()

    warm_live = collections.deque(maxlen=3)   # (as in the timed region: three delivered tensors alive, so that its allocator blocks exist before the clock runs)
    for s in range(args.warmup):
        warm_live.append(manager.fetch_feature(batches[s])[-1])
    torch.cuda.synchronize()
    warm_live.clear()
    # parity self-check on every rank, untimed: the rows this path just delivered == the synthetic table's formula, bit for bit.
    # (At N>1 this is the first time the exchange runs over real RCCL links: a wrong row must stop the run, not be timed.)
    # (with --warmup 0 batches[0] is the first TIMED minibatch: checking it here would cache its rows ahead of the clock)
    chk_batch = batches[0] if args.warmup > 0 else ids_for(total_steps + 100)
    chk_ids = chk_batch[0]
    got = manager.fetch_feature(chk_batch)[-1]
    want = feature_rows_torch(chk_ids, args.dim, args.seed)
    if not torch.equal(got, want):
        bad = int((got != want).any(dim=1).sum())
        raise RuntimeError(f"parity self-check failed on rank {rank}: {bad} of {chk_ids.numel()} delivered rows differ from the table")
    del got, want
    torch.cuda.synchronize()
    cache.stats(reset=True)
    cache.profile(reset=True)
    xch = manager.exchange if world > 1 and hasattr(manager.exchange, "reset_profile") else None
    if xch is not None:
        xch.reset_profile()
        xch.profile = True

    ahead = bool(args.counts_ahead and (world > 1 or args.rehearsal) and bucket and hasattr(manager.exchange, "counts_begin") and args.mode == "minibatch")
    if ahead:   # the loaders' pipeline (counts_ahead=True) on pre-sampled minibatches: exchange s+1's counts, then fetch s
        side = torch.cuda.Stream(device=device)

        def counts_for(s):
            blk = batches[s][2][0]
            with torch.cuda.stream(side):
                blk.counts_ticket = manager.exchange.counts_begin(blk.owner_counts.data_ptr())

    # ---------------------------------------------------------------- timed region
    # The interpreter's full (generation-2) garbage collection walks every object torch and numpy have created -- 25-60 ms in this
    # process -- and fires at an allocation count that depends on --steps (it landed inside the timed region for --steps 50 and
    # nowhere else: 1.46 -> 2.7 ms/step).  Collect now and move what exists to the permanent generation, so that a collection
    # inside the region only walks the few objects the region itself creates.
    import gc
    gc.collect()
    gc.freeze()
    gc.disable()   # ... and none at all while the clock runs (re-enabled right behind the region)
    live = collections.deque(maxlen=3)   # the last three delivered tensors stay referenced, as a loader's pipeline holds them (see roofline_allhit)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    rows_done = 0
    if ahead:
        counts_for(args.warmup)
    for s in range(args.warmup, args.warmup + args.steps):
        if ahead and s + 1 < args.warmup + args.steps:
            counts_for(s + 1)
        out = manager.fetch_feature(batches[s])[-1]
        rows_done += out.shape[0]
        live.append(out)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t_start
    gc.enable()
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, batches[args.warmup + args.steps - 1], out, seed=args.seed)
        log(f"last timed step's outputs written to {args.dump_outputs}: {dumped}")
    live.clear()

    hit, miss, bad = cache.stats()
    prof = cache.profile()
    stat = torch.tensor([elapsed, float(rows_done), float(hit), float(miss)], dtype=torch.float64, device=device)
    if world > 1:
        if single_dev:
            stat = stat.cpu()
        tmax = stat.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(stat, op=dist.ReduceOp.SUM)
        elapsed = float(tmax[0])
        rows_all, hit_all, miss_all = float(stat[1]), float(stat[2]), float(stat[3])
    else:
        rows_all, hit_all, miss_all = float(rows_done), float(hit), float(miss)

    # ---------------------------------------------------------------- N>1: the row exchange against the xGMI ceiling
    # achieved_xGMI = remote bytes received / t_exchange per GPU; ceiling 153 GB/s per pair, (N-1) pairs per GPU
    exchange_obj = None
    if xch is not None:
        xch.profile = False
        try:
            ms, calls, remote_rows = xch.fold_profile()
        except Exception as e:  # noqa: BLE001 -- diagnostics must never cost the headline number
            log(f"exchange timing unavailable: {e!r}")
            ms, calls, remote_rows = 0.0, 0, 0
        e = torch.tensor([ms, float(calls), float(remote_rows)], dtype=torch.float64, device="cpu" if single_dev else device)
        e_max = e.clone()
        dist.all_reduce(e_max, op=dist.ReduceOp.MAX)
        dist.all_reduce(e, op=dist.ReduceOp.SUM)
        if float(e[1]) > 0:
            avg_us = float(e[0]) / float(e[1]) * 1e3                       # mean over ranks and steps
            bytes_in = float(e[2]) / float(e[1]) * args.dim * 4            # per GPU per step
            ach = bytes_in / (avg_us * 1e-6) / 1e9 if avg_us > 0 else 0.0
            peak = 153.0 * (world - 1)
            exchange_obj = {"bound": "xgmi", "collective": "all-to-all-v of rows (RCCL)", "avg_us": round(avg_us, 2),
                            "slowest_rank_avg_us": round(float(e_max[0]) / max(float(e_max[1]), 1.0) * 1e3, 2),
                            "remote_bytes_in_per_gpu_per_step": int(bytes_in), "achieved": round(ach, 1), "peak": peak,
                            "unit": "GB/s per GPU ingress", "frac": round(ach / peak, 4),
                            "note": "HIP events around the row exchange on every rank; peak = 153 GB/s per peer link x (N-1) peers"}

    payload_bytes = rows_all * args.dim * 4
    value = payload_bytes / elapsed / 1e9
    ms_per_step = elapsed / args.steps * 1e3

    # ---------------------------------------------------------------- roofline of the probe+gather kernel (rank 0)
    # algorithmic bytes per launch (DESIGN.md "Kernels"): every probed row reads its int64 id and one 32x8 B tag set;
    # every hit additionally reads a dim*4 line and writes a dim*4 output row  (B_row = 2*dim*4+8+256)
    launches = max(prof.gather_launches, 1)
    box_copy = _box_copy_gbs(device) if (rank == 0 and args.full) else None   # how fast THIS box is (boxes differ by up to 10 %): torch's D2D blit, untimed, after the timed region
    tag_set_bytes = int(cache.geometry().tag_set_bytes)   # 128: 32-bit tags (every id < 2^32), 256: the reference's 64-bit tags
    alg_bytes = prof.gather_rows * (8 + tag_set_bytes) + prof.gather_hits * (2 * args.dim * 4)
    k_ms = prof.gather_ms / launches
    achieved = (alg_bytes / launches) / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0
    roofline = {
        "bound": "hbm", "kernel": "probe_gather_kernel", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": _pmc_traffic(args, world)[0], "traffic_source": _pmc_traffic(args, world)[1],
        "frac_of_measured_copy_6290": round(achieved / HBM_COPY_GBS, 4),
        # the same binary differs from box to box (profiles/README.md): the box's own copy rate, measured in this process, beside the guide's constant
        # a box-speed INDICATOR, not a ceiling (a blit of 1 GiB reads + writes 4.6-5.5 TB/s from box to box; a tuned float4 copy kernel 6.2-6.6): no ratio against it
        "box_d2d_blit_gbs": box_copy,
        "avg_launch_us": round(k_ms * 1e3, 2), "timing": "HIP events attached to each launch (hipExtLaunchKernelGGL): kernel begin -> end",
        "separate_event_bracket_would_add_us": round(prof.event_overhead_us, 2),
        "launches": int(prof.gather_launches),
        "rows_per_launch": round(prof.gather_rows / launches, 1), "hits_per_launch": round(prof.gather_hits / launches, 1),
        "alg_bytes_per_launch": int(alg_bytes / launches), "alg_bytes_per_row": f"8 (id) + {tag_set_bytes} (one set of 32 tags) + 2 x {args.dim * 4} per hit",
        "cold_fill_avg_us": round(prof.fill_ms / max(prof.fill_launches, 1) * 1e3, 2),
    }

    # ---------------------------------------------------------------- extra leg (--full, N=1): the hit path alone
    # BASELINE.md section 4 micro-benchmark: N = max rows per minibatch, unique uniform ids, cache pre-warmed with exactly
    # those ids, so every row is a hit and the probe+gather kernel moves B_row = 2*dim*4 + 8 + 256 bytes per row.
    roofline_allhit = None
    if args.full and world == 1 and args.mode == "minibatch" and not args.no_allhit:
        # (a) STEADY STATE: `sets` disjoint id sets, all pre-warmed, fetched in rotation.  One set is max_rows lines + as many output
        #     rows (151 + 151 MB at 36,864 x 4 KiB); by the time a set comes round again the other sets have pushed 4x that through the
        #     256 MiB Infinity Cache, so no launch finds its lines there -- these are HBM reads.  This is `frac`.
        # (b) the same launch on ONE set over and over (what this leg did until round 2): its lines and rows partly survive in the
        #     Infinity Cache from launch to launch -- reported under "mall_warm", not as the roofline figure.
        # (c) an independent check of the timing method: N probe-only launches back to back between ONE pair of ordinary events,
        #     divided by N (no per-launch event, no profiler), beside the same loop over a 1-row batch (the launch cadence itself).
        n_sets = 5 if max_rows * 5 <= args.rows else max(1, args.rows // max_rows)
        gen = torch.Generator(device=device).manual_seed(12345)
        perm = torch.randperm(args.rows, generator=gen, device=device)
        id_sets = [perm[k * max_rows: (k + 1) * max_rows].contiguous() for k in range(n_sets)]
        del perm
        for _ in range(2):
            for ids in id_sets:
                manager.fetch_feature((ids,))
        torch.cuda.synchronize()

        def k1_figures(id_list, launches, live_outputs):
            # live_outputs: how many delivered tensors stay referenced, as a loader's pipeline holds them.  With none kept, torch's allocator hands the
            # SAME block back for every fetch: the 151 MB of rows written by one launch are still in the 256 MiB Infinity Cache when the next one
            # overwrites them, the writes never reach HBM and the kernel reads 0.80 instead of 0.62-0.65 (profiles/r03_k1_old_vs_new.txt)
            ring = collections.deque(maxlen=max(live_outputs, 1))
            cache.stats(reset=True)
            cache.profile(reset=True)
            for k in range(launches):
                o = manager.fetch_feature((id_list[k % len(id_list)],))[-1]
                if live_outputs:
                    ring.append(o)
                del o
            torch.cuda.synchronize()
            ring.clear()
            h2, m2, _ = cache.stats()
            p2 = cache.profile()
            l2 = max(p2.gather_launches, 1)
            b2 = p2.gather_rows * (8 + tag_set_bytes) + p2.gather_hits * (2 * args.dim * 4)
            us2 = p2.gather_ms / l2 * 1e3
            ach2 = (b2 / l2) / (us2 * 1e-6) / 1e9 if us2 > 0 else 0.0
            return {"achieved": round(ach2, 1), "frac": round(ach2 / HBM_PEAK_GBS, 4), "frac_of_measured_copy_6290": round(ach2 / HBM_COPY_GBS, 4),
                    "avg_launch_us": round(us2, 2), "launches": int(p2.gather_launches), "rows_per_launch": round(p2.gather_rows / l2, 1),
                    "hit_ratio": round(h2 / max(h2 + m2, 1), 4), "alg_bytes_per_launch": int(b2 / l2), "no_miss_fill_launch_us": round(p2.fill_ms / max(p2.fill_launches, 1) * 1e3, 2)}
        steady = k1_figures(id_sets, args.allhit_launches, 3)
        warm = k1_figures(id_sets[:1], args.allhit_launches, 0)
        # (c) probe-only launches (coala_cache_serve_probe + serve_abort: K1 alone, the same kernel on the same ids), no events attached
        out_bufs = [torch.empty((max_rows, args.dim), dtype=torch.float32, device=device) for _ in range(3)]   # in rotation, like the delivered tensors above
        one = id_sets[0][:1].contiguous()
        b2b = {}
        try:
            for name, lists, nrow in (("rotating_sets", id_sets, max_rows), ("one_row_batch", [one], 1)):
                for ids in lists:                                         # untimed pass (profiling flag off path is the same kernel)
                    cache.serve_probe(out_bufs[0].data_ptr(), ids.data_ptr(), nrow)
                    cache.serve_abort()
                torch.cuda.synchronize()
                n_b2b = 60
                ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev_a.record()
                for k in range(n_b2b):
                    cache.serve_probe(out_bufs[k % 3].data_ptr(), lists[k % len(lists)].data_ptr(), nrow)
                    cache.serve_abort()
                ev_b.record()
                ev_b.synchronize()
                b2b[name + "_us_per_launch"] = round(ev_a.elapsed_time(ev_b) * 1e3 / n_b2b, 2)
            b2b["launches"] = n_b2b
            b2b["kernel_time_bounds_us"] = [round(b2b["rotating_sets_us_per_launch"] - b2b["one_row_batch_us_per_launch"], 2), b2b["rotating_sets_us_per_launch"]]
            b2b["what"] = ("N probe-only launches back to back between ONE pair of events / N: an upper bound of the kernel's duration (it contains the "
                           "launch-to-launch gap); minus the cadence of the same loop over a 1-row batch: a lower bound.  The attached-event figure "
                           "(avg_launch_us, what `frac` uses) must lie between the two.")
        except Exception as e:  # noqa: BLE001 -- a diagnostic: never costs the line
            b2b = {"error": repr(e)[:200]}
        del out_bufs
        cache.stats(reset=True)
        cache.profile(reset=True)
        roofline_allhit = {"bound": "hbm", "kernel": "probe_gather_kernel", **steady, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "id_sets_in_rotation": n_sets, "bytes_between_two_uses_of_a_set_MB": int((n_sets - 1) * 2 * max_rows * args.dim * 4 / 1e6),
                           "output_tensors_kept_alive": 3,
                           "mall_warm": {**warm, "note": "ONE id set re-fetched back to back into ONE output block (nothing kept alive: the allocator returns the same block): the rows "
                                                         "written by one launch are overwritten in the 256 MiB Infinity Cache by the next -- not an HBM figure; this is what `frac` was until round 3"},
                           "back_to_back_check": b2b,
                           "note": "untimed extra leg: every row a hit (pre-warmed unique uniform ids), steady state over rotating disjoint id sets, the last three output tensors kept alive"}

    # the kernel that dominates the STEP TIME on this workload is the cold fill, bound by the host link, not by HBM
    fill_launches = max(prof.fill_launches, 1)
    fill_us = prof.fill_ms / fill_launches * 1e3
    fill_bytes = prof.fill_rows * args.dim * 4 / fill_launches
    pcie_peak = 63.0  # GB/s, PCIe Gen5 x16 spec (/opt/skills/guides/MI355X_MICROARCH.md "Host link")
    roofline_cold = None
    if args.cold_tier in ("host", "shm") and prof.fill_rows:
        ach = fill_bytes / (fill_us * 1e-6) / 1e9 if fill_us > 0 else 0.0
        roofline_cold = {"bound": "pcie", "kernel": "miss_fill_kernel", "achieved": round(ach, 2), "peak": pcie_peak, "unit": "GB/s",
                         "frac": round(ach / pcie_peak, 4), "avg_launch_us": round(fill_us, 2),
                         "rows_per_launch": round(prof.fill_rows / fill_launches, 1), "alg_bytes_per_launch": int(fill_bytes),
                         "note": "rows read zero-copy from pinned host memory; a pinned hipMemcpy H2D reaches 57.5 GB/s on this box"}

    cpu_baseline = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and host_array is not None:
        cpu_baseline = run_cpu_baseline(args, host_array, [b[0] for b in batches[args.warmup:]], fanout, graph, seeds_for)

    if rank == 0:
        line = {
            "metric": "feature-gather GB/s (payload = rows x dim x 4 B delivered per second), IGB-medium GraphSAGE minibatch fetch",
            "value": round(value, 3), "unit": "GB/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{_shape_name(args.rows, args.dim)} {args.rows}x{args.dim} fp32 cold table in pinned host memory, "
                                   f"GraphSAGE fan-out {args.fanout} bs={args.batch}, {backend} cache {args.cache_mb} MiB/GPU, "
                                   f"mode={args.mode}",
                       "rows_per_step_per_gpu": round(rows_all / world / args.steps, 1),
                       "hit_ratio": round(hit_all / max(hit_all + miss_all, 1.0), 4),
                       "cache_backend": backend, **({"TEST_HOOK_single_device": True} if single_dev else {}),
                       "exchange_transport": (exchange_note or getattr(manager, "exchange_kind", None)) if (world > 1 or args.rehearsal) else None,
                       # what RCCL itself reports for the exchange's communicator (ncclCommCount), not the number it was created with
                       "rccl_ranks": (getattr(manager.exchange, "rccl_ranks", None) or
                                      (dist.get_world_size(comm.nccl_cache_gather) if (not single_dev and comm.nccl_cache_gather is not None) else None))
                       if (world > 1 or args.rehearsal) else None,
                       **({"rccl_rehearsal_one_rank": True} if args.rehearsal else {}),
                       "exchange_rounds": rounds_probe, "counts_ahead": bool(ahead), "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"),
                       "input_nodes": "bucketed by owner by the sampler (no routing pass, rows received in place)" if bucket else "sampler order",
                       "parity_check": "rows of one warm-up minibatch == synthetic table formula, bit-exact, on every rank", "cold_tier": {"hbm": "HBM", "shm": "POSIX shm + hipHostRegister, one segment mapped by every rank (Shared_UVA_Tensor_Manager)" + (": SECOND mapping of a segment another process created" if args.shm_attach else "")}.get(
                           args.cold_tier, "pinned host (hipHostMalloc), owner-partitioned" if cold_partitioned else "pinned host (hipHostMalloc)"),
                       "cold_tier_register_s": round(getattr(table, "register_s", 0.0), 2) or None,
                       "cold_tier_numa_node": [d.get("cold_tier_node_middle_page") for d in numa_all],
                       "numa": [{k: d.get(k) for k in ("mode", "gpu_numa_node", "bound_node", "cpus", "applied", "why") if d.get(k) is not None} for d in numa_all],
                       "prewarm_steps": args.prewarm, "rows_scale_factor": rows_scale, "full": bool(args.full),
                       "steps_per_epoch": steps_per_epoch,
                       "epoch_time_s_fetch_only_extrapolated": round(ms_per_step * steps_per_epoch / 1e3, 2)},
            "roofline": roofline,
            "roofline_allhit": roofline_allhit,
            "roofline_cold_fill": roofline_cold,
            "exchange": exchange_obj,
            "epoch": None,
            "cpu_baseline": cpu_baseline,
        }
    else:
        line = None

    # ---------------------------------------------------------------- extra legs (--full): epoch (end to end), fan-out 10,10, colour affinity
    # They run last and never cost the headline number silently: at N>1 a rank-local exception or a stall ends the whole job
    # with a non-zero exit code, after rank 0 has printed the line with an "error" field (RankGuard).
    guard.line = line

    def leg_fits(name, need_s):
        """An extra leg runs only if what is left of the time budget covers it -- the same decision on every rank; a skipped leg says so."""
        left = guard.remaining()
        ok = left >= need_s
        if world > 1:
            t = torch.tensor([1 if ok else 0], dtype=torch.int32)
            dist.all_reduce(t, op=dist.ReduceOp.MIN, group=comm.local_gloo_gather)
            ok = bool(int(t[0]))
        if not ok:
            log(f"{name} skipped: {left:.0f} s of the {guard.budget_s:.0f} s time budget left, {need_s:.0f} s wanted")
        return ok, {"skipped": f"{left:.0f} s of the run's {guard.budget_s:.0f} s time budget were left, this leg wants {need_s:.0f} s (--time-budget)"}

    _maybe_stall("extra_legs", rank)
    fits, skipped = leg_fits("epoch leg", 75.0) if (args.full and args.mode == "minibatch" and args.epoch_steps != 0) else (False, None)
    if skipped is not None and not fits and rank == 0:
        line["epoch"] = skipped
    if fits:
        partial = {}
        guard.partial = partial
        guard.arm(args.epoch_timeout, "epoch leg")
        epoch = run_epoch_leg(args, comm, graph, sampler, table, device, fanout, steps_per_epoch, backend=backend,
                              cold_partitioned=cold_partitioned, world=world, dev_index=dev_index, single_dev=single_dev,
                              out=partial, guard=guard)
        guard.partial = None
        if rank == 0:
            line["epoch"] = epoch
    # BASELINE.json configs[2] names fan-out 10,10 for the 8-GPU run: a short fetch-only measurement of that batch shape on the
    # same table / graph / cache size, at EVERY N (so that its per-N curve has an origin at N = 1), next to the weak-scaling
    # `value` above, which keeps the N = 1 fan-out so that the driver's per-N values stay comparable
    if args.full and args.mode == "minibatch" and args.fanout == "5,5" and not args.no_fanout_leg:
        fits, skipped = leg_fits("fan-out 10,10 leg", 30.0)
        if fits:
            guard.arm(120.0, "fan-out 10,10 leg")
            skipped = run_fanout_leg(args, comm, graph, table, device, [10, 10], backend, cold_partitioned, world, rank, train_ids,
                                     steps_per_epoch, single_dev)
        if rank == 0:
            line["config_fanout_10_10"] = skipped
    # N=1 only: the reference's distribution comparison (examples/Distribution_compare_script.sh:26-34) on one box -- two domains
    # x 1 rank on this GPU, real colours from the native colouring tool, node_color against baseline.  A child process: a failure
    # there is reported in the object and never costs the line.
    if args.full and world >= 2 and world % 2 == 0 and args.mode == "minibatch" and not args.no_color_affinity_leg and args.affinity_nodes > 0:
        fits, skipped = leg_fits("colour-affinity leg", 70.0)
        if fits:
            guard.arm(120.0, "colour-affinity leg (set-up)")
            skipped = run_color_affinity_domains(args, world, rank, dev_index, device, single_dev, backend, guard)
        if rank == 0:
            line[f"color_affinity_2x{world // 2}"] = skipped
    if args.full and world == 1 and args.mode == "minibatch" and not args.no_color_affinity_leg:
        fits, skipped = leg_fits("colour-affinity leg", 60.0)
        guard.disarm()     # (a child process with a timeout of its own, inside what is left of the budget)
        line["color_affinity"] = run_color_affinity_leg(timeout_s=max(30.0, min(400.0, guard.remaining() - 15.0))) if fits else skipped
    guard.disarm()
    if rank == 0:
        print(json.dumps(line), flush=True)
    guard.printed = True
    if world > 1:
        guard.arm(60.0, "teardown")
        dist.barrier()
    del manager
    if world > 1:
        guard.close()
        comm.destroy_process_group()
    elif args.rehearsal and dist.is_initialized():
        dist.destroy_process_group()


def run_color_affinity_domains(args, world, rank, dev_index, device, single_dev, backend, guard):
    """N >= 2: the reference's distribution comparison (examples/Distribution_compare_script.sh:26-34) ON the ranks of this job: the N
    ranks form 2 domains of K = N/2 ranks (MPI_Comm_Manager(node = rank // K): a domain = the ranks that share one owner-partitioned
    cache, node_distributor_pybind.cuh:150-222 routes every seed of the global batch to the domain whose cache holds most of its colour
    neighbourhood), real colours from the native colouring tool on a graph with planted communities, `node_color` against `baseline`
    over a bounded number of steps from a cold cache each, through the product's loader / distributor / scheduler / sampler / cache.
    Rows of the first steps are checked bit-exact against the table and every global batch must be partitioned exactly, in both
    modes.  -> dict (rank 0), None elsewhere."""
    import tempfile
    from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, SSD_INFO
    from COALA_GNN.color_info_gen import color_graph, save_color_files
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import PinnedFeatureTable, community_csc, feature_rows_torch, fill_table, fill_table_partition
    K = world // 2
    nodes, dim, batch = int(args.affinity_nodes), args.dim, args.batch
    fan = [int(f) for f in args.fanout.split(",")]
    t_leg = time.time()
    comm = MPI_Comm_Manager(rank // K, backend="gloo" if single_dev else None)     # 2 domains x K ranks
    comm.device_index = dev_index
    be = "isolated" if K == 1 else backend                                           # one rank per domain: nothing to partition
    comm.initialize_nested_process_group(be)
    assert (comm.local_size, comm.num_master_process) == (K, 2)
    indptr, indices = community_csc(nodes, args.avg_degree, 2048 if nodes >= 1_000_000 else 512, 0.9, seed=args.seed, device=device)
    n_train = int(0.6 * nodes)
    train_ids = torch.randperm(n_train, generator=torch.Generator().manual_seed(0))
    steps_epoch = n_train // (batch * world) - 1
    steps = min(steps_epoch, int(args.affinity_steps)) if args.affinity_steps > 0 else steps_epoch
    # colours: once, by rank 0 (generate_color_data.py:11-68), handed to the others as the three .npy files the distributor reads
    wg = dist.new_group(backend="gloo")                 # object collectives of this leg: a CPU group whatever the world's device backend is
    tmp = tempfile.mkdtemp(prefix="coala_bench_colors_") if rank == 0 else None
    box = [tmp]
    dist.broadcast_object_list(box, src=0, group=wg)
    tmp = box[0]
    meta = [None]
    if rank == 0:
        t1 = time.time()
        color, tk, sc, ncol, ncolored = color_graph(indptr.cpu().numpy(), indices.cpu().numpy(), np.arange(n_train, dtype=np.int64))
        save_color_files(tmp, color, tk, sc)
        meta = [{"num_colors": int(ncol), "colored_nodes": int(ncolored), "coloring_s": round(time.time() - t1, 2)}]
        del color, tk, sc
    dist.broadcast_object_list(meta, src=0, group=wg)   # (also the barrier behind which the files exist)
    files = [os.path.join(tmp, f) for f in ("color.npy", "topk.npy", "score.npy")]
    cache_mb = max(16, int(args.affinity_cache_mb) // K)    # per rank: a domain holds affinity_cache_mb whatever K is
    if K == 1:
        table = PinnedFeatureTable(nodes, dim, dev_index)
        fill_table(table.cpu_tensor, args.seed, device=device)
    else:                                                # owner-partitioned inside the domain, as the headline run
        table = PinnedFeatureTable((nodes + K - 1) // K, dim, dev_index)
        fill_table_partition(table.cpu_tensor, args.seed, comm.local_rank, K, device=device)
    res = {}
    for mode in ("baseline", "node_color"):
        guard.arm(90.0, f"colour-affinity leg ({mode})")
        nd = Node_Distributor(comm, train_ids, batch, *files, parsing_method=mode)
        smp = NeighborSampler(fan, seed=args.seed, bucket_by_owner=K if K > 1 else 0)   # the same sampler stream in both modes
        g = smp.make_graph(indptr, indices)
        loader = COALA_GNN_DataLoader(SSD_INFO(1, dim * 4, 1024, 0), nd, g, smp, batch, dim, fan, cache_mb, device, cache_backend=be,
                                      sim_buf=table, num_rows=nodes, cold_partitioned=K > 1)
        n_steps, verified, seen = 0, 0, []
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for input_nodes, seeds, blocks, feat in loader:
            if n_steps < 3:
                if not torch.equal(feat, feature_rows_torch(input_nodes, dim, args.seed)):
                    raise RuntimeError(f"colour-affinity leg ({mode}): rank {rank} received rows that differ from the table at step {n_steps}")
                verified += 1
            seen.append(seeds.cpu())
            n_steps += 1
            if n_steps >= steps:
                break
        torch.cuda.synchronize()
        wall = time.perf_counter() - t1
        hit, miss, _ = loader.COALA_GNN_Manager.COALA_GNN_Cache.stats()
        agg = loader.COALA_GNN_Manager.get_aggregate_time()
        loader.close()
        mine = {"domain": comm.master_process_index, "hit": int(hit), "miss": int(miss), "steps": n_steps, "verified": verified,
                "fetch_ms": agg / max(n_steps, 1) * 1e3, "wall_ms": wall / max(n_steps, 1) * 1e3}
        allr = [None] * world
        dist.all_gather_object(allr, mine, group=wg)
        seeds_all = [None] * world
        dist.all_gather_object(seeds_all, torch.cat(seen), group=wg)
        del loader, nd
        if rank == 0:
            union = torch.sort(torch.cat(seeds_all)).values
            want = torch.sort(train_ids[: n_steps * batch * world]).values
            dom = []
            for d in range(2):
                rs = [r for r in allr if r["domain"] == d]
                dom.append({"hit_ratio": round(sum(r["hit"] for r in rs) / max(sum(r["hit"] + r["miss"] for r in rs), 1), 4),
                            "fetch_ms_per_step": round(max(r["fetch_ms"] for r in rs), 4), "ranks": len(rs)})
            res[mode] = {"per_domain": dom, "steps": n_steps,
                         "hit_ratio_all_domains": round(sum(r["hit"] for r in allr) / max(sum(r["hit"] + r["miss"] for r in allr), 1), 4),
                         "rows_bit_exact_steps_per_rank": min(r["verified"] for r in allr),
                         "global_batches_partitioned_exactly": bool(torch.equal(union, want))}
    table.close()
    if rank != 0:
        return None
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    return {"what": f"colour-affinity seed routing vs baseline striping on the ranks of this job: 2 domains x {K} rank(s), "
                    + ("an isolated cache per domain" if K == 1 else f"an owner-partitioned cache over {K} GPUs per domain") +
                    ", each mode from a cold cache, same seeds and sampler stream",
            "graph": "planted communities", "nodes": nodes, "edges": int(indices.numel()), "dim": dim, "cache_mb_per_domain": cache_mb * K,
            "batch": batch, "fanout": args.fanout, **meta[0], **res,
            "hit_ratio_delta": round(res["node_color"]["hit_ratio_all_domains"] - res["baseline"]["hit_ratio_all_domains"], 4),
            "leg_seconds": round(time.time() - t_leg, 1)}


def run_color_affinity_leg(timeout_s=400):
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "tools", "color_affinity_probe.py")]
    t0 = time.time()
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s)
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        if out.returncode != 0 or not lines:
            return {"error": f"probe exited with code {out.returncode}: {out.stderr[-300:]}"}
        d = json.loads(lines[-1])
    except Exception as e:  # noqa: BLE001
        return {"error": repr(e)[:300]}
    keep = ("what", "graph", "nodes", "edges", "dim", "cache_mb_per_domain", "batch", "fanout", "num_colors", "coloring_s",
            "hit_ratio_all_domains", "fetch_ms_per_step_mean", "note")
    res = {k: d.get(k) for k in keep}
    res["steps_per_domain"] = d["baseline"][0]["steps"]
    res["per_domain_hit_ratio"] = {m: [r["hit_ratio"] for r in d[m]] for m in ("baseline", "node_color")}
    res["rows_bit_exact_and_batches_partitioned"] = all(r["rows_verified_bit_exact_steps"] > 0 and r["global_batches_partitioned_exactly"]
                                                        for m in ("baseline", "node_color") for r in d[m])
    res["leg_seconds"] = round(time.time() - t0, 1)
    return res


def run_fanout_leg(args, comm, graph, table, device, fanout, backend, cold_partitioned, world, rank, train_ids, steps_per_epoch,
                   single_dev, prewarm=150, steps=60):
    """Fetch-only rate of the same table / graph / cache size at another fan-out (own cache handle, own sampler)."""
    from COALA_GNN.COALA_GNN_Manager import COALA_GNN_Manager
    from COALA_GNN.sampler import NeighborSampler
    smp = NeighborSampler(fanout, seed=args.seed, bucket_by_owner=world if ((world > 1 or getattr(args, "rehearsal", False)) and backend != "isolated") else 0)
    mgr = COALA_GNN_Manager(node_distributor=None, num_ssds=1, page_size=args.dim * 4, num_elems=1024, ssd_read_offset=0,
                            cache_size=args.cache_mb, batch_size=args.batch, fan_out=fanout, dim=args.dim,
                            MPI_comm_manager=comm, device=device, cache_backend=backend, sim_buf=table, num_rows=args.rows,
                            cold_partitioned=cold_partitioned, exchange=args.exchange)
    mgr.sync_on_return = False
    mgr.timing_stride = 0

    def ids_for(step):
        lo = ((step % max(steps_per_epoch, 1)) * world + rank) * args.batch
        return smp.sample(graph, train_ids[lo: lo + args.batch].to(device))
    for s_ in range(prewarm):
        mgr.fetch_feature(ids_for(s_))
    batches = [ids_for(prewarm + s_) for s_ in range(steps)]
    torch.cuda.synchronize()
    mgr.COALA_GNN_Cache.stats(reset=True)
    import gc
    gc.collect()       # as in the headline region: no full collection of the interpreter while the clock runs
    gc.disable()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = 0
    for b in batches:
        rows += mgr.fetch_feature(b)[-1].shape[0]
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    gc.enable()
    hit, miss, _ = mgr.COALA_GNN_Cache.stats()
    t = torch.tensor([dt, float(rows), float(hit), float(miss)], dtype=torch.float64, device="cpu" if single_dev else device)
    if world > 1:
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        dt = float(tmax[0])
    del mgr
    return {"workload": f"same table and cache, GraphSAGE fan-out {','.join(map(str, fanout))} bs={args.batch} (BASELINE.json configs[2])",
            "value": round(float(t[1]) * args.dim * 4 / dt / 1e9, 3), "unit": "GB/s", "steps": steps, "prewarm_steps": prewarm,
            "ms_per_step": round(dt / steps * 1e3, 4), "rows_per_step_per_gpu": round(float(t[1]) / world / steps, 1),
            "hit_ratio": round(float(t[2]) / max(float(t[2] + t[3]), 1.0), 4)}


def _shape_name(rows, dim):
    return {(10_000_000, 1024): "IGB-medium-shaped", (100_000_000, 1024): "IGB-large-shaped", (111_059_956, 128): "ogbn-papers100M-shaped",
            (2_449_029, 100): "ogbn-products-shaped"}.get((rows, dim), "synthetic")


def _adam(params):
    """Adam in one fused kernel per step where this torch build supports it (the eager foreach path is a dozen launches)."""
    params = list(params)
    try:
        return torch.optim.Adam(params, lr=1e-3, fused=True)
    except (RuntimeError, TypeError, ValueError):
        return torch.optim.Adam(params, lr=1e-3)


def run_epoch_leg(args, comm, graph, sampler, table, device, fanout, steps_per_epoch, backend="isolated", cold_partitioned=False,
                  world=1, dev_index=0, single_dev=False, out=None, guard=None):
    """distribute -> sample -> fetch -> GraphSAGE fwd/bwd/Adam per step, through COALA_GNN_DataLoader: serial (the reference's
    __next__) and with the prefetching producer.  N>1: the same loop on every rank (global batch = batch x N, the partitioned
    cache behind the RCCL exchange, DistributedDataParallel model as in examples/sbatch_ssd_gnn_train.py:112); the time of a
    leg is the MAX over ranks."""
    import tempfile
    from COALA_GNN import COALA_GNN_DataLoader, Node_Distributor, SSD_INFO
    from COALA_GNN.harness import FlatGradAllReduce, SageMean, train_steps
    from COALA_GNN.synthetic import block_colors
    out = {} if out is None else out
    multi_rank = world > 1 or getattr(args, "rehearsal", False)
    out.update({"model": "GraphSAGE 2-layer mean, hidden 128, 19 classes, Adam (torch; out of scope, harness only)"
                         + ((", DistributedDataParallel" if args.ddp else ", data-parallel: gradients averaged with ONE all-reduce of a flat buffer per step "
                             "(--ddp: torch's DistributedDataParallel, +1.0 ms of host time per step)") if multi_rank else ""),
                "per_step": "distribute + sample + fetch_feature + forward/backward/optimizer", "steps_per_epoch": steps_per_epoch,
                "cache_backend": backend})
    # serial first: at N>1 the prefetching loader (exchange and DDP collectives issued from two host threads) only runs behind
    # a serial leg that completed on every rank
    modes = [("serial", 0), ("prefetch", 2)]
    if os.environ.get("COALA_SWITCH_INTERVAL"):  # experiment: GIL hand-off latency between the producer and the consumer thread
        sys.setswitchinterval(float(os.environ["COALA_SWITCH_INTERVAL"]))
    if os.environ.get("COALA_EPOCH_MODES"):
        modes = [m for m in modes if m[0] in os.environ["COALA_EPOCH_MODES"].split(",")]
    if not args.epoch_prefetch:
        modes = modes[:1]
        out["prefetch"] = None
        out["note"] = ("the default loader only: ONE host thread keeps the sampler two steps and the fetch one step ahead on their own streams (and, "
                       "at N > 1, issues the exchange's and DDP's collectives in one order on every rank); --epoch-prefetch adds the "
                       "producer-thread loader, which is level with it at N = 1")
    inject = os.environ.get("COALA_BENCH_INJECT_FAIL", "")  # test hook "rank:leg": that rank raises at the start of that leg

    def across_ranks(secs, nodes):
        if world == 1:
            return secs, nodes
        t = torch.tensor([secs, float(nodes)], dtype=torch.float64, device="cpu" if single_dev else device)
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return float(tmax[0]), int(t[1])

    # the soft time limit's decision is a collective of its own group: the loader's helper threads use the topology's gloo groups concurrently
    limit_group = dist.new_group(backend="gloo") if world > 1 else None
    with tempfile.TemporaryDirectory() as tmp:
        color, tk, sc, _ = block_colors(args.rows, nodes_per_color=4096)
        files = [os.path.join(tmp, f) for f in ("color.npy", "topk.npy", "score.npy")]
        np.save(files[0], color); np.save(files[1], tk); np.save(files[2], sc)
        del color
        n_train = int(0.6 * args.rows)
        epoch_steps = args.epoch_steps
        if world > 1 and epoch_steps < 0 and steps_per_epoch > 1500:
            epoch_steps = 1000  # N = 2: bound the leg (and stay far from the watchdog); N = 4, 8 measure the whole epoch
        full = epoch_steps < 0
        need = n_train if full else (epoch_steps * 2 + 260) * args.batch * world
        train_ids = torch.randperm(n_train, generator=torch.Generator().manual_seed(1))[: min(n_train, need)]
        graph.ndata["labels"] = (torch.arange(args.rows, device=device) * 7) % 19
        # the first GEMM / optimizer calls of a process load their code objects (about 0.4 s on this box): three throw-away training
        # steps on random rows keep that out of whichever leg happens to run first (the cache is not touched)
        warm_model = SageMean(args.dim, 128, 19).to(device)
        warm_opt = _adam(warm_model.parameters())
        warm = []
        for s_ in range(3):
            wb = sampler.sample(graph, train_ids[s_ * args.batch: (s_ + 1) * args.batch].to(device))
            warm.append((*wb, torch.randn(wb[0].numel(), args.dim, device=device)))
        train_steps(warm, warm_model, warm_opt, 3, device)
        del warm, warm_model, warm_opt
        for name, prefetch in modes:
            if guard is not None:
                guard.arm(args.epoch_timeout, f"epoch leg ({name})")
            if inject == f"{comm.global_rank}:{name}":
                raise RuntimeError(f"injected failure on rank {comm.global_rank} in the {name} epoch leg (COALA_BENCH_INJECT_FAIL)")
            nd = Node_Distributor(comm, train_ids, args.batch, *files, parsing_method="baseline")
            loader = COALA_GNN_DataLoader(SSD_INFO(1, args.dim * 4, 1024, 0), nd, graph, sampler, args.batch, args.dim, fanout,
                                          args.cache_mb, device, cache_backend=backend, sim_buf=table, num_rows=args.rows,
                                          prefetch=prefetch, cold_partitioned=cold_partitioned)
            torch.manual_seed(0)  # identical initial weights on every rank
            model = SageMean(args.dim, 128, 19).to(device)
            grad_sync = None
            if (world > 1 or getattr(args, "rehearsal", False)) and os.environ.get("COALA_BENCH_NO_DDP") != "1":   # (the knob of profiles/r04_ddp_overhead.txt: no gradient exchange at all)
                # the development hook (all ranks on one GPU) cannot use RCCL: gradients go through a gloo group there
                pg = dist.new_group(backend="gloo") if single_dev else None
                if args.ddp:
                    model = torch.nn.parallel.DistributedDataParallel(model, device_ids=[dev_index], process_group=pg)
                else:   # one all-reduce of a flat gradient buffer per step (COALA_GNN.harness.FlatGradAllReduce)
                    grad_sync = FlatGradAllReduce(model, group=pg)
            opt = _adam(model.parameters())
            # A leg that is merely SLOW must not end as a watchdog failure: half of what the leg may take at most is a soft limit, checked on
            # the host every 64 steps -- one decision for all ranks (the loop is full of collectives) -- after which the leg stops and says so.
            soft_s = 0.5 * min(args.epoch_timeout, guard.remaining() if guard is not None else args.epoch_timeout)
            if os.environ.get("COALA_BENCH_SOFT_LIMIT_S"):     # test hook: the soft limit alone, without shrinking the watchdog's
                soft_s = float(os.environ["COALA_BENCH_SOFT_LIMIT_S"])
            soft_end = time.time() + soft_s

            def out_of_time():
                late = time.time() > soft_end
                if world > 1:
                    f = torch.tensor([1 if late else 0], dtype=torch.int32)
                    dist.all_reduce(f, op=dist.ReduceOp.MAX, group=limit_group)
                    late = bool(int(f[0]))
                return late
            if full:  # one whole epoch from a cold cache, as the reference's "Epoch Time" of epoch 0
                steps, secs, nodes = train_steps(loader, model, opt, 1 << 60, device, stop_check=out_of_time, grad_sync=grad_sync)
                secs, nodes = across_ranks(secs, nodes)
                ms = secs / max(steps, 1) * 1e3
                if steps < steps_per_epoch - 1:   # the soft limit cut the epoch short: extrapolated, and labelled so
                    out[name] = {"steps": steps, "ms_per_step": round(ms, 3), "epoch_time_s_extrapolated": round(ms * steps_per_epoch / 1e3, 2),
                                 "cut_short": f"stopped after {steps} of {steps_per_epoch} steps at the leg's soft time limit; from a cold cache"}
                    log(f"[{name}] Epoch Time: {ms * steps_per_epoch / 1e3:.2f} (extrapolated: the leg stopped after {steps} steps at its soft time limit)")
                    if prefetch and world > 1:
                        for _ in loader:  # (a producer thread may be collectives ahead of its consumer: run the epoch out)
                            pass
                    else:
                        loader.close()
                    del loader, nd
                    continue
                out[name] = {"steps": steps, "ms_per_step": round(ms, 3), "epoch_time_s_measured": round(secs, 2),
                             "sampled_nodes": int(nodes)}
                log(f"[{name}] Epoch Time: {secs:.2f}   Number of sampled nodes : {nodes}   ({steps} steps, {ms:.3f} ms/step)")
                import contextlib
                with contextlib.redirect_stdout(sys.stderr):  # the reference's per-epoch lines (hit/miss/ratio, Aggregation time)
                    loader.print_stats()
                del loader, nd
                continue
            train_steps(loader, model, opt, 100, device, stop_check=out_of_time, grad_sync=grad_sync)  # warm the cache and the allocator
            steps, secs, nodes = train_steps(loader, model, opt, epoch_steps, device, stop_check=out_of_time, grad_sync=grad_sync)
            secs, nodes = across_ranks(secs, nodes)
            ms = secs / max(steps, 1) * 1e3
            out[name] = {"steps": steps, "ms_per_step": round(ms, 3), "epoch_time_s_extrapolated": round(ms * steps_per_epoch / 1e3, 2),
                         "sampled_nodes_per_step": round(nodes / max(steps, 1), 1)}
            log(f"[{name}] Epoch Time: {ms * steps_per_epoch / 1e3:.2f} (extrapolated from {steps} steps, {ms:.3f} ms/step)")
            if prefetch and world > 1:
                for _ in loader:  # a producer thread may be collectives ahead of its consumer, differently on every rank: run the epoch out
                    pass
            else:
                loader.close()    # the one-thread loader leaves at the same step on every rank: what it has enqueued is symmetric
            del loader, nd
    return out


def _box_copy_gbs(device, mib=1024, reps=10):
    """Read + written GB/s of torch's device-to-device copy of `mib` MiB on THIS box (HIP events): an indicator of how fast the box at hand
    is (the same binary differs by up to 10 % from box to box), NOT a ceiling -- the all-hit gather exceeds it.  None when it cannot be measured."""
    try:
        n = mib << 18
        src = torch.empty(n, dtype=torch.float32, device=device).fill_(1.0)
        dst = torch.empty_like(src)
        for _ in range(2):
            dst.copy_(src)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            dst.copy_(src)
        b.record()
        b.synchronize()
        gbs = 2.0 * n * 4 * reps / (a.elapsed_time(b) * 1e-3) / 1e9
        del src, dst
        return round(gbs, 1)
    except Exception:  # noqa: BLE001
        return None


def _kernel_source_sha16():
    import hashlib
    with open(os.path.join(PKG, "csrc", "coala_cache.hip"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def _pmc_traffic(args, world):
    """(HBM bytes per launch of the probe+gather kernel, where the figure comes from): the committed rocprofv3 PMC passes of THIS
    workload (tools/profile_round.sh -> profiles/pmc_probe_gather.json: separate --pmc FETCH_SIZE / WRITE_SIZE passes, FETCH_SIZE
    x2 as MI355X_MICROARCH.md prescribes for gfx950) -- a constant read from a tracked file, not a live measurement of this run.
    The file records the hash of the kernel source it was measured on: after any change of coala_cache.hip the figure is withheld
    (None, "stale ...") until the passes have been repeated.  (None, None) when the command line is not a profiled workload."""
    key = {(10_000_000, 1024, "5,5", 4096): "default", (111_059_956, 128, "15,10,5", 16384): "papers100m"}.get((args.rows, args.dim, args.fanout, args.cache_mb))
    if key is None or (args.batch, args.mode, world, args.cold_tier) != (1024, "minibatch", 1, "host"):
        return None, None
    path = os.path.join(ROOT, "profiles", "pmc_probe_gather.json")
    try:
        with open(path) as f:
            d = json.load(f).get(key)
        if not d:
            return None, None
        if d.get("kernel_source_sha16") != _kernel_source_sha16():
            return None, f"stale: profiles/pmc_probe_gather.json[{key}] was measured on another version of coala_cache.hip (re-run tools/profile_round.sh)"
        return d.get("hbm_bytes_per_launch"), "profiles/pmc_probe_gather.json <- " + str(d.get("source"))
    except Exception:
        return None, None


class _full_affinity(object):
    """Every thread of this process (OpenMP workers and runtime helpers included) on ALL the CPUs the job was started with, for the
    duration of the block: the NUMA binding done at import keeps a rank on its GPU's socket, and an "all cores" CPU baseline must not
    inherit that handicap.  Restored afterwards, thread by thread."""

    def __enter__(self):
        self.saved = {}
        full = ORIG_AFFINITY or os.sched_getaffinity(0)
        for tid in os.listdir("/proc/self/task"):
            try:
                self.saved[int(tid)] = os.sched_getaffinity(int(tid))
                os.sched_setaffinity(int(tid), full)
            except OSError:
                pass
        return len(full)

    def __exit__(self, *exc):
        for tid, mask in self.saved.items():
            try:
                os.sched_setaffinity(tid, mask)
            except OSError:
                pass
        return False


def _thread_counts(limit):
    return [t for t in (1, 2, 4, 8, 16, 32, 64, 128, 192, 256, 384, 512) if t <= limit] or [1]


def run_cpu_baseline(args, host_array, batches, fanout, graph=None, seeds_for=None):
    """The CPU oracle (oracle/coala_oracle.c: a port, the reference itself cannot be built here) on one host core, over a bounded
    sample of the same minibatches.  Also timed beside it, as BASELINE.md section 5 asks: the CPU gather on many cores -- an OpenMP
    row-memcpy gather (what `feat[input_nodes]` does on a host tensor) and torch.index_select, each with its thread count SWEPT and the
    best one reported -- and the oracle's sampler twin, one core and swept (DGL is not installed).  The all-core legs run with the
    process on every CPU it was started with, not on the NUMA node bench.py binds a rank to."""
    from oracle import oracle as O
    nb = min(args.cpu_baseline_batches, len(batches))
    if nb == 0:
        return None
    idx_host = [b.cpu().numpy() for b in batches[:nb]]
    orc = O.OracleCache(args.cache_mb, args.dim, host_array)
    t0 = time.perf_counter()
    rows = 0
    i = 0
    while time.perf_counter() - t0 < 8.0:  # a bounded ~8 s sample: the same minibatches, cycled
        ids = idx_host[i % nb]
        orc.read_feature(ids, O.SCHED_HITS_FIRST)
        rows += len(ids)
        i += 1
    dt = time.perf_counter() - t0
    orc.close()
    res = {"value": round(rows * args.dim * 4 / dt / 1e9, 3), "unit": "GB/s", "cores": 1, "kind": "port",
           "sample": f"{rows} rows ({i} minibatches of the timed region, cycled) through the C oracle from a cold cache, {dt:.1f}s",
           "host_cpus": os.cpu_count()}
    ms_oracle = dt / max(i, 1) * 1e3
    row_bytes = args.dim * 4
    k = min(nb, 16)
    with _full_affinity() as cpus_all:
        res["all_core_legs_affinity"] = {"cpus": cpus_all, "numa_binding_of_the_rank": {kk: NUMA_INFO.get(kk) for kk in ("applied", "bound_node", "cpus")},
                                         "note": "gather and sampler sweeps below run with every thread of the process on all CPUs of the job; the "
                                                 "table sits on the GPU's NUMA node (hipHostMalloc)"}
        # (torch carries its own libgomp; the oracle links the system's.  A parallel torch op first: with torch's pool never started the oracle's
        #  team degenerates -- 8 threads at 0.25 GB/s instead of 40 on the 8-CPU development container; tools/cpu_gather_probe.py has the box's table)
        (torch.ones(1 << 22) * 2.0).sum().item()
        # ---- OpenMP row-memcpy gather: the thread count swept, best reported; stops once more threads only get slower
        try:
            out = np.empty((max(len(x) for x in idx_host[:k]), args.dim), dtype=np.float32)
            out[...] = 0.0                                  # touched before the clock runs
            sweep = {}
            for th in _thread_counts(cpus_all):
                O.gather_rows_mt(host_array, idx_host[0], out, th)          # team start-up
                t0 = time.perf_counter()
                r2 = 0
                for ids in idx_host[:k]:
                    O.gather_rows_mt(host_array, ids, out, th)
                    r2 += len(ids)
                d2 = time.perf_counter() - t0
                sweep[th] = round(r2 * row_bytes / d2 / 1e9, 3)
                if th >= 8 and sweep[th] < 0.3 * max(sweep.values()):
                    break
            best = max(sweep, key=sweep.get)
            res["gather_openmp_memcpy"] = {"value": sweep[best], "unit": "GB/s", "threads": best, "gbs_by_threads": sweep,
                                           "ms_per_minibatch": round(np.mean([len(x) for x in idx_host[:k]]) * row_bytes / sweep[best] / 1e6, 3),
                                           "what": "oracle/coala_oracle.c orc_gather_rows_mt: out[i] = table[idx[i]], one memcpy per row, rows dealt to "
                                                   "OpenMP threads in blocks of 64; thread count swept, best reported"}
            del out
        except Exception as e:  # noqa: BLE001 -- a baseline leg never costs the line
            res.setdefault("gather_openmp_memcpy", {})["error"] = repr(e)[:200]
        # ---- torch.index_select over the same pinned table, thread count swept the same way
        try:
            t = torch.from_numpy(host_array)
            keep_threads = torch.get_num_threads()
            sweep = {}
            idx_t = [torch.from_numpy(x) for x in idx_host[:k]]
            for th in _thread_counts(cpus_all):
                torch.set_num_threads(th)
                torch.index_select(t, 0, idx_t[0])
                t0 = time.perf_counter()
                r2 = 0
                for ids in idx_t:
                    torch.index_select(t, 0, ids)
                    r2 += len(ids)
                d2 = time.perf_counter() - t0
                sweep[th] = round(r2 * row_bytes / d2 / 1e9, 3)
                if th >= 8 and sweep[th] < 0.5 * max(sweep.values()):
                    break
            torch.set_num_threads(keep_threads)
            best = max(sweep, key=sweep.get)
            res["index_select_all_cores"] = {"value": sweep[best], "unit": "GB/s", "threads": best, "gbs_by_threads": sweep,
                                             "ms_per_minibatch": round(np.mean([len(x) for x in idx_host[:k]]) * row_bytes / sweep[best] / 1e6, 3)}
        except Exception as e:  # noqa: BLE001
            res["index_select_all_cores"] = {"error": str(e)[:100]}
        if graph is not None and seeds_for is not None:  # CPU sampler (the oracle's twin of coala_sampler.hip), one core
            ip, ix = graph.indptr.cpu().numpy(), graph.indices.cpu().numpy()
            ks = 20
            seeds_host = [seeds_for(s).cpu().numpy() for s in range(ks)]
            t0 = time.perf_counter()
            for s in range(ks):
                O.sample_blocks(ip, ix, seeds_host[s], list(reversed(fanout)), args.seed, s)
            res["sampler_twin_one_core_ms_per_minibatch"] = round((time.perf_counter() - t0) / ks * 1e3, 3)
            # ... and on many host cores (OpenMP: the draws over the destination nodes -- the counter-based RNG makes the result independent
            # of the thread count -- and the first-appearance compaction as CAS inserts + a prefix sum).  A minibatch is ~1 ms of work on one
            # core, so waking every core of a big host costs far more than it saves (128 threads: 665 ms per minibatch on the round-3 box):
            # the thread count is swept and the best one is the baseline, with the whole sweep reported.
            sweep = {}
            for th in [t_ for t_ in _thread_counts(cpus_all) if t_ >= 2]:
                O.sample_blocks(ip, ix, seeds_host[0], list(reversed(fanout)), args.seed, 0, threads=th)   # team start-up
                t0 = time.perf_counter()
                for s in range(ks):
                    O.sample_blocks(ip, ix, seeds_host[s], list(reversed(fanout)), args.seed, s, threads=th)
                sweep[th] = round((time.perf_counter() - t0) / ks * 1e3, 3)
                if sweep[th] > 20 * res["sampler_twin_one_core_ms_per_minibatch"]:
                    break                                                     # more threads only get slower from here
            if sweep:
                best = min(sweep, key=sweep.get)
                res["sampler_twin_all_cores"] = {"ms_per_minibatch": sweep[best], "cores": best, "cores_available": cpus_all, "ms_by_threads": sweep,
                                                 "what": "OpenMP: draws over destination nodes per layer, compaction by CAS inserts + prefix sum; same blocks as "
                                                         "one core; thread count swept, best reported"}
    # ... and what the CPU path delivers where the GPU path delivers it, in HBM: the same gather into a pinned staging buffer, then one
    # host-to-device copy per minibatch, one after the other as `feat[input_nodes].to(device)` does (BASELINE.json configs[0];
    # examples/ssd_gnn_dataloader.py: CPU gather, then the copy).  Run on the rank's own NUMA binding (the GPU's socket), not on every CPU of
    # the host: the copy engine reads lines the gather threads have just written, and snooping them out of the OTHER socket's caches halves the
    # copy rate (9 against 19 GB/s delivered, profiles/r04_bench_default.json history).  Thread count swept here too, best reported.
    try:
        if torch.cuda.is_available() and isinstance(res.get("gather_openmp_memcpy"), dict) and "gbs_by_threads" in res["gather_openmp_memcpy"]:
            stage = torch.empty((max(len(x) for x in idx_host[:k]), args.dim), dtype=torch.float32, pin_memory=True)
            stage_np = stage.numpy()
            dev_out = torch.empty_like(stage, device="cuda")
            bound = len(os.sched_getaffinity(0))
            sweep = {}
            for th in [t_ for t_ in (8, 16, 32, 64, 128) if t_ <= bound] or [1]:
                O.gather_rows_mt(host_array, idx_host[0], stage_np, th)
                dev_out.copy_(stage, non_blocking=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r2 = 0
                for ids in idx_host[:k]:
                    O.gather_rows_mt(host_array, ids, stage_np, th)
                    dev_out[: len(ids)].copy_(stage[: len(ids)], non_blocking=True)
                    torch.cuda.synchronize()
                    r2 += len(ids)
                sweep[th] = round(r2 * row_bytes / (time.perf_counter() - t0) / 1e9, 3)
            best = max(sweep, key=sweep.get)
            res["gather_openmp_memcpy"]["delivered_to_hbm"] = {
                "value": sweep[best], "unit": "GB/s", "threads": best, "gbs_by_threads": sweep, "cpus_of_the_binding": bound,
                "ms_per_minibatch": round(np.mean([len(x) for x in idx_host[:k]]) * row_bytes / sweep[best] / 1e6, 3),
                "what": "the same gather into a pinned staging buffer + one H2D copy per minibatch, serially, threads on the GPU's NUMA node: rows in HBM "
                        "per second, the quantity `value` of this line counts"}
            del stage, dev_out
    except Exception as e:  # noqa: BLE001 -- a baseline leg never costs the line
        res.setdefault("gather_openmp_memcpy", {})["delivered_error"] = repr(e)[:200]
    # extrapolated epoch of the CPU path = steps x (best CPU sampler + best CPU gather), no training step
    steps_per_epoch = int(0.6 * args.rows) // args.batch - 1
    gathers = [ms_oracle] + [res[kk]["ms_per_minibatch"] for kk in ("gather_openmp_memcpy", "index_select_all_cores")
                             if isinstance(res.get(kk), dict) and res[kk].get("ms_per_minibatch")]
    h2d = (res.get("gather_openmp_memcpy") or {}).get("delivered_to_hbm")
    if h2d:
        res["epoch_time_s_extrapolated_sampler_plus_gather_plus_h2d"] = None   # filled below
    samplers = [v for v in (res.get("sampler_twin_one_core_ms_per_minibatch"), (res.get("sampler_twin_all_cores") or {}).get("ms_per_minibatch")) if v]
    res["best_cpu_gather_ms_per_minibatch"] = round(min(gathers), 3)
    res["epoch_time_s_extrapolated_sampler_plus_gather"] = round(steps_per_epoch * (min(gathers) + (min(samplers) if samplers else 0.0)) / 1e3, 1)
    if h2d:   # the like-for-like figure: sampled minibatches with their rows IN HBM, which is what the GPU path's epoch leg delivers
        res["epoch_time_s_extrapolated_sampler_plus_gather_plus_h2d"] = round(
            steps_per_epoch * (h2d["ms_per_minibatch"] + (min(samplers) if samplers else 0.0)) / 1e3, 1)
    return res


if __name__ == "__main__":
    main()
