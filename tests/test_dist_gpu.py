"""Owner-partitioned cache on ONE GPU with G logical ranks in one process (loopback exchange): exercises the real route /
serve / scatter kernels and the AllToAllExchange host logic's contract against the oracle's collective step
(orc_dist_fetch: COALA_GNN_Manager.py:143-211, ssd_gnn_cache.cuh:111-174).  The RCCL transport itself is covered by
test_manager_world1_gpu (1-rank RCCL group) and by the gloo world-2 CPU tests."""
import os

import numpy as np
import pytest

from _util import PinnedTable

pytestmark = pytest.mark.gpu


def _loopback_step(torch, caches, idx_list, dim):
    """What G ranks + all-to-all-v do, in one process: route on every rank, concatenate per owner in source-rank order,
    serve, hand the rows back, un-permute."""
    G = len(caches)
    routed = []
    for r in range(G):
        idx = idx_list[r]
        n = idx.numel()
        node = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
        mp = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
        cnt = torch.zeros(G, dtype=torch.int64, device="cuda")
        off = torch.zeros(G + 1, dtype=torch.int64, device="cuda")
        caches[r].route(idx.data_ptr(), n, G, node.data_ptr(), mp.data_ptr(), cnt.data_ptr(), off.data_ptr(), 0)
        routed.append((node, mp, cnt.cpu().tolist(), off.cpu().tolist()))
    outs = [torch.full((idx_list[r].numel(), dim), -3.0, dtype=torch.float32, device="cuda") for r in range(G)]
    recv_rows = [[None] * G for _ in range(G)]
    for o in range(G):
        parts = [routed[s][0][routed[s][3][o]: routed[s][3][o] + routed[s][2][o]] for s in range(G)]
        ids = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device="cuda")
        rows = torch.empty((max(ids.numel(), 1), dim), dtype=torch.float32, device="cuda")
        caches[o].serve(rows.data_ptr(), ids.data_ptr(), ids.numel())
        pos = 0
        for s in range(G):
            recv_rows[s][o] = rows[pos: pos + routed[s][2][o]]
            pos += routed[s][2][o]
    for r in range(G):
        n = idx_list[r].numel()
        if n == 0:
            continue
        packed = torch.cat([recv_rows[r][o] for o in range(G)])
        caches[r].scatter(outs[r].data_ptr(), packed.contiguous().data_ptr(), routed[r][1].data_ptr(), n)
    return outs


@pytest.mark.parametrize("G,dim,cache_mb,cold_part", [(2, 1024, 1, False), (4, 128, 1, False), (3, 100, 1, True), (8, 1024, 2, True),
                                                      (4, 256, 1, True)])
def test_partitioned_cache_matches_oracle(hiplib, oracle, G, dim, cache_mb, cold_part):
    import torch
    P = hiplib
    num_rows = 12000
    feat = oracle.make_features(num_rows, dim, seed=4)
    ctrl = P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, dim, True)
    if cold_part:  # COALA_FLAG_COLD_PARTITIONED: owner r pins only rows r, r+G, r+2G, ...
        shards = [PinnedTable(P, np.ascontiguousarray(feat[r::G])) for r in range(G)]
        caches = [P.SSD_GNN_NVSHMEM_Cache(ctrl, None, r, G, cache_mb, shards[r].device_ptr, num_rows=num_rows, rank=r,
                                          cold_partitioned=True) for r in range(G)]
        table = shards[0]
    else:
        table = PinnedTable(P, feat)
        caches = [P.SSD_GNN_NVSHMEM_Cache(ctrl, None, r, G, cache_mb, table.device_ptr, num_rows=num_rows, rank=r) for r in range(G)]
    orcs = [oracle.OracleCache(cache_mb, dim, feat, n_gpus=G, distributed=True) for _ in range(G)]
    rng = np.random.default_rng(G)
    for step in range(6):
        sizes = [int(rng.integers(0, 3000)) if step else 1500 for _ in range(G)]
        if step == 3:
            sizes[0] = 0  # a rank with an empty batch
        idx_np = [rng.choice(num_rows // 2, size=s, replace=False).astype(np.int64) for s in sizes]
        idx_t = [torch.from_numpy(i).cuda() if len(i) else torch.zeros(0, dtype=torch.int64, device="cuda") for i in idx_np]
        outs = _loopback_step(torch, caches, idx_t, dim)
        want = oracle.dist_fetch(orcs, idx_np, oracle.SCHED_HITS_FIRST)
        for r in range(G):
            assert outs[r].cpu().numpy().tobytes() == feat[idx_np[r]].tobytes() == want[r].tobytes()
            assert caches[r].stats()[:2] == (orcs[r].hit_cnt, orcs[r].miss_cnt), f"owner {r} counters differ at step {step}"
            keys, cnt, _ = caches[r].dump()
            assert np.array_equal(keys, orcs[r].keys()) and np.array_equal(cnt, orcs[r].set_cnt())
            # an owner only ever caches ids it owns
            live = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
            assert np.all(live % np.uint64(G) == np.uint64(r))
    assert sum(o.hit_cnt for o in orcs) > 0
    for c in caches:
        c.close()
    table.close()


def _loopback_step_split(torch, caches, idx_list, dim, rounds):
    """The split-phase sequence of coala_comm.cpp / AllToAllExchange with G logical ranks in one process: route, concatenate per
    owner, probe with the owner's OWN segment redirected into the requester's tensor, then per round {fill slice k of every
    peer's segment, hand slice k over}, un-permute per round.  A row leaves the owner only in the round that filled it."""
    G = len(caches)
    routed = []
    for r in range(G):
        idx = idx_list[r]
        n = idx.numel()
        node = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
        mp = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
        cnt = torch.zeros(G, dtype=torch.int64, device="cuda")
        off = torch.zeros(G + 1, dtype=torch.int64, device="cuda")
        caches[r].route(idx.data_ptr(), n, G, node.data_ptr(), mp.data_ptr(), cnt.data_ptr(), off.data_ptr(), 0)
        routed.append((node, mp, cnt.cpu().tolist(), off.cpu().tolist()))
    outs = [torch.full((max(idx_list[r].numel(), 1), dim), -3.0, dtype=torch.float32, device="cuda") for r in range(G)]
    rows_recv = [torch.full((max(idx_list[r].numel(), 1), dim), -5.0, dtype=torch.float32, device="cuda") for r in range(G)]
    owners = []
    for o in range(G):
        rc = [routed[s][2][o] for s in range(G)]
        rd = [sum(rc[:s]) for s in range(G)]
        ids = torch.cat([routed[s][0][routed[s][3][o]: routed[s][3][o] + rc[s]] for s in range(G)])
        tot = ids.numel()
        rows = torch.full((max(tot, 1), dim), -7.0, dtype=torch.float32, device="cuda")
        if tot:
            caches[o].serve_probe_redirect(rows.data_ptr(), ids.data_ptr(), tot, rd[o], rd[o] + rc[o], outs[o].data_ptr(),
                                           routed[o][1].data_ptr() + routed[o][3][o] * 8)
        owners.append((rc, rd, ids, tot, rows))
    for k in range(rounds):
        for o in range(G):
            rc, rd, ids, tot, rows = owners[o]
            rng = [(rd[s] + rc[s] * k // rounds, rd[s] + rc[s] * (k + 1) // rounds) for s in range(G) if s != o]
            if k == rounds - 1:
                rng.append((rd[o], rd[o] + rc[o]))
            if tot:
                caches[o].serve_fill_ranges(rows.data_ptr(), ids.data_ptr(), tot, rng)
        for r in range(G):                                    # "exchange" of round k + un-permute of what arrived
            sc, sd = routed[r][2], routed[r][3]
            land = []
            for o in range(G):
                if o == r:
                    continue
                rc, rd, _, _, rows = owners[o]
                a, b = rc[r] * k // rounds, rc[r] * (k + 1) // rounds
                assert sc[o] == rc[r]
                rows_recv[r][sd[o] + a: sd[o] + b] = rows[rd[r] + a: rd[r] + b]
                land.append((sd[o] + a, sd[o] + b))
            caches[r].scatter_ranges(outs[r].data_ptr(), rows_recv[r].data_ptr(), routed[r][1].data_ptr(), land)
    return [outs[r][: idx_list[r].numel()] for r in range(G)]


def _dist_fixture(P, oracle, G, dim, cache_mb, cold_part, num_rows, seed, cls="SSD_GNN_NVSHMEM_Cache"):
    feat = oracle.make_features(num_rows, dim, seed=seed)
    ctrl = P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, dim, True)
    if cold_part:
        tables = [PinnedTable(P, np.ascontiguousarray(feat[r::G])) for r in range(G)]
    else:
        tables = [PinnedTable(P, feat)] * G
    caches = [getattr(P, cls)(ctrl, None, r, G, cache_mb, tables[r].device_ptr, num_rows=num_rows, rank=r, cold_partitioned=cold_part)
              for r in range(G)]
    orcs = [oracle.OracleCache(cache_mb, dim, feat, n_gpus=G, distributed=True) for _ in range(G)]
    return feat, tables, caches, orcs


@pytest.mark.parametrize("G,dim,cache_mb,cold_part,rounds", [(2, 1024, 1, False, 2), (4, 128, 1, False, 3), (3, 100, 1, True, 2),
                                                             (8, 1024, 2, True, 2), (4, 256, 1, True, 1), (2, 512, 1, False, 4)])
def test_split_phase_partitioned_cache_matches_oracle(hiplib, oracle, G, dim, cache_mb, cold_part, rounds):
    """Own-shard bypass + fills in rounds + un-permute in rounds == the one-serve path == orc_dist_fetch, bit for bit
    (rows, hit/miss counters, tag table, round-robin cursors)."""
    import torch
    num_rows = 12000
    feat, tables, caches, orcs = _dist_fixture(hiplib, oracle, G, dim, cache_mb, cold_part, num_rows, seed=4)
    rng = np.random.default_rng(G + 10 * rounds)
    for step in range(6):
        sizes = [int(rng.integers(0, 3000)) if step else 1500 for _ in range(G)]
        if step == 3:
            sizes[0] = 0  # a rank with an empty batch
        if step == 4:
            sizes = [s if r == 1 else 0 for r, s in enumerate(sizes)]  # one requester only: owners serve, most receive nothing
        idx_np = [rng.choice(num_rows // 2, size=s, replace=step == 5).astype(np.int64) for s in sizes]  # last step: duplicates
        idx_t = [torch.from_numpy(i).cuda() if len(i) else torch.zeros(0, dtype=torch.int64, device="cuda") for i in idx_np]
        outs = _loopback_step_split(torch, caches, idx_t, dim, rounds)
        want = oracle.dist_fetch(orcs, idx_np, oracle.SCHED_HITS_FIRST)
        for r in range(G):
            assert outs[r].cpu().numpy().tobytes() == feat[idx_np[r]].tobytes() == want[r].tobytes(), f"rank {r} step {step}"
            assert caches[r].stats()[:2] == (orcs[r].hit_cnt, orcs[r].miss_cnt), f"owner {r} counters differ at step {step}"
            keys, cnt, _ = caches[r].dump()
            assert np.array_equal(keys, orcs[r].keys()) and np.array_equal(cnt, orcs[r].set_cnt())
    assert sum(o.hit_cnt for o in orcs) > 0
    for c in caches:
        c.close()
    for t in set(tables):
        t.close()


@pytest.mark.parametrize("G,dim,cache_mb,cold_part,rounds", [(2, 1024, 1, False, 2), (3, 100, 1, True, 2), (4, 256, 1, True, 3),
                                                             (8, 1024, 2, True, 2), (4, 128, 1, False, 1)])
def test_native_fetch_inproc_ranks_match_oracle(hiplib, oracle, G, dim, cache_mb, cold_part, rounds):
    """coala_cache_fetch_distributed itself -- the fused native call the product uses at N > 1 -- with G ranks as G host
    threads of this process on one GPU (in-process transport instead of RCCL, same orchestration: two streams, rounds,
    own-shard bypass), against orc_dist_fetch: rows, owner counters, tag tables, cursors, per-peer counts."""
    import ctypes as C
    import threading
    import torch
    from COALA_GNN.COALA_GNN_Manager import NativeExchange
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    num_rows, steps = 12000, 6
    feat, tables, caches, orcs = _dist_fixture(hiplib, oracle, G, dim, cache_mb, cold_part, num_rows, seed=6, cls="Isolated_Cache")
    group = C.c_void_p()
    _capi.check(L.coala_comm_group_create(G, C.byref(group)))
    exs = [NativeExchange(None, 0, r, G, 0, inproc_group=group, rounds=rounds) for r in range(G)]
    rng = np.random.default_rng(77 + G + 1000 * int(os.environ.get("COALA_TEST_SEED", "0")))   # COALA_TEST_SEED: soak runs over other plans
    plan = []
    for step in range(steps):
        sizes = [int(rng.integers(0, 3000)) if step else 1500 for _ in range(G)]
        if step == 2:
            sizes[G - 1] = 0
        if step == 4:
            sizes = [s if r == 0 else 0 for r, s in enumerate(sizes)]
        plan.append([rng.choice(num_rows // 2, size=s, replace=step == 5).astype(np.int64) for s in sizes])
    got = [[None] * G for _ in range(steps)]
    stats = [[None] * G for _ in range(steps)]
    counts = [[None] * G for _ in range(steps)]
    errors = []
    bar = threading.Barrier(G, timeout=180)

    def worker(r):
        try:
            torch.cuda.set_device(0)
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for step in range(steps):
                    ids = plan[step][r]
                    idx = torch.from_numpy(ids).cuda() if len(ids) else torch.zeros(0, dtype=torch.int64, device="cuda")
                    out = torch.full((max(len(ids), 1), dim), -9.0, dtype=torch.float32, device="cuda")
                    exs[r].fetch(caches[r], out.data_ptr() if len(ids) else 0, idx.data_ptr() if len(ids) else 0, len(ids))
                    stream.synchronize()
                    got[step][r] = out[: len(ids)].cpu().numpy()
                    counts[step][r] = (list(exs[r].last_send_counts), list(exs[r].last_recv_counts))
                    bar.wait()                      # every owner has finished serving this step
                    stats[step][r] = caches[r].stats()
                    bar.wait()
        except BaseException as e:  # noqa: BLE001
            errors.append((r, repr(e)))
            bar.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    for step in range(steps):
        want = oracle.dist_fetch(orcs, plan[step], oracle.SCHED_HITS_FIRST)
        for r in range(G):
            assert got[step][r].tobytes() == feat[plan[step][r]].tobytes() == want[r].tobytes(), f"rank {r} step {step}: rows differ"
            assert stats[step][r][:2] == (orcs[r].hit_cnt, orcs[r].miss_cnt), f"owner {r} counters differ at step {step}"
            send, recv = counts[step][r]
            assert send == [int((plan[step][r] % G == o).sum()) for o in range(G)]
            assert recv == [int((plan[step][s] % G == r).sum()) for s in range(G)]
    for r in range(G):
        keys, cnt, _ = caches[r].dump()
        assert np.array_equal(keys, orcs[r].keys()) and np.array_equal(cnt, orcs[r].set_cnt())
    assert sum(o.hit_cnt for o in orcs) > 0
    for e in exs:
        e.close()
    _capi.check(L.coala_comm_group_destroy(group))
    for c in caches:
        c.close()
    for t in set(tables):
        t.close()


@pytest.mark.parametrize("G,dim,rounds,ahead", [(2, 256, 2, False), (4, 1024, 2, False), (8, 128, 3, False), (3, 512, 2, True), (8, 1024, 4, True)])
def test_native_bucketed_fetch_from_sampler_output(hiplib, oracle, G, dim, rounds, ahead):
    """f-1 end to end: NeighborSampler(bucket_by_owner=G) -> coala_cache_fetch_distributed_bucketed on G in-process ranks (no routing
    pass, rows received in place, own bucket gathered in place): delivered rows, owner counters and tag tables == orc_dist_fetch
    fed with the same (bucketed) id lists.  ahead = True: the count exchange of step t+1 is issued (on a second stream, behind the
    sampler) BEFORE the fetch of step t, which then runs without a host synchronisation (coala_comm_counts_begin / _ahead)."""
    import ctypes as C
    import threading
    import torch
    from COALA_GNN.COALA_GNN_Manager import NativeExchange
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import powerlaw_csc
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    num_rows, steps = 20000, 4
    feat, tables, caches, orcs = _dist_fixture(hiplib, oracle, G, dim, 2, True, num_rows, seed=8, cls="Isolated_Cache")
    indptr, indices = powerlaw_csc(num_rows, 10.0, seed=4, device="cuda")
    group = C.c_void_p()
    _capi.check(L.coala_comm_group_create(G, C.byref(group)))
    exs = [NativeExchange(None, 0, r, G, 0, inproc_group=group, rounds=rounds) for r in range(G)]
    samplers = [NeighborSampler([5, 5], seed=r, bucket_by_owner=G) for r in range(G)]
    graphs = [s.make_graph(indptr, indices) for s in samplers]
    got = [[None] * G for _ in range(steps)]
    ids_seen = [[None] * G for _ in range(steps)]
    errors = []
    bar = threading.Barrier(G, timeout=180)

    def worker(r):
        try:
            torch.cuda.set_device(0)
            stream = torch.cuda.Stream()
            side = torch.cuda.Stream()

            def sample(step):
                seeds = torch.randperm(num_rows, generator=torch.Generator().manual_seed(100 * step + r))[:64].cuda()
                if not ahead:
                    return samplers[r].sample(graphs[r], seeds), None
                with torch.cuda.stream(side):   # sampler + count exchange on their own stream, ahead of the fetch that uses them
                    smp = samplers[r].sample(graphs[r], seeds)
                    ticket = exs[r].counts_begin(smp[2][0].owner_counts.data_ptr())
                    ev = torch.cuda.Event()
                    ev.record()
                torch.cuda.current_stream().wait_event(ev)
                return smp, ticket

            with torch.cuda.stream(stream):
                nxt = sample(0)
                for step in range(steps):
                    (input_nodes, _, blocks), ticket = nxt
                    if step + 1 < steps:
                        nxt = sample(step + 1)          # ahead: its count exchange goes out before this step's fetch
                    n = input_nodes.numel()
                    out = torch.full((n, dim), -9.0, dtype=torch.float32, device="cuda")
                    exs[r].fetch_bucketed(caches[r], out.data_ptr(), input_nodes.data_ptr(), n, blocks[0].owner_counts.data_ptr(), ticket=ticket)
                    stream.synchronize()
                    got[step][r] = out.cpu().numpy()
                    ids_seen[step][r] = input_nodes.cpu().numpy()
                    assert exs[r].last_send_counts == blocks[0].owner_counts_host
                    bar.wait()
        except BaseException as e:  # noqa: BLE001
            errors.append((r, repr(e)))
            bar.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    for step in range(steps):
        want = oracle.dist_fetch(orcs, ids_seen[step], oracle.SCHED_HITS_FIRST)
        for r in range(G):
            assert got[step][r].tobytes() == feat[ids_seen[step][r]].tobytes() == want[r].tobytes(), f"rank {r} step {step}"
    for r in range(G):
        assert caches[r].stats()[:2] == (orcs[r].hit_cnt, orcs[r].miss_cnt)
        keys, cnt, _ = caches[r].dump()
        assert np.array_equal(keys, orcs[r].keys()) and np.array_equal(cnt, orcs[r].set_cnt())
    for e in exs:
        e.close()
    _capi.check(L.coala_comm_group_destroy(group))
    for x in graphs:
        x.close()
    for c in caches:
        c.close()
    for t in set(tables):
        t.close()


def test_fill_and_scatter_over_many_ranges(hiplib, oracle):
    """More ranges than one kernel launch carries (64): serve_fill_ranges / scatter_ranges split them over several launches; rows,
    counters and table still equal one serve / one scatter."""
    import torch
    P = hiplib
    dim, num_rows, n = 128, 30000, 6000
    feat = oracle.make_features(num_rows, dim, seed=5)
    table = PinnedTable(P, feat)
    ctrl = P.SSD_GNN_SSD_Controllers(1, 512, 1024, 0, 0, dim, True)
    a = P.SSD_GNN_NVSHMEM_Cache(ctrl, None, 0, 1, 1, table.device_ptr, num_rows=num_rows, rank=0)
    b = P.SSD_GNN_NVSHMEM_Cache(ctrl, None, 0, 1, 1, table.device_ptr, num_rows=num_rows, rank=0)
    rng = np.random.default_rng(9)
    for step in range(3):
        ids = rng.choice(num_rows, size=n, replace=False).astype(np.int64)
        d_ids = torch.from_numpy(ids).cuda()
        out_a = torch.full((n, dim), -1.0, device="cuda")
        out_b = torch.full((n, dim), -1.0, device="cuda")
        a.serve(out_a.data_ptr(), d_ids.data_ptr(), n)
        cuts = sorted({0, n, *(int(c) for c in rng.integers(1, n, size=170))})
        ranges = list(zip(cuts[:-1], cuts[1:]))
        assert len(ranges) > 128
        rng.shuffle(ranges)
        b.serve_probe(out_b.data_ptr(), d_ids.data_ptr(), n)
        b.serve_fill_ranges(out_b.data_ptr(), d_ids.data_ptr(), n, ranges[:100])
        b.serve_fill_ranges(out_b.data_ptr(), d_ids.data_ptr(), n, ranges[100:])
        torch.cuda.synchronize()
        assert torch.equal(out_a, out_b) and out_b.cpu().numpy().tobytes() == feat[ids].tobytes()
        assert a.stats() == b.stats()
        for x, y in zip(a.dump(), b.dump()):
            assert np.array_equal(x, y)
        # un-permute through 171 ranges == one scatter
        perm = torch.randperm(n, device="cuda")
        dst1 = torch.zeros((n, dim), device="cuda")
        dst2 = torch.zeros((n, dim), device="cuda")
        a.scatter(dst1.data_ptr(), out_a.data_ptr(), perm.data_ptr(), n)
        a.scatter_ranges(dst2.data_ptr(), out_a.data_ptr(), perm.data_ptr(), ranges)
        torch.cuda.synchronize()
        assert torch.equal(dst1, dst2) and torch.equal(dst1[perm], out_a)
    a.close(); b.close()
    table.close()


def test_open_batch_is_guarded(hiplib, oracle):
    """a probe while a probed batch still waits for fills, a fill that overlaps an earlier one, or a fill for another
    batch size must be refused (stale verdicts would corrupt the next batch); serve_abort drops the open batch."""
    import torch
    P = hiplib
    dim, num_rows, n = 128, 4000, 600
    feat = oracle.make_features(num_rows, dim, seed=3)
    table = PinnedTable(P, feat)
    ctrl = P.SSD_GNN_SSD_Controllers(1, 512, 1024, 0, 0, dim, True)
    c = P.SSD_GNN_NVSHMEM_Cache(ctrl, None, 0, 1, 1, table.device_ptr, num_rows=num_rows, rank=0)
    orc = oracle.OracleCache(1, dim, feat, n_gpus=1, distributed=True)
    ids = np.random.default_rng(0).choice(num_rows, size=n, replace=False).astype(np.int64)
    d_ids = torch.from_numpy(ids).cuda()
    out = torch.full((n, dim), -1.0, device="cuda")
    c.serve_probe(out.data_ptr(), d_ids.data_ptr(), n)
    for bad in (lambda: c.serve_probe(out.data_ptr(), d_ids.data_ptr(), n), lambda: c.serve(out.data_ptr(), d_ids.data_ptr(), n),
                lambda: c._read(out.data_ptr(), d_ids.data_ptr(), n)):
        with pytest.raises(RuntimeError, match="still open"):
            bad()
    c.serve_fill(out.data_ptr(), d_ids.data_ptr(), n, 0, 200)
    with pytest.raises(RuntimeError, match="overlaps"):
        c.serve_fill(out.data_ptr(), d_ids.data_ptr(), n, 100, 300)
    with pytest.raises(RuntimeError, match="overlaps"):
        c.serve_fill_ranges(out.data_ptr(), d_ids.data_ptr(), n, [(300, 400), (350, 360)])
    with pytest.raises(RuntimeError, match="outside"):
        c.serve_fill(out.data_ptr(), d_ids.data_ptr(), n, 500, n + 1)
    c.serve_fill_ranges(out.data_ptr(), d_ids.data_ptr(), n, [(400, n), (200, 400)])   # coverage complete: the batch closes
    orc.read_feature(ids, oracle.SCHED_HITS_FIRST, want_rows=False)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == feat[ids].tobytes()
    with pytest.raises(RuntimeError, match="without a matching"):
        c.serve_fill(out.data_ptr(), d_ids.data_ptr(), n, 0, 1)
    # abort: the next batch starts clean (no stale verdicts), the aborted batch's misses stay uncached
    ids2 = np.random.default_rng(1).choice(num_rows, size=n, replace=False).astype(np.int64)
    d2 = torch.from_numpy(ids2).cuda()
    c.serve_probe(out.data_ptr(), d2.data_ptr(), n)
    c.serve_abort()
    c.serve(out.data_ptr(), d_ids.data_ptr(), n)               # the first batch again: every row a hit, nothing stale
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == feat[ids].tobytes()
    c.close()
    table.close()


@pytest.mark.parametrize("backend,exchange", [("isolated", None), ("nccl", "torch"), ("nvshmem", "torch"), ("nccl", "native"),
                                              ("nvshmem", "native")])
def test_manager_world1_gpu(hiplib, oracle, backend, exchange):
    """COALA_GNN_Manager.fetch_feature on one rank for every backend string: G = 1 degenerates to the isolated cache
    (SURVEY.md section 8e); the nccl/nvshmem flavours still run route -> exchange -> serve -> scatter."""
    import torch
    from COALA_GNN import MPI_Comm_Manager
    from COALA_GNN.COALA_GNN_Manager import COALA_GNN_Manager
    from COALA_GNN.synthetic import alloc_pinned_table
    dim, rows = 256, 30000
    table = alloc_pinned_table(rows, dim, seed=2, device=0)
    feat = oracle.make_features(rows, dim, seed=2)
    comm = MPI_Comm_Manager(0)
    comm.initialize_nested_process_group(backend)
    mgr = COALA_GNN_Manager(None, 1, dim * 4, 1024, 0, 8, 64, [5, 5], dim, comm, "cuda:0", cache_backend=backend,
                            sim_buf=table, num_rows=rows, exchange=exchange)
    assert mgr.max_sample_size == 64 * 36
    if exchange == "native":  # a real RCCL communicator of one rank: ncclAllToAll / ncclAllToAllv to self
        assert type(mgr.exchange).__name__ == "NativeExchange"
    orc = oracle.OracleCache(8, dim, feat, n_gpus=1, distributed=backend != "isolated")
    rng = np.random.default_rng(1)
    for step in range(5):
        idx = rng.choice(rows // 3, size=2000, replace=False).astype(np.int64)
        t_idx = torch.from_numpy(idx).cuda()
        batch = mgr.fetch_feature((t_idx, None, None))
        assert batch[0] is t_idx and len(batch) == 4
        got = batch[-1]
        assert got.shape == (2000, dim) and got.dtype == torch.float32
        want = orc.read_feature(idx, oracle.SCHED_HITS_FIRST)
        assert got.cpu().numpy().tobytes() == want.tobytes()
        assert mgr.COALA_GNN_Cache.stats()[:2] == (orc.hit_cnt, orc.miss_cnt)
        if mgr.exchange is not None:
            assert mgr.exchange.last_send_counts == [2000] and mgr.exchange.last_recv_counts == [2000]
    assert mgr.get_aggregate_time() > 0
    del mgr
    table.close()


@pytest.mark.parametrize("world,backend", [(2, "nccl"), (3, "nvshmem")])
def test_partitioned_path_multi_process_one_gpu(world, backend):
    """Real processes, real HIP kernels, owner-partitioned cold tier; transport = gloo with host staging (tests/_dist_gpu_worker.py)."""
    import os
    import socket
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(here, "_dist_gpu_worker.py"), backend], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for r, p in enumerate(procs):
        out, _ = p.communicate(timeout=400)
        assert p.returncode == 0 and f"rank {r} ok" in out, out[-3000:]


def test_reference_call_sequence_nccl_helpers(hiplib, oracle):
    """The reference's own "nccl" orchestration (COALA_GNN_Manager.py:143-211) replayed with its argument conventions on G
    logical ranks: split_node_list into [G][max_sample] buffers, nccl_get_feature over per-peer id / row buffers,
    map_feat_data with the [G][max_sample] meta buffer.  Exercises the pybind-mirror methods themselves."""
    import torch
    P = hiplib
    G, dim, num_rows, cache_mb, max_sample = 3, 128, 9000, 1, 2048
    feat = oracle.make_features(num_rows, dim, seed=21)
    table = PinnedTable(P, feat)
    ctrl = P.SSD_GNN_SSD_Controllers(1, 512, 1024, 0, 0, dim, True)
    caches = [P.Isolated_Cache(ctrl, None, r, G, cache_mb, table.device_ptr, num_rows=num_rows, rank=r) for r in range(G)]
    orcs = [oracle.OracleCache(cache_mb, dim, feat, n_gpus=G, distributed=True) for _ in range(G)]
    rng = np.random.default_rng(2)
    for step in range(4):
        idx_np = [rng.choice(num_rows, size=int(rng.integers(1, max_sample)), replace=False).astype(np.int64) for _ in range(G)]
        node = [torch.zeros(G * max_sample, dtype=torch.int64, device="cuda") for _ in range(G)]
        mp = [torch.zeros(G * max_sample, dtype=torch.int64, device="cuda") for _ in range(G)]
        cnt = [torch.zeros(G, dtype=torch.int64, device="cuda") for _ in range(G)]
        idx = [torch.from_numpy(i).cuda() for i in idx_np]
        for r in range(G):  # :152-153
            caches[r].split_node_list(idx[r].data_ptr(), len(idx_np[r]), node[r].data_ptr(), mp[r].data_ptr(), cnt[r].data_ptr(), G, max_sample)
        counts = [c.cpu().tolist() for c in cnt]
        # all_to_all of the id buffers (:156-165): recv[o][s] = node[s][o*max : o*max + counts[s][o]]
        outs = [torch.zeros((len(idx_np[r]), dim), dtype=torch.float32, device="cuda") for r in range(G)]
        got_rows = [[None] * G for _ in range(G)]
        for o in range(G):
            recv = [node[s][o * max_sample: o * max_sample + counts[s][o]].clone() for s in range(G)]  # separate, non-contiguous buffers
            gathered = [torch.zeros((counts[s][o], dim), dtype=torch.float32, device="cuda") for s in range(G)]  # :170-175
            caches[o].nccl_get_feature([t.data_ptr() for t in recv], [t.data_ptr() for t in gathered], [counts[s][o] for s in range(G)], G, max_sample)
            for s in range(G):
                got_rows[s][o] = gathered[s]           # send/recv (:194-203)
        for r in range(G):                            # :206-208 REMAP
            caches[r].map_feat_data(outs[r].data_ptr(), [got_rows[r][o].data_ptr() for o in range(G)], mp[r].data_ptr(),
                                    [counts[r][o] for o in range(G)], G, max_sample)
            assert outs[r].cpu().numpy().tobytes() == feat[idx_np[r]].tobytes()
        # separate per-peer buffers are served as one batch per peer, in peer order (documented in COALA_GNN_Pybind)
        for o in range(G):
            for s in range(G):
                ids = idx_np[s][idx_np[s] % G == o]
                orcs[o].read_feature(ids, oracle.SCHED_HITS_FIRST, want_rows=False)
            assert caches[o].stats()[:2] == (orcs[o].hit_cnt, orcs[o].miss_cnt)
    for c in caches:
        c.close()
    table.close()


@pytest.mark.parametrize("dim,tier", [(1024, "host"), (128, "host"), (300, "hbm")])
def test_split_serve_equals_one_serve(hiplib, oracle, dim, tier, monkeypatch):
    """coala_cache_serve_probe + coala_cache_serve_fill over slices that cover the batch once, in any order, leave rows, tag
    table, cursors and counters exactly as one coala_cache_serve (and as the oracle): ranking spans the whole batch."""
    import torch
    P = hiplib
    rng = np.random.default_rng(11)
    num_rows, G = 20000, 2
    feat = oracle.make_features(num_rows, dim, seed=9)
    owned = np.arange(0, num_rows, G)                       # owner 0 serves ids = 0 (mod G)
    table = PinnedTable(P, feat) if tier == "host" else None
    dev_table = torch.from_numpy(feat).cuda() if tier == "hbm" else None
    ptr = table.device_ptr if table is not None else dev_table.data_ptr()
    ctrl = P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, dim, True)
    a = P.SSD_GNN_NVSHMEM_Cache(ctrl, None, 0, G, 1, ptr, num_rows=num_rows, rank=0)
    b = P.SSD_GNN_NVSHMEM_Cache(ctrl, None, 0, G, 1, ptr, num_rows=num_rows, rank=0)
    orc = oracle.OracleCache(1, dim, feat, n_gpus=G, distributed=True)
    with pytest.raises(RuntimeError):                        # a fill needs its probe
        b.serve_fill(0, 0, 5, 0, 5)
    for step in range(6):
        n = int(rng.integers(1, 4000))
        ids = rng.choice(owned, size=n, replace=step % 2 == 0).astype(np.int64)   # duplicates every other step
        d_ids = torch.from_numpy(ids).cuda()
        out_a = torch.full((n, dim), -1.0, device="cuda")
        out_b = torch.full((n, dim), -1.0, device="cuda")
        a.serve(out_a.data_ptr(), d_ids.data_ptr(), n)
        cuts = sorted({0, n, *(int(c) for c in rng.integers(0, n + 1, size=3))})
        slices = list(zip(cuts[:-1], cuts[1:]))
        rng.shuffle(slices)
        b.serve_probe(out_b.data_ptr(), d_ids.data_ptr(), n)
        for lo, hi in slices:
            b.serve_fill(out_b.data_ptr(), d_ids.data_ptr(), n, lo, hi)
        orc.read_feature(ids, oracle.SCHED_HITS_FIRST, want_rows=False)
        torch.cuda.synchronize()
        assert out_b.cpu().numpy().tobytes() == feat[ids].tobytes() and torch.equal(out_a, out_b), f"step {step}"
        assert a.stats() == b.stats() == (orc.hit_cnt, orc.miss_cnt, 0)
        for x, y in zip(a.dump(), b.dump()):
            assert np.array_equal(x, y)
        assert np.array_equal(b.dump()[0], orc.keys()) and np.array_equal(b.dump()[1], orc.set_cnt())
    with pytest.raises(RuntimeError):                        # wrong batch size for the open batch
        b.serve_fill(out_b.data_ptr(), d_ids.data_ptr(), n + 1, 0, 1)
    a.close(); b.close()
    if table is not None:
        table.close()


def test_counts_ahead_ticket_ring_exhaustion_falls_back(hiplib, oracle):
    """More count exchanges issued ahead than the communicator's ring holds (COALA_COUNTS_RING = 8): the fetches whose tickets have
    left the ring exchange their counts again, synchronously -- on every rank alike, since every rank makes the same calls -- and
    deliver the same rows; the tickets still in the ring are used as issued."""
    import ctypes as C
    import threading
    import torch
    from COALA_GNN.COALA_GNN_Manager import NativeExchange
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    G, dim, num_rows, steps = 2, 128, 8000, 11
    assert _capi.COUNTS_RING == 8
    feat, tables, caches, orcs = _dist_fixture(hiplib, oracle, G, dim, 1, True, num_rows, seed=21, cls="Isolated_Cache")
    group = C.c_void_p()
    _capi.check(L.coala_comm_group_create(G, C.byref(group)))
    exs = [NativeExchange(None, 0, r, G, 0, inproc_group=group) for r in range(G)]
    ids_seen = [[None] * G for _ in range(steps)]
    used = [[None] * G for _ in range(steps)]
    errors = []

    def worker(r):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                batches = []
                for step in range(steps):                                         # every count exchange goes out first ...
                    ids = np.random.default_rng(40 * step + r).choice(num_rows, size=500 + 7 * step, replace=False)
                    ids = np.concatenate([ids[ids % G == o] for o in range(G)]).astype(np.int64)
                    cnt = torch.tensor([(ids % G == o).sum() for o in range(G)], dtype=torch.int64).cuda()
                    batches.append((ids, torch.from_numpy(ids).cuda(), cnt, exs[r].counts_begin(cnt.data_ptr())))
                for step, (ids, d_ids, cnt, ticket) in enumerate(batches):        # ... then the fetches, oldest ticket first
                    out = torch.full((len(ids), dim), -3.0, dtype=torch.float32, device="cuda")
                    used[step][r] = exs[r]._tickets - ticket <= _capi.COUNTS_RING
                    exs[r].fetch_bucketed(caches[r], out.data_ptr(), d_ids.data_ptr(), len(ids), cnt.data_ptr(), ticket=ticket)
                    torch.cuda.current_stream().synchronize()
                    assert out.cpu().numpy().tobytes() == feat[ids].tobytes(), f"rank {r} step {step}"
                    ids_seen[step][r] = ids
        except BaseException as e:  # noqa: BLE001
            errors.append((r, repr(e)))   # (the peer then times out on the in-process barrier: COALA_INPROC_TIMEOUT_S)

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    assert [u[0] for u in used] == [False] * 3 + [True] * 8 and all(u[0] == u[1] for u in used)   # 11 tickets, 8 slots: the first 3 fell back
    for step in range(steps):
        oracle.dist_fetch(orcs, ids_seen[step], oracle.SCHED_HITS_FIRST, want_rows=False)
    for r in range(G):
        assert caches[r].stats()[:2] == (orcs[r].hit_cnt, orcs[r].miss_cnt)
        keys, cnt, _ = caches[r].dump()
        assert np.array_equal(keys, orcs[r].keys()) and np.array_equal(cnt, orcs[r].set_cnt())
    for e in exs:
        e.close()
    _capi.check(L.coala_comm_group_destroy(group))
    for c in caches:
        c.close()
    for t in set(tables):
        t.close()


@pytest.mark.parametrize("dim,rounds,bucketed", [(100, 2, False), (99, 2, False), (1024, 3, False), (128, 1, False), (100, 2, True), (99, 3, True),
                                                 (1024, 2, "ahead")])
def test_native_fetch_rccl_one_rank_self_loopback(hiplib, oracle, dim, rounds, bucketed):
    """RcclTransport's grouped ncclSend / ncclRecv loop on the REAL transport.  RCCL cannot place two ranks on one device and a one-rank
    communicator skips the loop (p == rank), so until round 4 that code -- the element type chosen from the row size (dim 100: int64 x 50
    per row, dim 99: float x 99, dim 1024: int64 x 512), counts, displacements, the rounds on the communicator's own stream next to the
    fills on the caller's -- had never executed.  coala_comm_set_self_loopback sends the own segment down the road of a peer's: ids by
    ncclSend/ncclRecv to self, rows served into the staging buffer, shipped in `rounds` rounds by ncclSend/ncclRecv to self on the
    comm stream, un-permuted (or, bucketed, received in place).  Rows, counters, tag table and cursors against the oracle."""
    import torch
    from COALA_GNN.COALA_GNN_Manager import NativeExchange
    num_rows, cache_mb = 20000, 1
    feat, tables, caches, orcs = _dist_fixture(hiplib, oracle, 1, dim, cache_mb, False, num_rows, seed=12, cls="Isolated_Cache")
    ex = NativeExchange(None, 0, 0, 1, 0, rounds=rounds)        # a real RCCL communicator (ncclCommInitRank) of one rank
    assert ex.rccl_ranks == 1
    ex.set_self_loopback(True)
    rng = np.random.default_rng(5)
    stream = torch.cuda.Stream()
    side = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for step, n in enumerate([1500, 0, 3000, 1, 2500, 2500]):
            ids = rng.choice(num_rows // 2, size=n, replace=step == 5).astype(np.int64)
            idx = torch.from_numpy(ids).cuda() if n else torch.zeros(0, dtype=torch.int64, device="cuda")
            out = torch.full((max(n, 1), dim), -3.0, dtype=torch.float32, device="cuda")
            copy = torch.full((max(n, 1), dim), -5.0, dtype=torch.float32, device="cuda")   # (filled BEFORE the fetch: the consumer below must not race its fill)
            stream.synchronize()
            if bucketed:
                cnt = torch.tensor([n], dtype=torch.int64, device="cuda")
                ticket = None
                if bucketed == "ahead":
                    stream.synchronize()
                    with torch.cuda.stream(side):
                        ticket = ex.counts_begin(cnt.data_ptr())
                ex.fetch_events(2)               # begin / end events ride on the fetch's own launches (coala_comm_fetch_events; 1 = end events only)
                ex.fetch_bucketed(caches[0], out.data_ptr() if n else 0, idx.data_ptr() if n else 0, n, cnt.data_ptr(), ticket=ticket)
                begin, end_st, end_cs = ex.last_fetch_events()
                if n:
                    # a consumer on another stream that waits for BOTH end events -- and for nothing else -- sees every row
                    assert begin and end_st and end_cs
                    with torch.cuda.stream(side):
                        hiplib.stream_wait_event(end_st)
                        hiplib.stream_wait_event(end_cs)
                        copy[:n].copy_(out[:n])
                    side.synchronize()
                    assert copy[:n].cpu().numpy().tobytes() == feat[ids].tobytes(), f"step {step}: the consumer ran ahead of the fetch"
                    assert hiplib.event_elapsed_ms(begin, end_cs, wait=True) > 0.0
                else:
                    assert (begin, end_st, end_cs) == (None, None, None)
            else:
                ex.fetch(caches[0], out.data_ptr() if n else 0, idx.data_ptr() if n else 0, n)
                assert ex.last_fetch_events() == (None, None, None)      # routed fetches record nothing of the kind
            stream.synchronize()
            want = oracle.dist_fetch(orcs, [ids], oracle.SCHED_HITS_FIRST)[0]
            assert out[:n].cpu().numpy().tobytes() == feat[ids].tobytes() == want.tobytes(), f"step {step}: rows differ"
            if n == 0:
                assert float(out[0, 0]) == -3.0
            assert caches[0].stats()[:2] == (orcs[0].hit_cnt, orcs[0].miss_cnt)
            assert ex.last_send_counts == [n] and ex.last_recv_counts == [n]
    keys, cnt_, _ = caches[0].dump()
    assert np.array_equal(keys, orcs[0].keys()) and np.array_equal(cnt_, orcs[0].set_cnt())
    assert orcs[0].hit_cnt > 0 and orcs[0].miss_cnt > 0
    # ... and back: the same communicator without the loopback still delivers (own-shard bypass, no row exchange at one rank)
    ex.set_self_loopback(False)
    ids = rng.choice(num_rows // 2, size=800, replace=False).astype(np.int64)
    idx = torch.from_numpy(ids).cuda()
    out = torch.empty((800, dim), dtype=torch.float32, device="cuda")
    ex.fetch(caches[0], out.data_ptr(), idx.data_ptr(), 800)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == feat[ids].tobytes()
    ex.close()
    caches[0].close()
    tables[0].close()


@pytest.mark.parametrize("G,dim,rounds", [(3, 100, 2), (2, 1024, 3)])
def test_native_fetch_inproc_self_loopback_matches_oracle(hiplib, oracle, G, dim, rounds):
    """The loopback orchestration (no own-shard bypass: own rows staged, exchanged with oneself, un-permuted) with G in-process ranks:
    the delivered rows and every owner's table must be what the normal call produces -- i.e. what the oracle says."""
    import ctypes as C
    import threading
    import torch
    from COALA_GNN.COALA_GNN_Manager import NativeExchange
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    num_rows, steps = 12000, 4
    feat, tables, caches, orcs = _dist_fixture(hiplib, oracle, G, dim, 1, True, num_rows, seed=8, cls="Isolated_Cache")
    group = C.c_void_p()
    _capi.check(L.coala_comm_group_create(G, C.byref(group)))
    exs = [NativeExchange(None, 0, r, G, 0, inproc_group=group, rounds=rounds) for r in range(G)]
    for e in exs:
        e.set_self_loopback(True)
    rng = np.random.default_rng(91)
    plan = [[rng.choice(num_rows // 2, size=int(rng.integers(1, 2500)), replace=False).astype(np.int64) for _ in range(G)] for _ in range(steps)]
    got = [[None] * G for _ in range(steps)]
    errors = []
    bar = threading.Barrier(G, timeout=180)

    def worker(r):
        try:
            torch.cuda.set_device(0)
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for step in range(steps):
                    ids = plan[step][r]
                    idx = torch.from_numpy(ids).cuda()
                    out = torch.full((len(ids), dim), -9.0, dtype=torch.float32, device="cuda")
                    exs[r].fetch(caches[r], out.data_ptr(), idx.data_ptr(), len(ids))
                    stream.synchronize()
                    got[step][r] = out.cpu().numpy()
                    bar.wait()
        except BaseException as e:  # noqa: BLE001
            errors.append((r, repr(e)))
            bar.abort()
    threads = [threading.Thread(target=worker, args=(r,)) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    for step in range(steps):
        want = oracle.dist_fetch(orcs, plan[step], oracle.SCHED_HITS_FIRST)
        for r in range(G):
            assert got[step][r].tobytes() == feat[plan[step][r]].tobytes() == want[r].tobytes(), f"rank {r} step {step}: rows differ"
    for r in range(G):
        keys, cnt, _ = caches[r].dump()
        assert np.array_equal(keys, orcs[r].keys()) and np.array_equal(cnt, orcs[r].set_cnt())
        assert caches[r].stats()[:2] == (orcs[r].hit_cnt, orcs[r].miss_cnt)
    for e in exs:
        e.close()
    _capi.check(L.coala_comm_group_destroy(group))
    for c in caches:
        c.close()
    for t in set(tables):
        t.close()


def test_native_fetch_over_rccl_two_gpus():
    """The fused native fetch over a REAL RCCL communicator between two distinct GPUs (bucketed and routed), against the table.
    Needs two visible GPUs: skipped on the one-GPU development / round-end boxes; it is what the driver's multi-GPU node exercises
    through bench.py (whose first-minibatch check is the same comparison)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL cannot place two ranks on one device)")
    import os
    import socket
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", COALA_TEST_REAL_RCCL="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(here, "_dist_gpu_worker.py"), "nccl"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for r, p in enumerate(procs):
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0 and f"rank {r} ok" in out, out[-3000:]


@pytest.mark.parametrize("name,dim,num_rows,cache_mb,fanout,avg_degree,steps", [
    ("IGB-medium 10,10, 4 GiB x 8 (configs[2])", 1024, 10_000_000, 4096, [10, 10], 10.5, 3),
    ("papers100M 15,10,5, 16 GiB x 8 (configs[3])", 128, 111_059_956, 16384, [15, 10, 5], 6.0, 2),
    # configs[4]: the full table is 409.6 GB, the box's job may hold ~290 GB of host memory -> node count x 0.5 (SURVEY 8d allows a stated
    # scale factor; examples/ssd_gnn_dataloader.py:375-376 for the shape).  Everything else is the configuration's: 16 GiB of cache per
    # rank, 4-KiB lines, 131,072 sets per rank (nvshmem_cache.h:191-196), fan-out 10,10,10 at bs 1024, <= 1,362,944 rows per minibatch.
    ("IGB-large 10,10,10, 16 GiB x 8 + host spill (configs[4]), rows x 0.5", 1024, 50_000_000, 16384, [10, 10, 10], 10.5, 2),
])
def test_full_size_eight_inproc_ranks(hiplib, oracle, name, dim, num_rows, cache_mb, fanout, avg_degree, steps):
    """The 8-GPU configurations of BASELINE.json at full size on ONE MI355X: the whole table pinned on the host, partitioned by
    owner (IGB-medium: 8 shards of 5.12 GB; papers100M: 8 x 7.1 GB), 8 logical ranks (host threads) each with its shard of the
    partitioned cache (8 x 4 GiB / 8 x 16 GiB of HBM), the configuration's fan-out at bs = 1024, sampler output bucketed by owner
    -> the native fused fetch.  Size-independent properties: every delivered row equals the procedural table bit for bit, a
    batch never exceeds the reference's max_sample (123,904 / 1,081,344 rows), owner counters and whole tag tables equal the
    tag-only oracle fed with the same id lists, a second pass over the same minibatches is (almost) all hits.  configs[4], IGB-large,
    runs in the same distributed form with the node count scaled by 0.5 (8 shards of 25.6 GB = 204.8 GB pinned; the full 409.6 GB
    table is beyond the host memory a job may hold on the box): max_sample 1,362,944 rows = 5.58 GB of output per rank and step."""
    import ctypes as C
    import threading
    import torch
    from COALA_GNN.COALA_GNN_Manager import NativeExchange
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import PinnedFeatureTable, feature_rows_torch, fill_table_partition, powerlaw_csc
    from COALA_GNN_Pybind import _capi
    P = hiplib
    L = _capi.load()
    G, batch = 8, 1024
    max_sample = batch * int(np.prod([f + 1 for f in fanout]))
    shards = []
    for r in range(G):
        t = PinnedFeatureTable((num_rows - r + G - 1) // G, dim, 0)
        fill_table_partition(t.cpu_tensor, 6, r, G, device="cuda:0")
        shards.append(t)
    ctrl = P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, dim, True)
    caches = [P.Isolated_Cache(ctrl, None, r, G, cache_mb, shards[r].device_ptr, num_rows=num_rows, rank=r, cold_partitioned=True,
                               sync=False, max_batch=max_sample * 2) for r in range(G)]
    assert caches[0].geometry().num_sets == oracle.num_sets(cache_mb, oracle.cache_dim(dim))
    orcs = [oracle.OracleCache(cache_mb, dim, np.zeros((1, dim), dtype=np.float32), n_gpus=G, distributed=True, tag_only=True) for _ in range(G)]
    indptr, indices = powerlaw_csc(num_rows, avg_degree, seed=0, device="cuda")
    train = torch.randperm(int(0.6 * num_rows), generator=torch.Generator().manual_seed(1))
    group = C.c_void_p()
    _capi.check(L.coala_comm_group_create(G, C.byref(group)))
    exs = [NativeExchange(None, 0, r, G, 0, inproc_group=group) for r in range(G)]
    samplers = [NeighborSampler(fanout, seed=0, bucket_by_owner=G) for _ in range(G)]
    graphs = [s.make_graph(indptr, indices) for s in samplers]
    ids_seen = [[None] * G for _ in range(2 * steps)]
    errors = []
    bar = threading.Barrier(G, timeout=300)

    def worker(r):
        try:
            torch.cuda.set_device(0)
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for t in range(2 * steps):
                    step = t % steps                                # the second pass replays the first
                    lo = (step * G + r) * batch
                    ids, _, blocks = samplers[r].sample(graphs[r], train[lo: lo + batch].cuda(), step=step)
                    n = ids.numel()
                    assert batch <= n <= max_sample
                    feat = torch.full((n, dim), -7.0, dtype=torch.float32, device="cuda")
                    exs[r].fetch_bucketed(caches[r], feat.data_ptr(), ids.data_ptr(), n, blocks[0].owner_counts.data_ptr())
                    for a in range(0, n, 1 << 15):
                        assert torch.equal(feat[a: a + (1 << 15)], feature_rows_torch(ids[a: a + (1 << 15)], dim, 6)), f"rank {r} pass {t}"
                    stream.synchronize()
                    ids_seen[t][r] = ids.cpu().numpy()
                    bar.wait()
        except BaseException as e:  # noqa: BLE001
            errors.append((r, repr(e)))
            bar.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, errors
    first_pass = None
    for t in range(2 * steps):
        oracle.dist_fetch(orcs, ids_seen[t], oracle.SCHED_HITS_FIRST, want_rows=False)
        if t == steps - 1:
            first_pass = (sum(o.hit_cnt for o in orcs), sum(o.miss_cnt for o in orcs))
    total = sum(len(x) for row in ids_seen for x in row)
    hits = misses = 0
    for r in range(G):
        h, m, bad = caches[r].stats()
        assert (h, m, bad) == (orcs[r].hit_cnt, orcs[r].miss_cnt, 0), f"owner {r}"
        keys, cnt, _ = caches[r].dump()
        assert np.array_equal(keys, orcs[r].keys()) and np.array_equal(cnt, orcs[r].set_cnt()), f"owner {r}"
        hits, misses = hits + h, misses + m
    assert hits + misses == total
    second_hits = hits - first_pass[0]
    assert second_hits > 0.99 * (total // 2), (first_pass, hits, misses)   # replay: only ids beyond a set's 32 ways miss again
    for e in exs:
        e.close()
    _capi.check(L.coala_comm_group_destroy(group))
    for x in graphs:
        x.close()
    for c in caches:
        c.close()
    for t in shards:
        t.close()


def test_native_fetch_local_failure_does_not_strand_the_peers(hiplib, oracle, monkeypatch):
    """A rank that fails locally in the middle of the collective sequence (here: bucket counts that do not add up to its batch,
    detected after the count exchange) aborts the transport: its peers come back with an error instead of waiting for ever, every
    communicator of the group refuses further fetches, and tearing everything down still works."""
    import ctypes as C
    import threading
    import torch
    from COALA_GNN.COALA_GNN_Manager import NativeExchange
    from COALA_GNN_Pybind import _capi
    monkeypatch.setenv("COALA_INPROC_TIMEOUT_S", "20")
    L = _capi.load()
    G, dim, num_rows = 3, 64, 6000
    feat, tables, caches, orcs = _dist_fixture(hiplib, oracle, G, dim, 1, True, num_rows, seed=3, cls="Isolated_Cache")
    group = C.c_void_p()
    _capi.check(L.coala_comm_group_create(G, C.byref(group)))
    exs = [NativeExchange(None, 0, r, G, 0, inproc_group=group) for r in range(G)]
    outcome = [None] * G
    second = [None] * G

    def worker(r):
        torch.cuda.set_device(0)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            ids = np.sort(np.random.default_rng(5 + r).choice(num_rows, size=900, replace=False))
            ids = np.concatenate([ids[ids % G == o] for o in range(G)])          # bucketed by owner
            cnt = np.array([(ids % G == o).sum() for o in range(G)], dtype=np.int64)
            if r == 1:
                cnt[0] += 5                                                      # the counts of rank 1 do not sum to its batch
            idx, cnt_d = torch.from_numpy(ids).cuda(), torch.from_numpy(cnt).cuda()
            out = torch.empty((len(ids), dim), dtype=torch.float32, device="cuda")
            for attempt, slot in ((0, outcome), (1, second)):
                try:
                    exs[r].fetch_bucketed(caches[r], out.data_ptr(), idx.data_ptr(), len(ids), cnt_d.data_ptr())
                    stream.synchronize()
                    slot[r] = "ok"
                except RuntimeError as e:
                    slot[r] = str(e)

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a rank is still waiting for the one that failed"
    assert "bucket counts sum to" in outcome[1]
    assert all(o != "ok" for o in outcome), outcome                               # nobody reports success for the broken step
    assert all("aborted" in s or "destroy it" in s for s in second), second       # and the group stays unusable
    torch.cuda.synchronize()
    for e in exs:
        e.close()
    _capi.check(L.coala_comm_group_destroy(group))
    for c in caches:
        c.close()
    for t in set(tables):
        t.close()


@pytest.mark.parametrize("dim", [100, 128])
def test_native_fetch_random_call_sequence_on_one_group(hiplib, oracle, dim, monkeypatch):
    """A seeded sequence of a dozen fetches on ONE in-process group of three ranks, every kind interleaved on the same communicators: routed,
    bucketed, and bucketed with the counts exchanged ahead (one step ahead, i.e. in front of another fetch); `rounds` changed between the
    fetches over 1..4; a rank with an empty batch beside peers with full ones; a step in which nobody asks rank 2 for anything, so that it
    serves nothing and still receives its own rows; a peer's segment of 2 ids cut into 4 rounds (empty slices); a move of every rank to
    another stream; fetch_events(2) for the bucketed fetches of the second half, where a consumer that waits for the two end events and
    for nothing else must see every row.  Rows bit for bit against the oracle, per-peer counts against the host's."""
    import ctypes as C
    import threading
    import torch
    from COALA_GNN.COALA_GNN_Manager import NativeExchange
    from COALA_GNN_Pybind import _capi
    monkeypatch.setenv("COALA_INPROC_TIMEOUT_S", "20")   # a wait that never ends finishes the test, not the job
    L = _capi.load()
    G, num_rows = 3, 6000
    modes = ["routed", "bucketed", "ahead", "bucketed", "routed", "ahead", "ahead", "bucketed", "routed", "ahead", "bucketed", "routed"]
    steps, move_at = len(modes), 6                                                  # events on, and the other stream, from step 6 on
    EMPTY_RANK, NOBODY_ASKS_2, TINY_SEGMENT = 3, 7, 9
    rng = np.random.default_rng(2024 + dim)
    rounds = [int(k) for k in rng.permutation([1, 2, 3, 4] * 3)]
    rounds[TINY_SEGMENT] = 4
    plan = []
    for step in range(steps):
        batch = []
        for r in range(G):
            ids = rng.choice(num_rows, size=int(rng.integers(200, 901)), replace=False).astype(np.int64)
            if step == EMPTY_RANK and r == 1:
                ids = ids[:0]
            if step == NOBODY_ASKS_2:
                ids = ids[ids % G != 2]
            if step == TINY_SEGMENT and r == 0:
                ids = np.concatenate([ids[ids % G != 1], ids[ids % G == 1][:2]])      # 2 ids for owner 1, 4 rounds
            if modes[step] != "routed":
                ids = np.concatenate([ids[ids % G == o] for o in range(G)])          # as the sampler delivers them: bucketed by owner
            batch.append(ids)
        plan.append(batch)
    assert len(plan[EMPTY_RANK][1]) == 0 and all(len(plan[EMPTY_RANK][r]) for r in (0, 2))
    assert all((plan[NOBODY_ASKS_2][r] % G != 2).all() for r in range(G)) and len(plan[NOBODY_ASKS_2][2])
    assert int((plan[TINY_SEGMENT][0] % G == 1).sum()) == 2
    assert all(len(i) <= 900 for b in plan for i in b) and len(set(rounds)) == 4

    feat, tables, caches, orcs = _dist_fixture(hiplib, oracle, G, dim, 1, True, num_rows, seed=31, cls="Isolated_Cache")
    group = C.c_void_p()
    _capi.check(L.coala_comm_group_create(G, C.byref(group)))
    exs = [NativeExchange(None, 0, r, G, 0, inproc_group=group) for r in range(G)]
    got = [[None] * G for _ in range(steps)]
    counts = [[None] * G for _ in range(steps)]
    errors = []
    bar = threading.Barrier(G, timeout=60)

    def worker(r):
        try:
            torch.cuda.set_device(0)
            streams, side = [torch.cuda.Stream(), torch.cuda.Stream()], torch.cuda.Stream()
            ex, dev, tickets = exs[r], [], {}
            for step in range(steps):
                ids = plan[step][r]
                cnt = torch.tensor([int((ids % G == o).sum()) for o in range(G)], dtype=torch.int64).cuda()
                dev.append((torch.from_numpy(ids).cuda() if len(ids) else torch.zeros(0, dtype=torch.int64, device="cuda"), cnt))
            torch.cuda.synchronize()
            for step in range(steps):
                with torch.cuda.stream(streams[step >= move_at]):
                    stream = torch.cuda.current_stream()
                    ids, (idx, cnt), n, mode = plan[step][r], dev[step], len(plan[step][r]), modes[step]
                    if step + 1 < steps and modes[step + 1] == "ahead":               # the next fetch's counts go out in front of this fetch
                        tickets[step + 1] = ex.counts_begin(dev[step + 1][1].data_ptr())
                    ex.rounds = rounds[step]
                    out = torch.full((max(n, 1), dim), -9.0, dtype=torch.float32, device="cuda")
                    copy = torch.full((max(n, 1), dim), -5.0, dtype=torch.float32, device="cuda")
                    stream.synchronize()
                    out_ptr, idx_ptr = (out.data_ptr(), idx.data_ptr()) if n else (0, 0)
                    if mode == "routed":
                        ex.fetch(caches[r], out_ptr, idx_ptr, n)
                        assert ex.last_fetch_events() == (None, None, None)
                    else:
                        ex.fetch_events(2 if step >= move_at else 0)
                        ex.fetch_bucketed(caches[r], out_ptr, idx_ptr, n, cnt.data_ptr(), ticket=tickets.get(step))
                    counts[step][r] = (list(ex.last_send_counts), list(ex.last_recv_counts))
                    if mode != "routed" and step >= move_at and n:
                        begin, end_st, end_cs = ex.last_fetch_events()
                        assert begin and end_st and end_cs
                        with torch.cuda.stream(side):                                 # a consumer that waits for the end events only
                            hiplib.stream_wait_event(end_st)
                            hiplib.stream_wait_event(end_cs)
                            copy[:n].copy_(out[:n])
                        side.synchronize()
                        got[step][r] = copy[:n].cpu().numpy()
                        ms = hiplib.event_elapsed_ms(begin, end_cs, wait=False)       # complete by now: the rows have been read
                        assert ms is not None and ms >= 0.0, f"rank {r} step {step}: end event {ms}"
                    else:
                        if mode != "routed":
                            assert ex.last_fetch_events() == (None, None, None)
                        stream.synchronize()
                        got[step][r] = out[:n].cpu().numpy()
                    stream.synchronize()
                bar.wait()
        except BaseException as e:  # noqa: BLE001
            errors.append((r, repr(e)))
            bar.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads) and not errors, errors
    for step in range(steps):
        want = oracle.dist_fetch(orcs, plan[step], oracle.SCHED_HITS_FIRST)
        for r in range(G):
            assert got[step][r].tobytes() == feat[plan[step][r]].tobytes() == want[r].tobytes(), f"rank {r} step {step} ({modes[step]}): rows differ"
            send, recv = counts[step][r]
            assert send == [int((plan[step][r] % G == o).sum()) for o in range(G)], f"rank {r} step {step}"
            assert recv == [int((plan[step][s] % G == r).sum()) for s in range(G)], f"rank {r} step {step}"
    assert counts[NOBODY_ASKS_2][2][1] == [0] * G and sum(counts[NOBODY_ASKS_2][2][0]) > 0
    for r in range(G):
        assert caches[r].stats()[:2] == (orcs[r].hit_cnt, orcs[r].miss_cnt)
        keys, cnt_, _ = caches[r].dump()
        assert np.array_equal(keys, orcs[r].keys()) and np.array_equal(cnt_, orcs[r].set_cnt())
    assert sum(o.hit_cnt for o in orcs) > 0 and sum(o.miss_cnt for o in orcs) > 0
    for e in exs:
        e.close()
    _capi.check(L.coala_comm_group_destroy(group))
    for c in caches:
        c.close()
    for t in set(tables):
        t.close()
