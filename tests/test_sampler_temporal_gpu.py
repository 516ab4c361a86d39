"""GPU tests of temporal neighbour sampling (COALA_GNN.sampler.TemporalNeighborSampler; temporal_select in coala_sampler.hip).

The rule is exact integer arithmetic, so every output -- source lists, nbr, edge ids, source and destination times, input nodes -- is
compared bit for bit with the numpy restatement of tests/_temporal_ref.py (checked on its own in test_sampler_temporal_cpu.py).  Every
call uses at most 512 seeds."""
import ctypes as C

import numpy as np
import pytest

from _temporal_ref import decode, edge_case_graph, eligible, encode, node_bits_of, reference_layers, row_index, temporal_layer

pytestmark = pytest.mark.gpu

GUARD = 67
HUB = 1_000_003
T_MAX = 1 << 20


def _check_call(smp, g, host, nodes, times, step):
    """One sample of `smp` over the pairs (nodes, times): every layer equal to the reference, bit for bit.  host = (ip, ix, ts, index)."""
    import torch
    ip, ix, ts, index = host
    N = len(ip) - 1
    input_nodes, out_nodes, blocks = smp.sample(g, torch.from_numpy(nodes).cuda(), step=step, seed_times=torch.from_numpy(times).cuda())
    rev = list(reversed(smp.fanouts))
    ref, slot_time = reference_layers(ip, ix, ts, nodes, times, rev, smp.seed, step, smp.strategy, smp.inclusive, index)
    n_dst, dst_nodes, dst_times = len(nodes), nodes, times
    for l, (src_r, nbr_r, eid_r) in enumerate(ref):
        b = blocks[len(rev) - 1 - l]
        where = f"layer {l} of {rev}, {smp.strategy}, inclusive={smp.inclusive}, {len(nodes)} seeds, seed {smp.seed}, step {step}"
        src_nodes, src_times = decode(src_r, slot_time, N)
        src_nodes[: len(nodes)] = nodes
        assert b.indptr is None and b.num_dst == n_dst and b.num_src == len(src_r), where
        assert b.nbr.dtype == torch.int32 and tuple(b.nbr.shape) == (n_dst, rev[l])
        assert np.array_equal(b.nbr.cpu().numpy(), nbr_r), f"nbr differs: {where}"
        assert b.src_nodes.dtype == torch.int64 and np.array_equal(b.src_nodes.cpu().numpy(), src_nodes), f"source list differs: {where}"
        assert b.src_times.dtype == torch.int64 and np.array_equal(b.src_times.cpu().numpy(), src_times), f"source times differ: {where}"
        assert b.dst_times.dtype == torch.int64 and np.array_equal(b.dst_times.cpu().numpy(), dst_times), f"destination times differ: {where}"
        assert np.array_equal(b.dstdata["_ID"].cpu().numpy(), dst_nodes)
        if smp.edge_ids:
            assert b.edata["_ID"].dtype == torch.int64 and np.array_equal(b.edata["_ID"].cpu().numpy(), eid_r), f"edge ids differ: {where}"
        else:
            assert "_ID" not in b.edata and "dt" not in b.edata
        n_dst, dst_nodes, dst_times = len(src_r), src_nodes, src_times
    assert input_nodes is blocks[0].src_nodes and torch.equal(out_nodes.cpu(), torch.from_numpy(nodes))
    return blocks, ref, slot_time


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.fixture(scope="module")
def graphs(hiplib):
    """powerlaw_csc / community_csc (200000, 30) with edge_times sorted per row: name -> (host arrays and the reference's index, graph)."""
    from COALA_GNN.sampler import TemporalNeighborSampler, check_time_sorted
    from COALA_GNN.synthetic import community_csc, edge_times, powerlaw_csc
    made = {}
    for name, make in (("powerlaw", powerlaw_csc), ("community", community_csc)):
        d_ip, d_ix = make(200_000, 30, seed=1, device="cuda")
        d_ts = edge_times(d_ip, seed=4, t_max=T_MAX)
        check_time_sorted(d_ip, d_ts)
        g = TemporalNeighborSampler.make_graph(d_ip, d_ix, edata={"ts": d_ts})
        ip, ts = d_ip.cpu().numpy(), d_ts.cpu().numpy()
        made[name] = ((ip, d_ix.cpu().numpy(), ts, row_index(ip, ts)), g)
    yield made
    for _, g in made.values():
        g.close()


def _mixed_pairs(host, seed):
    """512 distinct (node, time) pairs: 32 below every timestamp, 32 above every timestamp, 64 at the timestamp of one of the node's own
    edges, one node at two times, and random times for the rest; many nodes share a time (the first two groups)."""
    ip, ix, ts, _ = host
    rng = np.random.default_rng(seed)
    N = len(ip) - 1
    perm = rng.permutation(N).astype(np.int64)
    own = perm[np.diff(ip)[perm] > 0][:64]                       # nodes queried at the timestamp of their own middle edge
    rest = perm[~np.isin(perm, own)]
    nodes = np.concatenate([rest[:64], own, rest[64: 64 + 384]])
    times = rng.integers(0, T_MAX, size=512).astype(np.int64)
    times[:32] = int(ts.min()) - 5
    times[32:64] = int(ts.max()) + 7
    times[64:128] = ts[ip[own] + np.diff(ip)[own] // 2]
    nodes[511] = nodes[200]                      # one node at two times
    times[511] = times[200] + 1000
    assert len(set(zip(nodes.tolist(), times.tolist()))) == 512
    return nodes, times


FANOUTS = [[10], [5, 5], [32, 1], [2, 5, 7]]
CASES = [(name, f, s, inc) for name in ("powerlaw", "community") for f in FANOUTS for s in ("uniform", "last") for inc in (False, True)]


@pytest.mark.parametrize("name,fanouts,strategy,inclusive", CASES, ids=[f"{n}-{'_'.join(map(str, f))}-{s}-{'le' if i else 'lt'}" for n, f, s, i in CASES])
def test_temporal_layers_exact(graphs, name, fanouts, strategy, inclusive):
    import torch
    from COALA_GNN.sampler import TemporalNeighborSampler
    host, g = graphs[name]
    edge_ids =(len(fanouts) + (strategy == "last") + inclusive) % 2 == 0     # on and off, under every strategy and both bounds
    smp = TemporalNeighborSampler(fanouts, strategy=strategy, inclusive=inclusive, seed=21, edge_ids=edge_ids)
    nodes, times = _mixed_pairs(host, seed=len(fanouts))
    _, ref, _ = _check_call(smp, g, host, nodes, times, step=3)
    eid = ref[0][2]
    assert (eid[:32] == -1).all(), "a time below every timestamp: empty rows"
    deg = np.diff(host[0])[nodes[32:64]]
    assert ((eid[32:64] >= 0).sum(1) == np.minimum(deg, fanouts[-1])).all(), "a time above every timestamp: the whole row is eligible"
    assert smp.step == 0
    smp.sample(g, torch.from_numpy(nodes[:4]).cuda(), seed_times=torch.from_numpy(times[:4]).cuda())
    assert smp.step == 1, "a call without step= advances the sampler's own"


def test_strict_and_inclusive_differ_at_an_edge_timestamp(graphs):
    from COALA_GNN.sampler import TemporalNeighborSampler
    host, g = graphs["powerlaw"]
    ip, ix, ts, index = host
    nodes, times = _mixed_pairs(host, seed=9)
    nodes, times = nodes[64:128], times[64:128]
    m_lt, m_le = eligible(ip, ts, nodes, times, False, index), eligible(ip, ts, nodes, times, True, index)
    assert (m_le > m_lt).all()
    small = np.nonzero(m_le <= 32)[0]
    assert len(small) > 0
    got = {}
    for inclusive in (False, True):
        smp = TemporalNeighborSampler([32], strategy="last", inclusive=inclusive, seed=1)
        blocks, _, _ = _check_call(smp, g, host, nodes, times, step=0)
        got[inclusive] = (blocks[0].edata["_ID"] >= 0).sum(1).cpu().numpy()
    assert np.array_equal(got[False][small], m_lt[small]) and np.array_equal(got[True][small], m_le[small])


# ------------------------------------------------------------------------------------------------ 2. hand-made graph
@pytest.fixture(scope="module")
def edge_graph(hiplib):
    import torch
    from COALA_GNN.sampler import TemporalNeighborSampler
    ip, ix, ts, named = edge_case_graph(f=5, hub_degree=HUB, seed=2)
    g = TemporalNeighborSampler.make_graph(*[torch.from_numpy(a).cuda() for a in (ip, ix)], edata={"ts": torch.from_numpy(ts).cuda()})
    yield (ip, ix, ts, row_index(ip, ts)), named, g
    g.close()


def _edge_pairs(host, named):
    """Every named row at its first, a middle and its last timestamp, one before and one past them; the hub at the same; every plain row
    once; a seed outside the graph and a negative one."""
    ip, ix, ts, _ = host
    N = len(ip) - 1
    nodes, times = [], []
    for name, v in named.items():
        row = ts[ip[v]: ip[v + 1]]
        qs = [0, 500] if len(row) == 0 else [int(row[0]) - 1, int(row[0]), int(row[len(row) // 2]), int(row[-1]), int(row[-1]) + 1]
        for q in sorted(set(qs)):
            nodes.append(v)
            times.append(q)
    rng = np.random.default_rng(5)
    for v in range(len(named) - 1, N - 1):
        nodes.append(v)
        times.append(int(rng.integers(0, 1000)))
    nodes += [N, N + 12345, -1, -7]
    times += [500, 501, 502, 123]                # they all take the node field num_nodes: distinct codes need distinct times
    assert len(nodes) <= 512
    return np.array(nodes, dtype=np.int64), np.array(times, dtype=np.int64)


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("strategy", ["uniform", "last"])
@pytest.mark.parametrize("fanouts", [[5], [5, 5], [32, 1]])
def test_temporal_on_edge_graph(edge_graph, fanouts, strategy, inclusive):
    from COALA_GNN.sampler import TemporalNeighborSampler
    host, named, g = edge_graph
    nodes, times = _edge_pairs(host, named)
    smp = TemporalNeighborSampler(fanouts, strategy=strategy, inclusive=inclusive, seed=8)
    blocks, ref, _ = _check_call(smp, g, host, nodes, times, step=1)
    eid = ref[0][2]
    assert (eid[-4:] == -1).all(), "seeds outside the graph: empty rows"
    hub = np.nonzero(nodes == named["hub"])[0]
    m = eligible(host[0], host[2], nodes[hub], times[hub], inclusive, host[3])
    assert m[0] == 0 and m[-1] == HUB and (np.diff(m) >= 0).all() and len(set(m.tolist())) >= 4, "the hub before its first edge, in between, past its last"
    assert ((eid[hub] >= 0).sum(1) == np.minimum(m, fanouts[-1])).all()


@pytest.mark.parametrize("strategy,inclusive", [("uniform", False), ("last", True)])
def test_nothing_is_written_outside_the_buffers(edge_graph, strategy, inclusive):
    """The C entry point with guard words in front of and behind every output buffer, over the edge-case pairs and codes that do not
    decode: a negative code, a slot past the table, a node field past the graph."""
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    host, named, g = edge_graph
    ip, ix, ts, index = host
    N = len(ip) - 1
    L = _capi.load()
    nodes, times = _edge_pairs(host, named)
    codes, slot_time = encode(nodes, times, N)
    bits = node_bits_of(N)
    codes = np.concatenate([codes, np.array([-1, (len(slot_time) << bits) | 3, (1 << bits) | ((1 << bits) - 1), 1 << 62], dtype=np.int64)])
    n, fan = len(codes), [5, 7]
    caps, specs = n, []
    for f in fan:
        specs.append((caps * (f + 1), caps * f))
        caps *= f + 1
    bufs, lay = [], []
    for src_cap, edge_cap in specs:
        src = torch.full((GUARD + src_cap + GUARD,), -77, dtype=torch.int64, device="cuda")
        nbr = torch.full((GUARD + edge_cap + GUARD,), -77, dtype=torch.int32, device="cuda")
        eid = torch.full((GUARD + edge_cap + GUARD,), -77, dtype=torch.int64, device="cuda")
        bufs.append((src, nbr, eid))
        lay.append(_capi.SamplerLayer(src[GUARD:].data_ptr(), nbr[GUARD:].data_ptr(), None, src_cap, edge_cap))
    d_codes, d_slot = torch.from_numpy(codes).cuda(), torch.from_numpy(slot_time).cuda()
    n_src, n_edges = (C.c_int64 * 2)(), (C.c_int64 * 2)()
    eid_p = (C.c_void_p * 2)(*[b[2][GUARD:].data_ptr() for b in bufs])
    ticket = C.c_int64(-1)
    _capi.check(L.coala_sampler_sample_layers_temporal(g._h, d_codes.data_ptr(), n, (C.c_int32 * 2)(*fan), 2, 13, 2, (_capi.SamplerLayer * 2)(*lay),
                                                       g.edge_times("ts").data_ptr(), d_slot.data_ptr(), len(slot_time), int(strategy == "last"),
                                                       int(inclusive), eid_p, None, None, C.byref(ticket), current_stream()))
    _capi.check(L.coala_sampler_wait_layers(g._h, ticket.value, n_src, n_edges, None))
    torch.cuda.synchronize()
    dst = codes
    for l, ((src_cap, edge_cap), (src, nbr, eid)) in enumerate(zip(specs, bufs)):
        for buf, cap in ((src, src_cap), (nbr, edge_cap), (eid, edge_cap)):
            assert torch.all(buf[:GUARD] == -77) and torch.all(buf[GUARD + cap:] == -77), "a guard word lost its sentinel"
        src_r, nbr_r, eid_r = temporal_layer(ip, ix, ts, dst, slot_time, fan[l], 13, 2, l, strategy, inclusive, index)
        assert n_src[l] == len(src_r) and n_edges[l] == len(dst) * fan[l]
        assert np.array_equal(src[GUARD: GUARD + len(src_r)].cpu().numpy(), src_r)
        assert np.array_equal(nbr[GUARD: GUARD + nbr_r.size].cpu().numpy(), nbr_r.reshape(-1))
        assert np.array_equal(eid[GUARD: GUARD + eid_r.size].cpu().numpy(), eid_r.reshape(-1))
        if l == 0:
            assert (eid_r[-4:] == -1).all() and src_r[n - 4: n - 1].tolist() == codes[-3:].tolist(), "not decodable: empty rows, inserted unless negative"
        dst = src_r


# ------------------------------------------------------------------------------------------------ 3. causality
@pytest.mark.parametrize("strategy,inclusive", [("uniform", False), ("uniform", True), ("last", False), ("last", True)])
def test_no_block_reads_the_future(graphs, strategy, inclusive):
    """Independent of the reference: through edata['_ID'] and dst_times, every sampled edge of every layer is older than its row's query
    time, a neighbour carries its row's time on, and edata['dt'] is the difference."""
    import torch
    from COALA_GNN.sampler import TemporalNeighborSampler
    host, g = graphs["community"]
    nodes, times = _mixed_pairs(host, seed=77)
    smp = TemporalNeighborSampler([4, 6, 3], strategy=strategy, inclusive=inclusive, seed=2)
    input_nodes, _, blocks = smp.sample(g, torch.from_numpy(nodes).cuda(), seed_times=torch.from_numpy(times).cuda())
    d_ts, d_ix = g.edge_times("ts"), g.indices
    some = 0
    for b in blocks:
        eid, valid = b.edata["_ID"], b.edata["_ID"] >= 0
        assert torch.equal(valid, b.nbr >= 0)
        when = d_ts[eid.clamp_min(0)]
        t_row = b.dst_times.unsqueeze(1).expand_as(eid)
        assert bool(((when <= t_row) if inclusive else (when < t_row))[valid].all()), "an edge from the future"
        dt = b.edata["dt"]
        assert dt.dtype == torch.int64 and dt.shape == eid.shape and torch.equal(dt, torch.where(valid, t_row - when, 0))
        assert bool((dt >= 0).all()) and (inclusive or bool((dt[valid] > 0).all()))
        assert torch.equal(b.edata["ts"], torch.where(valid, when, 0)), "graph edata through the edge ids"
        at = b.nbr.clamp_min(0).to(torch.int64)
        assert torch.equal(b.src_times[at][valid], t_row[valid]) and torch.equal(b.src_nodes[at][valid], d_ix[eid.clamp_min(0)][valid])
        assert torch.equal(b.src_times[: b.num_dst], b.dst_times)
        some += int(valid.sum())
    assert some > 1000 and torch.equal(blocks[0].dst_times, blocks[1].src_times)
    pairs = torch.stack([input_nodes, blocks[0].src_times], 1)
    assert len(torch.unique(pairs, dim=0)) == len(pairs), "distinct (node, time) items"
    assert len(torch.unique(input_nodes)) < len(input_nodes), "a node reached at two times is listed twice"


# ------------------------------------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("strategy", ["uniform", "last"])
def test_a_row_depends_on_its_pair_alone(graphs, strategy):
    import torch
    from COALA_GNN.sampler import TemporalNeighborSampler
    host, g = graphs["powerlaw"]
    ip = host[0]
    nodes, times = _mixed_pairs(host, seed=5)
    smp = TemporalNeighborSampler([10], strategy=strategy, seed=6)

    def rows(nodes, times):
        _, _, blocks = smp.sample(g, torch.from_numpy(nodes).cuda(), step=4, seed_times=torch.from_numpy(times).cuda())
        return blocks[0].edata["_ID"].cpu().numpy()
    batch = rows(nodes, times)
    assert np.array_equal(batch, rows(nodes, times)), "the same call twice"
    busy = [i for i in np.argsort(-np.diff(ip)[nodes]) if (batch[i] >= 0).sum() == 10][:3]
    assert len(busy) == 3
    for i in busy:
        assert np.array_equal(rows(nodes[i: i + 1], times[i: i + 1])[0], batch[i]), "alone"
    order = np.random.default_rng(0).permutation(512)
    assert np.array_equal(rows(nodes[order], times[order]), batch[order]), "another place in the batch"
    other = times.copy()                                    # other seed times move the slot index of the rows that keep theirs
    other[128:400] = np.random.default_rng(1).integers(0, T_MAX, size=272)
    kept = np.r_[0:128, 400:512]
    assert np.array_equal(rows(nodes, other)[kept], batch[kept]), "another slot index"


# ------------------------------------------------------------------------------------------------ 5. handle reuse
def test_temporal_calls_leave_the_handle_as_they_found_it(hiplib):
    """About 30 random calls on one handle -- temporal (both strategies), uniform fixed, uniform with -1 layers -- whose sizes sit on the
    lane-group, block and tile edges: every temporal result equals the reference, every uniform one the result of a fresh handle."""
    import torch
    from COALA_GNN.sampler import NeighborSampler, TemporalNeighborSampler
    from COALA_GNN.synthetic import edge_times, powerlaw_csc
    d_ip, d_ix = powerlaw_csc(20_000, 12, seed=3, device="cuda", max_degree=300)
    d_ts = edge_times(d_ip, seed=1, t_max=5000)
    g = TemporalNeighborSampler.make_graph(d_ip, d_ix, edata={"ts": d_ts})
    ip, ix, ts = d_ip.cpu().numpy(), d_ix.cpu().numpy(), d_ts.cpu().numpy()
    host = (ip, ix, ts, row_index(ip, ts))
    rng = np.random.default_rng(17)
    sizes = (0, 1, 2, 63, 64, 65, 255, 256, 257, 512)
    kinds = []
    for i in range(30):
        n = int(sizes[rng.integers(0, len(sizes))])
        nodes = rng.permutation(20_000)[:n].astype(np.int64)
        kind = ("temporal", "uniform", "full")[i % 3] if i < 24 else ("temporal", "temporal", "uniform")[i % 3]
        kinds.append(kind)
        if kind == "temporal":
            fan = [[10], [5, 5], [32, 1], [2, 5, 7], [1], [3, 3, 3, 3]][int(rng.integers(0, 6))]
            smp = TemporalNeighborSampler(fan, strategy=("uniform", "last")[int(rng.integers(0, 2))], inclusive=bool(rng.integers(0, 2)),
                                          seed=int(rng.integers(0, 100)), edge_ids=bool(rng.integers(0, 2)))
            _check_call(smp, g, host, nodes, rng.integers(-10, 5010, size=n).astype(np.int64), step=i)
            continue
        fan = [[10], [5, 5], [15, 10, 5]][int(rng.integers(0, 3))] if kind == "uniform" else [[-1], [3, -1], [-1, 4]][int(rng.integers(0, 3))]
        if kind == "full":
            nodes = nodes[:64]
        seeds = torch.from_numpy(nodes).cuda()
        eids = bool(rng.integers(0, 2))
        got = NeighborSampler(fan, seed=i, edge_ids=eids).sample(g, seeds, step=i)
        fresh = NeighborSampler.make_graph(d_ip, d_ix)
        want = NeighborSampler(fan, seed=i, edge_ids=eids).sample(fresh, seeds, step=i)
        for b, w in zip(got[2], want[2]):
            assert torch.equal(b.src_nodes, w.src_nodes), (i, kind, fan)
            for name in ("nbr", "indptr", "indices"):
                x, y = getattr(b, name), getattr(w, name)
                assert (x is None and y is None) or torch.equal(x, y), (i, kind, fan, name)
            if eids:
                assert torch.equal(b.edata["_ID"], w.edata["_ID"])
        fresh.close()
    assert kinds.count("temporal") >= 10 and kinds.count("uniform") >= 8 and kinds.count("full") >= 8
    g.close()


# ------------------------------------------------------------------------------------------------ 6. loader
def test_loader_with_temporal_sampler(hiplib, oracle, tmp_path):
    """A short COALA_GNN_DataLoader epoch with TemporalNeighborSampler(seed_time='t'): the query times come from graph.ndata, the rows
    delivered are the table's rows of input_nodes -- repeated ids included -- and the blocks are the reference's."""
    import torch
    from _util import ColorFiles
    from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, SSD_INFO
    from COALA_GNN.sampler import TemporalNeighborSampler
    from COALA_GNN.synthetic import alloc_pinned_table, block_colors, edge_times, feature_rows_torch, powerlaw_csc
    n_nodes, dim, batch = 20000, 64, 64
    table = alloc_pinned_table(n_nodes, dim, seed=3, device=0)
    indptr, indices = powerlaw_csc(n_nodes, 8.0, seed=1, device="cuda")
    d_ts = edge_times(indptr, seed=2, t_max=1000)
    labels = (torch.arange(n_nodes, device="cuda") * 7) % 5
    node_t = 200 + (torch.arange(n_nodes, device="cuda") * 13) % 700
    color, tk, sc, _ = block_colors(n_nodes, nodes_per_color=512)
    files = ColorFiles(tmp_path, color, tk, sc)
    comm = MPI_Comm_Manager(0)
    comm.initialize_nested_process_group("isolated")
    train_ids = torch.randperm(int(0.6 * n_nodes), generator=torch.Generator().manual_seed(0))[:64 * 3]
    nd = Node_Distributor(comm, train_ids, batch, files.color_file, files.topk_file, files.score_file, parsing_method="baseline")
    sampler = TemporalNeighborSampler([5, 5], seed_time="t", seed=5)
    g = sampler.make_graph(indptr, indices, ndata={"labels": labels, "t": node_t}, edata={"ts": d_ts})
    loader = COALA_GNN_DataLoader(SSD_INFO(1, dim * 4, 1024, 0), nd, g, sampler, batch, dim, sampler.fanouts, 4, "cuda:0", refresh_counter=3,
                                  cache_backend="isolated", sim_buf=table, num_rows=n_nodes, prefetch=1)
    ip, ix, ts = indptr.cpu().numpy(), indices.cpu().numpy(), d_ts.cpu().numpy()
    index = row_index(ip, ts)
    steps = repeats = 0
    for input_nodes, seeds, blocks, feat in loader:
        assert torch.equal(feat, feature_rows_torch(input_nodes, dim, 3)), "the rows of input_nodes, repeated ids included"
        repeats += len(input_nodes) - len(torch.unique(input_nodes))
        assert all(b.nbr is not None and b.nbr.shape[1] == 5 for b in blocks) and blocks[-1].num_dst == batch
        s = seeds.cpu().numpy()
        ref, slot_time = reference_layers(ip, ix, ts, s, node_t.cpu().numpy()[s], [5, 5], 5, steps, index=index)
        nodes_r, times_r = decode(ref[-1][0], slot_time, n_nodes)
        assert np.array_equal(input_nodes.cpu().numpy(), nodes_r) and np.array_equal(blocks[0].src_times.cpu().numpy(), times_r)
        assert np.array_equal(blocks[0].nbr.cpu().numpy(), ref[-1][1]) and np.array_equal(blocks[0].edata["_ID"].cpu().numpy(), ref[-1][2])
        assert torch.equal(blocks[-1].dstdata["labels"], labels[seeds]) and torch.equal(blocks[-1].dst_times, node_t[seeds])
        steps += 1
    assert steps >= 1 and repeats > 0
    del loader
    table.close()
