"""Link prediction on a graph with time, on the GPU: TemporalEdgePredictionSampler over 256 seed edges with 3 negatives each.

Every seed edge is queried at its own timestamp, its endpoints and negatives become (node, time) pairs, and strictness alone keeps the
answer out of the blocks: no block holds an edge with a timestamp >= its row's query time, so no seed edge and no later edge."""
import numpy as np
import pytest

import _edge_batch_ref as ER

pytestmark = pytest.mark.gpu

N, IN, HID, EMB = 3000, 20, 12, 16
N_EDGES, K = 256, 3
SEED = 21


@pytest.fixture(scope="module")
def setup(hiplib):
    import torch
    from COALA_GNN.sampler import TemporalNeighborSampler, sort_csc_by_time
    ip, ix = ER.symmetric_graph(N, 8, seed=6)
    rng = np.random.default_rng(6)
    d_ip, d_ix = torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda()
    # timestamps in [0, 400): a busy row holds simultaneous edges, and many seed edges share a timestamp
    d_ix, d_ts, _ = sort_csc_by_time(d_ip, d_ix, torch.from_numpy(rng.integers(0, 400, size=len(ix))).cuda())
    g = TemporalNeighborSampler.make_graph(d_ip, d_ix, edata={"ts": d_ts})
    eids = rng.choice(len(ix), size=N_EDGES, replace=False).astype(np.int64)
    yield torch, g, ip, d_ix.cpu().numpy(), d_ts.cpu().numpy(), eids
    g.close()


@pytest.mark.parametrize("strategy", ["uniform", "last"])
def test_temporal_edge_batches(setup, strategy):
    torch, g, ip, ix, ts, eids = setup
    from COALA_GNN.harness import SAGE, LinkPredictor, link_loss
    from COALA_GNN.sampler import TemporalEdgePredictionSampler, TemporalNeighborSampler, UniformNegativeSampler
    inner = TemporalNeighborSampler([5, 5], strategy=strategy, seed=SEED)
    w = TemporalEdgePredictionSampler(inner, negative_sampler=UniformNegativeSampler(K))
    assert w.fanouts == [5, 5, 1 + K]
    input_nodes, batch, blocks = w.sample(g, torch.from_numpy(eids).cuda(), step=2)
    # ---- the pairs: the endpoints and negatives of the edge_batch kernels, each at its edge's timestamp
    want = ER.edge_batch(ip, ix, eids, K, seed=SEED, step=2)
    nodes, times = batch.seed_nodes.cpu().numpy(), batch.seed_times.cpu().numpy()
    rows = ER.brute_force_rows(ip)
    t_e = ts[eids]
    src_w, dst_w = want["seed_nodes"][want["pos_src"]], want["seed_nodes"][want["pos_dst"]]
    assert np.array_equal(src_w, ix[eids]) and np.array_equal(dst_w, rows[eids])
    for name, node_w, time_w in (("pos_src", src_w, t_e), ("pos_dst", dst_w, t_e),
                                 ("neg_dst", want["seed_nodes"][want["neg_dst"].reshape(-1)], np.repeat(t_e, K)),
                                 ("neg_src", np.repeat(src_w, K), np.repeat(t_e, K))):
        at = getattr(batch, name).cpu().numpy().astype(np.int64)
        assert getattr(batch, name).dtype == torch.int32 and np.array_equal(nodes[at], node_w) and np.array_equal(times[at], time_w), name
    code = times * (N + 1) + nodes
    assert len(np.unique(code)) == len(code) and (np.diff(code) > 0).all(), "distinct pairs, ascending by time and then node id"
    assert len(np.unique(nodes)) < len(nodes), "a node queried at two times is two seeds"
    assert torch.equal(blocks[-1].dstdata["_ID"], batch.seed_nodes) and torch.equal(blocks[-1].dst_times, batch.seed_times)
    assert input_nodes is blocks[0].src_nodes and batch.eids.cpu().numpy().tolist() == eids.tolist()
    # ---- no edge of any block is as recent as its row's query time: no seed edge, and no later edge
    d_ts = torch.from_numpy(ts).cuda()
    edges = 0
    for b in blocks:
        eid = b.edata["_ID"]
        valid = eid >= 0
        assert not bool((d_ts[eid.clamp_min(0)] >= b.dst_times.unsqueeze(1))[valid].any())
        edges += int(valid.sum())
    # a seed edge may still sit in a row queried at a LATER time (another seed edge's endpoint): never in a row at its own time or before
    for e in eids[:32]:
        hit = (blocks[-1].edata["_ID"] == int(e)).any(1)
        assert bool((blocks[-1].dst_times[hit] > int(ts[e])).all())
    assert edges > 1000
    # ---- one training step
    torch.manual_seed(0)
    model = LinkPredictor(SAGE(IN, HID, EMB, 2, aggregator_type="mean")).cuda()
    x = torch.randn(N, IN, device="cuda")[input_nodes]
    pos, neg = model(blocks, x, batch)
    assert pos.shape == (N_EDGES,) and neg.shape == (N_EDGES * K,)
    loss = link_loss(pos, neg)
    loss.backward()
    assert bool(torch.isfinite(loss)) and loss.item() > 0
    grads = [p.grad for p in model.parameters()]
    assert all(gr is not None and bool(torch.isfinite(gr).all()) for gr in grads) and any(float(gr.abs().max()) > 0 for gr in grads)
