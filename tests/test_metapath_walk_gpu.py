"""GPU tests of the metapath walks (metapath_trace / metapath_select / metapath_items in coala_sampler.hip), bit for bit against
tests/_metapath_ref.py.  Two graphs.  "typed": 3 relations, 700 plain rows of 0..12 edges, among them rows that lack type 1, rows whose
type 0 is their first edge alone and rows whose type 2 is their last edge alone, then a row of 300 edges (three steps of the 16-lane
search) and a hub of 5,000, both reachable from the plain rows.  "bipartite": synthetic.bipartite_csc(40, 60, 4), users first."""
import numpy as np
import pytest

import _metapath_ref as MP
import _node2vec_ref as RW
import _pinsage_ref as RP

pytestmark = pytest.mark.gpu

PATHS = {"typed": {1: [1], 2: [2, 0], 3: [0, 1, 2]}, "bipartite": {1: [0], 2: [0, 1], 3: [0, 1, 0]}}


def _typed_graph():
    rng = np.random.default_rng(11)
    N, cols, types = 702, [], []
    for v in range(N - 2):
        d = int(rng.integers(0, 13))
        t = np.sort(rng.integers(0, 3, d))
        t = t[t != 1] if v % 7 == 0 else t
        t = np.r_[0, np.full(d - 1, 2)] if d and v % 11 == 0 else np.r_[np.full(d - 1, 0), 2] if d and v % 13 == 0 else t
        c = rng.integers(0, N, len(t))
        c[:(v % 5 == 0)] = N - 1 - (v // 5) % 2          # every fifth row's first edge comes from the hub or the 300-edge row
        cols.append(c)
        types.append(t)
    for d in (300, 5000):
        cols.append(rng.integers(0, N, d))
        types.append(np.sort(rng.integers(0, 3, d)))
    ip = np.zeros(N + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cols], out=ip[1:])
    return ip, np.concatenate(cols).astype(np.int64), np.concatenate(types).astype(np.int64)


@pytest.fixture(scope="module")
def graphs(hiplib):
    """name -> (device graph with edata['etype'], the reference's TypedGraph, 300 start nodes: a repeat, -1 and num_nodes among them)."""
    import torch
    from COALA_GNN.sampler import CSCGraph
    from COALA_GNN.synthetic import bipartite_csc
    out = {}
    for name, (ip, ix, et) in (("typed", _typed_graph()), ("bipartite", tuple(t.numpy() for t in bipartite_csc(40, 60, 4, seed=1)))):
        N = len(ip) - 1
        nodes = np.concatenate([[N - 1, N - 2, -1, N, N - 1], np.random.default_rng(N).integers(0, N, 295)]).astype(np.int64)
        g = CSCGraph(torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda(), edata={"etype": torch.from_numpy(et).cuda()})
        out[name] = (g, MP.TypedGraph(ip, ix, et), nodes)
    yield out
    for g, _, _ in out.values():
        g.close()


@pytest.mark.parametrize("name", ["typed", "bipartite"])
@pytest.mark.parametrize("restart", [0.0, 0.5])
@pytest.mark.parametrize("M,length,W", [(1, 3, 1), (2, 4, 5), (3, 6, 64), (2, 16, 3)])
def test_traces(graphs, name, restart, M, length, W):
    import torch
    from COALA_GNN.sampler import random_walk
    g, G, nodes = graphs[name]
    got = random_walk(g, torch.from_numpy(nodes).cuda(), length, restart, W, seed=7, step=3, metapath=PATHS[name][M]).cpu().numpy()
    want = MP.traces(G, nodes, PATHS[name][M], length, W, RP.threshold(restart), 7, 3)
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} walks differ"
    assert len(nodes) % 256 and np.all(want[2:4] == -1) and np.array_equal(want[0], want[4]) and (want[:, :, min(M, 2)] >= 0).any()


def test_one_relation_is_the_untyped_walk(graphs):
    """All edges of one type: metapath=[0] gives the untyped traces and the untyped sampler's blocks, bit for bit."""
    import torch
    from COALA_GNN.sampler import CSCGraph, RandomWalkNeighborSampler, random_walk
    g0, _, nodes = graphs["typed"]
    g = CSCGraph(g0.indptr, g0.indices, edata={"etype": torch.zeros(g0.num_edges, dtype=torch.int16, device="cuda")})
    d_nodes, seeds = torch.from_numpy(nodes).cuda(), torch.from_numpy(np.unique(nodes[nodes >= 0])).cuda()
    for length, restart, W in ((16, 0.25, 64), (1, 0.0, 1)):
        assert torch.equal(random_walk(g, d_nodes, length, restart, W, seed=2, step=9, metapath=[0]), random_walk(g, d_nodes, length, restart, W, seed=2, step=9))
    typed = RandomWalkNeighborSampler([5, 3], 4, 0.3, 20, seed=6, metapath=[0]).sample(g, seeds, step=1)
    plain = RandomWalkNeighborSampler([5, 3], 4, 0.3, 20, seed=6).sample(g, seeds, step=1)
    for a, b in zip(typed[2], plain[2]):
        assert torch.equal(a.src_nodes, b.src_nodes) and torch.equal(a.nbr, b.nbr) and torch.equal(a.edata["visit_counts"], b.edata["visit_counts"])
    g.close()


@pytest.mark.parametrize("name", ["typed", "bipartite"])
@pytest.mark.parametrize("k,R,W,M", [(3, 2, 10, 2), (32, 8, 64, 2), (5, 1, 16, 3)])
def test_walk_layers(graphs, name, k, R, W, M):
    """Two layers: Block.nbr, the visit counts and the source lists.  On the bipartite graph a walk of [0, 1] from an item records items."""
    import torch
    from COALA_GNN.sampler import RandomWalkNeighborSampler
    g, G, nodes = graphs[name]
    seeds = np.concatenate([np.unique(nodes[nodes >= 0])[:: 1 if k < 32 else 6], [-1]])     # distinct; users and items alike; a bad id
    _, _, blocks = RandomWalkNeighborSampler([k, k], R, 0.5, W, seed=3, metapath=PATHS[name][M]).sample(g, torch.from_numpy(seeds).cuda(), step=4)
    ref = MP.reference_layers(G, seeds, [k, k], PATHS[name][M], R, W, RP.threshold(0.5), 3, 4)
    for l, (src_r, loc_r, cnt_r, _) in enumerate(ref):
        b = blocks[1 - l]
        assert np.array_equal(b.src_nodes.cpu().numpy(), src_r), f"layer {l}: source list"
        assert np.array_equal(b.nbr.cpu().numpy(), loc_r), f"layer {l}: nbr"
        assert np.array_equal(b.edata["visit_counts"].cpu().numpy(), cnt_r), f"layer {l}: visit counts"
    assert (ref[0][3] >= 0).any() and np.all(ref[0][3][-1] == -1)
    if name == "bipartite" and M == 2:
        nbr = blocks[1].nbr.cpu().numpy()[seeds >= 40]
        reached = blocks[1].src_nodes.cpu().numpy()[np.maximum(nbr, 0)]
        assert np.all((reached >= 40) | (nbr < 0)) and (nbr >= 0).any(), "an item's neighbour is an item"


@pytest.mark.parametrize("name", ["typed", "bipartite"])
@pytest.mark.parametrize("M,L,W,K", [(2, 6, 2, 1), (3, 127, 1, 16)])
def test_walk_batch(graphs, name, M, L, W, K):
    import torch
    from COALA_GNN.sampler import walk_batch
    g, G, nodes = graphs[name]
    b = walk_batch(g, torch.from_numpy(nodes[:40]).cuda(), walk_length=L, num_walks=W, num_neg=K, seed=5, step=2, traces=True, metapath=PATHS[name][M])
    want = MP.walk_batch(G, nodes[:40], PATHS[name][M], L, W, K, 5, 2)
    for key in ("input_nodes", "pos", "neg", "traces"):
        assert np.array_equal(getattr(b, key).cpu().numpy(), want[key]), key
    assert b.n_bad == want["n_bad"] == 2


def test_metapath2vec_loss(graphs):
    """One forward and backward of MetaPath2Vec.loss: finite, and within twice the fp32 fallback's distance from the float64 loss and
    gradient (the bound of tests/test_skipgram_loss_gpu.py and tests/test_node2vec_model_gpu.py)."""
    import torch
    from COALA_GNN import MetaPath2Vec, block_ops
    torch.manual_seed(4)
    g, G, nodes = graphs["typed"]
    model = MetaPath2Vec(g, 16, [0, 1, 2], walk_length=10, context_size=5, walks_per_node=2, num_negative_samples=1, cache_mb=1, device="cuda:0", seed=3)
    start = np.unique(nodes[nodes >= 0])[:128]
    batch = model.sample(torch.from_numpy(start).cuda(), step=0)
    assert np.array_equal(batch.pos.cpu().numpy(), MP.walk_batch(G, start, [0, 1, 2], 10, 2, 1, 3, 0)["pos"])
    w0 = model.embedding.weight_host.numpy()[batch.input_nodes.cpu().numpy()].copy()
    loss = model.loss(batch)
    loss.backward()
    (_, leaf), = model.embedding.trace
    ref_loss, ref_grad = RW.skipgram_loss(w0, batch.pos.cpu().numpy(), batch.neg.cpu().numpy(), 5)
    low_h = torch.from_numpy(w0).cuda().requires_grad_(True)
    low = block_ops.skipgram_loss_torch(low_h, batch.pos, batch.neg, 5)
    low.backward()
    d_l, e_l = abs(float(low.detach()) - ref_loss), abs(float(loss.detach()) - ref_loss)
    d_g, e_g = (float(np.abs(t.grad.cpu().numpy().astype(np.float64) - ref_grad).max()) for t in (low_h, leaf))
    print(f"loss {ref_loss:.6f}; fallback fp32 distance loss {d_l:.3e} grad {d_g:.3e} | native loss {e_l:.3e} grad {e_g:.3e}")
    assert np.isfinite(float(loss.detach())) and bool(torch.isfinite(leaf.grad).all()) and e_l <= 2.0 * d_l and e_g <= 2.0 * d_g
    model.close()


@pytest.mark.parametrize("kernel", ["trace", "select", "items"])
def test_second_grid_pass(graphs, kernel):
    """Each typed kernel past one pass of its largest grid (8,192 blocks): 32,770 x 64 walks of a thread each; 131,080 rows of 16 lanes;
    2,050 x 64 walks of 16 lanes.  The start nodes repeat 200 ids, and a repeated id has the same walks."""
    import torch
    from COALA_GNN.sampler import RandomWalkNeighborSampler, random_walk, walk_batch
    g, G, nodes = graphs["typed"]
    start = np.resize(np.unique(nodes[nodes >= 0])[:200], {"trace": 32_770, "select": 131_080, "items": 2_050}[kernel])
    d_start = torch.from_numpy(start).cuda()
    if kernel == "trace":
        assert np.array_equal(random_walk(g, d_start, 2, 0.0, 64, seed=1, step=1, metapath=[2, 0]).cpu().numpy(), MP.traces(G, start, [2, 0], 2, 64, 0, 1, 1))
    elif kernel == "select":
        _, _, (b,) = RandomWalkNeighborSampler(1, 1, 0.0, 1, seed=1, metapath=[1]).sample(g, d_start, step=1)
        hop, nbr = MP.traces(G, start, [1], 1, 1, 0, 1, 1)[:, 0, 1], b.nbr.cpu().numpy()[:, 0]
        assert np.array_equal(np.where(nbr >= 0, b.src_nodes.cpu().numpy()[np.maximum(nbr, 0)], -1), hop)
        assert np.array_equal(b.edata["visit_counts"].cpu().numpy()[:, 0], (hop >= 0).astype(np.int32))
    else:
        b = walk_batch(g, d_start, walk_length=2, num_walks=64, num_neg=0, seed=1, step=1, traces=True, metapath=[0, 1])
        want = MP.walk_batch(G, start, [0, 1], 2, 64, 0, 1, 1)
        assert all(np.array_equal(getattr(b, key).cpu().numpy(), want[key]) for key in ("input_nodes", "pos", "traces"))
