"""GPU tests of the record sample_begin hands to sample_end (COALA_GNN.sampler._Pending), for every sampler kind: a sampler object keeps
nothing of a call, so calls begun back to back and ended out of order give what each gives alone; and the record names the owner counts
the loader sends ahead."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, N_SEEDS, FANOUTS, HUBS = 200, 16, [3, 2], (7, 123)


@pytest.fixture(scope="module")
def graph(hiplib):
    """200 nodes of mean in-degree 8 and two hub rows of degree 150 (the long rows of a ragged layer), distinct neighbours in every row.
    Edge types (3 relations) are sorted inside every row and the timestamp of an edge is its place in its row, so one graph serves the
    relation and the temporal samplers; ndata['qt'] holds a query time per node."""
    import torch
    from COALA_GNN.sampler import CSCGraph, sort_csc_by_etype
    rng = np.random.default_rng(3)
    deg = rng.poisson(8.0, size=N)
    deg[list(HUBS)] = 150
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = np.concatenate([np.sort(rng.choice(N, size=d, replace=False)) for d in deg]).astype(np.int64)
    E = int(ip[-1])
    indptr, indices = torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda()
    indices, etype, _ = sort_csc_by_etype(indptr, indices, torch.from_numpy(rng.integers(0, 3, size=E)).cuda())
    ts = torch.arange(E, device="cuda") - torch.repeat_interleave(indptr[:-1], indptr[1:] - indptr[:-1])
    g = CSCGraph(indptr, indices, ndata={"labels": torch.arange(N, device="cuda") % 7, "qt": torch.from_numpy(rng.integers(1, 160, size=N)).cuda()},
                 edata={"w": torch.from_numpy(rng.random(E).astype(np.float32)).cuda(), "etype": etype, "ts": ts})
    yield g
    g.close()


def _kinds():
    from COALA_GNN.sampler import (EdgePredictionSampler, LaborSampler, NeighborSampler, RandomWalkNeighborSampler, RelNeighborSampler,
                                   TemporalEdgePredictionSampler, TemporalNeighborSampler, UniformNegativeSampler)
    return {   # name -> (a fresh sampler, whether its seeds are edges)
        "plain": (lambda: NeighborSampler(FANOUTS, seed=5), False),
        "prob": (lambda: NeighborSampler(FANOUTS, seed=5, prob="w"), False),
        "edge_ids": (lambda: NeighborSampler(FANOUTS, seed=5, edge_ids=True), False),
        "full_layer": (lambda: NeighborSampler([3, -1], seed=5), False),
        "labor": (lambda: LaborSampler(FANOUTS, seed=5), False),
        "rel": (lambda: RelNeighborSampler(FANOUTS, 3, seed=5), False),
        "walk": (lambda: RandomWalkNeighborSampler(FANOUTS, 2, 0.5, 8, seed=5), False),
        "temporal": (lambda: TemporalNeighborSampler(FANOUTS, seed_time="qt", seed=5), False),
        "edge_prediction": (lambda: EdgePredictionSampler(NeighborSampler(FANOUTS, seed=5), exclude="self", negative_sampler=UniformNegativeSampler(2)), True),
        "temporal_edge_prediction": (lambda: TemporalEdgePredictionSampler(TemporalNeighborSampler(FANOUTS, seed=5),
                                                                           negative_sampler=UniformNegativeSampler(2)), True),
    }


KINDS = ["plain", "prob", "edge_ids", "full_layer", "labor", "rel", "walk", "temporal", "edge_prediction", "temporal_edge_prediction"]


def _tensors(out):
    """Every tensor of a sample() result by name: the input nodes, the seeds or the EdgeBatch, every block tensor and edata entry."""
    import torch
    input_nodes, seeds, blocks = out
    t = {"input_nodes": input_nodes}
    if isinstance(seeds, torch.Tensor):
        t["seeds"] = seeds
    else:
        t.update({f"batch.{k}": getattr(seeds, k) for k in ("eids", "seed_nodes", "pos_src", "pos_dst", "neg_src", "neg_dst", "seed_times")})
    for i, b in enumerate(blocks):
        t[f"{i}.num"] = torch.tensor([b.num_src, b.num_dst])
        for k in ("src_nodes", "nbr", "indptr", "indices", "dst_in_src", "owner_counts", "src_times", "dst_times"):
            t[f"{i}.{k}"] = getattr(b, k, None)
        for name, d in (("srcdata", b.srcdata), ("dstdata", b.dstdata), ("edata", b.edata)):
            for k in list(d.keys()):     # edata: also the entries made on first access, and graph.edata through the edge ids
                t[f"{i}.{name}.{k}"] = d[k]
    return t


@pytest.mark.parametrize("kind", KINDS)
def test_calls_begun_together_and_ended_out_of_order_equal_single_calls(graph, kind):
    import torch
    make, by_edge = _kinds()[kind]
    gen = torch.Generator().manual_seed(9)
    if by_edge:
        seeds = [torch.randperm(graph.num_edges, generator=gen)[:N_SEEDS].cuda() for _ in range(3)]
    else:   # both hubs among the seeds: the ragged layers have their long rows
        rest = [r[(r != HUBS[0]) & (r != HUBS[1])][: N_SEEDS - 2] for r in (torch.randperm(N, generator=gen) for _ in range(3))]
        seeds = [torch.cat([r[:5], torch.tensor(HUBS), r[5:]]).cuda() for r in rest]
    smp = make()
    pending = [smp.sample_begin(graph, seeds[i], step=i) for i in range(3)]
    got = {i: _tensors(smp.sample_end(pending[i])) for i in (1, 0, 2)}
    n_edges = 0
    for i in range(3):
        alone = make().sample(graph, seeds[i], step=i)
        want = _tensors(alone)
        assert got[i].keys() == want.keys(), f"step {i}"
        for k, w in want.items():
            assert (got[i][k] is None) == (w is None), f"step {i}: {k}"
            if w is not None:
                assert got[i][k].dtype == w.dtype and torch.equal(got[i][k], w), f"step {i}: {k}"
        n_edges += sum(int(b.in_degrees().sum()) for b in alone[2])
    assert n_edges > 0
    assert not any(torch.equal(got[0]["input_nodes"], got[i]["input_nodes"]) for i in (1, 2)), "the steps must differ for the order to matter"


@pytest.mark.parametrize("wrapped", [False, True], ids=["plain", "edge_prediction"])
def test_pending_names_the_owner_counts(graph, wrapped):
    import torch
    from COALA_GNN.sampler import EdgePredictionSampler, NeighborSampler
    G = 4
    for parts in (G, 0):
        smp = NeighborSampler(FANOUTS, seed=5, bucket_by_owner=parts)
        seeds = torch.arange(N_SEEDS, device="cuda") * 11
        if wrapped:
            smp = EdgePredictionSampler(smp)
        pending = smp.sample_begin(graph, seeds)
        counts = pending.owner_counts
        if not parts:
            assert counts is None and smp.sample_end(pending)[2][0].owner_counts is None
            continue
        assert isinstance(counts, torch.Tensor) and counts.is_cuda and counts.dtype == torch.int64 and tuple(counts.shape) == (G,)
        ptr = counts.data_ptr()
        input_nodes, _, blocks = smp.sample_end(pending)
        b = blocks[0]
        assert b.owner_counts.data_ptr() == ptr == pending.owner_counts.data_ptr()
        ids = input_nodes.cpu().numpy()
        assert b.owner_counts.cpu().tolist() == b.owner_counts_host == [int((ids % G == o).sum()) for o in range(G)]
        assert sum(b.owner_counts_host) == b.num_src > 0
