"""GPU test of what a sampler handle carries from call to call -- the clean extent of the hash table, the scan ticket and generation, the
shared scratch, the ring of pinned slots -- under edge batches, walk batches and node samples mixed on one handle: a full ring of eight
calls that nobody waits for, on two streams, collected backwards; a ticket that has left the ring; the handle after all that.  Every
result bit for bit: edge batches against tests/_edge_batch_ref.py, walk batches against tests/_node2vec_ref.py, node samples against a
second handle on the same graph that never sees a batch.

The graph is test_edge_batch_gpu.py's link graph with every row sorted by source id (what _node2vec_ref.edge_graph does to its graph):
the first walk batch has q != 1, which the walk kernel's near test (a binary search) and sampler.walk_batch_begin demand sorted rows
for.  Degrees, the hub and the degree-0 runs are the link graph's own.

NeighborSampler takes its fan-outs in DGL's order, input layer first, and samples the last one first: [-1, 2] puts a ragged layer behind
a fixed one, and the ninth call, [2, -1], is the sample whose first layer is ragged -- right behind a batch, whose clean extent it
inherits."""
import ctypes as C

import numpy as np
import pytest

import _edge_batch_ref as RE
import _node2vec_ref as RW

pytestmark = pytest.mark.gpu

RING = 8    # calls a handle keeps collectable (coala_sampler.hip: kRing)
# the eight calls, in order; walk: (n, W, L, K, p, q, out-of-range start nodes), edge: (n, k), node: (fanouts, seeds, bucket_by_owner)
CALLS = [("walk", 65, 3, 6, 2, 0.5, 2, True), ("edge", 1025, 5), ("node", [-1, 2], 64, 0), ("edge", 0, 1), ("walk", 0, 1, 1, 1, 1, 1, False),
         ("walk", 1024, 2, 12, 1, 1, 1, False), ("node", [5, 5], 300, 4), ("edge", 1, 64)]
NINTH = ("node", [2, -1], 64, 0)
SEED = 7


class _Ring(object):
    """The graph, both handles, and the begin / end / reference of a call by its CALLS entry and its step."""

    def __init__(self, torch):
        self.torch = torch
        ip, ix, _ = RE.link_graph(n_plain=2000, hub_degree=5000, seed=5)
        ix = np.concatenate([np.sort(ix[ip[v]: ip[v + 1]]) for v in range(len(ip) - 1)])
        self.ip, self.ix, self.N, self.E = ip, ix, len(ip) - 1, len(ix)
        from COALA_GNN.sampler import CSCGraph
        self.g = CSCGraph(torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda())
        self.clean = CSCGraph(self.g.indptr, self.g.indices)
        self.side = torch.cuda.Stream()

    def inputs(self, call, i):
        """The call's seed edges / start nodes / seed nodes: int64 numpy, a function of the call and its step."""
        rng = np.random.default_rng(1000 + i)
        if call[0] == "edge":
            e = rng.integers(0, self.E, size=call[1]).astype(np.int64)
            if len(e) > 2:
                e[-1] = e[1]                       # a repeated seed edge
            return e
        if call[0] == "walk":
            v = rng.integers(0, self.N, size=call[1]).astype(np.int64)
            if call[7]:
                v[[1, len(v) // 2]] = [-1, self.N]
            return v
        return rng.permutation(self.N)[: call[2]].astype(np.int64)

    def sampler(self, call):
        from COALA_GNN.sampler import NeighborSampler
        return NeighborSampler(call[1], seed=SEED, bucket_by_owner=call[3])

    def begin(self, call, i, x):
        """Enqueue call number i over the device tensor x on the stream of its turn, without waiting -> what end() takes."""
        from COALA_GNN.sampler import edge_batch, walk_batch_begin
        with self.torch.cuda.stream(self.side if i % 2 else None):
            if call[0] == "edge":
                return edge_batch(self.g, x, call[2], seed=SEED, step=i)
            if call[0] == "walk":
                return walk_batch_begin(self.g, x, call[5], call[6], call[3], num_walks=call[2], num_neg=call[4], seed=SEED, step=i, traces=True)
            return self.sampler(call).sample_begin(self.g, x, step=i)

    def end(self, call, pending):
        """Collect a call -> dict of numpy arrays (a node sample: a list of torch tensors and Nones)."""
        from COALA_GNN.sampler import edge_batch_wait, walk_batch_end
        from COALA_GNN_Pybind import _capi
        if call[0] == "edge":
            n_nodes, n_bad = C.c_int64(-1), C.c_int64(-1)
            _capi.check(_capi.load().coala_sampler_edge_batch_wait(self.g._h, pending[-1], C.byref(n_nodes), C.byref(n_bad)))
            b = edge_batch_wait(pending)
            assert b.seed_nodes.numel() == n_nodes.value
            return dict(seed_nodes=b.seed_nodes.cpu().numpy(), pos_src=b.pos_src.cpu().numpy(), pos_dst=b.pos_dst.cpu().numpy(),
                        neg_dst=b.neg_dst.cpu().numpy().reshape(call[1], call[2]), n_bad=n_bad.value)
        if call[0] == "walk":
            b = walk_batch_end(pending)
            return dict(input_nodes=b.input_nodes.cpu().numpy(), pos=b.pos.cpu().numpy(), neg=b.neg.cpu().numpy(), traces=b.traces.cpu().numpy(),
                        n_bad=b.n_bad)
        return self.flat(self.sampler(call).sample_end(pending))

    @staticmethod
    def flat(sample):
        out = [sample[0]]
        for b in sample[2]:
            out += [b.src_nodes, b.nbr, b.indptr, b.indices, b.dst_in_src]
        return out

    def want(self, call, i, x):
        if call[0] == "edge":
            return RE.edge_batch(self.ip, self.ix, x, call[2], seed=SEED, step=i)
        if call[0] == "walk":
            return RW.walk_batch(self.ip, self.ix, x, call[3], call[2], call[4], RW.thresholds(call[5], call[6]), seed=SEED, step=i)
        return self.flat(self.sampler(call).sample(self.clean, self.torch.from_numpy(x).cuda(), step=i))

    def same(self, call, got, want):
        if call[0] == "node":
            assert len(got) == len(want)
            for t, u in zip(got, want):
                assert (t is None) == (u is None) and (t is None or self.torch.equal(t, u))
            return
        for key in want:
            if key == "n_bad":
                assert got[key] == want[key]
            else:
                assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key

    def close(self):
        self.g.close()
        self.clean.close()


@pytest.fixture(scope="module")
def run(hiplib):
    """The whole sequence on one handle, run once: -> (the _Ring, per phase what the tests compare).  Nothing is asserted here but that
    the calls themselves succeed."""
    import torch
    from COALA_GNN_Pybind import _capi
    lib = _capi.load()
    r = _Ring(torch)
    calls = CALLS + [NINTH, CALLS[0], CALLS[1]]
    steps = list(range(RING + 1)) + [0, 1]         # the last two repeat the first two, step included
    xs = [r.inputs(c, i) for c, i in zip(calls, steps)]
    dev = [torch.from_numpy(x).cuda() for x in xs]
    wants = [r.want(c, i, x) for c, i, x in zip(calls, steps, xs)]      # the references, before the handle under test sees a call
    torch.cuda.synchronize()
    out = dict(wants=wants)
    pend = [r.begin(calls[j], steps[j], dev[j]) for j in range(RING)]  # a full ring that nobody has waited for ...
    got = [None] * RING
    for j in reversed(range(RING)):                                     # ... collected backwards
        got[j] = r.end(calls[j], pend[j])
    out["ring"] = got
    ninth = r.begin(calls[RING], steps[RING], dev[RING])
    first = pend[0][-1]                                                 # the first call's ticket: nine calls ago
    cnt = (C.c_int64 * 8)()
    out["left"] = []
    for wait in (lambda: lib.coala_sampler_wait(r.g._h, first, cnt, None), lambda: lib.coala_sampler_edge_batch_wait(r.g._h, first, cnt, None),
                 lambda: lib.coala_sampler_walk_batch_wait(r.g._h, first, cnt, None)):
        out["left"].append((wait(), _capi.last_error()))
    out["ninth"] = r.end(calls[RING], ninth)
    out["again"] = [r.end(calls[j], r.begin(calls[j], steps[j], dev[j])) for j in (RING + 1, RING + 2)]
    yield r, calls, out
    r.close()


def test_a_full_ring_collected_backwards(run):
    r, calls, out = run
    for j in range(RING):
        r.same(calls[j], out["ring"][j], out["wants"][j])
    assert out["ring"][0]["n_bad"] == 2
    for j in (3, 4):                                                    # the two empty batches
        nodes = out["ring"][j]["seed_nodes" if calls[j][0] == "edge" else "input_nodes"]
        assert nodes.shape == (0,) and out["ring"][j]["n_bad"] == 0


def test_a_ticket_that_has_left_the_ring(run):
    from COALA_GNN_Pybind import _capi
    r, calls, out = run
    assert len(out["left"]) == 3
    for rc, msg in out["left"]:
        assert rc == _capi.EINVAL and "not one of the last 8 calls" in msg
    r.same(calls[RING], out["ninth"], out["wants"][RING])


def test_the_handle_stays_usable(run):
    r, calls, out = run
    for k, j in enumerate((RING + 1, RING + 2)):
        r.same(calls[j], out["again"][k], out["wants"][j])
        r.same(calls[j], out["again"][k], out["ring"][k])                # the same tensors as the first time
