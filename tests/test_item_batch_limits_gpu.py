"""GPU tests of the edge-batch, walk-batch and trace kernels past one pass of their grid-stride loops, across table sizes on one handle,
and exactly at the item limit (coala_sampler_edge_batch, _walk_batch, _node2vec_walk, _random_walk; coala_sampler.hip).

What each case crosses:
  edge_items_kernel, 8192 blocks of 256 threads, one item each          -> 2,100,003 items (700,001 edges, k = 1)
  clear_table inside edge_/walk_relabel_clear_kernel, 4096 blocks       -> a table of 2,097,152 slots (541,200 and 992,200 items)
  the relabel item loop, 4096 blocks                                     -> 1,049,600 entries of pos and neg (8,200 x 8 walks of 7 hops, K = 1)
  walk_items_kernel / node2vec_trace_kernel, 16 lanes per walk           -> 131,200 walks; 131,073 walks of one start node each
  walk_trace_kernel, a thread per walk                                   -> 2,097,280 walks
  scan_assign_kernel's look-back over kMaxTiles = 8192 status words      -> 8,388,608 items, accepted; one edge or node more, refused
  grow_workspace / prepare_table / clean_items                           -> small, large and small calls in turn on one handle, batches
                                                                            and node samples mixed, five of them in flight at once

Everything is integer arithmetic and compared bit for bit, at the C ABI with sentinel-padded buffers, against the numpy-uint64 forms of
the references (tests/_edge_batch_ref.py, tests/_node2vec_ref.py), which test_item_batch_large_cpu.py holds to the Python-integer forms.
The graph has 300,007 nodes so that the negatives of a large batch are mostly distinct and the compaction has millions of keys, not
millions of hits on a few thousand.  A reference is computed once and shared by the tests that need it.

A stale slot shows one call late: clear_table runs inside the relabel kernel and decides whether the NEXT call on the handle finds a
clean table, so the table cases run the batch, then the same nodes at other positions, then a small batch, all on one handle."""
import ctypes as C

import numpy as np
import pytest

import _edge_batch_ref as RE
import _node2vec_ref as RW
import _pinsage_ref as RP

pytestmark = pytest.mark.gpu

PAD = 37            # sentinel entries in front of and behind every output
S64, S32 = -0x0123456789ABCDEF, -0x01234567
ITEM_LIMIT = 8192 * 1024
SEED = 11


def _table_size(items):
    """coala_sampler.hip: table_size."""
    t = 1024
    while t < 2 * items:
        t <<= 1
    return t


class _Big(object):
    """The large graph on the device, the inputs of the named cases and their references (made on first use, then shared)."""

    def __init__(self, torch):
        from COALA_GNN.sampler import CSCGraph
        self.torch = torch
        self.ip, self.ix, self.hub, self.zeros = RE.large_graph(seed=3)
        self.N, self.E = len(self.ip) - 1, len(self.ix)
        deg = np.diff(self.ip)
        assert self.N == 300_007 and deg[self.hub] >= 4000 and np.all(deg[self.zeros] == 0)
        at = np.flatnonzero(self.ix == self.zeros[1])         # the rows that still name a degree-0 node: a walk from there may end in it
        assert len(at)
        self.above = int(np.searchsorted(self.ip, at[0], side="right") - 1)
        self.g = CSCGraph(torch.from_numpy(self.ip).cuda(), torch.from_numpy(self.ix).cuda())
        self._want = {}

    def handle(self):
        """A fresh handle on the same device arrays: no scratch, no table yet."""
        from COALA_GNN.sampler import CSCGraph
        return CSCGraph(self.g.indptr, self.g.indices)

    def eids(self, n, seed, bad=False):
        """First, last, the hub's first and last, a repeated eid, then random ones (one of them repeated); bad: -1 and E among them."""
        ip, hub = self.ip, self.hub
        special = np.array([0, self.E - 1, ip[hub], ip[hub + 1] - 1, 7, 7], dtype=np.int64)
        e = np.concatenate([special, np.random.default_rng(seed).integers(0, self.E, size=max(n - len(special), 0))])[:n].astype(np.int64)
        if n > len(special) + 2:
            e[-1] = e[-2]
        if bad:
            e[[len(special) + 1, n // 2]] = [-1, self.E]
        return e

    def starts(self, n, seed, bad=False):
        """The hub, the degree-0 nodes, a node one hop above one of them, a repeated node, then random ones; bad: -1 and N among them."""
        first = np.concatenate([[self.hub], self.zeros, [self.above, 9, 9]]).astype(np.int64)
        v = np.concatenate([first, np.random.default_rng(seed).integers(0, self.N, size=max(n - len(first), 0))])[:n].astype(np.int64)
        if bad:
            v[[len(first) + 1, n // 2]] = [-1, self.N]
        return v

    def want_edge(self, eids, k, step, name=None):
        if name is None or name not in self._want:
            w = RE.edge_batch(self.ip, self.ix, eids, k, SEED, step, draw=RE.negatives_vec)
            if name is None:
                return w
            self._want[name] = w
        return self._want[name]

    def want_walk(self, nodes, L, W, K, pq, step, name=None):
        if name is None or name not in self._want:
            w = RW.walk_batch_vec(self.ip, self.ix, nodes, L, W, K, RW.thresholds(*pq), SEED, step)
            if name is None:
                return w
            self._want[name] = w
        return self._want[name]

    # the named cases: (inputs, arguments); the same arrays every time, so a reference made by one test serves the others
    def case_31(self, bad=True):
        return self.eids(700_001, seed=31, bad=bad), 1, 3

    def case_32(self):
        return self.eids(8_200, seed=32), 64, 5

    def case_42(self):
        return self.starts(8_200, seed=42, bad=True), 7, 8, 1, (4, 0.25), 2

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def big(hiplib):
    import torch
    b = _Big(torch)
    yield b
    b.close()


# ------------------------------------------------------------------------------------------------------------- the C ABI, guarded
def _guarded(torch, sizes, dtypes, fills):
    return [torch.full((m + 2 * PAD,), s, dtype=dt, device="cuda") for m, dt, s in zip(sizes, dtypes, fills)]


def _check_guards(bufs, sizes, fills):
    for b, m, s in zip(bufs, sizes, fills):
        assert bool((b[:PAD] == s).all()) and bool((b[PAD + m:] == s).all()), "a write outside an output's capacity"


def _edge_begin(big, g, eids, k, step, d_e=None):
    """coala_sampler_edge_batch on sentinel-padded buffers, not waited for -> what _edge_end takes."""
    from COALA_GNN_Pybind import _capi, current_stream
    torch = big.torch
    n = len(eids)
    d_e = torch.from_numpy(eids).cuda() if d_e is None else d_e
    sizes, fills = (n * (2 + k), n, n, n * k), (S64, S32, S32, S32)
    bufs = _guarded(torch, sizes, (torch.int64, torch.int32, torch.int32, torch.int32), fills)
    out = _capi.EdgeBatchOut(*[b.data_ptr() + PAD * b.element_size() for b in bufs])
    ticket = C.c_int64(-1)
    rc = _capi.load().coala_sampler_edge_batch(g._h, d_e.data_ptr(), n, k, SEED, step, C.byref(out), C.byref(ticket), current_stream())
    return dict(rc=rc, err=_capi.last_error() if rc else "", ticket=ticket.value, bufs=bufs, sizes=sizes, fills=fills, n=n, k=k, keep=(d_e, out))


def _edge_end(big, g, st):
    from COALA_GNN_Pybind import _capi
    assert st["rc"] == 0, st["err"]
    n, k, bufs, sizes = st["n"], st["k"], st["bufs"], st["sizes"]
    n_nodes, n_bad = C.c_int64(-1), C.c_int64(-1)
    _capi.check(_capi.load().coala_sampler_edge_batch_wait(g._h, st["ticket"], C.byref(n_nodes), C.byref(n_bad)))
    _check_guards(bufs, sizes, st["fills"])
    assert 0 <= n_nodes.value <= sizes[0]
    assert bool((bufs[0][PAD + n_nodes.value: PAD + sizes[0]] == S64).all()), "seed_nodes written past n_nodes"
    host = [b[PAD: PAD + m].cpu().numpy() for b, m in zip(bufs, sizes)]
    return dict(seed_nodes=host[0][: n_nodes.value], pos_src=host[1], pos_dst=host[2], neg_dst=host[3].reshape(n, k), n_bad=n_bad.value)


def _edge(big, g, eids, k, step):
    return _edge_end(big, g, _edge_begin(big, g, eids, k, step))


def _walk_begin(big, g, nodes, L, W, K, pq, step, traces=True, d_n=None):
    """coala_sampler_walk_batch on sentinel-padded buffers, not waited for -> what _walk_end takes."""
    from COALA_GNN_Pybind import _capi, current_stream
    torch = big.torch
    n = len(nodes)
    d_n = torch.from_numpy(nodes).cuda() if d_n is None else d_n
    sizes = (n + n * W * (L + 1) + n * W * K * L, n * W * (L + 1), n * W * K * (L + 1), n * W * (L + 1))
    fills = (S64, S32, S32, S64)
    bufs = _guarded(torch, sizes, (torch.int64, torch.int32, torch.int32, torch.int64), fills)
    ptrs = [b.data_ptr() + PAD * b.element_size() for b in bufs]
    out = _capi.WalkBatchOut(ptrs[0], ptrs[1], ptrs[2], ptrs[3] if traces else None)
    ticket = C.c_int64(-1)
    rc = _capi.load().coala_sampler_walk_batch(g._h, d_n.data_ptr(), n, W, L, *RW.thresholds(*pq), K, SEED, step, C.byref(out), C.byref(ticket),
                                               current_stream())
    return dict(rc=rc, err=_capi.last_error() if rc else "", ticket=ticket.value, bufs=bufs, sizes=sizes, fills=fills, shape=(n, W, L, K),
                traces=traces, keep=(d_n, out))


def _walk_end(big, g, st):
    from COALA_GNN_Pybind import _capi
    assert st["rc"] == 0, st["err"]
    (n, W, L, K), bufs, sizes = st["shape"], st["bufs"], st["sizes"]
    n_nodes, n_bad = C.c_int64(-1), C.c_int64(-1)
    _capi.check(_capi.load().coala_sampler_walk_batch_wait(g._h, st["ticket"], C.byref(n_nodes), C.byref(n_bad)))
    _check_guards(bufs, sizes, st["fills"])
    assert 0 <= n_nodes.value <= sizes[0]
    assert bool((bufs[0][PAD + n_nodes.value: PAD + sizes[0]] == S64).all()), "input_nodes written past n_nodes"
    if not st["traces"]:
        assert bool((bufs[3] == S64).all())
    host = [b[PAD: PAD + m].cpu().numpy() for b, m in zip(bufs, sizes)]
    return dict(input_nodes=host[0][: n_nodes.value], pos=host[1].reshape(n * W, L + 1), neg=host[2].reshape(n * W * K, L + 1),
                traces=host[3].reshape(n, W, L + 1), n_bad=n_bad.value)


def _walk(big, g, nodes, L, W, K, pq, step, traces=True):
    return _walk_end(big, g, _walk_begin(big, g, nodes, L, W, K, pq, step, traces))


def _same(got, want, keys):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
    assert got["n_bad"] == want["n_bad"]


EDGE_KEYS = ("seed_nodes", "pos_src", "pos_dst", "neg_dst")
WALK_KEYS = ("input_nodes", "pos", "neg", "traces")


def _refused(st):
    """A call refused for its item count: COALA_EINVAL naming the items, the ticket untouched, not one word written."""
    from COALA_GNN_Pybind import _capi
    assert st["rc"] == _capi.EINVAL and "items" in st["err"] and st["ticket"] == -1
    for b, s in zip(st["bufs"], st["fills"]):
        assert bool((b == s).all()), "a refused call wrote to an output"


def _small_edge_still_exact(big, g):
    eids = big.eids(65, seed=65)
    _same(_edge(big, g, eids, 5, 9), big.want_edge(eids, 5, 9, "edge small"), EDGE_KEYS)


def _small_walk_still_exact(big, g):
    nodes = big.starts(40, seed=40)
    _same(_walk(big, g, nodes, 6, 3, 1, (0.5, 2), 9), big.want_walk(nodes, 6, 3, 1, (0.5, 2), 9, "walk small"), WALK_KEYS)


# ----------------------------------------------------------------------------------------------------------------- edge batches
def test_edge_items_second_pass(big):
    """700,001 edges with one negative each: 2,100,003 items, 2,851 more than the 2,097,152 threads of edge_items_kernel's largest grid."""
    eids, k, step = big.case_31()
    assert len(eids) * (2 + k) > 8192 * 256
    got = _edge(big, big.g, eids, k, step)
    want = big.want_edge(eids, k, step, "3.1")
    _same(got, want, EDGE_KEYS)
    assert got["n_bad"] == 2 and len(got["seed_nodes"]) > 200_000
    bad = np.flatnonzero((eids < 0) | (eids >= big.E))
    assert len(bad) == 2 and np.all(got["pos_src"][bad] == -1) and np.all(got["pos_dst"][bad] == -1) and np.all(got["neg_dst"][bad] == -1)


def test_edge_table_cleared_in_two_passes(big):
    """8,200 edges with 64 negatives: 541,200 items in a table of 2,097,152 slots, twice the 1,048,576 threads that clear it.  A slot the
    first call fails to clear keeps a stale first position, and the second call -- the same edges reversed, so mostly the same nodes at
    other positions -- then loses a first occurrence.  Then a small batch in the table the second call left."""
    eids, k, step = big.case_32()
    assert _table_size(len(eids) * (2 + k)) == 2_097_152 and len(eids) * (2 + k) <= 4096 * 256
    g = big.handle()
    try:
        _same(_edge(big, g, eids, k, step), big.want_edge(eids, k, step, "3.2"), EDGE_KEYS)
        rev = eids[::-1].copy()
        _same(_edge(big, g, rev, k, step + 1), big.want_edge(rev, k, step + 1, "3.2 reversed"), EDGE_KEYS)
        _small_edge_still_exact(big, g)
    finally:
        g.close()


def test_edge_item_limit_without_negatives(big):
    """4,194,304 edges, k = 0: exactly 8,388,608 items, all 8192 tiles of the scan.  One edge more is refused before any launch."""
    n = ITEM_LIMIT // 2
    eids = big.eids(n + 1, seed=33)
    d_e = big.torch.from_numpy(eids).cuda()
    got = _edge_end(big, big.g, _edge_begin(big, big.g, eids[:n], 0, 4, d_e=d_e))
    src, dst = RE.endpoints(big.ip, big.ix, eids[:n])
    nodes, local = RE.compact(np.concatenate([src, dst]))            # the one compaction of the case (k = 0: no draws)
    want = dict(seed_nodes=nodes, pos_src=local[:n].astype(np.int32), pos_dst=local[n:].astype(np.int32), neg_dst=np.zeros((n, 0), np.int32), n_bad=0)
    _same(got, want, EDGE_KEYS)
    _refused(_edge_begin(big, big.g, eids, 0, 4, d_e=d_e))
    _small_edge_still_exact(big, big.g)


def test_edge_item_limit_with_64_negatives(big):
    """127,100 edges, k = 64: 8,388,600 items, the largest batch of 64 negatives; 127,101 edges are refused."""
    n, k = ITEM_LIMIT // 66, 64
    assert n == 127_100 and (n + 1) * (2 + k) > ITEM_LIMIT
    eids = big.eids(n + 1, seed=34)
    d_e = big.torch.from_numpy(eids).cuda()
    got = _edge_end(big, big.g, _edge_begin(big, big.g, eids[:n], k, 4, d_e=d_e))
    want = big.want_edge(eids[:n], k, 4)                              # one compaction gives every output
    _same(got, want, ("seed_nodes", "pos_src", "pos_dst"))
    assert got["n_bad"] == 0 and len(got["seed_nodes"]) > 290_000
    _refused(_edge_begin(big, big.g, eids, k, 4, d_e=d_e))
    _small_edge_still_exact(big, big.g)


def test_edge_batch_python_entry_at_the_second_pass(big):
    """sampler.edge_batch / edge_batch_wait at the 700,001-edge size: documented shapes and dtypes, the C ABI's values."""
    torch = big.torch
    from COALA_GNN.sampler import edge_batch, edge_batch_wait
    eids, k, step = big.case_31(bad=False)
    abi = _edge(big, big.g, eids, k, step)
    d_e = torch.from_numpy(eids).cuda()
    b = edge_batch_wait(edge_batch(big.g, d_e, k, seed=SEED, step=step))
    n = len(eids)
    assert b.seed_nodes.dtype == torch.int64 and b.seed_nodes.dim() == 1 and b.seed_nodes.is_cuda
    for t, m in ((b.pos_src, n), (b.pos_dst, n), (b.neg_src, n * k), (b.neg_dst, n * k)):
        assert t.dtype == torch.int32 and tuple(t.shape) == (m,)
    for key, t in (("seed_nodes", b.seed_nodes), ("pos_src", b.pos_src), ("pos_dst", b.pos_dst), ("neg_dst", b.neg_dst)):
        assert np.array_equal(t.cpu().numpy(), abi[key].reshape(-1)), key
    assert torch.equal(b.neg_src, b.pos_src.repeat_interleave(k)) and abi["n_bad"] == 0
    assert int(b.pos_src.max()) < b.seed_nodes.numel() and int(b.neg_dst.min()) >= 0


# ----------------------------------------------------------------------------------------------------------------- walk batches
def test_walk_items_second_pass(big):
    """2,050 start nodes x 64 walks: 131,200 walks, past the 131,072 lane groups of walk_items_kernel's largest grid; with and without
    the traces, which are coala_sampler_node2vec_walk's."""
    from COALA_GNN_Pybind import _capi, current_stream
    torch = big.torch
    nodes, L, W, K, pq, step = big.starts(2_050, seed=41), 1, 64, 0, (0.5, 2), 3
    assert len(nodes) * W > 8192 * 256 // 16
    want = big.want_walk(nodes, L, W, K, pq, step, "4.1")
    got = _walk(big, big.g, nodes, L, W, K, pq, step)
    _same(got, want, WALK_KEYS)
    _same(_walk(big, big.g, nodes, L, W, K, pq, step, traces=False), want, WALK_KEYS[:3])
    out = torch.full((len(nodes) * W * (L + 1) + 2 * PAD,), S64, dtype=torch.int64, device="cuda")
    d_n = torch.from_numpy(nodes).cuda()
    _capi.check(_capi.load().coala_sampler_node2vec_walk(big.g._h, d_n.data_ptr(), len(nodes), W, L, *RW.thresholds(*pq), SEED, step,
                                                         out.data_ptr() + PAD * 8, current_stream()))
    assert np.array_equal(out[PAD:-PAD].cpu().numpy().reshape(got["traces"].shape), got["traces"])


def test_walk_relabel_and_table_in_two_passes(big):
    """8,200 start nodes (two of them bad), 8 walks of 7 hops, one negative row: 1,049,600 entries of pos and neg (the relabel loop's
    second pass) and 992,200 items in a table of 2,097,152 slots (the clear's second pass).  Then the same start nodes reversed, then a
    small batch, on the one handle."""
    nodes, L, W, K, pq, step = big.case_42()
    n = len(nodes)
    assert n * W * (L + 1) * (1 + K) > 4096 * 256 and _table_size(n + n * W * (L + 1) + n * W * K * L) == 2_097_152
    g = big.handle()
    try:
        got = _walk(big, g, nodes, L, W, K, pq, step)
        _same(got, big.want_walk(nodes, L, W, K, pq, step, "4.2"), WALK_KEYS)
        assert got["n_bad"] == 2
        rev = nodes[::-1].copy()
        _same(_walk(big, g, rev, L, W, K, pq, step + 1), big.want_walk(rev, L, W, K, pq, step + 1, "4.2 reversed"), WALK_KEYS)
        _small_walk_still_exact(big, g)
    finally:
        g.close()


def test_walk_item_list_limit(big):
    """2,097,152 start nodes, one walk of 2 hops, no negatives: the item list (the start nodes and the traces) is exactly 8,388,608
    while n W (L + 1) (1 + K) is 6,291,456.  One node more is refused: the bound that holds n more at num_neg 0."""
    n, L, W, K, pq = ITEM_LIMIT // 4, 2, 1, 0, (0.5, 2)
    assert n + n * W * (L + 1) == ITEM_LIMIT and n * W * (L + 1) * (1 + K) == 6_291_456
    nodes = big.starts(n + 1, seed=43)
    d_n = big.torch.from_numpy(nodes).cuda()
    got = _walk_end(big, big.g, _walk_begin(big, big.g, nodes[:n], L, W, K, pq, 4, d_n=d_n))
    _same(got, big.want_walk(nodes[:n], L, W, K, pq, 4), WALK_KEYS)
    _refused(_walk_begin(big, big.g, nodes, L, W, K, pq, 4, d_n=d_n))
    _small_walk_still_exact(big, big.g)


def test_walk_stated_limit(big):
    """32,768 start nodes, 64 walks of one hop, one negative row: n W (L + 1) (1 + K) is exactly 8,388,608 while the item list holds
    6,324,224.  One node more is refused."""
    n, L, W, K, pq = 32_768, 1, 64, 1, (1, 1)
    assert n * W * (L + 1) * (1 + K) == ITEM_LIMIT and n + n * W * (L + 1) + n * W * K * L == 6_324_224
    nodes = big.starts(n + 1, seed=44)
    d_n = big.torch.from_numpy(nodes).cuda()
    got = _walk_end(big, big.g, _walk_begin(big, big.g, nodes[:n], L, W, K, pq, 4, d_n=d_n))
    want = big.want_walk(nodes[:n], L, W, K, pq, 4)
    _same(got, want, ("input_nodes", "pos"))
    assert got["n_bad"] == 0 and len(got["input_nodes"]) > 290_000
    _refused(_walk_begin(big, big.g, nodes, L, W, K, pq, 4, d_n=d_n))
    _small_walk_still_exact(big, big.g)


def test_walk_batch_python_entry_at_the_second_pass(big):
    """sampler.walk_batch at the 131,200-walk size: documented shapes and dtypes, the C ABI's values."""
    torch = big.torch
    from COALA_GNN.sampler import walk_batch
    nodes, L, W, K, pq, step = big.starts(2_050, seed=41), 1, 64, 0, (0.5, 2), 3
    abi = _walk(big, big.g, nodes, L, W, K, pq, step)
    b = walk_batch(big.g, torch.from_numpy(nodes).cuda(), pq[0], pq[1], L, num_walks=W, num_neg=K, seed=SEED, step=step, traces=True)
    n = len(nodes)
    assert b.input_nodes.dtype == torch.int64 and b.input_nodes.dim() == 1 and b.n_bad == 0
    assert b.pos.dtype == torch.int32 and tuple(b.pos.shape) == (n * W, L + 1)
    assert b.neg.dtype == torch.int32 and tuple(b.neg.shape) == (n * W * K, L + 1)
    assert b.traces.dtype == torch.int64 and tuple(b.traces.shape) == (n, W, L + 1)
    for key in WALK_KEYS:
        assert np.array_equal(getattr(b, key).cpu().numpy(), abi[key]), key


# ------------------------------------------------------------------------------------------------------ one handle, every transition
def _flat(sample):
    out = [sample[0]]
    for b in sample[2]:
        out += [b.src_nodes, b.nbr, b.indptr, b.indices]
    return out


def _same_sample(torch, got, want):
    assert len(got) == len(want)
    for t, u in zip(got, want):
        assert (t is None) == (u is None) and (t is None or torch.equal(t, u))


def test_one_handle_every_transition(big):
    """Small and large batches and node samples in turn on one handle: the scratch grows, the table is found stale and memset, found
    clean and trusted, across the sizes; the last five calls are enqueued without a host wait between them and collected afterwards,
    so the ring is crossed with large calls in flight.  Every batch against its reference, every node sample against a handle that
    never saw a batch."""
    torch = big.torch
    from COALA_GNN.sampler import NeighborSampler
    rng = np.random.default_rng(5)
    e31, k31, s31 = big.case_31()
    e32, k32, s32 = big.case_32()
    n42, L42, W42, K42, pq42, s42 = big.case_42()
    e_small, w_small = big.eids(65, seed=65), big.starts(40, seed=40)
    seeds = [torch.from_numpy(rng.permutation(big.N)[:m].astype(np.int64)).cuda() for m in (3_000, 500, 20_000)]
    fans = ([5, 5], [-1, 2], [32])
    g, clean = big.handle(), big.handle()
    try:
        clean_samples = [_flat(NeighborSampler(f, seed=3).sample(clean, s, step=j)) for j, (f, s) in enumerate(zip(fans, seeds))]
        _same(_edge(big, g, e_small, 5, 9), big.want_edge(e_small, 5, 9, "edge small"), EDGE_KEYS)                     # 1
        _same(_edge(big, g, e31, k31, s31), big.want_edge(e31, k31, s31, "3.1"), EDGE_KEYS)                            # 2
        _same_sample(torch, _flat(NeighborSampler(fans[0], seed=3).sample(g, seeds[0], step=0)), clean_samples[0])     # 3
        _same(_walk(big, g, n42, L42, W42, K42, pq42, s42), big.want_walk(n42, L42, W42, K42, pq42, s42, "4.2"), WALK_KEYS)   # 4
        # 5 .. 9: enqueued back to back, nothing waited for (the inputs are on the device beforehand: a copy from the host would wait)
        d32, d_ws, d31 = (torch.from_numpy(x).cuda() for x in (e32, w_small, e31))
        p5 = NeighborSampler(fans[1], seed=3).sample_begin(g, seeds[1], step=1)
        p6 = _edge_begin(big, g, e32, k32, s32, d_e=d32)
        p7 = _walk_begin(big, g, w_small, 6, 3, 1, (0.5, 2), 9, d_n=d_ws)
        p8 = _edge_begin(big, g, e31, k31, s31, d_e=d31)
        p9 = NeighborSampler(fans[2], seed=3).sample_begin(g, seeds[2], step=2)
        _same_sample(torch, _flat(NeighborSampler(fans[1], seed=3).sample_end(p5)), clean_samples[1])
        _same(_edge_end(big, g, p6), big.want_edge(e32, k32, s32, "3.2"), EDGE_KEYS)
        _same(_walk_end(big, g, p7), big.want_walk(w_small, 6, 3, 1, (0.5, 2), 9, "walk small"), WALK_KEYS)
        _same(_edge_end(big, g, p8), big.want_edge(e31, k31, s31, "3.1"), EDGE_KEYS)
        _same_sample(torch, _flat(NeighborSampler(fans[2], seed=3).sample_end(p9)), clean_samples[2])
    finally:
        g.close()
        clean.close()


# --------------------------------------------------------------------------------------------------------- trace kernels off the ring
@pytest.mark.parametrize("n,W,L,pq", [(2_050, 64, 3, (0.25, 4)), (131_073, 1, 2, (1, 1))])
def test_node2vec_trace_second_pass(big, n, W, L, pq):
    """coala_sampler_node2vec_walk past the 131,072 lane groups of its largest grid: 131,200 walks of 2,050 nodes at the far corner, and
    131,073 walks of one node each at p = q = 1 (the path without a search), bad start nodes among them."""
    from COALA_GNN_Pybind import _capi, current_stream
    torch = big.torch
    assert n * W > 8192 * 256 // 16
    nodes = big.starts(n, seed=n, bad=True)
    d_n = torch.from_numpy(nodes).cuda()
    out = torch.full((n * W * (L + 1) + 2 * PAD,), S64, dtype=torch.int64, device="cuda")
    _capi.check(_capi.load().coala_sampler_node2vec_walk(big.g._h, d_n.data_ptr(), n, W, L, *RW.thresholds(*pq), SEED, 6, out.data_ptr() + PAD * 8,
                                                         current_stream()))
    assert bool((out[:PAD] == S64).all()) and bool((out[-PAD:] == S64).all())
    got = out[PAD:-PAD].cpu().numpy().reshape(n, W, L + 1)
    want = RW.traces_vec(big.ip, big.ix, nodes, L, W, RW.thresholds(*pq), SEED, 6)
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} walks differ"
    bad = (nodes < 0) | (nodes >= big.N)
    assert bad.sum() == 2 and np.all(got[bad] == -1) and np.all(got[~bad][:, :, 0] == nodes[~bad, None])


def test_random_walk_trace_second_pass(big):
    """coala_sampler_random_walk with 32,770 start nodes x 64 walks: 2,097,280 walks, past the 2,097,152 threads of its largest grid."""
    from COALA_GNN_Pybind import _capi, current_stream
    torch = big.torch
    n, W, T = 32_770, 64, 2
    assert n * W > 8192 * 256
    nodes = big.starts(n, seed=62, bad=True)
    thr = RP.threshold(0.25)
    d_n = torch.from_numpy(nodes).cuda()
    out = torch.full((n * W * (T + 1) + 2 * PAD,), S64, dtype=torch.int64, device="cuda")
    _capi.check(_capi.load().coala_sampler_random_walk(big.g._h, d_n.data_ptr(), n, W, T, thr, SEED, 6, 0, out.data_ptr() + PAD * 8, current_stream()))
    assert bool((out[:PAD] == S64).all()) and bool((out[-PAD:] == S64).all())
    got = out[PAD:-PAD].cpu().numpy().reshape(n, W, T + 1)
    want = RP.traces(big.ip, big.ix, nodes, W, T, thr, SEED, 6)
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} walks differ"
    assert (got[:, :, 2] == -1).mean() > 0.2 and (got[:, :, 2] >= 0).mean() > 0.6      # termination 0.25: both outcomes in bulk
