"""GPU tests of the skip-gram batch kernels (coala_sampler_walk_batch / _wait; sampler.walk_batch): walks, negatives and the compacted
node list, bit for bit against the restatement of tests/_node2vec_ref.py, at the C ABI with sentinel-padded buffers."""
import ctypes as C

import numpy as np
import pytest

import _node2vec_ref as R

pytestmark = pytest.mark.gpu

PAD = 37            # sentinel entries in front of and behind every output
S64, S32 = -0x0123456789ABCDEF, -0x01234567
TILE = 1024         # items per tile of the scan (coala_sampler.hip: kTile)


@pytest.fixture(scope="module")
def setup(hiplib):
    import torch
    from COALA_GNN.sampler import CSCGraph
    ip, ix, special, named, n0 = R.edge_graph(5000)
    g = CSCGraph(torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda())
    first = np.concatenate([list(named.values()), special[:12], [named["own"]]]).astype(np.int64)
    yield torch, g, ip, ix, first
    g.close()


def _nodes(ip, first, n, seed=0, bad=False):
    rng = np.random.default_rng(seed)
    v = np.concatenate([first, rng.integers(0, len(ip) - 1, size=max(n - len(first), 0))])[:n].astype(np.int64)
    if bad:
        v[[1, n // 2]] = [-1, len(ip) - 1]
    return v


def _call(torch, g, nodes, L, W, K, thr, seed, step, traces=True):
    """The C ABI on sentinel-padded buffers -> dict as _node2vec_ref.walk_batch gives it, after checking the padding."""
    from COALA_GNN_Pybind import _capi, current_stream
    lib = _capi.load()
    n = len(nodes)
    d_n = torch.from_numpy(nodes).cuda()
    sizes = (n + n * W * (L + 1) + n * W * K * L, n * W * (L + 1), n * W * K * (L + 1), n * W * (L + 1))
    fills = (S64, S32, S32, S64)
    bufs = [torch.full((m + 2 * PAD,), s, dtype=dt, device="cuda") for m, dt, s in zip(sizes, (torch.int64, torch.int32, torch.int32, torch.int64), fills)]
    ptrs = [b.data_ptr() + PAD * b.element_size() for b in bufs]
    out = _capi.WalkBatchOut(ptrs[0], ptrs[1], ptrs[2], ptrs[3] if traces else None)
    ticket = C.c_int64(-1)
    _capi.check(lib.coala_sampler_walk_batch(g._h, d_n.data_ptr(), n, W, L, *thr, K, seed, step, C.byref(out), C.byref(ticket), current_stream()))
    n_nodes, n_bad = C.c_int64(-1), C.c_int64(-1)
    _capi.check(lib.coala_sampler_walk_batch_wait(g._h, ticket.value, C.byref(n_nodes), C.byref(n_bad)))
    host = [b.cpu().numpy() for b in bufs]
    for h, m, s in zip(host, sizes, fills):
        assert np.all(h[:PAD] == s) and np.all(h[PAD + m:] == s), "a write outside an output's capacity"
    assert np.all(host[0][PAD + n_nodes.value: PAD + sizes[0]] == S64), "input_nodes written past n_nodes"
    if not traces:
        assert np.all(host[3] == S64)
    return dict(input_nodes=host[0][PAD: PAD + n_nodes.value], pos=host[1][PAD: PAD + sizes[1]].reshape(n * W, L + 1),
                neg=host[2][PAD: PAD + sizes[2]].reshape(n * W * K, L + 1), traces=host[3][PAD: PAD + sizes[3]].reshape(n, W, L + 1), n_bad=n_bad.value)


def _same(got, want, traces=True):
    for key in ("input_nodes", "pos", "neg") + (("traces",) if traces else ()):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
    assert got["n_bad"] == want["n_bad"]


# (n, W, L, K): n W below one scan tile (the first four and the last) and above it, K = 0, 1 and 16, the longest walk
SHAPES = [(1, 1, 1, 0), (20, 2, 5, 0), (40, 3, 6, 1), (9, 2, 4, 16), (300, 5, 8, 1), (1100, 1, 2, 0), (70, 16, 3, 16), (5, 1, 127, 1)]
assert all((n * W < TILE) == (i < 4 or i == 7) for i, (n, W, L, K) in enumerate(SHAPES))


@pytest.mark.parametrize("n,W,L,K", SHAPES)
def test_walk_batch_bitwise(setup, n, W, L, K):
    torch, g, ip, ix, first = setup
    p, q = [(0.5, 2), (1, 1), (4, 0.25)][(n + K) % 3]
    thr = R.thresholds(p, q)
    nodes = _nodes(ip, first, n, seed=n + K)
    got = _call(torch, g, nodes, L, W, K, thr, seed=11, step=3)
    want = R.walk_batch(ip, ix, nodes, L, W, K, thr, seed=11, step=3)
    _same(got, want)
    assert want["n_bad"] == 0 and len(np.unique(got["input_nodes"])) == len(got["input_nodes"])
    _same(_call(torch, g, nodes, L, W, K, thr, seed=11, step=3, traces=False), want, traces=False)      # the same call twice, no traces
    # the traces are node2vec_random_walk's
    from COALA_GNN.sampler import node2vec_random_walk
    tr = node2vec_random_walk(g, torch.from_numpy(nodes).cuda(), p, q, L, num_walks=W, seed=11, step=3)
    assert np.array_equal(tr.cpu().numpy(), got["traces"])


@pytest.mark.parametrize("n,W,L,K", [(40, 3, 6, 1), (300, 5, 8, 16), (30, 2, 4, 0)])
def test_bad_start_nodes(setup, n, W, L, K):
    torch, g, ip, ix, first = setup
    thr = R.thresholds(0.5, 2)
    nodes = _nodes(ip, first, n, seed=1, bad=True)
    got = _call(torch, g, nodes, L, W, K, thr, seed=2, step=0)
    want = R.walk_batch(ip, ix, nodes, L, W, K, thr, seed=2, step=0)
    _same(got, want)
    assert got["n_bad"] == 2 and np.all(got["pos"][W: 2 * W] == -1) and np.all(got["neg"][W * K: 2 * W * K] == -1)
    _same(_call(torch, g, _nodes(ip, first, n, seed=1), L, W, K, thr, seed=2, step=0), R.walk_batch(ip, ix, _nodes(ip, first, n, seed=1), L, W, K, thr, 2, 0))


def test_python_entry_limits_and_tickets(setup):
    torch, g, ip, ix, first = setup
    from COALA_GNN.sampler import ITEM_LIMIT, NeighborSampler, edge_batch, edge_batch_wait, walk_batch, walk_batch_begin, walk_batch_end
    from COALA_GNN_Pybind import _capi, current_stream
    lib = _capi.load()
    nodes = _nodes(ip, first, 65, seed=4, bad=True)
    d = torch.from_numpy(nodes).cuda()
    b = walk_batch(g, d, 0.5, 2, 6, num_walks=3, num_neg=2, seed=5, step=7, traces=True)
    want = R.walk_batch(ip, ix, nodes, 6, 3, 2, R.thresholds(0.5, 2), 5, 7)
    assert b.n_bad == 2 and b.pos.dtype == torch.int32 and tuple(b.pos.shape) == (195, 7) and tuple(b.neg.shape) == (390, 7)
    for key in ("input_nodes", "pos", "neg", "traces"):
        assert np.array_equal(getattr(b, key).cpu().numpy(), want[key]), key
    assert walk_batch(g, d, 0.5, 2, 6, num_walks=3, num_neg=2, seed=5, step=7).traces is None
    assert len(b.tensors()) == 5
    # the item limit: n W (L + 1) (1 + K) <= 8,388,608, refused before any launch by the wrapper and by the C entry
    n_over = ITEM_LIMIT // (64 * 128 * 2) + 1
    many = torch.zeros(n_over, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="over the limit"):
        walk_batch_begin(g, many, 1, 1, 127, num_walks=64, num_neg=1)
    out = _capi.WalkBatchOut(many.data_ptr(), many.data_ptr(), many.data_ptr(), None)      # never written: the call is refused
    ticket = C.c_int64(-1)
    one = R.ONE
    rc = lib.coala_sampler_walk_batch(g._h, many.data_ptr(), n_over, 64, 127, one, one, one, 1, 0, 0, C.byref(out), C.byref(ticket), current_stream())
    assert rc == _capi.EINVAL and "items" in _capi.last_error() and ticket.value == -1
    assert lib.coala_sampler_walk_batch(g._h, many.data_ptr(), 4, 64, 127, one, one, one, 17, 0, 0, C.byref(out), C.byref(ticket), current_stream()) == _capi.EINVAL
    assert lib.coala_sampler_walk_batch(g._h, many.data_ptr(), 4, 2, 128, one, one, one, 1, 0, 0, C.byref(out), C.byref(ticket), current_stream()) == _capi.EINVAL
    assert lib.coala_sampler_walk_batch(g._h, many.data_ptr(), 4, 2, 12, one - 1, 0, 0, 1, 0, 0, C.byref(out), C.byref(ticket), current_stream()) == _capi.EINVAL
    for kwargs in (dict(num_neg=17), dict(num_neg=-1), dict(walk_length=0), dict(num_walks=65), dict(q=17.0)):
        with pytest.raises(ValueError):
            walk_batch_begin(g, d, **{**dict(p=1.0, q=1.0, walk_length=4), **kwargs})
    # each kind of wait refuses the other kinds' tickets; the right one still collects them, and the handle stays usable
    cnt = (C.c_int64 * 2)()
    pend = walk_batch_begin(g, d, 0.5, 2, 6, num_walks=3, num_neg=2, seed=5, step=7)
    assert lib.coala_sampler_wait(g._h, pend[-1], cnt, None) == _capi.EINVAL and "walk batch" in _capi.last_error()
    assert lib.coala_sampler_edge_batch_wait(g._h, pend[-1], cnt, None) == _capi.EINVAL
    again = walk_batch_end(pend)
    assert torch.equal(again.pos, b.pos) and torch.equal(again.input_nodes, b.input_nodes)
    ep = edge_batch(g, torch.arange(10, device="cuda"), 1)
    assert lib.coala_sampler_walk_batch_wait(g._h, ep[-1], cnt, None) == _capi.EINVAL and "not a walk batch" in _capi.last_error()
    edge_batch_wait(ep)
    _, _, blocks = NeighborSampler([3]).sample(g, d[2:20], step=0)
    sp = NeighborSampler([3]).sample_begin(g, d[2:20], step=0)
    assert lib.coala_sampler_walk_batch_wait(g._h, sp.ticket, cnt, None) == _capi.EINVAL
    _, _, blocks2 = NeighborSampler([3]).sample_end(sp)
    assert torch.equal(blocks[0].nbr, blocks2[0].nbr)
    third = walk_batch(g, d, 0.5, 2, 6, num_walks=3, num_neg=2, seed=5, step=7)
    assert torch.equal(third.neg, b.neg)
