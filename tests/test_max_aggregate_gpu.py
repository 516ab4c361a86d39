"""GPU tests of the max aggregation (coala_block_max_aggregate[_csr] and coala_block_max_aggregate_backward in coala_block_ops.hip,
Block.max_aggregate, SAGEConv('pool'), GINConv('max')).

Forward: a maximum rounds nothing, so out and arg are compared bit for bit with the rule restated in numpy (ref_max of
test_max_aggregate_cpu.py; ref_max_fixed below is the same rule with the loop over the slots of all rows at once).
Backward: grad_src[s, c] is the sum of the k gradients whose argmax is s, added by atomics in any order: k - 1 roundings, so
|got - ref| <= gamma(k) sum|g| (u = 2^-24, gamma(n) = n u / (1 - n u), from test_block_ops_gpu.py) against a float64 scatter; a
source that nobody wins stays exactly 0.
Everything outside an output region keeps its sentinel."""
import copy
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _util import SENTINEL, ColorFiles, Guarded
from test_block_ops_gpu import _gamma
from test_max_aggregate_cpu import make_values, ref_max, tie_fraction

pytestmark = pytest.mark.gpu

DIMS = [1, 3, 64, 100, 128, 301, 1024]    # scalar path (1, 3, 100, 301), 16-byte path (64, 128, 1024), more than 64 units a row (301, 1024)


def ref_max_fixed(nbr, x):
    """ref_max on a fixed block, slot by slot over all rows at once."""
    n_dst, f = nbr.shape
    out = np.zeros((n_dst, x.shape[1]), dtype=x.dtype)
    arg = np.full((n_dst, x.shape[1]), -1, dtype=np.int32)
    for j in range(f):
        s = nbr[:, j]
        v = x[np.maximum(s, 0)]
        valid = (s >= 0)[:, None]
        first = valid & (arg < 0)
        with np.errstate(invalid="ignore"):
            take = first | (valid & ((v > out) | (np.isnan(v) & ~np.isnan(out))))
        out = np.where(take, v, out)
        arg = np.where(take, s[:, None], arg).astype(np.int32)
    return out, arg


def _dense_nbr(rng, n_dst, f, n_src):
    """-1 anywhere in a row, rows without a valid entry, repeated sources; the last 7 sources unreferenced, the 4 before them are the
    rows of -inf, NaN, -0 and +0 of make_values(kind='special')"""
    nbr = rng.integers(0, n_src - 7, size=(n_dst, f)).astype(np.int32)
    nbr[rng.random((n_dst, f)) < 0.25] = -1
    rep = rng.random(n_dst) < 0.15
    nbr[rep, 0] = rng.integers(0, n_src - 7, size=int(rep.sum()))
    nbr[rep, f - 1] = nbr[rep, 0]
    nbr[rng.random(n_dst) < 0.05] = -1
    nbr[0] = -1
    nbr[1, :] = n_src - 8                      # only -inf
    nbr[2, :] = np.resize([n_src - 10, n_src - 11], f)   # -0, +0, -0, ...
    return nbr


def _values(rng, kind, n_src, dim):
    """make_values with its four whole rows of one special value moved in front of the 7 unreferenced sources"""
    x = make_values(rng, kind, n_src - 7, dim)
    return np.concatenate([x, rng.standard_normal((7, dim)).astype(np.float32)])


def _csr(rng, n_dst, n_src, rows=(150, 3001)):
    deg = rng.integers(0, 40, size=n_dst)
    deg[rng.random(n_dst) < 0.1] = 0
    deg[0] = 0
    deg[n_dst // 3], deg[n_dst // 2] = rows
    indptr = np.zeros(n_dst + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    idx = rng.integers(0, n_src - 7, size=int(indptr[-1])).astype(np.int32)
    return indptr, idx


def _rows_of(indptr, idx):
    return [[int(s) for s in idx[indptr[d]: indptr[d + 1]] if s >= 0] for d in range(len(indptr) - 1)]


def _forward(L, torch, x, off, nbr=None, indptr=None, idx=None, want_arg=True):
    """Through the C ABI into guarded buffers -> (out fp32, arg int32 or None)"""
    from COALA_GNN_Pybind import _capi, current_stream
    n_src, dim = x.shape
    n_dst = nbr.shape[0] if nbr is not None else len(indptr) - 1
    gx, out, arg = Guarded(torch, n_src, dim, off, x), Guarded(torch, n_dst, dim, off), Guarded(torch, n_dst, dim, off)
    if nbr is not None:
        d_nbr = torch.from_numpy(nbr).cuda()
        _capi.check(L.coala_block_max_aggregate(0, d_nbr.data_ptr(), gx.ptr, out.ptr, arg.ptr if want_arg else None, n_dst, nbr.shape[1], dim,
                                                current_stream()))
    else:
        d_ip, d_idx = torch.from_numpy(indptr).cuda(), torch.from_numpy(idx).cuda()
        _capi.check(L.coala_block_max_aggregate_csr(0, d_ip.data_ptr(), d_idx.data_ptr(), gx.ptr, out.ptr, arg.ptr if want_arg else None, n_dst,
                                                    dim, current_stream()))
    torch.cuda.synchronize()
    assert gx.region().tobytes() == x.tobytes(), "the input changed"
    a = arg.region()
    if not want_arg:
        assert np.all(a == np.float32(-2.0)), "arg = null, and something was stored"
    return out.region(), a.view(np.int32) if want_arg else None


def _same(got, got_arg, want, want_arg, what):
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), f"{what}: {bad.sum()} values differ; first at {tuple(np.argwhere(bad)[0])}: got {got[bad][0]!r} want {want[bad][0]!r}"
    if got_arg is not None:
        bad = got_arg != want_arg
        assert not bad.any(), f"{what}: {bad.sum()} argmax differ; first at {tuple(np.argwhere(bad)[0])}: got {got_arg[bad][0]} want {want_arg[bad][0]}"


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("f", [1, 5, 16, 32])
def test_max_dense_bit_exact(hiplib, f, dim, off):
    """Fixed blocks through the C ABI; off = 1 puts every buffer one float off 16-byte alignment (the scalar path at dim % 4 == 0).
    Distinct values, the tie-heavy integers and the special values; with arg and without."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(f * 4099 + dim * 3 + off)
    n_dst, n_src = 1031, 200
    nbr = _dense_nbr(rng, n_dst, f, n_src)
    for kind in ("normal", "ties", "special"):
        x = _values(rng, kind, n_src, dim)
        want, want_arg = ref_max_fixed(nbr, x)
        if kind == "ties" and f >= 16:
            assert tie_fraction([[s for s in r if s >= 0] for r in nbr], x) > 0.5
        got, got_arg = _forward(L, torch, x, off, nbr=nbr)
        _same(got, got_arg, want, want_arg, f"dense f={f} dim={dim} off={off} {kind}")
        got, _ = _forward(L, torch, x, off, nbr=nbr, want_arg=False)
        _same(got, None, want, None, f"dense f={f} dim={dim} off={off} {kind}, arg = null")
    assert np.all(want[0] == 0) and np.all(want_arg[0] == -1) and np.all(np.isneginf(want[1])) and np.all(want_arg[1] == n_src - 8)


def test_the_vectorised_reference_is_the_loop(hiplib):
    rng = np.random.default_rng(0)
    nbr = _dense_nbr(rng, 200, 9, 100)
    for kind in ("normal", "ties", "special"):
        x = _values(rng, kind, 100, 5)
        a, b = ref_max_fixed(nbr, x), ref_max([[s for s in r if s >= 0] for r in nbr], x)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def test_max_dense_more_rows_than_waves(hiplib):
    """40000 rows: more than the 32768 waves of the largest grid, so some waves take a second row."""
    import torch
    from COALA_GNN_Pybind import _capi
    rng = np.random.default_rng(9)
    nbr = _dense_nbr(rng, 40000, 5, 300)
    x = _values(rng, "special", 300, 12)
    got, got_arg = _forward(_capi.load(), torch, x, 0, nbr=nbr)
    _same(got, got_arg, *ref_max_fixed(nbr, x), "40000 rows")


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dim", DIMS)
def test_max_ragged_bit_exact(hiplib, dim, off):
    """A ragged block with empty rows, a row of 150 edges (3 chunks of 64) and one of 3001 (47 chunks, the last one partial)."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(dim * 7 + off)
    n_dst, n_src = 301, 500
    indptr, idx = _csr(rng, n_dst, n_src)
    idx[indptr[n_dst // 2] + 2000] = n_src - 9             # the NaN row, deep in the long row
    rows_of = _rows_of(indptr, idx)
    for kind in ("normal", "ties", "special"):
        x = _values(rng, kind, n_src, dim)
        want, want_arg = ref_max(rows_of, x)
        if kind == "ties":
            assert tie_fraction(rows_of, x) > 0.5
        got, got_arg = _forward(L, torch, x, off, indptr=indptr, idx=idx)
        _same(got, got_arg, want, want_arg, f"ragged dim={dim} off={off} {kind}")
        got, _ = _forward(L, torch, x, off, indptr=indptr, idx=idx, want_arg=False)
        _same(got, None, want, None, f"ragged dim={dim} off={off} {kind}, arg = null")
    assert np.all(want[0] == 0) and np.all(want_arg[0] == -1)


@pytest.mark.parametrize("f,dim,off", [(5, 128, 0), (32, 100, 0), (1, 1, 0), (32, 1024, 1), (17, 64, 0), (16, 301, 0)])
def test_dense_and_ragged_forms_give_the_same_bits(hiplib, f, dim, off):
    """The same rows in both forms (the ragged one drops the -1 slots): out and arg equal bit for bit."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(f + dim)
    n_dst, n_src = 1031, 300
    nbr = _dense_nbr(rng, n_dst, f, n_src)
    valid = nbr >= 0
    indptr = np.zeros(n_dst + 1, dtype=np.int64)
    np.cumsum(valid.sum(1), out=indptr[1:])
    for kind in ("ties", "special"):
        x = _values(rng, kind, n_src, dim)
        a_out, a_arg = _forward(L, torch, x, off, nbr=nbr)
        b_out, b_arg = _forward(L, torch, x, off, indptr=indptr, idx=nbr[valid])
        assert a_out.tobytes() == b_out.tobytes() and np.array_equal(a_arg, b_arg), f"{kind}: the two forms differ"


def _check_grad(got, arg, go, n_src, what):
    """got fp32 [n_src, dim] against the float64 scatter of go through arg, within gamma(k) sum|g|; exactly 0 where nothing lands"""
    import torch
    dim = go.shape[1]
    d, c = np.nonzero(arg >= 0)
    flat = torch.from_numpy(arg[d, c].astype(np.int64) * dim + c)
    g = torch.from_numpy(go[d, c].astype(np.float64))
    ref = torch.zeros(n_src * dim, dtype=torch.float64).index_add_(0, flat, g).numpy().reshape(n_src, dim)
    mag = torch.zeros(n_src * dim, dtype=torch.float64).index_add_(0, flat, g.abs()).numpy().reshape(n_src, dim)
    k = np.bincount(flat.numpy(), minlength=n_src * dim).reshape(n_src, dim)
    err = np.abs(got.astype(np.float64) - ref)
    bound = _gamma(k) * mag
    bad = ~(err <= bound)
    print(f"{what}: largest k {k.max()}, largest err / bound {np.max(err[k > 1] / bound[k > 1]) if (k > 1).any() else 0.0:.3f}")
    assert not bad.any(), f"{what}: {bad.sum()} elements past the bound; first at {tuple(np.argwhere(bad)[0])}: got {got[bad][0]!r} " \
                          f"want {ref[bad][0]!r} bound {bound[bad][0]!r}"
    assert np.all(got[k == 0] == 0.0), f"{what}: a source that nobody wins is not exactly 0"
    return k


def _grad_out(rng, n_dst, dim):
    go = rng.standard_normal((n_dst, dim)).astype(np.float32)
    go[rng.random(n_dst) < 0.03] *= np.float32(1e6)
    return go


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dim", [1, 3, 100, 128, 301, 1024])
def test_max_backward_against_float64(hiplib, dim, off):
    """The backward through the C ABI on the argmax of a tie-heavy fixed block (rows without an edge hold -1), a few grad_out rows
    scaled by 1e6."""
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    rng = np.random.default_rng(dim * 5 + off)
    n_dst, n_src, f = 2053, 150, 7
    nbr = _dense_nbr(rng, n_dst, f, n_src)
    _, arg = ref_max_fixed(nbr, _values(rng, "ties", n_src, dim))
    go = _grad_out(rng, n_dst, dim)
    d_arg = torch.from_numpy(arg).cuda()
    gg, gs = Guarded(torch, n_dst, dim, off, go), Guarded(torch, n_src, dim, off, 0.0)
    _capi.check(L.coala_block_max_aggregate_backward(0, d_arg.data_ptr(), gg.ptr, gs.ptr, n_dst, dim, current_stream()))
    torch.cuda.synchronize()
    assert gg.region().tobytes() == go.tobytes() and np.array_equal(d_arg.cpu().numpy(), arg), "an input changed"
    k = _check_grad(gs.region(), arg, go, n_src, f"backward dim={dim} off={off}")
    assert k.max() > 8 and np.all(k[n_src - 7:] == 0)


def _sampled_blocks(torch):
    from COALA_GNN.sampler import LaborSampler, NeighborSampler
    from COALA_GNN.synthetic import powerlaw_csc
    indptr, indices = powerlaw_csc(30000, 12.0, seed=2, device="cuda")
    seeds = torch.randperm(30000, generator=torch.Generator().manual_seed(1))[:512].cuda()
    out = []
    for name, smp in (("neighbor 10,5", NeighborSampler([10, 5], seed=3)), ("neighbor 5,-1", NeighborSampler([5, -1], seed=3)),
                      ("labor 5,5", LaborSampler([5, 5], seed=3))):
        g = smp.make_graph(indptr, indices)
        _, _, blocks = smp.sample(g, seeds)
        out += [(f"{name} layer {i}", b) for i, b in enumerate(blocks)]
    return out


@pytest.mark.parametrize("dim", [128, 50])
def test_block_max_aggregate_through_autograd_on_sampled_blocks(hiplib, dim):
    """Block.max_aggregate on the blocks of NeighborSampler([10, 5]), NeighborSampler([5, -1]) (a ragged block) and LaborSampler([5, 5]):
    the forward equals max_aggregate_torch bit for bit, with and without a gradient asked for, and the gradient is within the bound
    of the module docstring of the float64 scatter through the reference's argmax."""
    import torch
    rng = np.random.default_rng(dim)
    forms = set()
    for name, b in _sampled_blocks(torch):
        forms.add(b.nbr is None)
        x = make_values(rng, "ties" if "layer 0" in name else "normal", b.num_src, dim)
        go = _grad_out(rng, b.num_dst, dim)
        h = torch.from_numpy(x).cuda().requires_grad_(True)
        out = b.max_aggregate(h)
        want, want_arg = b.max_aggregate_torch(h.detach(), return_arg=True)
        assert torch.equal(out.detach().view(torch.int32), want.view(torch.int32)), f"{name}: forward differs from max_aggregate_torch"
        assert torch.equal(b.max_aggregate(h.detach()).view(torch.int32), want.view(torch.int32)), f"{name}: forward without arg differs"
        (out * torch.from_numpy(go).cuda()).sum().backward()
        _check_grad(h.grad.cpu().numpy(), want_arg.cpu().numpy(), go, b.num_src, name)
        # and the fallback's own gradient, in float64 on the same device
        h64 = torch.from_numpy(x).cuda().double().requires_grad_(True)
        (b.max_aggregate_torch(h64) * torch.from_numpy(go).cuda().double()).sum().backward()
        _check_grad(h64.grad.cpu().numpy(), want_arg.cpu().numpy(), go, b.num_src, name + " (fallback)")
    assert forms == {False, True}


def test_max_refuses_bad_shapes(hiplib):
    """Return codes only: nothing is launched, and the output buffers keep their sentinel."""
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    nbr = torch.zeros(64, dtype=torch.int32, device="cuda")
    ip = torch.zeros(65, dtype=torch.int64, device="cuda")
    a = torch.zeros(64 * 4, device="cuda")
    b = torch.full((64 * 4,), float(SENTINEL), device="cuda")
    st = current_stream()
    for n_dst, f, dim in ((1, 0, 4), (1, 33, 4), (1, 4, 0), (-1, 4, 4), (0, 33, 4)):
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_max_aggregate(0, nbr.data_ptr(), a.data_ptr(), b.data_ptr(), b.data_ptr(), n_dst, f, dim, st))
    for n_dst, dim in ((1, 0), (-1, 4)):
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_max_aggregate_csr(0, ip.data_ptr(), nbr.data_ptr(), a.data_ptr(), b.data_ptr(), b.data_ptr(), n_dst, dim, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_max_aggregate_backward(0, nbr.data_ptr(), a.data_ptr(), b.data_ptr(), n_dst, dim, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_max_aggregate(0, nbr.data_ptr(), None, b.data_ptr(), b.data_ptr(), 4, 4, 4, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_max_aggregate_backward(0, None, a.data_ptr(), b.data_ptr(), 4, 4, st))
    # n_dst == 0 is fine and launches nothing
    _capi.check(L.coala_block_max_aggregate(0, nbr.data_ptr(), a.data_ptr(), b.data_ptr(), b.data_ptr(), 0, 4, 4, st))
    _capi.check(L.coala_block_max_aggregate_csr(0, ip.data_ptr(), nbr.data_ptr(), a.data_ptr(), b.data_ptr(), b.data_ptr(), 0, 4, st))
    _capi.check(L.coala_block_max_aggregate_backward(0, nbr.data_ptr(), a.data_ptr(), b.data_ptr(), 0, 4, st))
    torch.cuda.synchronize()
    assert torch.all(b == float(SENTINEL))


@pytest.mark.parametrize("which", ["sage_pool", "gin_max"])
def test_models_on_max_aggregation_train_through_the_loader(hiplib, oracle, tmp_path, monkeypatch, which):
    """The loop of test_edge_weight_layers_gpu.py (2 epochs of 11 steps, batch 64, prefetching loader) with harness.SAGE('pool') and
    harness.GIN('max').  On the first batch a twin with the same weights runs with Block.max_aggregate forced onto the torch path: its
    loss has the same bits, since the dense ops are the same and the maximum is exact.  The labels are a function of what the model
    sees (the largest of a node's own first five feature columns, which reaches the output through both layers' self terms), so the
    loss comes down: the mean of the last 5 steps is below the mean of the first 5, and every loss is finite."""
    import torch
    from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, SSD_INFO
    from COALA_GNN.harness import GIN, SAGE
    from COALA_GNN.sampler import Block, NeighborSampler
    from COALA_GNN.synthetic import alloc_pinned_table, block_colors, feature_rows_torch, powerlaw_csc
    torch.manual_seed(0)
    n_nodes, dim, batch, fan, n_cls = 20000, 128, 64, [5, 5], 5
    table = alloc_pinned_table(n_nodes, dim, seed=3, device=0)
    indptr, indices = powerlaw_csc(n_nodes, 8.0, seed=1, device="cuda")
    labels = feature_rows_torch(torch.arange(n_nodes, device="cuda"), dim, 3)[:, :n_cls].argmax(1)
    color, tk, sc, ncol = block_colors(n_nodes, nodes_per_color=512)
    files = ColorFiles(tmp_path, color, tk, sc)
    comm = MPI_Comm_Manager(0)
    comm.initialize_nested_process_group("isolated")
    train_ids = torch.randperm(int(0.6 * n_nodes), generator=torch.Generator().manual_seed(0))[:64 * 12]
    nd = Node_Distributor(comm, train_ids, batch, files.color_file, files.topk_file, files.score_file, parsing_method="baseline")
    sampler = NeighborSampler(fan, seed=5)
    g = sampler.make_graph(indptr, indices, ndata={"labels": labels})
    loader = COALA_GNN_DataLoader(SSD_INFO(1, dim * 4, 1024, 0), nd, g, sampler, batch, dim, fan, 4, "cuda:0", refresh_counter=3,
                                  cache_backend="isolated", sim_buf=table, num_rows=n_nodes, prefetch=1)
    if which == "sage_pool":
        model = SAGE(dim, 64, n_cls, len(fan), aggregator_type="pool").cuda()
    else:
        model = GIN(dim, 64, n_cls, len(fan), aggregator_type="max").cuda()
    twin = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    native_calls, losses = [], []
    native = Block.max_aggregate
    monkeypatch.setattr(Block, "max_aggregate", lambda self, h: (native_calls.append(h.is_cuda), native(self, h))[1])
    for epoch in range(2):
        for input_nodes, seeds, blocks, feat in loader:
            batch_labels = blocks[-1].dstdata["labels"].view(-1)
            loss = torch.nn.functional.cross_entropy(model(blocks, feat), batch_labels)
            if not losses:
                with monkeypatch.context() as m:
                    m.setattr(Block, "max_aggregate", lambda self, h: self.max_aggregate_torch(h))
                    twin_loss = torch.nn.functional.cross_entropy(twin(blocks, feat), batch_labels)
                print(f"first loss: native {loss.item()!r}, torch path {twin_loss.item()!r}")
                assert loss.detach().view(torch.int32).item() == twin_loss.detach().view(torch.int32).item(), "first loss differs in its bits"
            opt.zero_grad(); loss.backward(); opt.step()
            losses.append(loss.item())
    print("losses:", " ".join(f"{x:.4f}" for x in losses))
    assert len(native_calls) == 2 * 22 and all(native_calls), "the model did not go through Block.max_aggregate on the GPU"
    assert len(losses) == 22 and all(math.isfinite(x) for x in losses)
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5, losses
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    del loader
    table.close()


@pytest.mark.parametrize("extra", [["--sage_aggregator", "pool"], ["--model_type", "gin", "--gin_aggregator", "max", "--eval_fan_out=-1,-1"]])
def test_example_training_script_runs_pool_and_gin(extra):
    """examples/train_synthetic.py with the new options, in a fresh process, at the size of
    test_gat_training_gpu.py::test_example_training_script_runs_gat_and_gcn, for one epoch."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "train_synthetic.py"), "--nodes", "60000", "--dim", "64",
                          "--batch_size", "256", "--epochs", "1", "--cache_size", "4", "--prefetch", "1"] + extra,
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    loss = re.search(r"final loss (\S+)", out.stdout)
    assert loss and math.isfinite(float(loss.group(1))), out.stdout[-2000:]
    assert "Test Acc" in out.stdout
