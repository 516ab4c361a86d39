"""GPU tests of the GATv2 attention kernels (coala_block_gatv2_aggregate[_csr][_backward] in coala_block_ops.hip) against float64.

Called through the C ABI on hand-made blocks: fixed rows with -1 anywhere, rows without a valid edge, repeated sources, fan-outs
1..32; CSR rows of degree 0 to past one 64-edge chunk and a hub of 70,001 in-edges; heads 1..16; D in {1, 3, 16, 64, 65, 128}; the
16-byte path and the scalar path (D % 4 != 0, or buffers one float off 16-byte alignment); rows of H * D <= 1024 floats (grad_attn summed
in registers) and above (the one-wave-a-block kernel); n_dst up to 100,003, past the grid cap; scores up to +-1e3.  Every output is
followed by sentinel guard words, and every input is checked untouched.

Tolerances.  Every bound is the first-order roundoff bound derived in tests/_gatv2_ref.py's docstring from the kernels' summation
orders -- the score's D-term dot (lane scan and LDS adds), 3 ulp for exp and log, one rescale per chunk of the online softmax, atomics
in any order for grad_src, the slot-order sum of grad_dst, and for grad_attn the per-wave chain, the block's LDS combine and the sum of
the partials buffer.  z_jc is a single correctly rounded fp32 addition, so its sign is the exact sum's and the float64 reference is on
the kernel's side of the kink at every element: none is excluded from any comparison.  The CPU twin (tests/test_gatv2_cpu.py) shows
that a correct fp32 evaluation lies inside these bounds and that three wrong kernels would not."""
import itertools

import numpy as np
import pytest

import _gatv2_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e33)
GUARD = 67
SLOPE = R.SLOPE


def _device(torch, arr, off, fill=None):
    flat = torch.full((off + arr.size + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    if fill is None:
        flat[off: off + arr.size] = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)).cuda()
    else:
        flat[off: off + arr.size] = fill
    return flat, flat.data_ptr() + 4 * off


def _region(flat, off, shape):
    h = flat.cpu().numpy()
    n = int(np.prod(shape))
    pad = np.concatenate([h[:off], h[off + n:]])
    assert np.array_equal(pad.view(np.int32), np.full(pad.shape, SENTINEL).view(np.int32)), "write outside the output region"
    return h[off: off + n].reshape(shape)


def _run(torch, L, form, graph, n_dst, n_src, fs, fd, attn, g, off, parts=None, want=(True, True, True), backward=True):
    """Forward and backward through the C ABI, every float buffer at float offset `off`, sentinels around every output and filling the
    outputs that are written whole.  want: which of grad_src, grad_dst, grad_attn are asked for (a null pointer otherwise).
    -> dict of out, lse, gs, gd, parts (the partials buffer) and ga (its fp32 sum over dim 0, as the autograd wrapper takes it)."""
    from COALA_GNN_Pybind import _capi, current_stream
    H, D = fs.shape[1], fs.shape[2]
    parts = R.default_parts(n_dst) if parts is None else parts
    ins = dict(fs=fs, fd=fd, attn=attn, g=g)
    bufs = {k: _device(torch, v, off) for k, v in ins.items()}
    o_buf, o = _device(torch, np.empty((n_dst, H, D), np.float32), off, fill=float(SENTINEL))
    s_buf, lse = _device(torch, np.empty((n_dst, H), np.float32), off, fill=float(SENTINEL))
    gs_buf, gs = _device(torch, np.empty((n_src, H, D), np.float32), off, fill=0.0)
    gd_buf, gd = _device(torch, np.empty((n_dst, H, D), np.float32), off, fill=float(SENTINEL))
    pa_buf, pa = _device(torch, np.empty((parts, H * D), np.float32), off, fill=float(SENTINEL))
    p = {k: v[1] for k, v in bufs.items()}
    st = current_stream()
    grads = (gs if want[0] else None, gd if want[1] else None, pa if want[2] else None)
    if form == "fixed":
        dn = torch.from_numpy(graph).cuda()
        f = graph.shape[1]
        _capi.check(L.coala_block_gatv2_aggregate(0, dn.data_ptr(), p["fs"], p["fd"], p["attn"], o, lse, n_dst, f, H, D, float(SLOPE), st))
        if backward:
            _capi.check(L.coala_block_gatv2_aggregate_backward(0, dn.data_ptr(), p["fs"], p["fd"], p["attn"], o, lse, p["g"], *grads, parts, n_dst,
                                                               f, H, D, float(SLOPE), st))
    else:
        indptr, indices = graph
        dp = torch.from_numpy(indptr).cuda()
        di = torch.from_numpy(np.append(indices, np.int32(-1))).cuda()   # one word past the edges: a block without edges has a buffer
        _capi.check(L.coala_block_gatv2_aggregate_csr(0, dp.data_ptr(), di.data_ptr(), p["fs"], p["fd"], p["attn"], o, lse, n_dst, H, D,
                                                      float(SLOPE), st))
        if backward:
            _capi.check(L.coala_block_gatv2_aggregate_csr_backward(0, dp.data_ptr(), di.data_ptr(), p["fs"], p["fd"], p["attn"], o, lse, p["g"],
                                                                   *grads, parts, n_dst, H, D, float(SLOPE), st))
    torch.cuda.synchronize()
    res = dict(out=_region(o_buf, off, (n_dst, H, D)), lse=_region(s_buf, off, (n_dst, H)), gs=_region(gs_buf, off, (n_src, H, D)),
               gd=_region(gd_buf, off, (n_dst, H, D)), parts=_region(pa_buf, off, (parts, H * D)))
    if n_dst == 0 or not (backward and want[2]):       # nothing is launched for an empty block: the wrapper hands out zeros then
        assert np.all(res["parts"] == SENTINEL)
        res["ga"] = np.zeros((H, D), np.float32)
    else:
        res["ga"] = pa_buf[off: off + parts * H * D].view(parts, H * D).sum(0).view(H, D).cpu().numpy()
    for k, v in ins.items():                                                       # inputs untouched
        assert np.array_equal(_region(bufs[k][0], off, v.shape), v)
    return res


def _fixed_case(torch, L, n_dst, f, H, D, off, big, log=None):
    rng = np.random.default_rng(n_dst * 7 + f * 131 + H * 17 + D + off)
    n_src = max(64, min(5000, n_dst // 4))
    nbr = R.fixed_nbr(rng, n_dst, f, n_src - 7)       # the last 7 sources are never referenced
    fs, fd, attn, g = R.make_inputs(rng, n_src, n_dst, H, D, big)
    got = _run(torch, L, "fixed", nbr, n_dst, n_src, fs, fd, attn, g, off)
    rows, srcs, nc = R.edges_fixed(nbr)
    ref = R.reference(rows, srcs, n_dst, n_src, nc, fs, fd, attn, g, R.default_parts(n_dst))
    R.check_all(got, ref, log)
    assert np.all(got["gs"][n_src - 7:] == 0.0), "an unreferenced source has a gradient"


LARGE_CASES = [(0, 4, 2, 8, 0, False), (1, 1, 1, 1, 1, False), (32_769, 31, 4, 16, 0, False), (100_003, 9, 1, 4, 1, True)]


@pytest.mark.parametrize("n_dst,f,H,D,off,big", R.SMALL_CASES + LARGE_CASES)
def test_gatv2_fixed_against_float64(hiplib, n_dst, f, H, D, off, big):
    import torch
    from COALA_GNN_Pybind import _capi
    _fixed_case(torch, _capi.load(), n_dst, f, H, D, off, big, log=print)


def _csr_graph(rng, n_dst, f, n_src):
    deg = rng.integers(0, 2 * f + 1, size=n_dst)
    if n_dst:
        deg[rng.random(n_dst) < 0.05] = rng.integers(65, 200)
        deg[0] = 0
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return indptr, rng.integers(0, n_src, size=int(indptr[-1])).astype(np.int32)


@pytest.mark.parametrize("n_dst,f,H,D,off,big", R.SMALL_CASES + [(0, 1, 1, 4, 0, False)])
def test_gatv2_csr_against_float64(hiplib, n_dst, f, H, D, off, big):
    """Degrees 0..2f, 5 % of the rows at 65..200 edges (two to four chunks, the online rescale), row 0 empty."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(n_dst * 5 + f * 31 + H * 3 + D + off)
    n_src = max(64, min(5000, n_dst // 4))
    indptr, indices = _csr_graph(rng, n_dst, f, n_src)
    fs, fd, attn, g = R.make_inputs(rng, n_src, n_dst, H, D, big)
    got = _run(torch, L, "csr", (indptr, indices), n_dst, n_src, fs, fd, attn, g, off)
    rows, srcs, nc = R.edges_csr(indptr, indices)
    R.check_all(got, R.reference(rows, srcs, n_dst, n_src, nc, fs, fd, attn, g, R.default_parts(n_dst)), log=print)


@pytest.mark.parametrize("big", [False, True])
def test_gatv2_csr_hub_against_float64(hiplib, big):
    """One row of 70,001 in-edges (1,094 chunks of the online softmax; grad_dst added to chunk after chunk) between small rows."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(99 + big)
    n_src, H, D = 3000, 2, 2
    deg = rng.integers(0, 9, size=41)
    deg[20] = 70_001
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rng.integers(0, n_src, size=int(indptr[-1])).astype(np.int32)
    fs, fd, attn, g = R.make_inputs(rng, n_src, len(deg), H, D, big)
    got = _run(torch, L, "csr", (indptr, indices), len(deg), n_src, fs, fd, attn, g, 0)
    rows, srcs, nc = R.edges_csr(indptr, indices)
    R.check_all(got, R.reference(rows, srcs, len(deg), n_src, nc, fs, fd, attn, g, R.default_parts(len(deg))), log=print)


@pytest.mark.parametrize("f,H,D,off,big", [(5, 4, 16, 0, False), (32, 2, 65, 1, True), (17, 8, 3, 0, True), (1, 16, 128, 1, False)])
def test_gatv2_fixed_and_csr_give_identical_bits(hiplib, f, H, D, off, big):
    """Fixed rows whose valid entries come first (the sampler's layout) against the same rows in CSR form: out, lse and grad_dst bit
    for bit."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(f * 11 + H + D + off)
    n_dst, n_src = (2000, 700) if H * D <= 512 else (300, 100)
    deg = rng.integers(0, f + 1, size=n_dst)
    deg[:3] = [0, f, 1]
    nbr = np.full((n_dst, f), -1, np.int32)
    for d in range(n_dst):
        nbr[d, :deg[d]] = rng.integers(0, n_src, size=deg[d])
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = nbr[nbr >= 0].astype(np.int32)
    fs, fd, attn, g = R.make_inputs(rng, n_src, n_dst, H, D, big)
    a = _run(torch, L, "fixed", nbr, n_dst, n_src, fs, fd, attn, g, off)
    b = _run(torch, L, "csr", (indptr, indices), n_dst, n_src, fs, fd, attn, g, off)
    for k in ("out", "lse", "gd"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{k} differs between the fixed and the CSR kernels"
    assert np.all(np.isneginf(a["lse"][deg == 0])) and np.isfinite(a["lse"][deg > 0]).all()


@pytest.mark.parametrize("form,H,D", [("fixed", 4, 16), ("csr", 2, 65), ("fixed", 16, 128)])
@pytest.mark.parametrize("parts", [1, None])
def test_gatv2_backward_is_reproducible(hiplib, form, H, D, parts):
    """Two backward launches on the same inputs: grad_attn (after the partials sum) and grad_dst bit for bit, with one partials row and
    with the wrapper's default; every row of the partials buffer is written."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(H + D)
    n_dst, n_src = (1200, 400) if H * D <= 512 else (120, 64)
    graph = R.fixed_nbr(rng, n_dst, 9, n_src) if form == "fixed" else _csr_graph(rng, n_dst, 6, n_src)
    fs, fd, attn, g = R.make_inputs(rng, n_src, n_dst, H, D, False)
    a = _run(torch, L, form, graph, n_dst, n_src, fs, fd, attn, g, 0, parts=parts)
    b = _run(torch, L, form, graph, n_dst, n_src, fs, fd, attn, g, 0, parts=parts)
    for k in ("ga", "gd", "parts", "out", "lse"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{k} differs between two launches"
    rows, srcs, nc = R.edges_fixed(graph) if form == "fixed" else R.edges_csr(*graph)
    R.check_all(a, R.reference(rows, srcs, n_dst, n_src, nc, fs, fd, attn, g, R.default_parts(n_dst) if parts is None else parts), log=print)


def test_gatv2_null_gradients_are_not_written(hiplib):
    """Each of the three gradient pointers may be null: the others have the bits of the full call, and the buffer behind a null stays as
    it was."""
    import torch
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(23)
    n_dst, n_src, H, D = 500, 200, 4, 16
    nbr = R.fixed_nbr(rng, n_dst, 7, n_src)
    fs, fd, attn, g = R.make_inputs(rng, n_src, n_dst, H, D, False)
    full = _run(torch, L, "fixed", nbr, n_dst, n_src, fs, fd, attn, g, 0)
    for want in itertools.product([False, True], repeat=3):
        got = _run(torch, L, "fixed", nbr, n_dst, n_src, fs, fd, attn, g, 0, want=want)
        for on, k, untouched in zip(want, ("gs", "gd", "parts"), (0.0, float(SENTINEL), float(SENTINEL))):
            if not on:
                assert np.all(got[k] == np.float32(untouched)), f"{k} was written through a null pointer's buffer"
        if want[1]:
            assert np.array_equal(got["gd"].view(np.int32), full["gd"].view(np.int32))
        if want[2]:
            assert np.array_equal(got["parts"].view(np.int32), full["parts"].view(np.int32))


def test_gatv2_refuses_bad_shapes(hiplib):
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    st = current_stream()
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    i64 = torch.zeros(65, dtype=torch.int64, device="cuda")
    a = torch.zeros(4096, device="cuda")
    b = torch.full((4096,), float(SENTINEL), device="cuda")
    A, B, N, P = a.data_ptr(), b.data_ptr(), i32.data_ptr(), i64.data_ptr()
    fixed_bad = ((1, 0, 2, 4), (1, 33, 2, 4), (1, 4, 0, 4), (1, 4, 17, 4), (1, 4, 2, 0), (-1, 4, 2, 4), (0, 33, 2, 4))
    for n, f, H, D in fixed_bad:
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_gatv2_aggregate(0, N, A, A, A, B, B, n, f, H, D, 0.2, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_gatv2_aggregate_backward(0, N, A, A, A, A, A, A, B, B, B, 1, n, f, H, D, 0.2, st))
    for n, H, D in ((1, 0, 4), (1, 17, 4), (1, 2, 0), (-1, 2, 4)):
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_gatv2_aggregate_csr(0, P, N, A, A, A, B, B, n, H, D, 0.2, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_gatv2_aggregate_csr_backward(0, P, N, A, A, A, A, A, A, B, B, B, 1, n, H, D, 0.2, st))
    for parts in (0, -3):                              # a partials buffer without a row
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_gatv2_aggregate_backward(0, N, A, A, A, A, A, A, B, B, B, parts, 1, 4, 2, 4, 0.2, st))
        with pytest.raises(RuntimeError, match="bad block shape"):
            _capi.check(L.coala_block_gatv2_aggregate_csr_backward(0, P, N, A, A, A, A, A, A, B, B, B, parts, 1, 2, 4, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_gatv2_aggregate(0, N, A, None, A, B, B, 1, 4, 2, 4, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_gatv2_aggregate(0, N, A, A, None, B, B, 1, 4, 2, 4, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_gatv2_aggregate_backward(0, N, A, A, A, A, None, A, B, B, B, 1, 1, 4, 2, 4, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_gatv2_aggregate_csr(0, None, N, A, A, A, B, B, 1, 2, 4, 0.2, st))
    with pytest.raises(RuntimeError, match="null buffer"):
        _capi.check(L.coala_block_gatv2_aggregate_csr_backward(0, P, None, A, A, A, A, A, A, B, B, B, 1, 1, 2, 4, 0.2, st))
    # n_dst == 0 is fine before any pointer is looked at; parts = 0 without a partials buffer is not a shape at all
    _capi.check(L.coala_block_gatv2_aggregate(0, None, None, None, None, None, None, 0, 4, 2, 4, 0.2, st))
    _capi.check(L.coala_block_gatv2_aggregate_csr_backward(0, None, None, None, None, None, None, None, None, None, None, None, 0, 0, 2, 4, 0.2, st))
    _capi.check(L.coala_block_gatv2_aggregate_backward(0, N, A, A, A, A, A, A, None, None, None, 0, 1, 4, 2, 4, 0.2, st))
    torch.cuda.synchronize()
    assert torch.all(b == float(SENTINEL))


@pytest.mark.parametrize("form", ["fixed", "csr"])
def test_block_gatv2_aggregate_autograd_matches_direct_calls(hiplib, form):
    """Block.gatv2_aggregate with autograd, for every subset of the three inputs that asks for a gradient: out and grad_dst bit for bit
    equal to the direct kernel calls, grad_src (float atomics in any order) and grad_attn (torch's sum of the partials) within the
    float64 bounds, and None for what was not asked."""
    import torch
    from COALA_GNN.sampler import Block
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    rng = np.random.default_rng(5 if form == "fixed" else 6)
    n_dst, n_src, H, D = 1500, 600, 4, 32
    fs, fd, attn, g = R.make_inputs(rng, n_src, n_dst, H, D, False)
    if form == "fixed":
        graph = R.fixed_nbr(rng, n_dst, 10, n_src)
        b = Block(torch.arange(n_src, device="cuda"), torch.from_numpy(graph).cuda(), n_dst)
        rows, srcs, nc = R.edges_fixed(graph)
    else:
        deg = rng.integers(0, 90, size=n_dst)
        indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        graph = (indptr, rng.integers(0, n_src, size=int(indptr[-1])).astype(np.int32))
        b = Block(torch.arange(n_src, device="cuda"), None, n_dst, indptr=torch.from_numpy(graph[0]).cuda(),
                  indices=torch.from_numpy(graph[1]).cuda())
        rows, srcs, nc = R.edges_csr(*graph)
    direct = _run(torch, L, form, graph, n_dst, n_src, fs, fd, attn, g, 0)
    ref = R.reference(rows, srcs, n_dst, n_src, nc, fs, fd, attn, g, R.default_parts(n_dst))
    R.check_all(direct, ref)
    for need in itertools.product([False, True], repeat=3):
        if not any(need):
            continue
        t = [torch.from_numpy(x).cuda().requires_grad_(n) for x, n in zip((fs, fd, attn[None]), need)]
        out = b.gatv2_aggregate(*t, negative_slope=float(SLOPE))
        (out * torch.from_numpy(g).cuda()).sum().backward()
        assert np.array_equal(out.detach().cpu().numpy().view(np.int32), direct["out"].view(np.int32))
        for x, n in zip(t, need):
            assert (x.grad is not None) == n
        if need[0]:
            R.check("gs", t[0].grad.cpu().numpy(), ref["gs"])
        if need[1]:
            assert np.array_equal(t[1].grad.cpu().numpy().view(np.int32), direct["gd"].view(np.int32))
        if need[2]:
            assert tuple(t[2].grad.shape) == (1, H, D)
            R.check("ga", t[2].grad[0].cpu().numpy(), ref["ga"])
    with torch.no_grad():                              # nothing needs a gradient: the same forward
        out = b.gatv2_aggregate(*[torch.from_numpy(x).cuda() for x in (fs, fd, attn)], negative_slope=float(SLOPE))
    assert np.array_equal(out.cpu().numpy().view(np.int32), direct["out"].view(np.int32))


@pytest.mark.parametrize("sampler", ["neighbor55", "full", "labor55"])
def test_sampled_blocks_native_agrees_with_fallback(hiplib, sampler):
    """Blocks from the samplers ([5, 5] fixed, [-1, -1] ragged, LABOR [5, 5]): native forward and backward against the float64 fallback
    (Block.gatv2_aggregate_torch on CPU float64 tensors), within the bounds."""
    import torch
    from COALA_GNN.sampler import LaborSampler, NeighborSampler
    from COALA_GNN.synthetic import powerlaw_csc
    indptr, indices = powerlaw_csc(20000, 8.0, seed=3, device="cuda")
    s = {"neighbor55": lambda: NeighborSampler([5, 5], seed=1), "full": lambda: NeighborSampler([-1, -1], seed=1),
         "labor55": lambda: LaborSampler([5, 5], seed=1)}[sampler]()
    graph = s.make_graph(indptr, indices)
    _, _, blocks = s.sample(graph, torch.randperm(20000, device="cuda")[:256])
    rng = np.random.default_rng(len(sampler))
    H, D = 4, 16
    for b in blocks:
        fs, fd, attn, gr = R.make_inputs(rng, b.num_src, b.num_dst, H, D, False)
        t = [torch.from_numpy(x).cuda().requires_grad_(True) for x in (fs, fd, attn)]
        out = b.gatv2_aggregate(*t, negative_slope=float(SLOPE))
        (out * torch.from_numpy(gr).cuda()).sum().backward()
        t64 = [torch.from_numpy(x.astype(np.float64)).requires_grad_(True) for x in (fs, fd, attn)]
        cpu = type(b)(b.src_nodes.cpu(), None if b.nbr is None else b.nbr.cpu(), b.num_dst,
                      indptr=None if b.indptr is None else b.indptr.cpu(), indices=None if b.indices is None else b.indices.cpu())
        ref_out = cpu.gatv2_aggregate_torch(*t64, negative_slope=float(SLOPE))
        (ref_out * torch.from_numpy(gr.astype(np.float64))).sum().backward()
        if b.nbr is None:
            rows, srcs, nc = R.edges_csr(b.indptr.cpu().numpy(), b.indices.cpu().numpy())
        else:
            rows, srcs, nc = R.edges_fixed(b.nbr.cpu().numpy())
        ref = R.reference(rows, srcs, b.num_dst, b.num_src, nc, fs, fd, attn, gr, R.default_parts(b.num_dst))
        for name, x in zip(("gs", "gd", "ga"), t64):                                           # the fallback is the reference
            assert np.allclose(x.grad.numpy(), ref[name][0], rtol=1e-10, atol=1e-10)
        assert np.allclose(ref_out.detach().numpy(), ref["out"][0], rtol=1e-12, atol=1e-12)
        got = dict(out=out.detach().cpu().numpy(), gs=t[0].grad.cpu().numpy(), gd=t[1].grad.cpu().numpy(), ga=t[2].grad.cpu().numpy())
        R.check_all(got, ref, log=print)


@pytest.mark.parametrize("inp", R.PARITY_INPUTS)
@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_gatv2_dispatch_parity(hiplib, form, inp):
    R.parity_check("cuda", form, inp)
