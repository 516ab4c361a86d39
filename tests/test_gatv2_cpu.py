"""CPU tests of the GATv2 surface: Block.gatv2_aggregate_torch (the fallback and reference of the native kernels) against a plain-loop
float64 restatement of the formulas, its gradients (gradcheck), GATv2Conv's DGL parameter names and its forward against the formula
written out with the [E, H, D] tensors, dispatch parity, the C ABI symbols, and the error bounds of the GPU tests (tests/_gatv2_ref.py):
the fp32 fallback stays inside them, three injected faults do not."""
import numpy as np
import pytest

import _gatv2_ref as R

SLOPE = 0.2


def _ref_loop(rows_of, fs, fd, attn, slope=SLOPE):
    """Plain loops, float64: rows_of[d] lists the source of every valid in-edge of d, in order.  -> out [n_dst, H, D], lse [n_dst, H]"""
    n_dst, H, D = len(rows_of), fs.shape[1], fs.shape[2]
    out = np.zeros((n_dst, H, D))
    lse = np.full((n_dst, H), -np.inf)
    for d, srcs in enumerate(rows_of):
        for h in range(H):
            e = []
            for s in srcs:
                acc = 0.0
                for c in range(D):
                    z = fs[s, h, c] + fd[d, h, c]
                    acc += attn[h, c] * (z if z > 0 else slope * z)
                e.append(acc)
            if not e:
                continue
            m = max(e)
            tot = sum(np.exp(x - m) for x in e)
            lse[d, h] = m + np.log(tot)
            for s, x in zip(srcs, e):
                out[d, h] += np.exp(x - m) / tot * fs[s, h]
    return out, lse


def _fixed_case(rng, n_dst=40, f=7, n_src=30, H=3, D=5):
    nbr = rng.integers(0, n_src, size=(n_dst, f)).astype(np.int32)
    nbr[rng.random((n_dst, f)) < 0.3] = -1                 # -1 anywhere in a row
    nbr[3] = -1                                            # a row without a valid edge
    nbr[4, :] = nbr[4, 0] if nbr[4, 0] >= 0 else 2         # one source repeated over a whole row
    nbr[5, 1] = nbr[5, 0] = 7                              # a source twice
    rows_of = [[int(s) for s in r if s >= 0] for r in nbr]
    return nbr, rows_of


def _ragged_case(rng, n_dst=25, n_src=40):
    deg = rng.integers(0, 12, size=n_dst)
    deg[[0, 7]] = 0                                        # rows without an edge
    deg[9] = 150                                           # longer than one 64-edge chunk
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rng.integers(0, n_src, size=int(indptr[-1])).astype(np.int32)
    indices[indptr[3]: indptr[4]] = 5                      # repeated sources
    rows_of = [[int(s) for s in indices[indptr[d]: indptr[d + 1]]] for d in range(n_dst)]
    return indptr, indices, rows_of


def _feats(rng, n_src, n_dst, H, D):
    return rng.standard_normal((n_src, H, D)), rng.standard_normal((n_dst, H, D)), rng.standard_normal((H, D))


def _fixed_block(torch, nbr, n_src, **kw):
    from COALA_GNN.sampler import Block
    return Block(torch.arange(n_src), torch.from_numpy(nbr), nbr.shape[0], **kw)


def _ragged_block(torch, indptr, indices, n_src):
    from COALA_GNN.sampler import Block
    return Block(torch.arange(n_src), None, len(indptr) - 1, indptr=torch.from_numpy(indptr), indices=torch.from_numpy(indices))


@pytest.mark.parametrize("H,D", [(1, 1), (1, 5), (3, 1), (3, 5)])
@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_gatv2_aggregate_torch_matches_loops(hiplib, form, H, D):
    import torch
    rng = np.random.default_rng(H * 10 + D + (form == "fixed"))
    if form == "fixed":
        nbr, rows_of = _fixed_case(rng)
        b, n_src, empty = _fixed_block(torch, nbr, 30), 30, [3]
        rows, srcs, nc = R.edges_fixed(nbr)
    else:
        indptr, indices, rows_of = _ragged_case(rng)
        b, n_src, empty = _ragged_block(torch, indptr, indices, 40), 40, [0, 7]
        rows, srcs, nc = R.edges_csr(indptr, indices)
    fs, fd, attn = _feats(rng, n_src, b.num_dst, H, D)
    ref, _ = _ref_loop(rows_of, fs, fd, attn)
    for a in (attn, attn[None]):                           # [H, D] and DGL's [1, H, D]
        got = b.gatv2_aggregate_torch(torch.from_numpy(fs), torch.from_numpy(fd), torch.from_numpy(a), SLOPE).numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
        assert np.all(got[empty] == 0.0) and np.isfinite(got).all()
    got = b.gatv2_aggregate(torch.from_numpy(fs), torch.from_numpy(fd), torch.from_numpy(attn[None]), SLOPE).numpy()   # CPU tensors: the fallback
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    # the closed-form float64 reference of the GPU tests states the same function
    g = rng.standard_normal((b.num_dst, H, D))
    ref64 = R.reference(rows, srcs, b.num_dst, n_src, nc, fs, fd, attn, g, 1, slope=SLOPE)
    np.testing.assert_allclose(ref64["out"][0], ref, rtol=1e-12, atol=1e-12)


def test_gatv2_aggregate_refuses_mismatched_shapes(hiplib):
    import torch
    rng = np.random.default_rng(2)
    nbr, _ = _fixed_case(rng)
    b = _fixed_block(torch, nbr, 30)
    fs, fd, attn = (torch.from_numpy(x) for x in _feats(rng, 30, 40, 3, 5))
    with pytest.raises(ValueError):
        b.gatv2_aggregate(fs, fd[:-1], attn)
    with pytest.raises(ValueError):
        b.gatv2_aggregate(fs, fd, attn[:, :4])


def _off_kink(rng, shape, offset):
    """Values offset + 0.04 i: the sum of a source value (offset 0.02) and a destination value (offset 0) is 0.02 + 0.04 n, at least 0.02 from 0."""
    return offset + 0.04 * rng.integers(-40, 40, size=shape).astype(np.float64)


@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_gatv2_aggregate_torch_gradcheck(hiplib, form):
    """float64 gradcheck away from the kink: every |z_jc| >= 1e-2, the finite-difference step is 1e-6."""
    import torch
    rng = np.random.default_rng(7)
    if form == "fixed":
        nbr, _ = _fixed_case(rng, n_dst=9, f=4, n_src=8)
        b, n_src = _fixed_block(torch, nbr, 8), 8
        rows, srcs, _ = R.edges_fixed(nbr)
    else:
        indptr, indices, _ = _ragged_case(rng, n_dst=12, n_src=10)
        b, n_src = _ragged_block(torch, indptr, indices, 10), 10
        rows, srcs, _ = R.edges_csr(indptr, indices)
    H, D = 2, 3
    fs, fd = _off_kink(rng, (n_src, H, D), 0.02), _off_kink(rng, (b.num_dst, H, D), 0.0)
    assert np.abs(fs[srcs] + fd[rows]).min() >= 1e-2
    attn = rng.standard_normal((1, H, D))
    args = [torch.from_numpy(x).requires_grad_(True) for x in (fs, fd, attn)]
    assert torch.autograd.gradcheck(lambda s, d, a: b.gatv2_aggregate_torch(s, d, a, SLOPE), args)


@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_reference_gradients_are_the_fallbacks(hiplib, form):
    """The closed-form float64 gradients of tests/_gatv2_ref.py against autograd through the float64 fallback."""
    import torch
    rng = np.random.default_rng(9)
    if form == "fixed":
        nbr, _ = _fixed_case(rng)
        b, n_src = _fixed_block(torch, nbr, 30), 30
        rows, srcs, nc = R.edges_fixed(nbr)
    else:
        indptr, indices, _ = _ragged_case(rng)
        b, n_src = _ragged_block(torch, indptr, indices, 40), 40
        rows, srcs, nc = R.edges_csr(indptr, indices)
    fs, fd, attn = _feats(rng, n_src, b.num_dst, 3, 5)
    g = rng.standard_normal((b.num_dst, 3, 5))
    t = [torch.from_numpy(x).requires_grad_(True) for x in (fs, fd, attn)]
    (b.gatv2_aggregate_torch(*t, SLOPE) * torch.from_numpy(g)).sum().backward()
    ref = R.reference(rows, srcs, b.num_dst, n_src, nc, fs, fd, attn, g, 1, slope=SLOPE)
    for name, x in zip(("gs", "gd", "ga"), t):
        np.testing.assert_allclose(x.grad.numpy(), ref[name][0], rtol=1e-10, atol=1e-10)


def test_gatv2conv_parameters_follow_dgl(hiplib):
    from COALA_GNN.nn import GATv2Conv
    m = GATv2Conv((12, 10), 6, 4)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == {"fc_src.weight": (24, 12), "fc_src.bias": (24,), "fc_dst.weight": (24, 10), "fc_dst.bias": (24,), "attn": (1, 4, 6)}
    assert all(float(b.detach().abs().max()) == 0.0 for b in (m.fc_src.bias, m.fc_dst.bias))
    nb = GATv2Conv(12, 6, 4, bias=False)
    assert {k: tuple(v.shape) for k, v in nb.state_dict().items()} == {"fc_src.weight": (24, 12), "fc_dst.weight": (24, 12), "attn": (1, 4, 6)}
    sh = GATv2Conv(12, 6, 4, share_weights=True)
    assert sh.fc_dst is sh.fc_src
    assert sorted(n for n, _ in sh.named_parameters()) == ["attn", "fc_src.bias", "fc_src.weight"]
    assert sum(p.dim() == 2 for p in sh.parameters()) == 1                      # one weight
    m.load_state_dict({k: v.clone() for k, v in GATv2Conv((12, 10), 6, 4).state_dict().items()}, strict=True)


def _dgl_formula(torch, rows, srcs, n_dst, feat_src, feat_dst, attn, slope):
    """DGL's GATv2Conv.forward with its [E, H, D] tensors written out: u_add_v, leaky_relu, the attn product, edge_softmax, u_mul_e_sum."""
    r, s = torch.from_numpy(rows), torch.from_numpy(srcs)
    e = torch.nn.functional.leaky_relu(feat_src[s] + feat_dst[r], slope)              # u_add_v, then leaky_relu: [E, H, D]
    e = (e * attn).sum(-1, keepdim=True)                                               # [E, H, 1]
    out = torch.zeros((n_dst,) + tuple(feat_src.shape[1:]), dtype=feat_src.dtype)
    for d in range(n_dst):                                                             # edge_softmax over each destination's in-edges
        sel = r == d
        if sel.any():
            out[d] = (torch.softmax(e[sel], dim=0) * feat_src[s[sel]]).sum(0)           # u_mul_e_sum
    return out


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("form", ["fixed", "ragged", "bucketed"])
def test_gatv2conv_matches_dgl_formula(hiplib, form, share):
    import torch
    from COALA_GNN.nn import GATv2Conv
    rng = np.random.default_rng(13)
    n_src = 60
    dst_in_src = None
    if form == "ragged":
        indptr, indices, _ = _ragged_case(rng, n_src=n_src)
        b = _ragged_block(torch, indptr, indices, n_src)
        rows, srcs, _ = R.edges_csr(indptr, indices)
    else:
        nbr, _ = _fixed_case(rng, n_dst=40, n_src=n_src)
        if form == "bucketed":                             # the destination rows are anywhere in the source list
            dst_in_src = torch.from_numpy(rng.permutation(n_src)[:40].astype(np.int32))
        b = _fixed_block(torch, nbr, n_src, dst_in_src=dst_in_src)
        rows, srcs, _ = R.edges_fixed(nbr)
    H, D, F = 3, 4, 9
    conv = GATv2Conv(F, D, H, share_weights=share).double()
    with torch.no_grad():
        for p in conv.parameters():
            p.copy_(torch.from_numpy(rng.standard_normal(tuple(p.shape))))
    x = torch.from_numpy(rng.standard_normal((n_src, F)))
    x_dst = b.dst_rows(x)
    got = conv(b, (x, x_dst)).detach()
    feat_src = (x @ conv.fc_src.weight.T + conv.fc_src.bias).view(-1, H, D)
    feat_dst = (x_dst @ conv.fc_dst.weight.T + conv.fc_dst.bias).view(-1, H, D)
    if share:
        idx = torch.arange(b.num_dst) if dst_in_src is None else dst_in_src.long()
        assert torch.allclose(feat_dst, feat_src[idx], rtol=1e-13, atol=1e-13)
        feat_dst = feat_src[idx]
    ref = _dgl_formula(torch, rows, srcs, b.num_dst, feat_src, feat_dst, conv.attn, conv.negative_slope).detach()
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-10, atol=1e-10)
    empty = sorted(set(range(b.num_dst)) - set(rows.tolist()))
    assert empty and np.all(got.numpy()[empty] == 0.0)


def test_gatv2conv_share_weights_uses_dst_rows(hiplib):
    """On an owner-bucketed block feat_src[:num_dst] is wrong; with share_weights the layer must gather through dst_in_src, and must
    not read h_dst."""
    import torch
    from COALA_GNN.nn import GATv2Conv
    rng = np.random.default_rng(17)
    nbr, _ = _fixed_case(rng, n_dst=40, n_src=60)
    perm = torch.from_numpy(rng.permutation(60)[:40].astype(np.int32))
    bucketed = _fixed_block(torch, nbr, 60, dst_in_src=perm)
    plain = _fixed_block(torch, nbr, 60)
    conv = GATv2Conv(9, 4, 3, share_weights=True).double()
    x = torch.from_numpy(rng.standard_normal((60, 9)))
    got = conv(bucketed, (x, None))
    feat_src = conv.fc_src(x).view(-1, 3, 4)
    want = bucketed.gatv2_aggregate_torch(feat_src, feat_src[perm.long()], conv.attn, 0.2)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert not torch.allclose(got, conv(plain, (x, None)), rtol=1e-3, atol=1e-3)


def test_gatv2_model_builds_and_runs_on_cpu_blocks(hiplib):
    import torch
    from COALA_GNN.harness import GATv2
    rng = np.random.default_rng(19)
    nbr1 = rng.integers(-1, 30, size=(12, 5)).astype(np.int32)     # layer 1: 12 dst among 30 src
    nbr2 = rng.integers(-1, 12, size=(4, 5)).astype(np.int32)      # layer 2: 4 dst among 12 src
    blocks = [_fixed_block(torch, nbr1, 30), _fixed_block(torch, nbr2, 12)]
    x = torch.randn(30, 8)
    for share in (False, True):
        out = GATv2(8, 6, 5, 2, 4, share_weights=share)(blocks, x)
        assert out.shape == (4, 5) and torch.allclose(out.exp().sum(1), torch.ones(4), atol=1e-5)


@pytest.mark.parametrize("inp", R.PARITY_INPUTS)
@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_gatv2_dispatch_parity_cpu(hiplib, form, inp):
    R.parity_check("cpu", form, inp)


def test_gatv2_symbols_resolve(hiplib):
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    for name in ("coala_block_gatv2_aggregate", "coala_block_gatv2_aggregate_backward", "coala_block_gatv2_aggregate_csr",
                 "coala_block_gatv2_aggregate_csr_backward"):
        assert getattr(L, name) is not None
    assert L.coala_abi_version() == 4


def _small_case(torch, case):
    """A fixed case of the GPU test (tests/_gatv2_ref.SMALL_CASES) as a CPU block, with its float64 reference."""
    n_dst, f, H, D, off, big = case
    rng = np.random.default_rng(n_dst * 7 + f * 131 + H * 17 + D + off)
    n_src = max(64, min(5000, n_dst // 4))
    nbr = R.fixed_nbr(rng, n_dst, f, n_src - 7)
    fs, fd, attn, g = R.make_inputs(rng, n_src, n_dst, H, D, big)
    rows, srcs, nc = R.edges_fixed(nbr)
    return nbr, n_src, (fs, fd, attn, g), (rows, srcs, nc)


@pytest.mark.parametrize("case", R.SMALL_CASES)
def test_fp32_fallback_is_inside_the_bounds(hiplib, case):
    """The fallback evaluated in fp32 on the CPU, forward and autograd backward, is a correct fp32 evaluation in another summation
    order: it lies inside the bounds the kernels are held to, at the GPU test's small shapes."""
    import torch
    nbr, n_src, (fs, fd, attn, g), (rows, srcs, nc) = _small_case(torch, case)
    n_dst = nbr.shape[0]
    parts = R.default_parts(n_dst)
    ref = R.reference(rows, srcs, n_dst, n_src, nc, fs, fd, attn, g, parts)
    b = _fixed_block(torch, nbr, n_src)
    t = [torch.from_numpy(x).requires_grad_(True) for x in (fs, fd, attn)]
    out = b.gatv2_aggregate_torch(*t, float(R.SLOPE))
    (out * torch.from_numpy(g)).sum().backward()
    got = dict(out=out.detach().numpy(), gs=t[0].grad.numpy(), gd=t[1].grad.numpy(), ga=t[2].grad.numpy())
    R.check_all(got, ref, log=print)


@pytest.mark.parametrize("fault,hit", [("v1", ("out", "gs", "gd", "ga")), ("no_t", ("gs",)), ("kink", ("gs", "gd"))])
@pytest.mark.parametrize("case", R.SMALL_CASES)
def test_injected_faults_are_outside_the_bounds(hiplib, case, fault, hit):
    """Three ways a kernel could be wrong -- GAT's score (attn applied after the sum over c), grad_src without its t_j attn k term, k_jc
    on the wrong side of 0 -- each land outside the bounds in every output they touch (with saturating scores: in the first).  At fan-out 1 no fault can show: every softmax is over one
    edge, a_j = 1 and t_j = 0 whatever the score, so the faulty values must then be the right ones."""
    import torch
    nbr, n_src, (fs, fd, attn, g), (rows, srcs, nc) = _small_case(torch, case)
    n_dst = nbr.shape[0]
    parts = R.default_parts(n_dst)
    ref = R.reference(rows, srcs, n_dst, n_src, nc, fs, fd, attn, g, parts)
    bad = R.reference(rows, srcs, n_dst, n_src, nc, fs, fd, attn, g, parts, fault=fault)
    touched = hit
    if nbr.shape[1] == 1:
        touched = hit = ()
    elif case[5]:
        # scores of +-1e3 saturate the softmax: a_j is 0 or 1 to many digits and t_j = a_j (dot_j - <g, out>) is at the level of its own
        # roundoff, so a fault in what passes through t_j alone (grad_dst, grad_attn) may hide; the first output it touches must show it
        hit = hit[:1]
    for name in touched:
        n_out = R.outside(bad[name][0], ref[name])
        print(f"{fault} {name}: {n_out} of {bad[name][0].size} elements outside")
        assert n_out > 0 or name not in hit, f"fault {fault!r} stays inside the bound of {name}"
    for name in set(("out", "gs", "gd", "ga")) - set(touched):
        assert R.outside(bad[name][0], ref[name]) == 0
