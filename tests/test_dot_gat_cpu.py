"""CPU tests of the scaled dot-product attention surface: the error bounds of the GPU tests (tests/_dot_gat_ref.py) -- an fp32 numpy
evaluation in the kernels' summation order stays inside them, three injected faults do not; Block.dot_gat_aggregate_torch (the fallback
and reference of the native kernels) against the float64 reference, dense and packed, fixed and ragged, and its gradients (gradcheck);
the shape and row checks; DotGatConv and HGTConv against a naive per-edge float64 restatement (tests/_hgt_ref.py); the state-dict names;
the HGT and DotGAT models against the global-id reference (tests/_hgt_global_ref.py), which is itself proved against the naive layer and
catches an injected fault; dispatch parity; the C ABI symbols."""
import numpy as np
import pytest

import _dot_gat_ref as R


def _block(torch, graph, n_src, **kw):
    from COALA_GNN.sampler import Block
    if isinstance(graph, tuple):
        return Block(torch.arange(n_src), None, len(graph[0]) - 1, indptr=torch.from_numpy(graph[0]), indices=torch.from_numpy(graph[1]), **kw)
    return Block(torch.arange(n_src), torch.from_numpy(graph), graph.shape[0], **kw)


def _case(form, seed, n_dst=40, f=7, P=30):
    rng = np.random.default_rng(seed)
    if form == "fixed":
        graph = R.fixed_rows(rng, n_dst, f, P)
        graph[5, 1] = graph[5, 0] = 7
        return rng, graph, R.edges_fixed(graph)
    graph = R.csr_rows(rng, n_dst, f, P)
    return rng, graph, R.edges_csr(*graph)


@pytest.mark.parametrize("case", R.SMALL_CASES)
def test_kernel_order_fp32_is_inside_the_bounds(hiplib, case):
    """The kernels restated in numpy fp32 in their own summation order (lane scan and LDS adds, butterfly sums, slot-order sums) lie
    inside the bounds the kernels are held to, at every case of the GPU test's small table."""
    row, P, (q, k, v, g), scale, (dst, rows, nc) = R.small_case(case)
    ref = R.reference(dst, rows, row.shape[0], P, nc, q, k, v, g, scale)
    R.check_all(R.kernel_order_fp32(row, q, k, v, g, scale), ref, log=print)


@pytest.mark.parametrize("fault,hit", [("no_scale", ("gq", "gk")), ("k_for_v", ("out",)), ("no_gout", ("gq", "gk"))])
@pytest.mark.parametrize("case", R.SMALL_CASES)
def test_injected_faults_are_outside_the_bounds(hiplib, case, fault, hit):
    """Three ways a kernel could be wrong -- the scale dropped from grad_k / grad_q, k summed in place of v, t_j without its -<g, out>
    term -- each land outside the bounds of the outputs they touch and leave the others alone.  At fan-out 1 every softmax is over one
    edge, a_j = 1 and t_j = 0 exactly, so only 'k_for_v' and 'no_gout' can show there; with scores of +-1e3 the softmax saturates, t_j
    is at the level of its own roundoff and a missing scale may hide, so the scale fault must show only where the scores are moderate."""
    row, P, (q, k, v, g), scale, (dst, rows, nc) = R.small_case(case)
    n_dst = row.shape[0]
    ref = R.reference(dst, rows, n_dst, P, nc, q, k, v, g, scale)
    bad = R.reference(dst, rows, n_dst, P, nc, q, k, v, g, scale, fault=fault)
    must = hit
    if fault == "no_scale" and (row.shape[1] == 1 or case[5]):
        must = ()
    for name in hit:
        n_out = R.outside(bad[name][0], ref[name])
        print(f"{fault} {name}: {n_out} of {bad[name][0].size} elements outside")
        assert n_out > 0 or name not in must, f"fault {fault!r} stays inside the bound of {name}"
    for name in set(("out", "gq", "gk", "gv")) - set(hit):
        assert R.outside(bad[name][0], ref[name]) == 0


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_dot_gat_aggregate_torch_matches_reference(hiplib, form, packed):
    """Forward and the three gradients of the float64 fallback against the closed-form reference; packed: k and v have P != num_src
    rows and the rows tensor holds -1."""
    import torch
    n_src, P = 30, (23 if packed else 30)
    rng, graph, (dst, rows, nc) = _case(form, 3 + packed, P=P)
    H, D = 3, 5
    b = _block(torch, graph, n_src)
    q, k, v, g = (x.astype(np.float64) for x in R.make_inputs(rng, P, b.num_dst, H, D, False))
    slots = graph[1] if form == "ragged" else graph
    if packed:
        nbr = np.where(slots >= 0, 0, -1).astype(np.int32)              # the block's own indices are not read in the packed form
        b = _block(torch, (graph[0], nbr) if form == "ragged" else nbr, n_src)
    t = [torch.from_numpy(x).requires_grad_(True) for x in (q, k, v)]
    out = b.dot_gat_aggregate_torch(*t, rows=torch.from_numpy(slots.astype(np.int64)) if packed else None, scale=0.3)
    (out * torch.from_numpy(g)).sum().backward()
    ref = R.reference(dst, rows, b.num_dst, P, nc, q, k, v, g, 0.3)
    np.testing.assert_allclose(out.detach().numpy(), ref["out"][0], rtol=1e-12, atol=1e-12)
    for name, x in zip(R.GRADS, t):
        np.testing.assert_allclose(x.grad.numpy(), ref[name][0], rtol=1e-10, atol=1e-10)
    assert np.all(out.detach().numpy()[ref["empty"]] == 0.0) and ref["empty"].any()
    # CPU tensors take the fallback; scale=None is D ** -0.5; k is v
    got = b.dot_gat_aggregate(t[0], t[1], t[2], rows=torch.from_numpy(slots) if packed else None, scale=0.3)
    assert torch.equal(got, out)
    kk = t[1].detach().clone().requires_grad_(True)
    o1 = b.dot_gat_aggregate(t[0].detach(), kk, kk, rows=torch.from_numpy(slots) if packed else None)
    o2 = b.dot_gat_aggregate_torch(t[0].detach(), kk.detach(), kk.detach(), rows=torch.from_numpy(slots) if packed else None, scale=D ** -0.5)
    assert torch.allclose(o1, o2, rtol=1e-13, atol=1e-13)
    o1.sum().backward()
    r2 = R.reference(dst, rows, b.num_dst, P, nc, q, kk.detach().numpy(), kk.detach().numpy(), np.ones_like(g), D ** -0.5)
    np.testing.assert_allclose(kk.grad.numpy(), r2["gk"][0] + r2["gv"][0], rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_dot_gat_aggregate_torch_gradcheck(hiplib, form):
    import torch
    rng, graph, _ = _case(form, 7, n_dst=9, f=4, P=8)
    b = _block(torch, graph, 8)
    args = [torch.from_numpy(rng.standard_normal(s)).requires_grad_(True) for s in ((b.num_dst, 2, 3), (8, 2, 3), (8, 2, 3))]
    assert torch.autograd.gradcheck(lambda q, k, v: b.dot_gat_aggregate_torch(q, k, v, scale=0.6), args)


def test_dot_gat_aggregate_refuses_bad_arguments(hiplib):
    import torch
    rng, graph, _ = _case("fixed", 2)
    b = _block(torch, graph, 30)
    q, k, v = torch.randn(40, 3, 5), torch.randn(30, 3, 5), torch.randn(30, 3, 5)
    for bad in ((q[:-1], k, v), (q, k[:-1], v[:-1]), (q, k, v[:, :2]), (q[:, :, :4], k, v), (q, k.flatten(1), v.flatten(1))):
        with pytest.raises(ValueError, match=r"\[40, H, D\]"):
            b.dot_gat_aggregate(*bad)
    rows = torch.from_numpy(graph.astype(np.int64))
    with pytest.raises(ValueError, match="one per neighbour slot"):
        b.dot_gat_aggregate(q, k, v, rows=rows[:, :-1])
    with pytest.raises(ValueError, match="integer"):
        b.dot_gat_aggregate(q, k, v, rows=rows.double())
    with pytest.raises(IndexError):
        b.dot_gat_aggregate(q, k[:20], v[:20], rows=rows)                   # rows reach 29
    assert b.dot_gat_aggregate(q, k[:20], v[:20], rows=rows.clamp_max(19)).shape == (40, 3, 5)


def test_dot_gat_symbols_resolve(hiplib):
    from COALA_GNN_Pybind import _capi
    L = _capi.load()
    for name in ("coala_block_dot_gat_aggregate", "coala_block_dot_gat_aggregate_backward", "coala_block_dot_gat_aggregate_csr",
                 "coala_block_dot_gat_aggregate_csr_backward"):
        assert getattr(L, name) is not None


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("inp", R.PARITY_INPUTS)
@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_dot_gat_dispatch_parity_cpu(hiplib, form, inp, packed):
    R.parity_check("cpu", form, inp, packed)


# ------------------------------------------------------------------------------------------------ the layers
import _hgt_ref as HR   # noqa: E402


def _layer_block(torch, form, rng, n_src=26, n_dst=14):
    """A small block with a destination without in-edges, -1 slots and repeated sources; 'bucketed': the destination rows are anywhere
    in the source list."""
    if form == "ragged":
        deg = rng.integers(0, 7, size=n_dst)
        deg[2] = 0
        deg[6] = 70                                            # more than one 64-slot chunk
        indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        return _block(torch, (indptr, rng.integers(0, n_src, size=int(indptr[-1])).astype(np.int32)), n_src)
    nbr = rng.integers(0, n_src, size=(n_dst, 6)).astype(np.int32)
    nbr[rng.random(nbr.shape) < 0.3] = -1
    nbr[2] = -1
    nbr[4, 1] = nbr[4, 0] = 3
    kw = {"dst_in_src": torch.from_numpy(rng.permutation(n_src)[:n_dst].astype(np.int32))} if form == "bucketed" else {}
    return _block(torch, nbr, n_src, **kw)


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("form", ["fixed", "ragged", "bucketed"])
def test_dotgatconv_matches_naive_layer(hiplib, form, paired):
    import torch
    from COALA_GNN.nn import DotGatConv
    rng = np.random.default_rng(31 + paired)
    b = _layer_block(torch, form, rng)
    H, D, F = 3, 4, 9
    conv = DotGatConv((F, F) if paired else F, D, H).double()
    names = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    assert names == ({"fc_src.weight": (H * D, F), "fc_dst.weight": (H * D, F)} if paired else {"fc.weight": (H * D, F)})
    x = torch.from_numpy(rng.standard_normal((b.num_src, F)))
    w_src, w_dst = ((conv.fc_src.weight, conv.fc_dst.weight) if paired else (conv.fc.weight, conv.fc.weight))
    xd = x.numpy()[HR.dst_index(b)]
    want = HR.dotgat_layer(b, x.numpy(), xd, w_src.detach().numpy(), w_dst.detach().numpy(), H, D)
    for feat in (x, (x, b.dst_rows(x))):
        np.testing.assert_allclose(conv(b, feat).detach().numpy(), want, rtol=1e-11, atol=1e-11)
    assert np.all(want[2] == 0.0)


def _hgt_params(layer):
    return {k: v.detach().numpy() for k, v in layer.state_dict().items() if not k.startswith("norm.")}


@pytest.mark.parametrize("T,R,in_size,use_norm", [(1, 1, 12, False), (3, 4, 12, True), (3, 4, 7, False), (1, 4, 7, True), (3, 1, 12, False)])
@pytest.mark.parametrize("form", ["fixed", "ragged", "bucketed"])
def test_hgtconv_matches_naive_layer(hiplib, form, T, R, in_size, use_norm):
    """T in {1, 3}; R in {1, 4} with relation 2 absent; an edge type outside the range (it sends nothing); a destination without
    in-edges (the skip path alone); in_size == H * D and != H * D; use_norm on and off; dropout 0."""
    import torch
    from COALA_GNN.nn import HGTConv
    rng = np.random.default_rng(T * 100 + R * 10 + in_size + use_norm)
    b = _layer_block(torch, form, rng)
    H, D = 3, 4
    layer = HGTConv(in_size, D, H, T, R, dropout=0.0, use_norm=use_norm).double()
    with torch.no_grad():
        for n, p in layer.named_parameters():
            p.copy_(torch.from_numpy(rng.standard_normal(tuple(p.shape)) * (0.5 if n.startswith("rel_") else 1.0)))
    slots = b.indices if b.nbr is None else b.nbr
    et = rng.integers(0, R, size=tuple(slots.shape))
    if R == 4:
        et[et == 2] = 3                                        # one relation absent
    et.reshape(-1)[::11] = R                                   # out of range: sends nothing
    et.reshape(-1)[5::13] = -1
    nt = rng.integers(0, T, size=b.num_src)
    x = torch.from_numpy(rng.standard_normal((b.num_src, in_size)))
    got = layer(b, x, torch.from_numpy(nt.astype(np.int32)), torch.from_numpy(et)).detach().numpy()
    di = HR.dst_index(b)
    want = HR.hgt_layer(b, x.numpy(), x.numpy()[di], nt, nt[di], et.reshape(-1), _hgt_params(layer), H, D)
    skip_only = want[2].copy()
    if use_norm:
        want = HR.layer_norm(want, layer.norm.weight.detach().numpy(), layer.norm.bias.detach().numpy())
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10)
    p = _hgt_params(layer)
    res = x.numpy()[di][2] if in_size == H * D else x.numpy()[di][2] @ p["residual_w"]
    np.testing.assert_allclose(skip_only, res * (1 - 1 / (1 + np.exp(-p["skip"][nt[di][2]]))), rtol=1e-12, atol=1e-12)
    got2 = layer(b, (x, b.dst_rows(x)), torch.from_numpy(nt), torch.from_numpy(et)).detach().numpy()
    assert np.array_equal(got, got2)
    if R > 1 and form == "ragged":                             # the injected fault of the reference: a softmax per relation
        bad = HR.hgt_layer(b, x.numpy(), x.numpy()[di], nt, nt[di], et.reshape(-1), p, H, D, per_relation_softmax=True)
        if use_norm:
            bad = HR.layer_norm(bad, layer.norm.weight.detach().numpy(), layer.norm.bias.detach().numpy())
        assert np.abs(bad - want).max() > 1e-3


def test_hgtconv_state_dict_and_checks(hiplib):
    import torch
    from COALA_GNN.nn import HGTConv
    T, R, H, D = 3, 4, 2, 5
    m = HGTConv(7, D, H, T, R, use_norm=True)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == {"k_weight": (T, 7, H * D), "q_weight": (T, 7, H * D), "v_weight": (T, 7, H * D), "a_weight": (T, H * D, H * D),
                      "rel_att": (R, H, D, D), "rel_msg": (R, H, D, D), "rel_pri": (R, H), "skip": (T,), "residual_w": (7, H * D),
                      "norm.weight": (H * D,), "norm.bias": (H * D,)}
    assert torch.all(m.rel_pri == 1) and torch.all(m.skip == 1)
    assert float(m.k_weight.detach().abs().max()) <= 7 ** -0.5 and float(m.rel_att.detach().abs().max()) <= D ** -0.5
    assert float(m.a_weight.detach().abs().max()) <= (H * D) ** -0.5
    assert "residual_w" not in HGTConv(H * D, D, H, T, R).state_dict() and "norm.weight" not in HGTConv(H * D, D, H, T, R).state_dict()
    rng = np.random.default_rng(1)
    b = _layer_block(torch, "fixed", rng)
    x = torch.randn(b.num_src, 7)
    et = torch.zeros(tuple(b.nbr.shape), dtype=torch.int64)
    for bad in (torch.full((b.num_src,), T), torch.full((b.num_src,), -1)):
        with pytest.raises(ValueError, match="node types"):
            m(b, x, bad, et)
    with pytest.raises(ValueError, match="node types"):
        m(b, x, torch.zeros(b.num_src - 1, dtype=torch.int64), et)
    with pytest.raises(ValueError):
        HGTConv(7, D, H, 0, R)


def test_relgatconv_pair_helper_keeps_its_results(hiplib):
    """The shared pair packing: rows name, for every valid slot, the pair (source, relation) it reads, sorted by relation then source."""
    import torch
    from COALA_GNN.nn import _pack_pairs
    rng = np.random.default_rng(4)
    b = _layer_block(torch, "fixed", rng)
    et = torch.from_numpy(rng.integers(-1, 4, size=tuple(b.nbr.shape)))
    rows, pair_rel, pair_src, counts = _pack_pairs(b, et, 3, torch.device("cpu"))
    nbr, t = b.nbr.reshape(-1).long(), et.reshape(-1)
    keep = (nbr >= 0) & (t >= 0) & (t < 3)
    assert torch.all(rows[~keep] == -1) and torch.equal(pair_rel[rows[keep]], t[keep]) and torch.equal(pair_src[rows[keep]], nbr[keep])
    key = pair_rel * b.num_src + pair_src
    assert torch.all(key[1:] > key[:-1]) and counts == torch.bincount(pair_rel, minlength=3).tolist()


# ------------------------------------------------------------------------------------------------ the models
def _model_setup(torch, kind):
    """The model of tests/test_hgt_model_gpu.py on the CPU in float64, and what its reference needs."""
    import _hgt_model_cases as HC
    model = HC.make_model(kind).double()
    return HC, model


@pytest.mark.parametrize("sampler,G", [("ns55", 0), ("nsF4", 0), ("ns55", 3)])
@pytest.mark.parametrize("kind", ["hgt", "dotgat"])
def test_global_reference_agrees_with_the_models_and_the_naive_layer(hiplib, oracle, kind, sampler, G):
    """On the samplers' numpy restatements (tests/_model_cases.reference_blocks; G = 3: an owner-bucketed input layer): the global-id
    reference in float64 agrees with the harness model run on the blocks in float64 -- logits, every parameter gradient, grad_X -- and,
    for HGT's first layer, with the naive per-edge layer of tests/_hgt_ref.py; one injected fault, a softmax per relation instead of
    over all of a node's in-edges, moves the logits."""
    import torch
    import _global_ref as GR
    import _hgt_global_ref as HG
    import _model_cases as MC
    HC, model = _model_setup(torch, kind)
    g = MC.graph()
    case = MC.Case("x", sampler, G, True, kind, 0)
    blocks = MC.reference_blocks(oracle, case)
    layers = [GR.decode(b) for b in blocks]
    Cmat = MC.loss_matrix(0)
    ref = HG.run(kind, MC.params_of(model), layers, g.X, Cmat, g.seeds, torch.float64, HC.HEADS, HC.ntype(), g.etype)
    got = HC.run(model, blocks, torch.from_numpy(g.X).double(), torch.from_numpy(Cmat).double())
    assert set(got) == set(ref)
    for name in ref:
        scale = max(1.0, float(np.abs(ref[name]).max()))
        assert np.abs(got[name] - ref[name]).max() <= 1e-10 * scale, name
    if kind == "hgt":
        bad = HG.run(kind, MC.params_of(model), layers, g.X, Cmat, g.seeds, torch.float64, HC.HEADS, HC.ntype(), g.etype, fault="per_relation")
        assert np.abs(bad["logits"] - ref["logits"]).max() > 1e-3 * np.abs(ref["logits"]).max()
        b = blocks[0]
        layer = model.layers[0]
        nt = HC.ntype()[b.src_nodes.numpy()]
        x = g.X[b.src_nodes.numpy()].astype(np.float64)
        di = HR.dst_index(b)
        et = b.edata["etype"].numpy().reshape(-1)
        want = HR.hgt_layer(b, x, x[di], nt, nt[di], et, _hgt_params(layer), layer.num_heads, layer.head_size)
        want = HR.layer_norm(want, layer.norm.weight.detach().numpy(), layer.norm.bias.detach().numpy())
        xt = torch.from_numpy(x)
        have = layer(b, (xt, b.dst_rows(xt)), torch.from_numpy(nt), b.edata["etype"]).detach().numpy()
        np.testing.assert_allclose(have, want, rtol=1e-9, atol=1e-9)


def test_hgt_model_checks(hiplib):
    import torch
    from COALA_GNN.harness import HGT
    with pytest.raises(ValueError, match="multiple"):
        HGT(8, 10, 3, 2, 4, 2, 2)
    m = HGT(8, 12, 3, 2, 4, 2, 2)
    rng = np.random.default_rng(0)
    b = _layer_block(torch, "fixed", rng)
    with pytest.raises(ValueError, match="node-type table"):
        m([b], torch.randn(b.num_src, 8))
    with pytest.raises(ValueError, match="edge_ids=True"):
        m([b], torch.randn(b.num_src, 8), ntype=torch.zeros(b.num_src, dtype=torch.int64))
