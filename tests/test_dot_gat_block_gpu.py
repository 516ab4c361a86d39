"""GPU tests of Block.dot_gat_aggregate: through autograd, the native kernels against dot_gat_aggregate_torch in float64 within the
bounds of tests/_dot_gat_ref.py; the native autograd Function must really have run (the fallback counts as failure); k is v; the packed
form with P != num_src and -1 rows, and with rows == nbr bit for bit equal to the dense form; validate=True raises IndexError before any
launch; dispatch parity (whatever the input, the shape, dtype and values of dot_gat_aggregate_torch)."""
import numpy as np
import pytest

import _dot_gat_ref as R

pytestmark = pytest.mark.gpu


class _Spy(object):
    def __init__(self, fn, name, log):
        self.fn, self.name, self.log = fn, name, log

    def apply(self, *args):
        self.log.append(self.name)
        return self.fn.apply(*args)


@pytest.fixture
def paths(monkeypatch):
    """-> (native, fallback): the names of the dot_gat autograd Functions that ran, and how often the torch fallback did."""
    from COALA_GNN import sampler as S
    native, fallback = [], []
    for name in ("_DotGatAggregate", "_DotGatAggregateCSR"):
        monkeypatch.setattr(S, name, _Spy(getattr(S, name), name, native))
    real = S.Block.dot_gat_aggregate_torch
    monkeypatch.setattr(S.Block, "dot_gat_aggregate_torch", lambda self, *a, **k: (fallback.append("dot_gat"), real(self, *a, **k))[1])
    return native, fallback


def _blocks(torch, form, rng, n_dst, n_src, f=9):
    from COALA_GNN.sampler import Block
    if form == "fixed":
        graph = R.fixed_rows(rng, n_dst, f, n_src)
        dev = Block(torch.arange(n_src, device="cuda"), torch.from_numpy(graph).cuda(), n_dst)
        return graph, dev, R.edges_fixed(graph)
    graph = R.csr_rows(rng, n_dst, f, n_src)
    dev = Block(torch.arange(n_src, device="cuda"), None, n_dst, indptr=torch.from_numpy(graph[0]).cuda(), indices=torch.from_numpy(graph[1]).cuda())
    return graph, dev, R.edges_csr(*graph)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("form", ["fixed", "csr"])
def test_block_dot_gat_aggregate_autograd(hiplib, paths, form, packed):
    """Forward and the three gradients through autograd against the float64 reference (which tests/test_dot_gat_cpu.py shows to be
    dot_gat_aggregate_torch in float64); packed: k and v have P != num_src rows, rows holds -1, and the block's own indices are zeros."""
    import itertools
    import torch
    native, fallback = paths
    rng = np.random.default_rng(5 + (form == "csr") + 2 * packed)
    n_dst, n_src, H, D = 700, 300, 4, 32
    P = 211 if packed else n_src
    graph, b, (dst, rows, nc) = _blocks(torch, form, rng, n_dst, P)
    slots = graph if form == "fixed" else graph[1]
    rows_t = None
    if packed:
        from COALA_GNN.sampler import Block
        zeros = torch.zeros(slots.shape, dtype=torch.int32, device="cuda")
        b = Block(torch.arange(n_src, device="cuda"), zeros, n_dst) if form == "fixed" else \
            Block(torch.arange(n_src, device="cuda"), None, n_dst, indptr=b.indptr, indices=zeros)
        rows_t = torch.from_numpy(slots).cuda()
    q, k, v, g = R.make_inputs(rng, P, n_dst, H, D, False)
    scale = float(R.scale_of(D))
    ref = R.reference(dst, rows, n_dst, P, nc, q, k, v, g, scale)
    first = None
    for need in itertools.product([False, True], repeat=3):
        t = [torch.from_numpy(x).cuda().requires_grad_(n) for x, n in zip((q, k, v), need)]
        out = b.dot_gat_aggregate(*t, rows=rows_t, scale=scale)
        R.check("out", out.detach().cpu().numpy(), ref["out"])
        first = out.detach() if first is None else first
        assert torch.equal(out.detach(), first)
        if any(need):
            (out * torch.from_numpy(g).cuda()).sum().backward()
        for name, x, n in zip(R.GRADS, t, need):
            assert (x.grad is not None) == n
            if n:
                R.check(name, x.grad.cpu().numpy(), ref[name])
    assert native == ["_DotGatAggregate" + ("CSR" if form == "csr" else "")] * 8 and not fallback, (native, fallback)
    # the float64 fallback on the device is the reference too
    t64 = [torch.from_numpy(x.astype(np.float64)).cuda().requires_grad_(True) for x in (q, k, v)]
    o64 = b.dot_gat_aggregate(*t64, rows=rows_t, scale=scale)
    assert fallback == ["dot_gat"]
    np.testing.assert_allclose(o64.detach().cpu().numpy(), ref["out"][0], rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("form", ["fixed", "csr"])
def test_block_dot_gat_k_is_v_and_default_scale(hiplib, paths, form):
    """k is v: autograd sums grad_k and grad_v; scale=None is D ** -0.5."""
    import torch
    native, fallback = paths
    rng = np.random.default_rng(41)
    n_dst, n_src, H, D = 400, 150, 2, 16
    _, b, (dst, rows, nc) = _blocks(torch, form, rng, n_dst, n_src)
    q, k, _, g = R.make_inputs(rng, n_src, n_dst, H, D, False)
    ref = R.reference(dst, rows, n_dst, n_src, nc, q, k, k, g, np.float32(D ** -0.5))
    kk = torch.from_numpy(k).cuda().requires_grad_(True)
    out = b.dot_gat_aggregate(torch.from_numpy(q).cuda(), kk, kk)
    (out * torch.from_numpy(g).cuda()).sum().backward()
    R.check("out", out.detach().cpu().numpy(), ref["out"])
    R.check("gk + gv", kk.grad.cpu().numpy(), (ref["gk"][0] + ref["gv"][0], ref["gk"][1] + ref["gv"][1] + R.U * np.abs(ref["gk"][0] + ref["gv"][0])))
    assert len(native) == 1 and not fallback


@pytest.mark.parametrize("form", ["fixed", "csr"])
def test_packed_rows_equal_to_the_index_give_the_dense_bits(hiplib, paths, form):
    """rows == the block's own index array: out and grad_q bit for bit those of the dense form, whether rows comes as int32 (handed
    through) or as int64 (converted once)."""
    import torch
    native, fallback = paths
    rng = np.random.default_rng(43)
    n_dst, n_src, H, D = 500, 200, 4, 16
    graph, b, _ = _blocks(torch, form, rng, n_dst, n_src)
    slots = b.nbr if form == "fixed" else b.indices
    q, k, v, g = (torch.from_numpy(x).cuda() for x in R.make_inputs(rng, n_src, n_dst, H, D, False))
    res = []
    for rows in (None, slots, slots.to(torch.int64)):
        qq = q.clone().requires_grad_(True)
        out = b.dot_gat_aggregate(qq, k, v, rows=rows)
        (out * g).sum().backward()
        res.append((out.detach(), qq.grad))
    for out, gq in res[1:]:
        assert torch.equal(out, res[0][0]) and torch.equal(gq, res[0][1])
    assert len(native) == 3 and not fallback


@pytest.mark.parametrize("form", ["fixed", "csr"])
def test_validate_raises_before_any_launch(hiplib, paths, form):
    import torch
    native, fallback = paths
    rng = np.random.default_rng(47)
    n_dst, n_src, H, D = 100, 60, 2, 8
    _, b, _ = _blocks(torch, form, rng, n_dst, n_src)
    slots = b.nbr if form == "fixed" else b.indices
    q, k, v, _ = (torch.from_numpy(x).cuda() for x in R.make_inputs(rng, n_src, n_dst, H, D, False))
    assert int(slots.max()) >= 40
    with pytest.raises(IndexError, match="40 rows"):
        b.dot_gat_aggregate(q, k[:40], v[:40], rows=slots)
    assert not native and not fallback
    out = b.dot_gat_aggregate(q, k, v, rows=slots, validate=False)          # rows in range: no check, the same result
    assert torch.equal(out, b.dot_gat_aggregate(q, k, v, rows=slots)) and len(native) == 2


def test_empty_tables_take_the_fallback(hiplib, paths):
    import torch
    from COALA_GNN.sampler import Block
    native, fallback = paths
    nbr = torch.full((5, 3), -1, dtype=torch.int32, device="cuda")
    b = Block(torch.arange(4, device="cuda"), nbr, 5)
    out = b.dot_gat_aggregate(torch.randn(5, 2, 4, device="cuda"), torch.zeros(0, 2, 4, device="cuda"), torch.zeros(0, 2, 4, device="cuda"), rows=nbr)
    assert out.shape == (5, 2, 4) and float(out.abs().max()) == 0.0 and fallback == ["dot_gat"] and not native


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("inp", R.PARITY_INPUTS)
@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_dot_gat_dispatch_parity(hiplib, paths, form, inp, packed):
    native, fallback = paths
    R.parity_check("cuda", form, inp, packed)
    native_ok = inp in ("3d", "colslice", "transposed") or (inp in ("fanout33", "nbr_slice") and form == "ragged")
    if native_ok:
        assert len(native) == 1 and native[0].endswith("CSR") == (form == "ragged"), (native, fallback)
    else:
        assert not native, f"{native}: this input is outside what the kernels take"
