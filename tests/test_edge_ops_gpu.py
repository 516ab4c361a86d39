"""GPU tests of the message-passing primitives Block.u_dot_v / edge_softmax / u_mul_e_sum (coala_block_u_dot_v, _edge_softmax[_backward],
_u_mul_e_sum, _e_mul_v_scatter) through autograd, on fixed and ragged blocks, and of attn_drop on GATConv / DotGatConv.

Tolerance, the convention of tests/test_time_attn_gpu.py: the float64 reference is the op's _torch twin at double, the fp32 fallback the
same twin at fp32 on the GPU; every element of the native result lies within twice the fallback's largest distance from the reference
plus 4 fp32 ulps of the element's reference magnitude.  -s prints the distances."""
import types

import numpy as np
import pytest
import torch

from _time_attn_ref import block_rows

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
FIXED = [(1, 1, 1, 1), (7, 5, 3, 6), (5, 32, 16, 4), (3, 10, 4, 128), (4100, 3, 2, 8), (0, 4, 2, 8), (4, 6, 2, 7)]
DEGREES = [0, 1, 63, 64, 65, 130, 3]   # the chunk edges; the softmax tile is one 64-slot chunk, so 65 and 130 stream
OPS = {"u_dot_v": ("u", "v"), "edge_softmax": ("e",), "u_mul_e_sum": ("u", "e")}
ATOMIC = ("grad_u",)                   # the one result that float atomics add up


def _block(case, seed=0):
    """A fixed block (n_dst, fanout, H, D) with -1 padding and an all-padding row, or the ragged block ("ragged", H, D) of DEGREES, on
    n_dst + 3 sources -> (block, H, D)."""
    from COALA_GNN.sampler import Block
    rng = np.random.default_rng(seed)
    if case[0] == "ragged":
        n_dst, indptr = len(DEGREES), np.concatenate([[0], np.cumsum(DEGREES)]).astype(np.int64)
        indices = rng.integers(0, n_dst + 3, size=int(indptr[-1])).astype(np.int32)
        return Block(torch.arange(n_dst + 3).cuda(), None, n_dst, indptr=torch.from_numpy(indptr).cuda(), indices=torch.from_numpy(indices).cuda()), *case[1:]
    n_dst, fan = case[:2]
    return Block(torch.arange(n_dst + 3).cuda(), torch.from_numpy(block_rows(rng, n_dst, fan, n_dst + 3)).cuda(), n_dst), *case[2:]


def _inputs(blk, H, D, seed=1):
    """{name: float64 CPU tensor} for u, v and a per-edge e of the block."""
    g = torch.Generator().manual_seed(seed)
    slots = blk.indices if blk.nbr is None else blk.nbr
    shapes = dict(u=(blk.num_src, H, D), v=(blk.num_dst, H, D), e=tuple(slots.shape) + (H,))
    return {n: torch.randn(s, generator=g).double() for n, s in shapes.items()}


def _run(fn, x, names, dtype=torch.float32, device="cuda"):
    """fn(*inputs) and its backward against a fixed random gradient -> {out, grad_<name>}, float64 on the CPU."""
    a = [x[n].to(device=device, dtype=dtype, copy=True).requires_grad_() for n in names]
    out = fn(*a)
    out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(out))
    return {n: t.detach().double().cpu() for n, t in [("out", out)] + [("grad_" + n, t.grad) for n, t in zip(names, a)]}


def _hold(ref, low, nat, tag):
    for n, want in ref.items():
        dist = float((low[n] - want).abs().max()) if want.numel() else 0.0
        err = (nat[n] - want).abs()
        print(f"{tag} {n:8s}: fallback fp32 distance {dist:.3e} | native {float(err.max()) if err.numel() else 0.0:.3e}")
        assert (err <= 2.0 * dist + 4 * EPS * want.abs()).all(), f"{tag} {n}: native {float(err.max()):.3e} from float64, the fallback {dist:.3e}"


@pytest.fixture
def native_calls(monkeypatch):
    """-> a list that grows by one with every call of a native edge Function."""
    from COALA_GNN import sampler as S
    calls = []
    for name in ("_UDotV", "_EdgeSoftmax", "_UMulESum"):
        monkeypatch.setattr(S, name, types.SimpleNamespace(apply=lambda *a, real=getattr(S, name): (calls.append(1), real.apply(*a))[1]))
    return calls


@pytest.mark.parametrize("case", FIXED + [("ragged", 3, 6), ("ragged", 4, 32)], ids=str)
def test_native_against_float64(hiplib, native_calls, case):
    blk, H, D = _block(case)
    x = _inputs(blk, H, D)
    for op, names in OPS.items():
        ref = _run(getattr(blk, op + "_torch"), x, names, torch.float64, "cpu")
        low = _run(getattr(blk, op + "_torch"), x, names)
        nat, again = _run(getattr(blk, op), x, names), _run(getattr(blk, op), x, names)
        _hold(ref, low, nat, f"{case} {op}")
        for n in nat:   # a second run gives the same bits, the atomics' sum apart
            assert n in ATOMIC or torch.equal(nat[n], again[n]), (op, n)
    assert len(native_calls) == 6, "the native kernels did not run"


def test_block_forms_agree_bit_for_bit(hiplib, native_calls):
    """The rows of a fixed block, padding included, as a ragged block; and H = 1 against weighted_sum_aggregate."""
    from COALA_GNN.sampler import Block
    blk, H, D = _block((7, 5, 3, 6))
    csr = Block(blk.src_nodes, None, 7, indptr=(torch.arange(8) * 5).cuda(), indices=blk.nbr.reshape(-1))
    x = _inputs(blk, H, D)
    flat = dict(x, e=x["e"].reshape(-1, H))
    for op, names in OPS.items():
        a, b = _run(getattr(blk, op), x, names), _run(getattr(csr, op), flat, names)
        for n in a:
            assert n in ATOMIC or torch.equal(a[n].reshape(b[n].shape), b[n]), (op, n)
    u, w = x["u"][:, :1].float().cuda().contiguous(), x["e"][..., 0].float().cuda().contiguous()
    assert torch.equal(blk.u_mul_e_sum(u, w.unsqueeze(-1))[:, 0], blk.weighted_sum_aggregate(u[:, 0], w))
    assert len(native_calls) == 7


@pytest.mark.parametrize("case", [(7, 5, 3, 6), ("ragged", 3, 6)], ids=str)
def test_edge_softmax_identities(hiplib, native_calls, case):
    """Rows sum to 1, padding is exactly 0, and a common offset of 1000 changes nothing: the scores are multiples of 1/64, so that
    e + 1000 is exact in fp32 and the shifted input is the same problem, not a rounded one."""
    blk, H, _ = _block(case)
    e = (_inputs(blk, H, 1)["e"] * 64).round() / 64
    a = blk.edge_softmax(e.float().cuda()).double().cpu()
    slots = (blk.indices if blk.nbr is None else blk.nbr).cpu()
    assert not a[slots < 0].any()
    rows, _, at = blk._edge_slots("cpu")
    sums = torch.zeros(blk.num_dst, H, dtype=torch.float64).index_add(0, rows, a.reshape(-1, H)[at])
    has = torch.bincount(rows, minlength=blk.num_dst) > 0
    assert not sums[~has].any() and float((sums[has] - 1.0).abs().max()) <= 4 * EPS
    ref = {"out": blk.edge_softmax_torch(e)}
    low = {"out": blk.edge_softmax_torch((e + 1000).float().cuda()).double().cpu()}
    _hold(ref, low, {"out": blk.edge_softmax((e + 1000).float().cuda()).double().cpu()}, f"{case} shifted")
    assert len(native_calls) == 2


@pytest.mark.parametrize("score", ["dot", "gat"])
def test_chain_equals_the_fused_attention(hiplib, native_calls, score):
    """u_mul_e_sum(edge_softmax(score)) against dot_gat_aggregate_torch / gat_aggregate_torch at float64."""
    blk, H, D = _block((7, 5, 3, 6))
    g = torch.Generator().manual_seed(4)
    if score == "dot":
        names, x = ("q", "k", "v"), {n: torch.randn(s, H, D, generator=g).double() for n, s in (("q", 7), ("k", 10), ("v", 10))}
        fused = lambda q, k, v: blk.dot_gat_aggregate_torch(q, k, v, scale=D ** -0.5)
        chain = lambda q, k, v: blk.u_mul_e_sum(v, blk.edge_softmax(blk.u_dot_v(k, q) * D ** -0.5))
    else:
        names, x = ("el", "er", "f"), {"el": torch.randn(10, H, generator=g).double(), "er": torch.randn(7, H, generator=g).double(),
                                      "f": torch.randn(10, H, D, generator=g).double()}
        fused = lambda el, er, f: blk.gat_aggregate_torch(el, er, f, 0.2)
        chain = lambda el, er, f: blk.u_mul_e_sum(f, blk.edge_softmax(torch.nn.functional.leaky_relu(blk.u_add_v(el, er), 0.2)))
    _hold(_run(fused, x, names, torch.float64, "cpu"), _run(fused, x, names), _run(chain, x, names), score)
    assert len(native_calls) == (3 if score == "dot" else 2)


def test_dispatch_takes_the_twin(hiplib, native_calls):
    """float64, H = 17, a CPU block and fan-out 33 never reach a native Function: the twins' shapes and values."""
    from COALA_GNN.sampler import Block
    g = torch.Generator().manual_seed(1)
    nbr = torch.randint(-1, 9, (6, 33), generator=g).to(torch.int32)
    for where, dtype, H, fan in [("cuda", torch.float64, 2, 4), ("cuda", torch.float32, 17, 4), ("cpu", torch.float32, 2, 4), ("cuda", torch.float32, 2, 33)]:
        blk = Block(torch.arange(9).to(where), nbr[:, :fan].contiguous().to(where), 6)
        u, v = torch.randn(9, H, 8, generator=g).to("cuda", dtype), torch.randn(6, H, 8, generator=g).to("cuda", dtype)
        e = blk.u_dot_v(u, v)
        assert e.shape == (6, fan, H) and e.dtype == dtype and torch.equal(e, blk.u_dot_v_torch(u, v))
        out = blk.u_mul_e_sum(u, e)
        assert out.shape == (6, H, 8)
        for got, want in ((blk.edge_softmax(e), blk.edge_softmax_torch(e)), (out, blk.u_mul_e_sum_torch(u, e))):
            torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)   # index_add's atomics reorder sums
    assert not native_calls, "a case outside the native bounds reached the kernel"


@pytest.mark.parametrize("layer", ["GATConv", "DotGatConv"])
def test_attn_drop(hiplib, native_calls, layer):
    """attn_drop = 0, and eval mode, are the layer as it was, bit for bit; in training the layer is the chain on the _torch twins
    under the same seed (the mask is torch's in both)."""
    from COALA_GNN import nn
    blk, H, D = _block((7, 5, 3, 6))
    make = lambda **kw: (nn.GATConv((8, 8), D, H, **kw) if layer == "GATConv" else nn.DotGatConv(8, D, H, **kw)).cuda()
    plain, drop = make(), make(attn_drop=0.5)
    drop.load_state_dict(plain.state_dict())
    h = torch.randn(10, 8, generator=torch.Generator().manual_seed(5)).cuda()
    feat = (h, h[:7])
    zero = make(attn_drop=0.0)
    zero.load_state_dict(plain.state_dict())
    assert torch.equal(zero(blk, feat), plain(blk, feat)) and torch.equal(drop.eval()(blk, feat), plain(blk, feat)) and not native_calls
    twins, _, _ = _block((7, 5, 3, 6))
    for op in OPS:
        setattr(twins, op, getattr(twins, op + "_torch"))
    torch.manual_seed(6)
    got = drop.train()(blk, feat)
    torch.manual_seed(6)
    want = drop(twins, feat)
    assert len(native_calls) == (2 if layer == "GATConv" else 3) and not torch.equal(got, plain(blk, feat))
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
