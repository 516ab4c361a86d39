"""GPU tests of the attention kernels (GAT, GATv2, scaled dot-product, relation-typed GAT; coala_block_*_aggregate[_csr][_backward] in
coala_block_ops.hip) against reference-free identities whose bounds hold no term common to a softmax group -- no max|z|, |m|, |lse|,
no offset -- at a common score offset B in {0, +-30, +-1000} with unit spread: the regime where an error common to a group does not
cancel where the mathematics says it must, and which the float64 comparisons of the operator tests let through.

The identities, the regime, the cases and the derivation of every bound are in tests/_softmax_identities.py; the CPU twin
(tests/test_softmax_identities_cpu.py) shows that an fp32 evaluation in the kernels' order lies inside every bound at every case
here, and that eight wrong kernels do not -- among them the three these tests found or were built for: the dot-product backward with its
score fused into the subtraction of lse while the forward rounds it (identity 1 at B = 1000, 4.6 times the bound), the four backwards
with weights exp(e_j - lse) not divided by their own sum (the total of identity 3 at B = +-1000), and RelGAT before its G / S.

Called through the C ABI: fixed fan-outs 1, 2, 5, 32 with -1 interspersed and rows of -1 alone; CSR degrees 0, 1, 63, 64, 65, 128, 129,
200 and a row of 4,097 (65 chunks), for dot-product and RelGAT with -1 slots and a whole chunk of -1 inside a row; H in {1, 4, 16}, D in
{2, 3, 16, 65}, R in {1, 3, 64}, n_dst 0, 1, 64..300, buffers at float offsets 0 and 1.  Every output is followed by sentinel guard
words and every input is checked untouched.  Each test prints its largest error / bound per identity and output."""
import numpy as np
import pytest

import _softmax_identities as S

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e33)
GUARD = 67


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


def run(case):
    """Forward and backward of case.op through the C ABI, every float buffer at float offset case.off, sentinels around every output and
    filling the outputs that are written whole -> the twin's dict (S.twin): out, lse, gt (the summed table's gradient) and gel, ger |
    gq, gk | gd, ga (the float64 sum of the grad_attn partials)."""
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L = _capi.load()
    st = current_stream()
    n, P, H, D, R, off, op = case.n_dst, case.P, case.H, case.D, case.R, case.off, case.op
    csr = case.form == "csr"
    bufs = {k: _device(torch, v, off) for k, v in case.inp.items()}
    p = {k: b[1] for k, b in bufs.items()}
    SN = float(SENTINEL)
    new = lambda shape, fill: _device(torch, np.empty(shape, np.float32), off, fill=fill) + (shape,)   # noqa: E731
    outs = dict(out=new((n, H, D), SN), lse=new((n, R, H) if op == "rel" else (n, H), SN), gt=new((P, H, D), 0.0))
    pad = lambda a: torch.from_numpy(np.append(np.ascontiguousarray(a).reshape(-1), np.int32(-1)).astype(np.int32)).cuda()   # noqa: E731
    idx = pad(case.idx)                                                # one word past the slots: a block without slots has a buffer
    keep = [idx] + ([torch.from_numpy(case.indptr).cuda()] if csr else [])   # held until the kernels have run
    graph = [keep[1].data_ptr(), idx.data_ptr()] if csr else [idx.data_ptr()]
    dims = [n] + ([] if csr else [case.f])
    suffix = "_csr" if csr else ""
    slope, scale = float(case.slope), float(case.scale)
    if op in ("gat", "rel"):
        outs.update(gel=new((P, H), 0.0), ger=new((n, R, H) if op == "rel" else (n, H), SN))
        if op == "rel":
            typ = pad(case.typ)
            keep.append(typ)
            graph.append(typ.data_ptr())
            dims.append(R)
        o = {k: v[1] for k, v in outs.items()}
        fwd = getattr(L, f"coala_block_{'rel_' if op == 'rel' else ''}gat_aggregate{suffix}")
        bwd = getattr(L, f"coala_block_{'rel_' if op == 'rel' else ''}gat_aggregate{suffix}_backward")
        _capi.check(fwd(0, *graph, p["el"], p["er"], p["tab"], o["out"], o["lse"], *dims, H, D, slope, st))
        saved = (o["lse"],) if op == "rel" else (o["out"], o["lse"])
        _capi.check(bwd(0, *graph, p["el"], p["er"], p["tab"], *saved, p["g"], o["gt"], o["gel"], o["ger"], *dims, H, D, slope, st))
    elif op == "dot":
        outs.update(gq=new((n, H, D), SN), gk=new((P, H, D), 0.0))
        o = {k: v[1] for k, v in outs.items()}
        _capi.check(getattr(L, f"coala_block_dot_gat_aggregate{suffix}")(0, *graph, p["q"], p["k"], p["tab"], o["out"], o["lse"], *dims, H, D, scale, st))
        _capi.check(getattr(L, f"coala_block_dot_gat_aggregate{suffix}_backward")(0, *graph, p["q"], p["k"], p["tab"], o["out"], o["lse"], p["g"], o["gq"],
                                                                                o["gk"], o["gt"], *dims, H, D, scale, st))
    else:
        parts = max(1, min(-(-n // 4), 1024))
        outs.update(gd=new((n, H, D), SN), parts=new((parts, H * D), SN))
        o = {k: v[1] for k, v in outs.items()}
        _capi.check(getattr(L, f"coala_block_gatv2_aggregate{suffix}")(0, *graph, p["tab"], p["fd"], p["attn"], o["out"], o["lse"], *dims, H, D, slope, st))
        _capi.check(getattr(L, f"coala_block_gatv2_aggregate{suffix}_backward")(0, *graph, p["tab"], p["fd"], p["attn"], o["out"], o["lse"], p["g"], o["gt"],
                                                                              o["gd"], o["parts"], parts, *dims, H, D, slope, st))
    torch.cuda.synchronize()
    del keep
    res = {k: _region(flat, off, shape) for k, (flat, _, shape) in outs.items()}
    if op == "gatv2":                                                  # nothing is launched for an empty block
        res["ga"] = res["parts"].astype(np.float64).sum(0).reshape(H, D) if n else np.zeros((H, D))
    for k, v in case.inp.items():                                      # inputs untouched
        assert np.array_equal(_region(bufs[k][0], off, v.shape), v), f"{k} was written"
    if n:
        assert all(np.isfinite(res[k]).all() for k in res if k != "lse")
        assert np.all(res["gt"][P - 7:] == 0.0), "an unreferenced table row has a gradient"
    return res


def _report(case, identity, ratios):
    for k, v in ratios.items():
        print(f"ratio {case.op} identity {identity} {k}: {v:.4f}")


IDS = [S.case_id(s) for s in S.CASES]
ORDER_IDS = [S.case_id(s) for s in S.ORDER_CASES]


@pytest.mark.parametrize("spec", S.CASES, ids=IDS)
def test_score_gradients_of_a_group_sum_to_zero(hiplib, spec):
    case = S.case_of(spec)
    x = S.exact(case)
    res = run(case)
    _report(case, 1, S.check_sum_to_zero(case, x, res))
    absent = ~x.present
    if case.op == "rel":
        assert np.all(np.isneginf(res["lse"][absent])) and np.all(res["ger"][absent] == 0.0)
    else:
        assert np.all(np.isneginf(res["lse"][absent[:, 0]])) and np.all(res["out"][absent[:, 0]] == 0.0)


@pytest.mark.parametrize("spec", S.CASES, ids=IDS)
def test_partition_of_unity(hiplib, spec):
    case = S.with_table(S.case_of(spec), "ones")
    _report(case, 2, S.check_unity(case, S.exact(case), run(case)))


@pytest.mark.parametrize("spec", S.CASES, ids=IDS)
def test_constant_rows_give_no_score_gradient(hiplib, spec):
    case = S.with_table(S.case_of(spec), "const")
    _report(case, 3, S.check_constant_rows(case, S.exact(case), run(case)))


@pytest.mark.parametrize("spec", S.DISJOINT_CASES, ids=[S.case_id(s) for s in S.DISJOINT_CASES])
def test_table_gradient_of_a_row_adds_up_to_grad_out(hiplib, spec):
    """Identity 3 with every slot reading a table row of its own: the sum over a row's sources is g[d]."""
    case = S.with_table(S.case_of(spec, disjoint=True), "const")
    _report(case, 3, S.check_constant_rows(case, S.exact(case), run(case)))


@pytest.mark.parametrize("spec", S.ORDER_CASES, ids=ORDER_IDS)
def test_order_of_a_row_does_not_matter(hiplib, spec):
    case = S.case_of(spec, same_order_heads=True)
    scores = S.exact(case).scores
    orders = S.ORDERS + (("bytype",) if case.op == "rel" else ())
    res = {o: (c, run(c)) for o in orders for c in [S.reorder(case, o, scores)]}
    _report(case, 4, S.check_orders(case, res))
    for c, r in res.values():                                          # identity 1 in every layout: the rescale path of the ascending one
        _report(case, 1, S.check_sum_to_zero(c, S.exact(c), r))
    ones = S.with_table(case, "ones")                                  # identity 2 on the ascending layout of the long row
    ones = S.reorder(ones, "asc", S.exact(ones).scores)
    _report(case, 2, S.check_unity(ones, S.exact(ones), run(ones)))
