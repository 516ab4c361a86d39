"""CPU twin of tests/test_softmax_identities_gpu.py: the bounds of tests/_softmax_identities.py hold for an fp32 evaluation in the kernels'
summation order and for the float64 torch fallbacks, at every case the GPU test runs, and kernels that are wrong in the ways that the
float64 comparisons cannot see break them.

Which identity sees which fault:
  rel_G            RelGAT's t_j = a_j (dot_j - G), the kernel before G / S: identity 1 at B = +-1000, where the group's a_j sum to 1 + delta
                   with delta ~ u |lse|;
  no_rescale_out,  the online softmax not rescaling the partial out, or l, in a chunk that raises the maximum: identities 2 and 4 on
  no_rescale_l     the ascending layout of a long row (in the descending layout the factor is 1 and the fault does nothing);
  gout_head        <g, out> of the neighbouring head: identity 3;
  raw_a            the backward's weights exp(e_j - lse) not divided by their sum S (the kernels as these tests found them): the table
                   gradient's sum over a row's own sources, identity 3, at B = +-1000, where S = 1 + O(u |lse|);
  lse_m            lse = m, log l dropped: identity 5, lse against float64; and, for a backward that does not divide by S, identity 3
                   at every B (S = l then).  The score gradients of identities 1 and 3 are blind to it by construction -- S
                   only multiplies <g, out*> - <g, out~>, which is rounding -- and a backward that divides by S does not depend on lse's
                   error at all;
  skip_lane63      the weighted sum skipping lane 63: identities 2 and 4 at degree 64;
  dot_fma          the dot-product backward forming scale * qk - lse as one fma while the forward rounds the product (the kernel as these
                   tests found it): identity 1 on fixed rows at B = +-1000."""
import numpy as np
import pytest

import _softmax_identities as S

IDS = [S.case_id(s) for s in S.CASES]
ORDER_IDS = [S.case_id(s) for s in S.ORDER_CASES]


def _three(case, run, u):
    """Identities 1 to 3 of one case under `run` (case -> result dict) -> ratios."""
    ratios = {}
    for table, check in (("rand", S.check_sum_to_zero), ("ones", S.check_unity), ("const", S.check_constant_rows)):
        c = S.with_table(case, table)
        for k, v in check(c, S.exact(c), run(c), u).items():
            ratios[f"{check.__name__[6:]} {k}"] = v
    return ratios


def _layouts(spec, run, table="rand"):
    case = S.case_of(spec, table=table, same_order_heads=True)
    scores = S.exact(case).scores
    orders = S.ORDERS + (("bytype",) if case.op == "rel" else ())
    return case, {o: (c, run(c)) for o in orders for c in [S.reorder(case, o, scores)]}


def test_cases_cover_the_regime():
    for op in S.OPS:
        mine = [s for s in S.CASES if s[0] == op]
        col = lambda i, sel=lambda s: True: {s[i] for s in mine if sel(s)}   # noqa: E731
        assert col(8) == set(S.OFFSETS) and col(4) == {1, 4, 16} and col(5) == {2, 3, 16, 65} and col(7) == {0, 1}
        assert col(3, lambda s: s[1] == "fixed") == {1, 2, 5, 32} and col(6) == {1, 3, 64} and {0, 1} < col(2) and max(col(2)) <= 300
        assert col(9) == {0, 4097} and {s[9] for s in S.ORDER_CASES if s[0] == op} == {0, 4097}
    case = S.case_of(next(s for s in S.CASES if s[0] == "dot" and s[1] == "csr" and s[2] >= 64))
    deg = np.diff(case.indptr)
    assert set(S.DEGS) <= set(deg.tolist())
    d = int(np.nonzero(deg == 200)[0][0])                          # a whole chunk of -1 inside a row
    assert np.all(case.idx[case.indptr[d] + 64: case.indptr[d] + 128] == -1) and np.any(case.idx[case.indptr[d]: case.indptr[d] + 64] >= 0)


@pytest.mark.parametrize("spec", S.CASES, ids=IDS)
def test_twin_is_inside_the_bounds(spec):
    ratios = _three(S.case_of(spec), S.twin, S.U32)
    print(ratios)


@pytest.mark.parametrize("spec", S.ORDER_CASES, ids=ORDER_IDS)
def test_twin_layouts_agree(spec):
    case, res = _layouts(spec, S.twin)
    print(S.check_orders(case, res))
    for c, r in res.values():                                      # identity 1 in every layout
        S.check_sum_to_zero(c, S.exact(c), r)


@pytest.mark.parametrize("spec", S.CASES, ids=IDS)
def test_float64_fallbacks_are_inside_the_bounds(hiplib, spec):
    """The plain-torch fallbacks, the reference everything else leans on, in float64 with autograd."""
    print(_three(S.case_of(spec), S.fallback64, S.U64))


@pytest.mark.parametrize("spec", S.ORDER_CASES, ids=ORDER_IDS)
def test_float64_fallback_layouts_agree(hiplib, spec):
    case, res = _layouts(spec, S.fallback64)
    print(S.check_orders(case, res, S.U64))


REL_1000 = [s for s in S.CASES if s[0] == "rel" and abs(s[8]) == 1000 and s[2] > 1 and s[6] < 64]


@pytest.mark.parametrize("spec", REL_1000, ids=[S.case_id(s) for s in REL_1000])
def test_relgat_without_the_division_breaks_identity_1(spec):
    assert {s[8] for s in REL_1000} == {1000.0, -1000.0}
    case = S.case_of(spec)
    x = S.exact(case)
    S.check_sum_to_zero(case, x, S.twin(case))
    bad, msg = S.violates(S.check_sum_to_zero, case, x, S.twin(case, "rel_G"))
    print(msg)
    assert bad and "grad_er" in msg


DOT_1000 = [s for s in S.CASES if s[0] == "dot" and abs(s[8]) == 1000 and s[1] == "fixed" and s[2] > 1]


@pytest.mark.parametrize("spec", DOT_1000, ids=[S.case_id(s) for s in DOT_1000])
def test_dot_product_with_a_fused_backward_score_breaks_identity_1(spec):
    """What the dot-product backward did before dot_score: scale * qk - lse as one fma, against the forward's rounded product.  The
    fixed rows show it (their fp32 twin with this fault reproduces what the kernel gave, 4.6 times the bound at B = +1000); in rows of
    60 to 200 edges the perturbations, independent from edge to edge, average out against a worst-case bound that grows with k."""
    assert {s[8] for s in DOT_1000} == {1000.0, -1000.0}
    case = S.case_of(spec)
    x = S.exact(case)
    S.check_sum_to_zero(case, x, S.twin(case))
    bad, msg = S.violates(S.check_sum_to_zero, case, x, S.twin(case, "dot_fma"))
    print(msg)
    assert bad and "grad_q" in msg


LONG = [s for s in S.ORDER_CASES if s[9] and s[4] == 1]


# RelGAT's forward has no partial out to rescale: its second pass knows every group's max
RESCALE = [(s, f) for s in LONG for f in ("no_rescale_out", "no_rescale_l") if not (s[0] == "rel" and f == "no_rescale_out")]


@pytest.mark.parametrize("spec,fault", RESCALE, ids=[f"{S.case_id(s)}-{f}" for s, f in RESCALE])
def test_a_skipped_rescale_breaks_identities_2_and_4(spec, fault):
    case, res = _layouts(spec, lambda c: S.twin(c, fault))
    bad, msg = S.violates(S.check_orders, case, res)
    print(msg)
    assert bad and "identity 4, out, asc against" in msg
    if case.op == "gatv2":      # its summed table is its score's input: with feat_src = 1 every score of a row is one word and no
        return                  # chunk raises the maximum, so identity 2 cannot see a rescale; identity 4 above does
    ones = S.with_table(case, "ones")
    ones = S.reorder(ones, "asc", S.exact(ones).scores)
    S.check_unity(ones, S.exact(ones), S.twin(ones))
    bad, msg = S.violates(S.check_unity, ones, S.exact(ones), S.twin(ones, fault))
    print(msg)
    assert bad


@pytest.mark.parametrize("spec", LONG, ids=[S.case_id(s) for s in LONG])
def test_a_skipped_slot_breaks_identities_2_and_4(spec):
    case, res = _layouts(spec, lambda c: S.twin(c, "skip_lane63"))
    deg64 = np.nonzero((np.diff(case.indptr) == 64) & (S.grid(case)[0][:, 0, 63] >= 0))[0]   # rows of 64 slots whose last is an edge
    assert len(deg64)
    bad, msg = S.violates(S.check_orders, case, res)
    print(msg)
    assert bad and "identity 4, out" in msg
    ones = S.with_table(case, "ones")
    x = S.exact(ones)
    out = S.twin(ones, "skip_lane63")["out"].astype(np.float64)
    want = x.present.sum(1)[:, None, None]
    full = np.abs(out[deg64] - want[deg64]).min()                   # every row of degree 64 has lost a weight
    print(f"rows of degree 64: out is off 1 by at least {full:.3e}")
    assert full > 1e-4
    assert S.violates(S.check_unity, ones, x, dict(out=out))[0]


DISJOINT_IDS = [S.case_id(s) for s in S.DISJOINT_CASES]


@pytest.mark.parametrize("spec", S.DISJOINT_CASES, ids=DISJOINT_IDS)
def test_unnormalised_weights_break_the_row_sums_of_identity_3(hiplib, spec):
    """a_j = exp(e_j - lse) from the fp32 lse, as the four backward kernels took it before they divided by S: at B = +-1000 the table
    gradient of a row's own sources is off g[d]; with lse = m on top (S = l) at every B.  The twin and the float64 fallback hold it."""
    case = S.with_table(S.case_of(spec, disjoint=True), "const")
    x = S.exact(case)
    print(S.check_constant_rows(case, x, S.twin(case)))
    print(S.check_constant_rows(case, x, S.fallback64(case), S.U64))
    S.check_constant_rows(case, x, S.twin(case, "lse_m"))           # a backward that divides by S does not see lse's error
    bad, msg = S.violates(S.check_constant_rows, case, x, S.twin(case, "raw_a"))
    print(msg)
    assert (bad and "table gradient" in msg) or abs(case.B) < 1000
    bad, msg = S.violates(S.check_constant_rows, case, x, S.twin(case, "raw_a+lse_m"))
    print(msg)
    assert bad                                                      # the row sums, or a score gradient grown by the factor l first


HEADS = [s for s in S.CASES if s[0] != "rel" and s[4] > 1 and s[2] > 1]


@pytest.mark.parametrize("spec", HEADS, ids=[S.case_id(s) for s in HEADS])
def test_the_neighbouring_heads_dot_breaks_identity_3(spec):
    case = S.with_table(S.case_of(spec), "const")
    x = S.exact(case)
    S.check_constant_rows(case, x, S.twin(case))
    bad, msg = S.violates(S.check_constant_rows, case, x, S.twin(case, "gout_head"))
    print(msg)
    assert bad


LSE = [s for s in S.CASES if s[0] in ("gat", "gatv2") and s[2] > 1]


@pytest.mark.parametrize("spec", LSE, ids=[S.case_id(s) for s in LSE])
def test_lse_without_log_l_breaks_identity_5(spec):
    """lse against float64, as tests/test_gat_ops_gpu.py and tests/_gatv2_ref.py now hold the kernels' to."""
    import _gatv2_ref
    import test_gat_ops_gpu
    case = S.case_of(spec)
    x = S.exact(case)
    i = case.inp
    if case.op == "gat":
        ref = test_gat_ops_gpu.reference(x.dd, x.pI, case.n_dst, case.P, x.nc, i["el"], i["er"], i["tab"], i["g"], slope=case.slope)
    else:
        ref = _gatv2_ref.reference(x.dd, x.pI, case.n_dst, case.P, x.nc, i["tab"], i["fd"], i["attn"], i["g"], 1, slope=case.slope)
    want, bound = ref["lse"]
    full = ~ref["empty"]
    assert full.any()

    def outside(lse):
        assert np.all(np.isneginf(lse[~full]))
        return int((~(np.abs(lse[full].astype(np.float64) - want[full]) <= bound[full])).sum())

    assert outside(S.twin(case)["lse"]) == 0
    multi = (x.k.reshape(case.n_dst, 1) > 1) & np.ones((1, case.H), bool)      # log l = 0 where the row has one edge
    n_bad = outside(S.twin(case, "lse_m")["lse"])
    print(f"lse = m: {n_bad} of {int(multi.sum())} (row, head) with more than one edge outside")
    assert n_bad > 0.5 * multi.sum() or not multi.any()
