"""Reference-free identities of the four attention block ops (GAT, GATv2, scaled dot-product, relation-typed GAT; coala_block_*_aggregate
[_csr][_backward] in coala_block_ops.hip): the case builders, fp32 twins of the kernels in their summation order, the bounds and the
checkers, shared by tests/test_softmax_identities_cpu.py and tests/test_softmax_identities_gpu.py (tests only).

The float64 comparisons of the operator tests carry u max|z|, u |m| and u |lse| in their bounds, so an error common to a softmax group
passes them.  The identities below hold for any scores, need no reference, and their bounds hold no term that is common to a group:
no max|z|, |m|, |lse| and no offset B.  What they may hold is k (a group's edges), K (a row's), nc (the row's 64-slot chunks), D, P =
ceil(D / 64) + 8 (the levels of a head's dot product: product, 6-step lane scan, one LDS add per 64-float pass), and the spread of the
scores inside a group, x_j = e_j - max e <= 0 and log l = log sum_j exp x_j, which differ from edge to edge.

The regime.  Every score of a group is B plus a unit-spread part, B in {0, +-30, +-1000}:
  GAT, RelGAT  er[d(, r), h] = B + N(0, 1/4), el = N(0, 1).  At |B| >= 30 every z_j of a group has one sign and k_j = (z_j > 0 ? 1 : slope) is
               common to it; B = 0 runs with negative_slope = 1, so k_j = 1.
  dot-product  the last column is reserved: k[:, h, D-1] = 1, q[d, h, D-1] = B / scale (D >= 2).
  GATv2        feat_dst[d, h, c] = +-|B| in every column (so k_jc is common to a column) and attn[h, :] sums to 1 (to 1 / slope for B < 0):
               the common shift is B; B = 0 runs with negative_slope = 1 and a random feat_dst.
Forward and backward form a score with the same code on the same words (the fixed and the CSR instantiation too), so the backward's
e_j is the forward's bit for bit and the bounds carry no rounding of the score itself; that is part of what the identities hold the
kernels to.  The scale a bound multiplies is computed in float64 from the inputs; the kernel's own scores differ from those by u |B|
per edge, which moves a_j by a relative 1e-3 at most and is inside the factor 1.01 below.

Conventions.  u = 2^-24, gamma(n) = n u / (1 - n u); first order in u, every bound multiplied by 1.01 for the second-order terms, plus
2^-100 times the magnitude it scales for weights that underflow; exp and log within 3 ulp (a relative 6u for exp).  a_j is the exact
softmax of the group, dot_j = <g[d, h], f_j>, |dot|_j = sum_c |g_c f_jc|, G = sum_j a_j dot_j (= <g, out> of the group), A = sum_j a_j
|dot|_j >= sum_c |g_c out_c|.  The issue's scale sum_j a_j (|dot_j| + |<g, out>|) is read with these sums of magnitudes: the rounding
of a D-term dot product is gamma(P) |dot|_j whatever the dot product itself cancels to.
  eta   the per-edge relative error of a forward weight exp(e_j - m) against the others of its row: u |x_j| from the subtraction, 6u from
        exp, and per rescale of the online softmax (at most nc - 1) 6u plus the rounding of m_old - m_new, whose sum telescopes to
        max|x|: eta = u (2 max|x| + 6 nc).  The rescale factor itself is one word applied to l and to the partial out alike.
  pu    numerator and denominator of out: the numerator sums its k products in slot order and is rescaled at most nc - 1 times, the
        denominator is a 6-level tree per chunk, nc adds and nc - 1 rescales, then 1 / l and the product:
        pu = gamma(k + nc) + gamma(6 + 2 nc) + 2u.  |out - sum_j a_j f_j| <= (2 eta + pu) sum_j a_j |f_j|.
  RelGAT's forward takes two passes: l from the online pass, a_j = exp(e_j - m) (1 / l) from the second, out one slot-order sum over the
        row's K edges of every relation: |out - ref| <= sum_j c_j a_j |f_j|, c_j = u (2 max|x| + 7 nc + 10) + gamma(6 + nc) + gamma(K + 1),
        the bound of tests/test_rel_gat_ops_gpu.py without its score terms.

1  score gradients of a group sum to zero.  The backward takes p~_j = exp(e_j - lse~) (1 + eps_j), eps_j <= u (7 + |x_j - log l|) (exp,
   the subtraction, and the division that follows); the p~_j sum to S = 1 + delta with delta ~ u |lse|, which is common, and the kernels
   divide by their own sum S~ (a wave sum per chunk, chunk after chunk): a~_j = p~_j / S~.  GAT, GATv2, dot-product: sum_j a~_j (dot~_j -
   <g, out~>~) = (S / S~) (<g, out*> - <g, out~>) + roundings, out* the exact softmax sum, so the common factor only multiplies a small number:
     |sum_j t_j| <= (2 eta + pu + 2 gamma(P)) A + sum_j a_j |dot_j - G| (eps_j + r),
   r the roundings of t_j and of the sum that follows: GAT 3u + gamma(6 + nc) (a tree per chunk, an add per chunk), times the common
   k_j, for grad_er[d, h]; dot-product 2u + gamma(k + 2 nc) (slot order, scale and add per chunk), times |scale|, for grad_q[d, h,
   D-1]; GATv2 4u + gamma(k + nc), times |attn_c| k_c, for grad_dst[d, h, c].  RelGAT subtracts G~ / S~ formed from the same a~_j and
   dot~_j, so neither eps_j nor the forward enters: |grad_er[d, r, h]| <= k ((gamma(7 + nc) + gamma(6 + nc) + u) A + (4u + gamma(6 + nc))
   sum_j a_j |dot_j - G|) (the 4u: the division of p~_j by S~, the subtraction and the two products of t_j).  With G in place of G / S the sum is (1 - S) G: that is offset-dependent and the bound rejects it.
   sum_p grad_el[p, h] over the block (float64 on the host) is the sum of the groups' sums: the sum of the bounds above plus
   gamma(K_p) |t_j| per edge for the atomics of table row p (K_p contributions, any order).
2  partition of unity.  With the summed table = 1 numerator and denominator add the same weights: |out - 1| <= pu where the row has an
   edge (RelGAT: |out - #relations present| <= sum over them of c_j), exactly 0 where it has none.
3  constant rows.  With every summed row = phi[h, :] all dot~_j are one word and out~_c = phi_c (1 + theta), |theta| <= pu, so
   |dot~ - <g, out~>~| <= tau = (2 gamma(P) + pu + u) sum_c |g_c phi_c| (RelGAT: G~ / S~ = dot~ (1 + theta'), tau = (gamma(7 + nc) +
   gamma(6 + nc) + u) sum_c |g_c phi_c|) and |t_j| <= a_j tau k_j.  Every gradient that passes through t_j alone is bounded by its
   terms' magnitudes: grad_er <= k tau, grad_el[p] <= sum_j k_j a_j tau; grad_q[d, h, c] <= |scale| tau sum_j a_j |k_jc|, grad_k[p, h,
   c] <= |scale| sum_j a_j tau |q_c|; grad_dst[d, h, c] <= |attn_c| tau sum_j a_j k_jc, grad_attn[h, c] <= sum_d tau sum_j a_j
   |lrelu(z_jc)| (its terms are t_j lrelu(z_jc): the input's magnitude multiplies the bound as |attn_c| and |scale| do).
   The total of grad_feat / grad_v / grad_src over the table rows is sum_d g[d] sum_j a~_j.  The weights are divided by their own sum, a
   6-level tree per chunk and an add per chunk, then one division each: |sum_j a~_j - 1| <= gamma(6 + nc) + 2u (the fallbacks, whose l
   is a plain sum: pu + u); a contribution a~_j g_c is one more product and table row p adds its K_p contributions in any order:
     |sum_p grad_table[p, h, c] - sum_d g[d, h, c]| <= sum_d (gamma(6 + nc) + 2u) |g_c| + sum_j (gamma(K_p) + u) a_j |g_c|
   over the rows with an edge (RelGAT: once per relation present; GATv2's grad_src also carries t_j attn_c k_jc, bounded as above).
   The block's total averages the rows' errors, so the cases of DISJOINT_CASES give every slot a table row of its own (K_p = 1) and
   hold the sum over each row's own sources to g[d]: |sum_j grad_table[p_j, h, c] - g[d, h, c]| <= (gamma(6 + nc) + 3u) |g_c|.
   Weights left as exp(e_j - lse) from the fp32 lse sum to 1 + O(u |lse|) and break this at B = +-1000 (fault 'raw_a': the kernels
   before `normalised`; their twins put the block's total off by 25u to 60u sum|g| there); with lse = m they break it at every B.
4  the order of a row does not matter.  A score does not depend on its slot, so every layout of a row's edges has the same out*:
   |out_A - out_B| <= 2 (2 eta + pu) sum_j a_j |f_j| (RelGAT: 2 sum_j c_j a_j |f_j|), and grad_er / grad_q[.., D-1] / grad_dst agree within twice
   the bound of 1.  Layouts: ascending by the score of head 0 (every chunk raises the running maximum: the rescale runs in every chunk),
   descending (it never runs), shuffled; RelGAT also shuffled then sorted by type.
The float64 torch fallbacks are held to the same formulas with u = 2^-53 and D + 2 in place of P (their dot products are plain sums)."""
import types

import numpy as np

from _dot_gat_ref import _butterfly, _segment_sums

U32 = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -100
SLOPE = np.float32(0.2)
OFFSETS = (0.0, 30.0, -30.0, 1000.0, -1000.0)
DEGS = (0, 1, 63, 64, 65, 128, 129, 200)
OPS = ("gat", "gatv2", "dot", "rel")
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- cases

def _graph(rng, op, form, n_dst, f, P, R, long_row):
    """fixed: idx [n_dst, f] with -1 interspersed and some rows all -1.  csr: degrees DEGS in turn (row 1: long_row edges, if any); the
    index arrays of dot / rel hold -1, and a row of 200 slots has its second chunk all -1."""
    holes = op in ("dot", "rel")
    if form == "fixed":
        idx = rng.integers(0, P, size=(n_dst, f)).astype(np.int32)
        idx[rng.random((n_dst, f)) < 0.25] = -1
        if n_dst > 1:
            idx[rng.random(n_dst) < 0.05] = -1
            idx[1] = -1
        if n_dst > 2:
            idx[2] = rng.integers(0, P, size=f)                     # a full row
        indptr = None
    else:
        deg = np.array([DEGS[i % len(DEGS)] for i in range(n_dst)] if n_dst != 1 else [65], dtype=np.int64)
        if long_row and n_dst > 1:
            deg[1] = long_row
        indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        idx = rng.integers(0, P, size=int(indptr[-1])).astype(np.int32)
        if holes:
            idx[rng.random(idx.shape) < 0.05] = -1
            for d in np.nonzero(deg == 200)[0][:2]:
                idx[indptr[d] + 64: indptr[d] + 128] = -1
    typ = None
    if op == "rel":
        typ = rng.integers(0, R, size=idx.shape).astype(np.int32)
        wild = rng.random(idx.shape) < 0.04
        typ[wild] = rng.choice(np.array([-1, R, 1000], dtype=np.int32), size=int(wild.sum()))
    return idx, typ, indptr


def make_case(op, form, n_dst, f, H, D, R, off, B, seed, long_row=0, table="rand", same_order_heads=False, disjoint=False):
    """One case: the graph, the fp32 inputs with the common offset B, the slope / scale.  table: 'rand', 'ones' (identity 2) or 'const'
    (identity 3) for the summed table.  same_order_heads: GAT / RelGAT el differs between heads by a constant, so one layout ascends in
    every head.  disjoint: every slot reads a table row of its own, so a row's part of the table gradient can be told from the others'."""
    rng = np.random.default_rng(seed)
    P = 97
    R = R if op == "rel" else 1
    idx, typ, indptr = _graph(rng, op, form, n_dst, f, P - 7, R, long_row)       # the last 7 table rows are never referenced
    if disjoint:
        idx[idx >= 0] = np.arange(int((idx >= 0).sum()), dtype=np.int32)
        P = int((idx >= 0).sum()) + 7
    c = types.SimpleNamespace(op=op, form=form, n_dst=n_dst, f=f, P=P, H=H, D=D, R=R, off=off, B=float(B), idx=idx, typ=typ, indptr=indptr,
                              slope=f32(1.0) if B == 0 else SLOPE, scale=f32(0.75 / np.sqrt(D)), table=table, seed=seed,
                              long_row=long_row, same_order_heads=same_order_heads, disjoint=disjoint)
    g = rng.standard_normal((n_dst, H, D)).astype(f32)
    tab = rng.standard_normal((P, H, D)).astype(f32)
    phi = rng.standard_normal((1, H, D)).astype(f32)
    if table == "ones":
        tab = np.ones_like(tab)
    elif table == "const":
        tab = np.broadcast_to(phi, tab.shape).copy()
    if op in ("gat", "rel"):
        el = rng.standard_normal((P, H)).astype(f32)
        if same_order_heads:
            el = (el[:, :1] + 0.25 * rng.standard_normal((1, H))).astype(f32)
        er = (0.5 * rng.standard_normal((n_dst, R, H)) + B).astype(f32)
        c.inp = dict(el=el, er=er if op == "rel" else er[:, 0], tab=tab, g=g)
    elif op == "dot":
        q = rng.standard_normal((n_dst, H, D)).astype(f32)
        k = rng.standard_normal((P, H, D)).astype(f32)
        k[:, :, D - 1] = 1.0
        q[:, :, D - 1] = f32(B) / c.scale
        c.inp = dict(q=q, k=k, tab=tab, g=g)
    else:
        attn = (rng.standard_normal((H, D)) / np.sqrt(D)).astype(f32)
        if B == 0:
            fd = (0.5 * rng.standard_normal((n_dst, H, D))).astype(f32)
        else:
            attn = (attn + ((1.0 if B > 0 else 1.0 / float(SLOPE)) - attn.sum(-1, keepdims=True)) / D).astype(f32)
            fd = np.full((n_dst, H, D), B, dtype=f32)
        c.inp = dict(fd=fd, attn=attn, tab=tab, g=g)
    return c


def with_table(case, table):
    return make_case(case.op, case.form, case.n_dst, case.f, case.H, case.D, case.R, case.off, case.B, case.seed, case.long_row, table,
                     case.same_order_heads, case.disjoint)


# (form, n_dst, fan-out, H, D, R, float offset, B, long row): every fan-out, H, D, R, offset and B of the issue appears for every op
_SHAPES = [("fixed", 300, 5, 4, 16, 3, 0, 1000.0, 0), ("fixed", 64, 32, 16, 3, 3, 1, -30.0, 0), ("fixed", 65, 1, 1, 65, 1, 0, 0.0, 0),
           ("fixed", 64, 2, 4, 2, 64, 1, -1000.0, 0), ("fixed", 90, 32, 4, 65, 64, 1, 30.0, 0), ("csr", 64, 0, 4, 16, 64, 0, 30.0, 0),
           ("csr", 72, 0, 1, 3, 1, 1, 1000.0, 0), ("csr", 64, 0, 16, 2, 3, 0, -1000.0, 0), ("csr", 64, 0, 4, 2, 3, 1, 0.0, 4097),
           ("fixed", 1, 5, 1, 2, 1, 0, 0.0, 0), ("csr", 1, 0, 4, 3, 3, 1, -30.0, 0), ("fixed", 0, 5, 4, 16, 3, 0, 1000.0, 0),
           ("csr", 0, 0, 1, 2, 1, 0, 30.0, 0)]
CASES = [(op,) + s for op in OPS for s in _SHAPES]
# the order cases of identity 4: rows of 0..200 edges and one of 4,097; fixed rows of 32 slots
_ORDER = [("csr", 64, 0, 1, 16, 3, 0, 1000.0, 4097), ("csr", 64, 0, 4, 3, 3, 1, -30.0, 4097), ("fixed", 64, 32, 4, 2, 3, 0, 0.0, 0)]
ORDER_CASES = [(op,) + s for op in OPS for s in _ORDER]
ORDERS = ("asc", "desc", "shuf")
# the cases whose slots read table rows of their own (identity 3, the table gradient row by row)
_DISJOINT = [("fixed", 90, 5, 4, 3, 3, 0, 1000.0, 0), ("csr", 24, 0, 4, 16, 3, 1, -1000.0, 0), ("fixed", 64, 32, 1, 2, 1, 1, 30.0, 0)]
DISJOINT_CASES = [(op,) + s for op in OPS for s in _DISJOINT]


def case_of(spec, table="rand", same_order_heads=False, disjoint=False):
    op, form, n_dst, f, H, D, R, off, B, long_row = spec
    seed = OPS.index(op) * 1000 + n_dst * 7 + f * 131 + H * 17 + D + R * 3 + off + int(abs(B)) + (B < 0)
    return make_case(op, form, n_dst, f, H, D, R, off, B, seed, long_row, table, same_order_heads, disjoint)


def case_id(spec):
    op, form, n_dst, f, H, D, R, off, B, long_row = spec
    return f"{op}-{form}-n{n_dst}-f{f}-H{H}-D{D}-R{R}-o{off}-B{B:g}" + ("-long" if long_row else "")


def grid(case):
    """-> idx [n_dst, NC, 64] (int64, -1: no edge), typ (0 for the untyped ops, -1: no edge), chunks per row: the slots as the kernels'
    64-slot chunks see them.  A slot of RelGAT whose type is outside [0, R) is no edge."""
    n = case.n_dst
    if case.form == "fixed":
        nc = np.ones(n, dtype=np.int64)
        idx = np.full((n, 1, 64), -1, dtype=np.int64)
        typ = np.zeros((n, 1, 64), dtype=np.int64)
        idx[:, 0, : case.f] = case.idx
        if case.typ is not None:
            typ[:, 0, : case.f] = case.typ
    else:
        deg = np.diff(case.indptr)
        nc = -(-deg // 64)
        NC = max(int(nc.max()) if n else 1, 1)
        idx = np.full((n, NC * 64), -1, dtype=np.int64)
        typ = np.zeros((n, NC * 64), dtype=np.int64)
        d = np.repeat(np.arange(n), deg)
        pos = np.arange(int(case.indptr[-1])) - np.repeat(case.indptr[:-1], deg)
        idx[d, pos] = case.idx
        if case.typ is not None:
            typ[d, pos] = case.typ
        idx, typ = idx.reshape(n, NC, 64), typ.reshape(n, NC, 64)
    bad = (idx < 0) | (typ < 0) | (typ >= case.R)
    return np.where(bad, -1, idx), np.where(bad, -1, typ), np.maximum(nc, 1)


def reorder(case, order, scores):
    """The case with the valid slots of every row laid out anew: 'asc' / 'desc' by scores (float64 [n_dst, NC, 64], of head 0), 'shuf',
    or 'bytype' (shuffled, then stable by type).  The -1 slots stay where they are."""
    idx, typ, _ = grid(case)
    n, NC, _ = idx.shape
    rng = np.random.default_rng(case.seed + 17)
    new_i, new_t = idx.reshape(n, -1).copy(), typ.reshape(n, -1).copy()
    sc = scores.reshape(n, -1)
    for d in range(n):
        pos = np.nonzero(new_i[d] >= 0)[0]
        if order in ("asc", "desc"):
            perm = pos[np.argsort(sc[d, pos], kind="stable")]
            if order == "desc":
                perm = perm[::-1]
        else:
            perm = rng.permutation(pos)
            if order == "bytype":
                perm = perm[np.argsort(new_t[d, perm], kind="stable")]
        new_i[d, pos], new_t[d, pos] = new_i[d, perm], new_t[d, perm]
    out = types.SimpleNamespace(**vars(case))
    if case.form == "fixed":
        keep = new_i[:, : case.f] >= 0                              # a slot that was no edge keeps its raw words
        out.idx = np.where(keep, new_i[:, : case.f], case.idx).astype(np.int32)
        if case.typ is not None:
            out.typ = np.where(keep, new_t[:, : case.f], case.typ).astype(np.int32)
    else:
        deg = np.diff(case.indptr)
        d = np.repeat(np.arange(n), deg)
        pos = np.arange(int(case.indptr[-1])) - np.repeat(case.indptr[:-1], deg)
        keep = new_i[d, pos] >= 0
        out.idx = np.where(keep, new_i[d, pos], case.idx).astype(np.int32)
        if case.typ is not None:
            out.typ = np.where(keep, new_t[d, pos], case.typ).astype(np.int32)
    return out


# ---------------------------------------------------------------------------------------------------------------- float64 side

def _edge_terms(case, dd, pI, tt, dt):
    """The scores of the edges (dd, pI, tt) in dtype dt, in the kernels' order where dt is fp32 -> e [E, H], k_j [E, H] (GAT, RelGAT: the
    leaky_relu factor of the score), z [E, H, D] and lrelu(z) (GATv2 only)."""
    i = case.inp
    H, D, hd = case.H, case.D, case.H * case.D
    slope = dt(case.slope)
    z3 = lz3 = None
    if case.op in ("gat", "rel"):
        er = i["er"].reshape(case.n_dst * case.R, H).astype(dt)
        z = i["el"].astype(dt)[pI] + er[dd * case.R + tt]
        e = np.where(z > 0, z, z * slope)
        kf = np.where(z > 0, dt(1), slope)
    elif case.op == "dot":
        prod = i["q"].astype(dt)[dd] * i["k"].astype(dt)[pI]
        e = dt(case.scale) * (_segment_sums(prod.reshape(-1, hd), D) if dt is f32 else prod.sum(-1))
        kf = np.ones_like(e)
    else:
        z3 = i["tab"].astype(dt)[pI] + i["fd"].astype(dt)[dd]
        lz3 = np.where(z3 > 0, z3, z3 * slope)
        term = i["attn"].astype(dt)[None] * lz3
        e = _segment_sums(term.reshape(-1, hd), D) if dt is f32 else term.sum(-1)
        kf = np.ones_like(e)
    return e.astype(dt), kf.astype(dt), z3, lz3


def exact(case):
    """float64 from the inputs: the valid edges in slot order and, per edge / group / row, what the bounds scale."""
    idx, typ, nc = grid(case)
    n, H, D, R = case.n_dst, case.H, case.D, case.R
    dI = np.broadcast_to(np.arange(n)[:, None, None], idx.shape)
    sel = idx >= 0
    dd, pI, tt = dI[sel], idx[sel], typ[sel]
    key = dd * R + tt
    x = types.SimpleNamespace(dd=dd, pI=pI, tt=tt, key=key, nc=nc, sel=sel)
    e, kf, z3, lz3 = _edge_terms(case, dd, pI, tt, np.float64)
    m = np.full((n * R, H), -np.inf)
    np.maximum.at(m, key, e)
    xx = e - m[key]
    l = np.zeros((n * R, H))
    np.add.at(l, key, np.exp(xx))
    a = np.exp(xx) / l[key] if len(key) else xx
    x.e, x.kf, x.a, x.x, x.logl, x.z3, x.lz3 = e, kf, a, xx, (np.log(l[key]) if len(key) else xx), z3, lz3
    x.scores = np.full(idx.shape, -np.inf)
    x.scores[sel] = e[:, 0] if len(key) else 0.0
    x.k = np.bincount(key, minlength=n * R).astype(np.float64)[:, None]            # a group's edges
    x.K = np.bincount(dd, minlength=n).astype(np.float64)                         # a row's
    x.ncg = np.repeat(nc, R).astype(np.float64)[:, None]
    x.maxx = np.zeros((n * R, H))
    np.maximum.at(x.maxx, key, np.abs(xx))
    g, tab = case.inp["g"].astype(np.float64), case.inp["tab"].astype(np.float64)
    gf = g[dd] * tab[pI]                                                           # [E, H, D]
    x.dot, x.adot = gf.sum(-1), np.abs(gf).sum(-1)
    grp = lambda v: _scatter(np.zeros((n * R,) + v.shape[1:]), key, v)   # noqa: E731
    x.G = grp(a * x.dot)
    x.A = grp(a * x.adot)
    x.absf = _scatter(np.zeros((n, H, D)), dd, a[..., None] * np.abs(tab[pI]))     # sum_j a_j |f_j| of the row
    x.sumf = _scatter(np.zeros((n, H, D)), dd, np.abs(tab[pI]))
    x.kfg = np.ones((n * R, H))
    if len(key):
        kmax = np.zeros((n * R, H))
        np.maximum.at(kmax, key, kf)
        x.kfg = np.where(x.k > 0, kmax, 1.0)
    x.present = (x.k[:, 0] > 0).reshape(n, R)
    return x


def _scatter(acc, index, v):
    np.add.at(acc, index, v)
    return acc


def _gam(n, u):
    n = np.asarray(n, dtype=np.float64)
    return n * u / (1.0 - n * u)


def _levels(case, u):
    return (-(-case.D // 64) + 8) if u == U32 else case.D + 2


def _fwd_consts(case, x, u):
    """(eta, pu) per group [n * R, H] (a group of the untyped ops is its row), and RelGAT's c_j per group."""
    eta = u * (2 * x.maxx + 6 * x.ncg)
    pu = _gam(x.k + x.ncg, u) + _gam(6 + 2 * x.ncg, u) + 2 * u
    c_rel = u * (2 * x.maxx + 7 * x.ncg + 10) + _gam(6 + x.ncg, u) + _gam(np.repeat(x.K, case.R)[:, None] + 1, u)
    return eta, pu, c_rel


def bound_group_sum(case, x, u=U32):
    """Identity 1: the bound of sum_j t_j of every group [n * R, H], before the op's own factor (k_j, scale, attn_c k_c)."""
    eta, pu, _ = _fwd_consts(case, x, u)
    P = _levels(case, u)
    dev = x.a * np.abs(x.dot - x.G[x.key])                                         # a_j |dot_j - G|
    n = case.n_dst * case.R
    if case.op == "rel":
        T = _scatter(np.zeros((n, case.H)), x.key, dev)
        return 1.01 * ((_gam(7 + x.ncg, u) + _gam(6 + x.ncg, u) + u) * x.A + (4 * u + _gam(6 + x.ncg, u)) * T) + TINY
    r = {"gat": 3 * u + _gam(6 + x.ncg, u), "dot": 2 * u + _gam(x.k + 2 * x.ncg, u), "gatv2": 4 * u + _gam(x.k + x.ncg, u)}[case.op]
    W = _scatter(np.zeros((n, case.H)), x.key, dev * (u * (7 + np.abs(x.x - x.logl)) + r[x.key]))
    return 1.01 * ((2 * eta + pu + 2 * _gam(P, u)) * x.A + W) + TINY


def _col_factor(case, x):
    """GATv2: |attn_c| k_c per (row, head, column), k_c the column's common leaky_relu factor (the largest of the row's, were they to
    differ)."""
    kfc = np.where(x.z3 > 0, 1.0, float(case.slope))
    top = np.zeros((case.n_dst, case.H, case.D))
    if len(x.dd):
        np.maximum.at(top, x.dd, kfc)
    return np.abs(case.inp["attn"].astype(np.float64))[None] * top


def check_sum_to_zero(case, x, res, u=U32):
    """Identity 1 -> {name: largest |value| / bound}; raises past a bound."""
    b = bound_group_sum(case, x, u)
    n, H, R = case.n_dst, case.H, case.R
    ratios = {}
    if case.op in ("gat", "rel"):
        bg = b * x.kfg
        shape = (n, R, H) if case.op == "rel" else (n, H)
        ratios["grad_er"] = _hold("identity 1, grad_er", res["ger"], 0.0, bg.reshape(shape))
        Kp = np.bincount(x.pI, minlength=case.P).astype(np.float64)
        t_abs = x.kf * x.a * np.abs(x.dot - x.G[x.key])
        total = res["gel"].astype(np.float64).sum(0)
        b_tot = bg.sum(0) + 1.01 * (_gam(Kp, u)[x.pI][:, None] * t_abs).sum(0) + TINY
        ratios["sum grad_el"] = _hold("identity 1, the block's sum of grad_el", total, 0.0, b_tot)
    elif case.op == "dot":
        ratios["grad_q"] = _hold("identity 1, grad_q[.., D-1]", res["gq"][:, :, case.D - 1], 0.0, abs(float(case.scale)) * b)
    else:
        ratios["grad_dst"] = _hold("identity 1, grad_dst", res["gd"], 0.0, _col_factor(case, x) * b[:, :, None])
    return ratios


def check_unity(case, x, res, u=U32):
    """Identity 2 (the case's summed table is 1)."""
    eta, pu, c_rel = _fwd_consts(case, x, u)
    n, H, R = case.n_dst, case.H, case.R
    present = x.present.sum(1).astype(np.float64)
    want = np.broadcast_to(present[:, None, None], (n, H, case.D))
    if case.op == "rel":
        b = 1.01 * np.where(x.k > 0, c_rel, 0.0).reshape(n, R, H).sum(1) + TINY
    else:
        b = 1.01 * np.where(x.k > 0, pu, 0.0) + TINY
    got = np.asarray(res["out"])
    assert np.all(got[present == 0] == 0.0), "identity 2: a row without an edge is not exactly 0"
    return {"out": _hold("identity 2, out", got, want, np.broadcast_to(b[:, :, None], want.shape))}


def check_constant_rows(case, x, res, u=U32, totals=True):
    """Identity 3 (every summed row of the case is phi[h, :]).  totals: also the total of the summed table's gradient."""
    eta, pu, _ = _fwd_consts(case, x, u)
    n, H, D, R = case.n_dst, case.H, case.D, case.R
    P = _levels(case, u)
    g, phi = case.inp["g"].astype(np.float64), case.inp["tab"][0].astype(np.float64)
    sgp = np.repeat(np.abs(g * phi[None]).sum(-1), R, axis=0)                      # [n * R, H], sum_c |g_c phi_c|
    if case.op == "rel":
        tau = (_gam(7 + x.ncg, u) + _gam(6 + x.ncg, u) + u) * sgp
    else:
        tau = (2 * _gam(P, u) + pu + u) * sgp
    tau = 1.01 * tau + TINY
    te = x.kf * x.a * tau[x.key]                                                   # the bound of |t_j|, [E, H]
    ratios = {}
    if case.op in ("gat", "rel"):
        shape = (n, R, H) if case.op == "rel" else (n, H)
        ratios["grad_er"] = _hold("identity 3, grad_er", res["ger"], 0.0, (np.where(x.k > 0, x.kfg * tau, 0.0)).reshape(shape) * 1.01)
        ratios["grad_el"] = _hold("identity 3, grad_el", res["gel"], 0.0, 1.01 * _scatter(np.zeros((case.P, H)), x.pI, te) + TINY)
    elif case.op == "dot":
        s = abs(float(case.scale))
        kE, qE = np.abs(case.inp["k"].astype(np.float64))[x.pI], np.abs(case.inp["q"].astype(np.float64))[x.dd]
        ratios["grad_q"] = _hold("identity 3, grad_q", res["gq"], 0.0, 1.01 * s * _scatter(np.zeros((n, H, D)), x.dd, te[..., None] * kE) + TINY)
        ratios["grad_k"] = _hold("identity 3, grad_k", res["gk"], 0.0, 1.01 * s * _scatter(np.zeros((case.P, H, D)), x.pI, te[..., None] * qE) + TINY)
    else:
        at = np.abs(case.inp["attn"].astype(np.float64))[None]
        kfc = np.where(x.z3 > 0, 1.0, float(case.slope))
        ratios["grad_dst"] = _hold("identity 3, grad_dst", res["gd"], 0.0, 1.01 * _scatter(np.zeros((n, H, D)), x.dd, te[..., None] * at * kfc) + TINY)
        b_ga = 1.01 * (te[..., None] * np.abs(x.lz3)).sum(0) * (1 + _gam(len(x.dd) + 8, u)) + TINY
        ratios["grad_attn"] = _hold("identity 3, grad_attn", res["ga"], 0.0, b_ga)
    if totals:
        # sum_p grad_table[p, h, c] = sum_d g[d, h, c] sum_j a_j: with weights that are normalised (sum_j a_j = 1 within pu) the table's
        # gradient adds up to g over the rows with an edge, once per relation present; gamma(K_p) for the sum into table row p
        gE = np.abs(g)[x.dd]
        want = (g * x.present.sum(1)[:, None, None]).sum(0)
        norm = _gam(6 + x.ncg, u) + 2 * u if u == U32 else pu + u   # the kernels' S: a tree per chunk, an add per chunk, one division
        b = (np.broadcast_to(np.where(x.k > 0, norm, 0.0), (n * R, H)).reshape(n, R, H).sum(1)[:, :, None] * np.abs(g)).sum(0)
        Kp = np.bincount(x.pI, minlength=case.P).astype(np.float64)
        b = 1.01 * (b + ((_gam(Kp, u)[x.pI] + u)[:, None, None] * x.a[..., None] * gE).sum(0)) + TINY
        via_t = 0.0
        if case.op == "gatv2":                                     # grad_src also carries t_j attn_c k_jc
            via_t = 1.01 * (te[..., None] * np.abs(case.inp["attn"].astype(np.float64))[None] * np.where(x.z3 > 0, 1.0, float(case.slope))).sum(0)
        ratios["sum grad_table"] = _hold("identity 3, the table gradient's total", np.asarray(res["gt"], np.float64).sum(0), want, b + via_t)
        if case.disjoint:                                          # K_p = 1: the sum over a row's own table rows is g[d] sum_j a_j
            rows = _scatter(np.zeros((n, H, D)), x.dd, np.asarray(res["gt"], np.float64)[x.pI])
            b = np.broadcast_to(np.where(x.k > 0, norm + u, 0.0), (n * R, H)).reshape(n, R, H).sum(1)[:, :, None] * np.abs(g)
            if case.op == "gatv2":
                kfc = np.where(x.z3 > 0, 1.0, float(case.slope))
                b = b + _scatter(np.zeros((n, H, D)), x.dd, te[..., None] * np.abs(case.inp["attn"].astype(np.float64))[None] * kfc)
            ratios["row sums of grad_table"] = _hold("identity 3, the table gradient's sum over a row's sources", rows,
                                                     g * x.present.sum(1)[:, None, None], 1.01 * b + TINY)
    return ratios


def bound_out(case, x, u=U32):
    """|out - sum_j a_j f_j| per element, free of score terms (identity 4 holds two layouts to twice this)."""
    eta, pu, c_rel = _fwd_consts(case, x, u)
    if case.op == "rel":
        tab = np.abs(case.inp["tab"].astype(np.float64))[x.pI]
        b = _scatter(np.zeros((case.n_dst, case.H, case.D)), x.dd, (c_rel[x.key] * x.a)[..., None] * tab)
    else:
        b = (2 * eta + pu)[:, :, None] * x.absf
    return 1.01 * b + TINY * x.sumf


def check_orders(case, results, u=U32):
    """Identity 4: results {layout name: (case in that layout, its result)} agree pairwise -> ratios.  The bounds are those of the first
    layout (k, nc, the spread and the scales are the same in every layout)."""
    names = list(results)
    c0 = results[names[0]][0]
    x = exact(c0)
    b_out = 2 * bound_out(c0, x, u)
    b1 = 2 * bound_group_sum(c0, x, u)
    key = {"gat": "ger", "rel": "ger", "dot": "gq", "gatv2": "gd"}[case.op]
    if case.op in ("gat", "rel"):
        b1 = (b1 * x.kfg).reshape(np.asarray(results[names[0]][1][key]).shape)
    elif case.op == "dot":
        b1 = abs(float(case.scale)) * b1
    else:
        b1 = _col_factor(c0, x) * b1[:, :, None]
    ratios = {"out": 0.0, key: 0.0}
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            ra, rb = results[a][1], results[b][1]
            ratios["out"] = max(ratios["out"], _hold(f"identity 4, out, {a} against {b}", ra["out"], np.asarray(rb["out"], np.float64), b_out))
            ga, gb = np.asarray(ra[key]), np.asarray(rb[key], np.float64)
            if case.op == "dot":
                ga, gb = ga[:, :, case.D - 1], gb[:, :, case.D - 1]
            ratios[key] = max(ratios[key], _hold(f"identity 4, {key}, {a} against {b}", ga, gb, b1))
    return ratios


def _hold(name, got, want, bound):
    """Every element of got within bound of want -> the largest error / bound."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    bound = np.broadcast_to(bound, err.shape)
    if not err.size:
        return 0.0
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.size} elements past the bound; at {i}: got {got[i]!r} want "
                             f"{np.broadcast_to(want, err.shape)[i]!r} bound {bound[i]!r} (error / bound {np.nanmax(err / np.maximum(bound, 1e-300)):.2f})")
    return float(np.max(err / np.maximum(bound, 1e-300)))


def violates(fn, *a, **kw):
    """Whether a checker raises -> (bool, its message)."""
    try:
        fn(*a, **kw)
    except AssertionError as e:
        return True, str(e)
    return False, ""


# ---------------------------------------------------------------------------------------------------------------- fp32 twins

FAULTS = ("rel_G", "no_rescale_out", "no_rescale_l", "gout_head", "lse_m", "skip_lane63", "dot_fma", "raw_a")


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def twin(case, fault=None):
    """The kernels of case.op restated in numpy fp32, in their summation orders (64-slot chunks, butterfly wave sums, the online softmax,
    slot-order accumulation, head_segment_add's dot products; the atomics in np.add.at's order) -> dict of out, lse and the gradients.
    fault: one of FAULTS, a kernel that is wrong in that way:
      rel_G           RelGAT's t_j with G in place of G / S (the kernel before its fix);
      no_rescale_out  the second chunk does not rescale the partial out;  no_rescale_l: ... nor l;
      gout_head       <g, out> taken from the neighbouring head;
      lse_m           lse stored as m alone, log l dropped;
      skip_lane63     the weighted sum skips lane 63 of every chunk;
      dot_fma         the dot-product backward's score fused into its subtraction, fma(scale, qk, -lse): the product unrounded where the
                      forward rounded it (the kernel before dot_score);
      raw_a           the backward's weights a_j = exp(e_j - lse) as they come from the fp32 lse, not divided by their group's sum S (the
                      kernels before `normalised`; rel_G implies it).
    Faults combine with '+'."""
    faults = set(fault.split("+")) if fault else set()
    assert faults <= set(FAULTS) and ("dot_fma" not in faults or case.op == "dot")
    idx, typ, _ = grid(case)
    n, H, D, R, P, hd = case.n_dst, case.H, case.D, case.R, case.P, case.H * case.D
    NC = idx.shape[1]
    valid = idx >= 0
    ic, tc = np.where(valid, idx, 0), np.where(valid, typ, 0)
    dI = np.broadcast_to(np.arange(n)[:, None, None], idx.shape)
    dd, pI, tt = dI[valid], ic[valid], tc[valid]
    inp = case.inp
    tab, g = inp["tab"], inp["g"]
    slope, scale = f32(case.slope), f32(case.scale)
    ee, kk, z3, lz3 = _edge_terms(case, dd, pI, tt, f32)
    e = np.full(idx.shape + (H,), -np.inf, dtype=f32)
    kf = np.ones(idx.shape + (H,), dtype=f32)
    gdot = np.zeros(idx.shape + (H,), dtype=f32)
    e[valid], kf[valid] = ee, kk
    gdot[valid] = _segment_sums((g[dd] * tab[pI]).reshape(-1, hd), D)
    rel = case.op == "rel"
    lanes = lambda v: np.moveaxis(v, 1, -1)   # noqa: E731  ([n, 64, ...] -> [n, ..., 64])
    one, zero = f32(1), f32(0)
    err = lambda: np.errstate(invalid="ignore", over="ignore", divide="ignore")   # noqa: E731

    def step(m, l, ev, mask):
        """One chunk of the online softmax: -> (m_new, l_new, p, the rescale factor)."""
        with err():
            mn = np.maximum(m, _butterfly(lanes(ev), np.maximum))
            p = np.where(mask, np.exp(ev - mn[:, None], dtype=f32), zero).astype(f32)
            sc = np.where(m == mn, one, np.where(np.isneginf(m), zero, np.exp(m - mn, dtype=f32))).astype(f32)
        return mn, sc, p, _butterfly(lanes(p), np.add)

    out = np.zeros((n, H, D), dtype=f32)
    if not rel:
        m = np.full((n, H), -np.inf, dtype=f32)
        l = np.zeros((n, H), dtype=f32)
        for c in range(NC):
            vv = valid[:, c]
            mn, sc, p, sm = step(m, l, e[:, c], vv[..., None])
            l = ((l if "no_rescale_l" in faults and c == 1 else (l * sc).astype(f32)) + sm).astype(f32)
            if not ("no_rescale_out" in faults and c == 1):
                out = (out * sc[..., None]).astype(f32)
            for j in range(64):
                if vv[:, j].any() and not ("skip_lane63" in faults and j == 63):
                    out = np.where(vv[:, j, None, None], out + (p[:, j, :, None] * tab[ic[:, c, j]]).astype(f32), out).astype(f32)
            m = mn
        with err():
            out = (out * np.where(l > 0, one / np.where(l > 0, l, one), zero).astype(f32)[..., None]).astype(f32)
            lse = np.where(l > 0, m + (zero if "lse_m" in faults else np.log(np.where(l > 0, l, one), dtype=f32)), f32(-np.inf)).astype(f32)
    else:
        oh = (tc[..., None] == np.arange(R)) & valid[..., None]                    # [n, NC, 64, R]
        m = np.full((n, R, H), -np.inf, dtype=f32)
        l = np.zeros((n, R, H), dtype=f32)
        for c in range(NC):
            mask = oh[:, c][..., None]                                             # [n, 64, R, 1]
            ev = np.where(mask, e[:, c][:, :, None, :], f32(-np.inf)).astype(f32)
            mn, sc, p, sm = step(m, l, ev, mask)
            l = ((l if "no_rescale_l" in faults and c == 1 else (l * sc).astype(f32)) + sm).astype(f32)
            m = mn
        with err():
            lse = np.where(l > 0, m + (zero if "lse_m" in faults else np.log(np.where(l > 0, l, one), dtype=f32)), f32(-np.inf)).astype(f32)
            inv = np.where(l > 0, one / np.where(l > 0, l, one), zero).astype(f32)
            a2 = np.where(valid[..., None], np.exp(e - m[dI, tc], dtype=f32) * inv[dI, tc], zero).astype(f32)
        for c in range(NC):
            for j in range(64):
                vj = valid[:, c, j]
                if vj.any() and not ("skip_lane63" in faults and j == 63):
                    out = np.where(vj[:, None, None], out + (a2[:, c, j, :, None] * tab[ic[:, c, j]]).astype(f32), out).astype(f32)

    # backward
    res = dict(out=out, lse=lse)
    gflat = g.reshape(n, hd)
    with err():
        lse_s = lse[dI, tc] if rel else lse[:, None, None, :]
        arg = e - lse_s
        if "dot_fma" in faults:
            qk = np.zeros(idx.shape + (H,), dtype=f32)
            qk[valid] = _segment_sums((inp["q"][dd] * inp["k"][pI]).reshape(-1, hd), D)
            arg = (np.float64(scale) * qk.astype(np.float64) - lse_s.astype(np.float64)).astype(f32)
        a = np.where(valid[..., None], np.exp(arg, dtype=f32), zero).astype(f32)
    raw = bool(faults & {"raw_a", "rel_G"})
    gt = np.zeros((P, H, D), dtype=f32)
    if not rel and not raw:                                                        # S: a wave sum per chunk, chunk after chunk
        S = np.zeros((n, H), dtype=f32)
        for c in range(NC):
            S += _butterfly(lanes(a[:, c]), np.add)
        with err():
            a = np.where(S[:, None, None, :] > 0, a / np.where(S > 0, S, one)[:, None, None, :], zero).astype(f32)
    if rel:
        G = np.zeros((n, R, H), dtype=f32)
        S = np.zeros((n, R, H), dtype=f32)
        for c in range(NC):
            mask = oh[:, c][..., None]
            G += _butterfly(lanes(np.where(mask, (a[:, c] * gdot[:, c])[:, :, None, :], zero).astype(f32)), np.add)
            S += _butterfly(lanes(np.where(mask, a[:, c][:, :, None, :], zero).astype(f32)), np.add)
        with err():
            Gs = G if "rel_G" in faults else np.where(S > 0, G / np.where(S > 0, S, one), zero).astype(f32)
            if not raw:
                Sj = S[dI, tc]
                a = np.where(Sj > 0, a / np.where(Sj > 0, Sj, one), zero).astype(f32)
        sub = Gs[dI, tc]
    else:
        gout = _segment_sums(gflat * out.reshape(n, hd), D)
        if "gout_head" in faults:
            gout = np.roll(gout, 1, axis=1)
        sub = gout[:, None, None, :]
    t = np.where(valid[..., None], ((a * (gdot - sub).astype(f32)).astype(f32) * kf).astype(f32), zero).astype(f32)
    aE, tE = a[valid], t[valid]
    if case.op in ("gat", "rel"):
        np.add.at(gt, pI, (aE[..., None] * g[dd]).astype(f32))
        gel = np.zeros((P, H), dtype=f32)
        np.add.at(gel, pI, tE)
        if rel:
            ger = np.zeros((n, R, H), dtype=f32)
            for c in range(NC):
                ger += _butterfly(lanes(np.where(oh[:, c][..., None], t[:, c][:, :, None, :], zero).astype(f32)), np.add)
        else:
            ger = np.zeros((n, H), dtype=f32)
            for c in range(NC):
                ger += _butterfly(lanes(t[:, c]), np.add)
        res.update(gt=gt, gel=gel, ger=ger)
    elif case.op == "dot":
        q, k = inp["q"], inp["k"]
        np.add.at(gt, pI, (aE[..., None] * g[dd]).astype(f32))
        gk = np.zeros((P, H, D), dtype=f32)
        np.add.at(gk, pI, ((scale * tE).astype(f32)[..., None] * q[dd]).astype(f32))
        gq = np.zeros((n, H, D), dtype=f32)
        for c in range(NC):
            acc = np.zeros((n, H, D), dtype=f32)
            for j in range(64):
                vj = valid[:, c, j]
                if vj.any():
                    acc = np.where(vj[:, None, None], _fma(t[:, c, j, :, None], k[ic[:, c, j]], acc), acc)
            gq = (scale * acc).astype(f32) if c == 0 else (gq + (scale * acc).astype(f32)).astype(f32)
        res.update(gt=gt, gk=gk, gq=gq)
    else:
        attn = inp["attn"]
        kfc = np.where(z3 > 0, one, slope).astype(f32)
        uE = ((tE[..., None] * attn[None]).astype(f32) * kfc).astype(f32)         # [E, H, D]
        np.add.at(gt, pI, ((aE[..., None] * g[dd]).astype(f32) + uE).astype(f32))
        ug = np.zeros(idx.shape + (H, D), dtype=f32)
        ug[valid] = uE
        gd = np.zeros((n, H, D), dtype=f32)
        for c in range(NC):
            acc = np.zeros((n, H, D), dtype=f32)
            for j in range(64):
                if valid[:, c, j].any():
                    acc = (acc + ug[:, c, j]).astype(f32)
            gd = acc if c == 0 else (gd + acc).astype(f32)
        ga = np.zeros((H, D), dtype=f32)
        for i in range(len(dd)):                                                   # a chain over the edges, as a wave adds its rows'
            ga = (ga + (tE[i][:, None] * lz3[i]).astype(f32)).astype(f32)
        res.update(gt=gt, gd=gd, ga=ga)
    return res


# ---------------------------------------------------------------------------------------------------------------- the torch fallbacks

def fallback64(case):
    """Block.*_aggregate_torch in float64 with autograd -> the twin's dict (no lse: the fallbacks keep none)."""
    import torch
    from COALA_GNN.sampler import Block
    n, P, R = case.n_dst, case.P, case.R
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).requires_grad_(True)   # noqa: E731
    src = torch.arange(P)
    raw = case.idx
    if case.op in ("dot", "rel"):                                                  # the packed form names every slot's row itself
        raw = np.where(case.idx >= 0, 0, case.idx).astype(np.int32)
    if case.form == "fixed":
        b = Block(src, torch.from_numpy(np.ascontiguousarray(raw)), n)
    else:
        b = Block(src, None, n, indptr=torch.from_numpy(case.indptr), indices=torch.from_numpy(np.ascontiguousarray(raw)))
    rows = torch.from_numpy(case.idx.astype(np.int64))
    i = case.inp
    g = torch.from_numpy(i["g"].astype(np.float64))
    if case.op == "gat":
        t = [T(i["el"]), T(i["er"]), T(i["tab"])]
        out = b.gat_aggregate_torch(*t, negative_slope=float(case.slope))
        names = ("gel", "ger", "gt")
    elif case.op == "rel":
        t = [T(i["el"]), T(i["er"]), T(i["tab"])]
        out = b.rel_gat_aggregate_torch(*t, torch.from_numpy(case.typ.astype(np.int64)), R, rows=rows, negative_slope=float(case.slope))
        names = ("gel", "ger", "gt")
    elif case.op == "dot":
        t = [T(i["q"]), T(i["k"]), T(i["tab"])]
        out = b.dot_gat_aggregate_torch(*t, rows=rows, scale=float(case.scale))
        names = ("gq", "gk", "gt")
    else:
        t = [T(i["tab"]), T(i["fd"]), T(i["attn"])]
        out = b.gatv2_aggregate_torch(*t, negative_slope=float(case.slope))
        names = ("gt", "gd", "ga")
    grads = torch.autograd.grad((out * g).sum(), t, allow_unused=True)
    res = dict(out=out.detach().numpy())
    for name, gr, leaf in zip(names, grads, t):
        res[name] = (torch.zeros_like(leaf) if gr is None else gr).detach().numpy()
    return res
