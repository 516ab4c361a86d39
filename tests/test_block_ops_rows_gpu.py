"""GPU tests of the block ops (coala_block_* in coala_block_ops.hip) on ragged blocks in which one wave takes several unlike rows.

Every kernel deals rows to waves by wave_rows() and keeps state between a wave's rows: the online softmax's max, sum and rescale, the
backward's <g, out>, S and t sums and its one-chunk flag, RelGAT's 256 group states, the first chunk that the mean, max and typed-sum
kernels hold in registers.  The grid is capped at 32,768 waves, so only a block of more rows makes a wave take a second one.  Here
n_dst = 3 * 32768 + 5: every wave takes three rows and five take four.  The first 512 waves take the rows of tests/_row_layouts.py's
table (many chunks -> empty, empty -> many chunks, one edge <-> many chunks, 64 <-> 65, 128 -> 3, 200 -> 70, empty -> empty -> 1, and
each kind as a wave's last row); every other row has 0..3 edges: 226,847 edges over 4,096 sources, some repeated inside a row, the last
7 never referenced.  The typed ops get types in which a wave's consecutive rows share no relation, and a row of one relation is
followed by a row of all R.  The GATv2 backward with a partials buffer has a grid of `parts` blocks: parts = 2 over 35 rows gives every
wave four or five rows of the same table (two waves, 17 and 18 rows, at H * D > 1024), and default_parts(5000) = 1024 blocks of about
five rows makes 904 waves take a second row.

Every case runs through the C ABI in the CSR form with the op's own _run, float64 reference, bounds and sentinel guards, imported from
the op's test file: no tolerance is new.  Those bounds take the chunks of each row (nc) and its edge count row by row, so unlike rows
need nothing added.  The mean op's checks take a fixed-form index array: a ragged row is given to them padded with -1, which the CSR
kernel's divisor (the row's length; no -1 inside) equals.  Then the rows of the busy waves are packed into a block of 1,541 rows and
run again: there every wave takes one row, and each row's out, lse, arg and per-destination (per-slot) gradients must have the bits of
the big launch -- no bound at all, so a carried state shows even where float64 bounds are loose.

The issue's case of default_parts at n_dst = 5000 is kept as set; its "five rows per wave" is five rows per block (four waves), so two
turns per busy wave is what it covers.  Two waves cannot end on three kinds of row, and two turns cannot hold what takes three rows or
starts in the middle of a sequence: those cases pass assert_transitions the names their size cannot hold, and it raises if one of them
is there after all.

Measured on an MI355X.  pytest --durations of this file: 30 passed in 9.4 s; test_rel_gat_rows[64-4-5-False] and [16-16-4-True] 1.3 s
each (their float64 reference has 25 M (row, relation, head) groups), 1.3 s of set-up, test_rel_sum_rows[68-1] 0.6 s, every other case
under 0.5 s; none over 5 s.  The parent commit's test_gat_csr_against_float64[100003-12-1-3-1-False], the nearest case there was (one
head, H * D = 3), takes 0.48 s on the same machine; test_gat_rows takes 0.09 .. 0.25 s a case.

What the file catches, on scratch builds of coala_block_ops.hip that change floating-point state only (never committed).  First the
edit as a plain removal, then the same reset done once per wave in front of its row loop -- right for a wave's first row, stale for
every later one, which is the defect this file is about:
  (a) softmax_row_begin's m_run / l_run reset    removed: all of test_gat_rows, test_dot_gat_rows, test_gatv2_rows and the five partials
                                                 tests fail.  Once per wave: the nine *_rows cases fail (the partials tests pass: their
                                                 forward runs on the row grid, one row a wave at 35 and 5,000 rows).
  (b) backward_row_front's gout / ssum reset     removed or once per wave: test_gat_rows and test_dot_gat_rows fail, all six cases.
  (c) the GAT backward's ter reset               removed or once per wave: test_gat_rows fails, all three cases.
  (d) rel_gat_aggregate_kernel's m_run / l_run   removed or once per wave: test_rel_gat_rows fails, all four cases.
      reset loop
  (e) mean_aggregate_kernel's inv taken once     test_mean_rows fails, all three cases.
      from the wave's first row
(a) and (d) shared one build with (e), (b) and (c) had one each; the failing tests tell them apart.  The suite from before this file
catches the plain removals too, in most cases of the ops' own files: LDS that nothing has set is read by every wave's first row.  It
catches (e) in test_mean_aggregate_against_float64's five fixed-form cases of n_dst >= 32,769, and the once-per-wave forms of (a), (b)
and (c) only in the attention ops' fixed-form cases of 100,003 rows and in test_gat_csr_against_float64[100003-...] -- three to five
cases per build, all with one head and H * D <= 4, none on a ragged block for GATv2 or dot_gat -- and the once-per-wave form of (d)
not at all: no older RelGAT case reaches a wave's second row.  (Run against the older test files of the ops changed in each build,
not against the whole suite.)"""
import functools
import types

import numpy as np
import pytest

import _dot_gat_ref as RD
import _gatv2_ref as RV2
import _row_layouts as RL
import test_block_ops_gpu as TB
import test_dot_gat_ops_gpu as TD
import test_gat_ops_gpu as TG
import test_gatv2_ops_gpu as TV2
import test_max_aggregate_gpu as TM
import test_rel_gat_ops_gpu as TRG
import test_rel_sum_gpu as TR
import test_weighted_sum_gpu as TW
from _util import Guarded

pytestmark = pytest.mark.gpu

N_DST, BUSY, N_SRC = RL.ROW_GRID_N_DST, RL.ROW_GRID_BUSY, 4096
N_WAVES = RL.row_grid_waves(N_DST)
WIDE = 200                          # the longest row of the table
DIM_OFF = [(4, 0), (5, 0), (68, 1)]  # float4; scalar; two 64-lane passes of the scalar path (68 floats one float off 16-byte alignment)
ATTENTION = [(2, 4, 0, False), (3, 5, 1, True), (4, 16, 0, False)]   # H, D, float offset, big scores: vec4 in one pass; scalar, heads across lanes; 64 floats
REL_GAT = [(3, 2, 4, True), (3, 2, 4, False), (64, 4, 5, False), (16, 16, 4, True)]   # R, H, D, sorted types; the last: R * H = 256 states
R_SUM = 3


def _cut(indptr, rows):
    """The CSR rows `rows` as a block of their own: -> (its indptr, the slots of the big block it takes, in order)"""
    deg = np.diff(indptr)[rows]
    ip = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(deg, out=ip[1:])
    return ip, np.repeat(indptr[rows] - ip[:-1], deg) + np.arange(ip[-1])


def _padded(blk, rows, width):
    """The rows as a fixed-form index array, -1 behind each row's edges"""
    ip, slots = _cut(blk.indptr, rows)
    deg = np.diff(ip)
    assert deg.max(initial=0) <= width
    nbr = np.full((len(rows), width), -1, dtype=np.int32)
    nbr[np.repeat(np.arange(len(rows)), deg), np.arange(ip[-1]) - np.repeat(ip[:-1], deg)] = blk.idx[slots]
    return nbr


@functools.lru_cache(maxsize=None)
def _block():
    """The block every row-grid test runs on (made once; no test writes to it), and its busy rows as a block of one row a wave."""
    rng = np.random.default_rng(20261126)
    deg = RL.transition_degrees(N_DST, N_WAVES, rng, BUSY)
    indptr = np.zeros(N_DST + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    idx = rng.integers(0, N_SRC - 7, size=int(indptr[-1])).astype(np.int32)
    rep = np.flatnonzero((deg >= 2) & (rng.random(N_DST) < 0.3))
    idx[indptr[rep + 1] - 1] = idx[indptr[rep]]                     # a source twice in the row
    sub = np.flatnonzero(np.arange(N_DST) % N_WAVES < BUSY)
    sub_indptr, slots = _cut(indptr, sub)
    assert len(sub) == 3 * BUSY + 5 and RL.row_grid_waves(len(sub)) >= len(sub)
    return types.SimpleNamespace(deg=deg, indptr=indptr, idx=idx, E=len(idx), sub=sub, sub_indptr=sub_indptr, slots=slots, sub_idx=idx[slots])


def _layout():
    blk = _block()
    RL.assert_transitions(blk.deg, N_WAVES)
    assert int(blk.idx.max()) < N_SRC - 7
    return blk


def _same_bits(big, small, what):
    """big: the busy rows (slots) of the big launch; small: the same rows of the launch that gives every wave one row"""
    a, b = np.ascontiguousarray(big).view(np.int32), np.ascontiguousarray(small).view(np.int32)
    bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())} words of a wave's later rows differ from the same rows run one a wave; first at {tuple(np.argwhere(bad)[0])}"


def _scaled(rng, shape):
    a = rng.standard_normal(shape).astype(np.float32)
    a[rng.random(shape[0]) < 0.03] *= np.float32(1e6)
    return a


# ---------------------------------------------------------------------------------------------------- mean, weighted sum, max, rel_sum
def _mean_csr(torch, L, indptr, idx, x, go, off):
    from COALA_GNN_Pybind import _capi, current_stream
    n_dst, (n_src, dim) = len(indptr) - 1, x.shape
    dp, di = torch.from_numpy(np.asarray(indptr)).cuda(), torch.from_numpy(np.append(idx, np.int32(-1))).cuda()
    h_buf, h = TB._device(torch, x, off)
    o_buf, o = TB._device(torch, np.empty((n_dst, dim), np.float32), off, fill=float(TB.SENTINEL))
    g_buf, g = TB._device(torch, go, off)
    gs_buf, gs = TB._device(torch, np.empty((n_src, dim), np.float32), off, fill=0.0)
    _capi.check(L.coala_block_mean_aggregate_csr(0, dp.data_ptr(), di.data_ptr(), h, o, n_dst, dim, current_stream()))
    _capi.check(L.coala_block_mean_aggregate_csr_backward(0, dp.data_ptr(), di.data_ptr(), g, gs, n_dst, dim, current_stream()))
    torch.cuda.synchronize()
    assert np.array_equal(TB._region(h_buf, off, x.shape), x) and np.array_equal(TB._region(g_buf, off, go.shape), go)
    return TB._region(o_buf, off, (n_dst, dim)), TB._region(gs_buf, off, (n_src, dim))


def _small_and_long(blk):
    return np.flatnonzero(blk.deg <= 3), np.flatnonzero(blk.deg > 3)


@pytest.mark.parametrize("dim,off", DIM_OFF)
def test_mean_rows(hiplib, dim, off):
    import torch
    from COALA_GNN_Pybind import _capi
    L, blk = _capi.load(), _layout()
    rng = np.random.default_rng(dim)
    x, go = _scaled(rng, (N_SRC, dim)), _scaled(rng, (N_DST, dim))
    out, gs = _mean_csr(torch, L, blk.indptr, blk.idx, x, go, off)
    for rows, width in zip(_small_and_long(blk), (3, WIDE)):
        TB._check_forward(_padded(blk, rows, width), x, out[rows])
    TB._check_backward(_padded(blk, np.arange(N_DST), WIDE), go, N_SRC, gs)
    assert np.all(gs[N_SRC - 7:] == 0.0)
    one, _ = _mean_csr(torch, L, blk.sub_indptr, blk.sub_idx, x, go[blk.sub], off)
    _same_bits(out[blk.sub], one, "mean out")


@pytest.mark.parametrize("dim,off", DIM_OFF)
def test_weighted_sum_rows(hiplib, dim, off):
    import torch
    from COALA_GNN_Pybind import _capi
    L, blk = _capi.load(), _layout()
    rng = np.random.default_rng(100 + dim)
    w = rng.standard_normal(blk.E).astype(np.float32)
    w[rng.random(blk.E) < 0.1] = 0
    x, go = _scaled(rng, (N_SRC, dim)), _scaled(rng, (N_DST, dim))
    out, gs, gw = TW._run_csr(L, torch, blk.indptr, blk.idx, w, x, go, off)
    TW._check(*TW._edge_list(indptr=blk.indptr, idx=blk.idx), w, x, go, N_DST, out, gs, gw, f"rows dim={dim}")
    assert np.all(gs[N_SRC - 7:] == 0.0)
    one, _, one_gw = TW._run_csr(L, torch, blk.sub_indptr, blk.sub_idx, w[blk.slots], x, go[blk.sub], off)
    _same_bits(out[blk.sub], one, "weighted sum out")
    _same_bits(gw[blk.slots], one_gw, "weighted sum grad_w")


@pytest.mark.parametrize("dim,off", DIM_OFF)
def test_max_rows(hiplib, dim, off):
    """Values, arg and the backward through the kernel's arg, on the tie-heavy values with +-0, +-inf and NaN."""
    import torch
    from COALA_GNN_Pybind import _capi, current_stream
    L, blk = _capi.load(), _layout()
    rng = np.random.default_rng(200 + dim)
    x = TM._values(rng, "special", N_SRC, dim)
    out, arg = TM._forward(L, torch, x, off, indptr=blk.indptr, idx=blk.idx)
    want, want_arg = np.empty_like(out), np.empty_like(arg)
    for rows, width in zip(_small_and_long(blk), (3, WIDE)):
        want[rows], want_arg[rows] = TM.ref_max_fixed(_padded(blk, rows, width), x)
    TM._same(out, arg, want, want_arg, f"rows dim={dim}")
    assert np.all(out[blk.deg == 0] == 0) and np.all(arg[blk.deg == 0] == -1)
    go = TM._grad_out(rng, N_DST, dim)
    d_arg = torch.from_numpy(arg).cuda()
    gg, gs = Guarded(torch, N_DST, dim, off, go), Guarded(torch, N_SRC, dim, off, 0.0)
    _capi.check(L.coala_block_max_aggregate_backward(0, d_arg.data_ptr(), gg.ptr, gs.ptr, N_DST, dim, current_stream()))
    torch.cuda.synchronize()
    k = TM._check_grad(gs.region(), want_arg, go, N_SRC, f"rows backward dim={dim}")
    assert np.all(k[N_SRC - 7:] == 0)
    one, one_arg = TM._forward(L, torch, x, off, indptr=blk.sub_indptr, idx=blk.sub_idx)
    _same_bits(out[blk.sub], one, "max out")
    _same_bits(arg[blk.sub], one_arg, "max arg")


@pytest.mark.parametrize("dim,off", DIM_OFF)
def test_rel_sum_rows(hiplib, dim, off):
    import torch
    blk = _layout()
    rng = np.random.default_rng(300 + dim)
    R = R_SUM
    t = RL.transition_types(blk.deg, N_WAVES, R, rng, BUSY)
    RL.assert_type_transitions(blk.deg, t, N_WAVES, R, BUSY)
    w = rng.standard_normal(blk.E).astype(np.float32)
    w[rng.random(blk.E) < 0.1] = 0
    x, go = _scaled(rng, (N_SRC, dim)), _scaled(rng, (N_DST, R * dim))
    case = TR._Case(torch, x, t, w, off, R, indptr=blk.indptr, idx=blk.idx)
    out, _ = TR._check_forward(torch, case, f"rows dim={dim}")
    gs, gw = case.backward(go)
    TR._check(torch, *case.edges(), t, w, x, go, N_DST, R, None, gs, gw, f"rows backward dim={dim}")
    assert np.all(gs[N_SRC - 7:] == 0.0)
    sub = TR._Case(torch, x, t[blk.slots], w[blk.slots], off, R, indptr=blk.sub_indptr, idx=blk.sub_idx)
    _same_bits(out[blk.sub], sub.forward(), "rel_sum out")
    _same_bits(gw[blk.slots], sub.backward(go[blk.sub])[1], "rel_sum grad_w")


# ---------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("H,D,off,big", ATTENTION)
def test_gat_rows(hiplib, H, D, off, big):
    import torch
    from COALA_GNN_Pybind import _capi
    L, blk = _capi.load(), _layout()
    rng = np.random.default_rng(400 + H * D)
    el, er, feat, g = TG._inputs(rng, N_SRC, N_DST, H, D, big)
    got = TG._run(torch, L, "csr", (blk.indptr, blk.idx), N_DST, N_SRC, el, er, feat, g, off)
    rows, srcs, nc = TG._edges_csr(blk.indptr, blk.idx)
    TG._check_all(got, TG.reference(rows, srcs, N_DST, N_SRC, nc, el, er, feat, g))
    assert np.all(got["gf"][N_SRC - 7:] == 0.0) and np.all(got["gel"][N_SRC - 7:] == 0.0)
    one = TG._run(torch, L, "csr", (blk.sub_indptr, blk.sub_idx), len(blk.sub), N_SRC, el, er[blk.sub], feat, g[blk.sub], off)
    for k in ("out", "lse", "ger"):
        _same_bits(got[k][blk.sub], one[k], f"gat {k}")


@pytest.mark.parametrize("H,D,off,big", ATTENTION)
def test_dot_gat_rows(hiplib, H, D, off, big):
    import torch
    from COALA_GNN_Pybind import _capi
    L, blk = _capi.load(), _layout()
    rng = np.random.default_rng(500 + H * D)
    q, k, v, g = RD.make_inputs(rng, N_SRC, N_DST, H, D, big)
    scale = RD.scale_of(D)
    got = TD._run(torch, L, "csr", (blk.indptr, blk.idx), N_DST, N_SRC, q, k, v, g, scale, off)
    dst, rr, nc = RD.edges_csr(blk.indptr, blk.idx)
    RD.check_all(got, RD.reference(dst, rr, N_DST, N_SRC, nc, q, k, v, g, scale), log=print)
    assert np.all(got["gk"][N_SRC - 7:] == 0.0) and np.all(got["gv"][N_SRC - 7:] == 0.0)
    one = TD._run(torch, L, "csr", (blk.sub_indptr, blk.sub_idx), len(blk.sub), N_SRC, q[blk.sub], k, v, g[blk.sub], scale, off)
    for name in ("out", "lse", "gq"):
        _same_bits(got[name][blk.sub], one[name], f"dot_gat {name}")


def _gatv2_check(got, ref, names):
    """_gatv2_ref.check_all for a call that asks for no grad_attn (it is what puts the backward on the row grid)"""
    for k in names:
        RV2.check(k, got[k], ref[k], print)
    full = ~ref["empty"]
    RV2.check("lse", got["lse"][full], (ref["lse"][0][full], ref["lse"][1][full]), print)
    assert np.all(np.isneginf(got["lse"][ref["empty"]])), "lse of a row without a valid edge is not -inf"
    assert np.all(got["out"][ref["empty"]] == 0.0) and np.all(got["gd"][ref["empty"]] == 0.0), "a row without a valid edge is not exactly 0"
    assert all(np.isfinite(got[k]).all() for k in names)


@pytest.mark.parametrize("H,D,off,big", ATTENTION)
def test_gatv2_rows(hiplib, H, D, off, big):
    """grad_attn is null: the backward then runs on the row grid like the other ops."""
    import torch
    from COALA_GNN_Pybind import _capi
    L, blk = _capi.load(), _layout()
    rng = np.random.default_rng(600 + H * D)
    fs, fd, attn, g = RV2.make_inputs(rng, N_SRC, N_DST, H, D, big)
    want = (True, True, False)
    got = TV2._run(torch, L, "csr", (blk.indptr, blk.idx), N_DST, N_SRC, fs, fd, attn, g, off, want=want)
    rows, srcs, nc = RV2.edges_csr(blk.indptr, blk.idx)
    _gatv2_check(got, RV2.reference(rows, srcs, N_DST, N_SRC, nc, fs, fd, attn, g, RV2.default_parts(N_DST)), ("out", "gs", "gd"))
    assert np.all(got["gs"][N_SRC - 7:] == 0.0)
    one = TV2._run(torch, L, "csr", (blk.sub_indptr, blk.sub_idx), len(blk.sub), N_SRC, fs, fd[blk.sub], attn, g[blk.sub], off, want=want)
    for k in ("out", "lse", "gd"):
        _same_bits(got[k][blk.sub], one[k], f"gatv2 {k}")


@pytest.mark.parametrize("R,H,D,srt", REL_GAT)
def test_rel_gat_rows(hiplib, R, H, D, srt):
    import torch
    from COALA_GNN_Pybind import _capi
    L, blk = _capi.load(), _layout()
    rng = np.random.default_rng(700 + R * H * D + srt)
    typ = RL.transition_types(blk.deg, N_WAVES, R, rng, BUSY, srt)
    RL.assert_type_transitions(blk.deg, typ, N_WAVES, R, BUSY)
    el, er, feat, g = TRG._inputs(rng, N_SRC, N_DST, R, H, D, False)
    graph = (blk.indptr, blk.idx, typ)
    got = TRG._run(torch, L, "csr", graph, N_DST, N_SRC, R, el, er, feat, g, 0)
    dst, row, t, nc = TRG._edges("csr", graph, R)
    TRG._check_all(got, TRG.reference(dst, row, t, N_DST, N_SRC, R, nc, el, er, feat, g))
    assert np.all(got["gf"][N_SRC - 7:] == 0.0) and np.all(got["gel"][N_SRC - 7:] == 0.0)
    one = TRG._run(torch, L, "csr", (blk.sub_indptr, blk.sub_idx, typ[blk.slots]), len(blk.sub), N_SRC, R, el, er[blk.sub], feat, g[blk.sub], 0)
    for k in ("out", "lse", "ger"):
        _same_bits(got[k][blk.sub], one[k], f"rel_gat {k}")


# ---------------------------------------------------------------------------------------------------- gatv2 backward with partials
def _partials_case(torch, L, n_dst, n_src, parts, busy, H, D, big, allow, seed):
    """The GATv2 backward with a partials buffer of `parts` rows on a table layout; then with one row a wave, bit for bit."""
    n_waves = RL.partials_waves(parts, H * D)
    rng = np.random.default_rng(seed)
    deg = RL.transition_degrees(n_dst, n_waves, rng, busy)
    RL.assert_transitions(deg, n_waves, allow)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    idx = rng.integers(0, n_src - 7, size=int(indptr[-1])).astype(np.int32)
    fs, fd, attn, g = RV2.make_inputs(rng, n_src, n_dst, H, D, big)
    got = TV2._run(torch, L, "csr", (indptr, idx), n_dst, n_src, fs, fd, attn, g, 0, parts=parts)
    rows, srcs, nc = RV2.edges_csr(indptr, idx)
    RV2.check_all(got, RV2.reference(rows, srcs, n_dst, n_src, nc, fs, fd, attn, g, parts, wave_rows=np.arange(n_dst)), log=print)
    assert np.all(got["gs"][n_src - 7:] == 0.0)
    one_parts = -(-n_dst // (n_waves // parts))                     # a block's waves take one row each
    one = TV2._run(torch, L, "csr", (indptr, idx), n_dst, n_src, fs, fd, attn, g, 0, parts=one_parts)
    for k in ("out", "lse", "gd"):
        _same_bits(got[k], one[k], f"gatv2 with partials {k}")


@pytest.mark.parametrize("H,D,big", [(2, 4, False), (8, 16, True), (10, 64, False), (16, 65, False)])
def test_gatv2_backward_with_partials_rows(hiplib, H, D, big):
    """H * D = 8, 128, 640 (1, 2 and 16 register passes, four waves a block) and 1040 (one wave a block: two waves of 18 and 17 rows, which
    have two last rows between them -- the one transition that size cannot hold)."""
    import torch
    from COALA_GNN_Pybind import _capi
    allow = ("last:empty",) if H * D > 1024 else ()
    _partials_case(torch, _capi.load(), RL.PARTS_N_DST, 64, RL.PARTS, None, H, D, big, allow, 800 + H * D)


def test_gatv2_backward_with_default_partials_rows(hiplib):
    """default_parts(5000) = 1024 blocks of four waves over 5,000 rows: about five rows a block, so 904 waves take a second row.  Two
    turns hold nothing of three rows, and the table's sequences start with neither 65 -> 64 nor many chunks -> 1."""
    import torch
    from COALA_GNN_Pybind import _capi
    n_dst = RL.DEFAULT_PARTS_N_DST
    assert RV2.default_parts(n_dst) == 1024
    _partials_case(torch, _capi.load(), n_dst, 1024, 1024, BUSY, 4, 16, False, ("65->64", "empty->empty->1", "many-chunk->1"), 900)
