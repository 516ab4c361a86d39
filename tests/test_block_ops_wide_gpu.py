"""GPU tests of the block ops (coala_block_* in coala_block_ops.hip) on tensors of more than 2^32 floats.

BASELINE's IGB configuration fetches 1.36 M input rows of 1024 floats per minibatch and the sampler allows 8.4 M rows per layer, so a
[n_src, 1024] table of more than 2^32 floats is a legal input to every block op.  Here one fp32 table X [2^22 + 4096, 1024] (17.2 GB),
filled once on the device, is shared by the module, with one zeroed buffer G of the same size for gradients.  At width 1024 the byte offset of a
row passes 2^32 at row 2^20, the float offset 2^31 at row 2^21 and 2^32 at row 2^22.  Probe rows: the 8 rows on each side of each of
these, row 0, the last row and 2,000 random rows.

  test_wide_source_table     X is the source table (for the attention ops viewed as [n, H, 1024 / H]; dot_gat reads it as k and as v and
                             asks for grad_k and grad_v in two calls, so that one gradient buffer is enough).  3,001 destination rows whose
                             neighbours are probe rows, addressed by their wide int32 indices; fixed form and the CSR form of the same
                             rows, forward and backward through the C ABI.  The probe rows are copied to the host and the indices
                             renumbered into them: on that compact twin every output must stay within the float64 reference and the
                             bounds of the op's own test file (imported from there).  The wide gradient table must be exactly 0 outside the
                             probe rows, and X unchanged.
  test_wide_destination_side n_dst = 2^22 + 4096 destination rows of fan-out 2 over a source table of 65,536 rows: the output and the
                             per-destination inputs (gatv2's feat_dst and dot_gat's q are X; grad_out is G with the probe rows filled)
                             are wide.  The forward is compared at the probe destinations with float64 on the twin, and as a whole, bit
                             for bit, with the same op run on slices of 2^20 destinations.  grad_out is nonzero on the probe destinations
                             only, so every other row adds exact zeros and the twin's bounds hold; per-destination gradients must be
                             exactly 0 outside the probe rows.  rel_sum's output is [n_dst, 3, 1024]: n_dst = 1,399,466 there, as many
                             rows of 3072 floats as G holds, 1,365 past the one at which the output reaches 2^32 floats.

Every test asserts that its indices (its probe destinations) lie on both sides of all three boundaries.

Measured on an MI355X.  torch.cuda.max_memory_allocated() of the file: 85,214,355,456 bytes (PEAK_BYTES) -- X, G and the two spare wide
buffers of the destination tests (68.8 GB), rel_sum's slice buffer of 12.9 GB and the temporaries of a sliced count_nonzero.  pytest
--durations: test_wide_source_table[gatv2-32-4] 3.3 s and [dot_gat-32-4] 3.2 s, the same ops at fan-out 16 1.9 s, every other source case
1.6 s or less -- the float64 reference of 67,000 edges of 1024 floats on the CPU is what takes the time; test_wide_destination_side 0.2 ..
1.9 s (rel_sum); 1.8 s of set-up; the file in 29 s.  In the
same run of the whole suite the parent commit's end-to-end training tests take 4.5 .. 5.4 s each and its slowest test 77 s
(test_bench_gpu.py)."""
import types

import numpy as np
import pytest

import _dot_gat_ref as RD
import _gatv2_ref as RV2
import test_block_ops_gpu as TB
import test_gat_ops_gpu as TG
import test_max_aggregate_gpu as TM
import test_rel_gat_ops_gpu as TRG
import test_rel_sum_gpu as TR
import test_weighted_sum_gpu as TW

pytestmark = pytest.mark.gpu

PEAK_BYTES = 85_214_355_456    # torch.cuda.max_memory_allocated() of this file on an MI355X; a test skips only when less than this is free
DIM = 1024
N_ROWS = 2**22 + 4096
N_DST = 3001              # destination rows of the wide-source case
N_SMALL = 65536           # source rows of the wide-destination case
SLICE = 2**20             # destinations per sliced run
R = 3
SLOPE = 0.2
ATTENTION = ("gat", "gatv2", "rel_gat", "dot_gat")


def _boundaries(width):
    """The first row whose offset reaches 2^32 bytes, 2^31 floats, 2^32 floats, for rows of `width` floats."""
    return tuple(-(-(2**e) // width) for e in (30, 31, 32))


def _probe_rows(n_rows, width, rng, n_random=2000):
    near = [b + d for b in _boundaries(width) for d in range(-8, 8)]
    return np.unique(np.concatenate([near, [0, n_rows - 1], rng.integers(0, n_rows, size=n_random)])).astype(np.int64)


def _assert_touches(rows, width=DIM):
    """`rows` (wide row numbers) lie on both sides of all three boundaries, within 8 rows of each."""
    rows = np.asarray(rows)
    for b in _boundaries(width):
        assert np.any((rows >= b - 8) & (rows < b)) and np.any((rows >= b) & (rows < b + 8)), f"nothing touches both sides of row {b}"


def _p(t):
    return t.data_ptr() if hasattr(t, "data_ptr") else t


@pytest.fixture(scope="module")
def wide(hiplib):
    import torch
    free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved()
    if free < PEAK_BYTES:
        pytest.skip(f"{free} bytes of device memory are free, the measured peak of this file is {PEAK_BYTES}")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20)
    X = torch.empty((N_ROWS, DIM), dtype=torch.float32, device="cuda")
    for a in range(0, N_ROWS, SLICE):
        X[a: a + SLICE].normal_(generator=gen)
    G = torch.zeros_like(X)
    assert X.numel() > 2**32
    probe = _probe_rows(N_ROWS, DIM, np.random.default_rng(7))
    w = types.SimpleNamespace(torch=torch, X=X, G=G, probe=probe, probe_t=torch.from_numpy(probe).cuda())
    w.x_t = X[w.probe_t].cpu().numpy()
    w.checksum = _checksum(torch, X)
    w.small = torch.empty((N_SMALL, DIM), dtype=torch.float32, device="cuda").normal_(generator=gen)
    spare = {}

    def buf(i):
        """Two more wide buffers, made on first use and shared by the wide-destination tests: with X and G the four wide tables of this file."""
        if i not in spare:
            spare[i] = torch.empty(N_ROWS * DIM, dtype=torch.float32, device="cuda")
        return spare[i]
    w.buf = buf
    yield w
    spare.clear()
    w.X = w.G = w.small = w.buf = X = G = None
    torch.cuda.empty_cache()


def _checksum(torch, table):
    """The sum of the table's words as integers, slice by slice (a reduction into int64 converts its whole input first)."""
    return sum(int(table[a: a + SLICE].view(torch.int32).sum(dtype=torch.int64)) for a in range(0, table.shape[0], SLICE))


def _nonzeros(torch, table):
    """torch.count_nonzero, slice by slice for the same reason."""
    return sum(int(torch.count_nonzero(table[a: a + SLICE])) for a in range(0, table.shape[0], SLICE))


def _take_rows(torch, table, rows_t, what):
    """The rows `rows_t` of a gradient table, which are then zeroed in place; everything else must be exactly 0."""
    got = table[rows_t].cpu().numpy()
    table[rows_t] = 0
    assert _nonzeros(torch, table) == 0, f"{what} is not exactly 0 outside the probe rows"
    return got


def _unchanged(w):
    assert _checksum(w.torch, w.X) == w.checksum and np.array_equal(w.X[w.probe_t].cpu().numpy(), w.x_t), "the table changed"
    assert _nonzeros(w.torch, w.G) == 0, "the gradient buffer was not left zeroed"


# ---------------------------------------------------------------------------------------------------- the C entries
def _call(L, name, blk, *args):
    from COALA_GNN_Pybind import _capi, current_stream
    fn = getattr(L, name.format("_csr" if blk.form == "csr" else ""))
    _capi.check(fn(0, *[_p(t) for t in blk.head], *[_p(a) for a in args], blk.n, *blk.fan, *blk.tail, current_stream()))


def _forward(L, op, blk, T, H):
    D = DIM // H
    b = lambda *tail: types.SimpleNamespace(form=blk.form, head=blk.head, n=blk.n, fan=blk.fan, tail=tail)   # noqa: E731
    if op == "mean":
        _call(L, "coala_block_mean_aggregate{}", b(DIM), T["x"], T["out"])
    elif op == "weighted":
        _call(L, "coala_block_weighted_sum{}", b(DIM), T["w"], T["x"], T["out"])
    elif op == "max":
        _call(L, "coala_block_max_aggregate{}", b(DIM), T["x"], T["out"], T["arg"])
    elif op == "rel_sum":
        _call(L, "coala_block_rel_sum{}", b(R, DIM), T["etype"], T["w"], T["x"], T["out"])
    elif op == "gat":
        _call(L, "coala_block_gat_aggregate{}", b(H, D, SLOPE), T["el"], T["er"], T["x"], T["out"], T["lse"])
    elif op == "gatv2":
        _call(L, "coala_block_gatv2_aggregate{}", b(H, D, SLOPE), T["x"], T["fd"], T["attn"], T["out"], T["lse"])
    elif op == "rel_gat":
        _call(L, "coala_block_rel_gat_aggregate{}", b(R, H, D, SLOPE), T["etype"], T["el"], T["er"], T["x"], T["out"], T["lse"])
    elif op == "dot_gat":
        _call(L, "coala_block_dot_gat_aggregate{}", b(H, D, float(RD.scale_of(D))), T["q"], T["x"], T["x"], T["out"], T["lse"])
    else:
        raise KeyError(op)


def _backward(L, op, blk, T, H, which=None):
    """which (dot_gat): 'k' asks for grad_q and grad_k, 'v' for grad_v alone -- both into T['gs']."""
    from COALA_GNN_Pybind import _capi, current_stream
    D = DIM // H
    b = lambda *tail: types.SimpleNamespace(form=blk.form, head=blk.head, n=blk.n, fan=blk.fan, tail=tail)   # noqa: E731
    if op == "mean":
        _call(L, "coala_block_mean_aggregate{}_backward", b(DIM), T["go"], T["gs"])
    elif op == "weighted":
        _call(L, "coala_block_weighted_sum{}_backward", b(DIM), T["w"], T["x"], T["go"], T["gs"], T["gw"])
    elif op == "max":
        _capi.check(L.coala_block_max_aggregate_backward(0, _p(T["arg"]), _p(T["go"]), _p(T["gs"]), blk.n, DIM, current_stream()))
    elif op == "rel_sum":
        _call(L, "coala_block_rel_sum{}_backward", b(R, DIM), T["etype"], T["w"], T["x"], T["go"], T["gs"], T["gw"])
    elif op == "gat":
        _call(L, "coala_block_gat_aggregate{}_backward", b(H, D, SLOPE), T["el"], T["er"], T["x"], T["out"], T["lse"], T["go"], T["gs"], T["gel"], T["ger"])
    elif op == "gatv2":
        blk2 = types.SimpleNamespace(form=blk.form, head=blk.head, n=T["parts"].shape[0], fan=(blk.n,) + tuple(blk.fan), tail=(H, D, SLOPE))
        _call(L, "coala_block_gatv2_aggregate{}_backward", blk2, T["x"], T["fd"], T["attn"], T["out"], T["lse"], T["go"], T["gs"], T["gd"], T["parts"])
    elif op == "rel_gat":
        _call(L, "coala_block_rel_gat_aggregate{}_backward", b(R, H, D, SLOPE), T["etype"], T["el"], T["er"], T["x"], T["lse"], T["go"], T["gs"], T["gel"], T["ger"])
    elif op == "dot_gat":
        grads = (T["gq"], T["gs"], None) if which == "k" else (None, None, T["gs"])
        _call(L, "coala_block_dot_gat_aggregate{}_backward", b(H, D, float(RD.scale_of(D))), T["q"], T["x"], T["x"], T["out"], T["lse"], T["go"], *grads)
    else:
        raise KeyError(op)


# ---------------------------------------------------------------------------------------------------- the twin's references
def _check(torch, op, tw, got, H, what, wave_rows=None, parts=None, cache=None):
    """Every output against the float64 reference and bounds of the op's own test file, on the compact twin: tw holds the fixed-form
    index array `nbr` [n_dst, f] into the twin's source rows `x` [n_src, 1024] and the op's other inputs; got the outputs, the
    per-source ones cut down to the twin's rows and every per-slot one in the fixed layout.  cache: a dict that keeps an attention op's
    reference for the next form of the same rows (a row of at most 32 edges is one chunk in either form, so the bounds are the same)."""
    cache = {} if cache is None else cache

    def once(make):
        if "ref" not in cache:
            cache["ref"] = make()
        return cache["ref"]
    nbr, x, go = tw["nbr"], tw["x"], tw["go"]
    n_dst, n_src, D = nbr.shape[0], x.shape[0], DIM // H
    x3, g3 = x.reshape(n_src, H, D), go.reshape(n_dst, H, D) if op != "rel_sum" else None
    o3 = lambda a: a.reshape(n_dst, H, D)   # noqa: E731
    if op == "mean":
        TB._check_forward(nbr, x, got["out"])
        TB._check_backward(nbr, go, n_src, got["gs"])
    elif op == "weighted":
        TW._check(*TW._edge_list(nbr=nbr), tw["w"], x, go, n_dst, got["out"], got["gs"], got["gw"], what)
    elif op == "max":
        want, want_arg = TM.ref_max_fixed(nbr, x)
        TM._same(got["out"], got["arg"], want, want_arg, what)
        TM._check_grad(got["gs"], want_arg, go, n_src, what)
    elif op == "rel_sum":
        TR._check(torch, *TR._edges(nbr=nbr), tw["etype"], tw["w"], x, go.reshape(n_dst, R * DIM), n_dst, R, got["out"], got["gs"], got["gw"], what)
    elif op == "gat":
        rows, srcs, nc = TG._edges_fixed(nbr)
        ref = once(lambda: TG.reference(rows, srcs, n_dst, n_src, nc, tw["el"], tw["er"], x3, g3))
        TG._check_all(dict(out=o3(got["out"]), lse=got["lse"], gf=got["gs"].reshape(n_src, H, D), gel=got["gel"], ger=got["ger"]), ref)
    elif op == "gatv2":
        rows, srcs, nc = RV2.edges_fixed(nbr)
        ref = once(lambda: RV2.reference(rows, srcs, n_dst, n_src, nc, x3, tw["fd"].reshape(n_dst, H, D), tw["attn"], g3, parts, wave_rows=wave_rows))
        RV2.check_all(dict(out=o3(got["out"]), lse=got["lse"], gs=got["gs"].reshape(n_src, H, D), gd=o3(got["gd"]), ga=got["ga"]), ref)
    elif op == "rel_gat":
        dst, row, typ, nc = TRG._edges("fixed", (nbr, tw["etype"]), R)
        ref = once(lambda: TRG.reference(dst, row, typ, n_dst, n_src, R, nc, tw["el"], tw["er"], x3, g3))
        TRG._check_all(dict(out=o3(got["out"]), lse=got["lse"], gf=got["gs"].reshape(n_src, H, D), gel=got["gel"], ger=got["ger"]), ref)
    elif op == "dot_gat":
        dst, rows, nc = RD.edges_fixed(nbr)
        ref = once(lambda: RD.reference(dst, rows, n_dst, n_src, nc, tw["q"].reshape(n_dst, H, D), x3, x3, g3, RD.scale_of(D)))
        RD.check_all(dict(out=o3(got["out"]), lse=got["lse"], gq=o3(got["gq"]), gk=got["gk"].reshape(n_src, H, D), gv=got["gv"].reshape(n_src, H, D)), ref)
    else:
        raise KeyError(op)


def _per_destination(op, rng, n, f, H):
    """The op's inputs that are not the source table, for n destination rows of f slots (host arrays): per-slot w and etype, per-row er,
    feat_dst, q, and attn."""
    D = DIM // H
    s = {}
    if op in ("weighted", "rel_sum"):
        s["w"] = rng.standard_normal((n, f)).astype(np.float32)
        s["w"][rng.random((n, f)) < 0.1] = 0
    if op == "rel_sum":
        s["etype"] = TR._types(rng, (n, f), R)
    if op == "rel_gat":
        s["etype"] = TRG._types(rng, (n, f), R, True)
    if op == "gat":
        s["er"] = rng.standard_normal((n, H)).astype(np.float32)
    if op == "rel_gat":
        s["er"] = rng.standard_normal((n, R, H)).astype(np.float32)
    if op == "gatv2":
        s["fd"] = rng.standard_normal((n, H * D)).astype(np.float32)
        s["attn"] = rng.standard_normal((H, D)).astype(np.float32)
        s["attn"][0, 0] = -abs(s["attn"][0, 0])
    if op == "dot_gat":
        s["q"] = rng.standard_normal((n, H * D)).astype(np.float32)
    return s


def _outputs(torch, op, n, f_or_E, H, bufs=None):
    """Device buffers of the per-destination outputs of n rows; bufs: two flat fp32 buffers to cut the wide ones (out, arg) from."""
    dev = "cuda"
    width = R * DIM if op == "rel_sum" else DIM
    T = {"out": torch.empty((n, width), device=dev) if bufs is None else bufs[0][: n * width].view(n, width)}
    if op == "max":
        T["arg"] = torch.empty((n, DIM), dtype=torch.int32, device=dev) if bufs is None else bufs[1][: n * DIM].view(torch.int32).view(n, DIM)
    if op in ATTENTION:
        T["lse"] = torch.empty((n, R, H) if op == "rel_gat" else (n, H), device=dev)
    if op in ("weighted", "rel_sum"):
        T["gw"] = torch.empty(f_or_E, device=dev)
    if op in ("gat", "rel_gat"):
        T["ger"] = torch.empty((n, R, H) if op == "rel_gat" else (n, H), device=dev)
    if op == "gatv2":
        T["parts"] = torch.empty((RV2.default_parts(n), DIM), device=dev)
    return T


# ---------------------------------------------------------------------------------------------------- 1. wide source table
def _twin_nbr(rng, n, f, nt, forced):
    """int32 [n, f] into nt twin rows: -1 anywhere, a source twice in a row, rows without a valid entry (row 0 among them); the rows
    `forced` (twin indices) each stand in slot 0 of a row of their own."""
    nbr = rng.integers(0, nt, size=(n, f)).astype(np.int32)
    nbr[rng.random((n, f)) < 0.25] = -1
    rep = rng.random(n) < 0.15
    nbr[rep, f - 1] = nbr[rep, 0]
    nbr[rng.random(n) < 0.05] = -1
    nbr[0] = -1
    nbr[10: 10 + len(forced), 0] = forced
    return nbr


SOURCE_CASES = [(op, f, 1) for op in ("mean", "weighted", "max", "rel_sum") for f in (1, 16, 32)]
SOURCE_CASES += [(op, f, H) for op in ATTENTION for f, H in ((1, 4), (16, 1), (32, 4))]


@pytest.mark.parametrize("op,f,H", SOURCE_CASES)
def test_wide_source_table(wide, op, f, H):
    from COALA_GNN_Pybind import _capi
    torch, L, w = wide.torch, _capi.load(), wide
    rng = np.random.default_rng(sum(map(ord, op)) * 131 + f * 7 + H)
    nt, n = len(w.probe), N_DST
    near = np.flatnonzero(np.isin(w.probe, [b + d for b in _boundaries(DIM) for d in range(-8, 8)] + [0, N_ROWS - 1]))
    nbr_t = _twin_nbr(rng, n, f, nt, near)
    nbr_w = np.where(nbr_t >= 0, w.probe[np.maximum(nbr_t, 0)], -1).astype(np.int32)
    assert int(nbr_w.max()) == N_ROWS - 1 and int(nbr_w.max()) * DIM > 2**32
    _assert_touches(nbr_w[nbr_w >= 0])
    valid = nbr_t >= 0
    small = _per_destination(op, rng, n, f, H)
    go = rng.standard_normal((n, R * DIM if op == "rel_sum" else DIM)).astype(np.float32)
    tw = dict(small, nbr=nbr_t, x=w.x_t, go=go)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    EL = GEL = None
    if op in ("gat", "rel_gat"):
        tw["el"] = rng.standard_normal((nt, H)).astype(np.float32)
        EL, GEL = torch.zeros((N_ROWS, H), device="cuda"), torch.zeros((N_ROWS, H), device="cuda")
        EL[w.probe_t] = up(tw["el"])
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(valid.sum(1), out=indptr[1:])
    cache = {}
    for form in ("fixed", "csr"):
        what = f"{op}, {form} form, fan-out {f}, H {H}"
        slot = (lambda a: a) if form == "fixed" else (lambda a: a[valid])
        if form == "fixed":
            head, fan = (up(nbr_w),), (f,)
        else:
            head, fan = (up(indptr), up(np.append(nbr_w[valid], np.int32(-1)))), ()
        blk = types.SimpleNamespace(form=form, head=head, n=n, fan=fan)
        T = _outputs(torch, op, n, (n, f) if form == "fixed" else (int(valid.sum()),), H)
        T.update(x=w.X, gs=w.G, go=up(go), el=EL, gel=GEL)
        for key in ("w", "etype"):
            if key in small:
                T[key] = up(np.append(slot(small[key]).reshape(-1), small[key].dtype.type(0)))
        for key in ("er", "fd", "attn", "q"):
            if key in small:
                T[key] = up(small[key])
        if op == "gatv2":
            T["gd"] = torch.empty((n, DIM), device="cuda")
        if op == "dot_gat":
            T["gq"] = torch.empty((n, DIM), device="cuda")
        _forward(L, op, blk, T, H)
        got = {}
        if op == "dot_gat":
            _backward(L, op, blk, T, H, "k")
            got["gk"] = _take_rows(torch, w.G, w.probe_t, f"grad_k: {what}")
            _backward(L, op, blk, T, H, "v")
            got["gv"] = _take_rows(torch, w.G, w.probe_t, f"grad_v: {what}")
        else:
            _backward(L, op, blk, T, H)
            got["gs"] = _take_rows(torch, w.G, w.probe_t, f"the gradient table: {what}")
        for key in ("out", "lse", "ger", "gd", "gq"):
            if key in T:
                got[key] = T[key].cpu().numpy()
        if "gw" in T:
            gw = T["gw"].cpu().numpy()
            got["gw"] = gw
            if form == "csr":
                got["gw"] = np.zeros((n, f), np.float32)
                got["gw"][valid] = gw
        if op == "max":
            arg = T["arg"].cpu().numpy()
            at = np.searchsorted(w.probe, np.maximum(arg, 0))
            assert np.all((arg < 0) | (w.probe[np.minimum(at, nt - 1)] == arg)), f"an argmax is no probe row: {what}"
            got["arg"] = np.where(arg >= 0, at, -1).astype(np.int32)
        if GEL is not None:
            got["gel"] = _take_rows(torch, GEL, w.probe_t, f"grad_el: {what}")
        if op == "gatv2":
            got["ga"] = T["parts"].sum(0).view(H, DIM // H).cpu().numpy()
        _check(torch, op, tw, got, H, what, parts=RV2.default_parts(n), cache=cache)
    _unchanged(w)


@pytest.mark.parametrize("H", [1, 4])
def test_pair_dot_on_the_wide_table(wide, H):
    """pair_dot has no block: pairs of probe rows of X [n, H, 1024 / H], forward and backward, within test_pair_dot_gpu.py's bounds
    (gamma(D + 1) sum|h_u h_v| forward; gamma(m + 1) sum|terms| for a row that m endpoints name)."""
    from COALA_GNN_Pybind import _capi, current_stream
    torch, L, w = wide.torch, _capi.load(), wide
    rng = np.random.default_rng(H)
    nt, P, D = len(w.probe), 6144, DIM // H
    near = np.flatnonzero(np.isin(w.probe, [b + d for b in _boundaries(DIM) for d in range(-8, 8)] + [0, N_ROWS - 1]))
    src, dst = rng.integers(0, nt, size=P), rng.integers(0, nt, size=P)
    src[100: 100 + len(near)], dst[300: 300 + len(near)] = near, near[::-1]
    src[5], dst[5] = near[0], near[0]
    src[10], dst[11] = -1, -1
    ok = (src >= 0) & (dst >= 0)
    wide_of = lambda a: np.where(a >= 0, w.probe[np.maximum(a, 0)], -1).astype(np.int32)   # noqa: E731
    _assert_touches(wide_of(src)[src >= 0])
    _assert_touches(wide_of(dst)[dst >= 0])
    g = rng.standard_normal((P, H)).astype(np.float32)
    d_s, d_d, d_g = (torch.from_numpy(a).cuda() for a in (wide_of(src), wide_of(dst), g))
    out = torch.empty((P, H), device="cuda")
    _capi.check(L.coala_block_pair_dot(0, w.X.data_ptr(), d_s.data_ptr(), d_d.data_ptr(), out.data_ptr(), P, H, D, current_stream()))
    _capi.check(L.coala_block_pair_dot_backward(0, w.X.data_ptr(), d_s.data_ptr(), d_d.data_ptr(), d_g.data_ptr(), w.G.data_ptr(), P, H, D, current_stream()))
    gh = _take_rows(torch, w.G, w.probe_t, "grad_h").reshape(nt, H, D)
    h = w.x_t.reshape(nt, H, D).astype(np.float64)
    a, b = np.where(ok, src, 0), np.where(ok, dst, 0)
    prod = h[a] * h[b] * ok[:, None, None]
    err = np.abs(out.cpu().numpy().astype(np.float64) - prod.sum(-1))
    assert np.all(err <= TB._gamma(D + 1) * np.abs(prod).sum(-1)) and np.all(out.cpu().numpy()[~ok] == 0)
    gref, gmag, m = np.zeros_like(h), np.zeros_like(h), np.zeros(nt, dtype=np.int64)
    for rows, t in ((a, g[:, :, None] * h[b] * ok[:, None, None]), (b, g[:, :, None] * h[a] * ok[:, None, None])):
        np.add.at(gref, rows, t)
        np.add.at(gmag, rows, np.abs(t))
        np.add.at(m, rows[ok], 1)
    assert np.all(np.abs(gh.astype(np.float64) - gref) <= TB._gamma(m + 1)[:, None, None] * gmag) and np.all(gh[m == 0] == 0)
    _unchanged(w)


# ---------------------------------------------------------------------------------------------------- 2. wide destination side
DEST_CASES = [(op, 1) for op in ("mean", "weighted", "max", "rel_sum")] + [(op, 4) for op in ATTENTION]


@pytest.mark.parametrize("op,H", DEST_CASES)
def test_wide_destination_side(wide, op, H):
    from COALA_GNN_Pybind import _capi
    torch, L, w = wide.torch, _capi.load(), wide
    seed = sum(map(ord, op))
    rng = np.random.default_rng(seed)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    f, D = 2, DIM // H
    width = R * DIM if op == "rel_sum" else DIM                       # floats of `out` per destination row
    n = w.G.numel() // width                                          # rel_sum: 1,365 rows past the one where `out` reaches 2^32 floats
    assert n * width > 2**32 + 8 * width and (n == N_ROWS or op == "rel_sum")
    pd = _probe_rows(n, width, rng)
    _assert_touches(pd, width)
    pd_t = torch.from_numpy(pd).cuda()
    randn = lambda *shape: torch.empty(shape, device="cuda").normal_(generator=gen)   # noqa: E731
    nbr = torch.randint(0, N_SMALL, (n, f), device="cuda", generator=gen).to(torch.int32)
    nbr[torch.rand((n, f), device="cuda", generator=gen) < 0.2] = -1
    T = dict(x=w.small)
    if op in ("weighted", "rel_sum"):
        T["w"] = randn(n, f)
    if op in ("rel_sum", "rel_gat"):
        T["etype"] = torch.randint(0, R + 1, (n, f), device="cuda", generator=gen).to(torch.int32)     # R: out of range, skipped
    if op in ("gat", "rel_gat"):
        T["el"], T["er"] = randn(N_SMALL, H), (randn(n, R, H) if op == "rel_gat" else randn(n, H))
    if op == "gatv2":
        T["fd"], T["attn"] = w.X, randn(H, D)
    if op == "dot_gat":
        T["q"] = w.X
    blk = types.SimpleNamespace(form="fixed", head=(nbr,), n=n, fan=(f,))
    T.update(_outputs(torch, op, n, (n, f), H, bufs=(w.buf(0), w.buf(1))))
    assert T["out"].numel() > 2**32
    _forward(L, op, blk, T, H)
    # the same op on slices of at most 2^20 destinations: the whole output, bit for bit
    S = _outputs(torch, op, SLICE, (SLICE, f), H)
    for a in range(0, n, SLICE):
        m = min(SLICE, n - a)
        Ts = dict(T)
        for key in ("w", "etype", "er", "fd", "q"):
            if key in T:
                Ts[key] = T[key][a: a + m]
        Ts.update({k: v for k, v in S.items() if k in ("out", "arg", "lse")})
        _forward(L, op, types.SimpleNamespace(form="fixed", head=(nbr[a: a + m],), n=m, fan=(f,)), Ts, H)
        for key in ("out", "arg", "lse"):
            if key in S:
                assert torch.equal(T[key][a: a + m].view(torch.int32), S[key][:m].view(torch.int32)), f"{op}: {key} of rows {a} .. {a + m} differs from the sliced run"
    S = Ts = None
    # backward: grad_out is nonzero on the probe destinations only
    go = rng.standard_normal((len(pd), width)).astype(np.float32)
    GO = w.G.view(-1)[: n * width].view(n, width)
    GO[pd_t] = torch.from_numpy(go).cuda()
    T.update(go=GO, gs=torch.zeros((N_SMALL, DIM), device="cuda"))
    if op in ("gat", "rel_gat"):
        T["gel"] = torch.zeros((N_SMALL, H), device="cuda")
    if op == "gatv2":
        T["gd"] = w.buf(1).view(n, DIM)
    if op == "dot_gat":
        T["gq"] = w.buf(1).view(n, DIM)
    got = {}
    # the compact twin: the probe destinations and the source rows they name
    nbr_p = nbr[pd_t].cpu().numpy()
    used = np.unique(nbr_p[nbr_p >= 0]).astype(np.int64)
    used_t = torch.from_numpy(used).cuda()
    tw = dict(nbr=np.where(nbr_p >= 0, np.searchsorted(used, np.maximum(nbr_p, 0)), -1).astype(np.int32), x=w.small[used_t].cpu().numpy(), go=go)
    for key in ("w", "etype", "er", "fd", "q"):
        if key in T:
            tw[key] = T[key][pd_t].cpu().numpy()
    if "attn" in T:
        tw["attn"] = T["attn"].cpu().numpy()
    if "el" in T:
        tw["el"] = T["el"][used_t].cpu().numpy()
    what = f"{op}, {n} destination rows, H {H}"
    if op == "dot_gat":
        _backward(L, op, blk, T, H, "k")
        got["gk"] = _take_rows(torch, T["gs"], used_t, f"grad_k: {what}")
        _backward(L, op, blk, T, H, "v")
        got["gv"] = _take_rows(torch, T["gs"], used_t, f"grad_v: {what}")
    else:
        _backward(L, op, blk, T, H)
        got["gs"] = _take_rows(torch, T["gs"], used_t, f"grad_src: {what}")
    if "gel" in T:
        got["gel"] = _take_rows(torch, T["gel"], used_t, f"grad_el: {what}")
    for key in ("out", "lse"):
        if key in T:
            got[key] = T[key][pd_t].cpu().numpy()
    for key in ("gw", "ger", "gd", "gq"):                              # per-destination gradients: exactly 0 off the probe rows
        if key in T:
            got[key] = _take_rows(torch, T[key], pd_t, f"{key}: {what}")
    if op == "max":
        arg = T["arg"][pd_t].cpu().numpy()
        at = np.searchsorted(used, np.maximum(arg, 0))
        assert np.all((arg < 0) | (used[np.minimum(at, len(used) - 1)] == arg)), f"an argmax is no source of its row: {what}"
        got["arg"] = np.where(arg >= 0, at, -1).astype(np.int32)
    if op == "gatv2":
        got["ga"] = T["parts"].sum(0).view(H, D).cpu().numpy()
    GO[pd_t] = 0
    T = None
    _check(torch, op, tw, got, H, what, wave_rows=pd, parts=RV2.default_parts(n))
    _unchanged(w)
