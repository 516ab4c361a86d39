"""The cache kernels at every line size, access width, tag width and cold tier, checked bit for bit and for stray writes.

coala_cache.hip instantiates K1 (probe_gather_kernel), K2 (miss_fill_kernel) and scatter_rows_kernel per line size (cache_dim 128 / 256 /
512 / 1024) and access width (16-byte accesses when dim % 4 == 0 and every row buffer is 16-byte aligned, 4-byte accesses otherwise),
K1 also per tag width, FULL (dim == cache_dim at 16-byte width) and REDIR (the split serve's redirected slice).  The cold tier picks
K2's launch shape: a narrow grid of 64-row verdict tiles with the dynamic deal behind pinned host memory, a wide grid of one-chunk
tiles with the static deal behind HBM.  The matrix below reaches every (line size, width, tag, FULL, REDIR) combination the product
dispatches, behind both tiers; the looping K1 on 4-KiB lines at 4-byte width, and more fill launches in one batch than K2 has ticket
counters, have a test each.

Every batch is checked against the plain gather feat[idx] (bytes; rejected ids give rows of exactly 0.0) and against the CPU oracle
run on the same ids: hit / miss / rejected counters, tag table, cursors, colour metadata and colour counters.  Every output region,
redirect target and cold table sits inside a buffer padded with a sentinel, and the padding is checked after every call."""
import numpy as np
import pytest

from _util import GUARD, SENTINEL, ColorFiles, Guarded, PinnedTable, synth_colors

pytestmark = pytest.mark.gpu

WAYS = 32
BAD_IDS = (-1, None, 2 ** 40)   # None: num_rows

# layouts per line size: (name, dim, output offset, cold-table offset) in floats; an odd offset is off 16-byte alignment
#   full: dim == cache_dim, aligned (16-byte accesses, FULL)    part: dim % 4 == 0 below cache_dim, aligned (16-byte accesses)
#   odd: dim % 4 != 0 in the upper part of the class            outoff: dim == cache_dim, output one float off alignment
#   coldoff: dim % 4 == 0, cold table one float off alignment   (the last three take the 4-byte path)
LAYOUTS = {
    128: [("full", 128, 0, 0), ("part", 64, 0, 0), ("odd", 127, 0, 0), ("outoff", 128, 1, 0), ("coldoff", 124, 0, 1)],
    256: [("full", 256, 0, 0), ("part", 132, 0, 0), ("odd", 255, 0, 0), ("outoff", 256, 1, 0), ("coldoff", 252, 0, 1)],
    512: [("full", 512, 0, 0), ("part", 260, 0, 0), ("odd", 509, 0, 0), ("outoff", 512, 1, 0), ("coldoff", 508, 0, 1)],
    1024: [("full", 1024, 0, 0), ("part", 516, 0, 0), ("odd", 602, 0, 0), ("odd", 1023, 0, 0), ("outoff", 1024, 1, 0),
           ("coldoff", 1020, 0, 1)],
}
CASES = [pytest.param(cd, dim, out_off, cold_off, k, id=f"cd{cd}-{name}{dim}") for cd, ls in LAYOUTS.items()
         for k, (name, dim, out_off, cold_off) in enumerate(ls)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


class ColdTable:
    """The feature table as the cold tier: pinned host memory ("host") or a device tensor ("hbm"), `off` floats into a buffer padded
    with the sentinel on both sides."""

    def __init__(self, torch, P, feat, tier, off):
        self.tier, self.feat = tier, feat
        if tier == "host":
            self.t = PinnedTable(P, feat, offset=off)
            self.ptr = self.t.device_ptr
        else:
            self.t = Guarded(torch, *feat.shape, off=off, fill=feat)
            self.ptr = self.t.ptr

    def assert_unchanged(self):
        if self.tier == "host":
            assert self.t.guards_intact() and self.t.array.tobytes() == self.feat.tobytes(), "the cold table changed"
        else:
            assert self.t.region().tobytes() == self.feat.tobytes(), "the cold table changed"

    def close(self):
        if self.tier == "host":
            self.t.close()


def _expected(feat, idx):
    """feat[idx] with the rows of rejected ids (outside [0, num_rows)) = 0.0."""
    good = (idx >= 0) & (idx < len(feat))
    want = feat[np.where(good, idx, 0)]
    want[~good] = 0.0
    return want, good


class Checker:
    """One cache handle and its oracle twin, compared after every batch."""

    def __init__(self, oracle, cache, orc, num_colors):
        self.O, self.cache, self.orc, self.num_colors = oracle, cache, orc, num_colors
        self.bad_total = 0

    def feed(self, idx, good):
        self.orc.read_feature(idx[good], self.O.SCHED_HITS_FIRST, want_rows=False)   # the oracle never sees rejected ids
        self.bad_total += int((~good).sum())

    def compare(self, what):
        orc = self.orc
        assert self.cache.stats() == (orc.hit_cnt, orc.miss_cnt, self.bad_total), f"{what}: counters"
        keys, cnt, meta = self.cache.dump()
        assert np.array_equal(keys, orc.keys()), f"{what}: tag table"
        assert np.array_equal(cnt, orc.set_cnt()), f"{what}: cursors"
        assert np.array_equal(meta.astype(np.uint64), orc.color_meta()), f"{what}: colour metadata"
        cc = np.zeros(self.num_colors + 1, dtype=np.int32)
        self.cache.get_cache_data(cc.ctypes.data, self.num_colors + 1)
        assert np.array_equal(cc, orc.color_counters()), f"{what}: colour counters"

    def resident(self, num_rows):
        k = self.orc.keys().reshape(-1)
        return np.unique(k[k < np.uint64(num_rows)]).astype(np.int64)


def _batches(rng, num_rows, num_sets, last_set, resident):
    """The batch sequence of one case as (kind, ids or a callable of the resident ids).  Batches with misses alternate with batches
    without, with misses at both generation parities (1, 3 | 4, 6) and none at both (2 | 5, 7); the empty batch takes no generation.
    num_rows - 1 is in every batch: the last miss of the first batch (so it is cached), then never evicted -- no other miss maps to
    its set -- and a hit from then on."""
    last = num_rows - 1
    others = np.setdiff1d(np.arange(num_rows - 1), np.arange(last_set, num_rows, num_sets))   # ids outside the last row's set

    def with_bad(ids):
        bad = np.array([num_rows if b is None else b for b in BAD_IDS], dtype=np.int64)
        pos = rng.choice(len(ids) + len(bad), size=len(bad), replace=False)
        out = np.empty(len(ids) + len(bad), dtype=np.int64)
        keep = np.ones(len(out), dtype=bool)
        keep[pos] = False
        out[pos] = bad
        out[keep] = ids
        return out

    def shuffled_with_last(ids):
        ids = np.append(ids, last)
        return ids[rng.permutation(len(ids))]

    def cold():          # distinct misses, a few of them twice, rejected ids; num_rows - 1 last
        ids = rng.choice(others, size=700, replace=False)
        ids = np.concatenate([ids, rng.choice(ids, size=40)])
        return np.append(with_bad(ids[rng.permutation(len(ids))]), last)

    def hits():          # cached ids only, with repeats: K2 finds nothing to fill
        res = resident()
        return shuffled_with_last(rng.choice(res, size=min(600, 2 * len(res))))

    def one_set():       # more than 32 misses into one set (not the last row's), plus random ids, repeats and rejected ids
        s = (last_set + 1 + int(rng.integers(0, num_sets - 1))) % num_sets if num_sets > 1 else last_set
        members = np.setdiff1d(np.arange(s, num_rows - 1, num_sets), resident())
        ids = np.concatenate([rng.choice(members, size=min(48, len(members)), replace=False), rng.choice(others, size=300)])
        return with_bad(shuffled_with_last(np.concatenate([ids, rng.choice(ids, size=30)])))

    def dups():          # heavy repeats
        pool = rng.choice(others, size=150, replace=False)
        return shuffled_with_last(rng.choice(pool, size=900))

    def fresh():         # misses and rejected ids
        return with_bad(shuffled_with_last(rng.choice(others, size=500, replace=False)))

    assert all(len(np.arange(s, num_rows - 1, num_sets)) > 48 + WAYS for s in range(num_sets)), "table too small for a set overflow"
    return [("cold", cold), ("hits", hits), ("one_set", one_set), ("dups", dups), ("hits", hits), ("empty", None),
            ("fresh", fresh), ("hits", hits)]


@pytest.mark.parametrize("tier", ["host", "hbm"])
@pytest.mark.parametrize("tag64", [False, True], ids=["tags32", "tags64"])
@pytest.mark.parametrize("cd,dim,out_off,cold_off,k", CASES)
def test_cache_shapes_match_gather_and_oracle(hiplib, oracle, torch_cuda, tmp_path, cd, dim, out_off, cold_off, k, tag64, tier):
    """One batch sequence per case: cold misses, all-hit repeats, an overflowing set, repeats, rejected ids, an empty batch; whole
    reads, and split serves (probe with a redirected slice, fills over shuffled range sets) into an aligned and an unaligned target."""
    torch = torch_cuda
    P = hiplib
    rng = np.random.default_rng(cd * 1000 + dim * 10 + 4 * k + 2 * tag64 + (tier == "hbm"))
    cache_mb = 3 if (k + tag64 + (tier == "hbm")) % 2 else (1 if cd >= 512 else 2)   # set counts: 3 MB -> not a power of two
    num_sets = oracle.num_sets(cache_mb, cd)
    num_rows = max(3000, 100 * num_sets + 77)
    feat = oracle.make_features(num_rows, dim, seed=cd + dim)
    num_colors = 9
    color, tk, sc = synth_colors(num_rows, num_colors, seed=dim)
    files = ColorFiles(tmp_path, color, tk, sc)
    items = np.zeros(2, dtype=np.int64)
    nd = P.Node_distributor_pybind(items.ctypes.data, 0, 1, 1, 1, files.color_file, files.topk_file, files.score_file)
    cold = ColdTable(torch, P, feat, tier, cold_off)
    ctrl = P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, dim, True)
    cache = P.Isolated_Cache(ctrl, nd, 0, 1, cache_mb, cold.ptr, num_rows=num_rows, tag64=tag64)
    g = cache.geometry()
    assert (g.cache_dim, g.num_sets) == (cd, num_sets)
    orc = oracle.OracleCache(cache_mb, dim, feat, node_color=color, num_colors=num_colors)
    chk = Checker(oracle, cache, orc, num_colors)
    last_set = (num_rows - 1) % num_sets
    split_target = {2: 0, 6: 1, 7: 0}   # split serves: batch -> redirect target offset (1: off alignment)
    for b, (kind, make) in enumerate(_batches(rng, num_rows, num_sets, last_set, lambda: chk.resident(num_rows))):
        what = f"batch {b} ({kind})"
        idx = make() if make else np.zeros(0, dtype=np.int64)
        n = len(idx)
        d_idx = torch.from_numpy(idx).cuda() if n else torch.zeros(1, dtype=torch.int64, device="cuda")
        out = Guarded(torch, n, dim, off=out_off)
        want, good = _expected(feat, idx)
        miss0, hit0 = orc.miss_cnt, orc.hit_cnt
        if b not in split_target:
            cache.read_feature(out.ptr, d_idx.data_ptr(), n)
            got = out.region()
        else:
            lo, hi = sorted(int(x) for x in rng.integers(0, n + 1, size=2))
            lo, hi = min(lo, n // 4), max(hi, n // 2)   # a slice of a quarter of the batch at least
            use_map = b != 7
            perm = rng.permutation(hi - lo).astype(np.int64)
            d_map = torch.from_numpy(perm).cuda() if use_map else None
            other = Guarded(torch, hi - lo, dim, off=split_target[b], fill=-4.0)
            cache.serve_probe_redirect(out.ptr, d_idx.data_ptr(), n, lo, hi, other.ptr, d_map.data_ptr() if use_map else 0)
            cuts = sorted({0, n, *(int(c) for c in rng.integers(0, n + 1, size=11))})
            ranges = list(zip(cuts[:-1], cuts[1:]))
            rng.shuffle(ranges)
            for part in range(3):
                if ranges[part::3]:
                    cache.serve_fill_ranges(out.ptr, d_idx.data_ptr(), n, ranges[part::3])
            got = out.region().copy()
            oth = other.region()
            assert np.all(got[lo:hi] == -2.0), f"{what}: a redirected row was also written to the batch's own output"
            got[lo:hi] = oth[perm if use_map else np.arange(hi - lo)]
        assert got.tobytes() == want.tobytes(), f"{what}: rows differ from feat[idx]"
        chk.feed(idx, good)
        chk.compare(what)
        if kind == "hits":
            assert orc.miss_cnt == miss0 and orc.hit_cnt - hit0 == n, f"{what}: not all hits"
        elif kind != "empty":
            assert orc.miss_cnt > miss0, f"{what}: no misses"
    assert orc.hit_cnt > 0 and chk.bad_total == 3 * 3
    cold.assert_unchanged()
    cache.close()
    cold.close()


@pytest.mark.parametrize("cd,dims", [pytest.param(cd, dims, id=f"cd{cd}") for cd, dims in
                                     [(128, (128, 96, 127)), (256, (256, 200, 253)), (512, (512, 300, 509)), (1024, (1024, 516, 602))]])
@pytest.mark.parametrize("out_off,src_off", [(0, 0), (1, 0), (0, 3)], ids=["aligned", "outoff", "srcoff"])
def test_scatter_every_geometry(hiplib, torch_cuda, cd, dims, out_off, src_off):
    """scatter / scatter_ranges (out[map[r]] = src[r]) at every line size, at both access widths (dim % 4, buffer alignment), against
    numpy, with guard words around both buffers; rows of `out` that no map entry names keep their value."""
    torch = torch_cuda
    P = hiplib
    rng = np.random.default_rng(cd + out_off + 7 * src_off)
    for dim in dims:
        feat = np.zeros((4, dim), dtype=np.float32)
        table = PinnedTable(P, feat)
        ctrl = P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, dim, True)
        cache = P.Isolated_Cache(ctrl, None, 0, 1, 1, table.device_ptr, num_rows=4)
        assert cache.geometry().cache_dim == cd
        n, m = 777, 777 + 41
        src_h = rng.standard_normal((n, dim)).astype(np.float32)
        mp = rng.permutation(m)[:n].astype(np.int64)
        d_map = torch.from_numpy(mp).cuda()
        src = Guarded(torch, n, dim, off=src_off, fill=src_h)
        out = Guarded(torch, m, dim, off=out_off, fill=-3.0)
        cache.scatter(out.ptr, src.ptr, d_map.data_ptr(), n)
        want = np.full((m, dim), -3.0, dtype=np.float32)
        want[mp] = src_h
        assert out.region().tobytes() == want.tobytes(), f"dim {dim}: scatter"
        assert src.region().tobytes() == src_h.tobytes()
        # the rows of a few shuffled ranges only (the rounds of a split row exchange)
        cuts = sorted({0, n, *(int(c) for c in rng.integers(0, n + 1, size=8))})
        ranges = list(zip(cuts[:-1], cuts[1:]))
        rng.shuffle(ranges)
        ranges = ranges[: max(1, len(ranges) - 2)]
        out = Guarded(torch, m, dim, off=out_off, fill=-3.0)
        cache.scatter_ranges(out.ptr, src.ptr, d_map.data_ptr(), ranges)
        want = np.full((m, dim), -3.0, dtype=np.float32)
        for lo, hi in ranges:
            want[mp[lo:hi]] = src_h[lo:hi]
        assert out.region().tobytes() == want.tobytes(), f"dim {dim}: scatter_ranges"
        cache.close()
        table.close()


@pytest.mark.parametrize("cd,dim,tag64", [(128, 128, False), (1024, 1023, True)], ids=["cd128-full-tags32", "cd1024-odd1023-tags64"])
def test_more_fill_launches_than_ticket_counters(hiplib, oracle, torch_cuda, cd, dim, tag64):
    """A host cold tier deals K2's tiles dynamically, from one ticket counter per fill launch, for the first kFillSlots (8) fill
    launches of a batch; later ones fall back to the static deal.  Here every batch is one probe and 11 fill calls (serve_fill and
    serve_fill_ranges), each with more 64-row tiles than its grid has waves (4 x 64 blocks at cache_dim 128, 4 x 24 at 1024: the
    narrow host-tier grid), over two batches (both ticket parities).  Rows, counters and tables equal the oracle's and those of a
    twin cache that serves each batch in one call."""
    torch = torch_cuda
    P = hiplib
    rng = np.random.default_rng(cd)
    host_waves = 4 * min(64, max(24, 16 * 1024 // cd))   # K2's waves behind a host tier (launch_shape: 4-wave blocks, 24..64 of them)
    per_call = 64 * host_waves + 333            # > host_waves tiles of 64 rows
    calls = 11
    num_rows = 30000 if cd == 128 else 12000
    feat = oracle.make_features(num_rows, dim, seed=11)
    table = PinnedTable(P, feat, offset=0)
    ctrl = P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, dim, True)
    split = P.Isolated_Cache(ctrl, None, 0, 1, 2, table.device_ptr, num_rows=num_rows, tag64=tag64)
    whole = P.Isolated_Cache(ctrl, None, 0, 1, 2, table.device_ptr, num_rows=num_rows, tag64=tag64)
    orc = oracle.OracleCache(2, dim, feat)
    bad_total = 0
    for b in range(2):
        n = calls * per_call + int(rng.integers(0, per_call))
        idx = rng.integers(0, num_rows, size=n).astype(np.int64)
        idx[rng.choice(n, size=5, replace=False)] = [-1, num_rows, 2 ** 40, num_rows + 1, -7]
        idx[-1] = num_rows - 1
        d_idx = torch.from_numpy(idx).cuda()
        want, good = _expected(feat, idx)
        out = Guarded(torch, n, dim)
        split.serve_probe(out.ptr, d_idx.data_ptr(), n)
        bounds = [k * per_call for k in range(calls)] + [n]   # call k fills [bounds[k], bounds[k+1]): >= per_call rows
        for k in rng.permutation(calls):
            lo, hi = bounds[k], bounds[k + 1]
            if k % 2:
                split.serve_fill(out.ptr, d_idx.data_ptr(), n, lo, hi)
            else:
                c1, c2 = sorted(int(x) for x in rng.integers(lo, hi + 1, size=2))
                parts = [(lo, c1), (c1, c2), (c2, hi)]
                rng.shuffle(parts)
                split.serve_fill_ranges(out.ptr, d_idx.data_ptr(), n, parts)
        ref = Guarded(torch, n, dim)
        whole.serve(ref.ptr, d_idx.data_ptr(), n)
        got = out.region()
        assert got.tobytes() == want.tobytes(), f"batch {b}: rows differ from feat[idx]"
        assert ref.region().tobytes() == want.tobytes(), f"batch {b}: the one-call serve differs from feat[idx]"
        m0 = orc.miss_cnt
        orc.read_feature(idx[good], oracle.SCHED_HITS_FIRST, want_rows=False)
        assert orc.miss_cnt > m0
        bad_total += int((~good).sum())
        for c in (split, whole):
            assert c.stats() == (orc.hit_cnt, orc.miss_cnt, bad_total), f"batch {b}: counters"
            keys, cnt, _ = c.dump()
            assert np.array_equal(keys, orc.keys()) and np.array_equal(cnt, orc.set_cnt()), f"batch {b}: tables"
    assert table.guards_intact() and table.array.tobytes() == feat.tobytes()
    split.close()
    whole.close()
    table.close()


def test_looping_probe_at_4k_lines_4byte_width(hiplib, oracle, torch_cuda):
    """Geo<1024, 1> has one row per chunk, so a batch of more than 2^20 rows (the papers100M 15,10,5 minibatch has 1,081,344) takes the
    looping probe+gather kernel instead of the loop-free one: dim 602, 1,100,000 distinct rows of a procedural pinned table, read twice.
    Rows exact (checked on the GPU in slices), padding behind the output untouched, second pass all hits, counters and tag table
    equal to the tag-only oracle's."""
    torch = torch_cuda
    P = hiplib
    from COALA_GNN.synthetic import alloc_pinned_table, feature_rows_torch
    dim, n, cache_mb = 602, 1_100_000, 16384
    num_rows = n
    table = alloc_pinned_table(num_rows, dim, seed=6, device=0)
    ctrl = P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, dim, True)
    cache = P.Isolated_Cache(ctrl, None, 0, 1, cache_mb, table.device_ptr, num_rows=num_rows)
    g = cache.geometry()
    assert g.cache_dim == 1024 and n > (1 << 20)   # one row per chunk at 4-byte width: more than 2^20 chunks
    assert n // g.num_sets < WAYS                  # every set holds all of its ids: the second pass is all hits
    orc = oracle.OracleCache(cache_mb, dim, np.zeros((1, dim), dtype=np.float32), tag_only=True)
    ids = torch.randperm(num_rows, generator=torch.Generator().manual_seed(5))
    d_idx = ids.cuda()
    flat = torch.empty(n * dim + GUARD, dtype=torch.float32, device="cuda")
    out = flat[: n * dim].view(n, dim)
    sentinel = torch.full((GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    for pass_no in range(2):
        out.fill_(-1.0)
        flat[n * dim:] = sentinel
        cache.read_feature(out.data_ptr(), d_idx.data_ptr(), n)
        orc.read_feature(ids.numpy(), oracle.SCHED_HITS_FIRST, want_rows=False)
        for lo in range(0, n, 1 << 17):
            hi = min(n, lo + (1 << 17))
            assert torch.equal(out[lo:hi], feature_rows_torch(d_idx[lo:hi], dim, 6)), f"pass {pass_no}: rows {lo}..{hi}"
        assert torch.equal(flat[n * dim:].view(torch.int32), sentinel.view(torch.int32)), "write behind the output"
        hit, miss, bad = cache.stats()
        assert (hit, miss, bad) == (orc.hit_cnt, orc.miss_cnt, 0)
        assert (hit, miss) == ((0, n) if pass_no == 0 else (n, n))
    keys, cnt, _ = cache.dump()
    assert np.array_equal(keys, orc.keys()) and np.array_equal(cnt, orc.set_cnt())
    cache.close()
    table.close()
