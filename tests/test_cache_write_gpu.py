"""GPU tests of the write-through row updates (coala_cache_write_rows / coala_cache_adagrad_rows) through Isolated_Cache: the cold
row and EVERY cache line of an id get the new value, nothing else of the table or the cache changes, and a later read returns the
table's bytes whether it hits or misses.  References and bounds: tests/_embedding_ref.py (mode 0 is bitwise)."""
import numpy as np
import pytest

from _embedding_ref import check_add, check_adagrad, make_grad, make_state
from _util import ColorFiles, PinnedTable, synth_colors

pytestmark = pytest.mark.gpu

LR, EPS, ALPHA = 0.05, 1e-10, -0.3
NUM_COLORS = 12


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def _off_tensor(torch, arr, off):
    """arr on the device, starting `off` floats into its allocation (1: off 16-byte alignment)."""
    flat = torch.zeros(arr.size + off + 3, dtype=torch.float32, device="cuda")
    view = flat[off: off + arr.size].view(arr.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    return view


class Rig:
    """A pinned table of random rows, an isolated cache with colours over it, an Adagrad state in HBM, and the checks (a)-(e)."""

    def __init__(self, torch, P, tmp_path, dim, cache_mb, num_rows, tag64=False, table_off=None, buf_off=0, seed=0, sync=True):
        self.torch, self.P, self.dim, self.rows, self.buf_off = torch, P, dim, num_rows, buf_off
        self.rng = np.random.default_rng(seed)
        feat = self.rng.uniform(-1.0, 1.0, size=(num_rows, dim)).astype(np.float32)
        self.table = PinnedTable(P, feat, offset=table_off)
        self.color, tk, sc = synth_colors(num_rows, NUM_COLORS, seed=1)
        files = ColorFiles(tmp_path, self.color, tk, sc)
        self._items = np.arange(8, dtype=np.int64)
        ctrl = P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, dim, True)
        self._nd = P.Node_distributor_pybind(self._items.ctypes.data, 0, 4, 1, 1, files.color_file, files.topk_file, files.score_file)
        self.cache = P.Isolated_Cache(ctrl, self._nd, 0, 1, cache_mb, self.table.device_ptr, num_rows=num_rows, tag64=tag64, sync=sync)
        self.state = _off_tensor(torch, make_state(self.rng, (num_rows, dim)), buf_off)

    def close(self):
        self.cache.close()
        self.table.close()

    def read(self, ids):
        torch = self.torch
        ids = np.asarray(ids, dtype=np.int64)
        out = torch.full((max(len(ids), 1), self.dim), -7.0, dtype=torch.float32, device="cuda")
        d = torch.from_numpy(ids).cuda() if len(ids) else torch.zeros(1, dtype=torch.int64, device="cuda")
        self.cache.read_feature(out.data_ptr(), d.data_ptr(), len(ids))
        return out.cpu().numpy()[: len(ids)]

    def cache_state(self):
        keys, cnt, meta = self.cache.dump()
        colors = np.zeros(NUM_COLORS + 1, dtype=np.int32)
        self.cache.get_cache_data(colors.ctypes.data, NUM_COLORS + 1)
        return keys, cnt, meta, colors, self.cache.stats()

    def mixed_ids(self, n, hot):
        """n pairwise distinct ids: about half cached (hot), the rest fresh, and -- from n = 2 on -- one outside the table."""
        if n == 0:
            return np.zeros(0, dtype=np.int64), 0
        n_bad = 1 if n >= 2 else 0
        n_hot = min((n - n_bad) // 2, len(hot))
        fresh_pool = np.setdiff1d(np.arange(self.rows), hot)
        ids = np.concatenate([self.rng.choice(hot, size=n_hot, replace=False),
                              self.rng.choice(fresh_pool, size=n - n_bad - n_hot, replace=False),
                              np.array([self.rows + 17] * n_bad, dtype=np.int64)])
        return self.rng.permutation(ids).astype(np.int64), n_bad

    def call_and_check(self, op, ids, n_bad, hot):
        torch, cache, tab = self.torch, self.cache, self.table
        n = len(ids)
        good = ids[(ids >= 0) & (ids < self.rows)]
        gpos = np.flatnonzero((ids >= 0) & (ids < self.rows))
        src = make_grad(self.rng, (max(n, 1), self.dim))
        d_src = _off_tensor(torch, src, self.buf_off)
        d_ids = torch.from_numpy(ids).cuda() if n else torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        tab0 = tab.array.copy()
        st0 = self.state.cpu().numpy()
        before = self.cache_state()
        if op == "assign":
            cache.write_rows(d_ids.data_ptr(), n, d_src.data_ptr(), "assign")
        elif op == "add":
            cache.write_rows(d_ids.data_ptr(), n, d_src.data_ptr(), "add", ALPHA)
        else:
            cache.adagrad_rows(d_ids.data_ptr(), n, d_src.data_ptr(), self.state.data_ptr(), LR, EPS)
        torch.cuda.synchronize()
        what = f"{op} n={n}"
        # (c) the cache's books are untouched; rejected ids are counted
        after = self.cache_state()
        for k in range(4):
            assert np.array_equal(before[k], after[k]), f"{what}: cache table {k} changed"
        assert after[4][:2] == before[4][:2], f"{what}: hit / miss changed"
        assert after[4][2] == before[4][2] + n_bad, f"{what}: range_errors {before[4][2]} -> {after[4][2]}, {n_bad} bad ids"
        # (a) the touched rows hold the expected values
        got = tab.array[good]
        st1 = self.state.cpu().numpy()
        if op == "assign":
            assert got.tobytes() == src[gpos].tobytes(), f"{what}: assigned rows differ"
        elif op == "add":
            check_add(got, tab0[good], src[gpos], ALPHA, what)
        else:
            check_adagrad(got, st1[good], tab0[good], st0[good], src[gpos], LR, EPS, what)
        # (b) every other row of table and state is byte-identical
        rest = np.ones(self.rows, dtype=bool)
        rest[good] = False
        assert tab.array[rest].tobytes() == tab0[rest].tobytes(), f"{what}: a row that was not named changed"
        if op == "adagrad":
            assert st1[rest].tobytes() == st0[rest].tobytes(), f"{what}: a state row that was not named changed"
        else:
            assert st1.tobytes() == st0.tobytes(), f"{what}: the state changed"
        # (d), (e) line == cold row: a read of the touched ids, their neighbours and the hot set returns the table's bytes
        back = np.unique(np.concatenate([good, np.clip(good + 1, 0, self.rows - 1), np.clip(good - 1, 0, self.rows - 1), hot]))
        assert self.read(back).tobytes() == tab.array[back].tobytes(), f"{what}: a read after the write does not return the table"
        if tab.offset:
            assert tab.guards_intact()


@pytest.mark.parametrize("dim,cache_mb,num_rows", [(1024, 1, 6000), (128, 1, 20000), (100, 1, 20000), (99, 1, 4000), (1, 1, 3000)])
@pytest.mark.parametrize("tag64", [False, True], ids=["tags32", "tags64"])
def test_writes_reach_cold_row_and_lines_and_nothing_else(hiplib, torch_cuda, tmp_path, dim, cache_mb, num_rows, tag64):
    rig = Rig(torch_cuda, hiplib, tmp_path, dim, cache_mb, num_rows, tag64=tag64, seed=dim)
    hot = rig.rng.choice(num_rows, size=200, replace=False).astype(np.int64)
    rig.read(hot)
    for n in (0, 1, 63, 64, 65, 1000):
        for op in ("assign", "add", "adagrad"):
            ids, n_bad = rig.mixed_ids(n, hot)
            rig.call_and_check(op, ids, n_bad, hot)
    hit, miss, _ = rig.cache.stats()
    assert hit > 0 and miss > 0          # the reads behind the writes both hit and missed
    rig.close()


@pytest.mark.parametrize("dim,table_off,buf_off", [(100, 1, 0), (128, 1, 0), (128, 0, 1), (100, 0, 1), (128, 0, 0)],
                         ids=["d100-table+1", "d128-table+1", "d128-bufs+1", "d100-bufs+1", "d128-guarded"])
def test_misaligned_table_and_buffers_take_the_scalar_path(hiplib, torch_cuda, tmp_path, dim, table_off, buf_off):
    """The table, or src / grad and the state, one float off 16-byte alignment; guards around the table stay intact, pad floats of the
    128-float lines (dim 100) cannot be seen, so the neighbours' reads cover them."""
    rig = Rig(torch_cuda, hiplib, tmp_path, dim, 1, 5000, table_off=table_off, buf_off=buf_off, seed=3)
    hot = rig.rng.choice(5000, size=200, replace=False).astype(np.int64)
    rig.read(hot)
    for n in (1, 65, 300):
        for op in ("assign", "add", "adagrad"):
            ids, n_bad = rig.mixed_ids(n, hot)
            rig.call_and_check(op, ids, n_bad, hot)
    assert rig.table.guards_intact()
    rig.close()


@pytest.mark.parametrize("op", ["assign", "adagrad"])
@pytest.mark.parametrize("tag64", [False, True], ids=["tags32", "tags64"])
def test_every_copy_of_a_tag_is_written(hiplib, torch_cuda, tmp_path, op, tag64):
    """A batch with a repeated miss leaves the id in several ways of its set; reads take the lowest.  A write must reach them all: once
    round robin has evicted the lowest copy, the next one is what a read returns."""
    torch = torch_cuda
    rig = Rig(torch, hiplib, tmp_path, 1024, 1, 4000, tag64=tag64, seed=9)
    cache = rig.cache
    assert cache.geometry().num_sets == 8
    rig.read([5, 5, 5])
    keys, cnt, _ = cache.dump()
    ways = np.flatnonzero(keys[5] == 5)
    c = int(ways[0])
    assert list(ways) == [c, c + 1, c + 2]
    ids = np.array([5], dtype=np.int64)
    src = make_grad(rig.rng, (1, 1024))
    d_src, d_ids = torch.from_numpy(src).cuda(), torch.from_numpy(ids).cuda()
    row0, st0 = rig.table.array[5].copy(), rig.state[5].cpu().numpy()
    if op == "assign":
        cache.write_rows(d_ids.data_ptr(), 1, d_src.data_ptr(), "assign")
    else:
        cache.adagrad_rows(d_ids.data_ptr(), 1, d_src.data_ptr(), rig.state.data_ptr(), LR, EPS)
    torch.cuda.synchronize()
    if op == "assign":
        assert rig.table.array[5].tobytes() == src[0].tobytes()
    else:
        check_adagrad(rig.table.array[5], rig.state[5].cpu().numpy(), row0, st0, src[0], LR, EPS, "adagrad of a triple copy")
    fresh = 8 * np.arange(1, 31, dtype=np.int64) + 5           # 30 more rows of set 5: round robin passes way c
    assert rig.read(fresh).tobytes() == rig.table.array[fresh].tobytes()
    keys, _, _ = cache.dump()
    assert keys[5, c] != 5 and keys[5, c + 1] == 5
    hit0, miss0, _ = cache.stats()
    got = rig.read([5])
    hit1, miss1, _ = cache.stats()
    assert (hit1, miss1) == (hit0 + 1, miss0), "the read of id 5 did not hit its second copy"
    assert got[0].tobytes() == rig.table.array[5].tobytes(), "the second copy of the id still holds the old row"
    rig.close()


def test_refusals_leave_the_handle_usable(hiplib, torch_cuda, tmp_path):
    torch, P = torch_cuda, hiplib
    rig = Rig(torch, P, tmp_path, 128, 1, 2000, seed=4)
    cache, dim = rig.cache, 128
    ids = torch.arange(10, 42, device="cuda", dtype=torch.int64)
    src = torch.from_numpy(make_grad(rig.rng, (32, dim))).cuda()
    out = torch.empty((32, dim), dtype=torch.float32, device="cuda")

    def good_write():
        cache.write_rows(ids.data_ptr(), 32, src.data_ptr(), "assign")
        torch.cuda.synchronize()
        assert rig.table.array[10:42].tobytes() == src.cpu().numpy().tobytes()
        assert rig.read(np.arange(10, 42)).tobytes() == rig.table.array[10:42].tobytes()

    cache.serve_probe(out.data_ptr(), ids.data_ptr(), 32)                      # an open serve batch
    with pytest.raises(RuntimeError, match="still open"):
        cache.write_rows(ids.data_ptr(), 32, src.data_ptr(), "assign")
    with pytest.raises(RuntimeError, match="still open"):
        cache.adagrad_rows(ids.data_ptr(), 32, src.data_ptr(), rig.state.data_ptr(), LR)
    cache.serve_abort()
    good_write()
    with pytest.raises(RuntimeError, match="mode 7"):
        cache.write_rows(ids.data_ptr(), 32, src.data_ptr(), 7)
    with pytest.raises(ValueError):
        cache.write_rows(ids.data_ptr(), 32, src.data_ptr(), "swap")
    with pytest.raises(RuntimeError, match="null buffer"):
        cache.write_rows(ids.data_ptr(), 32, 0, "assign")
    with pytest.raises(RuntimeError, match="null buffer"):
        cache.write_rows(0, 32, src.data_ptr(), "add", 2.0)
    with pytest.raises(RuntimeError, match="null buffer"):
        cache.adagrad_rows(ids.data_ptr(), 32, src.data_ptr(), 0, LR)
    with pytest.raises(RuntimeError, match="out of range"):
        cache.write_rows(ids.data_ptr(), -1, src.data_ptr(), "assign")
    with pytest.raises(RuntimeError, match="out of range"):
        cache.write_rows(ids.data_ptr(), 1 << 31, src.data_ptr(), "assign")
    cache.write_rows(0, 0, 0, "assign")                                         # n == 0: nothing to do, nothing to check
    src.neg_()
    good_write()
    ctrl = P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, dim, True)
    two = P.Isolated_Cache(ctrl, None, 0, 2, 1, rig.table.device_ptr, num_rows=2000)             # one of two caches over the table
    dist = P.SSD_GNN_NVSHMEM_Cache(ctrl, None, 0, 1, 1, rig.table.device_ptr, num_rows=2000)     # the distributed set index
    for other in (two, dist):
        with pytest.raises(RuntimeError, match="isolated cache of one GPU"):
            other.write_rows(ids.data_ptr(), 32, src.data_ptr(), "assign")
        with pytest.raises(RuntimeError, match="isolated cache of one GPU"):
            other.adagrad_rows(ids.data_ptr(), 32, src.data_ptr(), rig.state.data_ptr(), LR)
        other.serve(out.data_ptr(), ids.data_ptr(), 32)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == rig.table.array[10:42].tobytes()
        other.close()
    rig.close()


def test_a_read_on_another_stream_sees_the_write(hiplib, torch_cuda, tmp_path):
    """A write on stream A, then a read on stream B with no host synchronisation in between: the handle's program order holds."""
    torch = torch_cuda
    dim, num_rows, n = 256, 1 << 15, 1 << 14
    rig = Rig(torch, hiplib, tmp_path, dim, 8, num_rows, seed=6, sync=False)
    cache = rig.cache
    ids = torch.randperm(num_rows, generator=torch.Generator().manual_seed(1))[:n].cuda()
    out = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    cache.read_feature(out.data_ptr(), ids.data_ptr(), n)        # half of what fits is cached now
    torch.cuda.synchronize()
    for k in range(3):
        src = torch.full((n, dim), float(k + 1), dtype=torch.float32, device="cuda") + ids[:, None].float()
        torch.cuda.synchronize()
        with torch.cuda.stream(a):
            cache.write_rows(ids.data_ptr(), n, src.data_ptr(), "assign")
        with torch.cuda.stream(b):
            cache.read_feature(out.data_ptr(), ids.data_ptr(), n)
        torch.cuda.synchronize()
        assert torch.equal(out, src), f"round {k}: the read did not see the write"
        assert torch.equal(torch.from_numpy(rig.table.array)[ids.cpu()], src.cpu())
    rig.close()
