"""The miss list between the two cache kernels: the probe appends every missed position to one of its sharded lists, and the cold
fill of a whole read on a host tier streams from those lists (miss_fill_list_kernel).  Every case compares rows, tag table, cursors,
colour tags and hit / miss / rejected counters with the CPU oracle, bit for bit, at the smallest shapes at which the list can go
wrong: around the group size R (4 rows of 4-KiB and 400-B lines, 8 of 512-B ones), around a probe block and a shard round, batches
with no / one / only misses, a set that overflows inside one batch, rejected ids, and the counters' generation parity."""
import numpy as np
import pytest

from _util import PinnedTable
from test_cache_gpu import _compare_tables, _make_cache, torch_cuda  # noqa: F401  (torch_cuda: the fixture)

pytestmark = pytest.mark.gpu


class _Pair:
    """A cache on a pinned-host table and its oracle, fed the same batches."""

    def __init__(self, P, oracle, torch, dim, num_rows, tag64=False, cache_mb=1, seed=5):
        self.P, self.oracle, self.torch = P, oracle, torch
        self.dim, self.num_rows = dim, num_rows
        self.feat = oracle.make_features(num_rows, dim, seed=seed)
        self.table = PinnedTable(P, self.feat)
        self.cache, _ = _make_cache(P, self.table, cache_mb, tag64=tag64)
        self.orc = oracle.OracleCache(cache_mb, dim, self.feat)
        self.bad = 0

    def device(self, idx):
        d_idx = self.torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).cuda()
        out = self.torch.full((len(idx), self.dim), -7.0, dtype=self.torch.float32, device="cuda")
        return d_idx, out

    def read(self, idx, check_hits=True):
        """One whole read on both sides; ids outside the table are zero rows, counted and otherwise left alone."""
        idx = np.asarray(idx, dtype=np.int64)
        d_idx, out = self.device(idx)
        self.cache.read_feature(out.data_ptr(), d_idx.data_ptr(), len(idx))
        ok = (idx >= 0) & (idx < self.num_rows)
        self.orc.read_feature(idx[ok], self.oracle.SCHED_HITS_FIRST)
        self.bad += int((~ok).sum())
        want = np.zeros((len(idx), self.dim), dtype=np.float32)
        want[ok] = self.feat[idx[ok]]
        assert out.cpu().numpy().tobytes() == want.tobytes(), f"row bytes differ at n={len(idx)}"
        hit, miss, bad = self.cache.stats()
        assert (miss, bad) == (self.orc.miss_cnt, self.bad), f"miss / rejected counters differ at n={len(idx)}"
        if check_hits:
            assert hit == self.orc.hit_cnt, f"hit counter differs at n={len(idx)}"
        _compare_tables(self.cache, self.orc)

    def close(self):
        self.cache.close()
        self.table.close()


# (dim, group size R): 16-byte accesses on whole 4-KiB lines, on 512-B lines (two rows per pass), and the scalar form on a partly used line
GEOS = [(1024, 4), (128, 8), (100, 4)]


@pytest.mark.parametrize("tag64", [False, True], ids=["tags32", "tags64"])
@pytest.mark.parametrize("dim,R", GEOS)
def test_batch_sizes_around_a_group(hiplib, oracle, torch_cuda, dim, R, tag64):
    num_rows = 6000
    pr = _Pair(hiplib, oracle, torch_cuda, dim, num_rows, tag64=tag64)
    assert pr.cache.geometry().tag_set_bytes == (256 if tag64 else 128)
    rng = np.random.default_rng(dim + tag64)
    fresh = iter(rng.permutation(num_rows))   # every id taken from here is a miss the first time
    take = lambda n: np.array([next(fresh) for _ in range(n)], dtype=np.int64)
    for n in (1, R - 1, R, R + 1, 63, 64, 65, 257):
        cold = take(n)
        pr.read(cold)                                   # every row a miss
        pr.read(cold[rng.permutation(n)])               # no miss (the cache holds 256+ lines): the fill leaves on the counters
        one = cold.copy()
        one[rng.integers(n)] = take(1)[0]
        pr.read(one)                                    # exactly one miss
        half = cold.copy()
        half[::2] = take(len(half[::2]))
        pr.read(half[rng.permutation(n)])               # misses and hits mixed inside the groups
    assert pr.orc.hit_cnt > 0 and pr.orc.miss_cnt > 0
    pr.close()


@pytest.mark.parametrize("tag64", [False, True], ids=["tags32", "tags64"])
def test_set_overflow_has_non_winners(hiplib, oracle, torch_cuda, tag64):
    """More than 32 misses of one set in one batch (8 sets x 32 ways, the smallest cache the interface makes at 4-KiB lines): the rows
    past the last 32 of the set are streamed but publish nothing.  A second batch on the same handle finds exactly the winners."""
    pr = _Pair(hiplib, oracle, torch_cuda, 1024, 4000, tag64=tag64)
    assert pr.cache.geometry().num_sets == 8
    set3 = np.arange(100, dtype=np.int64) * 8 + 3
    set5 = np.arange(40, dtype=np.int64) * 8 + 5
    rng = np.random.default_rng(2)
    pr.read(rng.permutation(np.concatenate([set3, set5, np.array([0, 1, 2], dtype=np.int64)])))
    pr.read(rng.permutation(np.concatenate([set3, set5])))        # the winners hit, the others miss again
    pr.read(set3[::-1].copy())
    assert pr.orc.hit_cnt > 0
    pr.close()


@pytest.mark.parametrize("dim", [1024, 128])
def test_rejected_ids_are_counted_and_not_streamed(hiplib, oracle, torch_cuda, dim):
    num_rows = 3000
    pr = _Pair(hiplib, oracle, torch_cuda, dim, num_rows)
    rng = np.random.default_rng(9)
    warm = rng.choice(num_rows, size=90, replace=False).astype(np.int64)
    pr.read(warm)
    bad = np.array([num_rows, -1, 2**40, num_rows + 7, 2**32 - 1, -2**40], dtype=np.int64)
    cold = np.setdiff1d(np.arange(num_rows), warm)[:70].astype(np.int64)
    for k in (1, 70):                                # one group with everything in it, then several
        idx = rng.permutation(np.concatenate([warm[:k], cold[:k], bad]))
        pr.read(idx)
        cold = cold[k:]
    pr.read(bad)                                     # nothing but rejected ids: an empty list
    assert pr.cache.stats()[2] == pr.bad == 3 * len(bad)
    assert pr.cache.stats(reset=True)[2] == pr.bad   # ... and the counters start again after a reset
    pr.orc.reset_stats()
    pr.bad = 0
    pr.read(np.concatenate([bad[:2], warm[:5]]))
    pr.close()


@pytest.mark.parametrize("abort", [False, True], ids=["plain", "probe_abort_between"])
def test_counter_parity_over_generations(hiplib, oracle, torch_cuda, abort):
    """Batches with N, 0 and M misses back to back: every probe clears the next generation's counters, and an empty batch must not
    stream the list its predecessor of the same parity left behind.  With a probed and abandoned batch between them the parities
    shift by one."""
    num_rows = 5000
    pr = _Pair(hiplib, oracle, torch_cuda, 1024, num_rows)
    rng = np.random.default_rng(4)
    ids = rng.permutation(num_rows).astype(np.int64)
    a, b, probe_only = ids[:150], ids[150:187], ids[1000:1090]

    def between():
        if abort:   # a probe alone keeps no list and fills nothing; its rows only count as looked up
            d_idx, out = pr.device(probe_only)
            pr.cache.serve_probe(out.data_ptr(), d_idx.data_ptr(), len(probe_only))
            pr.cache.serve_abort()

    pr.read(a, check_hits=not abort)                 # N misses
    between()
    pr.read(a[::-1].copy(), check_hits=not abort)    # 0 misses: same parity as the batch before the last one when nothing comes between
    between()
    pr.read(np.concatenate([b, a[:20]]), check_hits=not abort)   # M misses
    pr.read(a[:7], check_hits=not abort)             # 0 again, the other parity
    pr.read(b[::-1].copy(), check_hits=not abort)
    pr.close()


@pytest.mark.parametrize("dim,n_miss", [(1024, 401), (128, 2051)])
def test_more_groups_than_waves(hiplib, oracle, torch_cuda, dim, n_miss):
    """A list longer than the fill's waves x R (24 blocks x 4 waves x 4 rows = 384 at 4-KiB lines, 64 x 4 x 8 = 2048 at 512-B ones) and
    no multiple of R: the later groups come from the ticket counter and the last one is short."""
    num_rows = 9000
    pr = _Pair(hiplib, oracle, torch_cuda, dim, num_rows, cache_mb=8 if dim == 1024 else 2)
    rng = np.random.default_rng(n_miss)
    ids = rng.permutation(num_rows).astype(np.int64)
    warm = ids[:300]
    pr.read(warm)
    pr.read(rng.permutation(np.concatenate([warm, ids[300:300 + n_miss]])))
    pr.read(ids[4000:4000 + n_miss])                 # nothing but misses
    pr.close()
