"""GPU tests of coala_cache_adam_rows / coala_cache_rowwise_adagrad_rows through Isolated_Cache, the way tests/test_cache_write_gpu.py
tests the other write-through updates (its Rig is reused): touched rows and touched state within the bounds of tests/_optim_ref.py, every
other row of the table and of every state table byte-identical, the step counters exactly +1, the cache's books untouched, rejected ids
counted, and a read afterwards returning the table's bytes."""
import numpy as np
import pytest

from _optim_ref import (INT32_MAX, adam_ref, check_adam, check_rowwise_adagrad, make_grad, make_signed_state, make_state, make_steps,
                        rowwise_additions)
from test_cache_write_gpu import Rig, _off_tensor

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, RW_EPS = 0.05, (0.9, 0.999), 1e-8, 1e-10
OPS = ("adam", "rowwise")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


class OptRig(Rig):
    """Rig plus Adam's state (m signed, v = the Rig's positive state, int32 steps drawn from PRIOR_STEPS) and the row-wise state."""

    def __init__(self, torch, P, tmp_path, dim, cache_mb, num_rows, fresh=False, **kw):
        super().__init__(torch, P, tmp_path, dim, cache_mb, num_rows, **kw)
        off = self.buf_off
        self.vec4 = dim % 4 == 0 and not self.table.offset and not off          # the 16-byte path (a table offset is 1 float or none)
        self.m = _off_tensor(torch, make_signed_state(self.rng, (num_rows, dim)), off)
        self.v = self.state
        self.steps = torch.from_numpy(make_steps(self.rng, num_rows)).cuda()
        self.row_state = _off_tensor(torch, make_state(self.rng, (num_rows,)), off)
        if fresh:
            for t in (self.m, self.v, self.steps, self.row_state):
                t.zero_()

    def states(self):
        self.torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in (self.m, self.v, self.steps, self.row_state))

    def call(self, op, d_ids, n, d_src, betas=BETAS, row_step=True, step=0, lr=LR):
        if op == "adam":
            self.cache.adam_rows(d_ids.data_ptr(), n, d_src.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), lr, betas, EPS,
                                 row_step_ptr=self.steps.data_ptr() if row_step else 0, step=step)
        else:
            self.cache.rowwise_adagrad_rows(d_ids.data_ptr(), n, d_src.data_ptr(), self.row_state.data_ptr(), lr, RW_EPS)

    def step_and_check(self, op, ids, n_bad, hot, src=None, what=None, **kw):
        """One call of `op`, then checks (a)-(e) of Rig.call_and_check against the references.  -> (good ids, their positions)"""
        torch, tab = self.torch, self.table
        n = len(ids)
        ok = (ids >= 0) & (ids < self.rows)
        good, gpos = ids[ok], np.flatnonzero(ok)
        if src is None:
            src = make_grad(self.rng, (max(n, 1), self.dim))
        d_src = _off_tensor(torch, src, self.buf_off)
        d_ids = torch.from_numpy(ids).cuda() if n else torch.zeros(1, dtype=torch.int64, device="cuda")
        tab0 = tab.array.copy()
        m0, v0, t0, s0 = self.states()
        before = self.cache_state()
        self.call(op, d_ids, n, d_src, **kw)
        m1, v1, t1, s1 = self.states()
        what = what or f"{op} dim={self.dim} n={n}"
        # (c) the cache's books are untouched; rejected ids are counted
        after = self.cache_state()
        for k in range(4):
            assert np.array_equal(before[k], after[k]), f"{what}: cache table {k} changed"
        assert after[4][:2] == before[4][:2], f"{what}: hit / miss changed"
        assert after[4][2] == before[4][2] + n_bad, f"{what}: range_errors {before[4][2]} -> {after[4][2]}, {n_bad} bad ids"
        # (a) the touched rows and the touched state hold the expected values
        got = tab.array[good]
        if op == "adam":
            betas = kw.get("betas", BETAS)
            if kw.get("row_step", True):
                t = np.minimum(t0[good].astype(np.int64) + 1, INT32_MAX)
                assert np.array_equal(t1[good], t), f"{what}: a touched row's step is not its old step + 1"
            else:
                t = kw["step"]
                assert np.array_equal(t1, t0), f"{what}: the step vector changed in a call that was not given one"
            check_adam(got, m1[good], v1[good], tab0[good], m0[good], v0[good], t, src[gpos], kw.get("lr", LR), betas[0], betas[1], EPS, what)
            assert s1.tobytes() == s0.tobytes(), f"{what}: the row-wise state changed"
        else:
            check_rowwise_adagrad(got, s1[good], tab0[good], s0[good], src[gpos], LR, RW_EPS, rowwise_additions(self.dim, self.vec4), what)
            assert m1.tobytes() == m0.tobytes() and v1.tobytes() == v0.tobytes() and t1.tobytes() == t0.tobytes(), f"{what}: Adam's state changed"
        # (b) every other row of the table and of every state table is byte-identical
        rest = np.ones(self.rows, dtype=bool)
        rest[good] = False
        assert tab.array[rest].tobytes() == tab0[rest].tobytes(), f"{what}: a row that was not named changed"
        for name, a, b in (("m", m1, m0), ("v", v1, v0), ("step", t1, t0), ("row state", s1, s0)):
            assert a[rest].tobytes() == b[rest].tobytes(), f"{what}: {name} of a row that was not named changed"
        # (d), (e) line == cold row: a read of the touched ids, their neighbours and the hot set returns the table's bytes
        back = np.unique(np.concatenate([good, np.clip(good + 1, 0, self.rows - 1), np.clip(good - 1, 0, self.rows - 1), hot]))
        assert self.read(back).tobytes() == tab.array[back].tobytes(), f"{what}: a read after the update does not return the table"
        if tab.offset:
            assert tab.guards_intact()
        return good, gpos


@pytest.mark.parametrize("dim,cache_mb,num_rows", [(1024, 1, 6000), (128, 1, 20000), (100, 1, 20000), (99, 1, 4000), (1, 1, 3000)])
@pytest.mark.parametrize("tag64", [False, True], ids=["tags32", "tags64"])
def test_updates_reach_cold_row_lines_and_state_and_nothing_else(hiplib, torch_cuda, tmp_path, dim, cache_mb, num_rows, tag64):
    rig = OptRig(torch_cuda, hiplib, tmp_path, dim, cache_mb, num_rows, tag64=tag64, seed=dim)
    hot = rig.rng.choice(num_rows, size=200, replace=False).astype(np.int64)
    rig.read(hot)
    for n in (0, 1, 63, 64, 65, 1000):
        for op in OPS:
            ids, n_bad = rig.mixed_ids(n, hot)
            rig.step_and_check(op, ids, n_bad, hot)
    hit, miss, _ = rig.cache.stats()
    assert hit > 0 and miss > 0
    rig.close()


@pytest.mark.parametrize("dim,table_off,buf_off", [(100, 1, 0), (128, 1, 0), (128, 0, 1), (100, 0, 1)],
                         ids=["d100-table+1", "d128-table+1", "d128-bufs+1", "d100-bufs+1"])
def test_misaligned_table_buffers_and_states_take_the_scalar_path(hiplib, torch_cuda, tmp_path, dim, table_off, buf_off):
    """The table, or grad and every state table, one float off 16-byte alignment; the guards around the table stay intact."""
    rig = OptRig(torch_cuda, hiplib, tmp_path, dim, 1, 5000, table_off=table_off, buf_off=buf_off, seed=3)
    assert not rig.vec4
    hot = rig.rng.choice(5000, size=200, replace=False).astype(np.int64)
    rig.read(hot)
    for n in (1, 65, 300):
        for op in OPS:
            ids, n_bad = rig.mixed_ids(n, hot)
            rig.step_and_check(op, ids, n_bad, hot)
    assert rig.table.guards_intact()
    rig.close()


@pytest.mark.parametrize("tag64", [False, True], ids=["tags32", "tags64"])
def test_rowwise_sum_stays_inside_its_half_wave(hiplib, torch_cuda, tmp_path, tag64):
    """dim 128 on the 16-byte path: two rows per wave pass, one per half-wave.  A rejected id next to a good one (either way round) is
    a dead half next to a live one; then two live rows whose gradients differ by 10^4, so that a sum that leaked across the halves
    would put the small row's state off by a factor of 10^8."""
    rig = OptRig(torch_cuda, hiplib, tmp_path, 128, 1, 5000, tag64=tag64, seed=11)
    assert rig.vec4
    hot = rig.rng.choice(5000, size=200, replace=False).astype(np.int64)
    rig.read(hot)
    outside = 5000 + 17
    for k, good in enumerate((int(hot[0]), int(np.setdiff1d(np.arange(5000), hot)[5]))):      # a cached row, a cold row
        rig.step_and_check("rowwise", np.array([good, outside], dtype=np.int64), 1, hot, what=f"[good, outside] {k}")
        rig.step_and_check("rowwise", np.array([outside, good], dtype=np.int64), 1, hot, what=f"[outside, good] {k}")
        rig.step_and_check("rowwise", np.array([outside, (good + 1) % 5000], dtype=np.int64), 1, hot, what=f"[outside, good + 1] {k}")
    pair = np.array([int(hot[1]), int(hot[2])], dtype=np.int64)
    src = make_grad(rig.rng, (2, 128))
    src = (np.sign(src) * np.abs(src) ** 0.1).astype(np.float32)               # magnitudes within [0.4, 1.6] ...
    src[0] *= np.float32(1e2)                                                   # ... then 10^4 apart
    src[1] *= np.float32(1e-2)
    for order in (pair, pair[::-1].copy()):
        rig.row_state[torch_cuda.from_numpy(pair).cuda()] = 0.0
        rig.step_and_check("rowwise", order, 0, hot, src=src if order is pair else src[::-1].copy(), what="two live rows, 10^4 apart")
    rig.close()


@pytest.mark.parametrize("dim", [1024, 128, 99])
def test_rowwise_state_is_bitwise_reproducible(hiplib, torch_cuda, tmp_path, dim):
    """Two runs from the same snapshot: the same bits in the row state and in the rows."""
    torch = torch_cuda
    rig = OptRig(torch, hiplib, tmp_path, dim, 1, 4000, seed=13)
    hot = rig.rng.choice(4000, size=200, replace=False).astype(np.int64)
    rig.read(hot)
    ids, _ = rig.mixed_ids(600, hot)
    good = ids[ids < 4000]
    src = make_grad(rig.rng, (600, dim))
    d_ids, d_src, d_good = torch.from_numpy(ids).cuda(), torch.from_numpy(src).cuda(), torch.from_numpy(good).cuda()
    rows0 = torch.from_numpy(rig.table.array[good]).cuda()
    s0 = rig.row_state.clone()
    results = []
    for run in range(2):
        rig.cache.write_rows(d_good.data_ptr(), len(good), rows0.data_ptr(), "assign")          # cold rows and lines back to the snapshot
        rig.row_state.copy_(s0)
        rig.call("rowwise", d_ids, 600, d_src)
        torch.cuda.synchronize()
        results.append((rig.row_state.cpu().numpy().tobytes(), rig.table.array[good].tobytes()))
    assert results[0][0] == results[1][0], "the row state differs between two runs from the same snapshot"
    assert results[0][1] == results[1][1]
    assert results[0][0] != s0.cpu().numpy().tobytes()
    rig.close()


@pytest.mark.parametrize("beta2", [0.999, 0.9999])
def test_adam_first_steps_of_fresh_rows(hiplib, torch_cuda, tmp_path, beta2):
    """Fresh rows (m = v = 0, step 0): t = 1, where upd is lr sign(g) up to eps / |g|, then the same rows again at t = 2, the first step
    at which 1 - beta2 ** t formed in fp32 is outside the bound (test_embedding_optim_cpu.py holds the reference to both facts)."""
    rig = OptRig(torch_cuda, hiplib, tmp_path, 128, 1, 5000, fresh=True, seed=17)
    hot = rig.rng.choice(5000, size=200, replace=False).astype(np.int64)
    rig.read(hot)
    ids, n_bad = rig.mixed_ids(300, hot)
    src = make_grad(rig.rng, (300, 128))
    z = np.zeros((300, 128), dtype=np.float32)
    _, _, _, upd = adam_ref(z, z, z, 1, src, LR, 0.9, beta2, EPS)
    assert np.all(np.sign(upd) == np.sign(src)) and np.all(np.abs(np.abs(upd) / np.float64(np.float32(LR)) - 1.0) < 2e-4)
    for t in (1, 2):
        good, _ = rig.step_and_check("adam", ids, n_bad, hot, src=src if t == 1 else None, betas=(0.9, beta2), what=f"fresh rows, beta2={beta2}, t={t}")
        assert np.all(rig.steps.cpu().numpy()[good] == t)
    rig.close()


def test_adam_with_the_callers_step_and_with_a_saturated_counter(hiplib, torch_cuda, tmp_path):
    rig = OptRig(torch_cuda, hiplib, tmp_path, 128, 1, 5000, seed=19)
    hot = rig.rng.choice(5000, size=200, replace=False).astype(np.int64)
    rig.read(hot)
    for step in (1, 2, 1000):
        ids, n_bad = rig.mixed_ids(200, hot)
        rig.step_and_check("adam", ids, n_bad, hot, row_step=False, step=step, what=f"no step vector, step={step}")
    ids, n_bad = rig.mixed_ids(200, hot)
    good = ids[ids < 5000]
    rig.steps[torch_cuda.from_numpy(good[::2]).cuda()] = INT32_MAX
    rig.steps[torch_cuda.from_numpy(good[1::4]).cuda()] = INT32_MAX - 1
    rig.step_and_check("adam", ids, n_bad, hot, what="saturated counters")
    t = rig.steps.cpu().numpy()
    assert np.all(t[good[::2]] == INT32_MAX) and np.all(t[good[1::4]] == INT32_MAX)
    rig.close()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("tag64", [False, True], ids=["tags32", "tags64"])
def test_every_copy_of_a_tag_is_updated(hiplib, torch_cuda, tmp_path, op, tag64):
    """The triple-copy case of test_cache_write_gpu.py: an id in three ways of its set; the update must reach all of them."""
    rig = OptRig(torch_cuda, hiplib, tmp_path, 1024, 1, 4000, tag64=tag64, seed=9)
    cache = rig.cache
    assert cache.geometry().num_sets == 8
    rig.read([5, 5, 5])
    keys, _, _ = cache.dump()
    ways = np.flatnonzero(keys[5] == 5)
    c = int(ways[0])
    assert list(ways) == [c, c + 1, c + 2]
    rig.step_and_check(op, np.array([5], dtype=np.int64), 0, np.array([5], dtype=np.int64), what=f"{op} of a triple copy")
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
    rig = OptRig(torch, P, tmp_path, 128, 1, 2000, seed=4)
    cache, dim = rig.cache, 128
    hot = np.arange(10, 42, dtype=np.int64)
    ids = torch.from_numpy(hot).cuda()
    src = torch.from_numpy(make_grad(rig.rng, (32, dim))).cuda()
    out = torch.empty((32, dim), dtype=torch.float32, device="cuda")
    I, S, M, V, T, R = ids.data_ptr(), src.data_ptr(), rig.m.data_ptr(), rig.v.data_ptr(), rig.steps.data_ptr(), rig.row_state.data_ptr()
    snap = (rig.table.array.copy(),) + rig.states()

    def refused(match, adam=None, rowwise=None):
        if adam is not None:
            with pytest.raises(RuntimeError, match=match):
                cache.adam_rows(*adam[0], **adam[1])
        if rowwise is not None:
            with pytest.raises(RuntimeError, match=match):
                cache.rowwise_adagrad_rows(*rowwise)

    cache.serve_probe(out.data_ptr(), I, 32)                                                    # an open serve batch
    refused("still open", ((I, 32, S, M, V, LR), dict(row_step_ptr=T)), (I, 32, S, R, LR))
    cache.serve_abort()
    refused("out of range", ((I, -1, S, M, V, LR), dict(row_step_ptr=T)), (I, -1, S, R, LR))
    refused("out of range", ((I, 1 << 31, S, M, V, LR), dict(row_step_ptr=T)), (I, 1 << 31, S, R, LR))
    refused("null buffer", ((0, 32, S, M, V, LR), dict(row_step_ptr=T)), (0, 32, S, R, LR))
    refused("null buffer", ((I, 32, 0, M, V, LR), dict(row_step_ptr=T)), (I, 32, 0, R, LR))
    refused("null buffer", ((I, 32, S, 0, V, LR), dict(row_step_ptr=T)), (I, 32, S, 0, LR))
    refused("null buffer", ((I, 32, S, M, 0, LR), dict(row_step_ptr=T)))
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, float("nan"))):
        refused("betas", ((I, 32, S, M, V, LR), dict(betas=betas, row_step_ptr=T)))
    refused("step=0", ((I, 32, S, M, V, LR), dict(row_step_ptr=0, step=0)))
    refused("step=-3", ((I, 32, S, M, V, LR), dict(row_step_ptr=0, step=-3)))
    cache.adam_rows(0, 0, 0, 0, 0, LR, row_step_ptr=0, step=1)                                   # n == 0: nothing to do
    cache.rowwise_adagrad_rows(0, 0, 0, 0, LR)
    ctrl = P.SSD_GNN_SSD_Controllers(1, 4096, 1024, 0, 0, dim, True)
    two = P.Isolated_Cache(ctrl, None, 0, 2, 1, rig.table.device_ptr, num_rows=2000)             # one of two caches over the table
    dist = P.SSD_GNN_NVSHMEM_Cache(ctrl, None, 0, 1, 1, rig.table.device_ptr, num_rows=2000)     # the distributed set index
    for other in (two, dist):
        with pytest.raises(RuntimeError, match="isolated cache of one GPU"):
            other.adam_rows(I, 32, S, M, V, LR, row_step_ptr=T)
        with pytest.raises(RuntimeError, match="isolated cache of one GPU"):
            other.rowwise_adagrad_rows(I, 32, S, R, LR)
        other.close()
    torch.cuda.synchronize()
    now = (rig.table.array,) + rig.states()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(snap, now)), "a refused call changed the table or a state"
    for op in OPS:                                                                               # ... then a correct call
        rig.step_and_check(op, hot, 0, hot, what=f"{op} after the refusals")
    rig.close()


@pytest.mark.parametrize("op", OPS)
def test_a_read_on_another_stream_sees_the_update(hiplib, torch_cuda, tmp_path, op):
    """An update on stream A, then a read on stream B with no host synchronisation in between: the handle's program order holds."""
    torch = torch_cuda
    dim, num_rows, n = 256, 1 << 14, 1 << 13
    rig = OptRig(torch, hiplib, tmp_path, dim, 4, num_rows, seed=6, sync=False, fresh=True)
    cache = rig.cache
    ids = torch.randperm(num_rows, generator=torch.Generator().manual_seed(1))[:n].cuda()
    out = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    src = torch.from_numpy(make_grad(rig.rng, (n, dim))).cuda()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    cache.read_feature(out.data_ptr(), ids.data_ptr(), n)        # half of what fits is cached now
    torch.cuda.synchronize()
    before = out.clone()
    with torch.cuda.stream(a):
        rig.call(op, ids, n, src)
    with torch.cuda.stream(b):
        cache.read_feature(out.data_ptr(), ids.data_ptr(), n)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(rig.table.array)[ids.cpu()]), "the read did not see the update"
    assert not torch.equal(out, before)
    assert bool((out != before).any(dim=1).all()), "a row kept its old value"
    rig.close()
