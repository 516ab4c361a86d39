"""CPU tests of tests/_row_layouts.py: the layouts tests/test_block_ops_rows_gpu.py runs on meet their own assertions at the sizes
used there, the dealing rule covers every row once, and the assertion helpers refuse a layout with a transition taken out -- so a
later edit of the table cannot leave the GPU file passing on rows that are all alike."""
import numpy as np
import pytest

import _row_layouts as RL

# (n_dst, n_waves, busy, the transitions the size cannot hold)
SIZES = [
    (RL.ROW_GRID_N_DST, RL.row_grid_waves(RL.ROW_GRID_N_DST), RL.ROW_GRID_BUSY, ()),
    (RL.PARTS_N_DST, RL.partials_waves(RL.PARTS, 8), None, ()),
    # one wave a block: two waves have two last rows
    (RL.PARTS_N_DST, RL.partials_waves(RL.PARTS, 1040), None, ("last:empty",)),
    # two turns: nothing of three rows, and the table's sequences start with neither 65 -> 64 nor many-chunk -> 1
    (RL.DEFAULT_PARTS_N_DST, RL.partials_waves(1024, 64), RL.ROW_GRID_BUSY, ("65->64", "empty->empty->1", "many-chunk->1")),
]


def test_the_dealing_rule():
    assert RL.row_grid_waves(1) == 4 and RL.row_grid_waves(32768) == 32768 and RL.row_grid_waves(32769) == 32768
    assert RL.row_grid_waves(RL.ROW_GRID_N_DST) == 32768
    assert RL.partials_waves(2, 1024) == 8 and RL.partials_waves(2, 1025) == 2
    for n_dst, n_waves in ((0, 4), (3, 8), (35, 8), (35, 2), (RL.ROW_GRID_N_DST, 32768)):
        waves = RL.deal(n_dst, n_waves)
        rows = np.concatenate(waves) if waves else np.zeros(0, np.int64)
        assert np.array_equal(np.sort(rows), np.arange(n_dst)), "a row is dealt twice or not at all"
        assert all(np.all(np.diff(r) == n_waves) and r[0] == w for w, r in enumerate(waves))
    turns = np.array([len(r) for r in RL.deal(RL.ROW_GRID_N_DST, 32768)])
    assert np.all(turns[:5] == 4) and np.all(turns[5:] == 3)
    assert [len(r) for r in RL.deal(RL.PARTS_N_DST, 8)] == [5, 5, 5, 4, 4, 4, 4, 4]


def test_kinds():
    assert RL.kinds([0, 1, 64, 65, 200]).tolist() == [RL.EMPTY, RL.ONE, RL.ONE, RL.MANY, RL.MANY]


@pytest.mark.parametrize("n_dst,n_waves,busy,allow", SIZES)
def test_layouts_meet_their_assertions(n_dst, n_waves, busy, allow):
    rng = np.random.default_rng(n_dst + n_waves)
    deg = RL.transition_degrees(n_dst, n_waves, rng, busy)
    assert len(deg) == n_dst and deg.min() == 0 and deg.max() == 200
    RL.assert_transitions(deg, n_waves, allow)
    quiet = np.arange(n_dst) % n_waves >= (n_waves if busy is None else busy)
    assert np.all(deg[quiet] <= 3)
    if not allow:
        for R in (3, 16, 64):
            for srt in (False, True):
                t = RL.transition_types(deg, n_waves, R, rng, busy, srt)
                assert len(t) == deg.sum()
                RL.assert_type_transitions(deg, t, n_waves, R, busy)
                if srt:
                    indptr = np.concatenate([[0], np.cumsum(deg)])
                    inner = np.ones(len(t), bool)
                    inner[indptr[:-1][deg > 0]] = False
                    assert np.all(np.diff(t)[inner[1:]] >= 0)


def _without(deg, n_waves, name):
    """deg with every occurrence of one transition taken out"""
    deg = deg.copy()
    n = len(deg)
    k = RL.kinds(deg)
    if name.startswith("last:"):
        kind = RL.LAST.index(name)
        last = np.arange(max(n - n_waves, 0), n)
        deg[last[k[last] == kind]] = 65 if kind != RL.MANY else 2
        return deg
    a = np.arange(max(n - n_waves, 0))
    b = a + n_waves
    hit = {"many-chunk->empty": (k[a] == RL.MANY) & (k[b] == RL.EMPTY), "empty->many-chunk": (k[a] == RL.EMPTY) & (k[b] == RL.MANY),
           "many-chunk->1": (k[a] == RL.MANY) & (deg[b] == 1), "1->many-chunk": (deg[a] == 1) & (k[b] == RL.MANY),
           "64->65": (deg[a] == 64) & (deg[b] == 65), "65->64": (deg[a] == 65) & (deg[b] == 64), "128->3": (deg[a] == 128) & (deg[b] == 3),
           "200->70": (deg[a] == 200) & (deg[b] == 70), "empty->empty->1": (deg[a] == 0) & (deg[b] == 0)}[name]
    for i in np.flatnonzero(hit):                      # row by row: a row changed as `b` may be the next pair's `a`
        if name == "empty->empty->1":
            if a[i] + 2 * n_waves < n and deg[a[i]] == 0 and deg[b[i]] == 0 and deg[a[i] + 2 * n_waves] == 1:
                deg[b[i]] = 2
        else:
            deg[b[i]] = 2 if RL.kinds(deg[b[i]]) != RL.ONE or deg[b[i]] in (1, 3) else 7
    return deg


@pytest.mark.parametrize("name", RL.REQUIRED)
def test_a_layout_without_one_transition_is_refused(name):
    n_dst, n_waves = RL.PARTS_N_DST, 8
    deg = RL.transition_degrees(n_dst, n_waves, np.random.default_rng(1), None)
    RL.assert_transitions(deg, n_waves)
    bad = _without(deg, n_waves, name)
    assert name in RL.missing_transitions(bad, n_waves)
    with pytest.raises(AssertionError):
        RL.assert_transitions(bad, n_waves)


def test_uniform_rows_are_refused():
    """What the older CSR cases had: every long row of one degree."""
    n_waves = RL.row_grid_waves(RL.ROW_GRID_N_DST)
    deg = np.full(RL.ROW_GRID_N_DST, 2)
    deg[:: 20] = 130
    assert len(RL.missing_transitions(deg, n_waves)) >= 6
    with pytest.raises(AssertionError):
        RL.assert_transitions(deg, n_waves)
    with pytest.raises(AssertionError):                # an impossible transition that is there after all
        RL.assert_transitions(RL.transition_degrees(RL.PARTS_N_DST, 8, np.random.default_rng(0)), 8, allow=("64->65",))


def test_degenerate_types_are_refused():
    n_dst, n_waves, R = RL.PARTS_N_DST, 8, 3
    rng = np.random.default_rng(2)
    deg = RL.transition_degrees(n_dst, n_waves, rng)
    t = RL.transition_types(deg, n_waves, R, rng)
    RL.assert_type_transitions(deg, t, n_waves, R)
    with pytest.raises(AssertionError):                # one relation everywhere: nothing comes, nothing goes between rows with edges
        RL.assert_type_transitions(deg, np.zeros_like(t), n_waves, R)
    indptr = np.concatenate([[0], np.cumsum(deg)])
    spread = t.copy()
    for d in range(n_dst):                             # no row of one relation alone in front of a full one
        if deg[d] >= 2:
            spread[indptr[d]: indptr[d] + 2] = [0, 1] if (d // n_waves) % 2 == 0 else [1, 0]
    with pytest.raises(AssertionError):
        RL.assert_type_transitions(deg, spread, n_waves, R)
