"""Ragged (CSR) block layouts in which one wave of a block-op kernel takes several unlike rows, one after the other (tests only, numpy).

Every kernel of coala_block_ops.hip deals destination rows to waves by wave_rows(): a wave takes row w, then w + n_waves, then
w + 2 n_waves, and keeps state in LDS and registers between them (the online softmax's max and sum, the backward's per-head sums, the
first chunk of a row).  A layout made here puts, into the rows that the first `busy` waves take, a fixed table of degrees in which
every change of kind that such state has to survive happens from one row of a wave to its next; every other row is small and random.

The dealing rule, restated from the launch code:
  row_grid launches                 n_waves = 4 * min(ceil(n_dst / 4), 8192)
  gatv2 backward with a partials    n_waves = 4 * parts for H * D <= 1024 (four waves a block), parts above (one wave a block)
  buffer of `parts` rows

A row's kind: empty, one chunk (1..64 slots) or many chunks (65 and more).  Wave w starts at sequence (4 w) mod 7 of SEQUENCES and walks
on through the table, one degree per turn, so seven consecutive waves start at seven different sequences and a wave of many turns
passes all of them.  What the table holds as consecutive rows of one wave is listed in REQUIRED."""
import numpy as np

EMPTY, ONE, MANY = 0, 1, 2
KIND_NAMES = ("empty", "one-chunk", "many-chunk")

SEQUENCES = ((0, 130, 0, 1), (130, 0, 130, 64), (64, 65, 64, 65), (1, 129, 1, 0), (128, 3, 0, 70), (200, 70, 1, 130), (0, 0, 1, 200))
_FLAT = np.array([d for s in SEQUENCES for d in s], dtype=np.int64)
_START = 16                         # wave w starts at _FLAT[16 w mod 28]: sequence 4 w mod 7

LAST = ("last:empty", "last:one-chunk", "last:many-chunk")
REQUIRED = ("many-chunk->empty", "empty->many-chunk", "many-chunk->1", "1->many-chunk", "64->65", "65->64", "128->3", "200->70",
            "empty->empty->1") + LAST

# the sizes tests/test_block_ops_rows_gpu.py uses: (n_dst, n_waves or None for the row grid, busy or None for every wave)
ROW_GRID_N_DST = 3 * 32768 + 5      # every wave of the capped grid takes three rows, five take four
ROW_GRID_BUSY = 512
PARTS = 2
PARTS_N_DST = 4 * (4 * PARTS) + 3   # four waves a block: every wave takes four rows, three take five
DEFAULT_PARTS_N_DST = 5000          # 1024 blocks of about five rows: 904 of the 4096 waves take a second row


def row_grid_waves(n_dst):
    return 4 * min(-(-n_dst // 4), 8192)


def partials_waves(parts, hd):
    return 4 * parts if hd <= 1024 else parts


def deal(n_dst, n_waves):
    """-> per wave (those that take a row at all), the rows it takes, in order"""
    return [np.arange(w, n_dst, n_waves) for w in range(min(n_waves, n_dst))]


def kinds(deg):
    deg = np.asarray(deg)
    return np.where(deg == 0, EMPTY, np.where(deg <= 64, ONE, MANY))


def transition_degrees(n_dst, n_waves, rng, busy=None):
    """A degree per row: the rows of the first `busy` waves (None: of every wave) follow the table, every other row gets 0..3."""
    deg = rng.integers(0, 4, size=n_dst).astype(np.int64)
    d = np.arange(n_dst)
    w, t = d % n_waves, d // n_waves
    on = w < (n_waves if busy is None else busy)
    deg[on] = _FLAT[(_START * w[on] + t[on]) % len(_FLAT)]
    return deg


def missing_transitions(deg, n_waves):
    """The names of REQUIRED that no wave has among its consecutive rows (the last three: as its last row)."""
    deg = np.asarray(deg)
    n = len(deg)
    a, b = deg[: max(n - n_waves, 0)], deg[n_waves:]
    ka, kb = kinds(a), kinds(b)
    c0, c1, c2 = deg[: max(n - 2 * n_waves, 0)], deg[n_waves: max(n - n_waves, n_waves)], deg[2 * n_waves:]
    last = kinds(deg[max(n - n_waves, 0):])
    have = {
        "many-chunk->empty": np.any((ka == MANY) & (kb == EMPTY)), "empty->many-chunk": np.any((ka == EMPTY) & (kb == MANY)),
        "many-chunk->1": np.any((ka == MANY) & (b == 1)), "1->many-chunk": np.any((a == 1) & (kb == MANY)),
        "64->65": np.any((a == 64) & (b == 65)), "65->64": np.any((a == 65) & (b == 64)), "128->3": np.any((a == 128) & (b == 3)),
        "200->70": np.any((a == 200) & (b == 70)), "empty->empty->1": np.any((c0 == 0) & (c1 == 0) & (c2 == 1)),
    }
    for k, name in zip((EMPTY, ONE, MANY), LAST):
        have[name] = np.any(last == k)
    return [name for name in REQUIRED if not have[name]]


def assert_transitions(deg, n_waves, allow=()):
    """Raises unless every transition of REQUIRED occurs in some wave.  allow: the names a layout cannot hold (too few turns, or fewer
    than three waves for the three kinds of last row): exactly these must be missing, so that a layout that grows gives them up."""
    missing = missing_transitions(deg, n_waves)
    assert sorted(missing) == sorted(allow), f"the layout lacks {sorted(set(missing) - set(allow))} and has {sorted(set(allow) - set(missing))}, listed as impossible"


def _busy_rows(n_dst, n_waves, busy):
    return [r for r in deal(n_dst, n_waves)[: n_waves if busy is None else busy]]


def transition_types(deg, n_waves, R, rng, busy=None, srt=False):
    """int32 slot types for the typed ops, flat in CSR order.  In a busy wave a row of turn t draws from the relations r = t mod 2 (mod 2),
    so consecutive rows of a wave share no relation: whatever is present in one row is absent from the next, and the converse.  Where
    the wave's first row has an edge and its second at least R, the first carries relation R - 1 alone and the second spreads over all
    R.  Every other row draws from [0, R), about 5 % of its slots outside (-1, R).  srt: sorted within a row, as the typed sampler
    gives them."""
    assert R >= 2, "one relation cannot come and go"
    deg = np.asarray(deg)
    n_dst = len(deg)
    indptr = np.concatenate([[0], np.cumsum(deg)])
    types = rng.integers(0, R, size=int(indptr[-1])).astype(np.int32)
    wild = rng.random(types.shape) < 0.05
    types[wild] = rng.choice(np.array([-1, R], dtype=np.int32), size=int(wild.sum()))
    for rows in _busy_rows(n_dst, n_waves, busy):
        special = len(rows) >= 2 and deg[rows[0]] >= 1 and deg[rows[1]] >= R
        for t, d in enumerate(rows):
            k = int(deg[d])
            if special and t == 0:
                row = np.full(k, R - 1)
            elif special and t == 1:
                row = rng.permutation(np.arange(k) % R)
            else:
                row = rng.choice(np.arange(t % 2, R, 2), size=k)
            types[indptr[d]: indptr[d + 1]] = row
    if srt:
        types = types[np.lexsort((types, np.repeat(np.arange(n_dst), deg)))]
    return types


def assert_type_transitions(deg, types, n_waves, R, busy=None):
    """Raises unless, in every busy wave, a relation present in one row is absent from the next wherever a row with an edge has a next
    row, and a relation absent from one row is present in the next wherever a row with an edge has a previous one; and unless some wave
    has a row of one relation alone followed by a row that holds all R."""
    deg = np.asarray(deg)
    indptr = np.concatenate([[0], np.cumsum(deg)])
    single_then_all = False
    for w, rows in enumerate(_busy_rows(len(deg), n_waves, busy)):
        sets = []
        for d in rows:
            t = types[indptr[d]: indptr[d + 1]]
            sets.append(set(int(x) for x in t[(t >= 0) & (t < R)]))
        loss = any(a - b for a, b in zip(sets, sets[1:]))
        gain = any(b - a for a, b in zip(sets, sets[1:]))
        assert loss or not any(sets[:-1]), f"wave {w}: no relation present in one row is absent from the next"
        assert gain or not any(sets[1:]), f"wave {w}: no relation absent from one row is present in the next"
        single_then_all |= any(len(a) == 1 and len(b) == R for a, b in zip(sets, sets[1:]))
    assert single_then_all, "no row of one relation is followed by a row that holds all of them"
