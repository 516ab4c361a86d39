"""CPU tests of the helpers that COALA_GNN.sampler's edge-type and edge-time functions share: sort_csc_by_etype / sort_csc_by_time sort
the same way, check_etype_sorted / check_time_sorted draw the row boundaries the same way, each with its own words."""
import numpy as np
import pytest


def test_sort_by_etype_and_by_time_agree_on_the_same_key():
    import torch
    from COALA_GNN.sampler import sort_csc_by_etype, sort_csc_by_time
    rng = np.random.default_rng(5)
    deg = rng.integers(0, 40, size=300)
    deg[[0, 17, 299]] = 0
    ip = torch.from_numpy(np.concatenate([[0], np.cumsum(deg)]).astype(np.int64))
    E = int(ip[-1])
    ix = torch.from_numpy(rng.integers(0, 300, size=E).astype(np.int64))
    for dtype in (torch.int64, torch.int32, torch.uint8):
        key = torch.from_numpy(rng.integers(0, 7, size=E)).to(dtype)     # few values: every row holds ties, which must keep their order
        a, b = sort_csc_by_etype(ip, ix, key), sort_csc_by_time(ip, ix, key)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and torch.equal(x, y)
        s_ix, s_key, perm = a
        assert s_key.dtype == dtype and torch.equal(s_ix, ix[perm]) and torch.equal(s_key, key[perm])
        k = key.numpy().astype(np.int64)
        want = np.concatenate([lo + np.argsort(k[lo:hi], kind="stable") for lo, hi in zip(ip[:-1].tolist(), ip[1:].tolist())] or [np.zeros(0, np.int64)])
        assert np.array_equal(perm.numpy(), want)
    for fn, words in ((sort_csc_by_etype, "edge types"), (sort_csc_by_time, "edge times")):
        with pytest.raises(ValueError, match=f"{words} must have shape"):
            fn(ip, ix, key[:-1])
        with pytest.raises(ValueError, match=f"{words} must be an integer tensor"):
            fn(ip, ix, key.double())


# rows [0, 3), [3, 3) (empty), [3, 6), [6, 8): a key may fall exactly where a row starts, and nowhere else
_IP = [0, 3, 3, 6, 8]
_CASES = [
    ("sorted", [0, 1, 2, 0, 1, 2, 0, 2], True),
    ("drop exactly at a row start, behind the empty row", [1, 1, 2, 0, 0, 0, 0, 0], True),
    ("drop at the last row's start", [0, 0, 0, 1, 1, 2, 0, 1], True),
    ("drop at the last position of a row", [0, 2, 1, 1, 1, 1, 1, 1], False),
    ("drop at the last position of the row behind the empty one", [0, 0, 0, 0, 2, 1, 1, 1], False),
    ("drop at the last position of the last row", [0, 0, 0, 0, 0, 0, 2, 1], False),
    ("drop at a row's second position", [2, 0, 0, 0, 0, 0, 0, 0], False),
]


@pytest.mark.parametrize("what,key,ok", _CASES, ids=[c[0] for c in _CASES])
def test_both_checks_draw_the_same_row_boundaries(what, key, ok):
    import torch
    from COALA_GNN.sampler import check_etype_sorted, check_time_sorted
    ip, key = torch.tensor(_IP), torch.tensor(key)
    checks = ((lambda: check_etype_sorted(ip, key, 3, "rel"), r"edata\['rel'\]: edge types must be non-decreasing.*sort_csc_by_etype\(indptr, indices, etype\)"),
              (lambda: check_time_sorted(ip, key, "when"), r"edata\['when'\]: edge times must be non-decreasing.*sort_csc_by_time\(indptr, indices, ts\)"))
    for check, message in checks:
        if ok:
            check()
        else:
            with pytest.raises(ValueError, match=message):
                check()


def test_each_check_keeps_its_own_words():
    import torch
    from COALA_GNN.sampler import check_etype_sorted, check_time_sorted
    ip, key = torch.tensor(_IP), torch.tensor(_CASES[0][1])
    with pytest.raises(ValueError, match=r"edata\['etype'\]: edge types must be an integer tensor$"):
        check_etype_sorted(ip, key.float(), 3)
    with pytest.raises(ValueError, match=r"edata\['ts'\]: edge times must be an integer tensor \(floating-point timestamps are not supported\)$"):
        check_time_sorted(ip, key.float())
    with pytest.raises(ValueError, match=r"edata\['etype'\]: edge types must have shape \(8,\) in CSC order, got \(7,\)"):
        check_etype_sorted(ip, key[:-1], 3)
    with pytest.raises(ValueError, match=r"edata\['ts'\]: edge times must have shape \(8,\) in CSC order, got \(7,\)"):
        check_time_sorted(ip, key[:-1])
    with pytest.raises(ValueError, match=r"edge types must lie in \[0, 2\) \(num_rels=2\)"):   # only types have a range: 2 is a fine time
        check_etype_sorted(ip, key, 2)
    check_time_sorted(ip, key - 5)                                                              # ... and a time may be negative
    for check in (lambda: check_etype_sorted(torch.tensor([0, 0, 0]), torch.zeros(0, dtype=torch.int64), 3),
                  lambda: check_time_sorted(torch.tensor([0, 0, 0]), torch.zeros(0, dtype=torch.int64))):
        check()                                                                                 # no edges: nothing to check
