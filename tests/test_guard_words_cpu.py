"""The guard-word helpers of the GPU tests (tests/_util.py) catch a write just outside a region: one float too many behind the last
row, one float before the first, at either alignment.  Runs on the CPU (torch CPU tensors stand in for device buffers)."""
import numpy as np
import pytest

from _util import GUARD, SENTINEL, Guarded, check_guards


@pytest.mark.parametrize("off", [0, 1, 4])
def test_untouched_padding_passes(off):
    import torch
    g = Guarded(torch, 5, 7, off=off, fill=np.arange(35, dtype=np.float32).reshape(5, 7), device="cpu")
    assert g.flat.numel() == off + 35 + GUARD
    assert np.array_equal(g.region(), np.arange(35, dtype=np.float32).reshape(5, 7))


@pytest.mark.parametrize("off", [0, 1, 4])
def test_row_written_one_float_too_long_fails(off):
    import torch
    rows, dim = 5, 7
    g = Guarded(torch, rows, dim, off=off, device="cpu")
    row = rows - 1                                   # the last row, moved with dim + 1 floats: lands in the padding
    g.flat[off + row * dim: off + (row + 1) * dim + 1] = 1.5
    with pytest.raises(AssertionError, match="0 floats after the end"):
        g.region()


def test_write_before_the_region_fails():
    import torch
    g = Guarded(torch, 3, 4, off=1, device="cpu")
    g.flat[0] = 0.0
    with pytest.raises(AssertionError, match="1 floats before"):
        g.region()


def test_a_changed_bit_of_the_sentinel_fails():
    flat = np.full(10 + GUARD, SENTINEL, dtype=np.float32)
    check_guards(flat, 0, 10)
    flat.view(np.int32)[10 + GUARD - 1] ^= 1         # the last padding float, one bit off (compared as bits, not as values)
    with pytest.raises(AssertionError):
        check_guards(flat, 0, 10)
