"""CPU tests of the message-passing primitives: the _torch twins (what a CPU block runs) against a Python loop over the rows, the shift
invariance of the softmax reference, and the refusals of the C entries (no kernel is launched here)."""
import pytest
import torch

from test_multi_aggregate_cpu import NBR, hand_block

ENTRIES = ("coala_block_u_dot_v", "coala_block_u_mul_e_sum", "coala_block_e_mul_v_scatter", "coala_block_edge_softmax",
           "coala_block_edge_softmax_backward")


@pytest.mark.parametrize("form", ["fixed", "ragged"])
def test_twins_match_a_loop_over_the_rows(hiplib, form):
    blk, H, D = hand_block(form), 3, 4
    g = torch.Generator().manual_seed(0)
    u, v = torch.randn(8, H, D, generator=g).double(), torch.randn(len(NBR), H, D, generator=g).double()
    e = blk.u_dot_v(u, v)                                   # float64 on the CPU: the twins
    a, s = blk.edge_softmax(e), blk.u_add_v(u[..., 0], v[..., 0])
    out = blk.u_mul_e_sum(u, a)
    valid = torch.from_numpy(NBR >= 0)
    assert e.shape == ((NBR.shape if form == "fixed" else (int(valid.sum()),)) + (H,))
    shifted = blk.edge_softmax(e + 1000.0)                  # the reference is shift-invariant, and 0 stays 0 on padding
    torch.testing.assert_close(shifted, a, rtol=1e-12, atol=0)

    def dense(t):   # [n_dst, fanout, H] of either form, 0 on padding
        return t if form == "fixed" else torch.zeros(NBR.shape + (H,), dtype=t.dtype).masked_scatter(valid.unsqueeze(-1), t)

    e, a, s, shifted = dense(e), dense(a), dense(s), dense(shifted)
    assert not e[~valid].any() and not a[~valid].any() and not s[~valid].any() and not shifted[~valid].any()
    for d, row in enumerate(NBR):
        src = [int(x) for x in row if x >= 0]
        if not src:
            assert not out[d].any()
            continue
        want = torch.stack([(u[x] * v[d]).sum(-1) for x in src])
        torch.testing.assert_close(e[d][valid[d]], want, rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(a[d][valid[d]], torch.softmax(want, 0), rtol=1e-13, atol=0)
        assert torch.equal(s[d][valid[d]], torch.stack([u[x, :, 0] + v[d, :, 0] for x in src]))
        torch.testing.assert_close(out[d], (torch.softmax(want, 0).unsqueeze(-1) * u[src]).sum(0), rtol=1e-13, atol=1e-13)


def test_refusals_and_abi(hiplib):
    from COALA_GNN_Pybind import _capi
    lib, blk = _capi.load(), hand_block("fixed")
    assert lib.coala_abi_version() == 4
    for name in ENTRIES:
        softmax, n_ptr = "softmax" in name, sum(t is _capi._VP for t in _capi.SYMBOLS[name][1]) - 1   # the last one is the stream
        for csr in (False, True):
            fn = getattr(lib, name + "_csr" * csr)
            assert name + "_csr" * csr in _capi.SYMBOLS

            def call(ptr, n_dst, heads):   # fan-out 4 on the fixed form, dim 8 where the entry has one
                return fn(0, *[ptr] * (n_ptr + csr), n_dst, *[4] * (not csr), heads, *[8] * (not softmax), None)

            for heads in (0, 17):
                assert call(1, 5, heads) == _capi.EINVAL and "heads" in _capi.last_error()
            assert call(None, 5, 2) == _capi.EINVAL and "null" in _capi.last_error()
            assert call(None, 0, 2) == _capi.OK
    with pytest.raises(ValueError):
        blk.edge_softmax(torch.zeros(5, 3, 2))
    with pytest.raises(ValueError):
        blk.u_mul_e_sum(torch.zeros(8, 2, 4), torch.zeros(5, 4, 3))
