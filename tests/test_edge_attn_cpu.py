"""Block.edge_attn_aggregate_torch (the fallback and reference of the edge-feature attention kernels) against a per-destination float64
loop, its autograd gradients, the argument checks, the C symbols, and TransformerConv(edge_dim=) against PyG's per-edge formula."""
import numpy as np
import pytest
import torch

SYMBOLS = ["coala_block_edge_attn_aggregate" + s for s in ("", "_backward", "_csr", "_csr_backward")]


def make_block(rows, ragged, device="cpu"):
    """rows: a list of int lists (-1: a slot without an edge) -> the fixed block padded with -1, or the ragged block of the same slots."""
    from COALA_GNN.sampler import Block
    n_src = max([max(r, default=0) for r in rows] + [len(rows) - 1]) + 1
    src = torch.arange(n_src, device=device)
    if ragged:
        indptr = torch.tensor(np.cumsum([0] + [len(r) for r in rows]), device=device)
        flat = torch.tensor([s for r in rows for s in r], dtype=torch.int32, device=device)
        return Block(src, None, len(rows), indptr=indptr, indices=flat)
    fan = max(len(r) for r in rows)
    return Block(src, torch.tensor([r + [-1] * (fan - len(r)) for r in rows], dtype=torch.int32, device=device), len(rows))


def inputs(blk, H, D, F, table, seed=0, M=11):
    """-> (q, k, v, qe, efeat, eids) in float64; eids is None in the slot form and repeats ids in the table form."""
    g = torch.Generator().manual_seed(seed)
    slots = blk.indices if blk.nbr is None else blk.nbr
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    eids = torch.randint(0, M, tuple(slots.shape), generator=g) if table else None
    efeat = r(M, F) if table else r(*slots.shape, F)
    return r(blk.num_dst, H, D), r(blk.num_src, H, D), r(blk.num_src, H, D), r(blk.num_dst, H, F), efeat, eids


def loop_ref(blk, q, k, v, qe, efeat, eids, scale):
    """For each destination and head, a numpy softmax over its slots that hold an edge."""
    q, k, v, qe = (t.numpy() for t in (q, k, v, qe))
    slots = (blk.indices if blk.nbr is None else blk.nbr).reshape(-1).numpy()
    x = efeat.reshape(-1, efeat.shape[-1]).numpy()
    xrow = np.arange(slots.size) if eids is None else eids.reshape(-1).numpy()
    bounds = blk.indptr.numpy() if blk.nbr is None else np.arange(blk.num_dst + 1) * blk.nbr.shape[1]
    out, eagg = np.zeros(q.shape), np.zeros(qe.shape)
    for d in range(blk.num_dst):
        js = [j for j in range(bounds[d], bounds[d + 1]) if slots[j] >= 0]
        for h in range(q.shape[1] if js else 0):
            e = np.array([scale * (q[d, h] @ k[slots[j], h] + qe[d, h] @ x[xrow[j]]) for j in js])
            a = np.exp(e - e.max())
            a /= a.sum()
            out[d, h] = sum(a[i] * v[slots[j], h] for i, j in enumerate(js))
            eagg[d, h] = sum(a[i] * x[xrow[j]] for i, j in enumerate(js))
    return torch.from_numpy(out), torch.from_numpy(eagg)


ROWS = [[1, -1, 2, 0], [], [3, 3, -1, -1], [4, 0, 1, 2], [-1, 5]]


@pytest.mark.parametrize("table", [True, False], ids=["table", "slot"])
@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
def test_fallback_against_the_loop(hiplib, ragged, table):
    blk = make_block(ROWS, ragged)
    x = inputs(blk, 3, 5, 4, table)
    for scale in (None, 0.7):
        got = blk.edge_attn_aggregate_torch(*x, scale=scale)
        assert blk.edge_attn_aggregate(*x, scale=scale)[0].shape == got[0].shape == (5, 3, 5) and got[1].shape == (5, 3, 4)   # the CPU dispatches here
        for g, w in zip(got, loop_ref(blk, *x, 5 ** -0.5 if scale is None else scale)):
            torch.testing.assert_close(g, w, rtol=1e-12, atol=1e-12)
    assert not got[0][1].any() and not got[1][1].any()   # a destination without an edge


@pytest.mark.parametrize("table", [True, False], ids=["table", "slot"])
def test_fallback_gradients(hiplib, table):
    blk = make_block(ROWS, False)
    *x, eids = inputs(blk, 2, 3, 4, table, seed=1)
    x = [t.requires_grad_() for t in x]
    assert torch.autograd.gradcheck(lambda *a: blk.edge_attn_aggregate_torch(*a, eids), x)


def test_symbols_and_argument_checks(hiplib):
    from COALA_GNN_Pybind import _capi
    lib = _capi.load()
    assert all(s in _capi.SYMBOLS and getattr(lib, s) for s in SYMBOLS) and lib.coala_abi_version() == 4
    blk = make_block(ROWS, False)
    q, k, v, qe, efeat, eids = inputs(blk, 2, 3, 4, True)
    for bad in [(q[:, :1], k, v, qe, efeat, eids), (q, k[:-1], v[:-1], qe, efeat, eids), (q, k, v, qe[:, :, :3], efeat, eids),
                (q, k, v, qe, efeat, eids[:, :2]), (q, k, v, qe, efeat, None), (q, k, v, qe, efeat, eids.double())]:
        with pytest.raises(ValueError, match="this block takes|integer"):
            blk.edge_attn_aggregate(*bad)
    with pytest.raises(IndexError):
        blk.edge_attn_aggregate(q, k, v, qe, efeat, eids.clamp_min(11))
    blk.edge_attn_aggregate(q, k, v, qe, efeat, torch.where(blk.nbr >= 0, eids, 99))   # ids are not read on padding


@pytest.mark.parametrize("concat, beta", [(True, False), (False, True)])
def test_transformer_conv_is_pygs_formula(hiplib, concat, beta):
    """Keys and values with lin_edge(x_j) added per edge, written out edge by edge."""
    from COALA_GNN.nn import TransformerConv
    torch.manual_seed(2)
    H, D, F = 2, 3, 4
    blk = make_block(ROWS, True)
    conv = TransformerConv(7, D, H, edge_dim=F, concat=concat, beta=beta).double()
    h, (_, _, _, _, efeat, eids) = torch.randn(blk.num_src, 7, dtype=torch.float64), inputs(blk, H, D, F, True)
    got = conv(blk, h, efeat, eids)
    q, k, v = (lin(h).view(-1, H, D) for lin in (conv.lin_query, conv.lin_key, conv.lin_value))
    rows = []
    for d in range(blk.num_dst):
        js = [j for j in range(int(blk.indptr[d]), int(blk.indptr[d + 1])) if blk.indices[j] >= 0]
        msg = torch.zeros(H, D, dtype=torch.float64)
        if js:
            e = torch.stack([conv.lin_edge(efeat[eids[j]]).view(H, D) for j in js])                    # [n, H, D]
            s = blk.indices[js].long()
            a = torch.softmax((q[d] * (k[s] + e)).sum(-1) / D ** 0.5, dim=0)                             # [n, H]
            msg = (a.unsqueeze(-1) * (v[s] + e)).sum(0)
        rows.append(msg.flatten() if concat else msg.mean(0))
    out, r = torch.stack(rows), conv.lin_skip(h[: blk.num_dst])
    b = torch.sigmoid(conv.lin_beta(torch.cat([out, r, out - r], -1))) if beta else 0.5
    want = b * r + (1 - b) * out if beta else out + r
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10)
    assert got.shape == (5, H * D if concat else D)
