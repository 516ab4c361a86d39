#!/usr/bin/env python3
"""Bit comparison of the attention kernels of two builds (profiles/r25_attention_kernel_refactor.txt).

COALA_PARENT_LIB=<libcoala_hip.so of another commit> is loaded beside this build's library in one process (ctypes, side by side, as in
tools/edge_weight_probe.py).  The forward and backward C entries of GAT, GATv2, dot-product and relation-typed GAT attention are called
from both on the same inputs, and every output must be torch.equal: out and lse; every gradient; GATv2's grad_attn partials at the same
`parts`.  The blocks are injective -- every source row stands in exactly one slot -- so a float atomic adds one term onto zero and the
atomic gradients are comparable bit for bit too.  Shapes: the places where the shared code takes another path (float4 / scalar rows, one
or several 64-float passes, a head boundary inside a pass, every RP of the GATv2 backward, rows of 0, 1, 63, 64, 65 and 200 slots, -1
slots inside fixed rows, a relation type out of range), scores with a common offset of about 1e3.
    COALA_PARENT_LIB=/path/to/parent/libcoala_hip.so python tools/attention_ab_probe.py"""
import ctypes as C
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "coala-gnn_amd")]
import torch  # noqa: E402
from COALA_GNN_Pybind import _capi, current_stream  # noqa: E402

if not os.environ.get("COALA_PARENT_LIB"):
    raise SystemExit(__doc__)
if os.path.realpath(os.environ["COALA_PARENT_LIB"]) == os.path.realpath(_capi.LIB_PATH):
    raise SystemExit("COALA_PARENT_LIB is the library under test: dlopen would hand back the same handle and every comparison would hold vacuously")
new = _capi.load()
par = C.CDLL(os.environ["COALA_PARENT_LIB"])
OPS = ("gat", "gatv2", "dot_gat", "rel_gat")
for op in OPS:
    for n in (f"coala_block_{op}_aggregate", f"coala_block_{op}_aggregate_backward", f"coala_block_{op}_aggregate_csr",
              f"coala_block_{op}_aggregate_csr_backward"):
        getattr(par, n).restype, getattr(par, n).argtypes = _capi.SYMBOLS[n]

torch.cuda.set_device(0)
st = current_stream()
gen = torch.Generator().manual_seed(25)
R, SLOPE, OFFSET = 3, 0.2, 1.0e3


def randn(*shape, mean=0.0):
    return (torch.randn(*shape, generator=gen) + mean).cuda()


def fixed_block(n_dst, f):
    """-> (None, idx [n_dst, f] int32 with -1 slots inside the rows, number of source rows); every source row in one slot."""
    valid = torch.rand(n_dst, f, generator=gen) < 0.8
    idx = torch.full((n_dst, f), -1, dtype=torch.int32)
    idx[valid] = torch.randperm(int(valid.sum()), generator=gen).int()
    return None, idx.cuda(), int(valid.sum())


def csr_block(lengths):
    indptr = torch.tensor([0] + lengths).cumsum(0)
    return indptr.cuda(), torch.randperm(int(indptr[-1]), generator=gen).int().cuda(), int(indptr[-1])


def run(lib, op, indptr, idx, etype, n_dst, f, heads, dim, tabs, go, parts):
    """Forward and backward of one op from one library -> {name: tensor}."""
    csr = indptr is not None
    fwd = getattr(lib, f"coala_block_{op}_aggregate" + ("_csr" if csr else ""))
    bwd = getattr(lib, f"coala_block_{op}_aggregate" + ("_csr" if csr else "") + "_backward")
    head = [0] + ([indptr.data_ptr()] if csr else []) + [idx.data_ptr()] + ([etype.data_ptr()] if op == "rel_gat" else [])
    shape = [n_dst] + ([] if csr else [f]) + ([R] if op == "rel_gat" else []) + [heads, dim]
    param = 1.0 / math.sqrt(dim) if op == "dot_gat" else SLOPE
    a, b, c = tabs
    out = torch.full((n_dst, heads, dim), float("nan"), device="cuda")
    lse = torch.full((n_dst, R, heads) if op == "rel_gat" else (n_dst, heads), float("nan"), device="cuda")
    assert fwd(*head, a.data_ptr(), b.data_ptr(), c.data_ptr(), out.data_ptr(), lse.data_ptr(), *shape, param, st) == 0, (op, "forward")
    res = {"out": out, "lse": lse}
    if op == "gatv2":  # grad_src by atomics; grad_dst and the partials are stored whole
        grads = {"grad_src": torch.zeros_like(a), "grad_dst": torch.full_like(b, float("nan")),
                 f"grad_attn_parts[{parts}]": torch.full((parts, heads * dim), float("nan"), device="cuda")}
        extra = [parts]
    elif op == "dot_gat":  # grad_q is stored whole
        grads = {"grad_q": torch.full_like(a, float("nan")), "grad_k": torch.zeros_like(b), "grad_v": torch.zeros_like(c)}
        extra = []
    else:  # (el, er, feat) -> grad_feat, grad_el by atomics, grad_er stored whole
        grads = {"grad_feat": torch.zeros_like(c), "grad_el": torch.zeros_like(a), "grad_er": torch.full_like(b, float("nan"))}
        extra = []
    saved = [lse.data_ptr()] if op == "rel_gat" else [out.data_ptr(), lse.data_ptr()]
    assert bwd(*head, a.data_ptr(), b.data_ptr(), c.data_ptr(), *saved, go.data_ptr(), *[g.data_ptr() for g in grads.values()], *extra, *shape, param,
               st) == 0, (op, "backward")
    torch.cuda.synchronize()
    res.update(grads)
    return res


def tables(op, n_src, n_dst, heads, dim):
    """The op's three tables, scores near OFFSET."""
    if op in ("gat", "rel_gat"):
        return randn(n_src, heads, mean=OFFSET), randn(n_dst, R, heads) if op == "rel_gat" else randn(n_dst, heads), randn(n_src, heads, dim)
    if op == "gatv2":  # z ~ OFFSET > 0 and sum_c attn ~ 1
        return randn(n_src, heads, dim), randn(n_dst, heads, dim, mean=OFFSET), (randn(heads, dim) * 0.1 + 1.0) / dim
    return randn(n_dst, heads, dim) * 0.1 + 1.0, randn(n_src, heads, dim, mean=OFFSET / math.sqrt(dim)), randn(n_src, heads, dim)  # q, k, v


CSR_ROWS = [0, 1, 63, 64, 65, 200] * 7
cases = [("fixed f=5", lambda: fixed_block(40, 5), 5, 4, 16),      # float4, one 64-float pass
         ("fixed f=32", lambda: fixed_block(40, 32), 32, 2, 65),   # scalar, three passes, a head boundary inside a pass
         ("fixed f=1", lambda: fixed_block(40, 1), 1, 16, 128),    # hd = 2048: GATv2 backward at RP = 0
         ("fixed f=5", lambda: fixed_block(40, 5), 5, 4, 128),     # RP = 8
         ("fixed f=7", lambda: fixed_block(41, 7), 7, 1, 64),      # RP = 1
         ("fixed f=7", lambda: fixed_block(41, 7), 7, 2, 64),      # RP = 2
         ("fixed f=7", lambda: fixed_block(41, 7), 7, 4, 64),      # RP = 4
         ("fixed f=3", lambda: fixed_block(40, 3), 3, 16, 64),     # RP = 16
         ("csr 0/1/63/64/65/200", lambda: csr_block(CSR_ROWS), 0, 4, 16),
         ("csr 0/1/63/64/65/200", lambda: csr_block(CSR_ROWS), 0, 2, 65),
         ("csr 0/1/63/64/65/200", lambda: csr_block(CSR_ROWS), 0, 4, 128),
         ("csr 0/1/63/64/65/200", lambda: csr_block(CSR_ROWS), 0, 16, 128)]
bad = 0
for name, make, f, heads, dim in cases:
    indptr, idx, n_src = make()
    n_dst = idx.shape[0] if indptr is None else indptr.numel() - 1
    etype = torch.randint(0, R, idx.shape, generator=gen).int()
    etype.view(-1)[torch.randperm(etype.numel(), generator=gen)[: max(1, etype.numel() // 16)]] = R  # out of range: treated as padding
    etype = etype.cuda()
    go = randn(n_dst, heads, dim)
    for op in OPS:
        tabs = tables(op, n_src, n_dst, heads, dim)
        for parts in ((1, min((n_dst + 3) // 4, 1024)) if op == "gatv2" else (0,)):
            got = [run(lib, op, indptr, idx, etype, n_dst, f, heads, dim, tabs, go, parts) for lib in (par, new)]
            lines = []
            for k in got[0]:
                same = torch.equal(got[0][k], got[1][k])
                finite = bool(torch.isfinite(got[1][k][got[1][k] != float("-inf")]).all())  # lse is -inf where a group has no edge
                bad += not (same and finite)
                lines.append(f"{k} {'equal' if same else 'DIFFERENT'}{'' if finite else ' NOT FINITE'}")
            print(f"{name:22s} H={heads:2d} D={dim:3d} {op:8s} " + ", ".join(lines))
print("done: every output equal bit for bit" if not bad else f"FAILED: {bad} outputs differ or are not finite")
sys.exit(1 if bad else 0)
