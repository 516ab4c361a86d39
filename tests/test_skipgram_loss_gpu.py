"""GPU tests of the fused skip-gram window loss (coala_block_skipgram_loss / _backward; block_ops.skipgram_loss) against the float64
table of tests/_node2vec_ref.py.

Tolerance.  The yardstick is the fallback: for every shape the distance of skipgram_loss_torch, run in fp32 on the same inputs, from the
float64 reference is measured -- |loss32 - loss64| and max |grad32 - grad64| -- and the native path must stay within TWICE that
distance.  Nothing is derived from the native path's own results, and nothing is added to the measured distance.
A distance is a maximum of rounding errors, so one sample of it is itself random (the fallback's index_add reorders its sums from run
to run, and a single scalar difference can be small by chance): it is taken as the largest over DRAWS independent inputs of the shape,
and the native path is run on the same DRAWS inputs, every one held to twice that distance.  The native gradient is accumulated in
double and rounded once, so its own value does not move with the order of its atomics.

Measured on the MI355X, three runs of this file (largest of the 6 draws; fallback loss / gradient distance, the gradient's as lowest..highest of
the three runs | native loss / gradient distance | largest native : fallback ratio of a run, loss / gradient; the bound is 2):
  D   1 L+1   2 C   2 R     37: 1.5e-07 / 5.8e-09..5.8e-09 | 3.5e-08 / 5.8e-09..5.8e-09 | 0.23 / 1.00
  D   1 L+1  21 C   2 R     37: 1.4e-07 / 1.0e-09..1.0e-09 | 5.4e-08 / 8.2e-10..8.2e-10 | 0.40 / 0.78
  D   1 L+1  21 C  10 R     37: 1.6e-07 / 7.5e-10..7.5e-10 | 6.1e-08 / 3.1e-10..3.1e-10 | 0.39 / 0.42
  D   1 L+1  21 C  21 R     37: 8.0e-08 / 1.4e-09..1.4e-09 | 5.1e-08 / 5.9e-10..5.9e-10 | 0.64 / 0.43
  D   1 L+1 128 C   2 R      9: 6.5e-08 / 8.9e-10..8.9e-10 | 5.4e-08 / 3.8e-10..3.8e-10 | 0.83 / 0.43
  D   1 L+1 128 C  64 R      9: 8.1e-08 / 1.1e-09..1.1e-09 | 6.1e-08 / 2.9e-10..2.9e-10 | 0.76 / 0.27
  D   1 L+1 128 C 128 R      9: 9.2e-08 / 4.6e-09..4.6e-09 | 4.2e-08 / 9.0e-10..9.0e-10 | 0.46 / 0.20
  D  16 L+1   2 C   2 R     37: 1.1e-07 / 4.3e-09..4.3e-09 | 3.9e-08 / 3.8e-09..3.8e-09 | 0.36 / 0.87
  D  16 L+1  21 C   2 R     37: 1.1e-07 / 6.9e-10..6.9e-10 | 4.2e-08 / 3.2e-10..3.2e-10 | 0.39 / 0.47
  D  16 L+1  21 C  10 R     37: 1.1e-07 / 4.4e-10..4.4e-10 | 5.6e-08 / 1.5e-10..1.5e-10 | 0.51 / 0.34
  D  16 L+1  21 C  21 R     37: 5.5e-08 / 1.2e-09..1.2e-09 | 5.5e-08 / 3.8e-10..3.8e-10 | 1.00 / 0.32
  D  16 L+1 128 C   2 R      9: 1.3e-07 / 4.6e-10..4.6e-10 | 6.5e-08 / 2.8e-10..2.8e-10 | 0.50 / 0.61
  D  16 L+1 128 C  64 R      9: 1.0e-07 / 6.7e-10..6.7e-10 | 5.6e-08 / 8.7e-11..8.7e-11 | 0.56 / 0.13
  D  16 L+1 128 C 128 R      9: 1.0e-07 / 5.7e-09..5.7e-09 | 3.5e-08 / 6.3e-10..6.3e-10 | 0.34 / 0.11
  D  33 L+1   2 C   2 R     37: 9.6e-08 / 4.9e-09..4.9e-09 | 5.4e-08 / 3.2e-09..3.2e-09 | 0.56 / 0.66
  D  33 L+1  21 C   2 R     37: 1.5e-07 / 4.8e-10..4.8e-10 | 2.8e-08 / 3.0e-10..3.0e-10 | 0.19 / 0.64
  D  33 L+1  21 C  10 R     37: 1.5e-07 / 2.9e-10..2.9e-10 | 4.9e-08 / 1.2e-10..1.2e-10 | 0.32 / 0.40
  D  33 L+1  21 C  21 R     37: 5.8e-08 / 1.1e-09..1.1e-09 | 5.8e-08 / 3.4e-10..3.4e-10 | 1.00 / 0.30
  D  33 L+1 128 C   2 R      9: 1.3e-07 / 4.3e-10..4.3e-10 | 3.2e-08 / 2.4e-10..2.4e-10 | 0.24 / 0.55
  D  33 L+1 128 C  64 R      9: 8.9e-08 / 5.7e-10..5.7e-10 | 4.5e-08 / 6.4e-11..6.4e-11 | 0.51 / 0.11
  D  33 L+1 128 C 128 R      9: 8.6e-08 / 3.4e-09..3.4e-09 | 4.5e-08 / 5.9e-10..5.9e-10 | 0.52 / 0.17
  D 128 L+1   2 C   2 R     37: 1.2e-07 / 4.0e-09..4.0e-09 | 6.0e-08 / 2.1e-09..2.1e-09 | 0.48 / 0.52
  D 128 L+1  21 C   2 R     37: 1.3e-07 / 3.5e-10..3.5e-10 | 6.5e-08 / 2.0e-10..2.0e-10 | 0.51 / 0.58
  D 128 L+1  21 C  10 R     37: 8.6e-08 / 2.6e-10..2.6e-10 | 5.0e-08 / 8.4e-11..8.4e-11 | 0.58 / 0.32
  D 128 L+1  21 C  21 R     37: 1.1e-07 / 8.8e-10..8.8e-10 | 4.6e-08 / 2.8e-10..2.8e-10 | 0.42 / 0.31
  D 128 L+1 128 C   2 R      9: 1.7e-07 / 2.8e-10..2.8e-10 | 6.7e-08 / 2.1e-10..2.1e-10 | 0.39 / 0.74
  D 128 L+1 128 C  64 R      9: 9.4e-08 / 6.3e-10..6.3e-10 | 3.9e-08 / 4.7e-11..4.7e-11 | 0.41 / 0.07
  D 128 L+1 128 C 128 R      9: 8.6e-08 / 2.5e-09..2.5e-09 | 5.8e-08 / 5.2e-10..5.2e-10 | 0.68 / 0.20
  D  16 L+1   2 C   2 R 140000: 1.5e-07 / 3.6e-10..3.6e-10 | 4.6e-08 / 3.7e-11..3.7e-11 | 0.31 / 0.11
  D 128 L+1   2 C   2 R  33000: 1.9e-07 / 2.2e-10..2.2e-10 | 1.1e-07 / 6.5e-11..6.5e-11 | 0.60 / 0.30
  D  33 L+1   3 C   2 R  33000: 8.9e-08 / 2.4e-10..2.4e-10 | 4.8e-08 / 4.7e-11..4.7e-11 | 0.54 / 0.20
  D  16 L+1   2 C   2 R      1: 2.9e-08 / 2.7e-08..2.7e-08 | 4.0e-08 / 3.3e-08..3.3e-08 | 1.39 / 1.24
  D 128 L+1  21 C  10 R      1: 9.2e-08 / 1.2e-08..1.2e-08 | 5.4e-08 / 5.9e-09..5.9e-09 | 0.59 / 0.51
The largest ratio of all is 1.39.
(a run prints these lines with -s; profiles/r20_node2vec.txt keeps them.)"""
import numpy as np
import pytest

import _node2vec_ref as R

pytestmark = pytest.mark.gpu

DRAWS = 6
DIMS = [1, 16, 33, 128]
# (L + 1, C): C = 2, L + 1 and one in between
WINDOWS = [(2, 2), (21, 2), (21, 10), (21, 21), (128, 2), (128, 64), (128, 128)]


def make_case(rng, N, D, n_rows, L1):
    """h and two tables with ended walks, whole -1 rows, a node repeated inside a window and -1 in column 0."""
    h = (rng.standard_normal((N, D)) * (0.8 / np.sqrt(D) ** 0.5)).astype(np.float32)
    pos = rng.integers(0, N, size=(n_rows, L1)).astype(np.int32)
    neg = rng.integers(0, N, size=(2 * n_rows, L1)).astype(np.int32)
    for r in range(0, n_rows, 3):
        pos[r, rng.integers(1, L1):] = -1                 # an ended walk
    if n_rows > 1:
        pos[1, 1] = pos[1, 0]                             # a node twice inside a window
        pos[n_rows // 2] = -1                             # a whole row of -1: an invalid start node
        neg[[0, 2 * n_rows - 1]] = -1
    if L1 > 4 and n_rows > 1:
        neg[3, 2] = neg[3, 4] = neg[3, 0]
    return h, pos, neg


def run(fn, h, pos, neg, C, **kw):
    import torch
    t = torch.from_numpy(h).cuda().requires_grad_(True)
    out = fn(t, torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda(), C, **kw)
    out.backward()
    torch.cuda.synchronize()
    return out.detach(), t.grad


def check_shape(block_ops, D, L1, C, n_rows, N=300, plain=False):
    """The comparison of the module docstring on DRAWS inputs of one shape.  plain: tables of
    random entries in [-1, N) (the large-R cases, where make_case's row loops would dominate)."""
    import torch
    cases, dist_l, dist_g = [], 0.0, 0.0
    for draw in range(DRAWS):
        rng = np.random.default_rng(1000 * D + 10 * L1 + C + 7919 * draw + n_rows)
        if plain:
            h = (rng.standard_normal((N, D)) * 0.5).astype(np.float32)
            pos, neg = (rng.integers(-1, N, size=(n_rows, L1)).astype(np.int32) for _ in range(2))
        else:
            h, pos, neg = make_case(rng, N, D, n_rows, L1)
        want, want_g = R.skipgram_loss(h, pos, neg, C)
        low, low_g = run(block_ops.skipgram_loss_torch, h, pos, neg, C)
        dist_l = max(dist_l, abs(float(low) - want))
        dist_g = max(dist_g, float(np.abs(low_g.cpu().numpy().astype(np.float64) - want_g).max()))
        cases.append((h, pos, neg, want, want_g))
    worst_l = worst_g = 0.0
    for h, pos, neg, want, want_g in cases:
        got, got_g = run(block_ops.skipgram_loss, h, pos, neg, C)
        assert got.dtype == torch.float32 and got.dim() == 0 and got_g.dtype == torch.float32
        worst_l = max(worst_l, abs(float(got) - want))
        worst_g = max(worst_g, float(np.abs(got_g.cpu().numpy().astype(np.float64) - want_g).max()))
        again, _ = run(block_ops.skipgram_loss, h, pos, neg, C)
        assert again.view(torch.int32).item() == got.view(torch.int32).item(), "the forward is bitwise reproducible"
    print(f"D {D:3d} L+1 {L1:3d} C {C:3d} R {n_rows:6d}: fallback fp32 distance loss {dist_l:.3e} grad {dist_g:.3e} | native loss {worst_l:.3e} "
          f"grad {worst_g:.3e}")
    assert worst_l <= 2.0 * dist_l, f"loss: native {worst_l:.3e} from float64, the fallback {dist_l:.3e}"
    assert worst_g <= 2.0 * dist_g, f"gradient: native {worst_g:.3e} from float64, the fallback {dist_g:.3e}"


@pytest.mark.parametrize("L1,C", WINDOWS)
@pytest.mark.parametrize("D", DIMS)
def test_loss_and_gradient_against_float64(hiplib, D, L1, C, monkeypatch):
    from COALA_GNN import block_ops
    ran = []
    real = block_ops._SkipgramLoss.apply
    monkeypatch.setattr(block_ops._SkipgramLoss, "apply", staticmethod(lambda *a: ran.append(1) or real(*a)))
    check_shape(block_ops, D, L1, C, 37 if L1 < 128 else 9)
    assert len(ran) == 2 * DRAWS, "the native path did not run (two calls per draw)"


@pytest.mark.parametrize("D,L1,C,n_rows", [(16, 2, 2, 140000), (128, 2, 2, 33000), (33, 3, 2, 33000), (16, 2, 2, 1), (128, 21, 10, 1)])
def test_row_counts(hiplib, D, L1, C, n_rows):
    """R = 1, and R above one grid step (8192 blocks of 16 / 4 / 4 rows at these shapes): the same bound."""
    from COALA_GNN import block_ops
    if n_rows == 1:
        check_shape(block_ops, D, L1, C, 1)
    else:
        check_shape(block_ops, D, L1, C, n_rows, N=500, plain=True)


def test_dispatch_parity(hiplib, monkeypatch):
    """Shapes past the LDS budget, fp16 rows and CPU tables reach the fallback, with the values and dtype the fallback gives."""
    import torch
    from COALA_GNN import block_ops
    ran = []
    real = block_ops._SkipgramLoss.apply
    monkeypatch.setattr(block_ops._SkipgramLoss, "apply", staticmethod(lambda *a: ran.append(1) or real(*a)))
    rng = np.random.default_rng(5)
    for D, L1, dtype, idx_dev, native in ((129, 128, torch.float32, "cuda", False), (128, 128, torch.float32, "cuda", True),
                                          (782, 21, torch.float32, "cuda", False), (780, 21, torch.float32, "cuda", True),
                                          (16, 21, torch.float16, "cuda", False), (16, 21, torch.float32, "cpu", False),
                                          (16, 21, torch.float64, "cuda", False)):
        h, pos, neg = make_case(rng, 60, D, 5, L1)
        t = torch.from_numpy(h).cuda().to(dtype)
        p, n = torch.from_numpy(pos).to(idx_dev), torch.from_numpy(neg).to(idx_dev)
        del ran[:]
        got = block_ops.skipgram_loss(t, p, n, 8)
        assert bool(ran) == native, (D, L1, dtype, idx_dev)
        want = block_ops.skipgram_loss_torch(t, p, n, 8)
        assert got.dtype == want.dtype and got.shape == want.shape and got.device == want.device
        ref, _ = R.skipgram_loss(t.double().cpu().numpy(), pos, neg, 8)
        tol = {torch.float16: 2e-2, torch.float32: 2e-6, torch.float64: 1e-12}[dtype]
        assert abs(float(got) - ref) <= tol * max(1.0, abs(ref)) and (native or float(got) == float(want))
    with pytest.raises(IndexError):
        block_ops.skipgram_loss(torch.zeros(4, 8, device="cuda"), torch.tensor([[0, 4]], device="cuda"), torch.tensor([[0, 1]], device="cuda"), 2)


def test_no_valid_pair(hiplib):
    import torch
    from COALA_GNN import block_ops
    h = torch.randn(10, 16, device="cuda", requires_grad=True)
    none = torch.full((6, 21), -1, dtype=torch.int32, device="cuda")
    lone = none.clone()
    lone[:, 0] = 3                                        # a start node whose walk ended at once: no pair either
    for pos, neg in ((none, none), (lone, none[:0]), (none[:0], lone), (none[:0], none[:0])):
        if h.grad is not None:
            h.grad = None
        out = block_ops.skipgram_loss(h, pos, neg, 10)
        out.backward()
        assert float(out.detach()) == 0.0 and (h.grad is None or float(h.grad.abs().max()) == 0.0)
    # a window that does not reach the valid pair: positions 0 and 20 hold nodes, C = 10
    far = none.clone()
    far[:, 0], far[:, 20] = 1, 2
    assert float(block_ops.skipgram_loss(h, far, none, 10).detach()) == 0.0
    # one table empty of pairs, the other not: the loss is the other's mean alone
    pos = torch.tensor([[0, 1, -1]], dtype=torch.int32, device="cuda")
    s = float((h[0] * h[1]).sum().detach())
    got = float(block_ops.skipgram_loss(h, pos, none[:, :3], 2).detach())
    assert abs(got - float(np.log1p(np.exp(-s)))) <= 1e-5 * max(1.0, abs(s))
