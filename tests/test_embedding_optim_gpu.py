"""GPU tests of SparseAdam and RowWiseAdagrad on a native NodeEmbedding: every step against the float64 one-step reference
(tests/_optim_ref.py) fed the reduced gradient the optimizer itself formed, the line-equals-cold-row invariant behind every step, Adam's
state in pinned host memory, one loader step through NodeEmbedding.from_manager / attach, and native against the torch backend."""
import numpy as np
import pytest

from _embedding_ref import U23, U24
from _optim_ref import (K_ADAM, adam_ref, check_adam, check_rowwise_adagrad, k_rowwise, make_grad, rowwise_additions,
                        rowwise_additions_torch, rowwise_adagrad_ref)
from _util import ColorFiles

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, RW_EPS = 0.05, (0.9, 0.999), 1e-8, 1e-10
NUM_ROWS, DIM = 5000, 64          # 1 MiB of 128-float lines holds 2048 rows: lookups both hit and miss
LATE = np.arange(NUM_ROWS - 50, NUM_ROWS)     # rows that sit out the first step


def _ids_for_step(rng, step):
    """Distinct ids with a quarter of them listed twice; the LATE rows join from the second step on, so their own t lags the global one."""
    pool = NUM_ROWS - len(LATE)
    ids = rng.choice(pool, size=500, replace=False)
    ids = np.concatenate([ids, ids[:125]])
    if step > 1:
        ids = np.concatenate([ids, LATE[:20], LATE[:5]])
    return rng.permutation(ids).astype(np.int64)


def _make(kind, reduce, backend="native"):
    import torch
    from COALA_GNN import NodeEmbedding, RowWiseAdagrad, SparseAdam
    torch.manual_seed(1)
    emb = NodeEmbedding(NUM_ROWS, DIM, cache_mb=1, device="cuda:0", backend=backend)
    if kind == "rowwise":
        return emb, RowWiseAdagrad([emb], lr=LR, eps=RW_EPS, reduce=reduce)
    mode = "global" if "global" in kind else "row"
    return emb, SparseAdam([emb], lr=LR, betas=BETAS, eps=EPS, reduce=reduce, step=mode, state_device_bytes=0 if "pinned" in kind else 1 << 30)


def _weights(emb):
    return emb.weight_host.numpy() if emb.backend == "native" else emb.weight.cpu().numpy()


def _snapshot(emb, opt):
    import torch
    torch.cuda.synchronize()
    return (_weights(emb).copy(),) + tuple(t.cpu().numpy().copy() for t in opt.state_of(emb)[:3 if hasattr(opt, "betas") else 1])


def _step(emb, opt, ids, coef):
    """Lookup, backward, step.  -> (uniq, g): the reduced gradient the optimizer formed from the trace, as numpy."""
    import torch
    d_ids = torch.from_numpy(ids).cuda()
    opt.zero_grad()
    rows = emb(d_ids)
    (rows * torch.from_numpy(coef).cuda()).sum().backward()
    uniq, g = opt._reduced(emb)
    opt.step()
    torch.cuda.synchronize()
    assert emb.trace == []
    return uniq.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("reduce", ["mean", "sum"])
@pytest.mark.parametrize("kind", ["adam-row", "adam-global", "adam-row-pinned", "adam-global-pinned", "rowwise"])
def test_native_steps_match_the_one_step_reference(hiplib, kind, reduce):
    import torch
    torch.cuda.set_device(0)
    rng = np.random.default_rng(2)
    emb, opt = _make(kind, reduce)
    adam = kind != "rowwise"
    if adam:
        m, v, steps = opt.state_of(emb)[:3]
        assert m.is_cuda == v.is_cuda == ("pinned" not in kind) and steps.is_cuda and steps.dtype == torch.int32
    w_start = _weights(emb).copy()
    never = np.ones(NUM_ROWS, dtype=bool)
    for step in range(1, 4):
        ids = _ids_for_step(rng, step)
        never[ids] = False
        coef = make_grad(rng, (len(ids), DIM))
        before = _snapshot(emb, opt)
        uniq, g = _step(emb, opt, ids, coef)
        assert np.array_equal(uniq, np.unique(ids))
        after = _snapshot(emb, opt)
        what = f"{kind} {reduce}, step {step}"
        if adam:
            w0, m0, v0, t0 = before
            w1, m1, v1, t1 = after
            if "global" in kind:
                t = step
                assert not t1.any()
            else:
                t = t0[uniq] + 1
                assert np.array_equal(t1[uniq], t)
            check_adam(w1[uniq], m1[uniq], v1[uniq], w0[uniq], m0[uniq], v0[uniq], t, g, LR, BETAS[0], BETAS[1], EPS, what)
        else:
            check_rowwise_adagrad(after[0][uniq], after[1][uniq], before[0][uniq], before[1][uniq], g, LR, RW_EPS, rowwise_additions(DIM, True), what)
        rest = np.ones(NUM_ROWS, dtype=bool)
        rest[uniq] = False
        for a, b in zip(after, before):
            assert a[rest].tobytes() == b[rest].tobytes(), f"{what}: something of a row that was not looked up changed"
        # the invariant: whatever the cache holds of the stepped rows and of a random draw is what the table holds
        back = np.unique(np.concatenate([uniq, rng.choice(NUM_ROWS, size=500, replace=False)]))
        assert emb.read(torch.from_numpy(back)).cpu().numpy().tobytes() == emb.weight_host.numpy()[back].tobytes()
    if adam and "global" not in kind:
        t = opt.state_of(emb)[2].cpu().numpy()
        assert int(t[LATE[:20]].max()) == 2 < opt.steps == 3        # the late rows' own count lags the optimizer's
    hit, miss, bad = emb._cache.stats()
    assert hit > 0 and miss > 0 and bad == 0
    assert never.any() and emb.weight_host.numpy()[never].tobytes() == w_start[never].tobytes()
    emb.close()


@pytest.mark.parametrize("kind", ["adam-row", "adam-global", "rowwise"])
def test_native_and_torch_backends_agree(hiplib, kind):
    """The same three steps on a native embedding and on the torch backend on the device, from the same start.  After every step each
    side is within its own bound of the reference from its OWN snapshot; after the first step, where both snapshots are the same
    bytes, the two sides differ by at most the sum of both bounds."""
    import torch
    torch.cuda.set_device(0)
    rng = np.random.default_rng(7)
    nat, nopt = _make(kind, "mean")
    tor, topt = _make(kind, "mean", backend="torch")
    torch.cuda.synchronize()
    tor.weight.copy_(nat.weight_host.cuda())
    adam = kind != "rowwise"
    A_n, A_t = rowwise_additions(DIM, True), rowwise_additions_torch(DIM)
    for step in range(1, 4):
        ids = _ids_for_step(rng, step)
        coef = make_grad(rng, (len(ids), DIM))
        snaps = [_snapshot(e, o) for e, o in ((nat, nopt), (tor, topt))]
        (uniq, g), (uniq_t, g_t) = _step(nat, nopt, ids, coef), _step(tor, topt, ids, coef)
        assert np.array_equal(uniq, uniq_t) and g.tobytes() == g_t.tobytes()
        outs = [_snapshot(e, o) for e, o in ((nat, nopt), (tor, topt))]
        for side, before, after, A in (("native", snaps[0], outs[0], A_n), ("torch", snaps[1], outs[1], A_t)):
            what = f"{kind} {side}, step {step}"
            if adam:
                t = step if "global" in kind else before[3][uniq] + 1
                check_adam(after[0][uniq], after[1][uniq], after[2][uniq], before[0][uniq], before[1][uniq], before[2][uniq], t, g, LR,
                           BETAS[0], BETAS[1], EPS, what)
            else:
                check_rowwise_adagrad(after[0][uniq], after[1][uniq], before[0][uniq], before[1][uniq], g, LR, RW_EPS, A, what)
        if step == 1:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(*snaps))
            if adam:
                ref, _, _, upd = adam_ref(snaps[0][0][uniq], snaps[0][1][uniq], snaps[0][2][uniq], 1, g, LR, BETAS[0], BETAS[1], EPS)
                bound = 2 * (U23 * np.abs(ref) + K_ADAM * U24 * np.abs(upd))
            else:
                ref, _, upd = rowwise_adagrad_ref(snaps[0][0][uniq], snaps[0][1][uniq], g, LR, RW_EPS)
                bound = 2 * U23 * np.abs(ref) + (k_rowwise(A_n) + k_rowwise(A_t)) * U24 * np.abs(upd)
            diff = np.abs(outs[0][0][uniq].astype(np.float64) - outs[1][0][uniq].astype(np.float64))
            assert np.all(diff <= bound), f"{kind}: native and torch differ by {float((diff / bound).max()):.3f} of the sum of their bounds"
    assert np.allclose(_weights(nat), _weights(tor), rtol=1e-4, atol=1e-5)
    nat.close()


@pytest.mark.parametrize("kind", ["adam", "rowwise"])
def test_one_loader_step_through_from_manager(hiplib, tmp_path, kind):
    import torch
    from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, NodeEmbedding, RowWiseAdagrad, SparseAdam, SSD_INFO
    from COALA_GNN.harness import SAGE
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import PinnedFeatureTable, block_colors, powerlaw_csc
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    n_nodes, dim, batch, fan = 2000, 128, 64, [5, 5]
    table = PinnedFeatureTable(n_nodes, dim, 0)
    table.cpu_tensor.uniform_(-0.1, 0.1)
    indptr, indices = powerlaw_csc(n_nodes, 8, seed=1, device="cuda")
    labels = (torch.arange(n_nodes, device="cuda") * 7) % 5
    color, tk, sc, _ = block_colors(n_nodes, nodes_per_color=512)
    files = ColorFiles(tmp_path, color, tk, sc)
    comm = MPI_Comm_Manager(0)
    comm.initialize_nested_process_group("isolated")
    train_ids = torch.randperm(int(0.6 * n_nodes), generator=torch.Generator().manual_seed(0))[:batch * 2]
    nd = Node_Distributor(comm, train_ids, batch, files.color_file, files.topk_file, files.score_file, parsing_method="baseline")
    sampler = NeighborSampler(fan, seed=5)
    g = sampler.make_graph(indptr, indices, ndata={"labels": labels})
    loader = COALA_GNN_DataLoader(SSD_INFO(1, dim * 4, 1024, 0), nd, g, sampler, batch, dim, fan, 1, "cuda:0", refresh_counter=3,
                                  cache_backend="isolated", sim_buf=table, num_rows=n_nodes, prefetch=0)
    emb = NodeEmbedding.from_manager(loader.COALA_GNN_Manager)
    model = SAGE(dim, 32, 5, 2, "mean").cuda()
    sparse = SparseAdam([emb], lr=LR, betas=BETAS, eps=EPS) if kind == "adam" else RowWiseAdagrad([emb], lr=LR, eps=RW_EPS)
    input_nodes, seeds, blocks, feat = next(iter(loader))
    torch.cuda.synchronize()
    w0 = table.array.copy()
    h = emb.attach(input_nodes, feat)
    assert h.is_leaf and h.data_ptr() == feat.data_ptr()
    torch.nn.functional.cross_entropy(model(blocks, h), blocks[-1].dstdata["labels"].view(-1)).backward()
    uniq, gr = sparse._reduced(emb)
    uniq, gr = uniq.cpu().numpy(), gr.cpu().numpy()
    keep = np.abs(gr).min(axis=1) >= 1e-15           # (the state bounds are relative: g * g * (1 - beta2) has to stay a normal fp32 number)
    assert keep.mean() > 0.5
    sparse.step()
    torch.cuda.synchronize()
    assert emb.trace == [] and np.array_equal(uniq, np.unique(input_nodes.cpu().numpy()))
    z = np.zeros((len(uniq), dim), dtype=np.float32)
    if kind == "adam":
        m, v, steps = (t.cpu().numpy() for t in sparse.state_of(emb)[:3])
        assert np.all(steps[uniq] == 1) and steps.sum() == len(uniq)
        k = uniq[keep]
        check_adam(table.array[k], m[k], v[k], w0[k], z[keep], z[keep], 1, gr[keep], LR, BETAS[0], BETAS[1], EPS, "loader step, adam")
    else:
        s = sparse.state_of(emb)[0].cpu().numpy()
        check_rowwise_adagrad(table.array[uniq], s[uniq], w0[uniq], z[:, 0], gr, LR, RW_EPS, rowwise_additions(dim, True), "loader step, row-wise")
    rest = np.ones(n_nodes, dtype=bool)
    rest[uniq] = False
    assert rest.any() and table.array[rest].tobytes() == w0[rest].tobytes()
    assert emb.read(torch.arange(n_nodes)).cpu().numpy().tobytes() == table.array.tobytes()
    del loader
    table.close()
