"""GPU tests of COALA_GNN.Node2Vec: one training step against the references, a short training run, and reproducibility.

One step = walk_batch -> NodeEmbedding lookup -> skipgram_loss -> backward -> SparseAdam.step().  It is checked link by link, each
against its own reference and with that reference's bound:
  * the batch equals tests/_node2vec_ref.walk_batch bit for bit;
  * the loss and the gradient of the looked-up rows stay within twice the distance of the fp32 fallback from the float64 table of
    _node2vec_ref (test_skipgram_loss_gpu.py's yardstick);
  * the table rows, Adam's state and the cached rows after the step equal tests/_optim_ref.adam_ref fed the gradient the optimizer
    reduced, within check_adam's bound -- the way, and the bound, of test_embedding_optim_gpu.py; rows that were not in the batch keep
    their bytes."""
import numpy as np
import pytest

import _node2vec_ref as R
from _optim_ref import check_adam

pytestmark = pytest.mark.gpu

LR, BETAS, EPS = 0.05, (0.9, 0.999), 1e-8


def _graph(num_nodes, community, seed):
    from COALA_GNN.sampler import CSCGraph
    from COALA_GNN.synthetic import community_csc, symmetrize_csc
    ip, ix = symmetrize_csc(*community_csc(num_nodes, 8, community=community, p_in=0.95, seed=seed, device="cuda"))
    return CSCGraph(ip, ix), ip.cpu().numpy(), ix.cpu().numpy()


def test_one_step_against_the_references(hiplib):
    import torch
    from COALA_GNN import Node2Vec, SparseAdam, block_ops
    torch.cuda.set_device(0)
    torch.manual_seed(4)
    g, ip, ix = _graph(2000, 250, 1)
    N, D, L, C, W, K = g.num_nodes, 16, 10, 5, 2, 1
    model = Node2Vec(g, D, L, C, walks_per_node=W, p=0.5, q=2.0, num_negative_samples=K, cache_mb=1, device="cuda:0", seed=3)
    emb = model.embedding
    opt = SparseAdam(emb, lr=LR, betas=BETAS, eps=EPS)
    try:
        rng = np.random.default_rng(0)
        nodes = rng.choice(N, size=128, replace=False).astype(np.int64)
        emb.read(torch.from_numpy(nodes[:64]))                                  # some rows are cached before the step, most are not
        batch = model.sample(torch.from_numpy(nodes).cuda(), step=0)
        want = R.walk_batch(ip, ix, nodes, L, W, K, R.thresholds(0.5, 2.0), seed=3, step=0)
        for key in ("input_nodes", "pos", "neg"):
            assert np.array_equal(getattr(batch, key).cpu().numpy(), want[key]), key
        assert batch.n_bad == 0
        ids = want["input_nodes"]
        torch.cuda.synchronize()
        w0 = emb.weight_host.numpy().copy()
        m0, v0, t0 = (t.cpu().numpy().copy() for t in opt.state_of(emb)[:3])
        # ---- loss and gradient
        loss = model.loss(batch)
        loss.backward()
        (_, leaf), = emb.trace
        assert leaf.detach().cpu().numpy().tobytes() == w0[ids].tobytes(), "the lookup returns the table's rows"
        ref_loss, ref_grad = R.skipgram_loss(w0[ids], want["pos"], want["neg"], C)
        low_h = torch.from_numpy(w0[ids]).cuda().requires_grad_(True)
        low = block_ops.skipgram_loss_torch(low_h, batch.pos, batch.neg, C)
        low.backward()
        d_l = abs(float(low.detach()) - ref_loss)
        d_g = float(np.abs(low_h.grad.cpu().numpy().astype(np.float64) - ref_grad).max())
        e_l = abs(float(loss.detach()) - ref_loss)
        e_g = float(np.abs(leaf.grad.cpu().numpy().astype(np.float64) - ref_grad).max())
        print(f"one step: loss {ref_loss:.6f}; fallback fp32 distance loss {d_l:.3e} grad {d_g:.3e} | native loss {e_l:.3e} grad {e_g:.3e}")
        assert e_l <= 2.0 * d_l and e_g <= 2.0 * d_g
        # ---- the update
        uniq, gr = opt._reduced(emb)
        uniq, gr = uniq.cpu().numpy(), gr.cpu().numpy()
        assert np.array_equal(uniq, np.sort(ids)) and np.array_equal(gr, leaf.grad.cpu().numpy()[np.argsort(ids)])
        opt.step()
        torch.cuda.synchronize()
        w1 = emb.weight_host.numpy()
        m1, v1, t1 = (t.cpu().numpy() for t in opt.state_of(emb)[:3])
        assert np.array_equal(t1[uniq], t0[uniq] + 1)
        check_adam(w1[uniq], m1[uniq], v1[uniq], w0[uniq], m0[uniq], v0[uniq], 1, gr, LR, BETAS[0], BETAS[1], EPS, "node2vec step")
        rest = np.ones(N, dtype=bool)
        rest[uniq] = False
        assert rest.any() and w1[rest].tobytes() == w0[rest].tobytes() and not m1[rest].any() and not t1[rest].any()
        # the cached rows are the table's rows: through the model's untracked read, for the stepped rows and a random draw
        back = np.unique(np.concatenate([uniq, rng.choice(N, size=300, replace=False)]))
        assert model(torch.from_numpy(back)).cpu().numpy().tobytes() == w1[back].tobytes()
        assert emb.trace == [] and tuple(model().shape) == (N, D)
    finally:
        model.close()
        g.close()


def test_forty_steps_lower_the_loss(hiplib):
    import torch
    from COALA_GNN import Node2Vec, SparseAdam
    torch.cuda.set_device(0)
    torch.manual_seed(5)
    g, ip, ix = _graph(512, 256, 2)
    model = Node2Vec(g, 16, 10, 5, walks_per_node=2, p=1.0, q=0.5, num_negative_samples=1, cache_mb=1, device="cuda:0", seed=1)
    opt = SparseAdam(model.embedding, lr=0.05)
    try:
        losses = []
        while len(losses) < 40:
            for batch in model.loader(128):
                loss = model.loss(batch)
                loss.backward()
                opt.step()
                losses.append(float(loss))
        assert len(losses) == 40 and model.step == 40 and all(np.isfinite(losses))
        first, last = float(np.mean(losses[:5])), float(np.mean(losses[-5:]))
        print(f"40 steps: mean loss of the first five {first:.4f}, of the last five {last:.4f}")
        assert last < first
    finally:
        model.close()
        g.close()


def test_same_seed_same_batches(hiplib):
    import torch
    from COALA_GNN import Node2Vec
    torch.cuda.set_device(0)
    g, ip, ix = _graph(512, 256, 2)
    models = [Node2Vec(g, 8, 6, 3, walks_per_node=2, p=0.5, q=2.0, num_negative_samples=2, cache_mb=1, device="cuda:0", seed=s, backend="torch")
              for s in (7, 7, 8)]
    try:
        epochs = [[(b.nodes.clone(), b.input_nodes.clone(), b.pos.clone(), b.neg.clone()) for b in m.loader(100)] for m in models]
        assert [len(e) for e in epochs] == [6, 6, 6] and all(m.step == 6 for m in models)
        assert all(torch.equal(x, y) for a, b in zip(epochs[0], epochs[1]) for x, y in zip(a, b)), "the same seed gives the same batches"
        assert not all(torch.equal(a[0], b[0]) for a, b in zip(epochs[0], epochs[2])), "another seed, another order"
        assert torch.equal(torch.sort(torch.cat([a[0] for a in epochs[0]])).values, torch.arange(512, device=g.device)), "an epoch visits every node once"
        second = [(b.nodes.clone(), b.pos.clone()) for b in models[0].loader(100)]
        assert not all(torch.equal(a[0], b[0]) for a, b in zip(epochs[0], second)), "the next epoch is shuffled anew"
        # batch number = step: batch 2 of the epoch again, by hand
        again = models[1].sample(epochs[0][2][0], step=2)
        assert torch.equal(again.pos, epochs[0][2][2]) and torch.equal(again.input_nodes, epochs[0][2][1])
        plain = [b.nodes for b in models[2].loader(100, shuffle=False)]
        assert torch.equal(torch.cat(plain), torch.arange(512, device=g.device))
    finally:
        for m in models:
            m.close()
        g.close()
