"""GPU tests of GraphConv / SAGEConv with edge_weight= on the native weighted sum (the checks of tests/_edge_weight_layers.py in
fp32 on the device), and a short training run of the example's GCN with edge weights through the prefetching loader."""
import math

import pytest

from _edge_weight_layers import check_layers, check_unweighted_graphconv_unchanged
from _util import ColorFiles

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("in_feats,out_feats", [(20, 8), (8, 20)])
def test_layers_with_edge_weight_against_dense_adjacency(hiplib, in_feats, out_feats, ragged):
    import torch
    check_layers("cuda", torch.float32, in_feats, out_feats, ragged)


@pytest.mark.parametrize("ragged", [False, True])
def test_graphconv_without_edge_weight_is_unchanged(hiplib, ragged):
    check_unweighted_graphconv_unchanged("cuda", ragged)


def test_gcn_trains_with_edge_weights_through_the_loader(hiplib, oracle, tmp_path):
    """The loop of test_loader_gpu.py::test_dataloader_epoch_and_sage_step (2 epochs of 11 steps, batch 64, prefetching loader) with
    the example's GCN taking block.edata['w'].  The labels are a function of what the model sees -- the class whose feature column
    has the largest weighted sum over a node's in-edges -- so the loss must come down: the mean of the last 5 steps is below the
    mean of the first 5, and every loss is finite."""
    import torch
    from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node_Distributor, SSD_INFO
    from COALA_GNN.harness import GCN
    from COALA_GNN.sampler import NeighborSampler
    from COALA_GNN.synthetic import alloc_pinned_table, block_colors, feature_rows_torch, powerlaw_csc
    torch.manual_seed(0)
    n_nodes, dim, batch, fan, n_cls = 20000, 128, 64, [5, 5], 5
    table = alloc_pinned_table(n_nodes, dim, seed=3, device=0)
    indptr, indices = powerlaw_csc(n_nodes, 8.0, seed=1, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    w = 1.0 - torch.rand(indices.numel(), generator=gen, device="cuda")
    w[torch.rand(indices.numel(), generator=gen, device="cuda") < 0.1] = 0.0
    rows = torch.repeat_interleave(torch.arange(n_nodes, device="cuda"), indptr[1:] - indptr[:-1])
    score = torch.zeros(n_nodes, n_cls, device="cuda").index_add_(0, rows, w[:, None] * feature_rows_torch(indices, dim, 3)[:, :n_cls])
    labels = score.argmax(1)
    color, tk, sc, ncol = block_colors(n_nodes, nodes_per_color=512)
    files = ColorFiles(tmp_path, color, tk, sc)
    comm = MPI_Comm_Manager(0)
    comm.initialize_nested_process_group("isolated")
    train_ids = torch.randperm(int(0.6 * n_nodes), generator=torch.Generator().manual_seed(0))[:64 * 12]
    nd = Node_Distributor(comm, train_ids, batch, files.color_file, files.topk_file, files.score_file, parsing_method="baseline")
    sampler = NeighborSampler(fan, seed=5, prob="w", edge_ids=True)
    g = sampler.make_graph(indptr, indices, ndata={"labels": labels}, edata={"w": w})
    loader = COALA_GNN_DataLoader(SSD_INFO(1, dim * 4, 1024, 0), nd, g, sampler, batch, dim, fan, 4, "cuda:0", refresh_counter=3,
                                  cache_backend="isolated", sim_buf=table, num_rows=n_nodes, prefetch=1)
    model = GCN(dim, 64, n_cls, len(fan), dropout=0.0, edge_weight="w").cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses = []
    for epoch in range(2):
        for input_nodes, seeds, blocks, feat in loader:
            batch_labels = blocks[-1].dstdata["labels"].view(-1)
            for b in blocks:
                eid = b.edata["_ID"]
                assert eid.shape == b.nbr.shape and torch.equal(eid >= 0, b.nbr >= 0)
                assert torch.equal(b.edata["w"], torch.where(eid >= 0, w[eid.clamp_min(0)], torch.zeros((), device="cuda")))
                assert sum(t is b.edata["w"] for t in b.tensors()) == 1
            loss = torch.nn.functional.cross_entropy(model(blocks, feat), batch_labels)
            opt.zero_grad(); loss.backward(); opt.step()
            losses.append(loss.item())
    print("losses:", " ".join(f"{x:.4f}" for x in losses))
    assert len(losses) == 22 and all(math.isfinite(x) for x in losses)
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5, losses
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    del loader
    table.close()
