"""Small consumers of the loader's 4-tuple on the native Block objects.  SageMean, a 2-layer GraphSAGE (mean) in plain torch, is
used by bench.py's epoch leg and the tests; it stands where examples/models.py:DistSAGE + dgl.nn.SAGEConv stand in the reference's
training script (examples/sbatch_ssd_gnn_train.py:98-145).  GAT and GCN mirror the reference's examples/models.py:GAT and :GCN on
COALA_GNN.nn's GATConv and GraphConv (--model_type gat|gcn); GAT's attention step is a native kernel (Block.gat_aggregate), and so is that
of GATv2, the same model on GATv2Conv layers (--model_type gatv2, Block.gatv2_aggregate).  GCN and
SAGE take edge_weight=<edata key> and then hand block.edata[key] to their layers (blocks sampled with NeighborSampler(edge_ids=True)).
SAGE(aggregator_type='pool') and GIN (--model_type gin) are the models on the native max aggregation (Block.max_aggregate).  RGCN
(--model_type rgcn) mirrors examples/models.py:RGCN on a homogenised graph: RelGraphConv layers, one weight matrix per edge type, on the
native relation-typed sum (Block.rel_sum_aggregate).  RGAT and RSAGE (--model_type rgat|rsage) mirror examples/models.py:RGAT and :RSAGE
the same way, on RelGATConv (the native relation-typed attention, Block.rel_gat_aggregate) and RelSAGEConv.  HGT (--model_type hgt) is the
Heterogeneous Graph Transformer on HGTConv layers, and DotGAT is GAT's shape on DotGatConv layers; both attend with the native scaled
dot-product kernel (Block.dot_gat_aggregate).  PinSAGE (--model_type pinsage) is the network of DGL's PinSAGE example on WeightedSAGEConv
layers, for blocks sampled by random walks (RandomWalkNeighborSampler): the visit counts weigh the neighbours."""
import time

import torch

from .nn import DotGatConv, DotPredictor, GATConv, GATv2Conv, GINConv, GraphConv, HGTConv, RelGATConv, RelGraphConv, RelSAGEConv, SAGEConv, WeightedSAGEConv

__all__ = ["SageMean", "SAGE", "GAT", "GATv2", "GCN", "GIN", "RGCN", "RGAT", "RSAGE", "HGT", "DotGAT", "PinSAGE", "LinkPredictor", "link_loss", "train_steps", "FlatGradAllReduce"]


class SageMean(torch.nn.Module):
    def __init__(self, in_dim, hidden, n_classes, n_layers=2):
        super().__init__()
        dims = [in_dim] + [hidden] * (n_layers - 1) + [n_classes]
        self.lin_self = torch.nn.ModuleList(torch.nn.Linear(dims[i], dims[i + 1]) for i in range(n_layers))
        self.lin_nbr = torch.nn.ModuleList(torch.nn.Linear(dims[i], dims[i + 1], bias=False) for i in range(n_layers))

    def forward(self, blocks, h):
        for i, b in enumerate(blocks):
            h = self.lin_self[i](b.dst_rows(h)) + self.lin_nbr[i](b.mean_aggregate(h))
            if i + 1 < len(blocks):
                h = torch.relu(h)
        return h


class GAT(torch.nn.Module):
    """examples/models.py:GAT: n_layers GATConv layers of num_heads heads, no activation between them (as in the reference), the
    heads flattened between layers; the last layer's heads are averaged and passed through log_softmax."""

    def __init__(self, in_feats, n_hidden, n_classes, n_layers, num_heads):
        super().__init__()
        dims = [in_feats] + [n_hidden * num_heads] * (n_layers - 1)
        outs = [n_hidden] * (n_layers - 1) + [n_classes]
        self.layers = torch.nn.ModuleList(GATConv((dims[i], dims[i]), outs[i], num_heads) for i in range(n_layers))

    def forward(self, blocks, x):
        h = x
        for i, (layer, block) in enumerate(zip(self.layers, blocks)):
            h = layer(block, (h, block.dst_rows(h)))
            if i + 1 < len(self.layers):
                h = h.flatten(1)
        return h.mean(1).log_softmax(dim=-1)


class GATv2(torch.nn.Module):
    """GAT's shape on GATv2Conv layers: n_layers layers of num_heads heads, no activation between them, the heads flattened between
    layers; the last layer's heads are averaged and passed through log_softmax.  share_weights: every layer uses one projection for the
    source and the destination rows (GATv2Conv's share_weights)."""

    def __init__(self, in_feats, n_hidden, n_classes, n_layers, num_heads, share_weights=False):
        super().__init__()
        dims = [in_feats] + [n_hidden * num_heads] * (n_layers - 1)
        outs = [n_hidden] * (n_layers - 1) + [n_classes]
        self.layers = torch.nn.ModuleList(GATv2Conv(dims[i], outs[i], num_heads, share_weights=share_weights) for i in range(n_layers))

    def forward(self, blocks, x):
        h = x
        for i, (layer, block) in enumerate(zip(self.layers, blocks)):
            h = layer(block, (h, block.dst_rows(h)))
            if i + 1 < len(self.layers):
                h = h.flatten(1)
        return h.mean(1).log_softmax(dim=-1)


class GCN(torch.nn.Module):
    """examples/models.py:GCN: n_layers GraphConv layers (norm='both'), dropout then relu between them."""

    def __init__(self, in_feats, h_feats, num_classes, num_layers=2, dropout=0.2, edge_weight=None):
        super().__init__()
        dims = [in_feats] + [h_feats] * (num_layers - 1) + [num_classes]
        self.layers = torch.nn.ModuleList(GraphConv(dims[i], dims[i + 1]) for i in range(num_layers))
        self.dropout = torch.nn.Dropout(dropout)
        self.edge_weight = edge_weight   # edata key of the per-edge weight every layer multiplies its messages by, or None

    def forward(self, blocks, x):
        h = x
        for i, (layer, block) in enumerate(zip(self.layers, blocks)):
            if self.edge_weight is None:
                h = layer(block, (h, block.dst_rows(h)))
            else:
                h = layer(block, (h, block.dst_rows(h)), edge_weight=block.edata[self.edge_weight])
            if i + 1 < len(self.layers):
                h = torch.relu(self.dropout(h))
        return h


class SAGE(torch.nn.Module):
    """GraphSAGE on COALA_GNN.nn.SAGEConv ('mean', 'gcn' as the reference's RSAGE model uses, or 'pool', the max-pooling aggregator),
    relu between the layers; with edge_weight=<edata key> every layer weighs its messages by block.edata[key]."""

    def __init__(self, in_feats, h_feats, num_classes, num_layers=2, aggregator_type="mean", edge_weight=None):
        super().__init__()
        dims = [in_feats] + [h_feats] * (num_layers - 1) + [num_classes]
        self.layers = torch.nn.ModuleList(SAGEConv(dims[i], dims[i + 1], aggregator_type) for i in range(num_layers))
        self.edge_weight = edge_weight

    def forward(self, blocks, x):
        h = x
        for i, (layer, block) in enumerate(zip(self.layers, blocks)):
            w = None if self.edge_weight is None else block.edata[self.edge_weight]
            h = layer(block, (h, block.dst_rows(h)), edge_weight=w)
            if i + 1 < len(self.layers):
                h = torch.relu(h)
        return h


class GIN(torch.nn.Module):
    """num_layers GINConv layers ('sum', 'max' or 'mean'), each with a two-layer MLP (Linear, relu, Linear) as its apply_func, relu
    between the layers; learn_eps makes every layer's eps a parameter."""

    def __init__(self, in_feats, h_feats, num_classes, num_layers=2, aggregator_type="sum", learn_eps=False):
        super().__init__()
        dims = [in_feats] + [h_feats] * (num_layers - 1) + [num_classes]
        self.layers = torch.nn.ModuleList(
            GINConv(torch.nn.Sequential(torch.nn.Linear(dims[i], h_feats), torch.nn.ReLU(), torch.nn.Linear(h_feats, dims[i + 1])),
                    aggregator_type, learn_eps=learn_eps) for i in range(num_layers))

    def forward(self, blocks, x):
        h = x
        for i, (layer, block) in enumerate(zip(self.layers, blocks)):
            h = layer(block, (h, block.dst_rows(h)))
            if i + 1 < len(self.layers):
                h = torch.relu(h)
        return h


class RGCN(torch.nn.Module):
    """R-GCN on a homogenised heterograph (one id space, one feature table, an integer type per edge): num_layers RelGraphConv layers
    with a self-loop, dropout then relu between them.  Every layer reads its edge types from block.edata[etype_key] -- gathered from
    graph.edata through the block's edge ids, so the blocks must come from a sampler made with edge_ids=True -- and normalises every
    message by 1 / c_{d,r}, the number of d's in-edges of that relation within the block (Block.rel_in_degrees): the R-GCN paper's
    per-relation mean."""

    def __init__(self, in_feats, h_feats, num_classes, num_layers, num_rels, regularizer=None, num_bases=None, dropout=0.2, etype_key="etype"):
        super().__init__()
        dims = [in_feats] + [h_feats] * (num_layers - 1) + [num_classes]
        self.layers = torch.nn.ModuleList(RelGraphConv(dims[i], dims[i + 1], num_rels, regularizer, num_bases) for i in range(num_layers))
        self.dropout = torch.nn.Dropout(dropout)
        self.num_rels, self.etype_key = num_rels, etype_key

    def forward(self, blocks, x):
        h = x
        for i, (layer, block) in enumerate(zip(self.layers, blocks)):
            if "_ID" not in block.edata:
                raise ValueError("RGCN needs the edge ids of its blocks to find their edge types: make the sampler with edge_ids=True")
            etype = block.edata[self.etype_key].to(h.device)
            t = etype.to(torch.int64)
            cnt = block.rel_in_degrees(etype, self.num_rels).to(h.device)
            in_range = (t >= 0) & (t < self.num_rels)
            rows = torch.arange(block.num_dst, device=h.device)
            if block.nbr is None:
                rows = torch.repeat_interleave(rows, (block.indptr[1:] - block.indptr[:-1]).to(h.device))
            else:
                rows = rows.unsqueeze(1).expand_as(t)
            norm = 1.0 / cnt[rows, t.clamp(0, self.num_rels - 1)].clamp_min(1).to(h.dtype) * in_range.to(h.dtype)
            h = layer(block, (h, block.dst_rows(h)), etype, norm)
            if i + 1 < len(self.layers):
                h = torch.relu(self.dropout(h))
        return h


def _block_etypes(block, key, model):
    """block.edata[key] for a model that reads its edge types from the blocks; RGCN's ValueError when they carry no edge ids."""
    if "_ID" not in block.edata:
        raise ValueError(f"{model} needs the edge ids of its blocks to find their edge types: make the sampler with edge_ids=True")
    return block.edata[key]


class RGAT(torch.nn.Module):
    """examples/models.py:RGAT on a homogenised heterograph (RGCN's input: one id space, one feature table, an integer type per edge):
    num_layers RelGATConv layers of n_heads heads of h_feats // n_heads features -- one GATConv per edge type, summed -- the heads
    flattened after every layer, relu then dropout between the layers, and a final Linear(h_feats, num_classes).  Every layer reads its
    edge types from block.edata[etype_key], so the blocks must come from a sampler made with edge_ids=True."""

    def __init__(self, in_feats, h_feats, num_classes, num_layers, num_rels, n_heads=4, dropout=0.2, etype_key="etype"):
        super().__init__()
        if h_feats % n_heads:
            raise ValueError(f"h_feats {h_feats} is not a multiple of n_heads {n_heads}")
        dims = [in_feats] + [h_feats] * (num_layers - 1)
        self.layers = torch.nn.ModuleList(RelGATConv(dims[i], h_feats // n_heads, n_heads, num_rels) for i in range(num_layers))
        self.dropout = torch.nn.Dropout(dropout)
        self.linear = torch.nn.Linear(h_feats, num_classes)
        self.num_rels, self.etype_key = num_rels, etype_key

    def forward(self, blocks, x):
        h = x
        for i, (layer, block) in enumerate(zip(self.layers, blocks)):
            etype = _block_etypes(block, self.etype_key, "RGAT").to(h.device)
            h = layer(block, (h, block.dst_rows(h)), etype).flatten(1)
            if i + 1 < len(self.layers):
                h = self.dropout(torch.relu(h))
        return self.linear(h)


class RSAGE(torch.nn.Module):
    """examples/models.py:RSAGE on a homogenised heterograph: num_layers RelSAGEConv layers of h_feats features -- one SAGEConv 'gcn' per
    edge type, summed -- relu then dropout between the layers, and a final Linear(h_feats, num_classes).  Edge types as for RGAT."""

    def __init__(self, in_feats, h_feats, num_classes, num_layers, num_rels, dropout=0.2, etype_key="etype"):
        super().__init__()
        dims = [in_feats] + [h_feats] * (num_layers - 1)
        self.layers = torch.nn.ModuleList(RelSAGEConv(dims[i], h_feats, num_rels) for i in range(num_layers))
        self.dropout = torch.nn.Dropout(dropout)
        self.linear = torch.nn.Linear(h_feats, num_classes)
        self.num_rels, self.etype_key = num_rels, etype_key

    def forward(self, blocks, x):
        h = x
        for i, (layer, block) in enumerate(zip(self.layers, blocks)):
            etype = _block_etypes(block, self.etype_key, "RSAGE").to(h.device)
            h = layer(block, (h, block.dst_rows(h)), etype)
            if i + 1 < len(self.layers):
                h = self.dropout(torch.relu(h))
        return self.linear(h)


class HGT(torch.nn.Module):
    """Heterogeneous Graph Transformer on a homogenised heterograph (RGCN's input, plus an integer type per node): num_layers HGTConv
    layers of num_heads heads of h_feats // num_heads features, and a final Linear(h_feats, num_classes).  HGTConv brings its own skip
    connection, dropout and LayerNorm (use_norm), so nothing stands between the layers.  ntype is the graph's node-type table
    [num_nodes], given at construction or per call (forward(blocks, x, ntype=...)); every layer indexes it with block.srcdata['_ID'].
    Every layer reads its edge types from block.edata[etype_key], so the blocks must come from a sampler made with edge_ids=True."""

    def __init__(self, in_feats, h_feats, num_classes, num_layers, num_heads, num_ntypes, num_rels, dropout=0.2, use_norm=True, ntype=None,
                 etype_key="etype"):
        super().__init__()
        if h_feats % num_heads:
            raise ValueError(f"h_feats {h_feats} is not a multiple of num_heads {num_heads}")
        dims = [in_feats] + [h_feats] * (num_layers - 1)
        self.layers = torch.nn.ModuleList(HGTConv(dims[i], h_feats // num_heads, num_heads, num_ntypes, num_rels, dropout, use_norm)
                                          for i in range(num_layers))
        self.linear = torch.nn.Linear(h_feats, num_classes)
        self.ntype, self.num_rels, self.etype_key = ntype, num_rels, etype_key

    def forward(self, blocks, x, ntype=None):
        table = self.ntype if ntype is None else ntype
        if table is None:
            raise ValueError("HGT needs the graph's node-type table [num_nodes]: HGT(..., ntype=) or forward(blocks, x, ntype=)")
        h = x
        for layer, block in zip(self.layers, blocks):
            etype = _block_etypes(block, self.etype_key, "HGT").to(h.device)
            nt = table[block.srcdata["_ID"].to(table.device)].to(h.device)
            h = layer(block, (h, block.dst_rows(h)), nt, etype)
        return self.linear(h)


class DotGAT(torch.nn.Module):
    """GAT's shape on DotGatConv layers: n_layers layers of num_heads heads, no activation between them, the heads flattened between
    layers; the last layer's heads are averaged and passed through log_softmax."""

    def __init__(self, in_feats, n_hidden, n_classes, n_layers, num_heads):
        super().__init__()
        dims = [in_feats] + [n_hidden * num_heads] * (n_layers - 1)
        outs = [n_hidden] * (n_layers - 1) + [n_classes]
        self.layers = torch.nn.ModuleList(DotGatConv(dims[i], outs[i], num_heads) for i in range(n_layers))

    def forward(self, blocks, x):
        h = x
        for i, (layer, block) in enumerate(zip(self.layers, blocks)):
            h = layer(block, h)
            if i + 1 < len(self.layers):
                h = h.flatten(1)
        return h.mean(1).log_softmax(dim=-1)


class PinSAGE(torch.nn.Module):
    """The network of DGL's PinSAGE example (SAGENet: WeightedSAGEConv layers of h_feats features, every one weighing its neighbours by
    block.edata[weight_key], the visit counts of RandomWalkNeighborSampler) with a Linear(h_feats, num_classes) on top for node
    classification.  Every layer's output rows have unit L2 norm, so nothing stands between the layers."""

    def __init__(self, in_feats, h_feats, num_classes, num_layers=2, weight_key="weights", dropout=0.0):
        super().__init__()
        dims = [in_feats] + [h_feats] * (num_layers - 1)
        self.layers = torch.nn.ModuleList(WeightedSAGEConv(dims[i], h_feats, h_feats, dropout=dropout) for i in range(num_layers))
        self.linear = torch.nn.Linear(h_feats, num_classes)
        self.weight_key = weight_key

    def forward(self, blocks, x):
        h = x
        for layer, block in zip(self.layers, blocks):
            if self.weight_key not in block.edata:
                raise ValueError(f"PinSAGE needs block.edata[{self.weight_key!r}]: sample the blocks with RandomWalkNeighborSampler")
            h = layer(block, (h, block.dst_rows(h)), block.edata[self.weight_key])
        return self.linear(h)


class LinkPredictor(torch.nn.Module):
    """Link prediction on any encoder of this module: the encoder's output rows (one per destination node of blocks[-1], the seed nodes
    of an EdgeBatch) are the node embeddings, and a pair's score is their dot product (DotPredictor), as in DGL's GraphSAGE
    link-prediction example.  forward(blocks, x, batch) -> (pos_score [n], neg_score [n * k]); an encoder that returns [N, H, D] gives
    [n, H] and [n * k, H]."""

    def __init__(self, encoder):
        super().__init__()
        self.encoder = encoder
        self.predictor = DotPredictor(validate=False)   # an EdgeBatch's pairs address the seed nodes by construction

    def forward(self, blocks, x, batch):
        h = self.encoder(blocks, x)
        return self.predictor(h, batch.pos_src, batch.pos_dst), self.predictor(h, batch.neg_src, batch.neg_dst)


def link_loss(pos_score, neg_score):
    """Binary cross-entropy with logits over the positive pairs (label 1) and the negative pairs (label 0), the mean over all of them:
    the loss of DGL's GraphSAGE link-prediction example."""
    score = torch.cat([pos_score.reshape(-1), neg_score.reshape(-1)])
    label = torch.cat([torch.ones_like(pos_score.reshape(-1)), torch.zeros_like(neg_score.reshape(-1))])
    return torch.nn.functional.binary_cross_entropy_with_logits(score, label)


class FlatGradAllReduce(object):
    """Data-parallel gradient averaging for the harness model: every parameter's gradient is a view into ONE flat buffer, averaged across the
    ranks with a single all-reduce per step (RCCL for GPU tensors).  Stands where DistributedDataParallel stands in the reference's script
    (examples/sbatch_ssd_gnn_train.py:112), with the same result for a model without unused parameters; torch's DDP costs this 1.6 ms
    training step another 1.0 ms of host time per iteration (measured at world size 1: 2.53 against 1.53 ms/step), which would bound a
    multi-GPU epoch whose fetch takes a third of that."""

    def __init__(self, model, group=None):
        import torch.distributed as dist
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.flat = torch.zeros(sum(p.numel() for p in self.params), dtype=self.params[0].dtype, device=self.params[0].device)
        off = 0
        for p in self.params:
            p.grad = self.flat[off: off + p.numel()].view_as(p)
            off += p.numel()
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self._dist = dist

    def zero(self):
        self.flat.zero_()         # (optimizer.zero_grad() would drop the views)

    def reduce(self):
        if self._dist.is_initialized():
            self._dist.all_reduce(self.flat, group=self.group)
            if self.world > 1:
                self.flat.div_(self.world)


def train_steps(loader, model, optimizer, max_steps, device, stop_check=None, check_every=64, grad_sync=None):
    """Runs up to max_steps iterations of the reference's training loop body; returns (steps, seconds, sampled_nodes).
    stop_check (optional): called every check_every steps on the host; a true answer ends the loop early (a caller with a time limit; in a
    multi-rank run it must give every rank the same answer at the same step -- the loop is full of collectives)."""
    loss_fn = torch.nn.CrossEntropyLoss()
    steps = nodes = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for input_nodes, seeds, blocks, feat in loader:
        nodes += len(input_nodes)
        labels = blocks[-1].dstdata["labels"].view(-1).to(device)
        blocks = [b.int().to(device) for b in blocks]
        loss = loss_fn(model(blocks, feat), labels)
        if grad_sync is not None:
            grad_sync.zero()
            loss.backward()
            grad_sync.reduce()
        else:
            optimizer.zero_grad()
            loss.backward()
        optimizer.step()
        steps += 1
        if steps >= max_steps:
            break
        if stop_check is not None and steps % check_every == 0 and stop_check():
            break
    torch.cuda.synchronize()
    return steps, time.perf_counter() - t0, nodes
