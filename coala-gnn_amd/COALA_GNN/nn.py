"""GATConv, GATv2Conv, GraphConv, SAGEConv, GINConv, RelGraphConv, RelGATConv and RelSAGEConv on the native Block objects, for the reference's GAT and GCN models (examples/models.py;
DGL is not installed on the MI355X image) and for DGL models ported to them.  All take (block, (h_src, h_dst)) as DGL's modules do on
a block.

GATConv's projections are dense and stay in torch; its attention step (score, per-destination softmax, weighted sum) is
Block.gat_aggregate, a native kernel on both block forms; GATv2Conv's, whose score is a dot product over the whole [H, D] row per edge,
is Block.gatv2_aggregate, a native kernel as well, without the [E, H, D] intermediates of the formula.  GraphConv reduces to Block.mean_aggregate times the in-degree.  With
edge_weight= (one value per neighbour slot, e.g. block.edata['w'] of a block sampled with edge_ids=True) GraphConv and SAGEConv
aggregate with Block.weighted_sum_aggregate, DGL's u_mul_e_sum.  SAGEConv's 'pool' and GINConv's 'max' take their maximum with
Block.max_aggregate (DGL's fn.max), a native kernel as well; GINConv's 'sum' is Block.weighted_sum_aggregate with unit weights.
RelGraphConv (one weight matrix per edge type) sums the messages per relation with Block.rel_sum_aggregate, a native kernel, and applies
all its weight matrices in one GEMM.  RelGATConv and RelSAGEConv are the layers of the reference's heterogeneous models RGAT and RSAGE
on a homogenised block -- HeteroGraphConv over one GATConv, or one SAGEConv 'gcn', per edge type, summed: RelGATConv's softmax per
(destination, relation) is Block.rel_gat_aggregate, a native kernel; RelSAGEConv needs Block.rel_sum_aggregate and one GEMM.
DotGatConv and HGTConv (the Heterogeneous Graph Transformer, on a homogenised block with a type per node and per edge) attend with a
scaled dot product, Block.dot_gat_aggregate, a native kernel without [E, H, D] intermediates; HGTConv applies its per-relation D x D
matrices per (source, relation) pair, not per edge, and folds the relation prior into the attention matrix.
WeightedSAGEConv is the layer of DGL's PinSAGE example on blocks sampled by random walks (RandomWalkNeighborSampler): the visit counts
in block.edata['weights'] weigh the neighbours' rows through Block.weighted_sum_aggregate."""
import torch

__all__ = ["GATConv", "GATv2Conv", "DotGatConv", "GraphConv", "SAGEConv", "WeightedSAGEConv", "GINConv", "RelGraphConv", "RelGATConv", "RelSAGEConv", "HGTConv", "DotPredictor"]


class GATConv(torch.nn.Module):
    """Graph attention layer with separate source and destination projections (DGL 1.x GATConv given a tuple in_feats).

    Semantics, for destination node d, head h and the valid in-edges j of d (source s_j) in the block:
        feat_src = fc_src(feat_drop(h_src)).view(-1, H, D);   feat_dst = fc_dst(feat_drop(h_dst)).view(-1, H, D)
        el[s, h] = sum_k feat_src[s, h, k] * attn_l[0, h, k];   er[d, h] = sum_k feat_dst[d, h, k] * attn_r[0, h, k]
        e_j = leaky_relu(el[s_j, h] + er[d, h], negative_slope);   a_j = softmax of e over d's in-edges
        out[d, h, :] = sum_j a_j feat_src[s_j, h, :] + bias.view(H, D);   then activation, if any
    -> [num_dst, H, D].  A destination without an in-edge gets the bias alone (DGL's allow_zero_in_degree=True).
    Parameters, with the names and shapes of DGL 1.x for a tuple in_feats, so that such a state_dict loads:
        fc_src.weight [H * D, in_src], fc_dst.weight [H * D, in_dst] (no bias), attn_l [1, H, D], attn_r [1, H, D], bias [H * D].
    Initialisation: Xavier-normal with the gain of relu for fc_src, fc_dst, attn_l and attn_r; bias zero.
    h_dst must be the destination rows of h_src: block.dst_rows(h_src) (h_src[:num_dst] unless the block is owner-bucketed).
    Attention dropout and residual connections are not provided."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, negative_slope=0.2, bias=True, activation=None):
        super().__init__()
        in_src, in_dst = in_feats if isinstance(in_feats, (tuple, list)) else (in_feats, in_feats)
        self._num_heads, self._out_feats = num_heads, out_feats
        self.fc_src = torch.nn.Linear(in_src, out_feats * num_heads, bias=False)
        self.fc_dst = torch.nn.Linear(in_dst, out_feats * num_heads, bias=False)
        self.attn_l = torch.nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = torch.nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.bias = torch.nn.Parameter(torch.empty(num_heads * out_feats)) if bias else None
        self.feat_drop = torch.nn.Dropout(feat_drop)
        self.negative_slope = negative_slope
        self.activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        gain = torch.nn.init.calculate_gain("relu")
        for w in (self.fc_src.weight, self.fc_dst.weight, self.attn_l, self.attn_r):
            torch.nn.init.xavier_normal_(w, gain=gain)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, block, feat):
        h_src, h_dst = feat
        H, D = self._num_heads, self._out_feats
        feat_src = self.fc_src(self.feat_drop(h_src)).view(-1, H, D)
        feat_dst = self.fc_dst(self.feat_drop(h_dst)).view(-1, H, D)
        el = (feat_src * self.attn_l).sum(-1)
        er = (feat_dst * self.attn_r).sum(-1)
        rst = block.gat_aggregate(el, er, feat_src, self.negative_slope)
        if self.bias is not None:
            rst = rst + self.bias.view(1, H, D)
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class GATv2Conv(torch.nn.Module):
    """GATv2 attention layer (Brody et al., "How Attentive are Graph Attention Networks?"; DGL 1.x GATv2Conv).

    Semantics, for destination node d, head h and the valid in-edges j of d (source s_j) in the block:
        feat_src = fc_src(feat_drop(h_src)).view(-1, H, D);   feat_dst = fc_dst(feat_drop(h_dst)).view(-1, H, D)
        e_j = sum_c attn[0, h, c] * leaky_relu(feat_src[s_j, h, c] + feat_dst[d, h, c], negative_slope);   a_j = softmax of e over d's in-edges
        out[d, h, :] = sum_j a_j feat_src[s_j, h, :];   then activation, if any
    -> [num_dst, H, D].  A destination without an in-edge gets zeros (DGL's allow_zero_in_degree=True).
    Parameters, with the names and shapes of DGL 1.x, so that such a state_dict loads with strict=True:
        fc_src.weight [H * D, in_src], fc_src.bias [H * D], fc_dst.weight [H * D, in_dst], fc_dst.bias [H * D], attn [1, H, D].
    The bias flag is the bias of the two Linears, as in DGL: there is no separate bias parameter, and with bias=False the two bias keys
    are absent.  DGL is not installed where this was written: the names are those of DGL's source as remembered, and they are what this
    layer fixes.
    share_weights=True with a single in_feats: fc_dst is fc_src (one weight in parameters(), no fc_dst.* key of its own values), and
    the layer takes feat_dst = block.dst_rows(feat_src) -- DGL's feat_src[:num_dst], right on owner-bucketed blocks too -- instead
    of a second projection; h_dst is then not read.  Otherwise h_dst must be the destination rows of h_src: block.dst_rows(h_src).
    Initialisation: Xavier-normal with the gain of relu for fc_src.weight, fc_dst.weight and attn; biases zero.
    Attention dropout and residual connections are not provided."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, negative_slope=0.2, bias=True, share_weights=False, activation=None):
        super().__init__()
        paired = isinstance(in_feats, (tuple, list))
        in_src, in_dst = in_feats if paired else (in_feats, in_feats)
        self._num_heads, self._out_feats = num_heads, out_feats
        self.share_weights = bool(share_weights) and not paired
        self.fc_src = torch.nn.Linear(in_src, out_feats * num_heads, bias=bias)
        self.fc_dst = self.fc_src if self.share_weights else torch.nn.Linear(in_dst, out_feats * num_heads, bias=bias)
        self.attn = torch.nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.feat_drop = torch.nn.Dropout(feat_drop)
        self.negative_slope = negative_slope
        self.activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        gain = torch.nn.init.calculate_gain("relu")
        for w in (self.fc_src.weight, self.fc_dst.weight, self.attn):
            torch.nn.init.xavier_normal_(w, gain=gain)
        for b in (self.fc_src.bias, self.fc_dst.bias):
            if b is not None:
                torch.nn.init.zeros_(b)

    def forward(self, block, feat):
        h_src, h_dst = feat
        H, D = self._num_heads, self._out_feats
        feat_src = self.fc_src(self.feat_drop(h_src)).view(-1, H, D)
        if self.share_weights:
            feat_dst = block.dst_rows(feat_src)
        else:
            feat_dst = self.fc_dst(self.feat_drop(h_dst)).view(-1, H, D)
        rst = block.gatv2_aggregate(feat_src, feat_dst, self.attn, self.negative_slope)
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class GraphConv(torch.nn.Module):
    """Graph convolution with norm='both' (DGL GraphConv's default), on a block:
        out[d] = in_deg(d)^-1/2 * sum_j out_deg(s_j)^-1/2 * h_src[s_j] @ weight + bias,   then activation, if any
    with the degrees counted over the valid edges of the block and clamped to at least 1.  weight [in_feats, out_feats] (Xavier-uniform),
    bias [out_feats] (zero): DGL's names and shapes.  The projection is applied before the aggregation when in_feats > out_feats, after
    it otherwise, as DGL does.  h_dst is accepted for DGL's calling convention and unused.
    edge_weight (one value per neighbour slot, shaped like block.edata['_ID']; padding slots unread): the message is h_src[s_j] * w_j,
    DGL's rule -- the sum replaces the unweighted one and both degrees stay the unweighted counts of valid edges.
    Deviation: a destination without an in-edge gets the bias alone; DGL raises unless allow_zero_in_degree=True, and then gives the
    same row."""

    def __init__(self, in_feats, out_feats, bias=True, activation=None):
        super().__init__()
        self._in_feats, self._out_feats = in_feats, out_feats
        self.weight = torch.nn.Parameter(torch.empty(in_feats, out_feats))
        self.bias = torch.nn.Parameter(torch.empty(out_feats)) if bias else None
        self.activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.weight)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, block, feat, edge_weight=None):
        h_src = feat[0] if isinstance(feat, (tuple, list)) else feat
        out_deg = block.out_degrees().to(device=h_src.device, dtype=h_src.dtype).clamp_min(1)
        in_deg = block.in_degrees().to(device=h_src.device, dtype=h_src.dtype).clamp_min(1)
        h = h_src * out_deg.pow(-0.5).unsqueeze(-1)
        if self._in_feats > self._out_feats:
            h = h @ self.weight
        if edge_weight is None:
            rst = block.mean_aggregate(h) * in_deg.sqrt().unsqueeze(-1)   # sum * in_deg^-1/2 = mean * in_deg^1/2; 0 without in-edges
        else:
            rst = block.weighted_sum_aggregate(h, edge_weight) * in_deg.pow(-0.5).unsqueeze(-1)
        if self._in_feats <= self._out_feats:
            rst = rst @ self.weight
        if self.bias is not None:
            rst = rst + self.bias
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class SAGEConv(torch.nn.Module):
    """GraphSAGE layer on a block, with DGL SAGEConv's parameter names so that such a state_dict loads:
        'mean':  out[d] = fc_self(h_dst[d]) + fc_neigh(mean_j h_src[s_j]) + bias
        'gcn':   out[d] = fc_neigh((sum_j h_src[s_j] + h_dst[d]) / (in_deg(d) + 1)) + bias        (no fc_self)
        'pool':  out[d] = fc_self(h_dst[d]) + fc_neigh(max_j relu(fc_pool(h_src))[s_j]) + bias    (element-wise maximum)
    over the valid in-edges j of d in the block; fc_self.weight / fc_neigh.weight [out_feats, in_feats] (no bias of their own,
    Xavier-uniform with the gain of relu), bias [out_feats] (zero); 'pool' adds fc_pool.weight [in_src, in_src] (Xavier-uniform with
    the gain of relu) and fc_pool.bias [in_src].  With edge_weight (one value per neighbour slot, shaped like block.edata['_ID'])
    every message is h_src[s_j] * w_j -- relu(fc_pool(h_src))[s_j] * w_j for 'pool', whose maximum then runs in plain torch -- while the
    divisor stays the unweighted in-degree: DGL's rule.  The projection runs before the aggregation when in_feats > out_feats, as DGL
    does ('pool' always projects after it, as in DGL).  feat is h_src or (h_src, h_dst); without h_dst the destination rows are
    block.dst_rows(h_src).  A destination without an in-edge gets fc_self(h_dst) + bias ('mean', 'pool': its maximum is 0, DGL's
    reducer) or fc_neigh(h_dst) + bias ('gcn').  The maximum is Block.max_aggregate: ties give their gradient to the first edge.
    The 'lstm' aggregator, feat_drop and norm are not provided."""

    def __init__(self, in_feats, out_feats, aggregator_type="mean", bias=True, activation=None):
        super().__init__()
        if aggregator_type not in ("mean", "gcn", "pool"):
            raise ValueError(f"aggregator_type {aggregator_type!r}: 'mean', 'gcn' or 'pool'")
        in_src, in_dst = in_feats if isinstance(in_feats, (tuple, list)) else (in_feats, in_feats)
        self._in_src_feats, self._out_feats, self._aggre_type = in_src, out_feats, aggregator_type
        if aggregator_type == "pool":
            self.fc_pool = torch.nn.Linear(in_src, in_src)
        self.fc_neigh = torch.nn.Linear(in_src, out_feats, bias=False)
        if aggregator_type != "gcn":
            self.fc_self = torch.nn.Linear(in_dst, out_feats, bias=False)
        self.bias = torch.nn.Parameter(torch.empty(out_feats)) if bias else None
        self.activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        gain = torch.nn.init.calculate_gain("relu")
        if self._aggre_type == "pool":
            torch.nn.init.xavier_uniform_(self.fc_pool.weight, gain=gain)
        torch.nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)
        if self._aggre_type != "gcn":
            torch.nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, block, feat, edge_weight=None):
        h_src, h_dst = feat if isinstance(feat, (tuple, list)) else (feat, block.dst_rows(feat))
        if self._aggre_type == "pool":
            h = torch.relu(self.fc_pool(h_src))
            neigh = block.max_aggregate(h) if edge_weight is None else block.max_aggregate_torch(h, edge_weight)
            rst = self.fc_self(h_dst) + self.fc_neigh(neigh)
            if self.bias is not None:
                rst = rst + self.bias
            return rst if self.activation is None else self.activation(rst)
        lin_before = self._in_src_feats > self._out_feats
        h = self.fc_neigh(h_src) if lin_before else h_src
        deg = block.in_degrees().to(device=h.device, dtype=h.dtype).unsqueeze(-1)
        if self._aggre_type == "mean":
            if edge_weight is None:
                neigh = block.mean_aggregate(h)
            else:
                neigh = block.weighted_sum_aggregate(h, edge_weight) / deg.clamp_min(1)
            rst = self.fc_self(h_dst) + (neigh if lin_before else self.fc_neigh(neigh))
        else:
            if edge_weight is None:
                total = block.mean_aggregate(h) * deg
            else:
                total = block.weighted_sum_aggregate(h, edge_weight)
            neigh = (total + (self.fc_neigh(h_dst) if lin_before else h_dst)) / (deg + 1)
            rst = neigh if lin_before else self.fc_neigh(neigh)
        if self.bias is not None:
            rst = rst + self.bias
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class WeightedSAGEConv(torch.nn.Module):
    """The convolution of DGL's PinSAGE example (examples/pytorch/pinsage/layers.py: WeightedSAGEConv) on a block, with its parameter
    names Q and W:
        n[d] = sum_j w_j * act(Q h_src[s_j]) / max(sum_j w_j, 1)
        z[d] = act(W [n[d] || h_dst[d]]),    out[d] = z[d] / ||z[d]||_2  (a zero norm counts as 1)
    over the valid slots j of d; weights has one value per neighbour slot, shaped like block.nbr -- block.edata['weights'] of a block
    from RandomWalkNeighborSampler, the visit counts (0 on padding).  Q: Linear(in_feats, hidden_feats), W: Linear(in_feats +
    hidden_feats, out_feats), Xavier-uniform with the gain of relu and zero biases, as in the example; dropout (the example uses 0.5)
    is applied to h_src before Q and to the concatenation before W.  The weighted sum is Block.weighted_sum_aggregate, a native kernel
    with gradients; feat is h_src or (h_src, h_dst)."""

    def __init__(self, in_feats, hidden_feats, out_feats, act=torch.relu, dropout=0.0):
        super().__init__()
        self.act = act
        self.Q = torch.nn.Linear(in_feats, hidden_feats)
        self.W = torch.nn.Linear(in_feats + hidden_feats, out_feats)
        self.dropout = torch.nn.Dropout(dropout)
        self.reset_parameters()

    def reset_parameters(self):
        gain = torch.nn.init.calculate_gain("relu")
        for lin in (self.Q, self.W):
            torch.nn.init.xavier_uniform_(lin.weight, gain=gain)
            torch.nn.init.zeros_(lin.bias)

    def forward(self, block, feat, weights):
        h_src, h_dst = feat if isinstance(feat, (tuple, list)) else (feat, block.dst_rows(feat))
        w = weights.to(device=h_src.device, dtype=h_src.dtype)
        valid = (block.nbr >= 0) if block.nbr is not None else None
        n = block.weighted_sum_aggregate(self.act(self.Q(self.dropout(h_src))), w)
        if valid is None:   # ragged block: one weight per edge, summed per row
            ws = torch.zeros(block.num_dst, dtype=w.dtype, device=w.device).index_add(0, block._slots(w.device)[0], w)
        else:
            ws = (w * valid.to(device=w.device, dtype=w.dtype)).sum(1)
        z = self.act(self.W(self.dropout(torch.cat([n / ws.clamp_min(1).unsqueeze(1), h_dst], 1))))
        norm = z.norm(2, 1, keepdim=True)
        return z / torch.where(norm == 0, torch.ones_like(norm), norm)


class GINConv(torch.nn.Module):
    """Graph isomorphism layer on a block, DGL GINConv's signature and names:
        out[d] = apply_func((1 + eps) * h_dst[d] + agg_j h_src[s_j]),   then activation, if any
    over the valid in-edges j of d in the block, agg one of 'sum', 'max' (element-wise) and 'mean'.  eps has shape [1] and the name
    'eps': a buffer holding init_eps, or a parameter with learn_eps=True; apply_func (any callable, usually an MLP) is registered under
    that name when it is a module.  'sum' is Block.weighted_sum_aggregate with unit weights on the valid slots -- an exact slot-order
    sum, unlike mean * in_deg -- 'mean' is Block.mean_aggregate and 'max' is Block.max_aggregate (ties give their gradient to the first
    edge).  With edge_weight (one value per neighbour slot, shaped like block.edata['_ID']) every message is h_src[s_j] * w_j, DGL's
    u_mul_e: 'sum' takes the weights in place of the units, 'mean' divides that sum by the unweighted in-degree, and 'max' runs in
    plain torch.  feat is h_src or (h_src, h_dst); without h_dst the destination rows are block.dst_rows(h_src).  A destination
    without an in-edge gets apply_func((1 + eps) * h_dst[d]): every aggregate is 0 there, DGL's reducers."""

    def __init__(self, apply_func=None, aggregator_type="sum", init_eps=0, learn_eps=False, activation=None):
        super().__init__()
        if aggregator_type not in ("sum", "max", "mean"):
            raise ValueError(f"aggregator_type {aggregator_type!r}: 'sum', 'max' or 'mean'")
        self.apply_func = apply_func
        self._aggregator_type = aggregator_type
        self.activation = activation
        eps = torch.tensor([float(init_eps)], dtype=torch.float32)
        if learn_eps:
            self.eps = torch.nn.Parameter(eps)
        else:
            self.register_buffer("eps", eps)

    def forward(self, block, feat, edge_weight=None):
        h_src, h_dst = feat if isinstance(feat, (tuple, list)) else (feat, block.dst_rows(feat))
        if self._aggregator_type == "max":
            neigh = block.max_aggregate(h_src) if edge_weight is None else block.max_aggregate_torch(h_src, edge_weight)
        elif self._aggregator_type == "mean" and edge_weight is None:
            neigh = block.mean_aggregate(h_src)
        else:
            slots = block.indices if block.nbr is None else block.nbr
            w = edge_weight if edge_weight is not None else torch.ones(slots.shape, dtype=h_src.dtype, device=h_src.device)
            neigh = block.weighted_sum_aggregate(h_src, w)
            if self._aggregator_type == "mean":
                neigh = neigh / block.in_degrees().to(device=neigh.device, dtype=neigh.dtype).clamp_min(1).unsqueeze(-1)
        rst = (1 + self.eps) * h_dst + neigh
        if self.apply_func is not None:
            rst = self.apply_func(rst)
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class _RelWeight(torch.nn.Module):
    """The per-relation weights of RelGraphConv under DGL's name `linear_r` (dgl.nn.TypedLinear's parameters): W [num_rels, in, out],
    or with regularizer='basis' W [num_bases, in, out] and coeff [num_rels, num_bases]."""

    def __init__(self, in_feat, out_feat, num_rels, regularizer, num_bases):
        super().__init__()
        self.in_feat, self.out_feat, self.num_rels = in_feat, out_feat, num_rels
        if regularizer is None:
            self.W = torch.nn.Parameter(torch.empty(num_rels, in_feat, out_feat))
        else:
            self.W = torch.nn.Parameter(torch.empty(num_bases, in_feat, out_feat))
            self.coeff = torch.nn.Parameter(torch.empty(num_rels, num_bases))
        self.regularizer = regularizer
        self.reset_parameters()

    def reset_parameters(self):   # dgl.nn.TypedLinear.reset_parameters
        with torch.no_grad():
            bound = 1.0 / self.in_feat ** 0.5
            self.W.uniform_(-bound, bound)
            if self.regularizer == "basis":
                torch.nn.init.xavier_uniform_(self.coeff, gain=torch.nn.init.calculate_gain("relu"))

    def weight(self):
        """[num_rels, in, out]: W itself, or W_r = sum_b coeff[r, b] W[b]"""
        if self.regularizer is None:
            return self.W
        return (self.coeff @ self.W.view(self.W.shape[0], -1)).view(self.num_rels, self.in_feat, self.out_feat)


class RelGraphConv(torch.nn.Module):
    """Relational graph convolution (Schlichtkrull et al., "Modeling Relational Data with Graph Convolutional Networks") on a block,
    DGL 1.x RelGraphConv's signature: forward(block, feat, etypes, norm=None) with
        out[d] = sum_j norm_j * h_src[s_j] @ W[etypes_j]
    over the valid in-edges j of d, then, in DGL's order: layer norm, + h_bias, + h_dst[d] @ loop_weight, activation, dropout.
    feat is h_src or (h_src, h_dst); without h_dst the destination rows are block.dst_rows(h_src).  etypes (any integer dtype) and norm
    have one value per neighbour slot, shaped like block.edata['_ID'] -- e.g. block.edata['etype'] of a block sampled with
    edge_ids=True; norm is also taken as [E, 1], as DGL passes it.  An edge whose type is outside [0, num_rels) sends nothing.
    The messages are never formed: Block.rel_sum_aggregate sums norm_j * h_src[s_j] per (destination, relation) in one native kernel,
    and  out = that.view(num_dst, num_rels * in_feat) @ W.view(num_rels * in_feat, out_feat)  applies every relation's matrix in one GEMM.
    regularizer: None -- W [num_rels, in_feat, out_feat]; 'basis' -- W [num_bases, in_feat, out_feat] and coeff [num_rels, num_bases],
    W_r = sum_b coeff[r, b] W[b] (num_bases defaults to num_rels).  'bdd' is not provided.
    Parameters, with the names and shapes of DGL 1.x so that such a state_dict loads:
        linear_r.W, linear_r.coeff ('basis' only), h_bias [out_feat] (bias=True), loop_weight [in_feat, out_feat] (self_loop=True),
        layer_norm_weight.weight / layer_norm_weight.bias [out_feat] (layer_norm=True).
    The names are those of DGL's source (dgl/nn/pytorch/conv/relgraphconv.py and linear.py) as recorded; DGL is not installed where
    this was written, so no checkpoint saved by DGL has been loaded.
    Initialisation, DGL's: W uniform in +-1/sqrt(in_feat), coeff and loop_weight Xavier-uniform with the gain of relu, h_bias zero."""

    def __init__(self, in_feat, out_feat, num_rels, regularizer=None, num_bases=None, bias=True, activation=None, self_loop=True,
                 dropout=0.0, layer_norm=False):
        super().__init__()
        if isinstance(num_rels, bool) or not isinstance(num_rels, int) or not 1 <= num_rels <= 64:
            raise ValueError(f"num_rels {num_rels!r}: 1..64 relations")
        if regularizer == "bdd":
            raise ValueError("regularizer 'bdd' (block-diagonal decomposition) is not provided: None or 'basis'")
        if regularizer not in (None, "basis"):
            raise ValueError(f"regularizer {regularizer!r}: None or 'basis'")
        if regularizer == "basis":
            num_bases = num_rels if num_bases is None else int(num_bases)
            if num_bases < 1:
                raise ValueError("num_bases must be >= 1")
        self.in_feat, self.out_feat, self.num_rels = in_feat, out_feat, num_rels
        self.linear_r = _RelWeight(in_feat, out_feat, num_rels, regularizer, num_bases)
        self.h_bias = torch.nn.Parameter(torch.zeros(out_feat)) if bias else None
        self.loop_weight = torch.nn.Parameter(torch.empty(in_feat, out_feat)) if self_loop else None
        if self_loop:
            torch.nn.init.xavier_uniform_(self.loop_weight, gain=torch.nn.init.calculate_gain("relu"))
        self.layer_norm_weight = torch.nn.LayerNorm(out_feat, elementwise_affine=True) if layer_norm else None
        self.activation = activation
        self.dropout = torch.nn.Dropout(dropout)

    def forward(self, block, feat, etypes, norm=None):
        h_src, h_dst = feat if isinstance(feat, (tuple, list)) else (feat, None)
        if norm is not None and norm.dim() == etypes.dim() + 1 and norm.shape[-1] == 1:
            norm = norm.squeeze(-1)
        agg = block.rel_sum_aggregate(h_src, etypes, self.num_rels, norm)                       # [num_dst, R, in]
        W = self.linear_r.weight().to(agg.dtype)
        h = agg.reshape(agg.shape[0], self.num_rels * self.in_feat) @ W.reshape(self.num_rels * self.in_feat, self.out_feat)
        if self.layer_norm_weight is not None:
            h = self.layer_norm_weight(h)
        if self.h_bias is not None:
            h = h + self.h_bias
        if self.loop_weight is not None:
            h = h + (block.dst_rows(h_src) if h_dst is None else h_dst) @ self.loop_weight
        if self.activation is not None:
            h = self.activation(h)
        return self.dropout(h)


def _check_num_rels(num_rels):
    if isinstance(num_rels, bool) or not isinstance(num_rels, int) or not 1 <= num_rels <= 64:
        raise ValueError(f"num_rels {num_rels!r}: 1..64 relations")


def _pack_pairs(block, etype, num_rels, dev):
    """The (source, relation) pairs that occur on a valid edge of the block, sorted by relation * num_src + source so that a relation's
    pairs are contiguous: -> (rows, pair_rel, pair_src, counts).  rows (int64, one value per neighbour slot, flat) is the slot's pair,
    -1 on a padding slot and on a type outside [0, num_rels); pair_rel / pair_src [P] are every pair's relation and local source;
    counts is the number of pairs per relation as a Python list -- the one host read."""
    _, src = block._slots(dev)
    t = etype.reshape(-1).to(device=dev, dtype=torch.int64)
    keep = (src >= 0) & (t >= 0) & (t < num_rels)
    pairs, inv = torch.unique(t[keep] * block.num_src + src[keep], return_inverse=True)   # sorted: grouped by relation
    rows = torch.full_like(src, -1)
    rows[keep] = inv
    pair_rel, pair_src = pairs // block.num_src, pairs % block.num_src
    counts = torch.bincount(pair_rel, minlength=num_rels).tolist()                        # the host read
    return rows, pair_rel, pair_src, counts


class RelGATConv(torch.nn.Module):
    """Graph attention with one GATConv per edge type, summed over the types, on a homogenised block: what DGL computes with
    HeteroGraphConv({etype: GATConv(in_feats, out_feats, num_heads)}, aggregate='sum') -- the layer of the reference's RGAT model -- in
    the int in_feats form, where a GATConv has one projection `fc` and takes feat_dst = feat_src[:num_dst].

    forward(block, (h_src, h_dst), etype) -> [num_dst, H, D]; etype (any integer dtype) has one value per neighbour slot, shaped like
    block.edata['_ID'].  For destination d, head h, relation r and the valid in-edges j of d with etype_j == r (source s_j):
        f_r(x) = (fc_weight[r] @ x).view(H, D);   el_j = <f_r(h_src[s_j])[h], attn_l[r, h]>;   er = <f_r(h_dst[d])[h], attn_r[r, h]>
        a_j = softmax over those j of leaky_relu(el_j + er, negative_slope)
        out[d, h, :] = sum_r (sum_j a_j f_r(h_src[s_j])[h, :] + bias[r].view(H, D)[h]);   then activation, if any
    Every relation's bias is added to every destination, as with DGL's allow_zero_in_degree=True, where a GATConv gives a node without
    in-edges its bias.  An edge whose type is outside [0, num_rels) sends nothing.  h_dst must be block.dst_rows(h_src).
    Parameters, stacked over the relations: fc_weight [R, H * D, in_feats], attn_l [R, H, D], attn_r [R, H, D], bias [R, H * D]; slice
    r holds fc.weight, attn_l[0], attn_r[0] and bias of relation r's DGL GATConv (from_gatconvs shows the mapping), and is initialised
    as GATConv.reset_parameters does: Xavier-normal with the gain of relu, bias zero.
    The projection does not cost R times the source rows: only the (source, relation) pairs that occur on a valid edge are projected,
    one GEMM per relation on its slice of the pairs (sorted by etype * num_src + src, so a relation's pairs are contiguous), and
    Block.rel_gat_aggregate reads them in its packed form.  The per-relation pair counts cost one host read per layer call, and the packed form's row check a second.  The
    destination side is one [num_dst, in] x [in, R * H] GEMM with the vectors fc_weight[r, h]^T attn_r[r, h].
    One difference from DGL: HeteroGraphConv skips a relation that has no edge anywhere in the block, bias included; this layer adds
    every relation's bias always.  Attention dropout and residual connections are not provided."""

    def __init__(self, in_feats, out_feats, num_heads, num_rels, feat_drop=0.0, negative_slope=0.2, bias=True, activation=None):
        super().__init__()
        _check_num_rels(num_rels)
        self._in_feats, self._out_feats, self._num_heads, self.num_rels = in_feats, out_feats, num_heads, num_rels
        self.fc_weight = torch.nn.Parameter(torch.empty(num_rels, num_heads * out_feats, in_feats))
        self.attn_l = torch.nn.Parameter(torch.empty(num_rels, num_heads, out_feats))
        self.attn_r = torch.nn.Parameter(torch.empty(num_rels, num_heads, out_feats))
        self.bias = torch.nn.Parameter(torch.empty(num_rels, num_heads * out_feats)) if bias else None
        self.feat_drop = torch.nn.Dropout(feat_drop)
        self.negative_slope = negative_slope
        self.activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        gain = torch.nn.init.calculate_gain("relu")
        with torch.no_grad():
            for r in range(self.num_rels):   # a slice at a time: the fans are those of one GATConv's fc [H * D, in] and attn [1, H, D]
                torch.nn.init.xavier_normal_(self.fc_weight[r], gain=gain)
                torch.nn.init.xavier_normal_(self.attn_l[r:r + 1], gain=gain)
                torch.nn.init.xavier_normal_(self.attn_r[r:r + 1], gain=gain)
            if self.bias is not None:
                self.bias.zero_()

    @classmethod
    def from_gatconvs(cls, convs, activation=None):
        """The layer that computes sum_r convs[r] on relation r's edges, from R COALA_GNN.nn.GATConv modules whose fc_src and fc_dst
        hold the same weights (DGL's single `fc`): fc_weight[r] = fc_src.weight, attn_l[r] = attn_l[0], attn_r[r] = attn_r[0],
        bias[r] = bias.  The parameters are copied."""
        convs = list(convs)
        c0 = convs[0]
        for c in convs:
            if not torch.equal(c.fc_src.weight, c.fc_dst.weight):
                raise ValueError("from_gatconvs takes GATConv modules whose fc_src and fc_dst hold the same weights")
            if (tuple(c.fc_src.weight.shape), c._num_heads, c.bias is None) != (tuple(c0.fc_src.weight.shape), c0._num_heads, c0.bias is None):
                raise ValueError("from_gatconvs takes GATConv modules of one shape")
        layer = cls(c0.fc_src.in_features, c0._out_feats, c0._num_heads, len(convs), feat_drop=c0.feat_drop.p,
                    negative_slope=c0.negative_slope, bias=c0.bias is not None, activation=activation)
        layer.to(device=c0.attn_l.device, dtype=c0.attn_l.dtype)
        with torch.no_grad():
            for r, c in enumerate(convs):
                layer.fc_weight[r] = c.fc_src.weight
                layer.attn_l[r] = c.attn_l[0]
                layer.attn_r[r] = c.attn_r[0]
                if c.bias is not None:
                    layer.bias[r] = c.bias
        return layer

    def forward(self, block, feat, etype):
        h_src, h_dst = feat
        R, H, D = self.num_rels, self._num_heads, self._out_feats
        h_src, h_dst = self.feat_drop(h_src), self.feat_drop(h_dst)
        rows, pair_rel, pair_src, counts = _pack_pairs(block, etype, R, h_src.device)
        parts, off = [], 0
        for r, c in enumerate(counts):
            if c:
                parts.append(h_src[pair_src[off:off + c]] @ self.fc_weight[r].t())
                off += c
        feat_pairs = (torch.cat(parts) if parts else h_src.new_zeros((0, H * D))).view(-1, H, D)
        el = (feat_pairs * self.attn_l[pair_rel]).sum(-1)
        w_r = (self.fc_weight.view(R, H, D, -1) * self.attn_r.unsqueeze(-1)).sum(2)           # [R, H, in]: fc_weight[r, h]^T attn_r[r, h]
        er = (h_dst @ w_r.view(R * H, -1).t()).view(-1, R, H)
        rst = block.rel_gat_aggregate(el, er, feat_pairs, etype, R, rows=rows.view(etype.shape), negative_slope=self.negative_slope)
        if self.bias is not None:
            rst = rst + self.bias.sum(0).view(1, H, D)
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class RelSAGEConv(torch.nn.Module):
    """GraphSAGE 'gcn' with one SAGEConv per edge type, summed over the types, on a homogenised block: what DGL computes with
    HeteroGraphConv({etype: SAGEConv(in_feats, out_feats, 'gcn')}, aggregate='sum'), the layer of the reference's RSAGE model.

    forward(block, feat, etype) -> [num_dst, out_feats]; feat is h_src or (h_src, h_dst) -- without h_dst the destination rows are
    block.dst_rows(h_src) -- and etype (any integer dtype) has one value per neighbour slot, shaped like block.edata['_ID']:
        h_neigh[d, r] = (sum over d's valid in-edges j of type r of h_src[s_j] + h_dst[d]) / (c[d, r] + 1)
        out[d] = sum_r (fc_neigh_weight[r] @ h_neigh[d, r] + bias[r]);   then activation, if any
    with c[d, r] the number of those edges (Block.rel_in_degrees).  No fc_self, as in SAGEConv 'gcn'; a relation without an edge at d
    sends fc_neigh_weight[r] @ h_dst[d] + bias[r], SAGEConv's row for a node without in-edges.  An edge whose type is outside
    [0, num_rels) sends nothing.  The sums are Block.rel_sum_aggregate, a native kernel, and all R matrices are applied in one GEMM:
    h_neigh viewed as [num_dst, R * in] times the weights viewed as [R * in, out].
    Parameters, stacked over the relations: fc_neigh_weight [R, out_feats, in_feats] (slice r is fc_neigh.weight of relation r's
    SAGEConv; Xavier-uniform with the gain of relu, per slice) and bias [R, out_feats] (zero).
    As RelGATConv, and unlike DGL's HeteroGraphConv, it does not skip a relation that has no edge anywhere in the block."""

    def __init__(self, in_feats, out_feats, num_rels, bias=True, activation=None):
        super().__init__()
        _check_num_rels(num_rels)
        self._in_feats, self._out_feats, self.num_rels = in_feats, out_feats, num_rels
        self.fc_neigh_weight = torch.nn.Parameter(torch.empty(num_rels, out_feats, in_feats))
        self.bias = torch.nn.Parameter(torch.empty(num_rels, out_feats)) if bias else None
        self.activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        gain = torch.nn.init.calculate_gain("relu")
        with torch.no_grad():
            for r in range(self.num_rels):
                torch.nn.init.xavier_uniform_(self.fc_neigh_weight[r], gain=gain)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, block, feat, etype):
        h_src, h_dst = feat if isinstance(feat, (tuple, list)) else (feat, block.dst_rows(feat))
        R = self.num_rels
        z = block.rel_sum_aggregate(h_src, etype, R)                                           # [num_dst, R, in]
        c = block.rel_in_degrees(etype, R).to(device=z.device, dtype=z.dtype)
        h_neigh = (z + h_dst.unsqueeze(1)) / (c + 1).unsqueeze(-1)
        rst = h_neigh.reshape(z.shape[0], R * self._in_feats) @ self.fc_neigh_weight.transpose(1, 2).reshape(R * self._in_feats, self._out_feats)
        if self.bias is not None:
            rst = rst + self.bias.sum(0)
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class DotGatConv(torch.nn.Module):
    """Dot-product attention layer (DGL 1.x DotGatConv; PyG's TransformerConv without edge features, bias, root weight and a separate
    value projection).  forward(block, feat) -> [num_dst, H, out_feats]; feat is h_src or (h_src, h_dst) -- without h_dst the destination
    rows are block.dst_rows(h_src).  For destination d, head h and the valid in-edges j of d (source s_j):
        q = fc_dst(h_dst).view(-1, H, D);   k = v = fc_src(h_src).view(-1, H, D)
        a_j = softmax over d's in-edges of <q[d, h], k[s_j, h]> / sqrt(D);   out[d, h, :] = sum_j a_j v[s_j, h, :]
    A destination without an in-edge gets zeros (DGL's allow_zero_in_degree=True).  Parameters, DGL's names and shapes: fc.weight
    [H * D, in_feats] for an int in_feats (one projection for both sides), fc_src.weight [H * D, in_src] and fc_dst.weight
    [H * D, in_dst] for a pair; no bias.  Initialisation: torch.nn.Linear's default, as in DGL.  The attention step is
    Block.dot_gat_aggregate, a native kernel.  get_attention is not provided."""

    def __init__(self, in_feats, out_feats, num_heads):
        super().__init__()
        self._num_heads, self._out_feats = num_heads, out_feats
        if isinstance(in_feats, (tuple, list)):
            self.fc_src = torch.nn.Linear(in_feats[0], out_feats * num_heads, bias=False)
            self.fc_dst = torch.nn.Linear(in_feats[1], out_feats * num_heads, bias=False)
        else:
            self.fc = torch.nn.Linear(in_feats, out_feats * num_heads, bias=False)

    def forward(self, block, feat):
        h_src, h_dst = feat if isinstance(feat, (tuple, list)) else (feat, None)
        H, D = self._num_heads, self._out_feats
        fc_src, fc_dst = (self.fc, self.fc) if hasattr(self, "fc") else (self.fc_src, self.fc_dst)
        k = fc_src(h_src).view(-1, H, D)
        if h_dst is None:
            q = block.dst_rows(k) if fc_dst is fc_src else fc_dst(block.dst_rows(h_src)).view(-1, H, D)
        else:
            q = fc_dst(h_dst).view(-1, H, D)
        return block.dot_gat_aggregate(q, k, k, scale=float(D) ** -0.5)


def _typed_linear(x, W, types, counts):
    """x[i] @ W[types[i]] for x [N, in], W [T, in, out]: one GEMM per type on its slice of the rows sorted by type.  counts: rows per type,
    a Python list (the caller's host read)."""
    if W.shape[0] == 1:
        return x @ W[0]
    order = torch.argsort(types, stable=True)
    xs = x[order]
    parts, off = [], 0
    for t, c in enumerate(counts):
        if c:
            parts.append(xs[off:off + c] @ W[t])
            off += c
    ys = torch.cat(parts) if parts else x.new_zeros((0, W.shape[2]))
    back = torch.empty_like(order)
    back[order] = torch.arange(order.numel(), device=order.device)
    return ys[back]


class HGTConv(torch.nn.Module):
    """Heterogeneous Graph Transformer layer (Hu et al., "Heterogeneous Graph Transformer"; DGL 1.x HGTConv) on a homogenised block:
    one id space, an integer type per node and per edge.

    forward(block, x, ntype, etype) -> [num_dst, H * D], H = num_heads, D = head_size.  x is h_src or (h_src, h_dst) -- without h_dst the
    destination rows are block.dst_rows(h_src); ntype [num_src] (any integer dtype) is the type of every source node in the block's
    source order (the destinations' types are block.dst_rows(ntype)); etype (any integer dtype) has one value per neighbour slot,
    shaped like block.edata['_ID'].  For destination d and the valid in-edges j of d (source s_j, type r_j), tau(.) a node's type:
        K = x_s @ k_weight[tau(s)],  V = x_s @ v_weight[tau(s)],  Q = x_d @ q_weight[tau(d)],  each viewed as [H, D]
        e_j[h] = (K[s_j, h] @ rel_att[r_j, h]) . Q[d, h] * rel_pri[r_j, h] / sqrt(D);   a = softmax of e over all of d's in-edges
        m[d, h] = sum_j a_j[h] (V[s_j, h] @ rel_msg[r_j, h])
        y = dropout(m.view(H * D) @ a_weight[tau(d)]);   alpha = sigmoid(skip[tau(d)])
        out = y * alpha + (x_d if in_size == H * D else x_d @ residual_w) * (1 - alpha);   then LayerNorm, if use_norm
    An edge whose type is outside [0, num_etypes) sends nothing; a destination without an edge has m = 0, so the skip path alone remains;
    a node type outside [0, num_ntypes) raises ValueError.
    Parameters, stacked: k_weight, q_weight, v_weight [T, in_size, H * D]; a_weight [T, H * D, H * D]; rel_att, rel_msg [R, H, D, D];
    rel_pri [R, H] (ones); skip [T] (ones); residual_w [in_size, H * D] only when in_size != H * D (Xavier-uniform); norm.weight /
    norm.bias with use_norm.  The typed weights are initialised as DGL's TypedLinear does, uniform in +-1/sqrt(fan-in) per slice.
    DGL is not installed where this was written.  The correspondence to DGL's names, written from memory of its source
    (dgl/nn/pytorch/conv/hgtconv.py) and not checked against a checkpoint: k_weight = linear_k.W, q_weight = linear_q.W, v_weight =
    linear_v.W, a_weight = linear_a.W; rel_att[:, h] = relation_att.{h}.W, rel_msg[:, h] = relation_msg.{h}.W ([R, D, D] each);
    rel_pri[:, h] = relation_pri.{h} ([R]); skip, residual_w and norm.* keep their names.
    How it runs: the typed linears are one GEMM per node type on a sorted slice.  The D x D relation matrices are applied per (source,
    relation) pair that occurs on a valid edge -- P <= E rows, RelGATConv's packing -- not per edge: per relation one batched matmul
    over the heads for K and one for V, on that relation's slice of the pairs, with rel_pri[r, h] / sqrt(D) folded into rel_att[r, h]
    (the score is linear in K).  One Block.dot_gat_aggregate call in its packed form then does the softmax over all of a node's
    in-edges and the weighted sum, in a native kernel that needs no edge types.  Host reads per call: the node counts per type (source
    and destination side together, one read; they also carry the range check) and the pair counts per relation (one read).
    Attention dropout is not provided."""

    def __init__(self, in_size, head_size, num_heads, num_ntypes, num_etypes, dropout=0.2, use_norm=False):
        super().__init__()
        for name, n in (("num_ntypes", num_ntypes), ("num_etypes", num_etypes)):
            if isinstance(n, bool) or not isinstance(n, int) or n < 1:
                raise ValueError(f"{name} {n!r}: at least one type")
        self.in_size, self.head_size, self.num_heads = in_size, head_size, num_heads
        self.num_ntypes, self.num_etypes = num_ntypes, num_etypes
        T, R, H, D = num_ntypes, num_etypes, num_heads, head_size
        P = torch.nn.Parameter
        self.k_weight, self.q_weight, self.v_weight = (P(torch.empty(T, in_size, H * D)) for _ in range(3))
        self.a_weight = P(torch.empty(T, H * D, H * D))
        self.rel_att, self.rel_msg = P(torch.empty(R, H, D, D)), P(torch.empty(R, H, D, D))
        self.rel_pri = P(torch.ones(R, H))
        self.skip = P(torch.ones(T))
        self.residual_w = P(torch.empty(in_size, H * D)) if in_size != H * D else None
        self.drop = torch.nn.Dropout(dropout)
        self.norm = torch.nn.LayerNorm(H * D) if use_norm else None
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            for w in (self.k_weight, self.q_weight, self.v_weight, self.a_weight, self.rel_att, self.rel_msg):
                bound = 1.0 / w.shape[-2] ** 0.5            # dgl.nn.TypedLinear.reset_parameters: the same bound for every slice
                w.uniform_(-bound, bound)
            self.rel_pri.fill_(1.0)
            self.skip.fill_(1.0)
            if self.residual_w is not None:
                torch.nn.init.xavier_uniform_(self.residual_w)

    def forward(self, block, x, ntype, etype):
        h_src, h_dst = x if isinstance(x, (tuple, list)) else (x, block.dst_rows(x))
        T, R, H, D = self.num_ntypes, self.num_etypes, self.num_heads, self.head_size
        dev = h_src.device
        if not isinstance(ntype, torch.Tensor) or ntype.is_floating_point() or ntype.is_complex() or ntype.dtype == torch.bool:
            raise ValueError("node types must be an integer tensor")
        if tuple(ntype.shape) != (block.num_src,):
            raise ValueError(f"node types of shape {tuple(ntype.shape)}: this block takes one per source node, ({block.num_src},)")
        nt_src = ntype.to(device=dev, dtype=torch.int64)
        nt_dst = block.dst_rows(nt_src)
        binned = [torch.bincount(torch.where((t < 0) | (t >= T), T, t), minlength=T + 1) for t in (nt_src, nt_dst)]
        cnt = torch.cat(binned).tolist()                                                     # host read 1: nodes per type
        cnt_src, cnt_dst = cnt[:T], cnt[T + 1: 2 * T + 1]
        if cnt[T] or cnt[2 * T + 1]:
            raise ValueError(f"node types must lie in [0, {T}) (num_ntypes={T})")
        k = _typed_linear(h_src, self.k_weight, nt_src, cnt_src).view(-1, H, D)
        v = _typed_linear(h_src, self.v_weight, nt_src, cnt_src).view(-1, H, D)
        q = _typed_linear(h_dst, self.q_weight, nt_dst, cnt_dst).view(-1, H, D)
        rows, pair_rel, pair_src, counts = _pack_pairs(block, etype, R, dev)                 # host read 2: pairs per relation
        att = self.rel_att * (self.rel_pri * (float(D) ** -0.5)).view(R, H, 1, 1)            # the prior and 1 / sqrt(D), folded in
        k_parts, v_parts, off = [], [], 0
        for r, c in enumerate(counts):
            if c:
                s = pair_src[off:off + c]
                k_parts.append(torch.bmm(k[s].transpose(0, 1), att[r]).transpose(0, 1))       # [c, H, D]
                v_parts.append(torch.bmm(v[s].transpose(0, 1), self.rel_msg[r]).transpose(0, 1))
                off += c
        k_pairs = torch.cat(k_parts) if k_parts else k.new_zeros((0, H, D))
        v_pairs = torch.cat(v_parts) if v_parts else v.new_zeros((0, H, D))
        m = block.dot_gat_aggregate(q, k_pairs, v_pairs, rows=rows.to(torch.int32).view(etype.shape), scale=1.0, validate=False)
        y = self.drop(_typed_linear(m.reshape(-1, H * D), self.a_weight, nt_dst, cnt_dst))
        alpha = torch.sigmoid(self.skip[nt_dst]).unsqueeze(-1)
        res = h_dst if self.residual_w is None else h_dst @ self.residual_w
        out = y * alpha + res * (1 - alpha)
        return out if self.norm is None else self.norm(out)


class DotPredictor(torch.nn.Module):
    """The score of a node pair is the dot product of the two embeddings: DGL's link-prediction predictor (apply_edges(fn.u_dot_v) on a
    pair graph), on block_ops.pair_dot.  h [N, D] -> [P], h [N, H, D] -> [P, H]; a pair with an index < 0 scores 0.  validate=False
    skips pair_dot's host read of the largest index, for pairs that address h by construction (an EdgeBatch's)."""

    def __init__(self, validate=True):
        super().__init__()
        self.validate = bool(validate)

    def forward(self, h, src, dst):
        from .block_ops import pair_dot
        return pair_dot(h, src, dst, validate=self.validate)
