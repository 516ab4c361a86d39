"""Autograd wrappers of the native block ops that `Block` (sampler.py) hands to a model: mean aggregation (SAGEConv's "mean"), weighted
sum aggregation (DGL's u_mul_e_sum, the edge_weight= path of GraphConv / SAGEConv), max aggregation (DGL's fn.max: SAGEConv's "pool",
GINConv's "max"), the relation-typed sum (RelGraphConv's message step), GAT / GATv2 attention aggregation, scaled dot-product
attention (DotGatConv's and HGTConv's message step) and relation-typed GAT attention (RelGATConv's message step), on fixed blocks and on the ragged CSR blocks of full layers.  pair_dot (DGL's u_dot_v on a pair graph: a link predictor's scores) is the one op here
that takes no block.  One kernel forward, one backward each; the kernels are in coala-gnn_amd/csrc/coala_block_ops.hip
(C ABI: coala_block_*).  Every op has one forward and one backward body for both block forms, which take the C entry and the block's
index tensors -- (nbr,) or (indptr, indices); the two Function classes of an op are shells that name the entries, and they stay two
because Block's callers and the tests tell by the class which form ran."""
import torch

from COALA_GNN_Pybind import _capi, current_stream

_lib = _capi.load()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _block(index):
    """How a C entry takes a block with the index tensors (nbr,) or (indptr, indices): -> (their pointers, which lead the arguments;
    n_dst; what stands between n_dst and the row width: the fan-out of the fixed form, nothing for CSR)."""
    if len(index) == 1:
        return (index[0].data_ptr(),), index[0].shape[0], (index[0].shape[1],)
    return (index[0].data_ptr(), index[1].data_ptr()), index[0].numel() - 1, ()


def _mean_forward(ctx, h_src, entry, index):
    """out[d] = mean of the rows h_src[s] over row d's valid entries (coala_block_mean_aggregate[_csr])."""
    h = h_src.contiguous()
    idx, n_dst, fan = _block(index)
    out = torch.empty((n_dst, h.shape[1]), dtype=torch.float32, device=h.device)
    _capi.check(entry(h.device.index or 0, *idx, h.data_ptr(), out.data_ptr(), n_dst, *fan, h.shape[1], current_stream()))
    ctx.save_for_backward(*index)
    ctx.src_shape = h.shape
    return out


def _mean_backward(ctx, grad_out, entry):
    if not ctx.needs_input_grad[0]:
        return None
    idx, n_dst, fan = _block(ctx.saved_tensors)
    g = grad_out.contiguous()
    grad_src = torch.zeros(ctx.src_shape, dtype=torch.float32, device=g.device)
    _capi.check(entry(g.device.index or 0, *idx, g.data_ptr(), grad_src.data_ptr(), n_dst, *fan, g.shape[1], current_stream()))
    return grad_src


class _MeanAggregate(torch.autograd.Function):
    """out[d] = mean of h_src[nbr[d, j]] over the valid j (coala_block_mean_aggregate): one kernel forward, one backward."""

    @staticmethod
    def forward(ctx, h_src, nbr):
        return _mean_forward(ctx, h_src, _lib.coala_block_mean_aggregate, (nbr,))

    @staticmethod
    def backward(ctx, grad_out):
        return _mean_backward(ctx, grad_out, _lib.coala_block_mean_aggregate_backward), None


class _MeanAggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_mean_aggregate_csr): row d averages h_src[indices[indptr[d]:indptr[d+1]]]."""

    @staticmethod
    def forward(ctx, h_src, indptr, indices):
        return _mean_forward(ctx, h_src, _lib.coala_block_mean_aggregate_csr, (indptr, indices))

    @staticmethod
    def backward(ctx, grad_out):
        return _mean_backward(ctx, grad_out, _lib.coala_block_mean_aggregate_csr_backward), None, None


def _weighted_forward(ctx, h_src, w, entry, index):
    """out[d] = sum over row d's valid entries of w * h_src[s], w laid out like the block's index array (coala_block_weighted_sum[_csr])."""
    h, w = h_src.contiguous(), w.contiguous()
    idx, n_dst, fan = _block(index)
    out = torch.empty((n_dst, h.shape[1]), dtype=torch.float32, device=h.device)
    _capi.check(entry(h.device.index or 0, *idx, w.data_ptr(), h.data_ptr(), out.data_ptr(), n_dst, *fan, h.shape[1], current_stream()))
    ctx.save_for_backward(h, w, *index)
    return out


def _weighted_backward(ctx, grad_out, entry):
    """grad_src and grad_w in one launch; a gradient nobody asked for is neither computed nor allocated."""
    need_src, need_w = ctx.needs_input_grad[:2]
    if not need_src and not need_w:
        return None, None
    h, w, *index = ctx.saved_tensors
    idx, n_dst, fan = _block(index)
    g = grad_out.contiguous()
    grad_src = torch.zeros_like(h) if need_src else None
    grad_w = torch.empty_like(w) if need_w else None
    _capi.check(entry(g.device.index or 0, *idx, w.data_ptr(), h.data_ptr(), g.data_ptr(), _ptr(grad_src), _ptr(grad_w), n_dst, *fan, g.shape[1],
                      current_stream()))
    return grad_src, grad_w


class _WeightedSum(torch.autograd.Function):
    """out[d] = sum over the valid j of w[d, j] * h_src[nbr[d, j]] (coala_block_weighted_sum): one kernel forward, one backward that
    gives grad_src and grad_w together."""

    @staticmethod
    def forward(ctx, h_src, w, nbr):
        return _weighted_forward(ctx, h_src, w, _lib.coala_block_weighted_sum, (nbr,))

    @staticmethod
    def backward(ctx, grad_out):
        return _weighted_backward(ctx, grad_out, _lib.coala_block_weighted_sum_backward) + (None,)


class _WeightedSumCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_weighted_sum_csr): row d sums w[e] * h_src[indices[e]] over e in indptr[d]:indptr[d+1]."""

    @staticmethod
    def forward(ctx, h_src, w, indptr, indices):
        return _weighted_forward(ctx, h_src, w, _lib.coala_block_weighted_sum_csr, (indptr, indices))

    @staticmethod
    def backward(ctx, grad_out):
        return _weighted_backward(ctx, grad_out, _lib.coala_block_weighted_sum_csr_backward) + (None,) * 2


def _rel_forward(ctx, h_src, w, etype, num_rels, entry, index):
    """out[d, r] = sum over row d's valid entries of type r of w * h_src[s] (coala_block_rel_sum[_csr]): [n_dst, R, dim]; etype and w are
    laid out like the block's index array.  w None: unit weights (a null pointer), and no grad_w."""
    h = h_src.contiguous()
    w = w.contiguous() if w is not None else None
    idx, n_dst, fan = _block(index)
    out = torch.empty((n_dst, num_rels, h.shape[1]), dtype=torch.float32, device=h.device)
    _capi.check(entry(h.device.index or 0, *idx, etype.data_ptr(), _ptr(w), h.data_ptr(), out.data_ptr(), n_dst, *fan, num_rels, h.shape[1],
                      current_stream()))
    ctx.save_for_backward(h, etype, *index, *((w,) if w is not None else ()))
    ctx.has_w = w is not None
    return out


def _rel_backward(ctx, grad_out, entry):
    """grad_src and grad_w in one launch (coala_block_rel_sum[_csr]_backward); a gradient nobody asked for is neither computed nor
    allocated."""
    h, etype, *index = ctx.saved_tensors
    w = index.pop() if ctx.has_w else None
    need_src, need_w = ctx.needs_input_grad[0], w is not None and ctx.needs_input_grad[1]
    if not need_src and not need_w:
        return None, None
    idx, n_dst, fan = _block(index)
    g = grad_out.contiguous()
    grad_src = torch.zeros_like(h) if need_src else None
    grad_w = torch.empty_like(w) if need_w else None
    _capi.check(entry(g.device.index or 0, *idx, etype.data_ptr(), _ptr(w), h.data_ptr(), g.data_ptr(), _ptr(grad_src), _ptr(grad_w), n_dst, *fan,
                      g.shape[1], g.shape[2], current_stream()))
    return grad_src, grad_w


class _RelSum(torch.autograd.Function):
    """out[d, r] = sum over the valid j with etype[d, j] == r of w[d, j] * h_src[nbr[d, j]] (coala_block_rel_sum): one kernel forward,
    one backward that gives grad_src and grad_w together."""

    @staticmethod
    def forward(ctx, h_src, w, nbr, etype, num_rels):
        return _rel_forward(ctx, h_src, w, etype, num_rels, _lib.coala_block_rel_sum, (nbr,))

    @staticmethod
    def backward(ctx, grad_out):
        return _rel_backward(ctx, grad_out, _lib.coala_block_rel_sum_backward) + (None,) * 3


class _RelSumCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_rel_sum_csr): etype and w have one value per entry of indices."""

    @staticmethod
    def forward(ctx, h_src, w, indptr, indices, etype, num_rels):
        return _rel_forward(ctx, h_src, w, etype, num_rels, _lib.coala_block_rel_sum_csr, (indptr, indices))

    @staticmethod
    def backward(ctx, grad_out):
        return _rel_backward(ctx, grad_out, _lib.coala_block_rel_sum_csr_backward) + (None,) * 4


def _max_forward(ctx, h_src, entry, index):
    """out[d, c] = max of h_src[s, c] over row d's valid entries, ties to the first slot (coala_block_max_aggregate[_csr]).  The kernel
    also saves the winning source of every element, which is skipped when h_src needs no gradient."""
    h = h_src.contiguous()
    idx, n_dst, fan = _block(index)
    out = torch.empty((n_dst, h.shape[1]), dtype=torch.float32, device=h.device)
    arg = torch.empty((n_dst, h.shape[1]), dtype=torch.int32, device=h.device) if ctx.needs_input_grad[0] else None
    _capi.check(entry(h.device.index or 0, *idx, h.data_ptr(), out.data_ptr(), _ptr(arg), n_dst, *fan, h.shape[1], current_stream()))
    if arg is not None:
        ctx.save_for_backward(arg)
    ctx.src_shape = h.shape
    return out


def _max_backward(ctx, grad_out):
    """grad_src[arg[d, c], c] += grad_out[d, c] (coala_block_max_aggregate_backward): one kernel for both block forms."""
    (arg,) = ctx.saved_tensors
    g = grad_out.contiguous()
    grad_src = torch.zeros(ctx.src_shape, dtype=torch.float32, device=g.device)
    _capi.check(_lib.coala_block_max_aggregate_backward(g.device.index or 0, arg.data_ptr(), g.data_ptr(), grad_src.data_ptr(), arg.shape[0],
                                                        arg.shape[1], current_stream()))
    return grad_src


class _MaxAggregate(torch.autograd.Function):
    """out[d, c] = max of h_src[nbr[d, j], c] over the valid j (coala_block_max_aggregate): one kernel forward, one backward."""

    @staticmethod
    def forward(ctx, h_src, nbr):
        return _max_forward(ctx, h_src, _lib.coala_block_max_aggregate, (nbr,))

    @staticmethod
    def backward(ctx, grad_out):
        return _max_backward(ctx, grad_out), None


class _MaxAggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_max_aggregate_csr): row d takes the maximum over h_src[indices[indptr[d]:indptr[d+1]]]."""

    @staticmethod
    def forward(ctx, h_src, indptr, indices):
        return _max_forward(ctx, h_src, _lib.coala_block_max_aggregate_csr, (indptr, indices))

    @staticmethod
    def backward(ctx, grad_out):
        return _max_backward(ctx, grad_out), None, None


def _gat_forward(ctx, el, er, feat_src, entry, index, negative_slope):
    """Per head, a softmax of leaky_relu(el[s] + er[d]) over row d's valid entries, then the weighted sum of feat_src[s]
    (coala_block_gat_aggregate[_csr]).  out and the log-sum-exp per (row, head) are the state of the backward."""
    el, er, f = el.contiguous(), er.contiguous(), feat_src.contiguous()
    idx, n_dst, fan = _block(index)
    H, D = f.shape[1], f.shape[2]
    out = torch.empty((n_dst, H, D), dtype=torch.float32, device=f.device)
    lse = torch.empty((n_dst, H), dtype=torch.float32, device=f.device)
    _capi.check(entry(f.device.index or 0, *idx, el.data_ptr(), er.data_ptr(), f.data_ptr(), out.data_ptr(), lse.data_ptr(), n_dst, *fan, H, D,
                      negative_slope, current_stream()))
    ctx.save_for_backward(el, er, f, out, lse, *index)
    ctx.slope = negative_slope
    return out


def _gat_backward(ctx, grad_out, entry):
    """-> (grad_el, grad_er, grad_feat), one launch."""
    el, er, f, out, lse, *index = ctx.saved_tensors
    idx, n_dst, fan = _block(index)
    g = grad_out.contiguous()
    grad_feat, grad_el, grad_er = torch.zeros_like(f), torch.zeros_like(el), torch.empty_like(er)
    _capi.check(entry(f.device.index or 0, *idx, el.data_ptr(), er.data_ptr(), f.data_ptr(), out.data_ptr(), lse.data_ptr(), g.data_ptr(),
                      grad_feat.data_ptr(), grad_el.data_ptr(), grad_er.data_ptr(), n_dst, *fan, f.shape[1], f.shape[2], ctx.slope,
                      current_stream()))
    return grad_el, grad_er, grad_feat


class _GatAggregate(torch.autograd.Function):
    """DGL GATConv's attention step on a fixed block (coala_block_gat_aggregate): one kernel forward, one backward (gradients for el, er
    and feat_src)."""

    @staticmethod
    def forward(ctx, el, er, feat_src, nbr, negative_slope):
        return _gat_forward(ctx, el, er, feat_src, _lib.coala_block_gat_aggregate, (nbr,), negative_slope)

    @staticmethod
    def backward(ctx, grad_out):
        return _gat_backward(ctx, grad_out, _lib.coala_block_gat_aggregate_backward) + (None,) * 2


class _GatAggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_gat_aggregate_csr): row d's edges are indices[indptr[d]:indptr[d+1]]."""

    @staticmethod
    def forward(ctx, el, er, feat_src, indptr, indices, negative_slope):
        return _gat_forward(ctx, el, er, feat_src, _lib.coala_block_gat_aggregate_csr, (indptr, indices), negative_slope)

    @staticmethod
    def backward(ctx, grad_out):
        return _gat_backward(ctx, grad_out, _lib.coala_block_gat_aggregate_csr_backward) + (None,) * 3


def _gatv2_parts(n_dst):
    """Rows of the grad_attn partials buffer, which is also the backward's grid: one block per four destination rows, 1024 at the most."""
    return max(1, min(-(-n_dst // 4), 1024))


def _gatv2_forward(ctx, feat_src, feat_dst, attn, entry, index, negative_slope):
    """Per head, a softmax over row d's valid entries of sum_c attn[h, c] leaky_relu(feat_src[s, h, c] + feat_dst[d, h, c]), then the
    weighted sum of feat_src[s] (coala_block_gatv2_aggregate[_csr]); no [E, H, D] intermediate.  lse is the state of the backward alone:
    it is computed, but not kept, when nothing needs a gradient."""
    fs, fd, at = feat_src.contiguous(), feat_dst.contiguous(), attn.contiguous()
    idx, n_dst, fan = _block(index)
    H, D = fs.shape[1], fs.shape[2]
    out = torch.empty((n_dst, H, D), dtype=torch.float32, device=fs.device)
    lse = torch.empty((n_dst, H), dtype=torch.float32, device=fs.device)
    _capi.check(entry(fs.device.index or 0, *idx, fs.data_ptr(), fd.data_ptr(), at.data_ptr(), out.data_ptr(), lse.data_ptr(), n_dst, *fan, H, D,
                      negative_slope, current_stream()))
    if any(ctx.needs_input_grad[:3]):
        ctx.save_for_backward(fs, fd, at, out, lse, *index)
    ctx.slope = negative_slope
    return out


def _gatv2_backward(ctx, grad_out, entry):
    """All three gradients in one launch (coala_block_gatv2_aggregate[_csr]_backward); a gradient nobody asked for is neither computed
    nor allocated.  grad_attn comes as [parts, H * D] partial sums, one row per block of the launch, and is their sum over dim 0."""
    need_src, need_dst, need_attn = ctx.needs_input_grad[:3]
    if not (need_src or need_dst or need_attn):
        return None, None, None
    fs, fd, at, out, lse, *index = ctx.saved_tensors
    idx, n_dst, fan = _block(index)
    g = grad_out.contiguous()
    H, D = fs.shape[1], fs.shape[2]
    parts = _gatv2_parts(n_dst)
    grad_src = torch.zeros_like(fs) if need_src else None
    grad_dst = torch.empty_like(fd) if need_dst else None
    partials = (torch.zeros if n_dst == 0 else torch.empty)((parts, H * D), dtype=torch.float32, device=fs.device) if need_attn else None
    _capi.check(entry(fs.device.index or 0, *idx, fs.data_ptr(), fd.data_ptr(), at.data_ptr(), out.data_ptr(), lse.data_ptr(), g.data_ptr(),
                      _ptr(grad_src), _ptr(grad_dst), _ptr(partials), parts, n_dst, *fan, H, D, ctx.slope, current_stream()))
    return grad_src, grad_dst, partials.sum(0).view_as(at) if need_attn else None


class _Gatv2Aggregate(torch.autograd.Function):
    """DGL GATv2Conv's attention step on a fixed block (coala_block_gatv2_aggregate): one kernel forward, one backward (gradients for
    feat_src, feat_dst and attn)."""

    @staticmethod
    def forward(ctx, feat_src, feat_dst, attn, nbr, negative_slope):
        return _gatv2_forward(ctx, feat_src, feat_dst, attn, _lib.coala_block_gatv2_aggregate, (nbr,), negative_slope)

    @staticmethod
    def backward(ctx, grad_out):
        return _gatv2_backward(ctx, grad_out, _lib.coala_block_gatv2_aggregate_backward) + (None,) * 2


class _Gatv2AggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_gatv2_aggregate_csr): row d's edges are indices[indptr[d]:indptr[d+1]]."""

    @staticmethod
    def forward(ctx, feat_src, feat_dst, attn, indptr, indices, negative_slope):
        return _gatv2_forward(ctx, feat_src, feat_dst, attn, _lib.coala_block_gatv2_aggregate_csr, (indptr, indices), negative_slope)

    @staticmethod
    def backward(ctx, grad_out):
        return _gatv2_backward(ctx, grad_out, _lib.coala_block_gatv2_aggregate_csr_backward) + (None,) * 3


def _rel_gat_forward(ctx, el, er, feat, rows, etype, num_rels, entry, index, negative_slope):
    """Per head and relation, a softmax of leaky_relu(el[row] + er[d, r]) over row d's entries of type r, then the weighted sum of
    feat[row] over all of them (coala_block_rel_gat_aggregate[_csr]).  rows (int32, -1: no edge) and etype (int32) are laid out like
    the block's index array, which the kernel reads only for its shape: rows stands in its place.  The log-sum-exp per (row, relation,
    head) is the state of the backward."""
    el, er, f = el.contiguous(), er.contiguous(), feat.contiguous()
    idx, n_dst, fan = _block(index)
    H, D = f.shape[1], f.shape[2]
    out = torch.empty((n_dst, H, D), dtype=torch.float32, device=f.device)
    lse = torch.empty((n_dst, num_rels, H), dtype=torch.float32, device=f.device)
    _capi.check(entry(f.device.index or 0, *idx[:-1], rows.data_ptr(), etype.data_ptr(), el.data_ptr(), er.data_ptr(), f.data_ptr(),
                      out.data_ptr(), lse.data_ptr(), n_dst, *fan, num_rels, H, D, negative_slope, current_stream()))
    ctx.save_for_backward(el, er, f, lse, rows, etype, *index)
    ctx.slope, ctx.num_rels = negative_slope, num_rels
    return out


def _rel_gat_backward(ctx, grad_out, entry):
    """-> (grad_el, grad_er, grad_feat), one launch."""
    el, er, f, lse, rows, etype, *index = ctx.saved_tensors
    idx, n_dst, fan = _block(index)
    g = grad_out.contiguous()
    grad_feat, grad_el, grad_er = torch.zeros_like(f), torch.zeros_like(el), torch.empty_like(er)
    _capi.check(entry(f.device.index or 0, *idx[:-1], rows.data_ptr(), etype.data_ptr(), el.data_ptr(), er.data_ptr(), f.data_ptr(),
                      lse.data_ptr(), g.data_ptr(), grad_feat.data_ptr(), grad_el.data_ptr(), grad_er.data_ptr(), n_dst, *fan, ctx.num_rels,
                      f.shape[1], f.shape[2], ctx.slope, current_stream()))
    return grad_el, grad_er, grad_feat


class _RelGatAggregate(torch.autograd.Function):
    """Relation-typed GAT attention on a fixed block (coala_block_rel_gat_aggregate): one kernel forward, one backward (gradients for
    el, er and feat)."""

    @staticmethod
    def forward(ctx, el, er, feat, rows, etype, num_rels, nbr, negative_slope):
        return _rel_gat_forward(ctx, el, er, feat, rows, etype, num_rels, _lib.coala_block_rel_gat_aggregate, (nbr,), negative_slope)

    @staticmethod
    def backward(ctx, grad_out):
        return _rel_gat_backward(ctx, grad_out, _lib.coala_block_rel_gat_aggregate_backward) + (None,) * 5


class _RelGatAggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_rel_gat_aggregate_csr): rows and etype have one value per entry of indices."""

    @staticmethod
    def forward(ctx, el, er, feat, rows, etype, num_rels, indptr, indices, negative_slope):
        return _rel_gat_forward(ctx, el, er, feat, rows, etype, num_rels, _lib.coala_block_rel_gat_aggregate_csr, (indptr, indices),
                                negative_slope)

    @staticmethod
    def backward(ctx, grad_out):
        return _rel_gat_backward(ctx, grad_out, _lib.coala_block_rel_gat_aggregate_csr_backward) + (None,) * 6


def _dot_gat_forward(ctx, q, k, v, rows, scale, entry, index):
    """Per head, a softmax of scale * <q[d], k[row]> over row d's entries with row >= 0, then the weighted sum of v[row]
    (coala_block_dot_gat_aggregate[_csr]); no [E, H, D] intermediate.  rows (int32, -1: no edge) is laid out like the block's index
    array, which the kernel reads only for its shape: rows stands in its place.  out and the log-sum-exp per (row, head) are the state
    of the backward, kept only when something needs a gradient."""
    qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
    idx, n_dst, fan = _block(index)
    H, D = kc.shape[1], kc.shape[2]
    out = torch.empty((n_dst, H, D), dtype=torch.float32, device=kc.device)
    lse = torch.empty((n_dst, H), dtype=torch.float32, device=kc.device)
    _capi.check(entry(kc.device.index or 0, *idx[:-1], rows.data_ptr(), qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), lse.data_ptr(),
                      n_dst, *fan, H, D, scale, current_stream()))
    if any(ctx.needs_input_grad[:3]):
        ctx.save_for_backward(qc, kc, vc, out, lse, rows, *index)
    ctx.scale = scale
    return out


def _dot_gat_backward(ctx, grad_out, entry):
    """-> (grad_q, grad_k, grad_v), one launch (coala_block_dot_gat_aggregate[_csr]_backward); a gradient nobody asked for is neither
    computed nor allocated."""
    need_q, need_k, need_v = ctx.needs_input_grad[:3]
    if not (need_q or need_k or need_v):
        return None, None, None
    q, k, v, out, lse, rows, *index = ctx.saved_tensors
    idx, n_dst, fan = _block(index)
    g = grad_out.contiguous()
    grad_q = torch.empty_like(q) if need_q else None
    grad_k = torch.zeros_like(k) if need_k else None
    grad_v = torch.zeros_like(v) if need_v else None
    _capi.check(entry(k.device.index or 0, *idx[:-1], rows.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(),
                      g.data_ptr(), _ptr(grad_q), _ptr(grad_k), _ptr(grad_v), n_dst, *fan, k.shape[1], k.shape[2], ctx.scale, current_stream()))
    return grad_q, grad_k, grad_v


class _DotGatAggregate(torch.autograd.Function):
    """Scaled dot-product attention on a fixed block (coala_block_dot_gat_aggregate): one kernel forward, one backward (gradients for q,
    k and v)."""

    @staticmethod
    def forward(ctx, q, k, v, rows, scale, nbr):
        return _dot_gat_forward(ctx, q, k, v, rows, scale, _lib.coala_block_dot_gat_aggregate, (nbr,))

    @staticmethod
    def backward(ctx, grad_out):
        return _dot_gat_backward(ctx, grad_out, _lib.coala_block_dot_gat_aggregate_backward) + (None,) * 3


class _DotGatAggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_dot_gat_aggregate_csr): rows has one value per entry of indices."""

    @staticmethod
    def forward(ctx, q, k, v, rows, scale, indptr, indices):
        return _dot_gat_forward(ctx, q, k, v, rows, scale, _lib.coala_block_dot_gat_aggregate_csr, (indptr, indices))

    @staticmethod
    def backward(ctx, grad_out):
        return _dot_gat_backward(ctx, grad_out, _lib.coala_block_dot_gat_aggregate_csr_backward) + (None,) * 4


class _PairDot(torch.autograd.Function):
    """out[p, hd] = <h[src_p, hd, :], h[dst_p, hd, :]> (coala_block_pair_dot): one kernel forward, one backward that adds both
    endpoints' gradients with float atomics into a zeroed grad_h.  h is [N, H, D] contiguous fp32, src / dst contiguous int32 [P]."""

    @staticmethod
    def forward(ctx, h, src, dst):
        P, (_, H, D) = src.numel(), h.shape
        out = torch.empty((P, H), dtype=torch.float32, device=h.device)
        _capi.check(_lib.coala_block_pair_dot(h.device.index or 0, h.data_ptr(), src.data_ptr(), dst.data_ptr(), out.data_ptr(), P, H, D,
                                              current_stream()))
        ctx.save_for_backward(h, src, dst)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        h, src, dst = ctx.saved_tensors
        g = grad_out.contiguous()
        grad_h = torch.zeros_like(h)
        _capi.check(_lib.coala_block_pair_dot_backward(h.device.index or 0, h.data_ptr(), src.data_ptr(), dst.data_ptr(), g.data_ptr(),
                                                       grad_h.data_ptr(), src.numel(), h.shape[1], h.shape[2], current_stream()))
        return grad_h, None, None


def _pair_args(h, src, dst):
    """The checks of pair_dot / pair_dot_torch."""
    if h.dim() not in (2, 3):
        raise ValueError(f"h of shape {tuple(h.shape)}: pair_dot takes [N, D] or [N, H, D]")
    for name, t in (("src", src), ("dst", dst)):
        if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError(f"{name} must be an integer tensor")
    if src.dim() != 1 or tuple(src.shape) != tuple(dst.shape):
        raise ValueError(f"src {tuple(src.shape)}, dst {tuple(dst.shape)}: one index each per pair, [P]")


def _pair_bound(h, src, dst):
    """IndexError when a pair index is >= N (one host read)."""
    if src.numel():
        top = int(torch.maximum(src.max(), dst.max()))
        if top >= h.shape[0]:
            raise IndexError(f"a pair index is {top}: h has {h.shape[0]} rows")


def pair_dot(h, src, dst, validate=True):
    """Scores of node pairs, DGL's fn.u_dot_v on a pair graph: h [N, D] -> [P], or h [N, H, D] -> [P, H], out[p] = <h[src_p], h[dst_p]>
    (per head).  src, dst: integer tensors [P].  A pair with an index < 0 scores 0 and gets no gradient; an index >= N raises IndexError
    (on the native path that check is one host read per call, which validate=False skips for a caller whose indices address h by
    construction, as an EdgeBatch's do).  Native kernels (one forward; one backward, float atomics) for fp32 h on the GPU with D >= 1
    and index tensors on the GPU; pair_dot_torch otherwise."""
    _pair_args(h, src, dst)
    native = (h.is_cuda and h.dtype == torch.float32 and src.is_cuda and dst.is_cuda and h.shape[-1] > 0 and h.numel() // max(h.shape[0], 1) < (1 << 31)
              and h.shape[0] < (1 << 31) and (h.dim() == 2 or h.shape[1] > 0))
    if not native:
        return pair_dot_torch(h, src, dst)
    if validate:
        _pair_bound(h, src, dst)
    s32, d32 = (t if t.dtype == torch.int32 else t.clamp(-1, (1 << 31) - 1).to(torch.int32) for t in (src, dst))
    h3 = h.contiguous().view(h.shape[0], 1 if h.dim() == 2 else h.shape[1], h.shape[-1])
    out = _PairDot.apply(h3, s32.contiguous(), d32.contiguous())
    return out.view(-1) if h.dim() == 2 else out


def pair_dot_torch(h, src, dst):
    """pair_dot in plain torch, any device and dtype, the same index rules: two [P, ...] gathers, a product and a sum.  The fallback of
    pair_dot, and its reference."""
    _pair_args(h, src, dst)
    s, d = src.to(device=h.device, dtype=torch.int64), dst.to(device=h.device, dtype=torch.int64)
    _pair_bound(h, s, d)
    keep = (s >= 0) & (d >= 0)
    prod = (h[s.clamp_min(0)] * h[d.clamp_min(0)]).sum(-1)
    return prod * keep.view((-1,) + (1,) * (prod.dim() - 1)).to(prod.dtype)


# ------------------------------------------------------------------------------------------------------------ skip-gram window loss
SKIPGRAM_MAX_FLOATS = 16384   # (walk_length + 1) * dim a lane group stages in LDS (coala_block_ops.hip: kSkipMaxFloats, 64 KB)
SKIPGRAM_MAX_LEN = 128


class _SkipgramLoss(torch.autograd.Function):
    """mean over the valid window pairs of pos of softplus(-<h[a], h[b]>) + the same mean of softplus(+<.,.>) over neg
    (coala_block_skipgram_loss, one launch per table that has rows).  The kernel stores one partial sum and one pair count per row;
    they are added up here in float64 and the loss is rounded to fp32 once: the same bits call after call.  The backward is one
    launch per table, one double atomic per (position, element) into ONE float64 buffer shaped like h, rounded to fp32 once.
    h [N, D] contiguous fp32; pos, neg contiguous int32 [R, L1]."""

    @staticmethod
    def forward(ctx, h, pos, neg, context):
        dev = h.device.index or 0
        total = torch.zeros((), dtype=torch.float64, device=h.device)
        saved, signs = [], []
        for rows, sign in ((pos, -1.0), (neg, 1.0)):
            R, L1 = rows.shape
            if R == 0:
                continue
            partial = torch.empty(R, dtype=torch.float32, device=h.device)
            count = torch.empty(R, dtype=torch.int32, device=h.device)
            _capi.check(_lib.coala_block_skipgram_loss(dev, h.data_ptr(), rows.data_ptr(), partial.data_ptr(), count.data_ptr(), R, L1, context,
                                                       h.shape[1], sign, current_stream()))
            n = count.sum(dtype=torch.int64).clamp_min(1)   # no valid pair: every partial is 0, and so is the mean
            total = total + partial.sum(dtype=torch.float64) / n
            saved += [rows, n]
            signs.append(sign)
        ctx.save_for_backward(h, *saved)
        ctx.args = (context, signs)
        return total.to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        h, *saved = ctx.saved_tensors
        context, signs = ctx.args
        acc = torch.zeros(h.shape, dtype=torch.float64, device=h.device)   # the kernels add in double: a node collects hundreds of terms
        for k, sign in enumerate(signs):
            rows, n = saved[2 * k], saved[2 * k + 1]
            scale = (grad_out.to(torch.float64) / n).contiguous()   # a device double: nothing waits for the host
            _capi.check(_lib.coala_block_skipgram_loss_backward(h.device.index or 0, h.data_ptr(), rows.data_ptr(), acc.data_ptr(), scale.data_ptr(),
                                                                rows.shape[0], rows.shape[1], context, h.shape[1], sign, current_stream()))
        return acc.to(torch.float32), None, None, None


def _skipgram_args(h, pos, neg, context_size):
    """The checks of skipgram_loss / skipgram_loss_torch."""
    if h.dim() != 2:
        raise ValueError(f"h of shape {tuple(h.shape)}: skipgram_loss takes [N, D]")
    for name, t in (("pos", pos), ("neg", neg)):
        if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError(f"{name} must be an integer tensor")
        if t.dim() != 2:
            raise ValueError(f"{name} of shape {tuple(t.shape)}: a walk table [R, walk_length + 1]")
        if isinstance(context_size, bool) or not isinstance(context_size, int) or not 2 <= context_size <= t.shape[1]:
            raise ValueError(f"context_size {context_size!r}: 2..{t.shape[1]}, the columns of {name}")


def _skipgram_bound(h, tables):
    """IndexError when a table entry is >= N (one host read)."""
    top = max([int(t.max()) for t in tables if t.numel()], default=-1)
    if top >= h.shape[0]:
        raise IndexError(f"a walk table entry is {top}: h has {h.shape[0]} rows")


def skipgram_loss(h, pos, neg, context_size, validate=True):
    """The skip-gram loss of walk tables, PyG's Node2Vec.loss: h fp32 [N, D]; pos, neg integer tables [R, L + 1] of rows of h, -1 = no
    node (a walk that has ended; a WalkBatch's pos and neg).  For a table, every window start a in 0 .. L + 1 - C (C = context_size) and
    every j in 1 .. C - 1 give the pair (rows[r, a], rows[r, a + j]), valid when both entries are >= 0, with the score s = <h[.], h[.]>;
        loss = mean over pos's valid pairs of softplus(-s) + mean over neg's valid pairs of softplus(s),
    a mean over no pair being 0.  softplus(-s) = -log(sigmoid(s)) stands in for PyG's -log(sigmoid(s) + 1e-15): the same value until
    sigmoid(s) nears 1e-15, where PyG's saturates at 34.5 and this one keeps growing like -s, with a gradient that does not vanish.
    Native kernels -- a walk's rows staged once in on-chip memory, every window dot formed from there; the backward adds one
    atomic per (position, element), not one per pair, into a float64 buffer
    rounded to fp32 once -- for fp32 h on the GPU with index tables on the GPU, L + 1 <= 128 and
    (L + 1) * D <= 16384; skipgram_loss_torch otherwise.  The forward value is bitwise reproducible on the native path.  An entry >= N
    raises IndexError (on the native path one host read per call, which validate=False skips for tables that address h by
    construction, as a WalkBatch's do)."""
    _skipgram_args(h, pos, neg, context_size)
    native = (h.is_cuda and h.dtype == torch.float32 and pos.is_cuda and neg.is_cuda and h.shape[1] > 0 and h.shape[0] < (1 << 31)
              and all(t.shape[1] <= SKIPGRAM_MAX_LEN and t.shape[1] * h.shape[1] <= SKIPGRAM_MAX_FLOATS for t in (pos, neg)))
    if not native:
        return skipgram_loss_torch(h, pos, neg, context_size)
    if validate:
        _skipgram_bound(h, (pos, neg))
    if pos.shape[0] == 0 and neg.shape[0] == 0:
        return h.sum() * 0.0
    p32, n32 = ((t if t.dtype == torch.int32 else t.clamp(-1, (1 << 31) - 1).to(torch.int32)).contiguous() for t in (pos, neg))
    return _SkipgramLoss.apply(h.contiguous(), p32, n32, context_size)


def _skipgram_table_torch(h, rows, context, sign):
    """One table's mean in plain torch: the window pairs as two [R, P] position lists, two gathers, a product and a sum."""
    R, L1 = rows.shape
    a = torch.arange(L1 - context + 1, device=h.device)
    j = torch.arange(1, context, device=h.device)
    first = a[:, None].expand(-1, context - 1).reshape(-1)
    second = (a[:, None] + j[None, :]).reshape(-1)
    total = h.new_zeros(())
    n = torch.zeros((), dtype=torch.int64, device=h.device)
    chunk = max(1, (1 << 24) // max(first.numel() * h.shape[1], 1))   # rows per pass: the gathers hold chunk * P * D elements
    for r0 in range(0, R, chunk):
        s, d = rows[r0: r0 + chunk][:, first], rows[r0: r0 + chunk][:, second]
        keep = (s >= 0) & (d >= 0)
        score = (h[s.clamp_min(0)] * h[d.clamp_min(0)]).sum(-1)
        # softplus(x) as -logsigmoid(-x): torch's softplus switches to the identity above 20, which is off by 2e-9 there
        total = total + (-torch.nn.functional.logsigmoid(-sign * score) * keep.to(score.dtype)).sum()
        n = n + keep.sum()
    return total / n.clamp_min(1).to(total.dtype)


def skipgram_loss_torch(h, pos, neg, context_size):
    """skipgram_loss in plain torch, any device and dtype, the same rules: built from gathers.  The fallback of skipgram_loss, and the
    building block of its float64 reference."""
    _skipgram_args(h, pos, neg, context_size)
    tables = [t.to(device=h.device, dtype=torch.int64) for t in (pos, neg)]
    _skipgram_bound(h, tables)
    return _skipgram_table_torch(h, tables[0], context_size, -1.0) + _skipgram_table_torch(h, tables[1], context_size, 1.0)
