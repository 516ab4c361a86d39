"""Autograd wrappers of the native block ops that `Block` (sampler.py) hands to a model: mean aggregation (SAGEConv's "mean"), weighted
sum aggregation (DGL's u_mul_e_sum, the edge_weight= path of GraphConv / SAGEConv), max aggregation (DGL's fn.max: SAGEConv's "pool",
GINConv's "max"), the relation-typed sum (RelGraphConv's message step) and GAT / GATv2 attention aggregation, on fixed blocks and on the ragged CSR blocks of full layers.  One kernel forward, one backward each; the
kernels are in coala-gnn_amd/csrc/coala_block_ops.hip (C ABI: coala_block_*)."""
import torch

from COALA_GNN_Pybind import _capi, current_stream

_lib = _capi.load()


class _MeanAggregate(torch.autograd.Function):
    """out[d] = mean of h_src[nbr[d, j]] over the valid j (coala_block_mean_aggregate): one kernel forward, one backward."""

    @staticmethod
    def forward(ctx, h_src, nbr):
        h = h_src.contiguous()
        n_dst, fanout = nbr.shape
        out = torch.empty((n_dst, h.shape[1]), dtype=torch.float32, device=h.device)
        _capi.check(_lib.coala_block_mean_aggregate(h.device.index or 0, nbr.data_ptr(), h.data_ptr(), out.data_ptr(), n_dst, fanout, h.shape[1],
                                                    current_stream()))
        ctx.save_for_backward(nbr)
        ctx.src_shape = h.shape
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None
        (nbr,) = ctx.saved_tensors
        g = grad_out.contiguous()
        grad_src = torch.zeros(ctx.src_shape, dtype=torch.float32, device=g.device)
        _capi.check(_lib.coala_block_mean_aggregate_backward(g.device.index or 0, nbr.data_ptr(), g.data_ptr(), grad_src.data_ptr(), nbr.shape[0],
                                                             nbr.shape[1], g.shape[1], current_stream()))
        return grad_src, None


class _MeanAggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_mean_aggregate_csr): row d averages h_src[indices[indptr[d]:indptr[d+1]]]."""

    @staticmethod
    def forward(ctx, h_src, indptr, indices):
        h = h_src.contiguous()
        n_dst = indptr.numel() - 1
        out = torch.empty((n_dst, h.shape[1]), dtype=torch.float32, device=h.device)
        _capi.check(_lib.coala_block_mean_aggregate_csr(h.device.index or 0, indptr.data_ptr(), indices.data_ptr(), h.data_ptr(), out.data_ptr(),
                                                        n_dst, h.shape[1], current_stream()))
        ctx.save_for_backward(indptr, indices)
        ctx.src_shape = h.shape
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        indptr, indices = ctx.saved_tensors
        g = grad_out.contiguous()
        grad_src = torch.zeros(ctx.src_shape, dtype=torch.float32, device=g.device)
        _capi.check(_lib.coala_block_mean_aggregate_csr_backward(g.device.index or 0, indptr.data_ptr(), indices.data_ptr(), g.data_ptr(),
                                                                 grad_src.data_ptr(), indptr.numel() - 1, g.shape[1], current_stream()))
        return grad_src, None, None


class _WeightedSum(torch.autograd.Function):
    """out[d] = sum over the valid j of w[d, j] * h_src[nbr[d, j]] (coala_block_weighted_sum): one kernel forward, one backward that
    gives grad_src and grad_w together; a gradient nobody asked for is neither computed nor allocated."""

    @staticmethod
    def forward(ctx, h_src, w, nbr):
        h, w = h_src.contiguous(), w.contiguous()
        n_dst, fanout = nbr.shape
        out = torch.empty((n_dst, h.shape[1]), dtype=torch.float32, device=h.device)
        _capi.check(_lib.coala_block_weighted_sum(h.device.index or 0, nbr.data_ptr(), w.data_ptr(), h.data_ptr(), out.data_ptr(), n_dst, fanout,
                                                  h.shape[1], current_stream()))
        ctx.save_for_backward(h, w, nbr)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        need_src, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not need_src and not need_w:
            return None, None, None
        h, w, nbr = ctx.saved_tensors
        g = grad_out.contiguous()
        grad_src = torch.zeros_like(h) if need_src else None
        grad_w = torch.empty_like(w) if need_w else None
        _capi.check(_lib.coala_block_weighted_sum_backward(g.device.index or 0, nbr.data_ptr(), w.data_ptr(), h.data_ptr(), g.data_ptr(),
                                                           grad_src.data_ptr() if need_src else None, grad_w.data_ptr() if need_w else None,
                                                           nbr.shape[0], nbr.shape[1], g.shape[1], current_stream()))
        return grad_src, grad_w, None


class _WeightedSumCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_weighted_sum_csr): row d sums w[e] * h_src[indices[e]] over e in indptr[d]:indptr[d+1]."""

    @staticmethod
    def forward(ctx, h_src, w, indptr, indices):
        h, w = h_src.contiguous(), w.contiguous()
        n_dst = indptr.numel() - 1
        out = torch.empty((n_dst, h.shape[1]), dtype=torch.float32, device=h.device)
        _capi.check(_lib.coala_block_weighted_sum_csr(h.device.index or 0, indptr.data_ptr(), indices.data_ptr(), w.data_ptr(), h.data_ptr(),
                                                      out.data_ptr(), n_dst, h.shape[1], current_stream()))
        ctx.save_for_backward(h, w, indptr, indices)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        need_src, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not need_src and not need_w:
            return None, None, None, None
        h, w, indptr, indices = ctx.saved_tensors
        g = grad_out.contiguous()
        grad_src = torch.zeros_like(h) if need_src else None
        grad_w = torch.empty_like(w) if need_w else None
        _capi.check(_lib.coala_block_weighted_sum_csr_backward(g.device.index or 0, indptr.data_ptr(), indices.data_ptr(), w.data_ptr(),
                                                               h.data_ptr(), g.data_ptr(), grad_src.data_ptr() if need_src else None,
                                                               grad_w.data_ptr() if need_w else None, indptr.numel() - 1, g.shape[1],
                                                               current_stream()))
        return grad_src, grad_w, None, None


def _rel_backward(ctx, grad_out, h, etype, w, entry, head):
    """Both gradients of the relation-typed sum in one launch (coala_block_rel_sum[_csr]_backward); `head` holds the arguments that
    describe the block.  A gradient nobody asked for is neither computed nor allocated; w None: no grad_w."""
    need_src, need_w = ctx.needs_input_grad[0], w is not None and ctx.needs_input_grad[1]
    if not need_src and not need_w:
        return None, None
    g = grad_out.contiguous()
    grad_src = torch.zeros_like(h) if need_src else None
    grad_w = torch.empty_like(w) if need_w else None
    _capi.check(entry(g.device.index or 0, *head, etype.data_ptr(), w.data_ptr() if w is not None else None, h.data_ptr(), g.data_ptr(),
                      grad_src.data_ptr() if need_src else None, grad_w.data_ptr() if need_w else None, *ctx.tail, current_stream()))
    return grad_src, grad_w


class _RelSum(torch.autograd.Function):
    """out[d, r] = sum over the valid j with etype[d, j] == r of w[d, j] * h_src[nbr[d, j]] (coala_block_rel_sum): [n_dst, R, dim], one
    kernel forward, one backward that gives grad_src and grad_w together.  w None: unit weights (a null pointer), and no grad_w."""

    @staticmethod
    def forward(ctx, h_src, w, nbr, etype, num_rels):
        h = h_src.contiguous()
        w = w.contiguous() if w is not None else None
        n_dst, fanout = nbr.shape
        out = torch.empty((n_dst, num_rels, h.shape[1]), dtype=torch.float32, device=h.device)
        _capi.check(_lib.coala_block_rel_sum(h.device.index or 0, nbr.data_ptr(), etype.data_ptr(), w.data_ptr() if w is not None else None,
                                             h.data_ptr(), out.data_ptr(), n_dst, fanout, num_rels, h.shape[1], current_stream()))
        ctx.save_for_backward(*((h, nbr, etype) + ((w,) if w is not None else ())))
        ctx.tail = (n_dst, fanout, num_rels, h.shape[1])
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, nbr, etype, *w = ctx.saved_tensors
        return _rel_backward(ctx, grad_out, h, etype, w[0] if w else None, _lib.coala_block_rel_sum_backward, (nbr.data_ptr(),)) + (None,) * 3


class _RelSumCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_rel_sum_csr): etype and w have one value per entry of indices."""

    @staticmethod
    def forward(ctx, h_src, w, indptr, indices, etype, num_rels):
        h = h_src.contiguous()
        w = w.contiguous() if w is not None else None
        n_dst = indptr.numel() - 1
        out = torch.empty((n_dst, num_rels, h.shape[1]), dtype=torch.float32, device=h.device)
        _capi.check(_lib.coala_block_rel_sum_csr(h.device.index or 0, indptr.data_ptr(), indices.data_ptr(), etype.data_ptr(),
                                                 w.data_ptr() if w is not None else None, h.data_ptr(), out.data_ptr(), n_dst, num_rels,
                                                 h.shape[1], current_stream()))
        ctx.save_for_backward(*((h, indptr, indices, etype) + ((w,) if w is not None else ())))
        ctx.tail = (n_dst, num_rels, h.shape[1])
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, indptr, indices, etype, *w = ctx.saved_tensors
        return _rel_backward(ctx, grad_out, h, etype, w[0] if w else None, _lib.coala_block_rel_sum_csr_backward,
                             (indptr.data_ptr(), indices.data_ptr())) + (None,) * 4


def _max_backward(ctx, grad_out):
    """grad_src[arg[d, c], c] += grad_out[d, c] (coala_block_max_aggregate_backward): one kernel for both block forms."""
    (arg,) = ctx.saved_tensors
    g = grad_out.contiguous()
    grad_src = torch.zeros(ctx.src_shape, dtype=torch.float32, device=g.device)
    _capi.check(_lib.coala_block_max_aggregate_backward(g.device.index or 0, arg.data_ptr(), g.data_ptr(), grad_src.data_ptr(), arg.shape[0],
                                                        arg.shape[1], current_stream()))
    return grad_src


class _MaxAggregate(torch.autograd.Function):
    """out[d, c] = max of h_src[nbr[d, j], c] over the valid j, ties to the first slot (coala_block_max_aggregate): one kernel forward,
    which also saves the winning source of every element -- skipped when h_src needs no gradient -- and one backward."""

    @staticmethod
    def forward(ctx, h_src, nbr):
        h = h_src.contiguous()
        n_dst, fanout = nbr.shape
        out = torch.empty((n_dst, h.shape[1]), dtype=torch.float32, device=h.device)
        arg = torch.empty((n_dst, h.shape[1]), dtype=torch.int32, device=h.device) if ctx.needs_input_grad[0] else None
        _capi.check(_lib.coala_block_max_aggregate(h.device.index or 0, nbr.data_ptr(), h.data_ptr(), out.data_ptr(),
                                                   arg.data_ptr() if arg is not None else None, n_dst, fanout, h.shape[1], current_stream()))
        if arg is not None:
            ctx.save_for_backward(arg)
        ctx.src_shape = h.shape
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return _max_backward(ctx, grad_out), None


class _MaxAggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_max_aggregate_csr): row d takes the maximum over h_src[indices[indptr[d]:indptr[d+1]]]."""

    @staticmethod
    def forward(ctx, h_src, indptr, indices):
        h = h_src.contiguous()
        n_dst = indptr.numel() - 1
        out = torch.empty((n_dst, h.shape[1]), dtype=torch.float32, device=h.device)
        arg = torch.empty((n_dst, h.shape[1]), dtype=torch.int32, device=h.device) if ctx.needs_input_grad[0] else None
        _capi.check(_lib.coala_block_max_aggregate_csr(h.device.index or 0, indptr.data_ptr(), indices.data_ptr(), h.data_ptr(), out.data_ptr(),
                                                       arg.data_ptr() if arg is not None else None, n_dst, h.shape[1], current_stream()))
        if arg is not None:
            ctx.save_for_backward(arg)
        ctx.src_shape = h.shape
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return _max_backward(ctx, grad_out), None, None


def _gat_contig(el, er, feat_src):
    return el.contiguous(), er.contiguous(), feat_src.contiguous()


class _GatAggregate(torch.autograd.Function):
    """DGL GATConv's attention step on a fixed block (coala_block_gat_aggregate): per head, a softmax of leaky_relu(el[s] + er[d]) over
    the valid nbr[d, j], then the weighted sum of feat_src[s].  One kernel forward, one backward (gradients for el, er and feat_src)."""

    @staticmethod
    def forward(ctx, el, er, feat_src, nbr, negative_slope):
        el, er, f = _gat_contig(el, er, feat_src)
        n_dst, fanout = nbr.shape
        H, D = f.shape[1], f.shape[2]
        out = torch.empty((n_dst, H, D), dtype=torch.float32, device=f.device)
        lse = torch.empty((n_dst, H), dtype=torch.float32, device=f.device)
        _capi.check(_lib.coala_block_gat_aggregate(f.device.index or 0, nbr.data_ptr(), el.data_ptr(), er.data_ptr(), f.data_ptr(), out.data_ptr(),
                                                   lse.data_ptr(), n_dst, fanout, H, D, negative_slope, current_stream()))
        ctx.save_for_backward(el, er, f, nbr, out, lse)
        ctx.slope = negative_slope
        return out

    @staticmethod
    def backward(ctx, grad_out):
        el, er, f, nbr, out, lse = ctx.saved_tensors
        g = grad_out.contiguous()
        grad_feat, grad_el, grad_er = torch.zeros_like(f), torch.zeros_like(el), torch.empty_like(er)
        _capi.check(_lib.coala_block_gat_aggregate_backward(f.device.index or 0, nbr.data_ptr(), el.data_ptr(), er.data_ptr(), f.data_ptr(),
                                                            out.data_ptr(), lse.data_ptr(), g.data_ptr(), grad_feat.data_ptr(), grad_el.data_ptr(),
                                                            grad_er.data_ptr(), nbr.shape[0], nbr.shape[1], f.shape[1], f.shape[2], ctx.slope,
                                                            current_stream()))
        return grad_el, grad_er, grad_feat, None, None


class _GatAggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_gat_aggregate_csr): row d's edges are indices[indptr[d]:indptr[d+1]]."""

    @staticmethod
    def forward(ctx, el, er, feat_src, indptr, indices, negative_slope):
        el, er, f = _gat_contig(el, er, feat_src)
        n_dst = indptr.numel() - 1
        H, D = f.shape[1], f.shape[2]
        out = torch.empty((n_dst, H, D), dtype=torch.float32, device=f.device)
        lse = torch.empty((n_dst, H), dtype=torch.float32, device=f.device)
        _capi.check(_lib.coala_block_gat_aggregate_csr(f.device.index or 0, indptr.data_ptr(), indices.data_ptr(), el.data_ptr(), er.data_ptr(),
                                                       f.data_ptr(), out.data_ptr(), lse.data_ptr(), n_dst, H, D, negative_slope, current_stream()))
        ctx.save_for_backward(el, er, f, indptr, indices, out, lse)
        ctx.slope = negative_slope
        return out

    @staticmethod
    def backward(ctx, grad_out):
        el, er, f, indptr, indices, out, lse = ctx.saved_tensors
        g = grad_out.contiguous()
        grad_feat, grad_el, grad_er = torch.zeros_like(f), torch.zeros_like(el), torch.empty_like(er)
        _capi.check(_lib.coala_block_gat_aggregate_csr_backward(f.device.index or 0, indptr.data_ptr(), indices.data_ptr(), el.data_ptr(),
                                                                er.data_ptr(), f.data_ptr(), out.data_ptr(), lse.data_ptr(), g.data_ptr(),
                                                                grad_feat.data_ptr(), grad_el.data_ptr(), grad_er.data_ptr(), indptr.numel() - 1,
                                                                f.shape[1], f.shape[2], ctx.slope, current_stream()))
        return grad_el, grad_er, grad_feat, None, None, None


def _gatv2_parts(n_dst):
    """Rows of the grad_attn partials buffer, which is also the backward's grid: one block per four destination rows, 1024 at the most."""
    return max(1, min(-(-n_dst // 4), 1024))


def _gatv2_forward(ctx, feat_src, feat_dst, attn, entry, index, n_dst, tail, negative_slope):
    """One launch (coala_block_gatv2_aggregate[_csr]); `index` (the block's index tensors) and `tail` describe the block.  lse is the state of
    the backward alone: it is computed, but not kept, when nothing needs a gradient."""
    fs, fd, at = feat_src.contiguous(), feat_dst.contiguous(), attn.contiguous()
    H, D = fs.shape[1], fs.shape[2]
    out = torch.empty((n_dst, H, D), dtype=torch.float32, device=fs.device)
    lse = torch.empty((n_dst, H), dtype=torch.float32, device=fs.device)
    _capi.check(entry(fs.device.index or 0, *(t.data_ptr() for t in index), fs.data_ptr(), fd.data_ptr(), at.data_ptr(), out.data_ptr(),
                      lse.data_ptr(), n_dst, *tail, H, D, negative_slope, current_stream()))
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
    n_dst, tail = out.shape[0], ((index[0].shape[1],) if len(index) == 1 else ())
    g = grad_out.contiguous()
    H, D = fs.shape[1], fs.shape[2]
    parts = _gatv2_parts(n_dst)
    grad_src = torch.zeros_like(fs) if need_src else None
    grad_dst = torch.empty_like(fd) if need_dst else None
    partials = (torch.zeros if n_dst == 0 else torch.empty)((parts, H * D), dtype=torch.float32, device=fs.device) if need_attn else None
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    _capi.check(entry(fs.device.index or 0, *(t.data_ptr() for t in index), fs.data_ptr(), fd.data_ptr(), at.data_ptr(), out.data_ptr(), lse.data_ptr(), g.data_ptr(),
                      ptr(grad_src), ptr(grad_dst), ptr(partials), parts, n_dst, *tail, H, D, ctx.slope, current_stream()))
    return grad_src, grad_dst, partials.sum(0).view_as(at) if need_attn else None


class _Gatv2Aggregate(torch.autograd.Function):
    """DGL GATv2Conv's attention step on a fixed block (coala_block_gatv2_aggregate): per head, a softmax over the valid nbr[d, j] of
    sum_c attn[h, c] leaky_relu(feat_src[s, h, c] + feat_dst[d, h, c]), then the weighted sum of feat_src[s].  One kernel forward, one
    backward (gradients for feat_src, feat_dst and attn); no [E, H, D] intermediate in either."""

    @staticmethod
    def forward(ctx, feat_src, feat_dst, attn, nbr, negative_slope):
        return _gatv2_forward(ctx, feat_src, feat_dst, attn, _lib.coala_block_gatv2_aggregate, (nbr,), nbr.shape[0], (nbr.shape[1],), negative_slope)

    @staticmethod
    def backward(ctx, grad_out):
        return _gatv2_backward(ctx, grad_out, _lib.coala_block_gatv2_aggregate_backward) + (None,) * 2


class _Gatv2AggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_gatv2_aggregate_csr): row d's edges are indices[indptr[d]:indptr[d+1]]."""

    @staticmethod
    def forward(ctx, feat_src, feat_dst, attn, indptr, indices, negative_slope):
        return _gatv2_forward(ctx, feat_src, feat_dst, attn, _lib.coala_block_gatv2_aggregate_csr, (indptr, indices), indptr.numel() - 1, (),
                              negative_slope)

    @staticmethod
    def backward(ctx, grad_out):
        return _gatv2_backward(ctx, grad_out, _lib.coala_block_gatv2_aggregate_csr_backward) + (None,) * 3
