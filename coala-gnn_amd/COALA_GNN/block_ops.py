"""Autograd wrappers of the native block ops that `Block` (sampler.py) hands to a model: mean aggregation (SAGEConv's "mean"), weighted
sum aggregation (DGL's u_mul_e_sum, the edge_weight= path of GraphConv / SAGEConv), max aggregation (DGL's fn.max: SAGEConv's "pool",
GINConv's "max"), LSTM aggregation (SAGEConv's "lstm": coala_lstm.hip, on the matrix units), the relation-typed sum (RelGraphConv's message step), GAT / GATv2 attention aggregation, scaled dot-product
attention (DotGatConv's and HGTConv's message step), temporal attention over a fused time encoding (TGATConv's message step, fixed
blocks alone), attention over edge features (TransformerConv's message step: coala_edge_attn.hip) and relation-typed GAT attention (RelGATConv's message step), on fixed blocks and on the ragged CSR blocks of full layers; and the
message-passing primitives on per-edge tensors (DGL's u_dot_v, edge_softmax, u_mul_e_sum: one Function each for both block forms).  pair_dot (DGL's u_dot_v on a pair graph: a link predictor's scores) is the one op here
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


LSTM_HIDDEN_STEP, LSTM_MAX_HIDDEN = 32, 256     # coala_lstm.hip: the native hidden sizes are the multiples of 32 up to 256


def _lstm_forward(ctx, xg, w_hh, entry, index):
    """out[d] = the last h of an LSTM run over row d's valid entries in slot order from h = c = 0, a step with source s taking
    z = xg[s] + h @ w_hh^T (coala_block_lstm_aggregate[_csr]): one kernel.  When a gradient is wanted the kernel also saves the
    activated gates [S, 4H] and c [S, H] of every slot; otherwise nothing of that size exists."""
    xg, w = xg.contiguous(), w_hh.contiguous()
    idx, n_dst, fan = _block(index)
    H, S = w.shape[1], index[-1].numel()
    out = torch.empty((n_dst, H), dtype=torch.float32, device=xg.device)
    need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
    gates = torch.empty((S, 4 * H), dtype=torch.float32, device=xg.device) if need else None
    cell = torch.empty((S, H), dtype=torch.float32, device=xg.device) if need else None
    _capi.check(entry(xg.device.index or 0, *idx, xg.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(gates), _ptr(cell), n_dst, *fan, H,
                      current_stream()))
    if need:
        ctx.save_for_backward(w, gates, cell, *index)
    ctx.xg_shape, ctx.spent = xg.shape, False
    return out


def lstm_grad_w_hh(dz, h_prev):
    """grad_w_hh [4H, H] = dz^T @ h_prev over the S slots, from the two buffers the backward kernel leaves: one batched product over at
    most 64 slices of at least 64 slots, and the sum of the slices.  One chain over all S slots measured 5 times the error of the
    step-wise fallback at S = 2240 (3.2e-06 against 6.6e-07): it rounds every step at the magnitude of the whole sum."""
    S = dz.shape[0]
    chunk = max(64, -(-S // 64))
    n = S // chunk
    if n < 2:
        return dz.t() @ h_prev
    body = torch.bmm(dz[: n * chunk].view(n, chunk, -1).transpose(1, 2), h_prev[: n * chunk].view(n, chunk, -1)).sum(0)
    return body + dz[n * chunk:].t() @ h_prev[n * chunk:] if S > n * chunk else body


def _lstm_backward(ctx, grad_out, entry):
    """One kernel walks every row in reverse: it turns the saved gates into dz in place, leaves h_prev [S, H] when grad_w_hh is wanted
    and adds dz into grad_xg with float atomics when grad_xg is wanted (coala_block_lstm_aggregate_backward[_csr]); grad_w_hh is then
    one dense batched product, lstm_grad_w_hh.  The saved gates are gone after it: a second backward through the same graph raises."""
    need_xg, need_w = ctx.needs_input_grad[:2]
    if not need_xg and not need_w:
        return None, None
    if ctx.spent:
        raise RuntimeError("lstm_aggregate: backward a second time -- the first one overwrote the saved gates (run the forward again)")
    w, gates, cell, *index = ctx.saved_tensors
    idx, n_dst, fan = _block(index)
    g = grad_out.contiguous()
    grad_xg = torch.zeros(ctx.xg_shape, dtype=torch.float32, device=g.device) if need_xg else None
    h_prev = torch.empty_like(cell) if need_w else None
    ctx.spent = True
    _capi.check(entry(g.device.index or 0, *idx, w.data_ptr(), g.data_ptr(), gates.data_ptr(), cell.data_ptr(), _ptr(h_prev), _ptr(grad_xg),
                      n_dst, *fan, w.shape[1], current_stream()))
    return grad_xg, lstm_grad_w_hh(gates, h_prev) if need_w else None


class _LSTMAggregate(torch.autograd.Function):
    """LSTM aggregation on a fixed block (coala_block_lstm_aggregate): one kernel forward, one kernel and one GEMM backward."""

    @staticmethod
    def forward(ctx, xg, w_hh, nbr):
        return _lstm_forward(ctx, xg, w_hh, _lib.coala_block_lstm_aggregate, (nbr,))

    @staticmethod
    def backward(ctx, grad_out):
        return _lstm_backward(ctx, grad_out, _lib.coala_block_lstm_aggregate_backward) + (None,)


class _LSTMAggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_lstm_aggregate_csr): row d runs over indices[indptr[d]:indptr[d+1]]."""

    @staticmethod
    def forward(ctx, xg, w_hh, indptr, indices):
        return _lstm_forward(ctx, xg, w_hh, _lib.coala_block_lstm_aggregate_csr, (indptr, indices))

    @staticmethod
    def backward(ctx, grad_out):
        return _lstm_backward(ctx, grad_out, _lib.coala_block_lstm_aggregate_backward_csr) + (None,) * 2


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


MULTI_AGGREGATORS = ("sum", "mean", "max", "min", "var", "std")   # the canonical order of the kernel's `planes` word


def multi_planes(aggregators):
    """The checked tuple of aggregator names -> the kernel's `planes` word: 4 bits per aggregator in the canonical order, holding
    its position in `aggregators` (its output plane), 15 where it is not wanted."""
    names = tuple(aggregators)
    for a in names:
        if a not in MULTI_AGGREGATORS:
            raise ValueError(f"aggregator {a!r}: multi_aggregate has {', '.join(MULTI_AGGREGATORS)}")
    if not names or len(set(names)) != len(names):
        raise ValueError(f"aggregators {names!r}: at least one name, each at most once")
    return sum((names.index(a) if a in names else 15) << (4 * k) for k, a in enumerate(MULTI_AGGREGATORS))


def _multi_forward(ctx, h_src, entry, index, planes, n_aggr, eps):
    """out[d, a, :] = the a-th wanted statistic of the rows h_src[s] over row d's valid entries (coala_block_multi_aggregate[_csr]).
    The kernel also saves the winning slots (with max or min) and the centred mean and std (with var or std) for the backward, which
    is skipped when h_src needs no gradient."""
    h = h_src.contiguous()
    idx, n_dst, fan = _block(index)
    dim = h.shape[1]
    grad = ctx.needs_input_grad[0]
    out = torch.empty((n_dst, n_aggr, dim), dtype=torch.float32, device=h.device)
    arg = torch.empty((n_dst, 2, dim), dtype=torch.int32, device=h.device) if grad and (planes >> 8 & 0xFF) != 0xFF else None
    mom = torch.empty((n_dst, 2, dim), dtype=torch.float32, device=h.device) if grad and (planes >> 16 & 0xFF) != 0xFF else None
    _capi.check(entry(h.device.index or 0, *idx, h.data_ptr(), out.data_ptr(), _ptr(arg), _ptr(mom), n_dst, *fan, dim, n_aggr, planes, eps,
                      current_stream()))
    ctx.save_for_backward(h if mom is not None else None, arg, mom, *index)
    ctx.src_shape, ctx.planes = h.shape, planes
    return out


def _multi_backward(ctx, grad_out, entry):
    """Every plane's gradient in one launch, one float atomic per (edge, element) (coala_block_multi_aggregate_backward[_csr]): not
    bitwise reproducible."""
    if not ctx.needs_input_grad[0]:
        return None
    h, arg, mom, *index = ctx.saved_tensors
    idx, n_dst, fan = _block(index)
    g = grad_out.contiguous()
    grad_src = torch.zeros(ctx.src_shape, dtype=torch.float32, device=g.device)
    _capi.check(entry(g.device.index or 0, *idx, _ptr(h), g.data_ptr(), _ptr(arg), _ptr(mom), grad_src.data_ptr(), n_dst, *fan, g.shape[2],
                      g.shape[1], ctx.planes, current_stream()))
    return grad_src


class _MultiAggregate(torch.autograd.Function):
    """Several statistics of h_src[nbr[d, j]] over the valid j at once (coala_block_multi_aggregate): one kernel forward, one backward."""

    @staticmethod
    def forward(ctx, h_src, nbr, planes, n_aggr, eps):
        return _multi_forward(ctx, h_src, _lib.coala_block_multi_aggregate, (nbr,), planes, n_aggr, eps)

    @staticmethod
    def backward(ctx, grad_out):
        return (_multi_backward(ctx, grad_out, _lib.coala_block_multi_aggregate_backward),) + (None,) * 4


class _MultiAggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_multi_aggregate_csr): row d reduces h_src[indices[indptr[d]:indptr[d+1]]]."""

    @staticmethod
    def forward(ctx, h_src, indptr, indices, planes, n_aggr, eps):
        return _multi_forward(ctx, h_src, _lib.coala_block_multi_aggregate_csr, (indptr, indices), planes, n_aggr, eps)

    @staticmethod
    def backward(ctx, grad_out):
        return (_multi_backward(ctx, grad_out, _lib.coala_block_multi_aggregate_backward_csr),) + (None,) * 5


def _edge_entry(name, index):
    """The C entry of a message-passing primitive for the block form of `index`: name, or name_csr."""
    return getattr(_lib, name if len(index) == 1 else name + "_csr")


def _edge_shape(index, heads):
    """A per-edge tensor of this block: [n_dst, fanout, H] beside nbr, [E, H] beside indices."""
    return tuple(index[-1].shape) + (heads,)


def _u_dot_v(u, v, index):
    """e[slot, h] = <u[s, h, :], v[d, h, :]>, 0 on a padding slot (coala_block_u_dot_v[_csr]); u, v contiguous fp32."""
    idx, n_dst, fan = _block(index)
    e = torch.empty(_edge_shape(index, u.shape[1]), dtype=torch.float32, device=u.device)
    _capi.check(_edge_entry("coala_block_u_dot_v", index)(u.device.index or 0, *idx, u.data_ptr(), v.data_ptr(), e.data_ptr(), n_dst, *fan,
                                                          u.shape[1], u.shape[2], current_stream()))
    return e


def _u_mul_e_sum(u, e, index):
    """out[d, h, :] = sum over row d's valid slots of e[slot, h] * u[s, h, :] (coala_block_u_mul_e_sum[_csr]); u, e contiguous fp32."""
    idx, n_dst, fan = _block(index)
    out = torch.empty((n_dst,) + tuple(u.shape[1:]), dtype=torch.float32, device=u.device)
    _capi.check(_edge_entry("coala_block_u_mul_e_sum", index)(u.device.index or 0, *idx, u.data_ptr(), e.data_ptr(), out.data_ptr(), n_dst, *fan,
                                                              u.shape[1], u.shape[2], current_stream()))
    return out


def _e_mul_v_scatter(w, x, n_src, index):
    """grad_u[s, h, :] = sum over the valid slots with source s of w[slot, h] * x[d, h, :] (coala_block_e_mul_v_scatter[_csr]): float
    atomics, not bitwise reproducible."""
    idx, n_dst, fan = _block(index)
    grad_u = torch.zeros((n_src,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    _capi.check(_edge_entry("coala_block_e_mul_v_scatter", index)(x.device.index or 0, *idx, w.data_ptr(), x.data_ptr(), grad_u.data_ptr(), n_dst,
                                                                  *fan, x.shape[1], x.shape[2], current_stream()))
    return grad_u


class _UDotV(torch.autograd.Function):
    """Block.u_dot_v on either block form, index = (nbr,) or (indptr, indices).  The primitives are each other's gradients: grad_v is
    u_mul_e_sum(u, grad_e), grad_u the reverse scatter of grad_e * v."""

    @staticmethod
    def forward(ctx, u, v, *index):
        u, v = u.contiguous(), v.contiguous()
        ctx.save_for_backward(u, v, *index)
        return _u_dot_v(u, v, index)

    @staticmethod
    def backward(ctx, grad_e):
        u, v, *index = ctx.saved_tensors
        g = grad_e.contiguous()
        grad_u = _e_mul_v_scatter(g, v, u.shape[0], index) if ctx.needs_input_grad[0] else None
        grad_v = _u_mul_e_sum(u, g, index) if ctx.needs_input_grad[1] else None
        return (grad_u, grad_v) + (None,) * len(index)


class _UMulESum(torch.autograd.Function):
    """Block.u_mul_e_sum on either block form: grad_e is u_dot_v(u, grad_out), grad_u the reverse scatter of e * grad_out."""

    @staticmethod
    def forward(ctx, u, e, *index):
        u, e = u.contiguous(), e.contiguous()
        ctx.save_for_backward(u, e, *index)
        return _u_mul_e_sum(u, e, index)

    @staticmethod
    def backward(ctx, grad_out):
        u, e, *index = ctx.saved_tensors
        g = grad_out.contiguous()
        grad_u = _e_mul_v_scatter(e, g, u.shape[0], index) if ctx.needs_input_grad[0] else None
        grad_e = _u_dot_v(u, g, index) if ctx.needs_input_grad[1] else None
        return (grad_u, grad_e) + (None,) * len(index)


def _edge_softmax(name, index, *tensors):
    """coala_block_edge_softmax[_backward][_csr] on contiguous fp32 per-edge tensors -> a new one of their shape."""
    idx, n_dst, fan = _block(index)
    out = torch.empty_like(tensors[0])
    _capi.check(_edge_entry(name, index)(out.device.index or 0, *idx, *(t.data_ptr() for t in tensors), out.data_ptr(), n_dst, *fan,
                                         out.shape[-1], current_stream()))
    return out


class _EdgeSoftmax(torch.autograd.Function):
    """Block.edge_softmax on either block form; the backward reads the saved output alone."""

    @staticmethod
    def forward(ctx, e, *index):
        a = _edge_softmax("coala_block_edge_softmax", index, e.contiguous())
        ctx.save_for_backward(a, *index)
        return a

    @staticmethod
    def backward(ctx, grad_a):
        a, *index = ctx.saved_tensors
        return (_edge_softmax("coala_block_edge_softmax_backward", index, a, grad_a.contiguous()),) + (None,) * len(index)


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


def _time_attn_parts(n_dst):
    """Rows of the grad_omega / grad_phase partials buffer, which is also the backward's grid: one block per four destination rows, 1024
    at the most (_gatv2_parts' rule)."""
    return max(1, min(-(-n_dst // 4), 1024))


class _TimeAttnAggregate(torch.autograd.Function):
    """Temporal attention on a fixed block (coala_block_time_attn_aggregate): per head, a softmax over row d's valid slots of
    scale * (<q[d], k[s]> + <qt[d], cos(omega * dt + phase)>), then out = the weighted sum of v[s] and tagg = the weighted sum of the
    time encodings; no [E, T] or [E, H, D] intermediate.  One kernel forward, one backward: gradients for q, k, v, qt, omega and phase
    (the last two as [parts, 2, T] partial sums, one row per block of the launch, summed here), none for dt; a gradient nobody asked for
    is neither computed nor allocated."""

    @staticmethod
    def forward(ctx, q, k, v, qt, omega, phase, dt, scale, nbr):
        qc, kc, vc, tc, om, ph = (t.contiguous() for t in (q, k, v, qt, omega, phase))
        n_dst, fan = nbr.shape
        H, D, T = kc.shape[1], kc.shape[2], tc.shape[2]
        out = torch.empty((n_dst, H, D), dtype=torch.float32, device=kc.device)
        tagg = torch.empty((n_dst, H, T), dtype=torch.float32, device=kc.device)
        lse = torch.empty((n_dst, H), dtype=torch.float32, device=kc.device)
        _capi.check(_lib.coala_block_time_attn_aggregate(kc.device.index or 0, nbr.data_ptr(), dt.data_ptr(), qc.data_ptr(), kc.data_ptr(),
                                                         vc.data_ptr(), tc.data_ptr(), om.data_ptr(), ph.data_ptr(), out.data_ptr(),
                                                         tagg.data_ptr(), lse.data_ptr(), n_dst, fan, H, D, T, scale, current_stream()))
        if any(ctx.needs_input_grad[:6]):
            ctx.save_for_backward(qc, kc, vc, tc, om, ph, dt, out, tagg, lse, nbr)
        ctx.scale = scale
        return out, tagg

    @staticmethod
    def backward(ctx, grad_out, grad_tagg):
        need = ctx.needs_input_grad[:6]
        if not any(need):
            return (None,) * 9
        q, k, v, qt, om, ph, dt, out, tagg, lse, nbr = ctx.saved_tensors
        n_dst, fan = nbr.shape
        H, D, T = k.shape[1], k.shape[2], qt.shape[2]
        g, gt = grad_out.contiguous(), grad_tagg.contiguous()
        grad_q = torch.empty_like(q) if need[0] else None
        grad_k = torch.zeros_like(k) if need[1] else None
        grad_v = torch.zeros_like(v) if need[2] else None
        grad_qt = torch.empty_like(qt) if need[3] else None
        parts = _time_attn_parts(n_dst)
        partials = (torch.zeros if n_dst == 0 else torch.empty)((parts, 2, T), dtype=torch.float32, device=k.device) if need[4] or need[5] else None
        _capi.check(_lib.coala_block_time_attn_aggregate_backward(
            k.device.index or 0, nbr.data_ptr(), dt.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), qt.data_ptr(), om.data_ptr(),
            ph.data_ptr(), out.data_ptr(), tagg.data_ptr(), lse.data_ptr(), g.data_ptr(), gt.data_ptr(), _ptr(grad_q), _ptr(grad_k), _ptr(grad_v),
            _ptr(grad_qt), _ptr(partials), parts, n_dst, fan, H, D, T, ctx.scale, current_stream()))
        sums = partials.sum(0) if partials is not None else None
        return (grad_q, grad_k, grad_v, grad_qt, sums[0].view_as(om) if need[4] else None, sums[1].view_as(ph) if need[5] else None, None, None,
                None)


def _edge_attn_forward(ctx, q, k, v, qe, efeat, eids, scale, entry, index):
    """Per head, a softmax over row d's edges of scale * (<q[d], k[s]> + <qe[d], x_j>), x_j = efeat[eids_j] (eids None: the slot's own
    row of efeat), then out = the weighted sum of v[s] and eagg = the weighted sum of the edge rows (coala_block_edge_attn_aggregate[_csr],
    csrc/coala_edge_attn.hip); no [E, H, D] intermediate.  eids is contiguous int32 or int64, read as it is."""
    qc, kc, vc, tc, xc = (t.contiguous() for t in (q, k, v, qe, efeat))
    idx, n_dst, fan = _block(index)
    H, D, F = kc.shape[1], kc.shape[2], tc.shape[2]
    out = torch.empty((n_dst, H, D), dtype=torch.float32, device=kc.device)
    eagg = torch.empty((n_dst, H, F), dtype=torch.float32, device=kc.device)
    lse = torch.empty((n_dst, H), dtype=torch.float32, device=kc.device)
    ctx.eid64 = int(eids is not None and eids.dtype == torch.int64)
    _capi.check(entry(kc.device.index or 0, *idx, _ptr(eids), ctx.eid64, qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), tc.data_ptr(), xc.data_ptr(),
                      out.data_ptr(), eagg.data_ptr(), lse.data_ptr(), n_dst, *fan, H, D, F, scale, current_stream()))
    if any(ctx.needs_input_grad[:5]):
        ctx.save_for_backward(qc, kc, vc, tc, xc, out, eagg, lse, *index, *(() if eids is None else (eids,)))
    ctx.scale, ctx.table = scale, eids is not None
    return out, eagg


def _edge_attn_backward(ctx, grad_out, grad_eagg, entry):
    """-> (grad_q, grad_k, grad_v, grad_qe, grad_efeat), one launch; a gradient nobody asked for is neither computed nor allocated.  The
    slot form's grad_efeat is written whole by the kernel, the table form's is zeroed here and takes float atomics."""
    need = ctx.needs_input_grad[:5]
    if not any(need):
        return (None,) * 5
    q, k, v, qe, x, out, eagg, lse, *rest = ctx.saved_tensors
    eids = rest.pop() if ctx.table else None
    idx, n_dst, fan = _block(rest)
    g, ge = grad_out.contiguous(), grad_eagg.contiguous()
    grad_q = torch.empty_like(q) if need[0] else None
    grad_k = torch.zeros_like(k) if need[1] else None
    grad_v = torch.zeros_like(v) if need[2] else None
    grad_qe = torch.empty_like(qe) if need[3] else None
    grad_x = (torch.zeros_like if ctx.table else torch.empty_like)(x) if need[4] else None
    _capi.check(entry(k.device.index or 0, *idx, _ptr(eids), ctx.eid64, q.data_ptr(), k.data_ptr(), v.data_ptr(), qe.data_ptr(), x.data_ptr(),
                      out.data_ptr(), eagg.data_ptr(), lse.data_ptr(), g.data_ptr(), ge.data_ptr(), _ptr(grad_q), _ptr(grad_k), _ptr(grad_v),
                      _ptr(grad_qe), _ptr(grad_x), n_dst, *fan, k.shape[1], k.shape[2], qe.shape[2], ctx.scale, current_stream()))
    return grad_q, grad_k, grad_v, grad_qe, grad_x


class _EdgeAttnAggregate(torch.autograd.Function):
    """Edge-feature attention on a fixed block of any fan-out (coala_block_edge_attn_aggregate): one kernel forward, one backward
    (gradients for q, k, v, qe and efeat).  efeat is 2-D: the table, or the slot form's rows viewed as [num_dst * fanout, F]."""

    @staticmethod
    def forward(ctx, q, k, v, qe, efeat, eids, scale, nbr):
        return _edge_attn_forward(ctx, q, k, v, qe, efeat, eids, scale, _lib.coala_block_edge_attn_aggregate, (nbr,))

    @staticmethod
    def backward(ctx, grad_out, grad_eagg):
        return _edge_attn_backward(ctx, grad_out, grad_eagg, _lib.coala_block_edge_attn_aggregate_backward) + (None,) * 3


class _EdgeAttnAggregateCSR(torch.autograd.Function):
    """The same on a ragged block (coala_block_edge_attn_aggregate_csr): eids and the slot form's rows have one entry per entry of indices."""

    @staticmethod
    def forward(ctx, q, k, v, qe, efeat, eids, scale, indptr, indices):
        return _edge_attn_forward(ctx, q, k, v, qe, efeat, eids, scale, _lib.coala_block_edge_attn_aggregate_csr, (indptr, indices))

    @staticmethod
    def backward(ctx, grad_out, grad_eagg):
        return _edge_attn_backward(ctx, grad_out, grad_eagg, _lib.coala_block_edge_attn_aggregate_csr_backward) + (None,) * 4


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


# ------------------------------------------------------------------------------------------------------------ typed linear
GATHER_MM_MAX_TYPES = 64      # coala_typed_mm.hip: kMaxTypes
GATHER_MM_MAX_WIDTH = 65535 * 64


class _GatherMM(torch.autograd.Function):
    """y[i] = x[rows[i]] @ op(W[types[i]]) on the fp32 matrix units (coala_block_gather_mm*): a plan (three small launches: order,
    seg) and one product kernel forward; backward, each only when needed, the same kernel on grad_y for grad_x (stored directly with
    rows None, added with float atomics into zeros otherwise) and one chunked kernel for grad_W (float atomics into zeros).  The plan
    is saved and reused.  x [N, in] and W contiguous fp32, types / rows contiguous int32 [M] (rows may be None: M == N)."""

    @staticmethod
    def forward(ctx, x, W, types, rows, transposed):
        M, T = types.numel(), W.shape[0]
        K, N = (W.shape[2], W.shape[1]) if transposed else (W.shape[1], W.shape[2])
        dev, st = x.device.index or 0, current_stream()
        i32 = dict(dtype=torch.int32, device=x.device)
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
        order, seg = torch.empty(M, **i32), torch.empty(T + 1, **i32)
        if M:
            work = torch.empty(_lib.coala_block_gather_mm_plan_work(M, T), **i32)
            _capi.check(_lib.coala_block_gather_mm_plan(dev, types.data_ptr(), _ptr(rows), M, T, order.data_ptr(), seg.data_ptr(), work.data_ptr(), st))
            _capi.check(_lib.coala_block_gather_mm(dev, x.data_ptr(), W.data_ptr(), order.data_ptr(), seg.data_ptr(), _ptr(rows), None, y.data_ptr(),
                                                   M, T, K, N, int(transposed), st))
        ctx.save_for_backward(x, W, order, seg, rows)
        ctx.transposed = transposed
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x, W, order, seg, rows = ctx.saved_tensors
        M, T, tr = order.numel(), W.shape[0], ctx.transposed
        K, N = (W.shape[2], W.shape[1]) if tr else (W.shape[1], W.shape[2])
        dev, st = x.device.index or 0, current_stream()
        g = grad_y.contiguous()
        grad_x = grad_w = None
        if ctx.needs_input_grad[0]:
            grad_x = torch.empty_like(x) if rows is None and M else torch.zeros_like(x)
            _capi.check(_lib.coala_block_gather_mm(dev, g.data_ptr(), W.data_ptr(), order.data_ptr(), seg.data_ptr(), None, _ptr(rows),
                                                   grad_x.data_ptr(), M, T, N, K, int(not tr), st))
        if ctx.needs_input_grad[1]:
            grad_w = torch.zeros_like(W)
            (p, p_rows, pk), (q, q_rows, qn) = ((g, None, N), (x, rows, K)) if tr else ((x, rows, K), (g, None, N))
            _capi.check(_lib.coala_block_gather_mm_backward_w(dev, p.data_ptr(), _ptr(p_rows), q.data_ptr(), _ptr(q_rows), order.data_ptr(),
                                                              seg.data_ptr(), grad_w.data_ptr(), M, T, pk, qn, st))
        return grad_x, grad_w, None, None, None


def _gather_mm_args(x, W, types, rows):
    """The checks of gather_mm / gather_mm_torch."""
    if x.dim() != 2 or W.dim() != 3:
        raise ValueError(f"x of shape {tuple(x.shape)}, W of shape {tuple(W.shape)}: gather_mm takes x [N, in] and W [T, ., .]")
    for name, t in (("types", types), ("rows", rows)):
        if t is None and name == "rows":
            continue
        if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError(f"{name} must be an integer tensor")
        if t.dim() != 1 or t.shape != types.shape:
            raise ValueError(f"{name} of shape {tuple(t.shape)}: one value per output row, [M]")
    if rows is None and types.shape[0] != x.shape[0]:
        raise ValueError(f"{types.shape[0]} types for the {x.shape[0]} rows of x: without rows, one type per row of x")


def _rows_bound(x, rows):
    """IndexError when a row index is >= N (one host read)."""
    if rows is not None and rows.numel():
        top = int(rows.max())
        if top >= x.shape[0]:
            raise IndexError(f"a row index is {top}: x has {x.shape[0]} rows")


def gather_mm(x, W, types, rows=None, transposed=False, validate=True):
    """The typed linear step, DGL's gather_mm / segment_mm (dgl.nn.TypedLinear's product) as one operation: -> y [M, out],
        y[i] = x[rows[i]] @ W[types[i]]       (rows=None: x[i];  transposed=True: W is [T, out, in] and W[types[i]].T is applied)
    x [N, in]; W [T, in, out]; types an integer tensor [M] in any order; rows an integer tensor [M] or None.  A row whose type lies
    outside [0, T) or whose rows[i] < 0 gives y[i] == 0 exactly and takes no gradient; rows[i] >= N raises IndexError (on the native
    path one host read per call, which validate=False skips for a caller whose rows address x by construction).  Native kernels
    (coala_typed_mm.hip: rows grouped by type on the device, one launch for all types on the fp32 matrix instructions, no sorted copy
    of x, no host read of its own) for fp32 x and W on the GPU, index tensors on the GPU, 1 <= T <= 64, in, out >= 1 and M, N < 2^31;
    gather_mm_torch otherwise.  The forward is bitwise reproducible and a row's bits do not depend on the other rows; grad_x with rows
    and grad_W are added with float atomics and are not.  grad_x and grad_W are each computed only when needed."""
    _gather_mm_args(x, W, types, rows)
    T, (d_in, d_out) = W.shape[0], ((W.shape[2], W.shape[1]) if transposed else (W.shape[1], W.shape[2]))
    native = (x.is_cuda and all(t is None or t.device == x.device for t in (W, types, rows)) and x.dtype == torch.float32
              and W.dtype == torch.float32 and 1 <= T <= GATHER_MM_MAX_TYPES and 1 <= d_in <= GATHER_MM_MAX_WIDTH
              and 1 <= d_out <= GATHER_MM_MAX_WIDTH and x.shape[1] == d_in and types.numel() < (1 << 31) and x.shape[0] < (1 << 31))
    if not native:
        return gather_mm_torch(x, W, types, rows, transposed, validate)
    if validate:
        _rows_bound(x, rows)
    t32 = types if types.dtype == torch.int32 else types.clamp(-1, T).to(torch.int32)
    r32 = rows if rows is None or rows.dtype == torch.int32 else rows.clamp(-1, (1 << 31) - 1).to(torch.int32)
    return _GatherMM.apply(x.contiguous(), W.contiguous(), t32.contiguous(), None if r32 is None else r32.contiguous(), bool(transposed))


def gather_mm_torch(x, W, types, rows=None, transposed=False, validate=True):
    """gather_mm in plain torch, any device and dtype, the same rules: a stable sort of the rows by type, one GEMM per type on its
    slice, the inverse permutation (one host read: the rows per type).  The fallback of gather_mm, and its reference."""
    _gather_mm_args(x, W, types, rows)
    T = W.shape[0]
    t = types.to(device=x.device, dtype=torch.int64)
    r = None if rows is None else rows.to(device=x.device, dtype=torch.int64)
    _rows_bound(x, r)
    Wm = W.transpose(1, 2) if transposed else W
    sends = (t >= 0) & (t < T) if r is None else (t >= 0) & (t < T) & (r >= 0)
    t = torch.where(sends, t, T)
    order = torch.argsort(t, stable=True)
    counts = torch.bincount(t, minlength=T + 1).tolist()                 # the host read
    parts, off = [], 0
    for ty, c in enumerate(counts[:T]):
        if c:
            idx = order[off:off + c]
            parts.append(x[idx if r is None else r[idx]] @ Wm[ty])
            off += c
    parts.append(x.new_zeros((counts[T], Wm.shape[2])))                  # the rows that send nothing
    back = torch.empty_like(order)
    back[order] = torch.arange(order.numel(), device=order.device)
    return torch.cat(parts)[back]
