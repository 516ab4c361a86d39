"""Float64 per-edge restatement of temporal attention (tests only): the reference of Block.time_attn_aggregate and of TGATConv.

Nothing is factorised: every neighbour slot of a fixed block gets its own key and value -- the source's row gathered per edge, Phi(dt)
= cos(omega * dt + phase) concatenated to it, the whole W_k / W_v applied -- then a masked softmax over the row's slots and the sum.
The op takes k, v and qt already projected, so op_ref forms each slot's score and value from those, the value's time part left as tagg.
Torch float64 on the CPU, autograd for the gradients."""
import numpy as np
import torch


def block_rows(rng, n_dst, fan, n_src):
    """nbr int32 [n_dst, fan] of random sources; with n_dst >= 3 (fan >= 3): -1 inside rows 0 and 2, row 1 all -1, a source twice in row 2."""
    nbr = rng.integers(0, n_src, size=(n_dst, fan)).astype(np.int32)
    if n_dst >= 3:
        nbr[1] = -1
        nbr[0, fan // 2] = nbr[2, fan // 2] = -1
        nbr[2, fan - 1] = nbr[2, 0]
    return nbr


def _softmax_rows(e, valid):
    """Softmax over dim 1 of e [n_dst, fan, H] among the valid slots; a row without one gets zeros."""
    e = e.masked_fill(~valid[:, :, None], float("-inf"))
    m = e.amax(1, keepdim=True)
    p = torch.exp(e - torch.where(torch.isfinite(m), m, torch.zeros_like(m))) * valid[:, :, None]
    l = p.sum(1, keepdim=True)
    return p / torch.where(l > 0, l, torch.ones_like(l))


def op_ref(nbr, q, k, v, qt, dt, omega, phase, scale=None):
    """-> (out [n_dst, H, D], tagg [n_dst, H, T]) from float64 tensors, slot by slot."""
    valid = nbr >= 0
    src = nbr.clamp_min(0).long()
    phi = torch.cos(dt.to(q.dtype)[:, :, None] * omega + phase)                        # [n_dst, fan, T]
    scale = q.shape[2] ** -0.5 if scale is None else scale
    e = scale * (torch.einsum("nhd,nfhd->nfh", q, k[src]) + torch.einsum("nht,nft->nfh", qt, phi))
    a = _softmax_rows(e, valid)
    return torch.einsum("nfh,nfhd->nhd", a, v[src]), torch.einsum("nfh,nft->nht", a, phi)


def layer_ref(conv, nbr, h_src, h_dst, dt):
    """TGATConv.forward per edge, with conv's own (float64) parameters: keys and values are w_k / w_v applied to [h_src[s_j] || Phi(dt_j)]."""
    H, D = conv._num_heads, conv._head_feats
    enc = conv.time_encoder
    valid = nbr >= 0
    x = torch.cat([h_src[nbr.clamp_min(0).long()], enc(dt.to(h_src.dtype) * conv.time_scale)], dim=-1)      # [n_dst, fan, F + T]
    q = (torch.cat([h_dst, enc(torch.zeros(h_dst.shape[0], dtype=h_src.dtype))], dim=-1) @ conv.w_q.t()).view(-1, H, D)
    k = (x @ conv.w_k.t()).view(*nbr.shape, H, D)
    v = (x @ conv.w_v.t()).view(*nbr.shape, H, D)
    a = _softmax_rows(torch.einsum("nhd,nfhd->nfh", q, k) * D ** -0.5, valid)
    attn = torch.einsum("nfh,nfhd->nhd", a, v).flatten(1)
    return conv.fc2(torch.relu(conv.fc1(torch.cat([attn, h_dst], dim=1))))
