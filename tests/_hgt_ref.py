"""Naive float64 restatements of DotGatConv and HGTConv that walk the edges one by one (tests only).  Written from the formulas of the
layers' docstrings; nothing here imports COALA_GNN.nn or calls a Block method: a block is read only through its slot arrays.  HGT's
D x D relation matrices are multiplied per edge and head, as DGL's HGTConv does."""
import numpy as np


def block_edges(block):
    """-> list per destination of (local source, slot position) of every valid slot, in slot order."""
    if block.nbr is None:
        ip, idx = block.indptr.cpu().numpy(), block.indices.cpu().numpy()
        return [[(int(idx[e]), e) for e in range(ip[d], ip[d + 1]) if idx[e] >= 0] for d in range(block.num_dst)]
    nbr = block.nbr.cpu().numpy()
    f = nbr.shape[1]
    return [[(int(nbr[d, j]), d * f + j) for j in range(f) if nbr[d, j] >= 0] for d in range(block.num_dst)]


def dst_index(block):
    return np.arange(block.num_dst) if block.dst_in_src is None else block.dst_in_src.cpu().numpy().astype(np.int64)


def _softmax_sum(scores, values):
    """scores: list of floats, values: list of vectors -> sum_j softmax(scores)_j values_j"""
    m = max(scores)
    w = [np.exp(s - m) for s in scores]
    tot = sum(w)
    return sum(wi / tot * vi for wi, vi in zip(w, values))


def dotgat_layer(block, h_src, h_dst, w_src, w_dst, H, D):
    """DotGatConv: q = h_dst @ w_dst^T, k = v = h_src @ w_src^T (w: [H * D, in], a Linear's weight); -> [num_dst, H, D]"""
    k = (h_src @ w_src.T).reshape(-1, H, D)
    q = (h_dst @ w_dst.T).reshape(-1, H, D)
    out = np.zeros((block.num_dst, H, D))
    for d, edges in enumerate(block_edges(block)):
        for h in range(H):
            if edges:
                out[d, h] = _softmax_sum([float(q[d, h] @ k[s, h]) / np.sqrt(D) for s, _ in edges], [k[s, h] for s, _ in edges])
    return out


def hgt_layer(block, x_src, x_dst, nt_src, nt_dst, etype, p, H, D, per_relation_softmax=False):
    """HGTConv without LayerNorm and dropout.  p: dict of float64 arrays under the layer's parameter names; etype: flat, one value per
    slot.  per_relation_softmax: the injected fault -- normalise over a destination's edges of one relation instead of all of them."""
    R = p["rel_att"].shape[0]
    out = np.zeros((block.num_dst, H * D))
    for d, edges in enumerate(block_edges(block)):
        td = int(nt_dst[d])
        qd = (x_dst[d] @ p["q_weight"][td]).reshape(H, D)
        m = np.zeros((H, D))
        live = [(s, int(etype[pos])) for s, pos in edges if 0 <= int(etype[pos]) < R]
        for h in range(H):
            scores, msgs, rels = [], [], []
            for s, r in live:
                ts = int(nt_src[s])
                ks = (x_src[s] @ p["k_weight"][ts]).reshape(H, D)[h]
                vs = (x_src[s] @ p["v_weight"][ts]).reshape(H, D)[h]
                scores.append(float((ks @ p["rel_att"][r, h]) @ qd[h]) * p["rel_pri"][r, h] / np.sqrt(D))
                msgs.append(vs @ p["rel_msg"][r, h])
                rels.append(r)
            if not live:
                continue
            if per_relation_softmax:
                for r in set(rels):
                    sel = [i for i, rr in enumerate(rels) if rr == r]
                    m[h] += _softmax_sum([scores[i] for i in sel], [msgs[i] for i in sel])
            else:
                m[h] = _softmax_sum(scores, msgs)
        y = m.reshape(H * D) @ p["a_weight"][td]
        alpha = 1.0 / (1.0 + np.exp(-p["skip"][td]))
        res = x_dst[d] if "residual_w" not in p else x_dst[d] @ p["residual_w"]
        out[d] = y * alpha + res * (1 - alpha)
    return out


def layer_norm(x, weight, bias, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * weight + bias
