"""float64 / float32 reference of harness.HGT and harness.DotGAT on sampled blocks, written in GLOBAL node ids and CSC edge positions
only (tests only).  The blocks are decoded once by tests/_global_ref.decode into triples (dst_gid, src_gid, eid); everything after that
works on [N, d] arrays indexed by global node id and on the triples: node types are ntype[gid], edge types are etype[eid].  Nothing
here imports COALA_GNN.nn or calls a Block method.  HGT's D x D relation matrices are applied per edge, as the layer's formula states it.

run(...) evaluates a model through torch autograd on the CPU in float64 or in float32 (every array cast down: the rounding scale of the
GPU tolerance) -> {name: float64 array} with 'logits', 'grad_X' and every parameter's gradient under its name in the model.
fault='per_relation' normalises HGT's softmax per (destination, relation) instead of over all of a destination's in-edges."""
import numpy as np
import torch


def _softmax_agg(score, msg, key, n_keys, dst, N):
    """score [E, H], msg [E, H, D]: softmax of score over the edges of one key, then the sum of a * msg per destination -> [N, H, D]"""
    H = score.shape[1]
    m = torch.full((n_keys, H), float("-inf"), dtype=score.dtype).scatter_reduce(0, key.unsqueeze(1).expand(-1, H), score.detach(), "amax")
    p = torch.exp(score - m[key])
    l = torch.zeros((n_keys, H), dtype=score.dtype).index_add(0, key, p)
    a = p / l[key]
    return torch.zeros((N,) + tuple(msg.shape[1:]), dtype=msg.dtype).index_add(0, dst, a.unsqueeze(-1) * msg)


def _typed(h, W, nt):
    """h[n] @ W[nt[n]] for every node n"""
    return torch.bmm(h.unsqueeze(1), W[nt]).squeeze(1)


def _hgt(P, layers, h, nt, etype, H, use_norm, fault):
    N = h.shape[0]
    n_layers = len(layers)
    for i, lay in enumerate(layers):
        p = {k.split(".", 2)[2]: v for k, v in P.items() if k.startswith(f"layers.{i}.")}
        D = p["rel_att"].shape[-1]
        R = p["rel_att"].shape[0]
        tri = torch.from_numpy(lay.tri)
        d, s, r = tri[:, 0], tri[:, 1], etype[tri[:, 2]]
        live = (r >= 0) & (r < R)
        d, s, r = d[live], s[live], r[live]
        K = _typed(h, p["k_weight"], nt).view(N, H, D)
        V = _typed(h, p["v_weight"], nt).view(N, H, D)
        Q = _typed(h, p["q_weight"], nt).view(N, H, D)
        ke = torch.einsum("ehd,ehdf->ehf", K[s], p["rel_att"][r])
        score = (ke * Q[d]).sum(-1) * p["rel_pri"][r] / float(D) ** 0.5
        msg = torch.einsum("ehd,ehdf->ehf", V[s], p["rel_msg"][r])
        if fault == "per_relation":
            agg = _softmax_agg(score, msg, d * R + r, N * R, d, N)
        else:
            agg = _softmax_agg(score, msg, d, N, d, N)
        y = _typed(agg.reshape(N, H * D), p["a_weight"], nt)
        alpha = torch.sigmoid(p["skip"][nt]).unsqueeze(-1)
        res = h @ p["residual_w"] if "residual_w" in p else h
        h = y * alpha + res * (1 - alpha)
        if use_norm:
            h = torch.nn.functional.layer_norm(h, (H * D,), p["norm.weight"], p["norm.bias"])
    assert i + 1 == n_layers
    return h @ P["linear.weight"].t() + P["linear.bias"]


def _dotgat(P, layers, h, H):
    N = h.shape[0]
    for i, lay in enumerate(layers):
        W = P[f"layers.{i}.fc.weight"]
        D = W.shape[0] // H
        k = (h @ W.t()).view(N, H, D)
        tri = torch.from_numpy(lay.tri)
        d, s = tri[:, 0], tri[:, 1]
        score = (k[d] * k[s]).sum(-1) / float(D) ** 0.5
        h = _softmax_agg(score, k[s], d, N, d, N)
        if i + 1 < len(layers):
            h = h.flatten(1)
    return h.mean(1).log_softmax(dim=-1)


def run(kind, params, layers, X, Cmat, seeds, dtype, heads, ntype=None, etype=None, use_norm=True, fault=None):
    """kind: 'hgt' or 'dotgat'; params: {name: array} as the model names them; layers: decoded blocks in model order."""
    P = {k: torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(True) for k, v in params.items()}
    x = torch.tensor(np.asarray(X), dtype=dtype).requires_grad_(True)
    if kind == "hgt":
        full = _hgt(P, layers, x, torch.from_numpy(np.asarray(ntype, dtype=np.int64)), torch.from_numpy(np.asarray(etype, dtype=np.int64)),
                    heads, use_norm, fault)
    else:
        full = _dotgat(P, layers, x, heads)
    logits = full[torch.from_numpy(np.asarray(seeds, dtype=np.int64))]
    (logits * torch.tensor(np.asarray(Cmat), dtype=dtype)).sum().backward()
    out = {"logits": logits, "grad_X": x.grad}
    for k, v in P.items():
        out[k] = v.grad if v.grad is not None else torch.zeros_like(v)
    return {k: v.detach().double().numpy() for k, v in out.items()}


def compare(got, ref64, ref32, factor, tag, log=print, factors=None):
    """The rule of tests/test_models_global_gpu.py: per array E32 = max |ref32 - ref64|; |got - ref64| <= max(factor * E32, 8 * 2^-24 *
    max |ref64|).  Prints error / E32 per array; -> the largest ratio.  factors: {array name: its own factor}."""
    worst, failed = 0.0, []
    for name, want in ref64.items():
        e32 = float(np.abs(ref32[name] - want).max())
        err = float(np.abs(got[name] - want).max())
        f = (factors or {}).get(name, factor)
        tol = max(f * e32, 8 * 2.0 ** -24 * float(np.abs(want).max()))
        ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio if err > 8 * 2.0 ** -24 * float(np.abs(want).max()) else 0.0)
        log(f"{tag} {name}: error {err:.3e} E32 {e32:.3e} error / E32 {ratio:.2f} bound {tol:.3e}")
        assert got[name].shape == want.shape, f"{tag} {name}: shape {got[name].shape}, the reference has {want.shape}"
        if not err <= tol:
            failed.append(f"{tag} {name}: error {err:.3e} above {tol:.3e} (E32 {e32:.3e})")
    assert not failed, "; ".join(failed)
    return worst
