"""PNAConv restated per edge (tests only): the message M(cat[h_src[s], h_dst[d]]) of every valid edge is materialised and each
destination's messages are reduced on their own, the way DGL and PyG state the layer; what follows the reduction (scalers, U,
batchnorm, the mixing layer, the residual) uses the layer's own modules.  Meant for a float64 copy of the layer on the CPU."""
import torch

REDUCE = {
    "sum": lambda m: m.sum(0),
    "mean": lambda m: m.mean(0),
    "max": lambda m: m.amax(0),
    "min": lambda m: m.amin(0),
    "var": lambda m: m.var(0, unbiased=False),
}


def pna_reference(layer, block, h_src, h_dst):
    rows, src = block._slots(h_src.device)
    rows, src = rows[src >= 0], src[src >= 0]
    deg = torch.bincount(rows, minlength=block.num_dst).to(h_src.dtype)
    log_d = torch.log(deg.clamp_min(1) + 1)
    scale = {"identity": torch.ones_like(log_d), "amplification": log_d / layer.delta, "attenuation": layer.delta / log_d}
    ti, outs = layer.tower_in_size, []
    for t, tower in enumerate(layer.towers):
        hs, hd = h_src[:, t * ti:(t + 1) * ti], h_dst[:, t * ti:(t + 1) * ti]
        msg = tower.M(torch.cat([hs[src], hd[rows]], 1))                                   # [E, ti]
        agg = []
        for d in range(block.num_dst):
            m = msg[rows == d]
            if len(m) == 0:
                agg.append(msg.new_zeros(len(layer.aggregators), ti))
                continue
            agg.append(torch.stack([torch.sqrt(torch.relu(REDUCE["var"](m)) + layer.eps) if a == "std" else REDUCE[a](m)
                                    for a in layer.aggregators]))
        agg = torch.stack(agg).flatten(1)                                                  # [num_dst, A * ti]
        scaled = torch.cat([agg * scale[s].unsqueeze(1) for s in layer.scalers], 1)
        outs.append(tower.dropout(tower.batchnorm(tower.U(torch.cat([hd, scaled], 1)))))
    out = layer.mixing_layer(torch.cat(outs, 1))
    return out + h_dst if layer.residual else out
