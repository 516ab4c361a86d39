"""The models of tests/test_hgt_model_gpu.py and of its CPU proof (tests only): harness.HGT, 2 layers, T = 3 node types, R = 4 edge types
(the graph of tests/_model_cases.py carries types 0..2: relation 3 has no edge), LayerNorm on, dropout 0; and harness.DotGAT, 2 layers.
The node type of node v is (v * 7 + v // 5) % 3, a table over the graph's global ids."""
import numpy as np
import torch

import _model_cases as MC

T, R, HEADS, HID = 3, 4, 2, 12


def ntype():
    v = np.arange(MC.N)
    return ((v * 7 + v // 5) % T).astype(np.int64)


def make_model(kind, seed=0):
    from COALA_GNN.harness import HGT, DotGAT
    torch.manual_seed(100 + seed)
    if kind == "hgt":
        m = HGT(MC.IN, HID, MC.NCLS, 2, HEADS, T, R, dropout=0.0, use_norm=True)
        with torch.no_grad():                     # away from their constant initial values, so that their gradients are tested in the open
            for layer in m.layers:
                layer.rel_pri.uniform_(0.5, 1.5)
                layer.skip.uniform_(-1.0, 1.0)
                layer.norm.weight.uniform_(0.5, 1.5)
                layer.norm.bias.uniform_(-0.5, 0.5)
        return m
    return DotGAT(MC.IN, HID // HEADS, MC.NCLS, 2, HEADS)


def run(model, blocks, X, Cmat):
    """_model_cases.run_model with HGT's node-type table -> {name: float64 array}"""
    input_nodes = blocks[0].src_nodes
    feat = X[input_nodes.to(X.device)].clone().requires_grad_(True)
    if hasattr(model, "num_rels"):
        logits = model(blocks, feat, ntype=torch.from_numpy(ntype()).to(X.device))
    else:
        logits = model(blocks, feat)
    return MC.finish(model, logits, feat, input_nodes, X.shape, Cmat)
