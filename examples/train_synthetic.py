#!/usr/bin/env python3
"""Minimal training script on the MI355X path, shaped like the reference's examples/sbatch_ssd_gnn_train.py:50-195 (same
objects, same loop, same printed lines), without DGL / mpi4py: on seeded synthetic data (no datasets on the box), or -- with
--path -- on a dataset directory in the reference's on-disk layout (--data IGB --dataset_size medium | --data OGB; :202-213, :273-285).

  python examples/train_synthetic.py --nodes 200000 --dim 128 --epochs 2
  python examples/train_synthetic.py --model_type gat --num_heads 4 --fan_out 5,5 --eval_fan_out=-1,-1
  python examples/train_synthetic.py --model_type gatv2 --num_heads 4 --share_weights
  python examples/train_synthetic.py --model_type gcn --edge_weights random --use_edge_weight
  python examples/train_synthetic.py --sampler labor --fan_out 10,10
  python examples/train_synthetic.py --sage_aggregator pool
  python examples/train_synthetic.py --model_type gin --gin_aggregator max
  python examples/train_synthetic.py --model_type rgcn --num_rels 4 --rgcn_regularizer basis --num_bases 2
  python examples/train_synthetic.py --model_type rgcn --num_rels 4 --sampler rel --rel_fan_out "10,3,0,-1;5,5,5,5"
  python examples/train_synthetic.py --model_type rgat --num_rels 4 --num_heads 4 --sampler rel --rel_fan_out "10,3,0,-1;5,5,5,5"
  python examples/train_synthetic.py --model_type rsage --num_rels 4
  python examples/train_synthetic.py --model_type hgt --num_heads 4 --num_rels 4 --num_ntypes 3
  python examples/train_synthetic.py --sampler pinsage --model_type pinsage --num_traversals 2 --termination_prob 0.5 --num_random_walks 10
  python examples/train_synthetic.py --task link --num_negs 5 --exclude reverse_id
  python examples/train_synthetic.py --sampler temporal --temporal_strategy last --time_decay 0.001
  python examples/train_synthetic.py --task link --sampler temporal --num_negs 5
  python examples/train_synthetic.py --node_embedding --emb_dim 64 --model_type rgcn --num_rels 4
  python examples/train_synthetic.py --node_embedding --emb_optimizer sgd --emb_lr 0.1 --task link
  python examples/train_synthetic.py --task node2vec --walk_length 20 --context_size 10 --walks_per_node 10 --p 0.5 --q 2 --num_negs 1 \
      --emb_dim 128 --emb_optimizer adam --emb_lr 0.01 --batch_size 128
  python examples/train_synthetic.py --path /data/IGB/ --data IGB --dataset_size medium --cache_size 4096
  python -m torch.distributed.run --nproc-per-node 8 examples/train_synthetic.py --cache_backend nccl ...

The caller of the hot path is out of scope of the port; this file only shows that the loop runs unchanged on the API mirror."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "coala-gnn_amd"))

import torch  # noqa: E402

from COALA_GNN import COALA_GNN_DataLoader, MPI_Comm_Manager, Node2Vec, Node_Distributor, NodeEmbedding, RowWiseAdagrad, SparseAdagrad, SparseAdam, SparseSGD, SSD_INFO  # noqa: E402
from COALA_GNN.color_info_gen import color_graph, save_color_files  # noqa: E402
from COALA_GNN.harness import GAT, GCN, GIN, HGT, RGAT, RGCN, RSAGE, SAGE, GATv2, LinkPredictor, PinSAGE, SageMean, link_loss  # noqa: E402
from COALA_GNN.sampler import (EdgePredictionSampler, LaborSampler, NeighborSampler, RandomWalkNeighborSampler, RelNeighborSampler,  # noqa: E402
                               TemporalEdgePredictionSampler, TemporalNeighborSampler, UniformNegativeSampler, reverse_edge_ids,
                               sort_csc_by_etype)
from COALA_GNN.synthetic import alloc_pinned_table, community_csc, edge_times, edge_types_by_source, powerlaw_csc, symmetrize_csc  # noqa: E402

T_MAX = 1 << 20    # --sampler temporal: synthetic edge timestamps lie in [0, T_MAX)
DECAY = "decay"    # --time_decay: the edata key the gcn / sage layers read their edge weights from


def add_time_decay(blocks, lam):
    """--time_decay LAMBDA: block.edata['decay'] = exp(-LAMBDA * dt) for every sampled edge (dt: the row's query time minus the edge's
    timestamp, made by TemporalNeighborSampler; padding slots are not read), the weights of the layers' edge_weight= path."""
    if lam is not None:
        for b in blocks:
            b.edata[DECAY] = torch.exp(-lam * b.edata["dt"].to(torch.float32))
    return blocks


def make_embedding(args, loader):
    """--node_embedding: the loader's table is the embedding table (random rows instead of features), its fetch is the lookup
    (NodeEmbedding.from_manager + attach), and a sparse optimizer writes the rows a step used back through the cache, beside the dense one.
    -> (embedding, sparse optimizer), or (None, None)."""
    if not args.node_embedding:
        return None, None
    emb = NodeEmbedding.from_manager(loader.COALA_GNN_Manager)
    if args.emb_optimizer == "adam":
        return emb, SparseAdam([emb], lr=args.emb_lr, betas=tuple(args.emb_betas), step=args.emb_step)
    cls = {"adagrad": SparseAdagrad, "rowwise_adagrad": RowWiseAdagrad, "sgd": SparseSGD}[args.emb_optimizer]
    return emb, cls([emb], lr=args.emb_lr)


def sparse_optimizer(args, emb):
    """--emb_optimizer over one NodeEmbedding."""
    if args.emb_optimizer == "adam":
        return SparseAdam([emb], lr=args.emb_lr, betas=tuple(args.emb_betas), step=args.emb_step)
    return {"adagrad": SparseAdagrad, "rowwise_adagrad": RowWiseAdagrad, "sgd": SparseSGD}[args.emb_optimizer]([emb], lr=args.emb_lr)


def train_node2vec(args):
    """--task node2vec: shallow embeddings of a graph without features, as PyG's Node2Vec example -- biased walks from every node,
    skip-gram windows with --num_negs negative rows per walk, a sparse optimizer over the embedding table.  The graph is
    symmetrize_csc(community_csc(..)): planted communities of 2,048 nodes, rows sorted by source id as the walks need at q != 1.  After
    every epoch: the mean loss, and how much closer (cosine) a node's embedding is to a node of its own community than to a random one."""
    device = f"cuda:{torch.cuda.current_device()}"
    indptr, indices = symmetrize_csc(*community_csc(args.nodes, 10.0, seed=0, device=device))
    torch.manual_seed(max(args.seed, 0))
    model = Node2Vec((indptr, indices), args.emb_dim or args.dim, args.walk_length, args.context_size, walks_per_node=args.walks_per_node, p=args.p,
                     q=args.q, num_negative_samples=args.num_negs, cache_mb=args.cache_size, device=device, seed=max(args.seed, 0))
    opt = sparse_optimizer(args, model.embedding)
    probe = torch.randperm(args.nodes, generator=torch.Generator().manual_seed(1))[:4096].to(device)
    for epoch in range(args.epochs):
        t0, total, steps = time.time(), 0.0, 0
        for batch in model.loader(args.batch_size):
            loss = model.loss(batch)
            loss.backward()
            opt.step()   # (clears the embedding's trace)
            total += float(loss.detach())
            steps += 1
        z = torch.nn.functional.normalize(model(probe), dim=1)
        same = (probe // 2048 * 2048 + (probe + 1) % 2048).clamp_max(args.nodes - 1)      # the next node of the same community
        other = probe[torch.randperm(probe.numel(), device=device)]
        gap = float(((z * torch.nn.functional.normalize(model(same), dim=1)).sum(1) - (z * torch.nn.functional.normalize(model(other), dim=1)).sum(1)).mean())
        print(f"Epoch {epoch:05d} | Loss {total / max(steps, 1):.4f} | Steps {steps} | cos(same community) - cos(random) {gap:+.4f} | "
              f"Time {time.time() - t0:.2f}s")
    model.close()


def train_link(args, comm, device, indptr, indices, feat, files, fan_out):
    """--task link: GraphSAGE (or GAT) link prediction as in DGL's example -- minibatches of seed edges, --num_negs uniform negative pairs
    per edge, the seed edges (and with --exclude reverse_id their reverses) taken out of the blocks, dot-product scores, BCE loss."""
    rev = None
    if args.exclude == "reverse_id":   # the reverse map needs a symmetric simple graph
        indptr, indices = symmetrize_csc(indptr, indices)
        rev = reverse_edge_ids(indptr, indices)
    edata = {}
    if args.sampler == "temporal":   # every seed edge is queried at its own timestamp: strict times keep it, and all later edges, out
        edata = {"ts": edge_times(indptr, seed=1, t_max=T_MAX)}
        sampler = TemporalEdgePredictionSampler(TemporalNeighborSampler(fan_out, strategy=args.temporal_strategy),
                                                negative_sampler=UniformNegativeSampler(args.num_negs))
    else:
        cls = LaborSampler if args.sampler == "labor" else NeighborSampler
        sampler = EdgePredictionSampler(cls(fan_out), exclude=None if args.exclude == "none" else args.exclude, reverse_eids=rev,
                                        negative_sampler=UniformNegativeSampler(args.num_negs))
    g = sampler.make_graph(indptr, indices, edata=edata)
    n_train = int(0.6 * indices.numel()) if args.num_train_edges is None else min(args.num_train_edges, indices.numel())
    train_eids = torch.randperm(indices.numel(), generator=torch.Generator().manual_seed(0))[:n_train]
    nd = Node_Distributor(comm, train_eids, args.batch_size, *files, parsing_method="baseline")   # the items are edge ids: no colour routing
    loader = COALA_GNN_DataLoader(SSD_INFO(1, args.dim * 4, 1024, 0), nd, g, sampler, args.batch_size, args.dim, sampler.fanouts,
                                  args.cache_size, device, refresh_counter=args.refresh_counter, cache_backend=args.cache_backend,
                                  sim_buf=feat, shuffle=False, num_rows=args.nodes, prefetch=args.prefetch)
    if args.seed >= 0:
        torch.manual_seed(args.seed)
    if args.model_type == "gat":
        encoder = GAT(args.dim, args.hidden_channels, args.hidden_channels, len(fan_out), args.num_heads)
    else:
        encoder = SAGE(args.dim, args.hidden_channels, args.hidden_channels, len(fan_out), args.sage_aggregator,
                       edge_weight=None if args.time_decay is None else DECAY)
    model = LinkPredictor(encoder).to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=args.learning_rate)
    emb, emb_optimizer = make_embedding(args, loader)
    count = 0
    model.train()
    for epoch in range(args.epochs):
        print(f"Epoch: {epoch}")
        epoch_start = time.time()
        for step, (input_nodes, batch, blocks, fetch_feature) in enumerate(loader):
            if step % 100 == 0:
                print(f"Rank: {comm.local_rank} step: {step}")
            count += 1
            if emb is not None:
                fetch_feature = emb.attach(input_nodes, fetch_feature)
            pos_score, neg_score = model(add_time_decay(blocks, args.time_decay), fetch_feature, batch)
            loss = link_loss(pos_score, neg_score)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            if emb is not None:
                emb_optimizer.step()   # (clears the embedding's trace)
            if count == 1:
                first_loss = loss.item()
        torch.cuda.synchronize()
        print(f"Epoch Time: {time.time() - epoch_start}")
        print(f"Total number of iterations: {count}")
        loader.print_stats()
    print(f"first loss {first_loss:.4f}")
    print(f"final loss {loss.item():.4f}")
    comm.global_comm.Barrier()
    del loader
    comm.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--fan_out", type=str, default="5,5")
    ap.add_argument("--eval_fan_out", type=str, default=None,
                    help="fan-outs of the evaluation loader (default: --fan_out); -1 takes every in-edge, e.g. -1,-1 for full neighbourhoods")
    ap.add_argument("--sampler", type=str, default="neighbor", choices=["neighbor", "labor", "rel", "pinsage", "temporal"],
                    help="labor: layer-neighbour sampling (LaborSampler) -- the same expected fan-out per node, fewer input nodes to fetch; "
                         "rel: a fan-out per edge type (RelNeighborSampler, --rel_fan_out; needs --model_type rgcn, rgat, rsage or hgt); "
                         "pinsage: the --fan_out most visited nodes of short random walks, with their visit counts as edge weights "
                         "(RandomWalkNeighborSampler; --num_traversals, --termination_prob, --num_random_walks); "
                         "temporal: synthetic edge timestamps and a query time per seed node, a row samples only among its edges older than "
                         "its query time (TemporalNeighborSampler; --temporal_strategy, --time_decay)")
    ap.add_argument("--temporal_strategy", type=str, default="uniform", choices=["uniform", "last"],
                    help="with --sampler temporal: draw the fan-out uniformly among the eligible edges, or take the most recent ones")
    ap.add_argument("--time_decay", type=float, default=None,
                    help="with --sampler temporal: LAMBDA; the gcn / sage layers weigh every message by exp(-LAMBDA * dt), dt = the row's query "
                         "time minus the edge's timestamp (block.edata['dt']), through their edge_weight= path")
    ap.add_argument("--num_traversals", type=int, default=2, help="with --sampler pinsage: hops per walk (1..16)")
    ap.add_argument("--termination_prob", type=float, default=0.5, help="with --sampler pinsage: a hop after the first ends the walk with this probability")
    ap.add_argument("--num_random_walks", type=int, default=10, help="with --sampler pinsage: walks per node (1..64)")
    ap.add_argument("--rel_fan_out", type=str, default=None,
                    help="with --sampler rel, in place of --fan_out: layers separated by ';', the --num_rels relations of a layer by ',' "
                         "(-1: every in-edge of the type, 0: none); a single number per layer applies to every relation, "
                         "e.g. \"10,3,0,-1;5,5,5,5\" or \"5;5\"")
    ap.add_argument("--layer_dependency", action="store_true", help="with --sampler labor: the same random numbers in every layer")
    ap.add_argument("--edge_weights", type=str, default="none", choices=["none", "random"],
                    help="random: seeded edge weights in (0, 1] with ~10%% zeros, sampled in proportion by the training sampler (DGL's "
                         "prob=); evaluation stays uniform")
    ap.add_argument("--use_edge_weight", action="store_true",
                    help="with --edge_weights random: the blocks carry their edge ids (NeighborSampler(edge_ids=True)) and the gcn / sage "
                         "layers multiply every message by its edge's weight, block.edata['w'] (DGL's edge_weight=); gat and gin ignore it")
    ap.add_argument("--walk_length", type=int, default=20, help="with --task node2vec: hops per walk (1..127; a walk holds walk_length + 1 nodes)")
    ap.add_argument("--context_size", type=int, default=10, help="with --task node2vec: nodes per skip-gram window (2..walk_length + 1)")
    ap.add_argument("--walks_per_node", type=int, default=10, help="with --task node2vec: walks per start node (1..64)")
    ap.add_argument("--p", type=float, default=1.0, help="with --task node2vec: the return parameter")
    ap.add_argument("--q", type=float, default=1.0, help="with --task node2vec: the in-out parameter (p = q = 1 is DeepWalk)")
    ap.add_argument("--task", type=str, default="node", choices=["node", "link", "node2vec"],
                    help="link: link prediction on the synthetic graph (EdgePredictionSampler over --sampler neighbor | labor, --model_type sage "
                         "| gat as the encoder, dot-product scores, BCE loss); the training items are edge ids")
    ap.add_argument("--num_negs", type=int, default=5, help="with --task link: uniform negative pairs per seed edge (0..64)")
    ap.add_argument("--num_train_edges", type=int, default=None, help="with --task link: training edges per epoch (default: 60 %% of the edges)")
    ap.add_argument("--exclude", type=str, default="self", choices=["none", "self", "reverse_id"],
                    help="with --task link: take the seed edges out of the sampled blocks (self), and their reverses too (reverse_id: the "
                         "synthetic graph is symmetrised first)")
    ap.add_argument("--node_embedding", action="store_true",
                    help="featureless nodes: the input row of every node is a learned embedding (NodeEmbedding over the loader's table and "
                         "cache, randomly initialised) updated by a sparse optimizer that touches only the minibatch's rows; synthetic graph, "
                         "--cache_backend isolated, one GPU, --prefetch 0")
    ap.add_argument("--emb_dim", type=int, default=None, help="with --node_embedding: floats per embedding row (default: --dim)")
    ap.add_argument("--emb_optimizer", type=str, default="adagrad", choices=["adagrad", "adam", "rowwise_adagrad", "sgd"],
                    help="with --node_embedding: SparseAdagrad, SparseAdam, RowWiseAdagrad (one float of state per row) or SparseSGD")
    ap.add_argument("--emb_betas", type=float, nargs=2, default=[0.9, 0.999], help="with --emb_optimizer adam: beta1 beta2")
    ap.add_argument("--emb_step", type=str, default="row", choices=["row", "global"],
                    help="with --emb_optimizer adam: bias corrections from each row's own update count (DGL) or from the optimizer's step count (torch)")
    ap.add_argument("--emb_lr", type=float, default=0.05, help="with --node_embedding: learning rate of the sparse optimizer")
    ap.add_argument("--batch_size", type=int, default=1024)
    ap.add_argument("--hidden_channels", type=int, default=128)
    ap.add_argument("--num_classes", type=int, default=19)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--cache_size", type=int, default=64, help="MB")
    ap.add_argument("--cache_backend", type=str, default="isolated", choices=["isolated", "nccl", "nvshmem"])
    ap.add_argument("--distribution", type=str, default="node_color", choices=["node_color", "baseline"])
    ap.add_argument("--refresh_counter", type=int, default=10)
    ap.add_argument("--prefetch", type=int, default=0)
    ap.add_argument("--learning_rate", type=float, default=0.01)
    ap.add_argument("--path", type=str, default=None, help="dataset root in the reference's layout (default: synthetic data)")
    ap.add_argument("--data", type=str, default="IGB", choices=["IGB", "OGB", "flat"])
    ap.add_argument("--dataset_size", type=str, default="experimental")
    # accepted so that the reference's command lines (examples/4GB_script.sh, Cache_compare_script.sh, Distribution_compare_script.sh) run as they are
    ap.add_argument("--num_layers", type=int, default=None, help="must equal the number of fan-outs when given")
    ap.add_argument("--feat_cpu", action="store_true", help="features in pinned host memory: always the case here (the NVMe tier is out of scope)")
    ap.add_argument("--model_type", type=str, default="sage", choices=["gat", "gatv2", "sage", "gcn", "gin", "rgcn", "rgat", "rsage", "hgt", "pinsage"],
                    help="sage: GraphSAGE (--sage_aggregator); gat: GAT with --num_heads heads (native attention aggregation); gatv2: the same model on GATv2Conv layers (--share_weights); gcn: GraphConv, "
                         "norm='both'; gin: GINConv layers (--gin_aggregator), an MLP in each; rgcn: RelGraphConv layers, one weight matrix per edge "
                         "type (--num_rels synthetic types, the source node's id modulo --num_rels; native relation-typed sum); rgat: RelGATConv layers, "
                         "a GATConv of --num_heads heads per edge type, summed (native relation-typed attention); rsage: RelSAGEConv layers, a SAGEConv "
                         "'gcn' per edge type, summed; pinsage: WeightedSAGEConv layers on the visit counts of --sampler pinsage")
    ap.add_argument("--sage_aggregator", type=str, default="mean", choices=["mean", "gcn", "pool"],
                    help="aggregator of --model_type sage; pool: the maximum of relu(fc_pool(h)) over the neighbours (native max aggregation)")
    ap.add_argument("--gin_aggregator", type=str, default="sum", choices=["sum", "max", "mean"], help="aggregator of --model_type gin")
    ap.add_argument("--seed", type=int, default=0,
                    help="seed of torch's generators, set before the model is built: its initial weights (and dropout masks) are the same "
                         "from run to run, as the synthetic data and the samplers' draws already are; negative: not seeded")
    ap.add_argument("--num_heads", type=int, default=4, help="attention heads of --model_type gat, gatv2 and rgat")
    ap.add_argument("--share_weights", action="store_true",
                    help="--model_type gatv2: one projection for the source and the destination rows of every layer (GATv2Conv's share_weights)")
    ap.add_argument("--num_rels", type=int, default=4, help="edge types of --model_type rgcn, rgat, rsage and hgt (1..64)")
    ap.add_argument("--num_ntypes", type=int, default=3,
                    help="node types of --model_type hgt (the Heterogeneous Graph Transformer on the native scaled dot-product attention): "
                         "synthetic, a node's id modulo --num_ntypes")
    ap.add_argument("--rgcn_regularizer", type=str, default="none", choices=["none", "basis"], help="weight regularizer of --model_type rgcn")
    ap.add_argument("--num_bases", type=int, default=None, help="bases of --rgcn_regularizer basis (default: --num_rels)")
    args = ap.parse_args()
    if args.num_layers is not None and args.num_layers != len(args.fan_out.split(",")) and args.num_layers != 2:
        ap.error("--num_layers does not match --fan_out")   # (the reference's own scripts pass --num_layers 2 with a 3-entry fan-out: tolerated)

    if args.node_embedding:
        if args.path or args.cache_backend != "isolated" or args.prefetch or int(os.environ.get("WORLD_SIZE", 1)) != 1:
            ap.error("--node_embedding runs on the synthetic graph with --cache_backend isolated, one GPU and --prefetch 0")
        if args.emb_dim is not None:
            args.dim = args.emb_dim
    local_rank = int(os.environ.get("LOCAL_RANK", os.environ.get("SLURM_LOCALID", 0)))
    node_rank = int(os.environ.get("SLURM_NODEID", 0))
    torch.cuda.set_device(local_rank)
    if args.task == "node2vec":   # no features, no GNN, no loader: walks, an embedding table and a sparse optimizer
        if args.path or args.node_embedding or int(os.environ.get("WORLD_SIZE", 1)) != 1 or not 0 <= args.num_negs <= 16:
            ap.error("--task node2vec runs on the synthetic graph on one GPU, with --num_negs 0..16 and without --node_embedding (it owns its table)")
        return train_node2vec(args)
    comm = MPI_Comm_Manager(node_rank)                                  # sbatch_ssd_gnn_train.py:262
    device = "cuda:" + str(comm.local_rank)
    comm.initialize_nested_process_group(args.cache_backend)            # :267
    rel_fan_out = None
    if args.sampler == "rel":
        if args.model_type not in ("rgcn", "rgat", "rsage", "hgt") or not args.rel_fan_out or args.edge_weights != "none" or args.layer_dependency:
            ap.error("--sampler rel needs --model_type rgcn, rgat, rsage or hgt and --rel_fan_out, and takes neither --edge_weights nor "
                     "--layer_dependency")
        rel_fan_out = [[int(f) for f in layer.split(",")] for layer in args.rel_fan_out.split(";")]
        rel_fan_out = [layer[0] if len(layer) == 1 else layer for layer in rel_fan_out]
        # what the loader sizes its fetch buffers from: the per-layer totals (RelNeighborSampler.fanouts), -1 for a layer with a -1
        args.fan_out = ",".join(str(f) for f in RelNeighborSampler(rel_fan_out, args.num_rels).fanouts)
    elif args.rel_fan_out:
        ap.error("--rel_fan_out needs --sampler rel")
    fan_out = [int(f) for f in args.fan_out.split(",")]
    eval_fan_out = fan_out if args.eval_fan_out is None else [int(f) for f in args.eval_fan_out.split(",")]
    if len(eval_fan_out) != len(fan_out):
        ap.error("--eval_fan_out needs as many layers as --fan_out")
    if args.model_type in ("rgat", "hgt") and (args.num_heads < 1 or args.hidden_channels % args.num_heads):
        ap.error(f"--model_type {args.model_type} needs --hidden_channels to be a multiple of --num_heads")
    if args.model_type == "hgt" and args.num_ntypes < 1:
        ap.error("--num_ntypes must be at least 1")
    if (args.model_type == "pinsage") != (args.sampler == "pinsage"):
        ap.error("--model_type pinsage and --sampler pinsage go together: the model reads the visit counts the sampler puts on its blocks")
    if args.sampler == "temporal" and (args.edge_weights != "none" or args.layer_dependency or eval_fan_out != fan_out or args.path
                                       or any(f < 1 for f in fan_out)):
        ap.error("--sampler temporal runs on the synthetic graph with fan-outs of 1..32 and takes neither --edge_weights, --layer_dependency "
                 "nor --eval_fan_out")
    if args.time_decay is not None and (args.sampler != "temporal" or args.model_type not in ("sage", "gcn")):
        ap.error("--time_decay needs --sampler temporal and --model_type sage or gcn")
    if args.sampler == "pinsage" and (args.edge_weights != "none" or args.layer_dependency or eval_fan_out != fan_out):
        ap.error("--sampler pinsage takes neither --edge_weights, --layer_dependency nor --eval_fan_out")

    dataset = None
    if args.path:   # IGBDatast_Shared_CSC_UVA / OGBDataset_Shared_UVA (:273-285): CSC in HBM, features in shared pinned host memory
        from COALA_GNN.datasets import SharedCSCDataset
        dataset = SharedCSCDataset(args.path, comm, device, num_classes=args.num_classes, layout=args.data, dataset_size=args.dataset_size)
        g0 = dataset[0]
        indptr, indices, labels, feat = g0.indptr, g0.indices, g0.ndata["labels"], dataset.feat_data
        args.nodes, args.dim = dataset.num_nodes, dataset.dim
        train_ids = torch.nonzero(g0.ndata["train_mask"], as_tuple=True)[0].clone()                          # :62
        test_ids = torch.nonzero(g0.ndata["test_mask"], as_tuple=True)[0].clone()                            # :63
        meta = {"IGB": os.path.join(args.path, args.dataset_size), "OGB": args.path, "flat": args.path}[args.data]   # :55-61
    else:           # synthetic stand-in
        indptr, indices = powerlaw_csc(args.nodes, 10.0, seed=0, device=device)
        labels = (torch.arange(args.nodes, device=device) * 7) % args.num_classes
        feat = alloc_pinned_table(args.nodes, args.dim, seed=0, device=comm.local_rank)
        if args.node_embedding:   # no input features: the table holds the embedding rows, randomly initialised
            feat.cpu_tensor.uniform_(-1.0, 1.0, generator=torch.Generator().manual_seed(max(args.seed, 0)))
        train_ids = torch.arange(int(0.6 * args.nodes))
        test_ids = torch.arange(int(0.8 * args.nodes), args.nodes)
        meta = None
    n_train = len(train_ids)
    if meta is not None and all(os.path.exists(os.path.join(meta, f)) for f in ("color.npy", "topk.npy", "score.npy")):
        tmp = meta  # the colouring tool's output next to the dataset, where the reference looks for it
    else:
        tmp = tempfile.mkdtemp(prefix="coala_color_")
        if comm.global_rank == 0:                                       # examples/color_info_gen/generate_color_data.py
            color, tk, sc, n_col, _ = color_graph(indptr.cpu().numpy(), indices.cpu().numpy(), train_ids.numpy())
            save_color_files(tmp, color, tk, sc)
            print(f"num_colors: {n_col}")
        comm.global_comm.Barrier()
        if comm.global_size > 1:
            tmp = comm.global_comm.allgather(tmp)[0]
    files = [os.path.join(tmp, f) for f in ("color.npy", "topk.npy", "score.npy")]

    if args.task == "link":
        if args.path or args.sampler not in ("neighbor", "labor", "temporal") or args.model_type not in ("sage", "gat") or args.edge_weights != "none":
            ap.error("--task link runs on the synthetic graph with --sampler neighbor | labor | temporal and --model_type sage | gat, without "
                     "--edge_weights")
        if args.sampler == "temporal" and args.exclude == "reverse_id":
            ap.error("--sampler temporal needs no exclusion pass (strict times leave the seed edges out): drop --exclude reverse_id")
        return train_link(args, comm, device, indptr, indices, feat, files, fan_out)
    train_nid = train_ids[torch.randperm(n_train, generator=torch.Generator().manual_seed(0))]               # :62-65
    nd = Node_Distributor(comm, train_nid, args.batch_size, *files, parsing_method=args.distribution)      # :68
    edata, prob = {}, None
    if args.edge_weights == "random":   # in CSC order, aligned with `indices`
        gw = torch.Generator(device=indices.device).manual_seed(1)
        w = 1.0 - torch.rand(indices.numel(), generator=gw, device=indices.device)
        w[torch.rand(indices.numel(), generator=gw, device=indices.device) < 0.1] = 0.0
        edata, prob = {"w": w}, "w"
    if args.use_edge_weight and prob is None:
        ap.error("--use_edge_weight needs --edge_weights random")
    ew = "w" if args.use_edge_weight and args.model_type not in ("gat", "gatv2", "gin", "rgcn", "rgat", "rsage", "hgt") else None
    ndata = {"labels": labels}
    if args.sampler == "temporal":   # a timestamp per edge (sorted inside every row) and a query time per node, which the sampler reads as seed_time
        edata = dict(edata, ts=edge_times(indptr, seed=1, t_max=T_MAX))
        ndata["t"] = T_MAX // 4 + (torch.arange(args.nodes, device=device) * 7919) % (3 * T_MAX // 4)
        if args.time_decay is not None:
            ew = DECAY
    typed = args.model_type in ("rgcn", "rgat", "rsage", "hgt")   # the models on typed edges
    if typed:   # the edge types of a homogenised heterograph, in CSC order; the blocks find theirs through their edge ids
        if not 1 <= args.num_rels <= 64:
            ap.error("--num_rels must be 1..64")
        edata = dict(edata, etype=edge_types_by_source(indices, args.num_rels))
        if rel_fan_out is not None:   # RelNeighborSampler wants every node's in-edges sorted by type (no other edata to carry along here)
            indices, edata["etype"], _ = sort_csc_by_etype(indptr, indices, edata["etype"])
    edge_ids = ew is not None or typed
    if args.sampler == "labor":
        if prob is not None:
            ap.error("--sampler labor does not sample by edge weight (--edge_weights)")
        sampler = LaborSampler(fan_out, layer_dependency=args.layer_dependency, edge_ids=edge_ids)
    elif rel_fan_out is not None:
        sampler = RelNeighborSampler(rel_fan_out, args.num_rels)
    elif args.sampler == "pinsage":
        sampler = RandomWalkNeighborSampler(fan_out, args.num_traversals, args.termination_prob, args.num_random_walks)
    elif args.sampler == "temporal":
        sampler = TemporalNeighborSampler(fan_out, strategy=args.temporal_strategy, seed_time="t", edge_ids=edge_ids or ew is not None)
    else:
        if args.layer_dependency:
            ap.error("--layer_dependency needs --sampler labor")
        sampler = NeighborSampler(fan_out, prob=prob, edge_ids=edge_ids)                            # :70-72
    g = sampler.make_graph(indptr, indices, ndata=ndata, edata=edata)
    train_loader = COALA_GNN_DataLoader(SSD_INFO(1, args.dim * 4, 1024, 0), nd, g, sampler, args.batch_size, args.dim, fan_out,
                                        args.cache_size, device, refresh_counter=args.refresh_counter,
                                        cache_backend=args.cache_backend, sim_buf=feat, shuffle=False, num_rows=args.nodes,
                                        prefetch=args.prefetch)                                             # :82-95
    if args.seed >= 0:
        torch.manual_seed(args.seed)
    if args.model_type == "gat":                                                                            # :220-231
        model = GAT(args.dim, args.hidden_channels, args.num_classes, len(fan_out), args.num_heads).to(device)
    elif args.model_type == "gatv2":
        model = GATv2(args.dim, args.hidden_channels, args.num_classes, len(fan_out), args.num_heads, args.share_weights).to(device)
    elif args.model_type == "gcn":
        model = GCN(args.dim, args.hidden_channels, args.num_classes, len(fan_out), edge_weight=ew).to(device)
    elif args.model_type == "gin":
        model = GIN(args.dim, args.hidden_channels, args.num_classes, len(fan_out), args.gin_aggregator).to(device)
    elif args.model_type == "rgat":
        model = RGAT(args.dim, args.hidden_channels, args.num_classes, len(fan_out), args.num_rels, args.num_heads).to(device)
    elif args.model_type == "hgt":
        ntype = torch.arange(args.nodes, device=device) % args.num_ntypes                                   # the graph's node-type table
        model = HGT(args.dim, args.hidden_channels, args.num_classes, len(fan_out), args.num_heads, args.num_ntypes, args.num_rels,
                    ntype=ntype).to(device)
    elif args.model_type == "rsage":
        model = RSAGE(args.dim, args.hidden_channels, args.num_classes, len(fan_out), args.num_rels).to(device)
    elif args.model_type == "pinsage":
        model = PinSAGE(args.dim, args.hidden_channels, args.num_classes, len(fan_out)).to(device)
    elif args.model_type == "rgcn":
        model = RGCN(args.dim, args.hidden_channels, args.num_classes, len(fan_out), args.num_rels,
                     None if args.rgcn_regularizer == "none" else args.rgcn_regularizer, args.num_bases).to(device)
    elif ew is not None or args.sage_aggregator != "mean":
        model = SAGE(args.dim, args.hidden_channels, args.num_classes, len(fan_out), args.sage_aggregator, edge_weight=ew).to(device)
    else:
        model = SageMean(args.dim, args.hidden_channels, args.num_classes, len(fan_out)).to(device)
    if comm.global_size > 1:
        model = torch.nn.parallel.DistributedDataParallel(model, device_ids=[comm.local_rank])             # :112
    loss_fcn = torch.nn.CrossEntropyLoss().to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=args.learning_rate)
    emb, emb_optimizer = make_embedding(args, train_loader)

    count = num_sampled_nodes = 0
    model.train()
    for epoch in range(args.epochs):                                                                        # :126-151
        print(f"Epoch: {epoch}")
        epoch_start = time.time()
        for step, (input_nodes, seeds, blocks, fetch_feature) in enumerate(train_loader):
            num_sampled_nodes += len(input_nodes)
            if step % 100 == 0:
                print(f"Rank: {comm.local_rank} step: {step}")
            count += 1
            batch_labels = blocks[-1].dstdata["labels"]
            blocks = add_time_decay([block.int().to(device) for block in blocks], args.time_decay)
            batch_labels = batch_labels.view(-1).to(device)
            if emb is not None:
                fetch_feature = emb.attach(input_nodes, fetch_feature)
            batch_pred = model(blocks, fetch_feature)
            loss = loss_fcn(batch_pred, batch_labels)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            if emb is not None:
                emb_optimizer.step()   # (clears the embedding's trace)
            if count == 1:
                first_loss = loss.item()
        torch.cuda.synchronize()
        print(f"Epoch Time: {time.time() - epoch_start}")
        print(f"Total number of iterations: {count}")
        print(f"Number of sampled nodes : {num_sampled_nodes}")
        train_loader.print_stats()
    print(f"first loss {first_loss:.4f}")
    print(f"final loss {loss.item():.4f}")
    comm.global_comm.Barrier()
    del train_loader

    # evaluation over the test nodes through a second loader, as the reference does (:156-195)
    test_nd = Node_Distributor(comm, test_ids, args.batch_size, *files, parsing_method=args.distribution)
    eval_sampler = sampler if eval_fan_out == fan_out and prob is None else NeighborSampler(eval_fan_out, edge_ids=edge_ids)
    test_loader = COALA_GNN_DataLoader(SSD_INFO(1, args.dim * 4, 1024, 0), test_nd, g, eval_sampler, args.batch_size, args.dim, eval_fan_out,
                                       args.cache_size, device, refresh_counter=args.refresh_counter,
                                       cache_backend=args.cache_backend, sim_buf=feat, shuffle=False, num_rows=args.nodes)
    model.eval()
    correct = total = 0
    with torch.no_grad():
        for step, (input_nodes, seeds, blocks, fetch_feature) in enumerate(test_loader):
            if step % 100 == 0:
                print("Eval step: ", step)
            blocks = add_time_decay([block.to(device) for block in blocks], args.time_decay)
            batch_labels = blocks[-1].dstdata["labels"].view(-1)
            pred = model(blocks, fetch_feature).argmax(1)
            correct += int((pred == batch_labels).sum())
            total += batch_labels.numel()
    print("Test Acc {:.2f}%".format(100.0 * correct / max(total, 1)))
    comm.global_comm.Barrier()
    del test_loader
    if dataset is not None:
        dataset.close()
    comm.destroy_process_group()


if __name__ == "__main__":
    main()
