"""node2vec / DeepWalk: shallow node embeddings trained on biased random walks with the skip-gram loss.

Node2Vec stands where PyG's torch_geometric.nn.Node2Vec and DGL's DeepWalk stand (Grover & Leskovec, "node2vec: Scalable Feature
Learning for Networks", KDD 2016; p = q = 1 is DeepWalk, Perozzi et al., KDD 2014).  The pieces are the project's own: the walks and
the batch are sampler.walk_batch (one native call: second-order walks, negatives, one list of distinct nodes), the rows are a
NodeEmbedding behind the feature cache, the loss is block_ops.skipgram_loss (the windows of a walk scored from on-chip memory), and
the update is a sparse optimizer over that embedding -- PyG trains its Node2Vec with SparseAdam.

Written from the papers and the public behaviour of PyG's class, not copied from it.  Differences that matter to a user:
  * walk_length counts HOPS: a walk holds walk_length + 1 nodes (PyG subtracts one from its argument and counts nodes);
  * the loss uses softplus where PyG adds 1e-15 inside the logarithm (block_ops.skipgram_loss);
  * the walks follow in-edges, as every sampler here: on a symmetric graph that is the usual walk;
  * one GPU, walks of at most 127 hops, no metapaths, no edge weights."""
import torch

from . import block_ops
from .embedding import NodeEmbedding
from .sampler import MAX_WALK_LENGTH, MAX_WALK_NEGATIVES, _as_graph, node2vec_thresholds, walk_batch

__all__ = ["Node2Vec"]


class Node2Vec(object):
    """Node2Vec(g, embedding_dim, walk_length, context_size, walks_per_node=1, p=1.0, q=1.0, num_negative_samples=1, cache_mb=64,
             device='cuda', seed=0, backend='native' | 'torch')

    g: a CSCGraph (or an (indptr, indices) pair of device tensors); with q != 1 its rows must be sorted by source id
    (sampler.sort_csc_by_src; synthetic.symmetrize_csc produces that order).  The model owns self.embedding, a NodeEmbedding of
    [num_nodes, embedding_dim] with the given backend: hand it to SparseAdam / RowWiseAdagrad / ....

        model = Node2Vec(g, 128, walk_length=20, context_size=10, walks_per_node=10)
        opt = SparseAdam(model.embedding, lr=0.01)
        for batch in model.loader(batch_size=128):
            loss = model.loss(batch); loss.backward(); opt.step()
        z = model()                      # every row, untracked

    The walks of a batch are a function of (seed, the batch's number in the epoch order, start node, walk): with the same seed, two
    runs see the same batches."""

    def __init__(self, g, embedding_dim, walk_length, context_size, walks_per_node=1, p=1.0, q=1.0, num_negative_samples=1, cache_mb=64,
                 device="cuda", seed=0, backend="native"):
        for name, x, lo, hi in (("embedding_dim", embedding_dim, 1, 1 << 20), ("walk_length", walk_length, 1, MAX_WALK_LENGTH),
                                ("walks_per_node", walks_per_node, 1, 64), ("num_negative_samples", num_negative_samples, 0, MAX_WALK_NEGATIVES)):
            if isinstance(x, bool) or not isinstance(x, int) or not lo <= x <= hi:
                raise ValueError(f"{name} {x!r}: {lo}..{hi}")
        if isinstance(context_size, bool) or not isinstance(context_size, int) or not 2 <= context_size <= walk_length + 1:
            raise ValueError(f"context_size {context_size!r}: 2..walk_length + 1 = {walk_length + 1} (a walk holds walk_length + 1 nodes)")
        node2vec_thresholds(p, q)
        self.graph = _as_graph(g)
        self.embedding_dim, self.walk_length, self.context_size = embedding_dim, walk_length, context_size
        self.walks_per_node, self.p, self.q, self.num_negative_samples = walks_per_node, float(p), float(q), num_negative_samples
        self.seed = int(seed)
        self.step = 0   # batches drawn so far: the `step` of the next batch's walks
        self.embedding = NodeEmbedding(self.graph.num_nodes, embedding_dim, cache_mb=cache_mb, device=device, backend=backend)

    def sample(self, nodes, step=None):
        """The WalkBatch of the start nodes `nodes`; step: the batch's number (default: the model's counter, which then advances)."""
        if step is None:
            step, self.step = self.step, self.step + 1
        return walk_batch(self.graph, nodes, self.p, self.q, self.walk_length, self.walks_per_node, self.num_negative_samples, seed=self.seed,
                          step=step)

    def loader(self, batch_size, shuffle=True):
        """One epoch: a generator of WalkBatch objects over all nodes, batch_size start nodes each, in an order shuffled by (seed, the
        step counter at the epoch's start) -- reproducible."""
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError(f"batch_size {batch_size!r}: a positive integer")
        N = self.graph.num_nodes
        if shuffle:
            gen = torch.Generator().manual_seed((self.seed * 1000003 + self.step) & ((1 << 63) - 1))
            order = torch.randperm(N, generator=gen)
        else:
            order = torch.arange(N)
        order = order.to(self.graph.device)
        for b0 in range(0, N, batch_size):
            yield self.sample(order[b0: b0 + batch_size])

    def loss(self, batch):
        """emb(batch.input_nodes) -- a tracked lookup: the sparse optimizer's step() finds the gradient -- then skipgram_loss."""
        h = self.embedding(batch.input_nodes)
        dev = h.device
        return block_ops.skipgram_loss(h, batch.pos.to(dev), batch.neg.to(dev), self.context_size, validate=False)

    def forward(self, ids=None):
        """Rows of the embedding, untracked: of `ids`, or of every node."""
        if ids is None:
            ids = torch.arange(self.graph.num_nodes, device=self.embedding.device)
        return self.embedding.read(ids)

    __call__ = forward

    def close(self):
        self.embedding.close()
