"""Native neighbour sampler for the COALA_GNN_DataLoader: `NeighborSampler(fanouts).sample(graph, seeds)`.

Stands where the reference passes dgl.dataloading.MultiLayerNeighborSampler (examples/sbatch_ssd_gnn_train.py:70-72; used
at COALA-GNN-Setup/COALA_GNN/COALA_GNN_DataLoader.py:162).  DGL is not installed on the MI355X image; any object with the
same .sample(graph, seeds) -> (input_nodes, output_nodes, blocks) still works with the loader.  The kernels are in
coala-gnn_amd/csrc/coala_sampler.hip (C ABI: coala_sampler_*).  The CSC arrays live in HBM (the reference keeps them in
shared pinned host memory and samples over PCIe: examples/ssd_gnn_dataloader.py:496-523)."""
import ctypes as C

import torch

from COALA_GNN_Pybind import _capi, current_stream

from .block_ops import (_DotGatAggregate, _DotGatAggregateCSR, _GatAggregate, _GatAggregateCSR, _Gatv2Aggregate, _Gatv2AggregateCSR, _MaxAggregate, _MaxAggregateCSR, _MeanAggregate,
                        _MeanAggregateCSR, _RelGatAggregate, _RelGatAggregateCSR, _RelSum, _RelSumCSR, _WeightedSum, _WeightedSumCSR)

__all__ = ["NeighborSampler", "LaborSampler", "RelNeighborSampler", "RandomWalkNeighborSampler", "random_walk", "sort_csc_by_etype",
           "check_etype_sorted", "CSCGraph", "Block", "ITEM_LIMIT", "EID", "EdgePredictionSampler", "as_edge_prediction_sampler",
           "UniformNegativeSampler", "EdgeBatch", "edge_batch", "edge_batch_wait", "reverse_edge_ids", "MAX_NEGATIVES",
           "TemporalNeighborSampler", "TemporalEdgePredictionSampler", "sort_csc_by_time", "check_time_sorted", "pair_code_bits",
           "node2vec_random_walk", "node2vec_thresholds", "sort_csc_by_src", "check_src_sorted", "WalkBatch", "walk_batch", "walk_batch_begin",
           "walk_batch_end", "MAX_WALK_LENGTH", "MAX_WALK_NEGATIVES"]

_lib = _capi.load()

EID = "_ID"   # DGL's dgl.EID: block.edata[EID] is the position of every sampled edge in the graph's CSC `indices` array
ITEM_LIMIT = 8192 * 1024   # items (destination nodes + neighbour slots) one layer may hold (coala_sampler.hip: kMaxTiles * kTile)


def _is_int_tensor(t):
    return isinstance(t, torch.Tensor) and not (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool)


def _as_graph(g):
    return CSCGraph(*g) if isinstance(g, tuple) else g


def _u64(x):
    """A seed or a step as the uint64 the C entries take: any Python integer, modulo 2^64."""
    return int(x) & ((1 << 64) - 1)


def _sort_csc_by_key(indptr, indices, key, what):
    """sort_csc_by_etype / sort_csc_by_time: a stable sort of every row's in-edges by an integer key, `what` its name in the messages."""
    if key.dim() != 1 or key.numel() != indices.numel():
        raise ValueError(f"edge {what} must have shape ({indices.numel()},) in CSC order, got {tuple(key.shape)}")
    if not _is_int_tensor(key):
        raise ValueError(f"edge {what} must be an integer tensor")
    deg = indptr[1:] - indptr[:-1]
    rows = torch.repeat_interleave(torch.arange(deg.numel(), device=indptr.device), deg, output_size=indices.numel())
    by_key = torch.sort(key.to(indptr.device), stable=True).indices
    perm = by_key[torch.sort(rows[by_key], stable=True).indices]
    return indices[perm], key[perm], perm


def _check_sorted_in_rows(indptr, key, name, what, int_note, sort_call, num_rels=None):
    """check_etype_sorted / check_time_sorted: an integer tensor of num_edges values (in [0, num_rels) when given), non-decreasing inside
    every row of the CSC.  `what`, `int_note` and `sort_call` are the caller's words in the messages."""
    E = int(indptr[-1].item()) if indptr.numel() else 0
    if not _is_int_tensor(key):
        raise ValueError(f"edata[{name!r}]: edge {what} must be an integer tensor{int_note}")
    if key.dim() != 1 or key.numel() != E:
        raise ValueError(f"edata[{name!r}]: edge {what} must have shape ({E},) in CSC order, got {tuple(key.shape)}")
    if E == 0:
        return
    t = key.to(indptr.device)
    if num_rels is not None and bool(((t < 0) | (t >= num_rels)).any()):
        raise ValueError(f"edata[{name!r}]: edge {what} must lie in [0, {num_rels}) (num_rels={num_rels})")
    drop = t[1:] < t[:-1]                                  # drop[p - 1]: the key falls from position p - 1 to p
    starts = indptr[1:-1]
    starts = starts[(starts > 0) & (starts < E)]           # ... which it may where a row starts
    drop[starts - 1] = False
    if bool(drop.any()):
        raise ValueError(f"edata[{name!r}]: edge {what} must be non-decreasing inside every row of the CSC; sort the graph with "
                         f"COALA_GNN.sampler.{sort_call}")


def sort_csc_by_etype(indptr, indices, etype):
    """Sort the in-edges of every node by edge type, DGL's dgl.sort_csc_by_tag: -> (indices_sorted, etype_sorted, perm).  Stable by
    (row, type): edges of one type keep their CSC order.  perm (int64 [E]) maps new positions to old, indices_sorted = indices[perm],
    so any other per-edge data is carried along as edata[key][perm].  Plain torch on the tensors' device; indptr is unchanged.
    RelNeighborSampler needs a graph in this order."""
    return _sort_csc_by_key(indptr, indices, etype, "types")


def check_etype_sorted(indptr, etype, num_rels, name="etype"):
    """What RelNeighborSampler asks of a graph's edge types, on the tensors' device: an integer tensor of num_edges values in
    [0, num_rels), non-decreasing inside every row of the CSC.  ValueError (naming sort_csc_by_etype) otherwise."""
    _check_sorted_in_rows(indptr, etype, name, "types", "", "sort_csc_by_etype(indptr, indices, etype)", num_rels)


def sort_csc_by_time(indptr, indices, ts):
    """Sort the in-edges of every node by timestamp, the twin of sort_csc_by_etype: -> (indices_sorted, ts_sorted, perm).  Stable by
    (row, time): simultaneous edges keep their CSC order.  perm (int64 [E]) maps new positions to old, indices_sorted = indices[perm],
    so any other per-edge data is carried along as edata[key][perm].  Plain torch on the tensors' device; indptr is unchanged.
    TemporalNeighborSampler needs a graph in this order."""
    return _sort_csc_by_key(indptr, indices, ts, "times")


def check_time_sorted(indptr, ts, name="ts"):
    """What TemporalNeighborSampler asks of a graph's edge timestamps, on the tensors' device: an integer tensor of num_edges values,
    non-decreasing inside every row of the CSC.  ValueError (naming sort_csc_by_time) otherwise."""
    _check_sorted_in_rows(indptr, ts, name, "times", " (floating-point timestamps are not supported)", "sort_csc_by_time(indptr, indices, ts)")


class CSCGraph(object):
    """int64 CSC (indptr[N+1], indices[E]) resident on one GPU + per-node data (labels...) + per-edge data in CSC order (edge weights
    for NeighborSampler(prob=key))."""

    def __init__(self, indptr, indices, ndata=None, edata=None):
        assert indptr.dtype == torch.int64 and indices.dtype == torch.int64
        assert indptr.is_cuda and indices.is_cuda, "the CSC arrays must be device tensors (HBM or a pinned-host alias)"
        self.indptr, self.indices = indptr.contiguous(), indices.contiguous()
        self.num_nodes = self.indptr.numel() - 1
        self.num_edges = self.indices.numel()
        self.device = self.indptr.device
        self.ndata = dict(ndata or {})
        self.edata = dict(edata or {})
        self._weights, self._etypes, self._etimes = {}, {}, {}   # edata key -> (the entry, its version, num_rels or None, the validated device copy): _edata
        self._max_in_degree = None
        self._src_sorted = None   # require_src_sorted: None = not checked yet, True = sorted, a ValueError = the refusal, kept
        self._h = C.c_void_p()
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _capi.check(_lib.coala_sampler_create(dev, self.indptr.data_ptr(), self.indices.data_ptr(), self.num_nodes,
                                              self.num_edges, C.byref(self._h)))

    @property
    def max_in_degree(self):
        """Largest in-degree of the graph: bounds the buffers of a full layer (fan-out -1).  Computed once, on first use."""
        if self._max_in_degree is None:
            self._max_in_degree = int((self.indptr[1:] - self.indptr[:-1]).max().item()) if self.num_nodes > 0 else 0
        return self._max_in_degree

    def require_src_sorted(self):
        """The second-order walks' demand at q != 1: rows sorted ascending by source id.  Checked once on the device (check_src_sorted)
        and remembered either way (the CSC arrays of a CSCGraph are not meant to change); ValueError (naming sort_csc_by_src) otherwise."""
        if self._src_sorted is None:
            try:
                check_src_sorted(self.indptr, self.indices)
                self._src_sorted = True
            except ValueError as e:
                self._src_sorted = e
        if self._src_sorted is not True:
            raise ValueError(str(self._src_sorted))

    def _edata(self, cache, key, role, make, tag=None):
        """edata[key] through `make` (validate, then the device copy the kernels read), kept in `cache` until the entry is replaced or
        modified in place or `tag` changes.  `role` names the sampler argument in the KeyError of a missing key."""
        if key not in self.edata:
            raise KeyError(f"edata has no {key!r}: the edge {role}={key!r}) (keys: {sorted(self.edata)})")
        t = self.edata[key]
        hit = cache.get(key)
        if hit is not None and hit[0] is t and hit[1] == t._version and hit[2] == tag:
            return hit[3]
        v = make(t)
        cache[key] = (t, t._version, tag, v)
        return v

    def edge_weights(self, key):
        """edata[key] as a contiguous fp32 tensor on the graph's device, validated once (num_edges values, finite, >= 0) and cached
        until the entry is replaced or modified in place.  KeyError when the key is missing, ValueError (naming it) when bad."""
        def make(t):
            if not isinstance(t, torch.Tensor) or t.is_complex():
                raise ValueError(f"edata[{key!r}]: edge weights must be a real tensor")
            if t.dim() != 1 or t.numel() != self.num_edges:
                raise ValueError(f"edata[{key!r}]: edge weights must have shape ({self.num_edges},) in CSC order, got {tuple(t.shape)}")
            w = t.to(device=self.device, dtype=torch.float32).contiguous()
            if w.numel() and bool((~torch.isfinite(w) | (w < 0)).any()):
                raise ValueError(f"edata[{key!r}]: edge weights must be finite and >= 0 (as fp32)")
            return w
        return self._edata(self._weights, key, "weights of NeighborSampler(prob", make)

    def edge_types(self, key, num_rels):
        """edata[key] as a contiguous int32 tensor on the graph's device for RelNeighborSampler, checked once on the device
        (check_etype_sorted: num_edges values in [0, num_rels), non-decreasing inside every row) and cached until the entry is replaced or
        modified in place, or close().  KeyError when the key is missing, ValueError (naming sort_csc_by_etype) when bad."""
        def make(t):
            check_etype_sorted(self.indptr, t, num_rels, key)
            return t.to(device=self.device, dtype=torch.int32).contiguous()
        return self._edata(self._etypes, key, "types of RelNeighborSampler(etype", make, num_rels)

    def edge_times(self, key):
        """edata[key] as a contiguous int64 tensor on the graph's device for TemporalNeighborSampler, checked once on the device
        (check_time_sorted: an integer tensor of num_edges values, non-decreasing inside every row) and cached until the entry is
        replaced or modified in place, or close().  KeyError when the key is missing, ValueError (naming sort_csc_by_time) when bad."""
        def make(t):
            check_time_sorted(self.indptr, t, key)
            return t.to(device=self.device, dtype=torch.int64).contiguous()
        return self._edata(self._etimes, key, "times of TemporalNeighborSampler(time", make)

    def close(self):
        self._etypes = {}
        self._etimes = {}
        if getattr(self, "_h", None):
            _lib.coala_sampler_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _EdgeData(dict):
    """block.edata of a block sampled with NeighborSampler(edge_ids=True): holds '_ID' (the CSC position of every neighbour slot, -1
    on padding); every other key of graph.edata is gathered through it on first access -- padding slots give 0 -- and kept.
    `lazy` (key -> function of no arguments) holds entries the sampler computes itself on first access (LaborSampler's
    'edge_weights'); they come before graph.edata, and they exist without edge ids (eid None: no '_ID', nothing gathered)."""

    def __init__(self, eid, graph, lazy=None):
        super().__init__({EID: eid} if eid is not None else {})
        self._source = graph.edata if graph is not None and eid is not None else {}
        self._lazy = dict(lazy or {})

    def __missing__(self, key):
        if key in self._lazy:
            v = self[key] = self._lazy[key]()
            return v
        src = self._source[key]               # KeyError for a key the graph does not have
        eid = self[EID]
        idx = eid.clamp_min(0)
        v = src[idx.to(src.device)].to(eid.device)
        v = v * (eid >= 0).to(v.dtype).view(eid.shape + (1,) * (v.dim() - eid.dim()))
        self[key] = v
        return v

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._lazy or key in self._source

    def get(self, key, default=None):
        return self[key] if key in self else default

    def keys(self):
        own = list(dict.keys(self)) + [k for k in self._lazy if not dict.__contains__(self, k)]
        return own + [k for k in self._source if k not in own]

    def materialised(self):
        """The tensors made so far (what Block.tensors() reports: a lazy entry nobody read holds no memory)."""
        return list(dict.values(self))


class Block(object):
    """One message-flow block: dst node d aggregates src rows nbr[d, j] >= 0 (fixed-stride form, a fixed fan-out), or
    indices[indptr[d]:indptr[d+1]] (ragged CSR form, a full layer: nbr is None).
    The first num_dst source nodes ARE the destination nodes (DGL's to_block convention)."""

    def __init__(self, src_nodes, nbr, num_dst, graph=None, dst_in_src=None, dst_nodes=None, owner_counts=None, owner_counts_host=None,
                 indptr=None, indices=None, eid=None, edata_graph=None, edata_lazy=None):
        self.src_nodes = src_nodes          # int64 [num_src] global ids
        self.nbr = nbr                      # int32 [num_dst, fanout], -1 padded; None for a full layer
        self.indptr = indptr                # int64 [num_dst + 1] (full layer) or None
        self.indices = indices              # int32 [E]: local source index of each in-edge (full layer) or None
        self.num_src = int(src_nodes.numel())
        self.num_dst = int(num_dst)
        # Owner-bucketed input layer (NeighborSampler(bucket_by_owner=G)): src_nodes is bucket 0 | bucket 1 | ... (stable inside a
        # bucket) instead of "dst nodes first", and dst_in_src[d] is where the d-th destination node sits in it.
        self.dst_in_src = dst_in_src        # int32 [num_dst] or None
        self.owner_counts = owner_counts    # device int64 [G] or None: what the partitioned fetch sends per owner
        self.owner_counts_host = owner_counts_host
        self.srcdata = {"_ID": src_nodes}
        self.dstdata = {"_ID": src_nodes[: self.num_dst] if dst_nodes is None else dst_nodes}
        # NeighborSampler(edge_ids=True): edata['_ID'] int64, shaped like nbr ([num_dst, fanout], -1 padded) or like indices ([E]), and
        # every graph.edata entry gathered through it on first access; LaborSampler: 'edge_weights', computed on first access, with or
        # without edge ids; an empty dict otherwise
        self.edata = _EdgeData(eid, edata_graph if edata_graph is not None else graph, edata_lazy) if eid is not None or edata_lazy else {}
        if graph is not None:
            for k, v in graph.ndata.items():  # blocks[-1].dstdata['labels'] (examples/sbatch_ssd_gnn_train.py:138)
                self.dstdata[k] = v[self.dstdata["_ID"]] if v.device == src_nodes.device else v[self.dstdata["_ID"].cpu()]

    def dst_rows(self, h_src):
        """Rows of the destination nodes inside a per-source tensor: h_src[:num_dst] (DGL's convention), or a gather through
        dst_in_src when the source list is owner-bucketed."""
        if self.dst_in_src is None:
            return h_src[: self.num_dst]
        return h_src[self.dst_in_src.to(torch.int64)]

    def tensors(self):
        """Every device tensor this block holds (for cross-stream lifetime bookkeeping by the prefetching loader)."""
        yield self.src_nodes
        for t in (self.nbr, self.indptr, self.indices, self.dst_in_src, self.owner_counts):
            if t is not None:
                yield t
        for d in (self.srcdata, self.dstdata):
            for v in d.values():
                if isinstance(v, torch.Tensor):
                    yield v
        for v in (self.edata.materialised() if isinstance(self.edata, _EdgeData) else self.edata.values()):
            if isinstance(v, torch.Tensor):
                yield v

    def number_of_src_nodes(self):
        return self.num_src

    def number_of_dst_nodes(self):
        return self.num_dst

    def int(self):   # examples/sbatch_ssd_gnn_train.py:139  block.int().to(device)
        return self

    def to(self, device):
        return self

    def _native_index(self):
        """The block's index tensors as the native ops take them, (nbr,) or (indptr, indices); None when they cannot: the tensors are
        not on the GPU, or nbr is not contiguous or has a fan-out above 32."""
        if self.nbr is None:
            if self.indptr.is_cuda and self.indices.is_cuda:
                return self.indptr.contiguous(), self.indices.contiguous()
        elif self.nbr.is_cuda and self.nbr.is_contiguous() and self.nbr.shape[1] <= 32:
            return (self.nbr,)
        return None

    def _slots(self, dev=None):
        """(row, local source index) of every neighbour slot in slot order, valid or not (-1: a padding slot): int64, on `dev` or, by
        default, on the block's device."""
        if self.nbr is None:
            deg = self.indptr[1:] - self.indptr[:-1]
            rows = torch.repeat_interleave(torch.arange(self.num_dst, device=deg.device), deg)
            src = self.indices.to(torch.int64)
        else:
            rows = torch.arange(self.num_dst, device=self.nbr.device).repeat_interleave(self.nbr.shape[1])
            src = self.nbr.reshape(-1).to(torch.int64)
        return (rows, src) if dev is None else (rows.to(dev), src.to(dev))

    def mean_aggregate(self, h_src):
        """Mean of the sampled neighbours' rows for every dst node: fp32 [num_dst, dim] (GraphSAGE 'mean').  Native kernel for
        fp32 2-D rows on the GPU (fan-out <= 32, or the ragged form of a full layer); plain torch otherwise.  A tensor with more than
        two dimensions ([num_src, H, D], GAT's output) takes the torch path, which keeps the trailing shape -- the rule of
        weighted_sum_aggregate, max_aggregate and rel_sum_aggregate -- and is not flattened for the kernel, which reads shape[1] as
        the row width."""
        index = self._native_index() if h_src.is_cuda and h_src.dtype == torch.float32 and h_src.dim() == 2 else None
        if index is not None:
            return (_MeanAggregateCSR if self.nbr is None else _MeanAggregate).apply(h_src, *index)
        return self.mean_aggregate_torch(h_src)

    def mean_aggregate_torch(self, h_src):
        """mean_aggregate in plain torch, any device and dtype, h_src [num_src, ...] -> [num_dst, ...]: its fallback, and its reference."""
        ones = (1,) * (h_src.dim() - 1)
        if self.nbr is None:   # ragged: sum the rows of each segment, divide by its length (an empty segment gives zeros)
            rows, idx = self._slots(h_src.device)
            valid = (idx >= 0).view((-1,) + ones).to(h_src.dtype)
            out = torch.zeros((self.num_dst,) + tuple(h_src.shape[1:]), dtype=h_src.dtype, device=h_src.device)
            out.index_add_(0, rows, h_src[idx.clamp_min(0)] * valid)
            deg = self.indptr[1:] - self.indptr[:-1]
            return out / deg.clamp_min(1).view((-1,) + ones).to(device=h_src.device, dtype=h_src.dtype)
        valid = (self.nbr >= 0).to(h_src.device)
        idx = self.nbr.clamp_min(0).to(device=h_src.device, dtype=torch.int64)
        g = h_src[idx] * valid.view(tuple(valid.shape) + ones).to(h_src.dtype)
        return g.sum(1) / valid.sum(1).clamp_min(1).view((-1,) + ones).to(h_src.dtype)

    def weighted_sum_aggregate(self, h_src, w):
        """Sum of the sampled neighbours' rows, each times its edge's weight, for every dst node: [num_dst, dim] (DGL's u_mul_e_sum,
        the edge_weight= path of GraphConv / SAGEConv).  w has one value per neighbour slot -- the shape of edata['_ID']: [num_dst,
        fanout] (padding slots are not read) or [E] on a ragged block.  Native kernels, with gradients for h_src and w, under the
        conditions of mean_aggregate (fp32 rows on the GPU; fan-out <= 32, or the ragged form); plain torch otherwise."""
        slots = self.indices if self.nbr is None else self.nbr
        if tuple(w.shape) != tuple(slots.shape):
            raise ValueError(f"edge weights of shape {tuple(w.shape)}: this block takes one per neighbour slot, {tuple(slots.shape)}")
        native = h_src.is_cuda and h_src.dtype == torch.float32 and h_src.dim() == 2 and w.is_cuda and w.dtype == torch.float32
        index = self._native_index() if native else None
        if index is not None:
            return (_WeightedSumCSR if self.nbr is None else _WeightedSum).apply(h_src, w, *index)
        return self.weighted_sum_aggregate_torch(h_src, w)

    def weighted_sum_aggregate_torch(self, h_src, w):
        """weighted_sum_aggregate in plain torch, any device and dtype, h_src [num_src, ...] -> [num_dst, ...]: its fallback, and its
        reference."""
        dev = h_src.device
        ones = (1,) * (h_src.dim() - 1)
        w = w.to(device=dev, dtype=h_src.dtype)
        if self.nbr is None:
            rows, idx = self._slots(dev)
            valid = (idx >= 0).to(h_src.dtype)
            out = torch.zeros((self.num_dst,) + tuple(h_src.shape[1:]), dtype=h_src.dtype, device=dev)
            return out.index_add(0, rows, h_src[idx.clamp_min(0)] * (w * valid).view((-1,) + ones))
        valid = (self.nbr >= 0).to(device=dev, dtype=h_src.dtype)
        idx = self.nbr.clamp_min(0).to(device=dev, dtype=torch.int64)
        return (h_src[idx] * (w * valid).view(tuple(valid.shape) + ones)).sum(1)

    def _rel_args(self, etype, num_rels, w):
        """The checks of rel_sum_aggregate / rel_sum_aggregate_torch / rel_in_degrees -> the block's slot array."""
        slots = self.indices if self.nbr is None else self.nbr
        if isinstance(num_rels, bool) or not isinstance(num_rels, int) or not 1 <= num_rels <= 64:
            raise ValueError(f"num_rels {num_rels!r}: 1..64 relations")
        if not _is_int_tensor(etype):
            raise ValueError("edge types must be an integer tensor")
        if tuple(etype.shape) != tuple(slots.shape):
            raise ValueError(f"edge types of shape {tuple(etype.shape)}: this block takes one per neighbour slot, {tuple(slots.shape)}")
        if w is not None and tuple(w.shape) != tuple(slots.shape):
            raise ValueError(f"edge weights of shape {tuple(w.shape)}: this block takes one per neighbour slot, {tuple(slots.shape)}")
        return slots

    def rel_sum_aggregate(self, h_src, etype, num_rels, w=None):
        """Sum of the sampled neighbours' rows per relation, for every dst node: [num_dst, num_rels, dim], out[d, r] = the sum over d's
        valid edges j of type etype_j == r of w_j * h_src[s_j] (RelGraphConv's message step: the result viewed as [num_dst, R * dim]
        times W viewed as [R * dim, out] is sum_j w_j W[etype_j] h_src[s_j]).  etype: any integer dtype, one value per neighbour slot
        -- the shape of edata['_ID'] -- converted once to contiguous int32; w: one weight per slot, or None for 1.  A padding slot's
        type and weight are not used; a valid edge whose type is outside [0, num_rels) contributes nothing; a relation absent from a
        row, and a row without an edge, give zeros.  Native kernels, with gradients for h_src and w, under the conditions of
        weighted_sum_aggregate; rel_sum_aggregate_torch otherwise."""
        self._rel_args(etype, num_rels, w)
        native = (h_src.is_cuda and h_src.dtype == torch.float32 and h_src.dim() == 2 and etype.is_cuda
                  and (w is None or (w.is_cuda and w.dtype == torch.float32)))
        index = self._native_index() if native else None
        if index is not None:
            lo, hi = -(1 << 31), (1 << 31) - 1   # a type that int32 cannot hold is out of range either way: -1
            t32 = etype if etype.dtype == torch.int32 else torch.where((etype < lo) | (etype > hi), -1, etype).to(torch.int32)
            return (_RelSumCSR if self.nbr is None else _RelSum).apply(h_src, w, *index, t32.contiguous(), num_rels)
        return self.rel_sum_aggregate_torch(h_src, etype, num_rels, w)

    def rel_sum_aggregate_torch(self, h_src, etype, num_rels, w=None):
        """rel_sum_aggregate in plain torch, any device and dtype, both block forms, the same skip rules: its fallback, and its
        reference.  It gathers an [E, dim] intermediate and index_adds it into num_dst * num_rels rows."""
        self._rel_args(etype, num_rels, w)
        dev = h_src.device
        rows, src = self._slots(dev)
        t = etype.reshape(-1).to(device=dev, dtype=torch.int64)
        keep = (src >= 0) & (t >= 0) & (t < num_rels)
        msg = h_src[src[keep]]
        if w is not None:
            msg = msg * w.reshape(-1).to(device=dev, dtype=h_src.dtype)[keep].view((-1,) + (1,) * (h_src.dim() - 1))
        out = torch.zeros((self.num_dst * num_rels,) + tuple(h_src.shape[1:]), dtype=h_src.dtype, device=dev)
        return out.index_add(0, rows[keep] * num_rels + t[keep], msg).view((self.num_dst, num_rels) + tuple(h_src.shape[1:]))

    def rel_in_degrees(self, etype, num_rels):
        """Valid in-edges of every destination node per relation: int64 [num_dst, num_rels], the c_{i,r} of the R-GCN paper; an edge
        whose type is outside [0, num_rels) is counted nowhere."""
        dev = self._rel_args(etype, num_rels, None).device
        rows, src = self._slots(dev)
        t = etype.reshape(-1).to(device=dev, dtype=torch.int64)
        keep = (src >= 0) & (t >= 0) & (t < num_rels)
        return torch.bincount(rows[keep] * num_rels + t[keep], minlength=self.num_dst * num_rels).view(self.num_dst, num_rels)

    def max_aggregate(self, h_src):
        """Element-wise maximum of the sampled neighbours' rows for every dst node: fp32 [num_dst, dim] (DGL's fn.max: SAGEConv 'pool',
        GINConv 'max').  torch.max(dim)'s rule over the valid slots in slot order: ties keep the first slot, which alone receives the
        gradient; a NaN propagates; a dst node without an in-edge gets zeros (DGL's reducer).  Native kernels under the conditions of
        mean_aggregate (fp32 2-D rows on the GPU; fan-out <= 32, or the ragged form); plain torch otherwise."""
        index = self._native_index() if h_src.is_cuda and h_src.dtype == torch.float32 and h_src.dim() == 2 else None
        if index is not None:
            return (_MaxAggregateCSR if self.nbr is None else _MaxAggregate).apply(h_src, *index)
        return self.max_aggregate_torch(h_src)

    def max_aggregate_torch(self, h_src, w=None, return_arg=False):
        """max_aggregate in plain torch, any device and dtype: its fallback, and its reference.  The winner of every (row, column) is
        found first -- the first NaN if the row holds one, else the first slot that equals the maximum -- and the output is gathered
        through it, so the gradient goes to that slot alone.  w (one value per neighbour slot, as weighted_sum_aggregate takes): the
        messages are h_src[s_j] * w_j (DGL's u_mul_e, then max).  return_arg: -> (out, arg), arg the int32 local source index of every
        winner, -1 for a row without a valid edge."""
        dev = h_src.device
        trail = tuple(h_src.shape[1:])
        ones = (1,) * len(trail)
        rows, src = self._slots(dev)
        E = src.numel()
        if E == 0:
            out = torch.zeros((self.num_dst,) + trail, dtype=h_src.dtype, device=dev)
            return (out, torch.full(out.shape, -1, dtype=torch.int32, device=dev)) if return_arg else out
        msg = h_src[src.clamp_min(0)]                                             # [E, ...]: every slot's message, in slot order
        if w is not None:
            msg = msg * w.reshape(-1).to(device=dev, dtype=h_src.dtype).view((E,) + ones)
        v = msg.detach()
        valid = (src >= 0).view((E,) + ones).expand_as(v)
        nan = valid & torch.isnan(v)
        at = rows.view((E,) + ones).expand_as(v)
        shape = (self.num_dst,) + trail
        vmax = torch.full(shape, float("-inf"), dtype=v.dtype, device=dev).scatter_reduce(
            0, at, torch.where(valid & ~nan, v, torch.full_like(v, float("-inf"))), "amax")
        has_nan = torch.zeros(shape, dtype=torch.int8, device=dev).scatter_reduce(0, at, nan.to(torch.int8), "amax").bool()
        wins = torch.where(has_nan[rows], nan, valid & ~nan & (v == vmax[rows]))
        slot = torch.arange(E, device=dev).view((E,) + ones).expand_as(v)
        first = torch.full(shape, E, dtype=torch.int64, device=dev).scatter_reduce(0, at, torch.where(wins, slot, torch.full_like(slot, E)), "amin")
        some = first < E
        first = first.clamp_max(E - 1)
        out = torch.where(some, msg.gather(0, first), torch.zeros((), dtype=msg.dtype, device=dev))
        if not return_arg:
            return out
        arg = torch.where(some, src.view((E,) + ones).expand_as(v).gather(0, first), torch.full_like(first, -1)).to(torch.int32)
        return out, arg

    def num_src_nodes(self):   # DGL's block API (examples/models.py calls block.num_dst_nodes())
        return self.num_src

    def num_dst_nodes(self):
        """Number of destination nodes.  On an owner-bucketed input block h[:num_dst_nodes()] is NOT the destination rows of a
        per-source tensor h: use dst_rows(h)."""
        return self.num_dst

    def _edges(self):
        """(row, local source index) of every valid edge, int64 on the block's device."""
        rows, src = self._slots()
        valid = src >= 0
        return rows[valid], src[valid]

    def in_degrees(self):
        """Valid in-edges of every destination node within the block: int64 [num_dst] (DGL's block.in_degrees())."""
        if self.nbr is not None:
            return (self.nbr >= 0).sum(1)
        rows, _ = self._edges()
        return torch.bincount(rows, minlength=self.num_dst)

    def out_degrees(self):
        """Edges leaving every source node within the block: int64 [num_src] (DGL's block.out_degrees())."""
        _, src = self._edges()
        return torch.bincount(src, minlength=self.num_src)

    def gat_aggregate(self, el, er, feat_src, negative_slope=0.2):
        """DGL GATConv's attention step: for every dst node d and head h, a softmax over d's valid in-edges of
        leaky_relu(el[s, h] + er[d, h], negative_slope), then sum_j a_j feat_src[s_j, h, :].  el [num_src, H], er [num_dst, H],
        feat_src [num_src, H, D] -> fp32 [num_dst, H, D]; a dst node without an in-edge gets zeros.  Native kernels (gradients for
        all three inputs) for fp32 GPU tensors, fan-out <= 32 or the ragged form of a full layer, and H <= 16; plain torch otherwise."""
        native = (el.is_cuda and er.is_cuda and feat_src.is_cuda and all(t.dtype == torch.float32 for t in (el, er, feat_src))
                  and feat_src.dim() == 3 and feat_src.shape[1] <= 16)
        index = self._native_index() if native else None
        if index is not None:
            return (_GatAggregateCSR if self.nbr is None else _GatAggregate).apply(el, er, feat_src, *index, float(negative_slope))
        return self.gat_aggregate_torch(el, er, feat_src, negative_slope)

    def gat_aggregate_torch(self, el, er, feat_src, negative_slope=0.2):
        """gat_aggregate in plain torch, any device and dtype: an edge-list softmax (scatter max, exp, index_add) that materialises the
        gathered [E, H, D] source rows.  The fallback of gat_aggregate, and its reference."""
        rows, src = self._edges()
        dev = feat_src.device
        rows, src = rows.to(dev), src.to(dev)
        H = feat_src.shape[1]
        e = torch.nn.functional.leaky_relu(el[src] + er[rows], negative_slope)              # [E, H]
        m = torch.full((self.num_dst, H), float("-inf"), dtype=e.dtype, device=dev)
        m = m.scatter_reduce(0, rows.unsqueeze(1).expand(-1, H), e.detach(), "amax").detach()   # the shift cancels in the softmax
        p = torch.exp(e - m[rows])
        l = torch.zeros((self.num_dst, H), dtype=e.dtype, device=dev).index_add(0, rows, p)
        a = p / l[rows]
        out = torch.zeros((self.num_dst,) + tuple(feat_src.shape[1:]), dtype=feat_src.dtype, device=dev)
        return out.index_add(0, rows, a.unsqueeze(-1).to(feat_src.dtype) * feat_src[src])

    def gatv2_aggregate(self, feat_src, feat_dst, attn, negative_slope=0.2):
        """DGL GATv2Conv's attention step: for every dst node d and head h, a softmax over d's valid in-edges of
        sum_c attn[h, c] * leaky_relu(feat_src[s, h, c] + feat_dst[d, h, c], negative_slope), then sum_j a_j feat_src[s_j, h, :].
        feat_src [num_src, H, D], feat_dst [num_dst, H, D], attn [H, D] or [1, H, D] -> [num_dst, H, D]; a dst node without an in-edge
        gets zeros.  Native kernels (gradients for all three inputs, no [E, H, D] intermediate) under the conditions of gat_aggregate:
        fp32 GPU tensors, fan-out <= 32 or the ragged form of a full layer, and H <= 16; plain torch otherwise."""
        if attn.dim() == 3 and attn.shape[0] == 1:
            attn = attn[0]
        if feat_src.dim() != 3 or tuple(attn.shape) != tuple(feat_src.shape[1:]) or tuple(feat_dst.shape) != (self.num_dst,) + tuple(attn.shape):
            raise ValueError(f"feat_src {tuple(feat_src.shape)}, feat_dst {tuple(feat_dst.shape)}, attn {tuple(attn.shape)}: this block takes "
                             f"[{self.num_src}, H, D], [{self.num_dst}, H, D] and [H, D] or [1, H, D]")
        native = (feat_src.is_cuda and feat_dst.is_cuda and attn.is_cuda and all(t.dtype == torch.float32 for t in (feat_src, feat_dst, attn))
                  and feat_src.shape[1] <= 16)
        index = self._native_index() if native else None
        if index is not None:
            return (_Gatv2AggregateCSR if self.nbr is None else _Gatv2Aggregate).apply(feat_src, feat_dst, attn, *index, float(negative_slope))
        return self.gatv2_aggregate_torch(feat_src, feat_dst, attn, negative_slope)

    def gatv2_aggregate_torch(self, feat_src, feat_dst, attn, negative_slope=0.2):
        """gatv2_aggregate in plain torch, any device and dtype: an edge-list softmax that materialises [E, H, D] (the gathered source
        rows, their sum with the destination rows, its leaky_relu).  The fallback of gatv2_aggregate, and its reference."""
        rows, src = self._edges()
        dev = feat_src.device
        rows, src = rows.to(dev), src.to(dev)
        H = feat_src.shape[1]
        fs = feat_src[src]                                                                       # [E, H, D]
        e = (torch.nn.functional.leaky_relu(fs + feat_dst[rows], negative_slope) * attn.reshape((1,) + tuple(feat_src.shape[1:]))).sum(-1)
        m = torch.full((self.num_dst, H), float("-inf"), dtype=e.dtype, device=dev)
        m = m.scatter_reduce(0, rows.unsqueeze(1).expand(-1, H), e.detach(), "amax").detach()   # the shift cancels in the softmax
        p = torch.exp(e - m[rows])
        l = torch.zeros((self.num_dst, H), dtype=e.dtype, device=dev).index_add(0, rows, p)
        a = p / l[rows]
        out = torch.zeros((self.num_dst,) + tuple(feat_src.shape[1:]), dtype=feat_src.dtype, device=dev)
        return out.index_add(0, rows, a.unsqueeze(-1).to(feat_src.dtype) * fs)

    def _rel_gat_args(self, el, er, feat, etype, num_rels, rows):
        """The checks of rel_gat_aggregate / rel_gat_aggregate_torch -> (el [P, H], feat [P, H, D]): the tables as the packed form takes
        them, the dense form's viewed as [num_src * R, ...]."""
        slots = self._rel_args(etype, num_rels, None)
        R = num_rels
        if rows is None:
            ok = feat.dim() == 4 and tuple(feat.shape[:2]) == (self.num_src, R) and tuple(el.shape) == tuple(feat.shape[:3])
            want = f"[{self.num_src}, {R}, H], [{self.num_dst}, {R}, H] and [{self.num_src}, {R}, H, D]"
        else:
            if not _is_int_tensor(rows):
                raise ValueError("rows must be an integer tensor")
            if tuple(rows.shape) != tuple(slots.shape):
                raise ValueError(f"rows of shape {tuple(rows.shape)}: this block takes one per neighbour slot, {tuple(slots.shape)}")
            ok = feat.dim() == 3 and tuple(el.shape) == tuple(feat.shape[:2])
            want = f"[P, H], [{self.num_dst}, {R}, H] and [P, H, D]"
        if not ok or tuple(er.shape) != (self.num_dst, R, feat.shape[-2]):
            raise ValueError(f"el {tuple(el.shape)}, er {tuple(er.shape)}, feat {tuple(feat.shape)}: this block takes {want}")
        H = feat.shape[-2]
        return el.reshape(-1, H), feat.reshape(-1, H, feat.shape[-1])

    def rel_gat_aggregate(self, el, er, feat, etype, num_rels, rows=None, negative_slope=0.2):
        """Relation-typed GAT attention (RelGATConv's message step; DGL's HeteroGraphConv over one GATConv per edge type, summed): for
        every dst node d, head h and relation r, a softmax of leaky_relu(el[.., h] + er[d, r, h], negative_slope) over d's valid
        in-edges of type r alone, then out[d, h, :] = sum_r sum_j a_j feat[.., h, :] -> [num_dst, H, D].  etype: any integer dtype, one
        value per neighbour slot, the shape of edata['_ID'].  er is [num_dst, R, H].  Which row of el / feat an edge reads:
          rows=None (dense): el [num_src, R, H], feat [num_src, R, H, D]; an edge of type r from source s reads el[s, r], feat[s, r];
          rows given (packed): el [P, H], feat [P, H, D]; rows has one integer per neighbour slot and the edge in slot j reads row
            rows_j < P (IndexError otherwise; on the native path that check is one host read per call).  A slot is then an edge
            exactly when rows_j >= 0: the block's own index array is not read.
        A relation absent from a row contributes nothing; a row without a valid edge gives zeros; a valid edge whose type is outside
        [0, num_rels) contributes nothing and receives no gradient.  Native kernels (one forward, one backward with gradients for el,
        er and feat) under the conditions of gat_aggregate -- fp32 GPU tensors, fan-out <= 32 or the ragged form, H <= 16 -- and
        R * H <= 256, for tables that are not empty; rel_gat_aggregate_torch otherwise."""
        el2, feat2 = self._rel_gat_args(el, er, feat, etype, num_rels, rows)
        R, H = num_rels, feat2.shape[1]
        native = (all(t.is_cuda and t.dtype == torch.float32 for t in (el, er, feat)) and etype.is_cuda and (rows is None or rows.is_cuda)
                  and H <= 16 and R * H <= 256 and 0 < feat2.shape[0] < (1 << 31) and feat2.shape[2] > 0)
        index = self._native_index() if native else None
        if index is None:
            return self.rel_gat_aggregate_torch(el, er, feat, etype, num_rels, rows, negative_slope)
        t = etype.to(torch.int64)
        if rows is None:
            src = index[-1].to(torch.int64)
            row = torch.where((src >= 0) & (t >= 0) & (t < R), src * R + t, -1)
        else:
            row = torch.where((t >= 0) & (t < R), rows.to(torch.int64), -1).clamp_min(-1)
            if row.numel() and int(row.max()) >= feat2.shape[0]:   # one host read: the kernels do not check an index they are given
                raise IndexError(f"rows holds {int(row.max())}: el and feat have {feat2.shape[0]} rows")
        t32 = t.clamp(-1, R).to(torch.int32)   # the kernel only compares a type with [0, R)
        fn = _RelGatAggregateCSR if self.nbr is None else _RelGatAggregate
        return fn.apply(el2, er, feat2, row.to(torch.int32).contiguous(), t32.contiguous(), R, *index, float(negative_slope))

    def rel_gat_aggregate_torch(self, el, er, feat, etype, num_rels, rows=None, negative_slope=0.2):
        """rel_gat_aggregate in plain torch, any device and dtype, both block forms, the same skip rules: an edge-list softmax keyed by
        dst * R + etype that materialises the gathered [E, H, D] rows.  The fallback of rel_gat_aggregate, and its reference."""
        el2, feat2 = self._rel_gat_args(el, er, feat, etype, num_rels, rows)
        dev = feat.device
        R, H = num_rels, feat2.shape[1]
        dst, src = self._slots(dev)
        t = etype.reshape(-1).to(device=dev, dtype=torch.int64)
        row = src * R + t if rows is None else rows.reshape(-1).to(device=dev, dtype=torch.int64)
        keep = ((src >= 0) if rows is None else (row >= 0)) & (t >= 0) & (t < R)
        dst, row, key = dst[keep], row[keep], dst[keep] * R + t[keep]
        e = torch.nn.functional.leaky_relu(el2[row] + er.reshape(-1, H)[key], negative_slope)       # [E, H]
        m = torch.full((self.num_dst * R, H), float("-inf"), dtype=e.dtype, device=dev)
        m = m.scatter_reduce(0, key.unsqueeze(1).expand(-1, H), e.detach(), "amax").detach()        # the shift cancels in the softmax
        p = torch.exp(e - m[key])
        l = torch.zeros((self.num_dst * R, H), dtype=e.dtype, device=dev).index_add(0, key, p)
        a = p / l[key]
        out = torch.zeros((self.num_dst,) + tuple(feat2.shape[1:]), dtype=feat2.dtype, device=dev)
        return out.index_add(0, dst, a.unsqueeze(-1).to(feat2.dtype) * feat2[row])


    def _dot_gat_args(self, q, k, v, rows, scale):
        """The checks of dot_gat_aggregate / dot_gat_aggregate_torch -> the scale as a float (None: D ** -0.5)."""
        slots = self.indices if self.nbr is None else self.nbr
        P = "P" if rows is not None else str(self.num_src)
        ok = k.dim() == 3 and tuple(v.shape) == tuple(k.shape) and tuple(q.shape) == (self.num_dst,) + tuple(k.shape[1:])
        if ok and rows is None:
            ok = k.shape[0] == self.num_src
        if not ok:
            raise ValueError(f"q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}: this block takes [{self.num_dst}, H, D], "
                             f"[{P}, H, D] and [{P}, H, D]")
        if rows is not None:
            if not _is_int_tensor(rows):
                raise ValueError("rows must be an integer tensor")
            if tuple(rows.shape) != tuple(slots.shape):
                raise ValueError(f"rows of shape {tuple(rows.shape)}: this block takes one per neighbour slot, {tuple(slots.shape)}")
        return float(k.shape[2]) ** -0.5 if scale is None else float(scale)

    def dot_gat_aggregate(self, q, k, v, rows=None, scale=None, validate=True):
        """Scaled dot-product attention (the message step of DGL's DotGatConv and HGTConv, PyG's TransformerConv without edge features):
        for every dst node d and head h, a softmax over d's in-edges j of scale * <q[d, h, :], k[.., h, :]>, then sum_j a_j v[.., h, :]
        -> [num_dst, H, D]; scale=None means D ** -0.5.  q is [num_dst, H, D].  Which row of k / v an edge reads:
          rows=None (dense): k and v are [num_src, H, D] and the edge in a slot reads the row of its source, the block's own index;
          rows given (packed): k and v are [P, H, D]; rows has one integer per neighbour slot -- rel_gat_aggregate's packed form -- and
            the edge in slot j reads row rows_j < P (IndexError otherwise; on the native path that check is one host read per call,
            which validate=False skips for a caller whose rows are an inverse index by construction).  A slot is then an edge exactly
            when rows_j >= 0: the block's own index array is not read.
        A dst node without an edge gets zeros.  k is v is allowed: autograd sums the two gradients.  Native kernels (one forward, one
        backward with gradients for q, k and v, no [E, H, D] intermediate) under the conditions of gat_aggregate -- fp32 GPU tensors,
        fan-out <= 32 or the ragged form, H <= 16 -- for tables that are not empty; dot_gat_aggregate_torch otherwise.  rows that is
        already contiguous int32 is handed to the kernels as it is."""
        scale = self._dot_gat_args(q, k, v, rows, scale)
        native = (all(t.is_cuda and t.dtype == torch.float32 for t in (q, k, v)) and (rows is None or rows.is_cuda) and k.shape[1] <= 16
                  and 0 < k.shape[0] < (1 << 31) and k.shape[1] > 0 and k.shape[2] > 0)
        index = self._native_index() if native else None
        if index is None:
            return self.dot_gat_aggregate_torch(q, k, v, rows, scale)
        if rows is None:
            row = index[-1]
        else:
            if validate and rows.numel() and int(rows.max()) >= k.shape[0]:   # one host read: the kernels do not check an index they are given
                raise IndexError(f"rows holds {int(rows.max())}: k and v have {k.shape[0]} rows")
            row = rows
            if row.dtype != torch.int32:
                row = row.clamp(-1, (1 << 31) - 1).to(torch.int32)
            row = row.contiguous()
        fn = _DotGatAggregateCSR if self.nbr is None else _DotGatAggregate
        return fn.apply(q, k, v, row, scale, *index)

    def dot_gat_aggregate_torch(self, q, k, v, rows=None, scale=None):
        """dot_gat_aggregate in plain torch, any device and dtype, both block forms, the dense and the packed form: an edge-list softmax
        that materialises the gathered [E, H, D] rows of k and v and their product with q.  The fallback of dot_gat_aggregate, and its
        reference."""
        scale = self._dot_gat_args(q, k, v, rows, scale)
        dev = k.device
        dst, src = self._slots(dev)
        row = src if rows is None else rows.reshape(-1).to(device=dev, dtype=torch.int64)
        keep = row >= 0
        dst, row = dst[keep], row[keep]
        if rows is not None and row.numel() and int(row.max()) >= k.shape[0]:   # the dense form's rows are the block's own
            raise IndexError(f"rows holds {int(row.max())}: k and v have {k.shape[0]} rows")
        H = k.shape[1]
        e = (q[dst] * k[row]).sum(-1) * scale                                                   # [E, H]
        m = torch.full((self.num_dst, H), float("-inf"), dtype=e.dtype, device=dev)
        m = m.scatter_reduce(0, dst.unsqueeze(1).expand(-1, H), e.detach(), "amax").detach()   # the shift cancels in the softmax
        p = torch.exp(e - m[dst])
        l = torch.zeros((self.num_dst, H), dtype=e.dtype, device=dev).index_add(0, dst, p)
        a = p / l[dst]
        out = torch.zeros((self.num_dst,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev)
        return out.index_add(0, dst, a.unsqueeze(-1).to(v.dtype) * v[row])

    def _exclude_args(self, eids):
        """The checks of exclude_edges / exclude_edges_torch -> the block's edge ids."""
        if not isinstance(self.edata, _EdgeData) or not dict.__contains__(self.edata, EID):
            raise ValueError("exclude_edges needs a block that carries edge ids (edata['_ID']): sample with edge_ids=True")
        made = [k for k in dict.keys(self.edata) if k != EID]
        if made:
            raise RuntimeError(f"exclude_edges: edata already holds {made}, made for the edges before the exclusion; exclude first")
        if not isinstance(eids, torch.Tensor) or eids.dtype != torch.int64 or eids.dim() != 1:
            raise ValueError("exclude_edges takes a sorted int64 tensor of edge ids, [n]")
        return self.edata[EID]

    def _excluded(self, nbr, indptr, indices, eid):
        """The block with its slots replaced: src_nodes, dst_in_src, owner_counts, srcdata and dstdata are this block's own (a source
        node that only an excluded edge reached stays in the list, unreferenced); edata is derived anew -- '_ID', graph edata through
        it, and LABOR's 'edge_weights' as 1 / surviving in-degree."""
        lazy = None
        if "edge_weights" in self.edata._lazy and indptr is not None:
            def edge_weights():
                deg = indptr[1:] - indptr[:-1]
                return torch.repeat_interleave(1.0 / deg.to(torch.float32), deg, output_size=int(indices.numel()))
            lazy = {"edge_weights": edge_weights}
        # The exclusion ran on the current stream and read this block's slot arrays, which the loader's sampler allocated on another: tell
        # the allocator, or it may hand them out again there while the kernels still read them (a no-op on the stream they came from).
        for t in (self.nbr, self.indptr, self.indices, self.edata[EID]):
            if t is not None and t.is_cuda:
                t.record_stream(torch.cuda.current_stream(t.device))
        b = Block(self.src_nodes, nbr, self.num_dst, dst_in_src=self.dst_in_src, owner_counts=self.owner_counts,
                  owner_counts_host=self.owner_counts_host, indptr=indptr, indices=indices, eid=eid, edata_lazy=lazy)
        b.edata._source = self.edata._source
        b.srcdata, b.dstdata = self.srcdata, self.dstdata
        return b

    def exclude_edges(self, eids):
        """-> a Block without the edges whose id (edata['_ID'], a CSC position) is in `eids`, a SORTED int64 tensor on the block's
        device: DGL's exclude= of as_edge_prediction_sampler, applied to a sampled block.  Fixed form: the surviving slots of a row move
        to its front in their old order and nbr and '_ID' hold -1 behind them; ragged form: a new indptr / indices / '_ID', the
        surviving edges in their old order.  An id that is in no slot changes nothing.  The source list is not recompacted.  Needs a
        block with edge ids (ValueError) whose edata holds no entry made for the old edges (RuntimeError).  Native kernels on the GPU
        (fan-out <= 32, or the ragged form, whose new size costs one host read); exclude_edges_torch otherwise."""
        eid = self._exclude_args(eids)
        index = self._native_index() if eids.is_cuda and eid.is_cuda else None
        if index is None:
            return self.exclude_edges_torch(eids)
        ex = eids.contiguous()
        eid = eid.contiguous()
        dev = eid.device.index or 0
        if self.nbr is not None:
            nbr, new_eid = torch.empty_like(index[0]), torch.empty_like(eid)
            _capi.check(_lib.coala_block_exclude_edges(dev, index[0].data_ptr(), eid.data_ptr(), ex.data_ptr(), ex.numel(), nbr.data_ptr(),
                                                       new_eid.data_ptr(), self.num_dst, index[0].shape[1], current_stream()))
            return self._excluded(nbr, None, None, new_eid)
        indptr, indices = index
        new_indptr = torch.zeros(self.num_dst + 1, dtype=torch.int64, device=eid.device)
        counts = torch.empty(self.num_dst, dtype=torch.int64, device=eid.device)
        args = (dev, indptr.data_ptr(), indices.data_ptr(), eid.data_ptr(), ex.data_ptr(), ex.numel())
        _capi.check(_lib.coala_block_exclude_edges_csr(*args, counts.data_ptr(), None, None, None, self.num_dst, current_stream()))
        torch.cumsum(counts, 0, out=new_indptr[1:])
        E = int(new_indptr[-1])
        new_indices = torch.empty(E, dtype=torch.int32, device=eid.device)
        new_eid = torch.empty(E, dtype=torch.int64, device=eid.device)
        _capi.check(_lib.coala_block_exclude_edges_csr(*args, None, new_indptr.data_ptr(), new_indices.data_ptr(), new_eid.data_ptr(), self.num_dst,
                                                       current_stream()))
        return self._excluded(None, new_indptr, new_indices, new_eid)

    def exclude_edges_torch(self, eids):
        """exclude_edges in plain torch (torch.isin and a stable sort), any device, the same rule: its fallback, and its reference."""
        eid = self._exclude_args(eids)
        listed = torch.isin(eid, eids.to(eid.device))
        if self.nbr is not None:
            keep = (self.nbr >= 0) & ~listed
            order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices   # survivors first, each part in its old order
            front = torch.arange(self.nbr.shape[1], device=keep.device).unsqueeze(0) < keep.sum(1, keepdim=True)
            nbr = torch.where(front, self.nbr.gather(1, order), torch.full_like(self.nbr, -1))
            return self._excluded(nbr, None, None, torch.where(front, eid.gather(1, order), torch.full_like(eid, -1)))
        keep = ~listed
        rows, _ = self._slots()
        indptr = torch.zeros(self.num_dst + 1, dtype=torch.int64, device=eid.device)
        torch.cumsum(torch.bincount(rows[keep], minlength=self.num_dst), 0, out=indptr[1:])
        return self._excluded(None, indptr, self.indices[keep], eid[keep])


class _Pending(object):
    """A sample_begin call on its way to sample_end: the graph, the seeds as the kernels got them, their number n, the fan-outs in sampling
    order (rev), per layer the src / nbr / indptr / eid buffers (an indptr entry is None for a fixed layer; eid is None without edge
    ids), the edge weights of prob= or None, and the call's ticket.  bucketed / owner_counts / dst_in_src: the owner-bucketing buffers,
    None when off.  extra: what one sampler kind carries besides (RandomWalkNeighborSampler's visit counts, TemporalNeighborSampler's decode
    context).  batch: the EdgeBatch an edge-prediction wrapper adds."""
    __slots__ = ("graph", "seeds", "n", "rev", "src", "nbr", "indptr", "eid", "weights", "ticket", "bucketed", "owner_counts", "dst_in_src",
                 "extra", "batch")

    def __init__(self, graph, seeds, n, rev, weights, extra):
        self.graph, self.seeds, self.n, self.rev, self.weights, self.extra = graph, seeds, n, rev, weights, extra
        self.eid = self.bucketed = self.owner_counts = self.dst_in_src = self.batch = None


class NeighborSampler(object):
    stream_safe = True  # every kernel and allocation of sample() goes to torch's current stream
    completes_on_host = True  # sample() / sample_end() return after the host has seen the event behind the sample's last kernel (coala_sampler_wait)

    def __init__(self, fanouts, seed=0, bucket_by_owner=0, prob=None, edge_ids=False):
        self.fanouts = [int(f) for f in fanouts]
        if not 1 <= len(self.fanouts) <= 8:
            raise ValueError("1..8 layers")
        for f in self.fanouts:   # -1: every in-edge (DGL's full neighbourhood); the block of such a layer is ragged (Block.indptr)
            if f != -1 and not 1 <= f <= 32:
                raise ValueError(f"fan-out {f}: each fan-out must be 1..32, or -1 for every in-edge")
        self.seed = int(seed)
        self.step = 0
        # G > 0: deliver the input nodes bucketed by owner = id % G, the layout the owner-partitioned cache fetches without a
        # routing pass and without an un-permute (blocks[0] then carries dst_in_src / owner_counts; see Block)
        self.bucket_by_owner = int(bucket_by_owner)
        if not 0 <= self.bucket_by_owner <= 64:
            raise ValueError("bucket_by_owner must be 0..64")
        # DGL's prob=: the edata key of non-negative per-edge weights.  A fixed layer then draws f distinct edges of positive weight
        # with probability proportional to it (all of them when there are at most f; never one of weight 0); a -1 layer still takes
        # every in-edge
        self.prob = prob
        # every block carries edata: '_ID' (DGL's dgl.EID; the CSC position of each sampled edge, written by the sampling kernels) and,
        # through it, graph.edata.  Off: edata is empty and the call is given no edge-id buffers
        self.edge_ids = bool(edge_ids)

    @staticmethod
    def make_graph(indptr, indices, ndata=None, edata=None):
        return CSCGraph(indptr, indices, ndata, edata)

    def sample(self, g, seed_nodes, step=None):
        """-> (input_nodes, output_nodes, blocks), blocks[0] is the input layer (DGL order)."""
        return self.sample_end(self.sample_begin(g, seed_nodes, step))

    def sample_begin(self, g, seed_nodes, step=None):
        """Enqueue the sample on the current stream and return without waiting (the kernels read their sizes from the device);
        sample_end(pending) collects the counts and builds the blocks.  A caller with something else to enqueue in between -- the
        loader launches step t+1's sample right behind step t's fetch -- never waits for the sampler at all."""
        return self._begin(_as_graph(g), seed_nodes, step)

    def _begin(self, g, seed_nodes, step, extra=None):
        """sample_begin: the buffers, the one C ABI call (_entry says which) on the current stream -> the call's _Pending record."""
        weights = g.edge_weights(self.prob) if self.prob is not None else None   # raises before any launch
        ragged = self._ragged
        seeds = seed_nodes.to(g.device, dtype=torch.int64).contiguous()
        n = seeds.numel()
        rev = list(reversed(self.fanouts))          # DGL samples the output layer first
        L = len(rev)
        # capacities (include/coala_hip.h, coala_sampler_layer_t): exact host bounds up to the first full layer; a full layer holds
        # at most cap * max_in_degree edges and never more than ITEM_LIMIT items, which bounds every layer behind it
        caps, src_caps, edge_caps = [n], [], []
        bounded = False
        for f in rev:
            cap = caps[-1]
            if ragged(f):   # a LABOR layer takes ~cap * f edges, but only the device knows: the bound is the full layer's
                edge_caps.append(min(cap * self._row_bound(g, f), ITEM_LIMIT))
                src_caps.append(min(cap + edge_caps[-1], ITEM_LIMIT))
                bounded = True
            elif bounded:
                src_caps.append(min(cap * (f + 1), ITEM_LIMIT))
                edge_caps.append(min(cap * f, ITEM_LIMIT))
            else:
                src_caps.append(cap * (f + 1))
                edge_caps.append(cap * f)
            caps.append(src_caps[-1])
        p = _Pending(g, seeds, n, rev, weights, extra)
        p.src = [torch.empty(max(src_caps[l], 1), dtype=torch.int64, device=g.device) for l in range(L)]
        p.nbr = [torch.empty(max(edge_caps[l], 1), dtype=torch.int32, device=g.device) for l in range(L)]
        p.indptr = [torch.empty(caps[l] + 1, dtype=torch.int64, device=g.device) if ragged(rev[l]) else None for l in range(L)]
        if self.edge_ids:
            p.eid = [torch.empty(max(edge_caps[l], 1), dtype=torch.int64, device=g.device) for l in range(L)]
        G = self.bucket_by_owner
        bk = None
        if G > 0:
            p.bucketed = torch.empty(max(caps[L], 1), dtype=torch.int64, device=g.device)
            p.owner_counts = torch.empty(G, dtype=torch.int64, device=g.device)
            p.dst_in_src = torch.empty(max(caps[L - 1], 1), dtype=torch.int32, device=g.device)
            bk = C.byref(_capi.SamplerBucketing(G, 0, p.bucketed.data_ptr(), p.owner_counts.data_ptr(), p.dst_in_src.data_ptr()))
        lay = (_capi.SamplerLayer * L)(*[_capi.SamplerLayer(p.src[l].data_ptr(), p.nbr[l].data_ptr(), p.indptr[l].data_ptr() if p.indptr[l] is not None else None,
                                                            src_caps[l], edge_caps[l]) for l in range(L)])
        eid_p = (C.c_void_p * L)(*[t.data_ptr() for t in p.eid]) if p.eid is not None else None
        fn, fans, kind = self._entry(p, (C.c_int32 * L)(*rev), eid_p)
        ticket = C.c_int64(-1)
        # three launches per layer, nothing else: no host wait here (n_src_host = n_edges_host = NULL)
        _capi.check(fn(g._h, seeds.data_ptr(), n, *fans, self.seed, self.step if step is None else int(step), lay, *kind, None, None,
                       *((bk,) if self._takes_bucketing else ()), C.byref(ticket), current_stream()))
        p.ticket = ticket.value
        if step is None:
            self.step += 1
        return p

    def _ragged(self, f):
        """Whether a layer of fan-out f gives a ragged (CSR) block, whose size only the device knows."""
        return f == -1

    def _row_bound(self, g, f):
        """The most edges a row of a ragged layer of fan-out f can hold, known on the host."""
        return g.max_in_degree

    _takes_bucketing = True   # whether the C entry point of _entry has a bucketing argument

    def _entry(self, p, fan, eid_p):
        """The C entry point of this sampler kind -> (function, its fan-out arguments, its arguments between `layers` and `n_src_host`).
        A kind with buffers of its own allocates them here, into p.extra."""
        return (_lib.coala_sampler_sample_layers_edge_ids, (fan, len(p.rev)), (p.weights.data_ptr() if p.weights is not None else None, eid_p))

    def _wait(self, p):
        """Wait for the counts of a sample_begin (an event wait: only for that call's kernels) -> per layer the source nodes and the
        edges, and the owner counts or None.  Raises when the device refused a full layer (or the fixed layers behind it) for its size."""
        L = len(p.rev)
        n_src = (C.c_int64 * L)()
        n_edges = (C.c_int64 * L)()
        ch = (C.c_int64 * self.bucket_by_owner)() if p.owner_counts is not None else None
        _capi.check(_lib.coala_sampler_wait_layers(p.graph._h, p.ticket, n_src, n_edges, ch))
        return n_src, n_edges, list(ch) if ch is not None else None

    def sample_end(self, pending):
        """Wait for the counts of a sample_begin and build the blocks."""
        p = pending
        g, L = p.graph, len(p.rev)
        n_src, n_edges, counts_host = self._wait(p)
        blocks = []
        n_dst = p.n
        for l in range(L):
            ns, f = n_src[l], p.rev[l]
            if p.indptr[l] is not None:   # ragged block: CSR over the destination nodes
                nbr_l = None
                csr = dict(indptr=p.indptr[l][: n_dst + 1], indices=p.nbr[l][: n_edges[l]], **self._block_extras(p.indptr[l][: n_dst + 1], n_edges[l], f))
                if p.eid is not None:
                    csr["eid"] = p.eid[l][: n_edges[l]]
            else:
                nbr_l = p.nbr[l][: n_dst * f].view(n_dst, f)
                csr = {} if p.eid is None else dict(eid=p.eid[l][: n_dst * f].view(n_dst, f))
            if p.owner_counts is not None and l == L - 1:   # the input layer: owner-bucketed source list
                blocks.insert(0, Block(p.bucketed[:ns], nbr_l, n_dst, graph=g if l == 0 else None, edata_graph=g, dst_in_src=p.dst_in_src[:n_dst],
                                       dst_nodes=p.src[l][:n_dst], owner_counts=p.owner_counts, owner_counts_host=counts_host, **csr))
            else:
                blocks.insert(0, Block(p.src[l][:ns], nbr_l, n_dst, graph=g if l == 0 else None, edata_graph=g, **csr))
            n_dst = ns
        input_nodes = blocks[0].src_nodes
        return input_nodes, p.seeds, blocks

    def _block_extras(self, indptr, n_edges, f):
        """More Block arguments for a ragged layer of fan-out f."""
        return {}


class LaborSampler(NeighborSampler):
    """Layer-neighbour sampling, DGL's dgl.dataloading.LaborSampler with importance_sampling=0 (Balin & Catalyurek, "Layer-Neighbor
    Sampling -- Defusing Neighborhood Explosion in GNNs", NeurIPS 2023), in place of NeighborSampler: same interface, same loader.
    A layer draws one random number per SOURCE node and shares it among its destination nodes, so destination nodes with a common
    neighbour agree on taking it: every row still holds `fanout` neighbours in expectation (all of them when it has no more), but
    the batch has fewer distinct input nodes to fetch.  The rule is in the header of coala_sampler.hip.

    Every block is ragged (Block.indptr / Block.indices, nbr is None), whatever the fan-out; -1 is the full layer of NeighborSampler.
    block.edata['edge_weights'] (fp32 [E], made on first access) is 1 / in_degree(d) of the edge's row in the block, DGL's
    Hajek-normalised weight -- all taken edges of a LABOR-0 row have the same inclusion probability.
    layer_dependency=True uses the same random numbers in every layer of a call (DGL's option of that name).
    A row's length is random, so the buffers are those of a full layer (cap * max_in_degree edges, at most ITEM_LIMIT items); the
    loader sizes its fetch buffers from its fan_out argument as batch * prod(f + 1), the bound of NeighborSampler's input nodes."""

    def __init__(self, fanouts, seed=0, bucket_by_owner=0, edge_ids=False, layer_dependency=False, importance_sampling=0, prob=None):
        if prob is not None:
            raise ValueError("LaborSampler: prob= (weighted LABOR) is not supported")
        if importance_sampling != 0:
            raise ValueError(f"LaborSampler: importance_sampling={importance_sampling!r} is not supported, only 0 (LABOR-0)")
        super().__init__(fanouts, seed=seed, bucket_by_owner=bucket_by_owner, edge_ids=edge_ids)
        self.layer_dependency = bool(layer_dependency)
        self.importance_sampling = 0

    def _ragged(self, f):
        return True

    def _entry(self, p, fan, eid_p):
        return _lib.coala_sampler_sample_layers_labor, (fan, len(p.rev)), (eid_p, int(self.layer_dependency))

    def _block_extras(self, indptr, n_edges, f):
        def edge_weights():
            deg = indptr[1:] - indptr[:-1]
            return torch.repeat_interleave(1.0 / deg.to(torch.float32), deg, output_size=n_edges)
        return dict(edata_lazy={"edge_weights": edge_weights})


class RelNeighborSampler(NeighborSampler):
    """Neighbour sampling with a fan-out per edge type, what DGL's NeighborSampler does on a heterograph (on a homogenised graph:
    dgl.sort_csc_by_tag, then sample_etype_neighbors(etype_sorted=True)), in place of NeighborSampler: same interface, same loader.
    The graph carries its edge types in graph.edata[etype] (any integer dtype, CSC order, values in [0, num_rels)), and the in-edges of
    every node must be sorted by type -- sort_csc_by_etype does that.  The first sample from a graph checks it once on the device and
    keeps an int32 copy on the CSCGraph (until close()); a graph that fails raises ValueError before anything is launched.

    fanouts: one entry per layer (model order, as NeighborSampler's), each an int applied to every relation (as DGL does) or a
    sequence of num_rels ints.  Per relation: 0 takes nothing, -1 every in-edge of that type, f in 1..32 at most f of them, drawn
    without replacement (all when the node has at most f); a layer needs one non-zero entry.  The rule is in the header of
    coala_sampler.hip: relations draw from streams of their own, and with num_rels == 1 a row holds the edges NeighborSampler draws.

    Every block is ragged (Block.indptr / Block.indices, nbr is None); a row lists its edges in ascending CSC position, so grouped by
    relation.  With edge_ids (the default here: RelGraphConv reads block.edata[etype] through them) the blocks carry edata.
    self.fanouts holds the per-layer totals -- the sum of a layer's fan-outs, or -1 when one of them is -1.  A layer without a -1 holds at
    most min(total, max_in_degree) edges per row, which sizes its buffers; one with a -1 is sized as a full layer.  The loader sizes its
    fetch buffers from its fan_out argument and knows nothing of relations: pass it these totals (sampler.fanouts)."""

    def __init__(self, fanouts, num_rels, etype="etype", seed=0, bucket_by_owner=0, edge_ids=True, prob=None):
        if prob is not None:
            raise ValueError("RelNeighborSampler: prob= (weighted draws per relation) is not supported")
        if isinstance(num_rels, bool) or not isinstance(num_rels, int) or not 1 <= num_rels <= 64:
            raise ValueError(f"num_rels {num_rels!r}: 1..64 relations")
        fanouts = list(fanouts)
        super().__init__([-1] * len(fanouts), seed=seed, bucket_by_owner=bucket_by_owner, edge_ids=edge_ids)
        self.num_rels, self.etype = num_rels, etype
        self.rel_fanouts = []
        for f in fanouts:
            per_rel = [int(x) for x in f] if hasattr(f, "__iter__") else [int(f)] * num_rels
            if len(per_rel) != num_rels:
                raise ValueError(f"fan-outs {per_rel}: a layer takes one int, or one per relation ({num_rels})")
            for x in per_rel:
                if not -1 <= x <= 32:
                    raise ValueError(f"fan-out {x}: each fan-out must be 0..32, or -1 for every in-edge of the relation")
            if not any(per_rel):
                raise ValueError(f"fan-outs {per_rel}: a layer must take edges of at least one relation")
            self.rel_fanouts.append(per_rel)
        self.fanouts = [-1 if -1 in per_rel else sum(per_rel) for per_rel in self.rel_fanouts]

    def _ragged(self, f):
        return True

    def _row_bound(self, g, f):
        return g.max_in_degree if f == -1 else min(f, g.max_in_degree)

    def _entry(self, p, fan, eid_p):
        types = p.graph.edge_types(self.etype, self.num_rels)   # raises before any launch
        L = len(p.rev)
        rel_fan = (C.c_int32 * (L * self.num_rels))(*[f for per_rel in reversed(self.rel_fanouts) for f in per_rel])
        return _lib.coala_sampler_sample_layers_rel, (rel_fan, self.num_rels, L), (types.data_ptr(), eid_p)


def _walk_threshold(prob, name):
    """floor(prob * 2^53) as an int: the integer the walk kernels compare 53 random bits with.  The product is exact in fp64."""
    if isinstance(prob, bool) or not isinstance(prob, (int, float)) or not 0.0 <= float(prob) < 1.0:
        raise ValueError(f"{name} {prob!r}: a probability in [0, 1)")
    return int(float(prob) * 9007199254740992.0)


class RandomWalkNeighborSampler(NeighborSampler):
    """Importance-based neighbour sampling by random walks, DGL's dgl.sampling.RandomWalkNeighborSampler / PinSAGESampler on a homogeneous
    graph (Ying et al., "Graph Convolutional Neural Networks for Web-Scale Recommender Systems", KDD 2018), in place of NeighborSampler:
    same sample / sample_begin / sample_end, same loader.  From every destination node num_random_walks walks of num_traversals hops
    start; a hop after the first ends the walk with probability termination_prob.  The node's neighbours are the num_neighbors nodes
    the walks visit most often (a tie goes to the smaller id), most visited first.  The rule is in the header of coala_sampler.hip.

    num_neighbors: an int (one layer) or one per layer in model order, each 1..32; it is self.fanouts, what the loader is given: the
    input nodes are bounded as NeighborSampler's, batch * prod(k + 1).  num_traversals 1..16, num_random_walks 1..64, their product at
    most 512; termination_prob in [0, 1).  A walk follows in-edges, the direction the CSC is stored in: DGL's walk on a symmetric graph.
    Every block is fixed-stride (Block.nbr [num_dst, k], -1 padded).  block.edata[weight_column] is fp32 [num_dst, k], the visit count
    of every slot (0 on padding), made on first access from the int32 counts the kernel wrote (block.edata['visit_counts']): what
    Block.weighted_sum_aggregate and SAGEConv / GraphConv (edge_weight=) take.  A chosen neighbour is a node the walks reached, not an edge of the graph: there are no
    edge ids, and prob= is not supported."""

    def __init__(self, num_neighbors, num_traversals, termination_prob, num_random_walks, seed=0, bucket_by_owner=0, weight_column="weights",
                 prob=None, edge_ids=False):
        if prob is not None:
            raise ValueError("RandomWalkNeighborSampler: prob= (weighted walks) is not supported")
        if edge_ids:
            raise ValueError("RandomWalkNeighborSampler: edge_ids is not supported: a chosen neighbour is not an edge of the graph")
        ks = [num_neighbors] if isinstance(num_neighbors, int) else list(num_neighbors)
        for k in ks:
            if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 32:
                raise ValueError(f"num_neighbors {k!r}: each layer keeps 1..32 neighbours")
        for name, x, hi in (("num_traversals", num_traversals, 16), ("num_random_walks", num_random_walks, 64)):
            if isinstance(x, bool) or not isinstance(x, int) or not 1 <= x <= hi:
                raise ValueError(f"{name} {x!r}: 1..{hi}")
        if num_traversals * num_random_walks > 512:
            raise ValueError(f"num_random_walks * num_traversals = {num_traversals * num_random_walks}: at most 512 visits per node")
        self.term_threshold = _walk_threshold(termination_prob, "termination_prob")
        super().__init__(ks, seed=seed, bucket_by_owner=bucket_by_owner)
        self.num_neighbors = list(self.fanouts)
        self.num_traversals, self.num_random_walks, self.termination_prob = num_traversals, num_random_walks, float(termination_prob)
        self.weight_column = weight_column

    def _entry(self, p, fan, eid_p):
        p.extra = [torch.empty_like(t) for t in p.nbr]   # int32 [edge_cap] per layer: the visit count of every neighbour slot
        cnt_p = (C.c_void_p * len(p.extra))(*[t.data_ptr() for t in p.extra])
        walk = _capi.SamplerWalk(self.num_traversals, self.num_random_walks, self.term_threshold)
        return _lib.coala_sampler_sample_layers_walk, (fan, len(p.rev)), (C.byref(walk), cnt_p)

    def sample_end(self, pending):
        input_nodes, seeds, blocks = super().sample_end(pending)
        for l, b in enumerate(reversed(blocks)):   # counts are in sampling order, blocks in model order
            c = pending.extra[l][: b.nbr.numel()].view(b.nbr.shape)
            b.edata = _EdgeData(None, None, {self.weight_column: lambda c=c: c.to(torch.float32)})
            b.edata["visit_counts"] = c   # the kernel's int32 counts: held by the block, so Block.tensors() reports their buffer
        return input_nodes, seeds, blocks


def random_walk(g, nodes, length, restart_prob=0.0, num_walks=1, seed=0, step=0):
    """Random walks over a CSCGraph, DGL's dgl.sampling.random_walk on a homogeneous graph: -> int64 [n, num_walks, length + 1] on the
    graph's device.  [i, w, 0] is nodes[i], then the nodes walk w visits; a hop after the first ends the walk with probability
    restart_prob, a node without an in-edge ends it, and -1 fills the rest.  An out-of-range start node gives a row of -1.  A walk
    follows in-edges (DGL's walk on a symmetric graph).  length 1..16, num_walks 1..64.
    Unlike DGL's, the walks are a function of (seed, step, start node, w) -- they are walk w of that node in the first sampled layer of
    RandomWalkNeighborSampler(num_traversals=length, termination_prob=restart_prob, seed=seed) at that step -- so a start node given
    twice gets the same traces twice: ask for num_walks independent walks from one node instead of repeating it."""
    for name, x, hi in (("length", length, 16), ("num_walks", num_walks, 64)):
        if isinstance(x, bool) or not isinstance(x, int) or not 1 <= x <= hi:
            raise ValueError(f"{name} {x!r}: 1..{hi}")
    thr = _walk_threshold(restart_prob, "restart_prob")
    g = _as_graph(g)
    nodes = nodes.to(g.device, dtype=torch.int64).contiguous()
    out = torch.empty((nodes.numel(), num_walks, length + 1), dtype=torch.int64, device=g.device)
    _capi.check(_lib.coala_sampler_random_walk(g._h, nodes.data_ptr(), nodes.numel(), num_walks, length, thr, _u64(seed), _u64(step), 0,
                                               out.data_ptr(), current_stream()))
    return out


MAX_WALK_LENGTH = 127      # hops of a second-order walk (coala_sampler.hip: kN2vMaxLength)
MAX_WALK_NEGATIVES = 16    # negative rows per walk of a walk batch (kN2vMaxNeg)
_MIN_ACCEPT = 1 << 28      # smallest threshold node2vec_random_walk takes: an acceptance ratio of 1/16


def node2vec_thresholds(p, q):
    """(thr_return, thr_near, thr_far) of node2vec's return parameter p and in-out parameter q, the three integers the walk kernel
    compares 32 random bits with: m = max(1/p, 1, 1/q), int((1/p) / m * 2^32), int(1 / m * 2^32), int((1/q) / m * 2^32), in float64.
    The largest is exactly 2^32.  ValueError unless p, q > 0 and finite."""
    for name, x in (("p", p), ("q", q)):
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not 0.0 < float(x) < float("inf"):
            raise ValueError(f"{name} {x!r}: a positive finite number")
    a, b = 1.0 / float(p), 1.0 / float(q)
    m = max(a, 1.0, b)
    return int(a / m * 4294967296.0), int(1.0 / m * 4294967296.0), int(b / m * 4294967296.0)


def sort_csc_by_src(indptr, indices):
    """Sort the in-edges of every node by source id, the twin of sort_csc_by_etype / sort_csc_by_time: -> (indices_sorted, perm).  Stable:
    repeated edges keep their CSC order.  perm (int64 [E]) maps new positions to old, indices_sorted = indices[perm], so per-edge data
    is carried along as edata[key][perm].  Plain torch on the tensors' device; indptr is unchanged.  node2vec_random_walk and walk_batch
    need a graph in this order when q != 1 (synthetic.symmetrize_csc already produces it)."""
    srt, _, perm = _sort_csc_by_key(indptr, indices, indices, "sources")
    return srt, perm


def check_src_sorted(indptr, indices):
    """What the second-order walks ask of a graph at q != 1, on the tensors' device: source ids non-decreasing inside every row of the
    CSC.  ValueError (naming sort_csc_by_src) otherwise."""
    E = indices.numel()
    if E < 2:
        return
    drop = indices[1:] < indices[:-1]
    starts = indptr[1:-1]
    starts = starts[(starts > 0) & (starts < E)]
    drop[starts - 1] = False
    if bool(drop.any()):
        raise ValueError("the rows of the graph must be sorted ascending by source id for a second-order walk with q != 1; sort it with "
                         "COALA_GNN.sampler.sort_csc_by_src(indptr, indices)")


def _walk_args(g, nodes, p, q, walk_length, num_walks, what):
    """The checks node2vec_random_walk and walk_batch share -> (graph, start nodes on its device, thresholds)."""
    for name, x, hi in (("walk_length", walk_length, MAX_WALK_LENGTH), ("num_walks", num_walks, 64)):
        if isinstance(x, bool) or not isinstance(x, int) or not 1 <= x <= hi:
            raise ValueError(f"{name} {x!r}: 1..{hi}")
    thr = node2vec_thresholds(p, q)
    if min(thr) < _MIN_ACCEPT:
        raise ValueError(f"p={p!r}, q={q!r}: the smallest of 1/p, 1, 1/q is below 1/16 of the largest; a hop gives up after 256 rejected "
                         f"candidates, which such a ratio would reach too often")
    g = _as_graph(g)
    if thr[1] != thr[2]:
        g.require_src_sorted()
    nodes = nodes.to(g.device, dtype=torch.int64).contiguous()
    if nodes.dim() != 1:
        raise ValueError(f"start nodes of shape {tuple(nodes.shape)}: {what} takes a 1-D tensor of node ids")
    return g, nodes, thr


def node2vec_random_walk(g, nodes, p, q, walk_length, num_walks=1, seed=0, step=0):
    """node2vec's second-order random walks over a CSCGraph, DGL's dgl.sampling.node2vec_random_walk on a homogeneous graph: -> int64
    [n, num_walks, walk_length + 1] on the graph's device.  [i, w, 0] is nodes[i], then the nodes walk w visits; from `cur`, having come
    from `prev`, an in-neighbour x of cur is taken with a weight of 1/p when x == prev, 1 when x is an in-neighbour of prev, 1/q
    otherwise (rejection sampling; the exact integer rule is in the header of coala_sampler.hip).  A node without an in-edge ends the
    walk and -1 fills the rest; an out-of-range start node gives a row of -1.  A walk follows in-edges (DGL's walk on a symmetric
    graph).  walk_length 1..127, num_walks 1..64, p, q > 0 with min(1/p, 1, 1/q) / max(1/p, 1, 1/q) >= 1/16 (the node2vec paper's grid
    0.25 .. 4 just fits); with q != 1 the rows of the graph must be sorted by source id (sort_csc_by_src; checked once per graph).
    The walks are a function of (seed, step, start node, w) on a stream of their own: at p = q = 1 they are valid uniform walks, but
    NOT the traces random_walk gives for the same arguments; and a start node given twice gets the same traces twice."""
    g, nodes, thr = _walk_args(g, nodes, p, q, walk_length, num_walks, "node2vec_random_walk")
    out = torch.empty((nodes.numel(), num_walks, walk_length + 1), dtype=torch.int64, device=g.device)
    _capi.check(_lib.coala_sampler_node2vec_walk(g._h, nodes.data_ptr(), nodes.numel(), num_walks, walk_length, *thr, _u64(seed), _u64(step),
                                                 out.data_ptr(), current_stream()))
    return out


def _batch_begin(entry, g, *args):
    """One batch call on the current stream, without waiting -> its ticket.  args: `entry`'s, between the handle and ticket_out."""
    ticket = C.c_int64(-1)
    _capi.check(entry(g._h, *args, C.byref(ticket), current_stream()))
    return ticket.value


def _batch_collect(wait, g, ticket):
    """Wait for the event behind a batch call (only for its kernels) -> (n_nodes, n_bad)."""
    n_nodes, n_bad = C.c_int64(0), C.c_int64(0)
    _capi.check(wait(g._h, ticket, C.byref(n_nodes), C.byref(n_bad)))
    return n_nodes.value, n_bad.value


class WalkBatch(object):
    """One skip-gram minibatch of walks.  input_nodes: int64 [n_nodes], the distinct nodes of the batch in order of first appearance
    (the start nodes first); pos int32 [n * W, L + 1]: every walk as indices into input_nodes, -1 once it has ended; neg int32
    [n * W * K, L + 1]: K rows per walk, the walk's start node in column 0 and uniformly drawn nodes behind it (PyG's neg_sample);
    traces: int64 [n, W, L + 1] global ids (node2vec_random_walk's, bit for bit), or None when not asked for.  n_bad: how many start
    nodes were outside the graph; their rows of pos, neg and traces are -1 and they add no node."""

    def __init__(self, nodes, input_nodes, pos, neg, traces=None, n_bad=0):
        self.nodes, self.input_nodes, self.pos, self.neg, self.traces, self.n_bad = nodes, input_nodes, pos, neg, traces, n_bad

    def tensors(self):
        """Every device tensor the batch holds (the loader's lifetime bookkeeping, as Block.tensors())."""
        return [t for t in (self.nodes, self.input_nodes, self.pos, self.neg, self.traces) if t is not None]


def walk_batch_begin(g, nodes, p, q, walk_length, num_walks=1, num_neg=1, seed=0, step=0, traces=False):
    """Enqueue the walk-batch kernels for the start nodes on the current stream, without waiting: -> the pending call walk_batch_end
    takes.  ValueError before any launch for arguments node2vec_random_walk refuses, num_neg outside 0..16, or more than ITEM_LIMIT
    = n * num_walks * (walk_length + 1) * (1 + num_neg) items."""
    if isinstance(num_neg, bool) or not isinstance(num_neg, int) or not 0 <= num_neg <= MAX_WALK_NEGATIVES:
        raise ValueError(f"num_neg {num_neg!r}: 0..{MAX_WALK_NEGATIVES} negative rows per walk")
    g, nodes, thr = _walk_args(g, nodes, p, q, walk_length, num_walks, "walk_batch")
    n, W, L1, K = nodes.numel(), num_walks, walk_length + 1, num_neg
    items = n + n * W * L1 + n * W * K * walk_length
    if max(n * W * L1 * (1 + K), items) > ITEM_LIMIT:
        raise ValueError(f"{n} start nodes, {W} walks of {walk_length} hops and {K} negatives hold {max(n * W * L1 * (1 + K), items)} items: "
                         f"over the limit of {ITEM_LIMIT}")
    input_nodes = torch.empty(max(items, 1), dtype=torch.int64, device=g.device)
    pos = torch.empty((n * W, L1), dtype=torch.int32, device=g.device)
    neg = torch.empty((n * W * K, L1), dtype=torch.int32, device=g.device)
    tr = torch.empty((n, W, L1), dtype=torch.int64, device=g.device) if traces else None
    out = _capi.WalkBatchOut(input_nodes.data_ptr(), pos.data_ptr(), neg.data_ptr() if neg.numel() else None, tr.data_ptr() if traces and n else None)
    ticket = _batch_begin(_lib.coala_sampler_walk_batch, g, nodes.data_ptr(), n, W, walk_length, *thr, K, _u64(seed), _u64(step), C.byref(out))
    return (g, nodes, input_nodes, pos, neg, tr, ticket)


def walk_batch_end(pending):
    """Wait for the event behind a walk_batch_begin call (only for its kernels) -> WalkBatch.  Start nodes outside [0, num_nodes) are
    counted in its n_bad, as node2vec_random_walk gives them a row of -1."""
    g, nodes, input_nodes, pos, neg, tr, ticket = pending
    n_nodes, n_bad = _batch_collect(_lib.coala_sampler_walk_batch_wait, g, ticket)
    return WalkBatch(nodes, input_nodes[:n_nodes], pos, neg, tr, n_bad)


def walk_batch(g, nodes, p=1.0, q=1.0, walk_length=20, num_walks=1, num_neg=1, seed=0, step=0, traces=False):
    """walk_batch_end(walk_batch_begin(...)): the skip-gram batch of node2vec walks from `nodes` (PyG's Node2Vec.sample)."""
    return walk_batch_end(walk_batch_begin(g, nodes, p, q, walk_length, num_walks, num_neg, seed, step, traces))


def pair_code_bits(num_nodes, n_slots):
    """node_bits of the (node, time slot) pair code slot << node_bits | node: the bit length of num_nodes, so that the value
    num_nodes itself fits the node field and names no node.  ValueError when the code would not fit 62 bits."""
    node_bits = int(num_nodes).bit_length()
    slot_bits = max(int(n_slots) - 1, 0).bit_length()
    if node_bits + slot_bits > 62:
        raise ValueError(f"{n_slots} distinct query times on a graph of {num_nodes} nodes: a (node, time) pair takes {node_bits} + {slot_bits} "
                         f"bits, over the 62 of a code; sample fewer distinct times per call")
    return node_bits


class TemporalNeighborSampler(NeighborSampler):
    """Temporal neighbour sampling (PyG's NeighborLoader(time_attr=, temporal_strategy=), GraphBolt's temporal_sample_neighbors, TGN's
    most recent neighbours), in place of NeighborSampler: same loader.  graph.edata[time] holds an int64 timestamp per edge in CSC
    order, non-decreasing inside every row (sort_csc_by_time; checked once per graph).  Every seed node comes with a query time t, and
    every layer samples only among the in-edges with timestamp < t (inclusive=True: <= t, PyG's rule); a neighbour inherits the query
    time of the row that reached it.  strategy 'uniform' draws `fanout` of the eligible edges without replacement (all when there are
    no more), 'last' takes the `fanout` most recent.  The rule is in the header of coala_sampler.hip.

    sample(g, seed_nodes, step=None, seed_times=None): the times are seed_times (int64, one per seed), else
    g.ndata[seed_time][seed_nodes] when the sampler was given seed_time= (what lets the unchanged loader drive it), else ValueError.
    The (seed node, time) pairs of a call must be distinct.  A node reached at two different times is two items: Block.src_nodes holds
    node ids and may repeat one; Block.src_times / Block.dst_times (int64) hold the query time of every source / destination item.
    Every block is fixed-stride.  With edge_ids (the default) block.edata carries '_ID', graph.edata through it (so edata[time]), and
    'dt' (int64, shaped like nbr): the row's query time minus the edge's timestamp, 0 on padding -- what time-decay weights and time
    encodings are made from.  Not provided (ValueError): fan-out -1, prob=, bucket_by_owner > 0 (the owner of a pair is not the owner of
    its node), floating-point timestamps, node timestamps."""

    STRATEGIES = ("uniform", "last")

    def __init__(self, fanouts, time="ts", strategy="uniform", inclusive=False, seed_time=None, seed=0, edge_ids=True, prob=None,
                 bucket_by_owner=0, node_time=None):
        fanouts = [int(f) for f in fanouts]
        if any(f == -1 for f in fanouts):
            raise ValueError("TemporalNeighborSampler: fan-out -1 (every eligible in-edge) is not supported; each fan-out must be 1..32")
        if prob is not None:
            raise ValueError("TemporalNeighborSampler: prob= (weighted temporal draws) is not supported")
        if bucket_by_owner:
            raise ValueError("TemporalNeighborSampler: bucket_by_owner is not supported: the owner of a (node, time) pair is not the owner of its node")
        if node_time is not None:
            raise ValueError("TemporalNeighborSampler: node timestamps are not supported, only edge timestamps (time=)")
        if strategy not in self.STRATEGIES:
            raise ValueError(f"strategy {strategy!r}: 'uniform' or 'last'")
        super().__init__(fanouts, seed=seed, edge_ids=edge_ids)
        self.time, self.strategy, self.inclusive, self.seed_time = time, strategy, bool(inclusive), seed_time

    def _seed_times(self, g, seeds, seed_times):
        if seed_times is None:
            if self.seed_time is None:
                raise ValueError("TemporalNeighborSampler: no query times: pass seed_times=, or build the sampler with seed_time= "
                                 "(a key of graph.ndata)")
            if self.seed_time not in g.ndata:
                raise KeyError(f"ndata has no {self.seed_time!r}: the query times of TemporalNeighborSampler(seed_time={self.seed_time!r})")
            col = g.ndata[self.seed_time]
            seed_times = col[seeds.to(col.device)]
        if not _is_int_tensor(seed_times):
            raise ValueError("seed times must be an integer tensor (floating-point timestamps are not supported)")
        if seed_times.dim() != 1 or seed_times.numel() != seeds.numel():
            raise ValueError(f"seed times of shape {tuple(seed_times.shape)}: one per seed node, ({seeds.numel()},)")
        return seed_times.to(g.device, dtype=torch.int64)

    def sample(self, g, seed_nodes, step=None, seed_times=None):
        """-> (input_nodes, output_nodes, blocks), blocks[0] the input layer; input_nodes is blocks[0].src_nodes, repeated ids included."""
        return self.sample_end(self.sample_begin(g, seed_nodes, step, seed_times))

    def sample_begin(self, g, seed_nodes, step=None, seed_times=None):
        """NeighborSampler.sample_begin over the codes of the (seed node, query time) pairs.  The table of distinct times and the codes
        are made on the device; the one host read is the number of distinct times."""
        g = _as_graph(g)
        ts = g.edge_times(self.time)   # raises before any launch
        if seed_nodes.dim() != 1:
            raise ValueError(f"seed nodes of shape {tuple(seed_nodes.shape)}: a 1-D tensor of node ids")
        seeds = seed_nodes.to(g.device, dtype=torch.int64).contiguous()
        times = self._seed_times(g, seeds, seed_times)
        slot_time, slot = torch.unique(times, sorted=True, return_inverse=True)
        bits = pair_code_bits(g.num_nodes, slot_time.numel())
        # a seed id outside the graph takes the node field num_nodes, which names no node: an empty row
        codes = (slot << bits) | torch.where((seeds >= 0) & (seeds < g.num_nodes), seeds, g.num_nodes)
        return self._begin(g, codes, step, extra=(seeds, slot_time.contiguous(), bits, ts))

    _takes_bucketing = False

    def _entry(self, p, fan, eid_p):
        _, slot_time, _, ts = p.extra
        return (_lib.coala_sampler_sample_layers_temporal, (fan, len(p.rev)),
                (ts.data_ptr(), slot_time.data_ptr(), slot_time.numel(), self.STRATEGIES.index(self.strategy), int(self.inclusive), eid_p))

    def sample_end(self, pending):
        """Wait for the counts, decode every layer's source codes into node ids and query times, and build the blocks."""
        p = pending
        g, n = p.graph, p.n
        seeds, slot_time, bits, ts = p.extra
        n_src, _, _ = self._wait(p)
        cur = torch.cuda.current_stream(g.device)
        mask = (1 << bits) - 1
        blocks = []
        n_dst, dst_times = n, slot_time[p.seeds >> bits] if n else p.seeds
        for l, f in enumerate(p.rev):
            ns = n_src[l]
            code_l = p.src[l][:ns]
            code_l.record_stream(cur)   # allocated on the stream of sample_begin, decoded on this one
            src_nodes, src_times = code_l & mask, slot_time[code_l >> bits] if ns else code_l
            src_nodes[:n] = seeds       # the seeds as they were given: an id outside the graph was coded as num_nodes
            eid_l = p.eid[l][: n_dst * f].view(n_dst, f) if p.eid is not None else None
            lazy = None
            if eid_l is not None:
                def dt(eid_l=eid_l, t_row=dst_times):
                    return torch.where(eid_l >= 0, t_row.unsqueeze(1) - ts[eid_l.clamp_min(0)], 0)
                lazy = {"dt": dt}
            # the output layer's destination items are the seeds (src_nodes[:n]): Block gathers graph.ndata for them
            b = Block(src_nodes, p.nbr[l][: n_dst * f].view(n_dst, f), n_dst, graph=g if l == 0 else None, edata_graph=g, eid=eid_l, edata_lazy=lazy)
            b.src_times, b.dst_times = src_times, dst_times
            b.srcdata["_TIME"], b.dstdata["_TIME"] = src_times, dst_times   # Block.tensors() reports what srcdata / dstdata hold
            blocks.insert(0, b)
            n_dst, dst_times = ns, src_times
        return blocks[0].src_nodes, seeds, blocks


MAX_NEGATIVES = 64   # negative pairs per seed edge (coala_sampler.hip: kMaxNeg)


class UniformNegativeSampler(object):
    """DGL's dgl.dataloading.negative_sampler.Uniform(k): every seed edge (u, v) gets k pairs (u, v'), v' uniform over the nodes of the
    graph; a pair that happens to be an edge, or v' == u, is kept.  Here the draws are a function of (seed, step, edge id, j): the rule
    is in the header of coala_sampler.hip."""

    def __init__(self, k):
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= MAX_NEGATIVES:
            raise ValueError(f"k {k!r}: 0..{MAX_NEGATIVES} negative pairs per edge")
        self.k = k


class EdgeBatch(object):
    """The pairs of one link-prediction minibatch.  eids: the seed edges (CSC positions); seed_nodes: int64 [n_nodes], the distinct
    endpoints of the positive and negative pairs in order of first appearance -- the destination nodes of blocks[-1], so the rows of
    the model's output; pos_src, pos_dst int32 [n] and neg_src, neg_dst int32 [n * k] index it.  The source of negative j of edge i
    (entry i * k + j) is pos_src[i]: neg_src is made on first access.  seed_times (TemporalEdgePredictionSampler; None otherwise): int64
    [n_nodes], the query time of every entry of seed_nodes -- the seeds are then distinct (node, time) pairs, and a node may repeat."""

    def __init__(self, eids, seed_nodes, pos_src, pos_dst, neg_dst, k, seed_times=None):
        self.eids, self.seed_nodes, self.pos_src, self.pos_dst, self.neg_dst, self.k = eids, seed_nodes, pos_src, pos_dst, neg_dst, k
        self.seed_times = seed_times
        self._neg_src = None

    @property
    def neg_src(self):
        if self._neg_src is None:
            self._neg_src = self.pos_src.repeat_interleave(self.k) if self.k else self.pos_src[:0]
        return self._neg_src

    def tensors(self):
        """Every device tensor the batch holds (the loader's lifetime bookkeeping, as Block.tensors())."""
        return [t for t in (self.eids, self.seed_nodes, self.pos_src, self.pos_dst, self.neg_dst, self._neg_src, self.seed_times) if t is not None]


def edge_batch(g, eids, num_neg, seed=0, step=0):
    """Enqueue the edge-batch kernels for the seed edges `eids` (CSC positions) on the current stream, without waiting: -> the pending
    call edge_batch_wait takes.  ValueError before any launch when n * (2 + num_neg) is over ITEM_LIMIT."""
    if isinstance(num_neg, bool) or not isinstance(num_neg, int) or not 0 <= num_neg <= MAX_NEGATIVES:
        raise ValueError(f"num_neg {num_neg!r}: 0..{MAX_NEGATIVES} negative pairs per edge")
    eids = eids.to(g.device, dtype=torch.int64).contiguous()
    n = eids.numel()
    if eids.dim() != 1:
        raise ValueError(f"seed edges of shape {tuple(eids.shape)}: a 1-D tensor of edge ids")
    if n * (2 + num_neg) > ITEM_LIMIT:
        raise ValueError(f"{n} seed edges with {num_neg} negatives each hold {n * (2 + num_neg)} items: over the limit of {ITEM_LIMIT}")
    nodes = torch.empty(max(n * (2 + num_neg), 1), dtype=torch.int64, device=g.device)
    pos = torch.empty((2, max(n, 1)), dtype=torch.int32, device=g.device)
    neg = torch.empty(max(n * num_neg, 1), dtype=torch.int32, device=g.device)
    out = _capi.EdgeBatchOut(nodes.data_ptr(), pos[0].data_ptr(), pos[1].data_ptr(), neg.data_ptr())
    ticket = _batch_begin(_lib.coala_sampler_edge_batch, g, eids.data_ptr(), n, num_neg, _u64(seed), _u64(step), C.byref(out))
    return (g, eids, n, num_neg, nodes, pos, neg, ticket)


def edge_batch_wait(pending):
    """Wait for the event behind an edge_batch call (only for its kernels) -> EdgeBatch.  IndexError when a seed edge was outside
    [0, num_edges); the graph handle stays usable."""
    g, eids, n, num_neg, nodes, pos, neg, ticket = pending
    n_nodes, n_bad = _batch_collect(_lib.coala_sampler_edge_batch_wait, g, ticket)
    if n_bad > 0:
        raise IndexError(f"{n_bad} of the {n} seed edges are outside [0, {g.num_edges})")
    return EdgeBatch(eids, nodes[:n_nodes], pos[0][:n], pos[1][:n], neg[: n * num_neg], num_neg)


def reverse_edge_ids(indptr, indices):
    """For a symmetric simple graph in CSC form: int64 [E], the position of every edge's reverse -- edge e = (u -> v) maps to the
    position of (v -> u); a self-loop maps to itself.  What EdgePredictionSampler(exclude='reverse_id') takes as reverse_eids.  Plain
    torch on the tensors' device.  ValueError when a row holds a neighbour twice, or an edge has no reverse."""
    N, E = indptr.numel() - 1, indices.numel()
    deg = indptr[1:] - indptr[:-1]
    dst = torch.repeat_interleave(torch.arange(N, device=indptr.device), deg, output_size=E)
    src = indices.to(torch.int64)
    key, order = torch.sort(dst * N + src, stable=True)        # sorted (dst, src) keys, and the edge each one belongs to
    if E > 1 and bool((key[1:] == key[:-1]).any()):
        raise ValueError("reverse_edge_ids: a row holds the same neighbour twice; the graph must be simple")
    want = src * N + dst                                         # the key of every edge's reverse
    at = torch.searchsorted(key, want).clamp_max(max(E - 1, 0))
    if E and bool((key[at] != want).any()):
        raise ValueError("reverse_edge_ids: an edge has no reverse; the graph must be symmetric")
    return order[at] if E else torch.zeros(0, dtype=torch.int64, device=indptr.device)


class _EdgePrediction(object):
    """What the two edge-prediction wrappers share: the negative sampler, the attributes the loader reads, make_graph, sample, and the
    edge batch of the seed edges.  A wrapper checks its inner sampler, then adds sample_begin / sample_end."""

    def __init__(self, sampler, negative_sampler, bucket_by_owner):
        if negative_sampler is not None and not isinstance(negative_sampler, UniformNegativeSampler):
            raise ValueError("negative_sampler: a UniformNegativeSampler, or None")
        self.sampler = sampler
        self.num_neg = negative_sampler.k if negative_sampler is not None else 0
        # what the loader takes as fan_out: it sizes its fetch buffers as batch * prod(f + 1), and a batch of seed edges has up to
        # batch * (2 + k) seed nodes -- one more entry, 1 + k, makes that product the bound of the input nodes
        self.fanouts = list(sampler.fanouts) + [1 + self.num_neg]
        self.bucket_by_owner = bucket_by_owner
        self.stream_safe = sampler.stream_safe
        self.completes_on_host = sampler.completes_on_host

    make_graph = staticmethod(NeighborSampler.make_graph)

    def sample(self, g, eids, step=None):
        """-> (input_nodes, EdgeBatch, blocks), blocks[0] the input layer; blocks[-1]'s destination nodes (items) are the batch's seeds."""
        return self.sample_end(self.sample_begin(g, eids, step))

    def _edge_batch(self, g, eids, step):
        """The edge batch of the seed edges at the inner sampler's seed and step, waited for: the one host wait of a wrapper."""
        return edge_batch_wait(edge_batch(g, eids, self.num_neg, self.sampler.seed, self.sampler.step if step is None else int(step)))


class EdgePredictionSampler(_EdgePrediction):
    """Link-prediction minibatches, DGL's dgl.dataloading.as_edge_prediction_sampler: wraps a NeighborSampler, LaborSampler or
    RelNeighborSampler.  sample / sample_begin / sample_end take seed EDGE ids (CSC positions) and return (input_nodes, EdgeBatch,
    blocks): the endpoints of the seed edges and of k negative pairs per edge (negative_sampler, a UniformNegativeSampler) are made
    the seed nodes of the inner sampler, and with exclude= the seed edges are taken out of every block so that the model cannot read
    the answer: 'self' the batch's edges, 'reverse_id' those and reverse_eids[eids] (reverse_edge_ids gives that map for a symmetric
    graph).  exclude needs edge ids on the blocks: it turns edge_ids on in the inner sampler.  The 3-tuple keeps batch[0] and batch[2]
    where the loader and the manager read them: give the wrapper to COALA_GNN_DataLoader with a plain distributor over edge ids,
    and self.fanouts (the inner fan-outs and one more entry, 1 + k) as its fan_out."""

    def __init__(self, sampler, exclude=None, reverse_eids=None, negative_sampler=None):
        if isinstance(sampler, TemporalNeighborSampler):
            raise ValueError("EdgePredictionSampler: a TemporalNeighborSampler takes (node, time) seeds; wrap it in TemporalEdgePredictionSampler")
        if not isinstance(sampler, NeighborSampler) or isinstance(sampler, RandomWalkNeighborSampler) and exclude is not None:
            raise ValueError("EdgePredictionSampler wraps a NeighborSampler, LaborSampler or RelNeighborSampler; RandomWalkNeighborSampler has no "
                             "edge ids to exclude by")
        if exclude not in (None, "self", "reverse_id"):
            raise ValueError(f"exclude {exclude!r}: None, 'self' or 'reverse_id'")
        if exclude == "reverse_id" and reverse_eids is None:
            raise ValueError("exclude='reverse_id' needs reverse_eids (reverse_edge_ids(indptr, indices))")
        super().__init__(sampler, negative_sampler, sampler.bucket_by_owner)
        self.exclude, self.reverse_eids = exclude, reverse_eids
        if exclude is not None:
            sampler.edge_ids = True

    def sample_begin(self, g, eids, step=None):
        """Enqueue the edge batch, wait for its two counts (the one host wait of the wrapper), then enqueue the inner sample over the
        batch's seed nodes.  -> the inner sampler's pending record, its `batch` the EdgeBatch."""
        g = _as_graph(g)
        batch = self._edge_batch(g, eids, step)
        pending = self.sampler.sample_begin(g, batch.seed_nodes, step)
        pending.batch = batch
        return pending

    def sample_end(self, pending):
        batch = pending.batch
        input_nodes, _, blocks = self.sampler.sample_end(pending)
        if self.exclude is not None:
            ex = batch.eids
            if self.exclude == "reverse_id":
                ex = torch.cat([ex, self.reverse_eids.to(ex.device)[ex]])
            ex = torch.sort(ex).values
            blocks = [b.exclude_edges(ex) for b in blocks]
        return input_nodes, batch, blocks


class TemporalEdgePredictionSampler(_EdgePrediction):
    """Link-prediction minibatches on a graph with time (PyG's LinkNeighborLoader(edge_label_time=)): wraps a TemporalNeighborSampler,
    same sample / sample_begin / sample_end / fanouts as EdgePredictionSampler.  Seed edge e is queried at t_e = its own timestamp: its
    two endpoints and the destinations of its k uniform negatives (the edge_batch kernels, unchanged) become the pairs (node, t_e).
    The distinct pairs -- ascending by time and then by node id -- are the inner sampler's seeds: batch.seed_nodes / batch.seed_times,
    indexed by batch.pos_src / pos_dst / neg_dst.  No exclusion pass runs: with strict times (inclusive=False, required) the seed edge
    and every edge not older than it are outside every block by construction."""

    def __init__(self, sampler, negative_sampler=None):
        if not isinstance(sampler, TemporalNeighborSampler):
            raise ValueError("TemporalEdgePredictionSampler wraps a TemporalNeighborSampler")
        if sampler.inclusive:
            raise ValueError("TemporalEdgePredictionSampler needs inclusive=False: with ts <= t the seed edge itself would be eligible")
        super().__init__(sampler, negative_sampler, 0)

    def sample_begin(self, g, eids, step=None):
        """Enqueue the edge batch and wait for its counts, make the distinct (node, t_e) pairs in plain torch, then enqueue the inner
        sample over them.  -> the inner sampler's pending record, its `batch` the EdgeBatch."""
        g = _as_graph(g)
        ts = g.edge_times(self.sampler.time)   # raises before any launch
        raw = self._edge_batch(g, eids, step)
        n, k = raw.eids.numel(), self.num_neg
        t_e = ts[raw.eids]
        at = torch.cat([raw.pos_src, raw.pos_dst, raw.neg_dst]).to(torch.int64)          # the items [src.. | dst.. | negatives..]
        slot_time, slot = torch.unique(torch.cat([t_e, t_e, t_e.repeat_interleave(k)]), sorted=True, return_inverse=True)
        bits = pair_code_bits(g.num_nodes, slot_time.numel())
        pairs, where = torch.unique((slot << bits) | raw.seed_nodes[at], sorted=True, return_inverse=True)
        where = where.to(torch.int32)
        nodes, times = pairs & ((1 << bits) - 1), slot_time[pairs >> bits] if n else pairs
        batch = EdgeBatch(raw.eids, nodes, where[:n], where[n: 2 * n], where[2 * n:], k, seed_times=times)
        pending = self.sampler.sample_begin(g, nodes, step, seed_times=times)
        pending.batch = batch
        return pending

    def sample_end(self, pending):
        input_nodes, _, blocks = self.sampler.sample_end(pending)
        return input_nodes, pending.batch, blocks


def as_edge_prediction_sampler(sampler, exclude=None, reverse_eids=None, reverse_etypes=None, negative_sampler=None, prefetch_labels=None):
    """DGL's dgl.dataloading.as_edge_prediction_sampler, same signature -> EdgePredictionSampler.  reverse_etypes (heterographs) and
    prefetch_labels are not supported."""
    if reverse_etypes is not None or prefetch_labels is not None:
        raise ValueError("as_edge_prediction_sampler: reverse_etypes and prefetch_labels are not supported")
    return EdgePredictionSampler(sampler, exclude=exclude, reverse_eids=reverse_eids, negative_sampler=negative_sampler)
