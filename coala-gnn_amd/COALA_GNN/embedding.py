"""Trainable node embeddings in the table the feature cache fronts, with sparse optimizers that touch only a minibatch's rows.

NodeEmbedding stands where DGL's dgl.nn.NodeEmbedding stands, SparseAdagrad / SparseAdam / SparseSGD where dgl.optim's do, RowWiseAdagrad
where DGL-KE's row-wise Adagrad does: node types without input features get a learned row per node, too many to keep as a dense parameter
in HBM.  The 'native' backend keeps the table in pinned host memory behind an Isolated_Cache: a lookup is the cache's read_feature, an
optimizer step is ONE native call (coala_cache_adagrad_rows / _adam_rows / _rowwise_adagrad_rows, or coala_cache_write_rows in 'add' mode
for SGD) that updates the cold row and every cache line of each id
(write-through: include/coala_hip.h).  The 'torch' backend keeps a plain tensor on any device and does the same with torch ops: the
fallback for a machine without the GPU, and the reference the tests compare against.

The trace / step protocol and the 'mean' rule of the optimizers follow DGL's, written from memory of DGL's source, not copied from it."""
import math

import torch

__all__ = ["NodeEmbedding", "SparseAdagrad", "SparseAdam", "RowWiseAdagrad", "SparseSGD"]


def _as_ids(ids, device):
    ids = torch.as_tensor(ids)
    if ids.dtype != torch.int64:
        ids = ids.to(torch.int64)
    return ids.to(device).contiguous().view(-1)


class NodeEmbedding(object):
    """NodeEmbedding(num_rows, dim, cache_mb, device, init_func=None, backend='native' | 'torch')

    emb(ids) looks the rows up (through the cache with the native backend) and returns a LEAF tensor that requires grad; the pair
    (ids, tensor) is recorded in emb.trace, and the sparse optimizer's step() reads the gradients from there, as in DGL.
    emb.read(ids) / emb.write(ids, rows) are the untracked forms.  init_func(tensor) fills the [num_rows, dim] host table in place (or
    returns the values to copy in); default: uniform in (-1, 1).

    Native calls are enqueued on torch's current stream and do not wait: emb.weight_host, the host view of the table, is up to date
    only after that stream has been synchronised."""

    def __init__(self, num_rows, dim, cache_mb=64, device="cuda", init_func=None, backend="native"):
        if backend not in ("native", "torch"):
            raise ValueError("backend must be 'native' or 'torch'")
        if int(num_rows) < 1 or int(dim) < 1:
            raise ValueError("num_rows and dim must be positive")
        self.num_rows, self.dim, self.backend = int(num_rows), int(dim), backend
        self.device = torch.device(device)
        self.trace = []
        self._table = self._cache = self._manager = None
        if backend == "native":
            if self.device.type != "cuda":
                raise ValueError("the native backend runs on the GPU: pass a cuda device, or backend='torch'")
            import COALA_GNN_Pybind as P
            from .synthetic import PinnedFeatureTable
            index = torch.cuda.current_device() if self.device.index is None else self.device.index
            self.device = torch.device("cuda", index)
            self._table = PinnedFeatureTable(self.num_rows, self.dim, index)
            self.weight_host = self._table.cpu_tensor
            self._init(self.weight_host, init_func)
            ctrl = P.SSD_GNN_SSD_Controllers(1, self.dim * 4, 1024, 0, index, self.dim, True)
            self._cache = P.Isolated_Cache(ctrl, None, 0, 1, int(cache_mb), self._table.device_ptr, num_rows=self.num_rows, sync=False)
        else:
            self.weight = torch.empty((self.num_rows, self.dim), dtype=torch.float32, device=self.device)
            self._init(self.weight, init_func)
            self.weight_host = self.weight if self.device.type == "cpu" else None

    @staticmethod
    def _init(t, init_func):
        if init_func is None:
            t.uniform_(-1.0, 1.0)
            return
        r = init_func(t)
        if r is not None and r is not t:
            t.copy_(r)

    @classmethod
    def from_manager(cls, manager, num_rows=None):
        """The table and the cache a COALA_GNN_Manager (a COALA_GNN_DataLoader's .COALA_GNN_Manager) already has, as an embedding: the
        loader's pipelined fetch IS the lookup -- hand its rows to attach() -- and the sparse optimizer writes through the same cache.
        For an isolated manager of one GPU over a writable table; ValueError otherwise (a second cache over the table would keep stale
        lines).  num_rows: rows of the table when the manager's sim_buf does not tell (.rows or .shape[0]).

        Staleness: the loader enqueues the fetch of the NEXT minibatch before this step's update is enqueued, so rows of a batch may have
        been read before the previous step's update reached them.  The gap is bounded by the loader's look-ahead (one fetch with
        prefetch=0), as with DGL's prefetching; the update itself always starts from the table's current value, never from the stale
        copy.  It is not closed here.  A loader with prefetch > 0 drives the cache from a second host thread, which a handle that is also
        written to does not allow: use prefetch=0."""
        import COALA_GNN_Pybind as P
        cache = getattr(manager, "COALA_GNN_Cache", None)
        comm = getattr(manager, "MPI_comm_manager", None)
        if getattr(manager, "cache_backend", None) != "isolated" or not isinstance(cache, P.Isolated_Cache):
            raise ValueError("NodeEmbedding.from_manager needs an isolated cache (cache_backend='isolated')")
        if getattr(cache, "num_gpus", 1) != 1 or getattr(comm, "local_size", 1) != 1:
            raise ValueError("NodeEmbedding.from_manager needs a manager of one GPU: caches of several GPUs over one table would keep stale lines")
        buf = manager.sim_buf
        if num_rows is None:
            num_rows = getattr(buf, "rows", None)
        if num_rows is None and hasattr(buf, "shape"):
            num_rows = int(buf.shape[0])
        if num_rows is None:
            raise ValueError("NodeEmbedding.from_manager: pass num_rows=, the manager's table does not tell")
        self = cls.__new__(cls)
        self.num_rows, self.dim, self.backend = int(num_rows), int(manager.dim), "native"
        self.device = torch.device(manager.device)
        self.trace = []
        self._table, self._cache, self._manager = None, cache, manager
        host = getattr(buf, "cpu_tensor", None)
        if host is None and isinstance(buf, torch.Tensor) and buf.device.type == "cpu":
            host = buf
        self.weight_host = host
        return self

    # ---------------------------------------------------------------------------------------------------- lookups
    def read(self, ids):
        """fp32 [len(ids), dim] rows, untracked."""
        ids = _as_ids(ids, self.device)
        if self.backend == "torch":
            return self.weight[ids]
        out = torch.empty((ids.numel(), self.dim), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._cache.read_feature(out.data_ptr(), ids.data_ptr(), ids.numel())
        return out

    def __call__(self, ids):
        ids = _as_ids(ids, self.device)
        return self.attach(ids, self.read(ids))

    def attach(self, input_nodes, rows):
        """Mark rows that were fetched elsewhere (the loader's fetch of input_nodes) as this step's embedding output: returns them as a
        leaf that requires grad (same storage) and records (input_nodes, leaf) in the trace."""
        ids = _as_ids(input_nodes, self.device)
        if rows.dim() != 2 or rows.shape[0] != ids.numel() or rows.shape[1] != self.dim:
            raise ValueError(f"attach: rows of shape {tuple(rows.shape)} for {ids.numel()} ids of dim {self.dim}")
        leaf = rows.detach().requires_grad_(True)
        self.trace.append((ids, leaf))
        return leaf

    def reset_trace(self):
        self.trace = []

    # ---------------------------------------------------------------------------------------------------- updates
    def write(self, ids, rows):
        """row(ids[i]) = rows[i], untracked.  Repeated ids are deduplicated first and the LAST occurrence wins (the native call wants
        pairwise distinct ids)."""
        ids = _as_ids(ids, self.device)
        rows = torch.as_tensor(rows, dtype=torch.float32).to(self.device)
        if rows.dim() != 2 or rows.shape[0] != ids.numel() or rows.shape[1] != self.dim:
            raise ValueError(f"write: rows of shape {tuple(rows.shape)} for {ids.numel()} ids of dim {self.dim}")
        uniq, inv = torch.unique(ids, return_inverse=True)
        last = torch.zeros(uniq.numel(), dtype=torch.int64, device=self.device)
        last.scatter_reduce_(0, inv, torch.arange(ids.numel(), device=self.device), "amax", include_self=False)
        self._assign(uniq, rows[last].contiguous())

    def _assign(self, uniq, rows):
        if self.backend == "torch":
            self.weight[uniq] = rows
        elif uniq.numel():
            with torch.cuda.device(self.device):
                self._cache.write_rows(uniq.data_ptr(), uniq.numel(), rows.data_ptr(), "assign")

    def _add(self, uniq, rows, alpha):
        """row(uniq[i]) += alpha * rows[i]; uniq pairwise distinct."""
        if self.backend == "torch":
            self.weight[uniq] = torch.addcmul(self.weight[uniq], rows, torch.tensor(float(alpha), dtype=torch.float32, device=self.device))
        elif uniq.numel():
            with torch.cuda.device(self.device):
                self._cache.write_rows(uniq.data_ptr(), uniq.numel(), rows.data_ptr(), "add", float(alpha))

    def _adagrad(self, uniq, grad, state, lr, eps):
        """One Adagrad step on pairwise distinct rows; state: a [num_rows, dim] tensor (torch backend) or a device-visible pointer."""
        if self.backend == "torch":
            s = state[uniq] + grad * grad
            state[uniq] = s
            self.weight[uniq] = self.weight[uniq] - (lr * grad) / (s.sqrt() + eps)
        elif uniq.numel():
            with torch.cuda.device(self.device):
                self._cache.adagrad_rows(uniq.data_ptr(), uniq.numel(), grad.data_ptr(), int(state), float(lr), float(eps))

    def _adam(self, uniq, grad, m, v, row_step, step, lr, betas, eps):
        """One Adam step on pairwise distinct rows.  m, v: [num_rows, dim] tensors (torch backend) or device-visible pointers; row_step:
        the int32 [num_rows] counter tensor (t = ++row_step[id] per row) or None (t = step for every row)."""
        b1, b2 = betas
        if self.backend == "torch":
            f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))     # noqa: E731  (the scalars as the native call receives them)
            b1, b2, lr, eps = f32(b1), f32(b2), f32(lr), f32(eps)
            if row_step is not None:
                t = torch.clamp(row_step[uniq].to(torch.int64) + 1, max=2 ** 31 - 1)
                row_step[uniq] = t.to(torch.int32)
                t = t.to(torch.float64)
            else:
                t = torch.full((uniq.numel(),), float(step), dtype=torch.float64, device=self.device)
            # 1 - beta^t as -expm1(t ln beta), in float64, once per row (beta = 0: ln = -inf, no correction)
            bc1 = -torch.expm1(t * (math.log(b1) if b1 > 0 else -math.inf))
            bc2 = -torch.expm1(t * (math.log(b2) if b2 > 0 else -math.inf))
            step_size = (lr / bc1).to(torch.float32)[:, None]
            rsbc2 = bc2.rsqrt().to(torch.float32)[:, None]
            # exp_avg is signed: its two terms can cancel, so they are added in float64 and rounded once (the kernel carries the
            # product's rounding error to the same end)
            mn = (b1 * m[uniq].to(torch.float64) + (1.0 - b1) * grad.to(torch.float64)).to(torch.float32)
            vn = torch.addcmul(torch.tensor(1.0 - b2, dtype=torch.float32, device=self.device) * (grad * grad), v[uniq],
                               torch.tensor(b2, dtype=torch.float32, device=self.device))
            m[uniq] = mn
            v[uniq] = vn
            self.weight[uniq] = self.weight[uniq] - (step_size * mn) / (vn.sqrt() * rsbc2 + eps)
        elif uniq.numel():
            with torch.cuda.device(self.device):
                self._cache.adam_rows(uniq.data_ptr(), uniq.numel(), grad.data_ptr(), int(m), int(v), float(lr), (float(b1), float(b2)), float(eps),
                                      row_step_ptr=0 if row_step is None else row_step.data_ptr(), step=int(step))

    def _rowwise_adagrad(self, uniq, grad, row_state, lr, eps):
        """One row-wise Adagrad step on pairwise distinct rows; row_state: the fp32 [num_rows] tensor (both backends)."""
        if self.backend == "torch":
            # the row mean in fp32, summed pairwise (ceil(log2 dim) additions on any path), so that its rounding does not depend on the device
            sq = grad * grad
            width = 1 << max(self.dim - 1, 0).bit_length()
            sq = torch.nn.functional.pad(sq, (0, width - self.dim))
            while width > 1:
                width //= 2
                sq = sq[:, :width] + sq[:, width:]
            s = row_state[uniq] + sq[:, 0] / float(self.dim)
            row_state[uniq] = s
            self.weight[uniq] = self.weight[uniq] - (lr / (s.sqrt() + eps))[:, None] * grad
        elif uniq.numel():
            with torch.cuda.device(self.device):
                self._cache.rowwise_adagrad_rows(uniq.data_ptr(), uniq.numel(), grad.data_ptr(), row_state.data_ptr(), float(lr), float(eps))

    def close(self):
        if self._manager is None and self._cache is not None:
            self._cache.close()
        self._cache = None
        if self._table is not None:
            self.weight_host = None
            self._table.close()
            self._table = None


class _SparseOptimizer(object):
    def __init__(self, params, lr, reduce="mean"):
        params = [params] if isinstance(params, NodeEmbedding) else list(params)
        if not params or not all(isinstance(p, NodeEmbedding) for p in params):
            raise TypeError("a sparse optimizer takes NodeEmbedding objects")
        if reduce not in ("mean", "sum"):
            raise ValueError("reduce must be 'mean' or 'sum'")
        if not lr > 0:
            raise ValueError("lr must be positive")
        self.params, self.lr, self.reduce = params, float(lr), reduce

    def zero_grad(self):
        """Drop the recorded lookups (their gradients with them)."""
        for emb in self.params:
            emb.reset_trace()

    def _reduced(self, emb):
        """The trace as (distinct ids, one gradient row per id): rows of a repeated id are summed, and with reduce='mean' divided by
        how often the id was looked up -- DGL's rule; 'sum' is what nn.Embedding(sparse=True) hands torch.optim.Adagrad."""
        pairs = [(i, r.grad) for i, r in emb.trace if r.grad is not None]
        if not pairs:
            return None, None
        ids = torch.cat([i for i, _ in pairs])
        grads = torch.cat([g for _, g in pairs]).to(torch.float32)
        uniq, inv, cnt = torch.unique(ids, return_inverse=True, return_counts=True)
        g = torch.zeros((uniq.numel(), emb.dim), dtype=torch.float32, device=grads.device).index_add_(0, inv, grads)
        if self.reduce == "mean":
            g /= cnt.to(torch.float32)[:, None]
        return uniq, g

    @torch.no_grad()
    def step(self):
        """One update per embedding from its trace, then the trace is cleared."""
        for emb in self.params:
            uniq, g = self._reduced(emb)
            if uniq is not None:
                self._update(emb, uniq, g)
            emb.reset_trace()


class SparseSGD(_SparseOptimizer):
    """SparseSGD(params, lr, reduce='mean' | 'sum'): row -= lr * g on the rows a step looked up (one coala_cache_write_rows call in 'add'
    mode with the native backend)."""

    def _update(self, emb, uniq, g):
        emb._add(uniq, g, -self.lr)


class SparseAdagrad(_SparseOptimizer):
    """SparseAdagrad(params, lr, eps=1e-10, reduce='mean' | 'sum', state_device_bytes=1 GiB): element-wise Adagrad state, as
    torch.optim.Adagrad and DGL's SparseAdagrad keep it (not DGL-KE's one value per row).  One coala_cache_adagrad_rows call per step with
    the native backend.  The state of a native embedding is a zeroed HBM tensor when num_rows * dim * 4 bytes fit state_device_bytes,
    else pinned host memory the kernel reads and writes over the host link; it is never cached."""

    def __init__(self, params, lr, eps=1e-10, reduce="mean", state_device_bytes=1 << 30):
        super().__init__(params, lr, reduce)
        self.eps, self.state_device_bytes = float(eps), int(state_device_bytes)
        self._state = {}

    def state_of(self, emb):
        """(tensor [num_rows, dim] -- on the device, or the host view of a pinned state --, pointer for the native call)"""
        st = self._state.get(id(emb))
        if st is None:
            if emb.backend == "torch" or emb.num_rows * emb.dim * 4 <= self.state_device_bytes:
                t = torch.zeros((emb.num_rows, emb.dim), dtype=torch.float32, device=emb.device)
                st = (t, t.data_ptr(), None)
            else:
                from .synthetic import PinnedFeatureTable
                tab = PinnedFeatureTable(emb.num_rows, emb.dim, emb.device.index or 0)
                tab.cpu_tensor.zero_()
                st = (tab.cpu_tensor, tab.device_ptr, tab)
            self._state[id(emb)] = st
        return st[0], st[1]

    def _update(self, emb, uniq, g):
        t, ptr = self.state_of(emb)
        emb._adagrad(uniq, g, t if emb.backend == "torch" else ptr, self.lr, self.eps)


class SparseAdam(_SparseOptimizer):
    """SparseAdam(params, lr, betas=(0.9, 0.999), eps=1e-8, reduce='mean' | 'sum', step='row' | 'global', state_device_bytes=1 GiB)

    step='row' is DGL's SparseAdam: every row counts its own updates (int32, in HBM) and its bias corrections use that count -- lazy Adam.
    step='global' uses the optimizer's step count for every row it touches, torch.optim.SparseAdam's rule.  One coala_cache_adam_rows
    call per step with the native backend.  exp_avg, exp_avg_sq and the step vector of a native embedding are zeroed HBM tensors when
    num_rows * (2 * dim + 1) * 4 bytes fit state_device_bytes; otherwise exp_avg and exp_avg_sq live in pinned host memory, which the
    kernel reads and writes over the host link.  None of it is cached."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, reduce="mean", step="row", state_device_bytes=1 << 30):
        super().__init__(params, lr, reduce)
        try:
            b1, b2 = (float(b) for b in betas)
        except (TypeError, ValueError):
            raise ValueError("betas must be a pair of floats")
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError("betas must lie in [0, 1)")
        if step not in ("row", "global"):
            raise ValueError("step must be 'row' or 'global'")
        if not eps >= 0:
            raise ValueError("eps must not be negative")
        self.betas, self.eps, self.step_mode, self.state_device_bytes = (b1, b2), float(eps), step, int(state_device_bytes)
        self.steps = 0          # step() calls so far: t of step='global'
        self._state = {}

    def state_bytes(self, emb):
        """Bytes of exp_avg, exp_avg_sq and the step vector of emb."""
        return emb.num_rows * (2 * emb.dim + 1) * 4

    def state_of(self, emb):
        """(exp_avg, exp_avg_sq, row_step, pointer of exp_avg, pointer of exp_avg_sq): [num_rows, dim] fp32 tensors -- on the device, or
        the host views of pinned tables -- and the int32 [num_rows] step vector on the device."""
        st = self._state.get(id(emb))
        if st is None:
            steps = torch.zeros(emb.num_rows, dtype=torch.int32, device=emb.device)
            if emb.backend == "torch" or self.state_bytes(emb) <= self.state_device_bytes:
                m, v = (torch.zeros((emb.num_rows, emb.dim), dtype=torch.float32, device=emb.device) for _ in range(2))
                st = (m, v, steps, m.data_ptr(), v.data_ptr(), None)
            else:
                from .synthetic import PinnedFeatureTable
                tabs = [PinnedFeatureTable(emb.num_rows, emb.dim, emb.device.index or 0) for _ in range(2)]
                for tab in tabs:
                    tab.cpu_tensor.zero_()
                st = (tabs[0].cpu_tensor, tabs[1].cpu_tensor, steps, tabs[0].device_ptr, tabs[1].device_ptr, tabs)
            self._state[id(emb)] = st
        return st[:5]

    def step(self):
        self.steps += 1
        super().step()

    def _update(self, emb, uniq, g):
        m, v, steps, m_ptr, v_ptr = self.state_of(emb)
        native = emb.backend != "torch"
        emb._adam(uniq, g, m_ptr if native else m, v_ptr if native else v, steps if self.step_mode == "row" else None, self.steps, self.lr,
                  self.betas, self.eps)


class RowWiseAdagrad(_SparseOptimizer):
    """RowWiseAdagrad(params, lr, eps=1e-10, reduce='mean' | 'sum'): DGL-KE's Adagrad with ONE float of state per row, the mean of the
    row's squared gradients summed over the steps -- 4 bytes per row where SparseAdagrad keeps 4 * dim, so the state of a table far larger
    than HBM still lives in HBM (a zeroed fp32 [num_rows] tensor).  One coala_cache_rowwise_adagrad_rows call per step with the native
    backend."""

    def __init__(self, params, lr, eps=1e-10, reduce="mean"):
        super().__init__(params, lr, reduce)
        if not eps >= 0:
            raise ValueError("eps must not be negative")
        self.eps = float(eps)
        self._state = {}

    def state_of(self, emb):
        """(tensor [num_rows] on the embedding's device, its pointer)"""
        t = self._state.get(id(emb))
        if t is None:
            t = self._state[id(emb)] = torch.zeros(emb.num_rows, dtype=torch.float32, device=emb.device)
        return t, t.data_ptr()

    def _update(self, emb, uniq, g):
        emb._rowwise_adagrad(uniq, g, self.state_of(emb)[0], self.lr, self.eps)
