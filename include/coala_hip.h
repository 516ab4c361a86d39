/*
 * coala_hip.h -- C ABI of libcoala_hip.so: the MI355X (gfx950) feature-cache / minibatch-assembly path.
 *
 * This is the drop-in boundary for the hot path of jeongminpark417/COALA-GNN.  Every entry point names the
 * reference interface it replaces (paths relative to /root/reference).  Plain pointers and sizes only: no torch,
 * pybind or C++ types cross this boundary.  All functions return 0 on success or a negative COALA_E* code;
 * coala_last_error() returns a thread-local message for the last failure.  Nothing here ever calls exit().
 *
 * Streams: `stream` is a hipStream_t passed as void*.  Work is enqueued on it and the call returns without
 * synchronising, unless the handle was created with COALA_FLAG_SYNC (the reference's behaviour: every native call
 * ends in cudaDeviceSynchronize, COALA_GNN_Modules/ssd_gnn_cache.cuh:266) in which case the call returns after the
 * stream has drained.  A cache or sampler handle keeps its own work in program order across streams: a call on another
 * stream than the handle's previous call first waits there (hipStreamWaitEvent, no host wait) for that call's work.  One handle
 * is driven by one host thread at a time.
 */
#ifndef COALA_HIP_H
#define COALA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COALA_OK 0
#define COALA_EINVAL (-1)   /* bad argument                                    */
#define COALA_EHIP (-2)     /* a HIP runtime call failed                       */
#define COALA_ENOMEM (-3)   /* allocation failed                               */
#define COALA_EIO (-4)      /* file / shm failure                              */
#define COALA_EFORMAT (-5)  /* malformed .npy                                  */
#define COALA_ERANGE (-6)   /* an index was outside [0, num_rows)              */
#define COALA_ECOMM (-7)    /* an RCCL call failed                             */

#define COALA_WAYS 32u /* COALA_GNN_Modules/ssd_gnn_cache.cuh:61,204 */
#define COALA_COUNTS_RING 8 /* count exchanges issued ahead (coala_comm_counts_begin) whose tickets stay valid */

#define COALA_FLAG_SYNC 1u        /* synchronise the stream before returning (reference semantics)            */
#define COALA_FLAG_DISTRIBUTED 2u /* set = (id / n_gpus) % sets   (nvshmem_cache.h:191-196,347) instead of id % sets */
#define COALA_FLAG_PROFILE 4u     /* record hipEvents around the probe+gather kernel (see coala_cache_profile) */
#define COALA_FLAG_TAG64 16u      /* keep the reference's 64-bit tags (a set = 32 x 8 B = two 128-B lines, isolated_cache.h:552) even when
                                     num_rows < 2^32.  Default: 32-bit tags whenever every id fits -- a set is then ONE 128-B line, half
                                     the probe bytes; coala_cache_dump widens them, so the visible table state is the same.            */
#define COALA_FLAG_COLD_PARTITIONED 8u /* cold_table holds only this owner's rows: row k = node id k*n_gpus + rank, i.e. the
                                          cold row of id is id / n_gpus.  An owner of the partitioned cache never reads any
                                          other row, so each GPU pins 1/n_gpus of the table next to its own PCIe link instead
                                          of all GPUs mapping one shared copy (shared_UVA.cuh:42-100).                        */

const char* coala_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int coala_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Cache geometry: replaces SSD_GNN_SSD_Controllers (COALA_GNN_Modules/ssd_gnn_cache.cuh:10-55).
 * cache_dim = 128/256/512/1024 for dim <= 128/256/512/1024; COALA_EINVAL for dim > 1024 (reference throws).
 * ------------------------------------------------------------------------------------------------------------ */
int coala_cache_dim(int dim);
/* num_sets = (cache_mb * 2^20 / (cache_dim*4)) / 32   (ssd_gnn_cache.cuh:96-97,239-240) */
uint64_t coala_cache_num_sets(uint64_t cache_mb, int cache_dim);

typedef struct coala_cache coala_cache_t; /* opaque */

typedef struct coala_cache_config {
    int32_t device;            /* HIP device ordinal (SSD_GNN_SSD_Controllers.cudaDevice)                              */
    int32_t dim;               /* floats per row of the cold table and of every output row                            */
    uint64_t cache_mb;         /* cache capacity in MiB (Isolated_Cache ctor `cache_size`, ssd_gnn_cache.cuh:227)      */
    int32_t n_gpus;            /* GPUs sharing the owner-partitioned cache (1 = isolated)                             */
    int32_t rank;              /* this GPU's rank in [0, n_gpus)                                                      */
    int32_t global_rank;       /* only used in print_stats lines (isolated_cache.h:136-138)                           */
    uint32_t flags;            /* COALA_FLAG_*                                                                        */
    const float* cold_table;   /* device-visible pointer to fp32 [num_rows, dim]: pinned host (zero-copy) or HBM.      */
                               /* Replaces `sim_buf` (ssd_gnn_cache.cuh:227; isolated_cache.h:323-331).  Row stride is */
                               /* `dim` floats (the reference strides by cache_dim: SURVEY.md section 3.3, defect 2).  */
    uint64_t num_rows;         /* rows of cold_table; ids outside [0,num_rows) are rejected (COALA_ERANGE)            */
    const int64_t* node_color; /* HOST pointer to int64[num_rows] colours (Node_distributor_pybind::color_buffer_ptr,  */
                               /* node_distributor_pybind.cuh:226-229) or NULL: copied to the device at creation      */
    int32_t num_colors;        /* colours are 0..num_colors inclusive (0 = uncoloured); num_colors+1 counters are kept */
    int32_t reserved;
    uint64_t max_batch;        /* rows per call to pre-size scratch for (0 = grow on demand)                          */
} coala_cache_config_t;

/* Replaces Isolated_Cache / SSD_GNN_NVSHMEM_Cache ctors (ssd_gnn_cache.cuh:84-109,227-252) and
 * Isolated_cache_handle / NVSHMEM_cache_handle ctors (isolated_cache.h:520-636, nvshmem_cache.h:525-640). */
int coala_cache_create(const coala_cache_config_t* cfg, coala_cache_t** out);
/* Replaces the destructors (isolated_cache.h:638-653, ssd_gnn_cache.cuh:366-369). */
int coala_cache_destroy(coala_cache_t* h);

typedef struct coala_cache_geometry {
    uint64_t num_sets;
    uint32_t num_ways;
    uint32_t cache_dim;   /* floats per line */
    uint64_t line_bytes;  /* cache_dim * 4   */
    uint64_t table_bytes; /* HBM bytes held by lines + tags + metadata */
    uint32_t tag_set_bytes; /* bytes of one set's 32 tags as stored: 128 (32-bit tags) or 256 (COALA_FLAG_TAG64 / num_rows >= 2^32) */
    uint32_t reserved;
} coala_cache_geometry_t;
int coala_cache_geometry(const coala_cache_t* h, coala_cache_geometry_t* out);

/* out[i, 0:dim] = cache(idx[i]) for i in [0, n).  Replaces Isolated_Cache::read_feature (ssd_gnn_cache.cuh:255-268),
 * Isolated_read_feature_kernel (cache_kernel.cu:59-77) and Isolated_cache_d_t::get_data (isolated_cache.h:335-475).
 * With COALA_FLAG_DISTRIBUTED the set index is the distributed one (see coala_cache_serve).
 * `out` fp32 [n, dim] and `idx` int64 [n] are device pointers.  Batch-synchronous, deterministic replacement:
 * every probe sees the pre-call table; misses then take ways (set_cnt + k) % 32 in order of position. */
int coala_cache_read_feature(coala_cache_t* h, float* out, const int64_t* idx, int64_t n, void* stream);

/* Owner-side serve of the partitioned cache: same as coala_cache_read_feature but always with the distributed set index
 * set = (id / n_gpus) % sets, whatever the handle's flags.  Replaces Isolated_Cache::nccl_get_feature
 * (ssd_gnn_cache.cuh:297-325: get_data(id, out, local_size, true)) and SSD_GNN_NVSHMEM_Cache::read_feature
 * (ssd_gnn_cache.cuh:132-174) minus the transport.  ids = concatenation, in source-rank order, of the ids routed to
 * this owner; out = packed fp32 [n, dim] in the same order. */
int coala_cache_serve(coala_cache_t* h, float* out, const int64_t* ids, int64_t n, void* stream);

/* The same serve in two phases, for callers that overlap the cold fill with the exchange of rows that are already in place
 * (ssd_gnn_cache.cuh:132-174 serves and ships peer by peer on separate streams): serve_probe classifies the WHOLE batch and
 * copies the hits; serve_fill completes the positions [begin, end) -- ranking still spans the whole batch, so any set of
 * fills that covers [0, n) exactly once, in any order, leaves table, counters and rows exactly as one coala_cache_serve does.
 * Same out / ids / n in every call of one batch.  The batch stays OPEN until its fills have covered [0, n): until then any
 * new probe (read_feature, serve, serve_probe*) and any fill that overlaps an earlier one returns COALA_EINVAL;
 * coala_cache_serve_abort drops an open batch (its misses stay uncached, rows of unfilled positions are undefined). */
int coala_cache_serve_probe(coala_cache_t* h, float* out, const int64_t* ids, int64_t n, void* stream);
int coala_cache_serve_fill(coala_cache_t* h, float* out, const int64_t* ids, int64_t n, int64_t begin, int64_t end, void* stream);
/* One fill over a union of disjoint position ranges (HOST arrays begins/ends of n_ranges entries): one kernel launch per 64
 * ranges.  A row exchange split into rounds fills "the k-th slice of every peer's segment" with one call per round. */
int coala_cache_serve_fill_ranges(coala_cache_t* h, float* out, const int64_t* ids, int64_t n, const int64_t* begins,
                                  const int64_t* ends, int n_ranges, void* stream);
int coala_cache_serve_abort(coala_cache_t* h, void* stream);

/* serve_probe with part of the batch delivered elsewhere: rows at batch positions [begin, end) are written to
 * redirect->out[row_map[pos - begin], 0:dim] (row_map: device int64[end-begin], NULL = row pos - begin) instead of
 * out[pos, 0:dim], by the probe and by every later fill of the batch.  This is how the requester's OWN shard of a
 * distributed fetch goes straight into the caller's tensor (the reference's `j == i` local copy,
 * COALA-GNN-Setup/COALA_GNN/COALA_GNN_Manager.py:195-199) while staying part of the owner's one batch per step.
 * `out` may be NULL when the redirect covers the whole batch.
 * Every row_map entry must lie in [0, 2^31): the probe carries a row's destination as a 32-bit value (a batch never has more
 * rows than that: n <= 2^31 - 1 is checked).  The entries live in device memory, so the library cannot check them on the host: a
 * value outside that range addresses the wrong row.  The library's own caller (coala_cache_fetch_distributed) passes positions
 * of the batch, which are below n by construction. */
typedef struct coala_row_redirect {
    int64_t begin, end;
    float* out;
    const int64_t* row_map;
} coala_row_redirect_t;
int coala_cache_serve_probe_redirect(coala_cache_t* h, float* out, const int64_t* ids, int64_t n, const coala_row_redirect_t* redirect,
                                     void* stream);

/* Bucket idx by owner = id % n_parts, stable inside each bucket.  Replaces Isolated_Cache::split_node_list
 * (ssd_gnn_cache.cuh:283-295) / nccl_split_node_list_kernel (cache_kernel.cu:79-91) and the routing half of
 * NVSHMEM_send_requests_kernel (cache_kernel.cu:4-17).
 *   node_out, map_out : int64 device buffers.  bucket_stride > 0: bucket g starts at g*bucket_stride (the reference's
 *                       [G][max_sample] layout).  bucket_stride == 0: buckets are packed back to back (all-to-all-v
 *                       send layout) and offsets_out[g] (int64[n_parts+1], device) receives the bucket starts.
 *   counts_out        : int64[n_parts] device. */
int coala_cache_route(coala_cache_t* h, const int64_t* idx, int64_t n, int n_parts, int64_t bucket_stride,
                      int64_t* node_out, int64_t* map_out, int64_t* counts_out, int64_t* offsets_out, void* stream);

/* out[map[r], 0:dim] = src[r, 0:dim] for r in [0, n).  Replaces Isolated_Cache::map_feat_data
 * (ssd_gnn_cache.cuh:327-356) / nccl_gather_feature_kernel + block_memcpy (cache_kernel.cu:113-137). */
int coala_cache_scatter(coala_cache_t* h, float* out, const float* src, const int64_t* map, int64_t n, void* stream);
/* The same for the rows r of a union of disjoint ranges (HOST arrays): what one round of a split row exchange delivered. */
int coala_cache_scatter_ranges(coala_cache_t* h, float* out, const float* src, const int64_t* map, const int64_t* begins,
                               const int64_t* ends, int n_ranges, void* stream);

/* Floats per row of the cold table / output (cfg.dim). */
int64_t coala_cache_row_dim(const coala_cache_t* h);

/* ------------------------------------------------------------------------------------------------------------
 * Write-through row updates: trainable rows (DGL's dgl.nn.NodeEmbedding under dgl.optim.SparseAdagrad) in the table the cache
 * fronts.  Not in the reference, which only reads.  cfg.cold_table stays `const float*`; these calls cast it, so a handle that is
 * written to needs a WRITABLE, device-visible table (pinned host or HBM).
 *   ids   : device int64[n], pairwise distinct (the caller's duty).
 *   src / grad : device-visible fp32 [n, dim].
 *   state : device-visible fp32 [num_rows, dim], HBM or pinned host, addressed by id; it is not cached.  Adam has two (exp_avg,
 *           exp_avg_sq) and an optional int32 [num_rows] step vector; row-wise Adagrad has one fp32 [num_rows] vector instead.
 * What a write changes.  row(id) is the cold-table row `id` plus every cache line whose tag equals id.  A write stores the new value to
 * the cold row and to EVERY way of the id's set whose tag matches, not only the lowest one: the same id can sit in several ways (a read
 * inserts one copy per duplicate miss of a batch), reads take the lowest matching way, and once round robin evicts that copy the next
 * one is read.
 * Where the old value comes from (mode 1, Adagrad, Adam, row-wise Adagrad).  It is read once: on a hit from the lowest matching line (no host-link read),
 * otherwise from the cold row.
 * The invariant.  Before and after every call, every valid line holds the bytes of its cold row in floats [0, dim).
 * What a write leaves alone.  It never inserts, evicts or ranks: keys, set_cnt, color_meta, the colour counters and the hit / miss
 * counters are exactly as before, and line floats [dim, cache_dim) are not touched.
 * Bad ids.  An id outside [0, num_rows) writes nothing and is counted in range_errors, as a rejected read is.  With a repeated id the
 * row holds an unspecified mix of the writes; nothing out of bounds is read or written and the handle stays usable.
 * Order and refusals.  The call takes the handle's program order across streams exactly as a read does, and synchronises only under
 * COALA_FLAG_SYNC.  COALA_EINVAL with a message, before any launch, for: a null handle; n outside [0, 2^31 - 1]; a null buffer with
 * n > 0; a mode outside 0..1; an open serve batch; cfg.n_gpus != 1, COALA_FLAG_DISTRIBUTED or COALA_FLAG_COLD_PARTITIONED (a second
 * cache over the same table would keep stale lines; so the cold row is always `id`).  n == 0 returns COALA_OK and launches nothing.
 * Adam also refuses a beta outside [0, 1) and, without a row_step vector, step < 1.
 * One kernel per call.  16-byte accesses when dim % 4 == 0 and the cold table, src / grad and every [num_rows, dim] state table are
 * 16-byte aligned, 4-byte accesses otherwise (the rule of coala_cache_read_feature).
 * ------------------------------------------------------------------------------------------------------------ */
/* mode 0 (assign): row(id) = src[i];  mode 1 (add): row(id) = fmaf(alpha, src[i], row(id)) */
int coala_cache_write_rows(coala_cache_t* h, const int64_t* ids, int64_t n, const float* src, int mode, float alpha, void* stream);
/* s = state[id] + g*g;  state[id] = s;  row(id) -= lr * g / (sqrtf(s) + eps),  g = grad[i]  (torch.optim.Adagrad / DGL SparseAdagrad,
 * element-wise state) */
int coala_cache_adagrad_rows(coala_cache_t* h, const int64_t* ids, int64_t n, const float* grad, float* state, float lr, float eps,
                             void* stream);
/* Adam, per element (DGL's SparseAdam; torch.optim.SparseAdam's rule up to rounding):
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g*g;  row(id) -= lr (m / bc1) / (sqrt(v / bc2) + eps),  bc_i = 1 - beta_i^t.
 * t is the row's own count after the increment when row_step != NULL (t = ++row_step[id], saturating at INT32_MAX: lazy Adam, as DGL
 * counts), else `step` >= 1 for every row (torch's rule).  bc_i = -expm1(t ln beta_i), once per row in double, ln beta_i from the fp32
 * beta_i; 1 - beta^t itself loses four digits to cancellation at t = 1, beta2 = 0.999.  exp_avg / exp_avg_sq: [num_rows, dim] each. */
int coala_cache_adam_rows(coala_cache_t* h, const int64_t* ids, int64_t n, const float* grad, float* exp_avg, float* exp_avg_sq,
                          int32_t* row_step, int64_t step, float lr, float beta1, float beta2, float eps, void* stream);
/* Row-wise Adagrad (DGL-KE's rule; one float of state per row):
 *   s = row_state[id] + (1 / dim) sum_k g_k^2;  row_state[id] = s;  row(id)_k -= lr g_k / (sqrtf(s) + eps).
 * The sum has a fixed order (per lane, then an xor butterfly over the row's lanes): s is bitwise reproducible from run to run. */
int coala_cache_rowwise_adagrad_rows(coala_cache_t* h, const int64_t* ids, int64_t n, const float* grad, float* row_state, float lr,
                                     float eps, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Native fused fetch of the owner-partitioned cache over RCCL (one process per GPU, one communicator per cache group).
 * Replaces, in one call: SSD_GNN_NVSHMEM_Cache::send_requests + read_feature (ssd_gnn_cache.cuh:111-174) and the "nccl"
 * orchestration of COALA_GNN_Manager.fetch_feature (COALA-GNN-Setup/COALA_GNN/COALA_GNN_Manager.py:143-211):
 * route -> all-to-all(counts) -> one host read -> all-to-all-v(ids) -> probe (own shard straight into `out`) ->
 * { cold fill of slice k  ||  all-to-all-v(rows of slice k-1) on a second stream } -> un-permute.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct coala_comm coala_comm_t;
/* ncclGetUniqueId: called by ONE rank; the 128 bytes are handed to the others by any side channel (torch.distributed). */
int coala_comm_unique_id(void* out_id, size_t cap);
/* ncclCommInitRank: collective over the nranks processes of the group (one process per GPU, RCCL over xGMI). */
int coala_comm_create(const void* id_bytes, int rank, int nranks, int device, coala_comm_t** out);
int coala_comm_destroy(coala_comm_t* c);
/* Ranks of the communicator AS THE TRANSPORT SEES THEM: ncclCommCount for RCCL (and ncclCommUserRank is checked against `rank`
 * at creation), the group size for the in-process transport.  Negative on failure. */
int coala_comm_size(const coala_comm_t* c);
/* In-process transport: the nranks ranks of a group are host THREADS of one process (one communicator each, any mix of
 * devices, several ranks per device allowed); ids and rows move with device-to-device copies ordered by events -- a copy kernel
 * on the receiver's device when the sender's memory is on the same device or on a peer whose access could be enabled
 * (hipDeviceCanAccessPeer / hipDeviceEnablePeerAccess, once per device pair), the runtime's hipMemcpyAsync otherwise.  Same orchestration as over RCCL -- it is how the parity tests run G logical ranks on one GPU, and how a
 * single-process multi-GPU driver would use the partitioned cache.  The group outlives its communicators. */
typedef struct coala_comm_group coala_comm_group_t;
int coala_comm_group_create(int nranks, coala_comm_group_t** out);
int coala_comm_group_destroy(coala_comm_group_t* g);
int coala_comm_create_inproc(coala_comm_group_t* g, int rank, int device, coala_comm_t** out);
/* Row-exchange rounds per fetch, 1..8 (default 2, or COALA_EXCHANGE_ROUNDS): round k ships the k-th slice of every peer's
 * segment while the cold fill of slice k+1 runs.  Must be the same on every rank. */
int coala_comm_set_rounds(coala_comm_t* c, int rounds);
int coala_comm_get_rounds(const coala_comm_t* c); /* 0 for a null handle */
/* Diagnostics (off by default; the same setting on every rank): with on != 0 a rank's OWN segment takes the road of a peer's -- no
 * own-shard bypass, its rows are served into the staging buffer, shipped in rounds on the communicator's stream and un-permuted, and
 * the RCCL transport moves it with ncclSend + ncclRecv to ITSELF inside the same group call as the peers' segments instead of a local
 * copy.  Delivered rows and cache state are the same.  It exists so that a communicator of one rank -- all a one-GPU box can create
 * over RCCL -- executes every line of the exchange (counts, datatypes, displacements, both streams) on the real transport. */
int coala_comm_set_self_loopback(coala_comm_t* c, int on);
/* per-peer id counts of the last fetch (host int64[nranks] each, either may be NULL) */
int coala_comm_last_counts(const coala_comm_t* c, int64_t* send, int64_t* recv);
/* out[i, 0:dim] = row of idx[i], wherever its owner (idx[i] % nranks) is.  Collective: every rank of the communicator calls
 * it once per step (n may be 0).  Split-phase: ids go out, the owner probes its ONE batch per step (the concatenation of what
 * it received, in source-rank order), the requester's own shard lands directly in `out`, and the rows of the other peers come
 * back in rounds on the communicator's own stream while the owner's cold fill of the next round runs on `stream`.
 * Synchronises `stream` once, in the middle (the counts); everything after that is enqueued, and `stream` is ordered behind
 * the communicator's stream on return.  Error behaviour: argument and allocation checks happen before the first collective; a
 * failure after it aborts the transport (ncclCommAbort) so that the peers fail too instead of waiting -- the communicator
 * then only accepts coala_comm_destroy. */
int coala_cache_fetch_distributed(coala_cache_t* h, coala_comm_t* c, float* out, const int64_t* idx, int64_t n, void* stream);
/* The same for ids that arrive ALREADY bucketed by owner (idx = bucket 0 | bucket 1 | ..., counts_dev = device int64[nranks]
 * bucket sizes summing to n -- what coala_sampler_sample delivers with `bucketing`): no routing pass, no un-permute, the rows
 * of owner p are received straight into out[offset of bucket p ...] and the own bucket is gathered in place.
 * out[i] = row of idx[i] as above. */
int coala_cache_fetch_distributed_bucketed(coala_cache_t* h, coala_comm_t* c, float* out, const int64_t* idx, int64_t n,
                                           const int64_t* counts_dev, void* stream);
/* The bucketed fetch without its host synchronisation (opt-in): the count exchange is split off and issued AHEAD -- typically right
 * behind the sampler that produced counts_dev, on the sampler's stream, one or two steps before the fetch -- and the fetch then
 * finds both count vectors on the host.  coala_comm_counts_begin is a collective (counts all-to-all + a copy to pinned memory +
 * an event; no host wait; up to 8 may be outstanding); every rank issues its calls on one communicator in the same order.
 * coala_cache_fetch_distributed_bucketed_ahead(ticket) waits for that exchange's event (normally long complete) and runs the rest of
 * the sequence -- ids, probe, fill rounds beside row rounds -- fully stream-ordered.  Rows and cache state equal the plain call's. */
int coala_comm_counts_begin(coala_comm_t* c, const int64_t* counts_dev, void* stream, int64_t* ticket_out);
int coala_cache_fetch_distributed_bucketed_ahead(coala_cache_t* h, coala_comm_t* c, float* out, const int64_t* idx, int64_t n,
                                                 int64_t ticket, void* stream);
/* ------------------------------------------------------------------------------------------------------------
 * Completion and timing of a read WITHOUT packets of their own.  With coala_cache_fetch_events(h, 1) every coala_cache_read_feature
 * attaches a begin event to its first kernel launch and an end event to its last one (hipExtLaunchKernelGGL: the events ride on the
 * two dispatch packets).  coala_cache_last_fetch_events hands out the pair of the most recent call -- owned by the handle, valid for
 * the next 2048 calls, NULL when that call launched nothing (n = 0), when the handle profiles (COALA_FLAG_PROFILE uses the dispatches'
 * event slots itself) or for the split-phase serve calls: the caller then records an event of its own.  A consumer on another stream
 * waits with coala_stream_wait_event (hipStreamWaitEvent); coala_event_elapsed_ms gives begin -> end in milliseconds (wait = 0:
 * returns 1, no error, while the end event has not completed).  What it costs, by the kernels' own timestamps (profiles/r04_handover.txt):
 * plain launches hand over from the fill of one read to the probe of the next without a gap; these riding events 14 us per read (an
 * attached event makes its kernel wait for, and be waited for by, its neighbours); ONE hipEventRecord behind the read 6 us; a recorded
 * timing pair + completion event 15 us.  So: the cheapest completion signal is one recorded event, and this interface is for per-read
 * TIMING (what COALA_FLAG_PROFILE does per kernel).  The reference synchronises the device after every call instead
 * (ssd_gnn_cache.cuh:266).
 * ------------------------------------------------------------------------------------------------------------ */
int coala_cache_fetch_events(coala_cache_t* h, int enable);
int coala_cache_last_fetch_events(const coala_cache_t* h, void** begin_ev, void** end_ev);
int coala_stream_wait_event(void* stream, void* event);
int coala_event_elapsed_ms(void* begin_ev, void* end_ev, int wait, float* ms_out);

/* The same for a fetch over a communicator (opt-in; bucketed fetches).  enable = 1: a bucketed fetch hands out two END events -- the one its
 * last fill launch on the caller's stream carries anyway (the hand-over to the row round), and one recorded behind the last row round on
 * the communicator's own stream -- so that a consumer's stream can wait for the rows without a completion event recorded on the caller's
 * stream (the rows are complete once BOTH have completed).  enable = 2: additionally a BEGIN event on the probe's launch, for a timer
 * (begin -> end_ev_comm); an event on a launch costs that launch about 5 us (profiles/r04_handover.txt), so a caller that samples its
 * timing asks for it on the sampled fetches only.  coala_comm_last_fetch_events hands out the three (owned by the communicator, valid for
 * 2048 fetches; begin_ev NULL with enable = 1; end_ev_comm NULL for a communicator of one rank; all NULL after a routed fetch or an empty
 * batch: the caller then records its own).  Independently of this switch the fetch puts its internal hand-over events (fill of round k ->
 * row round k) on the fill launches and waits for the last row round only. */
int coala_comm_fetch_events(coala_comm_t* c, int enable);
int coala_comm_last_fetch_events(const coala_comm_t* c, void** begin_ev, void** end_ev_stream, void** end_ev_comm);

/* Timing of the row exchange (all rounds of a fetch, HIP events on the communicator's stream; includes any wait for the fill of
 * a later round): enable = 1 / 0 switches it, -1 leaves it; out (nullable) receives the totals since the last reset. */
typedef struct coala_comm_profile {
    double rows_ms;          /* summed duration of the row exchange */
    uint64_t calls;          /* fetches timed */
    uint64_t remote_rows_in; /* rows received from other ranks */
} coala_comm_profile_t;
int coala_comm_profile(coala_comm_t* c, int enable, coala_comm_profile_t* out, int reset);

/* Copy the colour occupancy counters to HOST memory dst[0 .. n_entries).  Replaces get_cache_data
 * (ssd_gnn_cache.cuh:176-186,270-280).  The reference copies num_colors entries; pass num_colors+1 to also get the
 * last colour.  Synchronises `stream`. */
int coala_cache_color_counts(coala_cache_t* h, int32_t* dst, int32_t n_entries, void* stream);
/* The same snapshot in two halves: _async enqueues the copy at this point of `stream` and returns without waiting; _finish (any
 * thread) waits for that copy only and delivers dst[0 .. n_entries).  One snapshot may be pending per handle. */
int coala_cache_color_counts_async(coala_cache_t* h, int32_t n_entries, void* stream);
int coala_cache_color_counts_finish(coala_cache_t* h, int32_t* dst, int32_t n_entries);

/* hit / miss counters since the last reset.  Replaces print_stats_kernel / print_stats (cache_kernel.cu:139-143,
 * isolated_cache.h:132-141), which print and reset.  Synchronises `stream`.  range_errors counts rejected ids. */
int coala_cache_stats(coala_cache_t* h, uint64_t* hit, uint64_t* miss, uint64_t* range_errors, int reset, void* stream);

/* Debug / test access to the table (device -> host copies; synchronising).  Any pointer may be NULL.
 * keys: u64[sets*32]; set_cnt: u32[sets]; color_meta: u32[sets*32]. */
int coala_cache_dump(coala_cache_t* h, uint64_t* keys, uint32_t* set_cnt, uint32_t* color_meta, void* stream);

/* With COALA_FLAG_PROFILE: accumulated hipEvent time (ms) and launch count of the probe+gather kernel and of the
 * cold-fill kernel since the last reset; rows_* are the rows each processed.  Synchronises the recorded events. */
typedef struct coala_cache_profile {
    double gather_ms;
    uint64_t gather_launches;
    uint64_t gather_rows;   /* rows probed */
    uint64_t gather_hits;   /* rows copied from HBM lines */
    double fill_ms;
    uint64_t fill_launches;
    uint64_t fill_rows;
    double event_overhead_us; /* median elapsed time of an EMPTY hipEvent bracket on the same stream: what every bracketed */
                              /* launch above includes on top of the kernel itself                                        */
} coala_cache_profile_t;
int coala_cache_profile(coala_cache_t* h, coala_cache_profile_t* out, int reset);

/* ------------------------------------------------------------------------------------------------------------
 * Offline graph colouring + colour-affinity tables (host only).  Replaces Graph_Coloring
 * (COALA_GNN_Modules/graph_coloring.h:15-68, graph_coloring.cpp) driven by examples/color_info_gen/generate_color_data.py.
 * All buffers are HOST pointers owned by the caller, int64 (the reference aliases int64 torch tensors as uint64).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct coala_coloring coala_coloring_t;
int coala_coloring_create(uint64_t num_nodes, coala_coloring_t** out);                                  /* Graph_Coloring(u64) */
int coala_coloring_destroy(coala_coloring_t* g);
int coala_coloring_set_adj_csc(coala_coloring_t* g, const int64_t* indptr, const int64_t* indices);     /* set_adj_csc */
int coala_coloring_set_color_buffer(coala_coloring_t* g, int64_t* color);                               /* set_color_buffer (zeroed [N]) */
/* set_topk_color_buffer / set_topk_affinity_buffer: [num_colors*topk]; either pointer may be NULL to keep the current one */
int coala_coloring_set_topk_buffers(coala_coloring_t* g, int64_t* topk_color, double* topk_affinity, int topk);
/* cpu_color_graph_optimized(train_ptr, n): seeds sampled from the training nodes with glibc rand(); seed 1 reproduces the
 * reference (which never calls srand) */
int coala_coloring_color_optimized(coala_coloring_t* g, const int64_t* train, uint64_t n_train, unsigned seed);
int coala_coloring_color_all(coala_coloring_t* g, unsigned seed);                                       /* cpu_color_graph */
uint64_t coala_coloring_num_color(const coala_coloring_t* g);                                           /* get_num_color */
uint64_t coala_coloring_num_color_node(const coala_coloring_t* g);                                      /* get_num_color_node */
/* with_affinity=1: cpu_calculate_color_affinity; 0: cpu_count_nearest_color_less_memory */
int coala_coloring_topk(coala_coloring_t* g, int with_affinity);
int coala_coloring_nearest(coala_coloring_t* g);                                                        /* cpu_count_nearest_color */

/* ------------------------------------------------------------------------------------------------------------
 * Neighbour sampler + block compaction over a CSC graph resident in device-visible memory (HBM, or pinned host).
 * Replaces the DGL call on the hot path: graph_sampler.sample(g, seeds) with
 * dgl.dataloading.MultiLayerNeighborSampler(fanouts) (COALA-GNN-Setup/COALA_GNN/COALA_GNN_DataLoader.py:162,
 * examples/sbatch_ssd_gnn_train.py:70-72; graph: examples/ssd_gnn_dataloader.py:523).  DGL's arithmetic is not under
 * /root/reference; the contract (coala_sampler.hip header) is pinned by properties and by the CPU twin in oracle/.
 * ------------------------------------------------------------------------------------------------------------ */
#define COALA_SAMPLER_MAX_LAYERS 8
typedef struct coala_sampler coala_sampler_t;
/* indptr int64[num_nodes+1], indices int64[num_edges]: device-visible, borrowed for the sampler's lifetime. */
int coala_sampler_create(int device, const int64_t* indptr, const int64_t* indices, int64_t num_nodes, int64_t num_edges,
                         coala_sampler_t** out);
int coala_sampler_destroy(coala_sampler_t* s);
/* Sample n_layers layers starting from `seeds` (device int64[n_seeds]).  fanouts[l] is the fan-out of the l-th SAMPLED
 * layer (DGL walks reversed(fanouts): pass them already reversed).  Layer l's destination nodes are layer l-1's source
 * nodes.  Outputs, all device buffers owned by the caller, for cap_0 = n_seeds, cap_{l+1} = cap_l*(fanouts[l]+1):
 *   src_nodes_out[l] : int64[cap_{l+1}]        source (input) nodes of block l: its dst nodes first, then new ones
 *   nbr_local_out[l] : int32[cap_l*fanouts[l]] row d holds the local indices of dst d's sampled neighbours, -1 padded
 *   n_src_host[l]    : HOST int64, number of source nodes of block l.  Non-NULL: the call returns when the counts are there (it
 *                      waits on an event behind the sampler's one kernel, not on the stream).  NULL: the call only enqueues;
 *                      collect the counts later with coala_sampler_wait(ticket) -- up to 8 calls may be outstanding.
 * The sample is a short sequence of kernels on `stream` (three per layer, four more for the bucketing); the layers read their sizes
 * from device memory, so nothing waits in between.
 * Randomness: counter-based, keyed by (seed, step, layer, node id): same arguments, same sample.
 *
 * bucketing (nullable): additionally deliver the input nodes of the LAST layer bucketed by owner = id % n_parts, stable inside
 * each bucket -- the layout the owner-partitioned fetch sends (coala_cache_fetch_distributed_bucketed: no routing pass, rows are
 * received straight into the output tensor).  With it nbr_local_out[n_layers-1] indexes `bucketed_nodes` and dst_in_src[d] is
 * the position of the block's d-th destination node in it (the "dst nodes first" convention cannot hold for a bucketed list);
 * src_nodes_out[n_layers-1] still receives the unbucketed first-appearance list. */
typedef struct coala_sampler_bucketing {
    int32_t n_parts;         /* owners (1..64); 0 = off                                  */
    int32_t reserved;
    int64_t* bucketed_nodes; /* device int64[cap_L]                                      */
    int64_t* counts;         /* device int64[n_parts]: bucket sizes                      */
    int32_t* dst_in_src;     /* device int32[cap_{L-1}]                                  */
} coala_sampler_bucketing_t;
int coala_sampler_sample(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                         uint64_t seed, uint64_t step, int64_t* const* src_nodes_out, int32_t* const* nbr_local_out,
                         int64_t* n_src_host, const coala_sampler_bucketing_t* bucketing, int64_t* ticket_out, void* stream);
/* Counts of an earlier call (its ticket): n_src_host[n_layers] and, when it bucketed, bucket_counts_host[n_parts] (either NULL). */
int coala_sampler_wait(coala_sampler_t* s, int64_t ticket, int64_t* n_src_host, int64_t* bucket_counts_host);

/* Per-layer outputs, for fixed and full layers alike (coala_sampler_sample_layers).  fanouts[l] is 1..32, or -1 for a FULL layer:
 * every in-edge of every destination node, in CSC order (repeated edges and self-loops kept, degree 0 gives an empty segment); it
 * draws no random numbers, and fixed layers keep their layer index l as the RNG key.  The source list follows the same rule as a
 * fixed layer: the dst nodes first, then every other neighbour in order of first appearance in the row-major (d, edge) scan.
 * A full layer's block is CSR: indptr_local int64[n_dst + 1] (exclusive scan of the degrees) and nbr_local int32[E] (local source
 * index of each edge).
 * Capacities, with dst_cap_0 = n_seeds:
 *   fixed layer, no full layer before it: src_cap >= dst_cap * (f + 1), edge_cap >= dst_cap * f, and dst_cap * (f + 1) <= 8,388,608
 *     (checked here: COALA_EINVAL); dst_cap of the next layer = dst_cap * (f + 1);
 *   full layer: indptr_local holds dst_cap + 1 entries; its item count n_dst + E must stay <= min(8,388,608, src_cap) and E <= edge_cap;
 *     dst_cap of the next layer = min(8,388,608, src_cap);
 *   fixed layer behind a full layer: its worst case n_dst * (f + 1) must stay <= min(8,388,608, src_cap), n_dst * f <= edge_cap;
 *     dst_cap of the next layer = min(dst_cap * (f + 1), 8,388,608, src_cap).
 * The last two are known on the device only and are checked there: the call's remaining kernels then see empty layers and write
 * nothing past the capacities, and coala_sampler_wait_layers (or this call, when it waits) returns COALA_EINVAL with a message that
 * names the layer and its item count.  The handle stays usable.  With `bucketing`, bucketed_nodes holds dst_cap of the layer after
 * the last one, dst_in_src the last layer's dst_cap; a full input layer's nbr_local then indexes bucketed_nodes. */
typedef struct coala_sampler_layer {
    int64_t* src_nodes;    /* device int64[src_cap]: source nodes of the block                                    */
    int32_t* nbr_local;    /* device int32[edge_cap]: fixed -> [n_dst, f] -1 padded; full -> [E]                 */
    int64_t* indptr_local; /* full or LABOR layer: device int64[dst_cap + 1]; fixed layer: unused (NULL)          */
    int64_t src_cap;
    int64_t edge_cap;
} coala_sampler_layer_t;
/* As coala_sampler_sample, with per-layer outputs and fan-out -1.  n_edges_host[l] (nullable, HOST): E of a full layer, n_dst * f of
 * a fixed one.  coala_sampler_sample keeps refusing -1: its dense outputs cannot hold a full layer. */
int coala_sampler_sample_layers(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                                uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, int64_t* n_src_host,
                                int64_t* n_edges_host, const coala_sampler_bucketing_t* bucketing, int64_t* ticket_out, void* stream);
/* As coala_sampler_sample_layers, with edge-weighted fixed layers (DGL's NeighborSampler(fanouts, prob=...), replace=False).
 * edge_weights: device fp32[num_edges] in CSC order (aligned with `indices`), finite and >= 0 (the caller validates them), borrowed for
 * the call.  A fixed layer draws f distinct edges of positive weight with probability proportional to the weight (Efraimidis-Spirakis
 * keys; the exact rule is in the header of coala_sampler.hip), takes every positive-weight edge when there are at most f, never takes
 * a weight-0 edge, and lists them in CSC order, -1 padded.  Full layers (-1) keep every in-edge and read no weights.  Outputs,
 * capacities, refusals and bucketing are those of coala_sampler_sample_layers; counts come back through coala_sampler_wait_layers. */
int coala_sampler_sample_layers_weighted(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                                         uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, const float* edge_weights,
                                         int64_t* n_src_host, int64_t* n_edges_host, const coala_sampler_bucketing_t* bucketing,
                                         int64_t* ticket_out, void* stream);
/* As coala_sampler_sample_layers (edge_weights NULL) or coala_sampler_sample_layers_weighted (edge_weights given), and additionally
 * the CSC position of every sampled edge.  edge_ids_out: NULL, or an array of n_layers device pointers, each NULL (not wanted) or
 * int64[edge_cap of that layer], laid out exactly like the layer's nbr_local (fixed layer: [n_dst, f]; full layer: [E]).  Entry
 * (d, j) is the position e in the graph's `indices` array of the edge that slot holds -- indptr[v_d] <= e < indptr[v_d + 1] and
 * indices[e] is the neighbour -- and -1 where nbr_local is -1.  The ids of a fixed row are pairwise distinct (the draw is without
 * replacement), which tells repeated edges apart; a full row's ids are indptr[v] .. indptr[v + 1] - 1 in order.  The draw, the source
 * lists, nbr_local, indptr_local, the capacities, the refusals and the ticket / wait protocol are those of the calls above, bit for
 * bit for the same (seed, step); a refused layer writes nothing to its edge_ids_out.  The ids are stored by the kernels that read the
 * neighbours (one 8-byte store per slot): no launch is added, and a NULL array or entry costs nothing. */
int coala_sampler_sample_layers_edge_ids(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                                         uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, const float* edge_weights,
                                         int64_t* const* edge_ids_out, int64_t* n_src_host, int64_t* n_edges_host,
                                         const coala_sampler_bucketing_t* bucketing, int64_t* ticket_out, void* stream);
/* LABOR layer-neighbour sampling (DGL's LaborSampler(fanouts, importance_sampling=0); Balin & Catalyurek, NeurIPS 2023): as
 * coala_sampler_sample_layers_edge_ids without edge weights, but a fan-out k in 1..32 is a LABOR layer.  One random number r_t per
 * SOURCE node t is shared by every destination node of the layer: a destination node of in-degree deg <= k takes every in-edge;
 * otherwise its in-edge from t is taken iff mulhi64(r_t, deg) < k, r_t = splitmix64(labor_key(seed, step, l) ^ t) (the key is in the
 * header of coala_sampler.hip).  A row holds k neighbours in expectation, repeated edges are taken or left together, and destination
 * nodes that share a neighbour agree on it, so the source list is shorter than that of k independent picks per row.
 * layer_dependency != 0 drops the layer index from the key: every layer of the call sees the same r_t.
 * Every layer's block is CSR, exactly as a full layer's: indptr_local int64[n_dst + 1] is required for every layer, nbr_local holds
 * the E taken edges (ascending CSC position inside a row, rows in destination order), edge_ids_out (NULL, or per layer NULL or
 * int64[edge_cap]) their CSC positions.  E is known on the device only: capacities, the device-side refusal (n_dst + E over
 * min(8,388,608, src_cap), or E over edge_cap), the source-list rule, bucketing and the ticket / wait protocol are those of a full
 * layer; n_edges_host[l] is E.  A -1 entry is a full layer.  An out-of-range destination id gives an empty row.  Same arguments,
 * same sample.  Two launches stand where a full layer's degree_scan and full_insert stand; nothing is added to the stream. */
int coala_sampler_sample_layers_labor(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                                      uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, int64_t* const* edge_ids_out,
                                      int layer_dependency, int64_t* n_src_host, int64_t* n_edges_host,
                                      const coala_sampler_bucketing_t* bucketing, int64_t* ticket_out, void* stream);
/* Relation layers: a fan-out per edge type (DGL's NeighborSampler on a heterograph; on a homogenised graph dgl.sort_csc_by_tag followed by
 * sample_etype_neighbors(etype_sorted=True)).  etype: DEVICE int32[num_edges] in CSC order (aligned with `indices`), values in
 * [0, num_rels), borrowed for the call.  The types MUST BE NON-DECREASING INSIDE EVERY ROW [indptr[v], indptr[v + 1]): the in-edges of
 * relation r of a node are then one segment of its row, found by binary search.  This call does not verify the order -- that is the
 * caller's duty (COALA_GNN.sampler.sort_csc_by_etype sorts a graph; RelNeighborSampler checks it once per graph).  Types out of
 * order give rows that are not what the rule says, but nothing is read or written out of bounds.
 * rel_fanouts: HOST int32[n_layers][num_rels], layers in sampling order.  Relation r of layer l with f = rel_fanouts[l][r] and deg_r
 * in-edges of that type: f == 0 takes none, f == -1 or deg_r <= f takes them all, otherwise f distinct edges of the segment by the
 * uniform sampler's draw with the counters 64 r + j (the exact rule is in the header of coala_sampler.hip; with num_rels == 1 a row holds
 * the edges coala_sampler_sample_layers_edge_ids draws at the same seed and step).  A layer whose fan-outs are all -1 is a full layer.
 * Every layer's block is CSR, exactly as a LABOR layer's: indptr_local is required for every layer, nbr_local holds the E taken edges in
 * ascending CSC position inside a row (hence grouped by relation), edge_ids_out (NULL, or per layer NULL or int64[edge_cap]) their
 * CSC positions.  Capacities, the device-side refusal, the source-list rule, bucketing and the ticket / wait protocol are those of a
 * full layer; counts come back through coala_sampler_wait_layers.  COALA_EINVAL (with a message) for num_rels outside 1..64, a fan-out
 * outside {-1, 0..32}, a layer whose fan-outs are all 0, or a NULL etype. */
int coala_sampler_sample_layers_rel(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* rel_fanouts, int num_rels,
                                    int n_layers, uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, const int32_t* etype,
                                    int64_t* const* edge_ids_out, int64_t* n_src_host, int64_t* n_edges_host,
                                    const coala_sampler_bucketing_t* bucketing, int64_t* ticket_out, void* stream);
/* Random-walk layers (DGL's dgl.sampling.RandomWalkNeighborSampler / PinSAGESampler on a homogeneous graph): as coala_sampler_sample_layers,
 * but every layer is a walk layer.  From every destination node num_random_walks walks of num_traversals hops each start; a hop follows
 * a uniformly drawn in-edge, and a hop after the first ends the walk with probability term_threshold / 2^53 (term_threshold =
 * floor(termination_prob * 2^53) < 2^53, computed by the caller); a node without an in-edge ends it too.  The row of a destination node
 * holds the fanouts[l] (1..32) most visited nodes, most visited first, a tie going to the smaller node id, -1 padded -- a fixed-stride
 * block exactly as a uniform fixed layer's: indptr_local must be NULL, -1 fan-outs are refused, capacities, the source-list rule,
 * bucketing and the ticket / wait protocol are those of coala_sampler_sample_layers (n_edges_host[l] = n_dst * fanouts[l]).
 * visit_counts_out: NULL, or an array of n_layers device pointers, each NULL or int32[edge_cap of that layer] laid out like nbr_local:
 * how often the slot's node was visited, 0 on padding.  The draws are keyed by (seed, step, layer, destination node) on a stream of
 * their own (the exact rule is in the header of coala_sampler.hip): same arguments, same sample, whatever the batch.  Limits:
 * num_traversals 1..16, num_random_walks 1..64, their product <= 512; COALA_EINVAL (with a message) before any launch otherwise.
 * One launch stands where a uniform layer's sample_insert stands; nothing is added to the stream. */
typedef struct coala_sampler_walk {
    int32_t num_traversals;   /* hops per walk, 1..16                           */
    int32_t num_random_walks; /* walks per destination node, 1..64              */
    uint64_t term_threshold;  /* floor(termination_prob * 2^53), below 2^53     */
} coala_sampler_walk_t;
int coala_sampler_sample_layers_walk(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                                     uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, const coala_sampler_walk_t* walk,
                                     int32_t* const* visit_counts_out, int64_t* n_src_host, int64_t* n_edges_host,
                                     const coala_sampler_bucketing_t* bucketing, int64_t* ticket_out, void* stream);
/* The walks themselves (DGL's dgl.sampling.random_walk): traces_out device int64[n, num_walks, length + 1]; traces_out[i, w, 0] =
 * nodes[i], then the nodes walk w of nodes[i] visits, -1 once it has ended.  An out-of-range start node gives a row of -1.  By
 * definition this is walk w of node nodes[i] in sampled layer `layer` (0..7) of coala_sampler_sample_layers_walk at the same seed,
 * step and term_threshold: repeated start nodes get identical traces.  One kernel on `stream`; nothing is waited for. */
int coala_sampler_random_walk(coala_sampler_t* s, const int64_t* nodes, int64_t n, int num_walks, int length, uint64_t term_threshold,
                              uint64_t seed, uint64_t step, int layer, int64_t* traces_out, void* stream);
/* Temporal layers (PyG's NeighborLoader(time_attr=, temporal_strategy=), GraphBolt's temporal_sample_neighbors): as
 * coala_sampler_sample_layers_edge_ids without bucketing, but a destination item is a pair (node v, query time t) and a row draws only
 * from the edges with a timestamp before t.  edge_ts: device int64[num_edges] in CSC order, non-decreasing inside every row (the
 * caller's duty).  slot_time: device int64[n_slots], the distinct query times of the call, ascending.  A pair is the int64 code
 * slot << node_bits | v, node_bits the bit length of num_nodes; seed_codes (device int64[n_seeds], distinct) and every layer's src_nodes
 * hold such codes: a neighbour inherits its row's slot.  A code that is negative, or decodes to slot >= n_slots or v >= num_nodes, gives
 * an empty row.  Eligible edges of (v, t): the prefix of the row with ts < t (inclusive != 0: ts <= t), m edges, found by a search.
 * strategy 0 (uniform): all of them when m <= fanout, else fanout distinct ones by the uniform layer's draw with deg := m on a stream
 * keyed by (seed, step, layer, v, t) -- not by the slot, the batch or the grid; strategy 1 (last): the min(m, fanout) most recent, in
 * ascending position, nothing drawn.  The exact rule is in the header of coala_sampler.hip.  Every layer is fixed-stride (fan-out 1..32,
 * indptr_local NULL); capacities, the source-list rule, edge_ids_out and the ticket / wait protocol are a uniform fixed layer's, counts
 * come back through coala_sampler_wait_layers, and the call leaves the hash table cleared for any call that follows on the handle.
 * COALA_EINVAL (with a message) before any launch for a fan-out outside 1..32, a strategy outside 0..1, a NULL edge_ts or slot_time, or
 * node_bits + bit_length(n_slots - 1) > 62.  One launch stands where a uniform layer's sample_insert stands; nothing is added. */
int coala_sampler_sample_layers_temporal(coala_sampler_t* s, const int64_t* seed_codes, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                                         uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, const int64_t* edge_ts,
                                         const int64_t* slot_time, int64_t n_slots, int strategy /* 0 uniform, 1 last */, int inclusive,
                                         int64_t* const* edge_ids_out /* nullable */, int64_t* n_src_host, int64_t* n_edges_host,
                                         int64_t* ticket, void* stream);
/* Counts of an earlier call, with the edge counts of its layers; returns the device-side refusal of a full, LABOR or relation layer, if any. */
int coala_sampler_wait_layers(coala_sampler_t* s, int64_t ticket, int64_t* n_src_host, int64_t* n_edges_host, int64_t* bucket_counts_host);
/* Edge minibatches for link prediction (DGL's as_edge_prediction_sampler with negative_sampler.Uniform(num_neg)).  eids: device
 * int64[n], seed edges as CSC positions 0 <= e < num_edges.  Edge e has destination v, the row with indptr[v] <= e < indptr[v+1] (found
 * by an upper-bound search: degree-0 rows around v are never chosen), and source u = indices[e].  It gets num_neg (0..64) negative
 * pairs (u, v'_j), v'_j = mulhi64(splitmix64(nkey + j), num_nodes), nkey = sample_key(seed, step, 0, e) ^ 0xA54FF53A5F1D36F1 (a stream
 * of its own; sample_key is in the header of coala_sampler.hip): a function of (seed, step, e, j) alone, not of the batch, the edge's
 * place in it or the grid.  Negatives that are real edges, or equal u, are kept (as in DGL).
 * Outputs (device): seed_nodes int64[n (2 + num_neg)] = the distinct ids of the item list [src_0.. | dst_0.. | v'_{0,0} .. v'_{n-1,k-1}]
 * in order of first appearance (the source-list rule of the layers), n_nodes of them; pos_src, pos_dst int32[n] and neg_dst
 * int32[n, num_neg]: where every item sits in seed_nodes.  The source of a negative is its edge's pos_src.  An e outside [0, num_edges)
 * gives -1 in all of its entries, adds no node and is counted in n_bad.  Nothing is written past these capacities.
 * Limit: n (2 + num_neg) <= 8,388,608 items; COALA_EINVAL (with a message) before any launch otherwise, and for num_neg outside 0..64.
 * Three launches on `stream` (items + hash insert, the layers' scan_assign, relabel + table clear); no memset, copy or wait.
 * The batch contract, which coala_sampler_walk_batch shares: the call takes a ticket of the handle's ring like a sample; n_nodes and n_bad
 * go to pinned host memory from the kernels, and the batch kind's own wait (coala_sampler_edge_batch_wait, coala_sampler_walk_batch_wait)
 * collects them behind the call's event.  Each kind of wait -- these two, coala_sampler_wait and coala_sampler_wait_layers -- refuses the
 * other kinds' tickets with COALA_EINVAL, without waiting. */
typedef struct coala_edge_batch {
    int64_t* seed_nodes; /* int64[n (2 + num_neg)]                     */
    int32_t* pos_src;    /* int32[n]                                   */
    int32_t* pos_dst;    /* int32[n]                                   */
    int32_t* neg_dst;    /* int32[n, num_neg]; may be NULL, num_neg 0  */
} coala_edge_batch_t;
int coala_sampler_edge_batch(coala_sampler_t* s, const int64_t* eids, int64_t n, int num_neg, uint64_t seed, uint64_t step,
                             const coala_edge_batch_t* out, int64_t* ticket_out, void* stream);
int coala_sampler_edge_batch_wait(coala_sampler_t* s, int64_t ticket, int64_t* n_nodes_host, int64_t* n_bad_host);
/* Second-order walks (node2vec; DGL's dgl.sampling.node2vec_random_walk on a homogeneous graph): traces_out device int64[n, num_walks,
 * length + 1]; traces_out[i, w, 0] = nodes[i], then the nodes walk w visits, -1 once it has ended (a node without an in-edge, or a
 * neighbour id outside the graph).  An out-of-range start node gives a row of -1.  num_walks 1..64, length 1..127.  A hop is drawn by
 * rejection: a uniformly drawn in-edge of the current node is taken with probability thr / 2^32, thr = thr_return when it leads back
 * to the previous node, thr_near when it leads to an in-neighbour of the previous node, thr_far otherwise; after 256 refused attempts
 * the last candidate is taken.  The caller computes the thresholds from p and q (m = max(1/p, 1, 1/q): (1/p)/m, 1/m, (1/q)/m times
 * 2^32): any three values in [0, 2^32] whose largest is 2^32; COALA_EINVAL (with a message) otherwise, and nothing is launched.  The
 * exact rule, its keys and counters, is in the header of coala_sampler.hip; the walks are a function of (seed, step, start node, w)
 * on a stream of their own -- not coala_sampler_random_walk's.  When thr_near != thr_far the rows of the graph MUST BE SORTED
 * ASCENDING BY SOURCE ID (the near test is a binary search; not verified here: COALA_GNN.sampler.sort_csc_by_src sorts a graph);
 * unsorted rows give walks that are not what the rule says, but nothing is read out of bounds.  One kernel on `stream`; nothing is
 * waited for. */
int coala_sampler_node2vec_walk(coala_sampler_t* s, const int64_t* nodes, int64_t n, int num_walks, int length, uint64_t thr_return,
                                uint64_t thr_near, uint64_t thr_far, uint64_t seed, uint64_t step, int64_t* traces_out, void* stream);
/* Skip-gram batches (PyG's Node2Vec.pos_sample / neg_sample): the walks of coala_sampler_node2vec_walk from `nodes`, num_neg (0..16)
 * negative rows per walk, and everything relabelled to one list of distinct nodes.  Outputs (device), W = num_walks, L = length:
 *   pos int32[n W, L + 1]: every trace as indices into input_nodes, -1 where the walk has ended;
 *   neg int32[n W num_neg, L + 1] (may be NULL with num_neg 0): row (walk, j) holds the walk's start node in column 0 and in column
 *     t >= 1 the node mulhi64(splitmix64((kw ^ 0x6A09E667F3BCC909) + 128 j + t), num_nodes), kw the walk's key; an invalid start node
 *     gives rows of -1;
 *   input_nodes int64[n + n W (L + 1) + n W num_neg L]: the distinct ids of the item list [valid start nodes | pos rows row-major | neg
 *     columns 1.. row-major] in order of first appearance, n_nodes of them;
 *   traces int64[n, W, L + 1], nullable: the global-id traces, bit-identical to coala_sampler_node2vec_walk's.
 * Nothing is written past these capacities.  Limit: n W (L + 1) (1 + num_neg) <= 8,388,608 items; COALA_EINVAL (with a message) before
 * any launch otherwise, and for arguments coala_sampler_node2vec_walk refuses.  Three launches on `stream`; no memset, copy or wait.
 * Ticket, pinned words and wait: the batch contract of coala_sampler_edge_batch; n_bad counts the out-of-range start nodes. */
typedef struct coala_walk_batch {
    int64_t* input_nodes;
    int32_t* pos;
    int32_t* neg;
    int64_t* traces;
} coala_walk_batch_t;
int coala_sampler_walk_batch(coala_sampler_t* s, const int64_t* nodes, int64_t n, int num_walks, int length, uint64_t thr_return,
                             uint64_t thr_near, uint64_t thr_far, int num_neg, uint64_t seed, uint64_t step, const coala_walk_batch_t* out,
                             int64_t* ticket_out, void* stream);
int coala_sampler_walk_batch_wait(coala_sampler_t* s, int64_t ticket, int64_t* n_nodes_host, int64_t* n_bad_host);

/* Block op for the consumer of these blocks (the native Block objects stand where DGL blocks stand in
 * examples/sbatch_ssd_gnn_train.py:138-141; dgl.nn.SAGEConv's "mean" reduces to this): out[d, :] = mean over the valid j of
 * h_src[nbr[d, j], :]; nbr int32 [n_dst, fanout] (-1 padded, fan-out <= 32), fp32 rows of `dim` floats.  The backward adds
 * grad_out[d] / count(d) into grad_src[nbr[d, j]] with hardware float atomics (grad_src zeroed by the caller). */
int coala_block_mean_aggregate(int device, const int32_t* nbr, const float* h_src, float* out, int64_t n_dst, int fanout, int dim, void* stream);
int coala_block_mean_aggregate_backward(int device, const int32_t* nbr, const float* grad_out, float* grad_src, int64_t n_dst, int fanout,
                                        int dim, void* stream);
/* The same op on a ragged (CSR) block, the form of a full layer: row d averages h_src[indices[e]] for e in
 * [indptr[d], indptr[d+1]), summed in that order (bit-identical to the dense op on any row both can express); an empty row gives
 * zeros.  One wave aggregates a row, so a hub row of 10^6 edges runs on one wave. */
int coala_block_mean_aggregate_csr(int device, const int64_t* indptr, const int32_t* indices, const float* h_src, float* out, int64_t n_dst,
                                   int dim, void* stream);
int coala_block_mean_aggregate_csr_backward(int device, const int64_t* indptr, const int32_t* indices, const float* grad_out, float* grad_src,
                                            int64_t n_dst, int dim, void* stream);
/* Weighted sum aggregation (DGL's u_mul_e_sum: GraphConv / SAGEConv with edge_weight=): out[d, :] = sum over the valid j of
 * w[d, j] * h_src[nbr[d, j], :]; nbr int32 [n_dst, fanout] (-1 padded, fan-out 1..32), w fp32 [n_dst, fanout] (one weight per slot; a
 * padding slot's weight is not used), fp32 rows of `dim` floats; a row without a valid entry gives zeros.  The CSR form sums
 * w[e] * h_src[indices[e]] over e in [indptr[d], indptr[d+1]) in that order (w fp32 [E]), one wave per row.  The sum runs in slot order
 * with one fma per term, and both forms run the same code: bit-identical on any row both can express.  Bad shapes are refused with
 * COALA_EINVAL and nothing is launched.
 * Backward, both gradients in one launch, either output may be NULL (not wanted):
 *   grad_src[s_j, :] += w_j * grad_out[d, :]        hardware float atomics: the caller zeroes grad_src [n_src, dim], the order varies;
 *   grad_w[d, j] = <grad_out[d, :], h_src[s_j, :]>   shaped like w, written whole, 0 on a padding slot; deterministic, and the same bits
 *                                                   in both forms.  h_src is read only when grad_w is given.
 * Bytes per row of deg valid edges: forward reads deg * (4 dim + 8) and writes 4 dim; backward reads 4 dim + 8 deg (+ 4 dim deg for
 * grad_w), adds 4 dim deg through atomics and writes 4 per slot. */
int coala_block_weighted_sum(int device, const int32_t* nbr, const float* w, const float* h_src, float* out, int64_t n_dst, int fanout, int dim,
                             void* stream);
int coala_block_weighted_sum_backward(int device, const int32_t* nbr, const float* w, const float* h_src, const float* grad_out, float* grad_src,
                                      float* grad_w, int64_t n_dst, int fanout, int dim, void* stream);
int coala_block_weighted_sum_csr(int device, const int64_t* indptr, const int32_t* indices, const float* w, const float* h_src, float* out,
                                 int64_t n_dst, int dim, void* stream);
int coala_block_weighted_sum_csr_backward(int device, const int64_t* indptr, const int32_t* indices, const float* w, const float* h_src,
                                          const float* grad_out, float* grad_src, float* grad_w, int64_t n_dst, int dim, void* stream);
/* Max aggregation (DGL's fn.max reducer: SAGEConv "pool", GINConv "max"): out[d, c] = max over the valid j of h_src[nbr[d, j], c], and
 * arg[d, c] = the local source index of the winning slot (int32 [n_dst, dim], the only state the backward needs; NULL for inference:
 * nothing is stored).  nbr int32 [n_dst, fanout] (-1 padded, fan-out 1..32), fp32 rows of `dim` floats; the CSR form takes the maximum
 * over e in [indptr[d], indptr[d+1]), any degree, one wave per row.  The rule is torch.max(dim)'s: the running maximum starts from the
 * first valid slot, and a later slot replaces it when its value is greater, or is NaN while the maximum is not.  So ties (+-0
 * included) keep the first slot in slot order, a NaN propagates with arg at the first NaN, and a row of -inf gives -inf with a valid
 * arg.  A row without a valid entry gives out = 0 and arg = -1 (DGL's reducer at zero in-degree).  Nothing is rounded and both forms
 * run the same code: out and arg are deterministic, and bit-identical on any row both forms can express.  Bad shapes are refused with
 * COALA_EINVAL (fan-out 1..32, dim >= 1, n_dst >= 0); n_dst == 0 launches nothing.
 * Backward, one entry point for both forms: grad_src[arg[d, c], c] += grad_out[d, c] wherever arg[d, c] >= 0, hardware float atomics:
 * the caller zeroes grad_src [n_src, dim], the order varies.
 * Bytes per row of deg valid edges: forward reads deg * (4 dim + 4) and writes 4 dim (8 dim with arg); backward reads 8 dim and adds
 * 4 dim through atomics. */
int coala_block_max_aggregate(int device, const int32_t* nbr, const float* h_src, float* out, int32_t* arg, int64_t n_dst, int fanout, int dim,
                              void* stream);
int coala_block_max_aggregate_csr(int device, const int64_t* indptr, const int32_t* indices, const float* h_src, float* out, int32_t* arg,
                                  int64_t n_dst, int dim, void* stream);
int coala_block_max_aggregate_backward(int device, const int32_t* arg, const float* grad_out, float* grad_src, int64_t n_dst, int dim,
                                       void* stream);
/* Relation-typed sum (the message step of DGL's RelGraphConv, before its weights): out[d, r, :] = sum over the valid j of row d with
 * etype[d, j] == r of w[d, j] * h_src[nbr[d, j], :], so that out viewed as [n_dst, num_rels * dim] times W viewed as [num_rels * dim, o]
 * is sum_j w_j W[etype_j] h_src[s_j] in one GEMM.  etype int32, one value per neighbour slot, laid out like nbr ([n_dst, fanout]) or
 * like indices ([E]); w fp32 in the same layout, or NULL: every weight is 1; out fp32 [n_dst, num_rels, dim], written whole: a
 * relation absent from a row stores exact zeros, and so does a row without a valid entry.  A padding slot's etype and w are never used;
 * a valid slot whose type is outside [0, num_rels) contributes nothing and is never used as an index.  The sum of a relation runs in
 * slot order with one fma per term from +0, the weighted sum's arithmetic: on finite inputs out[:, r, :] has the bits of
 * coala_block_weighted_sum with w * [etype == r] (with num_rels == 1 and every type 0: with w), and both forms run the same code:
 * bit-identical on any row both can express.  Refused with COALA_EINVAL and nothing launched: fan-out outside 1..32, dim < 1,
 * n_dst < 0, num_rels outside 1..64 (a row's relations are kept as a 64-bit mask); n_dst == 0 launches nothing.
 * Backward, both gradients in one launch, either output may be NULL (not wanted); grad_out fp32 [n_dst, num_rels, dim]:
 *   grad_src[s_j, :] += w_j * grad_out[d, etype_j, :]        hardware float atomics: the caller zeroes grad_src, the order varies;
 *   grad_w[d, j] = <grad_out[d, etype_j, :], h_src[s_j, :]>   shaped like w, written whole, 0 on a padding slot and on a type out of
 *                                                            range; deterministic, the same bits in both forms, and with num_rels
 *                                                            == 1 those of coala_block_weighted_sum_backward.  h_src is read only
 *                                                            when grad_w is given.
 * Bytes per row of deg valid edges: forward reads deg * (4 dim + 12), plus 12 deg again per relation present when deg > 64, and writes
 * 4 dim num_rels; backward reads 12 deg + 4 dim deg (+ 8 dim deg for grad_w), adds 4 dim deg through atomics and writes 4 per slot. */
int coala_block_rel_sum(int device, const int32_t* nbr, const int32_t* etype, const float* w, const float* h_src, float* out, int64_t n_dst,
                        int fanout, int num_rels, int dim, void* stream);
int coala_block_rel_sum_backward(int device, const int32_t* nbr, const int32_t* etype, const float* w, const float* h_src, const float* grad_out,
                                 float* grad_src, float* grad_w, int64_t n_dst, int fanout, int num_rels, int dim, void* stream);
int coala_block_rel_sum_csr(int device, const int64_t* indptr, const int32_t* indices, const int32_t* etype, const float* w, const float* h_src,
                            float* out, int64_t n_dst, int num_rels, int dim, void* stream);
int coala_block_rel_sum_csr_backward(int device, const int64_t* indptr, const int32_t* indices, const int32_t* etype, const float* w,
                                     const float* h_src, const float* grad_out, float* grad_src, float* grad_w, int64_t n_dst, int num_rels,
                                     int dim, void* stream);
/* GAT attention aggregation (DGL GATConv's message step; its projections are dense and stay outside).  For dst d, head h and the
 * valid in-edges j of d with source s_j:
 *   z_j = el[s_j, h] + er[d, h];  e_j = leaky_relu(z_j, negative_slope);  a_j = exp(e_j - m) / sum_k exp(e_k - m), m = max_k e_k;
 *   out[d, h, :] = sum_j a_j feat[s_j, h, :].
 * el fp32 [n_src, heads], er fp32 [n_dst, heads], feat fp32 [n_src, heads, dim], out fp32 [n_dst, heads, dim], all contiguous;
 * heads 1..16, dim >= 1, heads * dim < 2^31.  A row without a valid edge gives exactly 0.
 * Saved state: lse fp32 [n_dst, heads] = m + log(sum_k exp(e_k - m)), the log-sum-exp of the row's scores (-inf for a row without a
 * valid edge); the backward recomputes p_j = exp(e_j - lse) from it and takes a_j = p_j / S, S = sum_k p_k of the row, summed in a fixed
 * order.  The p_j sum to 1 + O(u |lse|), lse being one fp32 word; divided by their own sum the a_j sum to 1 within a few u whatever
 * offset the row's scores share, so grad_feat adds up over the sources to grad_out and sum_j t_j stays at rounding level.  The same
 * holds for the GATv2, dot-product and relation-typed entries below (there per relation).  The leaky_relu product of a score is one
 * rounded product in both directions, so the backward's e_j is the forward's bit for bit.
 * Fixed form: nbr int32 [n_dst, fanout], -1 padded, fan-out 1..32.  CSR form: the edges of row d are indices[indptr[d] .. indptr[d+1])
 * (indptr int64 [n_dst + 1], indices int32), any degree: one wave takes a row 64 edges at a time with an online max and rescale.  The
 * forward is deterministic; a fixed row whose valid entries come first, in CSC order, gives the bits of the same CSR row (out, lse and
 * the backward's grad_er).
 * Backward, with g = grad_out [n_dst, heads, dim] and out / lse from the forward:
 *   t_j = a_j (<g[d, h, :], feat[s_j, h, :]> - <g[d, h, :], out[d, h, :]>) (z_j > 0 ? 1 : negative_slope);
 *   grad_feat[s_j, h, :] += a_j g[d, h, :];  grad_el[s_j, h] += t_j;  grad_er[d, h] = sum_j t_j.
 * grad_feat [n_src, heads, dim] and grad_el [n_src, heads] are accumulated with hardware float atomics: the caller zeroes them, and the
 * order of the additions varies.  grad_er [n_dst, heads] is written whole. */
int coala_block_gat_aggregate(int device, const int32_t* nbr, const float* el, const float* er, const float* feat, float* out, float* lse,
                              int64_t n_dst, int fanout, int heads, int dim, float negative_slope, void* stream);
int coala_block_gat_aggregate_backward(int device, const int32_t* nbr, const float* el, const float* er, const float* feat, const float* out,
                                       const float* lse, const float* grad_out, float* grad_feat, float* grad_el, float* grad_er, int64_t n_dst,
                                       int fanout, int heads, int dim, float negative_slope, void* stream);
int coala_block_gat_aggregate_csr(int device, const int64_t* indptr, const int32_t* indices, const float* el, const float* er, const float* feat,
                                  float* out, float* lse, int64_t n_dst, int heads, int dim, float negative_slope, void* stream);
int coala_block_gat_aggregate_csr_backward(int device, const int64_t* indptr, const int32_t* indices, const float* el, const float* er,
                                           const float* feat, const float* out, const float* lse, const float* grad_out, float* grad_feat,
                                           float* grad_el, float* grad_er, int64_t n_dst, int heads, int dim, float negative_slope, void* stream);
/* Relation-typed GAT attention aggregation (the message step of DGL's HeteroGraphConv over one GATConv per edge type, aggregate =
 * 'sum', on a homogenised block): GAT's rule with the softmax per (destination, relation) and the relations' results summed.  Every
 * neighbour slot carries `row`, the row of el / feat that its edge reads (int32, -1 on a padding slot; it stands where nbr / indices
 * stand in the other entries, and the caller guarantees 0 <= row < P), and `etype` (int32), both laid out like the block's index array:
 * [n_dst, fanout], or [E] beside indptr.  For dst d, head h, relation r and the slots j of d with row_j >= 0 and etype_j == r:
 *   z_j = el[row_j, h] + er[d, r, h];  e_j = leaky_relu(z_j, negative_slope);  a_j = exp(e_j - m) / sum_k exp(e_k - m) over those j;
 *   out[d, h, :] = sum_r sum_j a_j feat[row_j, h, :].
 * el fp32 [P, heads], feat fp32 [P, heads, dim], er fp32 [n_dst, num_rels, heads], out fp32 [n_dst, heads, dim], all contiguous.  A
 * relation absent from a row contributes nothing; a row without a valid edge gives exactly 0; a valid slot whose type is outside
 * [0, num_rels) contributes nothing, receives no gradient, and its type is only ever compared.  A padding slot's etype is not read.
 * Saved state: lse fp32 [n_dst, num_rels, heads], the log-sum-exp of the scores of (d, r), -inf where (d, r) has no edge.
 * Limits: heads 1..16, fan-out 1..32 or the CSR form (any degree, one wave takes a row 64 slots at a time), num_rels 1..64 and
 * num_rels * heads <= 256 (a wave keeps two floats per (relation, head) on chip), dim >= 1, heads * dim < 2^31.  Anything else is
 * refused with COALA_EINVAL ("bad block shape", "null buffer") and nothing is launched; n_dst == 0 launches nothing and reads no pointer.
 * out and lse are deterministic, and both forms run the same code: bit-identical on a row both can express (a fixed row whose valid
 * entries come first).
 * Backward, with g = grad_out [n_dst, heads, dim], p_j = exp(e_j - lse[d, etype_j, h]), dot_j = <g[d, h, :], feat[row_j, h, :]>,
 * G[r, h] = sum of p_j dot_j, S[r, h] = sum of p_j over relation r's slots and a_j = p_j / S[etype_j, h] (S is 1 up to the rounding of
 * lse; dividing by it makes a group's a_j sum to 1 and its a_j (dot_j - G / S) sum to zero as the exact ones do):
 *   t_j = a_j (dot_j - G[etype_j, h] / S[etype_j, h]) (z_j > 0 ? 1 : negative_slope);
 *   grad_feat[row_j, h, :] += a_j g[d, h, :];  grad_el[row_j, h] += t_j;  grad_er[d, r, h] = sum of t_j over relation r's slots.
 * grad_feat [P, heads, dim] and grad_el [P, heads] are accumulated with hardware float atomics: the caller zeroes them, and the order
 * of the additions varies.  grad_er [n_dst, num_rels, heads] is written whole (0 where (d, r) has no edge), deterministic, the same
 * bits in both forms.  The forward's out is not needed.
 * Bytes per row of deg valid edges, hd = heads * dim: the forward reads deg * (4 hd + 8 + 4 heads) + 4 num_rels heads and writes
 * 4 hd + 4 num_rels heads; the backward reads deg * (4 hd + 8) + 4 hd + 8 num_rels heads, adds 4 hd deg through atomics and writes
 * 4 num_rels heads; a row of more than 64 slots reads its source rows twice in the backward (the second time from the cache). */
int coala_block_rel_gat_aggregate(int device, const int32_t* row, const int32_t* etype, const float* el, const float* er, const float* feat,
                                  float* out, float* lse, int64_t n_dst, int fanout, int num_rels, int heads, int dim, float negative_slope,
                                  void* stream);
int coala_block_rel_gat_aggregate_backward(int device, const int32_t* row, const int32_t* etype, const float* el, const float* er,
                                           const float* feat, const float* lse, const float* grad_out, float* grad_feat, float* grad_el,
                                           float* grad_er, int64_t n_dst, int fanout, int num_rels, int heads, int dim, float negative_slope,
                                           void* stream);
int coala_block_rel_gat_aggregate_csr(int device, const int64_t* indptr, const int32_t* row, const int32_t* etype, const float* el,
                                      const float* er, const float* feat, float* out, float* lse, int64_t n_dst, int num_rels, int heads, int dim,
                                      float negative_slope, void* stream);
int coala_block_rel_gat_aggregate_csr_backward(int device, const int64_t* indptr, const int32_t* row, const int32_t* etype, const float* el,
                                               const float* er, const float* feat, const float* lse, const float* grad_out, float* grad_feat,
                                               float* grad_el, float* grad_er, int64_t n_dst, int num_rels, int heads, int dim,
                                               float negative_slope, void* stream);
/* GATv2 attention aggregation (DGL GATv2Conv's message step; its projections are dense and stay outside).  The score does not split
 * into a per-source and a per-destination scalar: for dst d, head h and the valid in-edges j of d with source s_j,
 *   z_jc = feat_src[s_j, h, c] + feat_dst[d, h, c];  e_j = sum_c attn[h, c] * leaky_relu(z_jc, negative_slope);
 *   a_j = exp(e_j - m) / sum_k exp(e_k - m), m = max_k e_k;  out[d, h, :] = sum_j a_j feat_src[s_j, h, :].
 * feat_src fp32 [n_src, heads, dim], feat_dst fp32 [n_dst, heads, dim], attn fp32 [heads, dim], out fp32 [n_dst, heads, dim], all
 * contiguous; heads 1..16, dim >= 1, heads * dim < 2^31.  A row without a valid edge gives exactly 0.  lse fp32 [n_dst, heads] is the
 * log-sum-exp of the row's scores (-inf for a row without a valid edge), the state the backward needs besides out.
 * Fixed form: nbr int32 [n_dst, fanout], -1 padded, fan-out 1..32.  CSR form: the edges of row d are indices[indptr[d] .. indptr[d+1]),
 * any degree: one wave takes a row 64 edges at a time, GAT's online max and rescale.  Per chunk the scores are summed into on-chip
 * memory first, then the chunk's source rows are read a second time (from the cache) for the weighted sum: no buffer of a size
 * proportional to the number of edges exists.  The forward is deterministic, and a fixed row whose valid entries come first, in CSC
 * order, gives the bits of the same CSR row (out, lse and the backward's grad_dst).
 * Backward, with g = grad_out [n_dst, heads, dim], out / lse from the forward, a_j = exp(e_j - lse) / S from recomputed scores (S the
 * row's sum of exp(e_j - lse), as in the GAT entry; a row of more than 64 edges walks its scores once more for it),
 * t_j = a_j (<g[d, h, :], feat_src[s_j, h, :]> - <g[d, h, :], out[d, h, :]>) and k_jc = z_jc > 0 ? 1 : negative_slope:
 *   grad_src[s_j, h, c] += a_j g[d, h, c] + t_j attn[h, c] k_jc   hardware float atomics: the caller zeroes grad_src [n_src, heads, dim],
 *                                                                the order of the additions varies;
 *   grad_dst[d, h, c]    = sum_j t_j attn[h, c] k_jc              [n_dst, heads, dim], written whole, in slot order: deterministic;
 *   grad_attn[h, c]      = sum_d sum_j t_j leaky_relu(z_jc)        delivered as partial sums, without atomics.
 * Each of the three outputs may be NULL (not wanted: not computed); with all three NULL nothing is launched.
 * The grad_attn rule: grad_attn_parts is fp32 [parts, heads * dim], parts >= 1 chosen by the caller (for instance
 * min(ceil(n_dst / 4), 1024)).  The launch then has exactly `parts` blocks; block b sums the rows its waves take (row d belongs to
 * wave d mod the number of waves) in a fixed order and stores row b of the buffer whole, zeros if it took no row.  grad_attn is the
 * sum of the buffer over its first dimension, which the caller takes; the same parts gives the same bits, run after run.  A row of
 * heads * dim <= 1024 floats runs four waves a block, a longer one a single wave a block.
 * Refused with COALA_EINVAL and nothing launched: "bad block shape" (fan-out outside 1..32, heads outside 1..16, dim < 1, n_dst < 0,
 * parts < 1 with a partials buffer), "null buffer"; n_dst == 0 launches nothing and reads no pointer.
 * Bytes per row of deg valid edges, hd = heads * dim: the forward reads deg * (4 hd + 4) + 8 hd from memory (GAT's plus feat_dst and
 * attn; the second read of a source row is a cache hit) and writes 4 hd; the backward reads deg * (4 hd + 4) + 16 hd, adds 4 hd deg
 * through atomics and writes 4 hd. */
int coala_block_gatv2_aggregate(int device, const int32_t* nbr, const float* feat_src, const float* feat_dst, const float* attn, float* out,
                                float* lse, int64_t n_dst, int fanout, int heads, int dim, float negative_slope, void* stream);
int coala_block_gatv2_aggregate_backward(int device, const int32_t* nbr, const float* feat_src, const float* feat_dst, const float* attn,
                                         const float* out, const float* lse, const float* grad_out, float* grad_src, float* grad_dst,
                                         float* grad_attn_parts, int parts, int64_t n_dst, int fanout, int heads, int dim, float negative_slope,
                                         void* stream);
int coala_block_gatv2_aggregate_csr(int device, const int64_t* indptr, const int32_t* indices, const float* feat_src, const float* feat_dst,
                                    const float* attn, float* out, float* lse, int64_t n_dst, int heads, int dim, float negative_slope,
                                    void* stream);
int coala_block_gatv2_aggregate_csr_backward(int device, const int64_t* indptr, const int32_t* indices, const float* feat_src,
                                             const float* feat_dst, const float* attn, const float* out, const float* lse, const float* grad_out,
                                             float* grad_src, float* grad_dst, float* grad_attn_parts, int parts, int64_t n_dst, int heads,
                                             int dim, float negative_slope, void* stream);
/* Scaled dot-product attention aggregation (the message step of DGL's DotGatConv and HGTConv and of PyG's TransformerConv without edge
 * features; the projections are dense and stay outside).  Every neighbour slot carries the row of k / v its edge reads: row int32, -1
 * = no edge, laid out [n_dst, fanout] (fan-out 1..32) or, for the CSR form, along indptr (slot e of row d for indptr[d] <= e <
 * indptr[d+1], any degree).  A caller whose k / v have one row per source node passes the block's own index array.  For dst d, head h
 * and the slots j of d with row_j >= 0:
 *   e_j = scale * <q[d, h, :], k[row_j, h, :]>;  a_j = exp(e_j - m) / sum_i exp(e_i - m), m = max_i e_i;
 *   out[d, h, :] = sum_j a_j v[row_j, h, :];  lse[d, h] = m + log sum_i exp(e_i - m).
 * q fp32 [n_dst, heads, dim], k and v fp32 [P, heads, dim] (k == v allowed), out fp32 [n_dst, heads, dim], lse fp32 [n_dst, heads], all
 * contiguous; heads 1..16, dim >= 1, heads * dim < 2^31, P < 2^31.  A row index is never checked: every row_j >= 0 must be < P.  A row
 * without an edge gives out exactly 0 and lse -inf.  16-byte accesses when dim % 4 == 0 and v and out are 16-byte aligned, scalar ones
 * otherwise.  One wave takes a row 64 slots at a time, GAT's online max and rescale; per chunk the dot products are summed into on-chip
 * memory first, then the chunk's v rows are read for the weighted sum: no buffer of a size proportional to the number of edges exists.
 * Backward, with g = grad_out [n_dst, heads, dim], out / lse from the forward, a_j = exp(e_j - lse) / S from recomputed scores (S the
 * row's sum of exp(e_j - lse), as in the GAT entry; a row of more than 64 slots walks its scores once more for it) and
 * t_j = a_j (<g[d, h, :], v[row_j, h, :]> - <g[d, h, :], out[d, h, :]>).  The recomputed e_j is the forward's bit for bit: scale times the
 * finished dot product is one rounded product in both directions, never fused into the subtraction after it, so the a_j of a row sum to
 * what lse says and sum_j t_j stays at rounding level whatever offset the row's scores share:
 *   grad_v[row_j, h, :] += a_j g[d, h, :]              hardware float atomics: the caller zeroes grad_v [P, heads, dim], the order varies;
 *   grad_k[row_j, h, :] += scale t_j q[d, h, :]        the same, grad_k [P, heads, dim];
 *   grad_q[d, h, :]      = scale sum_j t_j k[row_j, h, :]   [n_dst, heads, dim], written whole, summed in slot order: no atomics.
 * Each of the three outputs may be NULL (not wanted: not computed); with all three NULL nothing is launched.
 * Determinism: out, lse and grad_q are bitwise reproducible, and a fixed row whose valid entries come first gives the bits of the same
 * CSR row; grad_k and grad_v depend on the order of the atomics.
 * Refused with COALA_EINVAL and nothing launched: "bad block shape" (fan-out outside 1..32, heads outside 1..16, dim < 1, n_dst < 0),
 * "null buffer"; n_dst == 0 launches nothing and reads no pointer.  The grid is capped as for the other block ops.
 * Bytes per row of deg edges, hd = heads * dim: the forward reads deg * (8 hd + 4) + 4 hd (k and v rows, the slot words, q) and writes
 * 4 hd + 4 heads; the backward reads deg * (8 hd + 4) + 12 hd (the second read of a k row is a cache hit), adds 8 hd deg through
 * atomics and writes 4 hd. */
int coala_block_dot_gat_aggregate(int device, const int32_t* row, const float* q, const float* k, const float* v, float* out, float* lse,
                                  int64_t n_dst, int fanout, int heads, int dim, float scale, void* stream);
int coala_block_dot_gat_aggregate_backward(int device, const int32_t* row, const float* q, const float* k, const float* v, const float* out,
                                           const float* lse, const float* grad_out, float* grad_q, float* grad_k, float* grad_v, int64_t n_dst,
                                           int fanout, int heads, int dim, float scale, void* stream);
int coala_block_dot_gat_aggregate_csr(int device, const int64_t* indptr, const int32_t* row, const float* q, const float* k, const float* v,
                                      float* out, float* lse, int64_t n_dst, int heads, int dim, float scale, void* stream);
int coala_block_dot_gat_aggregate_csr_backward(int device, const int64_t* indptr, const int32_t* row, const float* q, const float* k,
                                               const float* v, const float* out, const float* lse, const float* grad_out, float* grad_q,
                                               float* grad_k, float* grad_v, int64_t n_dst, int heads, int dim, float scale, void* stream);
/* Edge exclusion (link prediction: the seed edges, and their reverses, leave the message-flow blocks).  excluded: device int64
 * [n_excluded], SORTED ascending, CSC positions (a few thousand at most; every slot binary-searches its edge id in it).  eid is the
 * block's edge-id array (coala_sampler_sample_layers_edge_ids), laid out like its index array.
 *   fixed form: nbr int32 [n_dst, fanout], eid int64 [n_dst, fanout] -> nbr_out, eid_out of the same shapes (other buffers than the
 *     inputs): the valid slots whose id is not listed, in their old order at the front of the row, -1 in both arrays behind them.
 *   CSR form, two calls of one kernel with the row scan between them left to the caller: with new_indptr NULL the call writes
 *     counts_out int64[n_dst], the surviving edges of every row; with new_indptr int64[n_dst + 1] (the exclusive scan of those counts)
 *     it writes the survivors of row d to indices_out / eid_out from new_indptr[d] on, in their old order.
 * An id that is in no slot changes nothing.  One launch each; "bad block shape" / "null buffer" as for the other block ops. */
int coala_block_exclude_edges(int device, const int32_t* nbr, const int64_t* eid, const int64_t* excluded, int64_t n_excluded, int32_t* nbr_out,
                              int64_t* eid_out, int64_t n_dst, int fanout, void* stream);
int coala_block_exclude_edges_csr(int device, const int64_t* indptr, const int32_t* indices, const int64_t* eid, const int64_t* excluded,
                                  int64_t n_excluded, int64_t* counts_out, const int64_t* new_indptr, int32_t* indices_out, int64_t* eid_out,
                                  int64_t n_dst, void* stream);
/* Pair scores (DGL's fn.u_dot_v on a pair graph; the score of a link predictor): out[p, hd] = <h[src_p, hd, :], h[dst_p, hd, :]>,
 * h fp32 [N, heads, dim], src / dst int32 [n_pairs], out fp32 [n_pairs, heads].  A wave -- a group of 16 or 32 lanes for dim <= 16 /
 * 32 -- takes one (pair, head): two row reads, one fma per term and a butterfly sum, no [n_pairs, dim] intermediate; bitwise
 * reproducible.  A pair with an index < 0 scores 0 and gets no gradient; an index >= N is not checked here (the caller's duty).
 * Backward, one launch: grad_h[src_p, hd, :] += g[p, hd] h[dst_p, hd, :] and grad_h[dst_p, hd, :] += g[p, hd] h[src_p, hd, :] with
 * hardware float atomics (grad_h [N, heads, dim] zeroed by the caller; the order varies). */
int coala_block_pair_dot(int device, const float* h, const int32_t* src, const int32_t* dst, float* out, int64_t n_pairs, int heads, int dim,
                         void* stream);
int coala_block_pair_dot_backward(int device, const float* h, const int32_t* src, const int32_t* dst, const float* grad_out, float* grad_h,
                                  int64_t n_pairs, int heads, int dim, void* stream);
/* Skip-gram window loss of walk tables (PyG's Node2Vec.loss, with softplus for -log(sigmoid + 1e-15)).  rows int32 [R, L1], indices
 * into h fp32 [N, dim] (contiguous), -1 = no node; context C in 2..L1.  For every row r, window start a in 0 .. L1 - C and j in
 * 1 .. C - 1 the pair (a, a + j) scores s = <h[rows[r, a]], h[rows[r, a + j]]> when both indices are >= 0.  partial[r] = the sum
 * over the row's valid pairs of softplus(sign * s) (sign = -1: positive walks, +1: negatives), count[r] (int32) their number; the
 * caller adds them up.  One wave (a group of 16 or 32 lanes for dim <= 16 / 32) stages the row's L1 embedding rows in LDS once; a lane
 * then forms the dots of its own pairs from there and sums their losses in a double, and the group's sums are added in a fixed
 * butterfly: bitwise reproducible.  L1 * dim <= 16384 floats and L1 <= 128, COALA_EINVAL ("bad walk table shape") otherwise; R == 0
 * launches nothing.  An index >= N is not checked here (the caller's duty).
 * Backward: grad_acc is a DOUBLE buffer [N, dim], zeroed by the caller, and scale a DEVICE double (the upstream gradient over the
 * number of valid pairs: nothing waits for the host).  grad_acc[rows[r, t], :] += scale * sum over the pairs that hold position t of
 * sign * sigmoid(sign * s) * h[other]: the scores are recomputed from LDS (fp32, the group's lanes on one dot), their coefficients
 * kept in registers, each position's gradient row is summed over all its pairs in a double and added with ONE hardware double atomic
 * per (position, element), not one per pair.  The caller rounds grad_acc to fp32 once: the hundreds of additions a node of a batch
 * collects leave no fp32 rounding and no visible trace of their order. */
int coala_block_skipgram_loss(int device, const float* h, const int32_t* rows, float* partial, int32_t* count, int64_t n_rows, int len,
                              int context, int dim, float sign, void* stream);
int coala_block_skipgram_loss_backward(int device, const float* h, const int32_t* rows, double* grad_acc, const double* scale, int64_t n_rows,
                                       int len, int context, int dim, float sign, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Shared pinned-host ("UVA") region.  Replaces SharedUVAManager (COALA_GNN_Modules/shared_UVA.cuh:26-115):
 * creator shm_open+ftruncate, everybody mmap + hipHostRegister + hipHostGetDevicePointer.  The MPI barrier between
 * create and open (shared_UVA.cuh:76,79) is the caller's job (torch.distributed barrier): is_creator selects the role.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct coala_shm coala_shm_t;
int coala_shm_open(const char* name, uint64_t bytes, int is_creator, int device, coala_shm_t** out);
void* coala_shm_host_ptr(const coala_shm_t* s);   /* SharedUVAManager::get_host_ptr   */
void* coala_shm_device_ptr(const coala_shm_t* s); /* SharedUVAManager::get_device_ptr */
int coala_shm_close(coala_shm_t* s, int unlink);  /* SharedUVAManager::cleanup        */

/* Plain pinned host allocation visible to the device (private cold tier; hipHostMalloc mapped). */
int coala_pinned_alloc(uint64_t bytes, int device, void** host_ptr, void** device_ptr);
int coala_pinned_free(void* host_ptr);
/* "dddd:bb:dd.f" of HIP device `device` (hipDeviceGetPCIBusId; initialises the runtime).  The host side places a rank's threads
 * and its cold-tier shard on that GPU's NUMA node (COALA_GNN/numa.py reads /sys/bus/pci/devices/<id>/numa_node); the reference
 * leaves the placement of its one shared segment to chance (COALA_GNN_Modules/shared_UVA.cuh:60-100). */
int coala_device_pci_bus_id(int device, char* out, size_t cap);

/* ------------------------------------------------------------------------------------------------------------
 * .npy reader and node distributor.  Replace parse_numpy_file / load_file_to_memory
 * (COALA_GNN_Modules/node_distributor_pybind.cuh:11-109) and Node_distributor_pybind (:112-238).
 * ------------------------------------------------------------------------------------------------------------ */
/* Parse a .npy v1/v2 header in memory.  want_dim is 1 or 2 (the reference's regex choice); when the stored shape has a
 * different rank, *ndim_out is 0 and shape is untouched (the reference leaves its vector empty).  descr receives e.g. "<i8". */
int coala_npy_parse(const char* buf, size_t len, int want_dim, int64_t* shape, int* ndim_out, size_t* data_off,
                    char* descr, size_t descr_cap);

typedef struct coala_distributor coala_distributor_t;
/* Node_distributor_pybind(u64 items, int n_nodes)  (node_distributor_pybind.cuh:133-136) */
int coala_distributor_create_plain(const int64_t* items, int num_nodes, coala_distributor_t** out);
/* Node_distributor_pybind(u64 items, int node_id, int batch, int local_size, int n_nodes, color, topk, score) (:138-148) */
int coala_distributor_create(const int64_t* items, int node_id, int batch_size, int local_size, int num_nodes,
                             const char* color_file, const char* topk_file, const char* score_file,
                             coala_distributor_t** out);
int coala_distributor_destroy(coala_distributor_t* d);
int coala_distributor_num_colors(const coala_distributor_t* d);          /* get_num_colors (:224-226) */
const int64_t* coala_distributor_color_ptr(const coala_distributor_t* d); /* get_color_buffer_ptr (:228-231) */
int64_t coala_distributor_num_color_entries(const coala_distributor_t* d);
/* distribute_node_with_affinity(u64 offset, u64 out, list[u64] meta)  (:150-222).  meta[j] -> int32 counters of domain j,
 * indexed by colour (num_colors+1 entries).  out -> int64[batch_size*local_size].  Re-entrant per handle. */
int coala_distributor_assign(const coala_distributor_t* d, uint64_t offset, int64_t* out, const int32_t* const* meta,
                             int n_meta);

#ifdef __cplusplus
}
#endif
#endif /* COALA_HIP_H */
