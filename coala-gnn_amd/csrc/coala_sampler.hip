// coala_sampler.hip -- uniform multi-layer neighbour sampler + block compaction over a CSC graph, for gfx950.
//
// Replaces the third-party step of the hot path: dgl.dataloading.MultiLayerNeighborSampler(fanouts).sample(g, seeds) on a
// CSC graph (call site /root/reference/COALA-GNN-Setup/COALA_GNN/COALA_GNN_DataLoader.py:162, sampler built at
// examples/sbatch_ssd_gnn_train.py:70-72, graph at examples/ssd_gnn_dataloader.py:523).  The arithmetic of that step
// lives in DGL 2.5, which is not under /root/reference: parity is pinned by properties and by the CPU twin in
// oracle/coala_oracle.c (same counter-based RNG), not by DGL's RNG stream.
//
// Contract (per layer, fan-out f, destination nodes dst[0..n_dst)):
//   * node v with in-degree deg = indptr[v+1]-indptr[v]: all in-neighbours when deg <= f, otherwise f distinct positions
//     drawn by Floyd's algorithm with r(j) = splitmix64(key(seed, step, layer, v) + j), t = mulhi64(r, j+1);
//   * source nodes of the block = dst nodes first (in order), then every other sampled neighbour in order of FIRST
//     APPEARANCE in the row-major (d, j) scan -- made deterministic with an atomicMin on the first position + prefix sum,
//     whatever order the hash-table inserts land in;
//   * nbr_local[d*f + j] = index of the j-th sampled neighbour of dst d inside the source list, or -1.
//
// Full layers (fan-out -1, DGL's "every in-edge"; coala_sampler_sample_layers):
//   * dst d (node v) gets every in-edge indices[indptr[v] .. indptr[v+1]) in CSC order, repeated edges and self-loops kept, an
//     empty segment for degree 0 (what a fixed layer returns when deg <= f);
//   * source nodes: the same rule -- dst nodes first, then every other neighbour in order of first appearance in the row-major
//     (d, edge) scan;
//   * block in CSR form: indptr_local int64[n_dst + 1] = exclusive scan of the degrees, nbr_local int32[E] = local source index of
//     each edge;
//   * no randomness is drawn; fixed layers of the same list keep their layer index l as the RNG key;
//   * limit: n_dst + E <= kMaxTiles * kTile items (8,388,608), n_dst + E <= src_cap and E <= edge_cap.  Only the device knows E,
//     so the check is made there: a refused layer reports 0 items, every later kernel of the call sees empty layers and does
//     nothing, and coala_sampler_wait_layers returns the error with the layer and its item count.  Fixed layers behind a full
//     layer have a device-known destination count; their worst-case bound n_dst * (f + 1) is checked on the device by the full
//     layer's scan_assign in the same way.  Nothing is written past the caller's capacities; the handle stays usable.
//   Launches: degree_scan (degrees -> indptr_local and E: tile_scan, the single-pass tile-ticket scan of scan_assign, on the same
//   status words; publish_ragged_layer makes the check), full_insert (one thread per item position p < n_dst + E: a binary search in indptr_local finds the destination, so a
//   hub of 10^6 in-edges is spread over the whole grid), then scan_assign / relabel_clear in their full-layer instantiations.
//   The hash table of a full layer is sized by its device-known item count: the kernel in front of the layer (the previous layer's
//   relabel_clear, run after this layer's degree_scan, or table_clear for a first layer) clears exactly that much.
//
// Weighted fixed layers (DGL's NeighborSampler(fanouts, prob=...); coala_sampler_sample_layers_weighted), fan-out f in 1..32.
// Destination node v's in-edges sit at CSC positions indptr[v] + j, 0 <= j < deg, with fp32 weights w[indptr[v] + j] (finite,
// >= 0, CSC order, validated by the caller):
//   * P = number of edges with w > 0.  P <= f: the row takes exactly those P edges (DGL's rule for replace=False);
//   * otherwise f distinct positive-weight edges, by weighted sampling without replacement with Efraimidis-Spirakis keys, in fp64:
//       r_j = splitmix64((sample_key(seed, step, layer, v) ^ kWeightedStream) + j),  u_j = (r_j >> 11) * 2^-53,
//       E_j = -log1p(-u_j)  (Exp(1)),  key_j = E_j / (double)w_j;
//     the f smallest (key_j, j) pairs win, a tie going to the lower position.  A weight-0 edge is never a candidate, whatever the
//     key of a positive edge (a key may be +inf without an edge of weight 0 ever overtaking it).  E_j depends on (seed, step,
//     layer, v, j) only: not on the batch, the grid or the order in which waves run.  (A 24-bit fp32 uniform would quantise the
//     smallest exponentials of a 10^6-edge row to ~6 % and bias ties toward low positions: hence 53 bits and fp64.)
//   * the chosen edges are written in ascending CSC position, valid entries first, then -1: a row with every weight positive and
//     deg <= f is the uniform path's row, bit for bit.  Source list, first appearance, item limit, refusal and bucketing are those of
//     a uniform fixed layer; an out-of-range destination id gives an empty row.
//   * full layers (-1) of a weighted list keep every in-edge and read no weights.
//   Launches: weighted_select<GS> replaces sample_insert (GS lanes per row stream the row in GS-edge chunks, keep the running
//   best f spread over the lanes, and pay for a shuffle merge only when a chunk holds a key below the f-th best); a row of more
//   than kHubDegree in-edges goes on a per-layer device list instead (atomic counter; capacity num_edges / (kHubDegree + 1), sized
//   at create time -- a row that finds the list full is scanned in place), and weighted_select_hub runs each listed row on a block
//   of 16 waves, merging their best-f lists in LDS.  Then scan_assign / relabel_clear / bucketing run unchanged.
//
// LABOR layers (DGL's LaborSampler(fanouts, importance_sampling=0), Balin & Catalyurek, NeurIPS 2023; coala_sampler_sample_layers_labor),
// fan-out k in 1..32.  One random number per SOURCE node, shared by every destination node of the layer: destination nodes with a
// common neighbour agree on taking it, so the source list shrinks while a row still holds k neighbours in expectation.
//   * labor_key(seed, step, layer) = splitmix64(splitmix64(seed ^ 0x9E3779B97F4A7C15 * (layer + 1)) ^ step * 0xD1B54A32D192ED03)
//     ^ kLaborStream: the two outer rounds of sample_key and a stream constant of its own, so a LABOR layer never replays the draws
//     of a uniform or weighted layer.  With layer_dependency the layer index is dropped (the first round hashes `seed` alone): every
//     layer of the call then sees the same r_t;
//   * r_t = splitmix64(labor_key ^ (uint64)t) for source node t;
//   * destination node v with in-degree deg: deg <= k takes every in-edge (the uniform path's rule); otherwise the in-edge at CSC
//     position e = indptr[v] + j with t = indices[e] is taken iff mulhi64(r_t, (uint64)deg) < k -- probability ceil(k 2^64 / deg) /
//     2^64, exact integer arithmetic; repeated edges t -> v are taken or left together; r_t depends on neither v nor j;
//   * the block is ragged, as a full layer's: taken edges in ascending CSC position inside a row, rows in destination order,
//     indptr_local int64[n_dst + 1], nbr_local int32[E]; source list, first appearance, item limit (n_dst + E, E known on the device
//     only), refusal and bucketing are those of a full layer; an out-of-range destination id gives an empty row; a -1 layer of a
//     LABOR list is the full layer above.
//   Launches: labor_count_scan stands where degree_scan stands (a lane group per row counts its taken edges with ballots, a row of
//   more than kHubDegree in-edges is counted by the whole block; then degree_scan's tile_scan and publish_ragged_layer: the same
//   capacity check and count words), labor_insert where full_insert stands (the same test again, survivors compacted to indptr_local[d] + rank by ballot
//   prefix, stored with their edge id when asked and hash-inserted; a hub row again on the whole block), then scan_assign /
//   relabel_clear in their full-layer instantiations and the bucketing kernels, unchanged.  No launch, memset or host wait is added.
//
// Relation layers (DGL's NeighborSampler on a heterograph: a fan-out per edge type; on a homogenised graph dgl.sort_csc_by_tag +
// sample_etype_neighbors(etype_sorted=True); coala_sampler_sample_layers_rel).  The graph has num_rels relations (1..64) and an int32
// type per edge in CSC order, NON-DECREASING INSIDE EVERY ROW (the caller's duty; not verified here).  The in-edges of relation r of
// node v are then one segment [s_r, s_r + deg_r) of [indptr[v], indptr[v+1]): s_r is the lower bound of r among the row's types (s_0
// the row's start), s_r + deg_r the lower bound of r + 1.  A layer has one fan-out per relation, f_r in {-1, 0, 1..32}:
//   * f_r == 0: the relation contributes nothing;
//   * f_r == -1 or deg_r <= f_r: every edge of the segment is taken;
//   * otherwise f_r distinct positions of the segment, relative to s_r, by sample_insert_kernel's Floyd loop with deg := deg_r,
//     fanout := f_r and r(j) = splitmix64(sample_key(seed, step, layer, v) + 64 r + j), t = mulhi64(r(j), deg_r - f_r + j + 1): the
//     counters 64 r + j (j < 32) never collide between relations, and relation 0 replays the uniform sampler's draws;
//   * the block is ragged, as a LABOR layer's: taken edges of a row in ascending CSC position (hence grouped by relation), rows in
//     destination order, indptr_local int64[n_dst + 1], nbr_local int32[E], edge ids when asked; source list, first appearance, item
//     limit (checked on the device), refusal and bucketing are those of a full layer; an out-of-range destination id gives an empty
//     row.  A layer whose fan-outs are all -1 IS the full layer (it runs degree_scan / full_insert and reads no types); with one
//     relation and fan-out f a row holds the edges NeighborSampler([f]) draws at the same seed and step, in ascending order.
//   * types that are not sorted give rows that are not what the rule says, but nothing is read or written out of bounds: every
//     boundary is a position inside the row, a segment of negative length counts as empty, and both passes compute the same counts.
//   Launches: rel_count_scan stands where degree_scan / labor_count_scan stand (a lane group per row, lane r finds the end of
//   relation r by binary search over the types: a row is never walked, so there is no hub list; then the tile scan and
//   publish_ragged_layer of the other two), rel_insert where full_insert / labor_insert stand (the same boundaries again; per drawn
//   relation the Floyd draws with a lane per candidate and the picks sorted inside the group; a taken-whole segment copied in lane
//   strides, one of more than kHubDegree edges by the whole block), then scan_assign / relabel_clear in their full-layer
//   instantiations and the bucketing kernels, unchanged.  The fan-outs travel by value in the kernel arguments.
//
// Random-walk layers (DGL's dgl.sampling.RandomWalkNeighborSampler / PinSAGESampler on a homogeneous graph; coala_sampler_sample_layers_walk):
// a node's neighbours are the k nodes its short random walks visit most often, and the visit counts go to the model as edge weights.
// A layer has k = num_neighbors (the fan-out, 1..32), T = num_traversals (1..16), W = num_random_walks (1..64, W T <= 512) and a
// termination threshold thr = floor(termination_prob * 2^53), an integer the host computes (termination_prob in [0, 1): exact in fp64).
//   * keys: destination node v (a node of the graph) of sampled layer l has wkey = sample_key(seed, step, l, v) ^ kWalkStream,
//     kWalkStream = 0x3C6EF372FE94F82B: a stream of its own, so a walk layer never replays the draws of another layer kind;
//   * walk w (0 <= w < W) starts at u = v; hop h = 0 .. T-1, with c = 2 (16 w + h):
//       1. h >= 1 and (splitmix64(wkey + c) >> 11) < thr: the walk ends (the first hop is never terminated, as in DGL);
//       2. deg = indptr[u+1] - indptr[u]; deg == 0: the walk ends;
//       3. u = indices[indptr[u] + mulhi64(splitmix64(wkey + c + 1), deg)], and this visit of u is recorded.
//     A step follows an IN-edge, the direction every sampler here reads the CSC in; on a symmetric graph this is DGL's walk.  The
//     visits of v's walks depend on (seed, step, l, v) only: not on the batch, v's place in it, the grid or the order of the waves;
//   * selection: count(u) = recorded visits of u over the W walks (u == v counts like any other node, as in DGL).  The row takes the
//     min(k, distinct visited) nodes of largest count, a tie going to the smaller node id, written in that order, valid entries
//     first, then -1; the per-slot visit count is int32, 0 on padding.  An out-of-range destination id, or a node of in-degree 0,
//     gives an empty row.  A chosen neighbour is a node, not an edge of the graph: there are no edge ids;
//   * source list, first appearance, nbr_local, the item limit and its refusal, and owner bucketing are a uniform fixed layer's.
//   Launches: walk_select<GS> replaces sample_insert (GS lanes per row, GS >= max(W, k + 1): a lane per walk writes its visits to
//   fixed positions of an LDS array, the group counts them by all-pairs comparison and takes k rounds of arg-max on (count, -id));
//   a walk never scans a row, so there is no hub list and no ragged form.  scan_assign / relabel_clear / bucketing run unchanged:
//   three launches per layer, no memset, no host wait.  coala_sampler_random_walk stores the traces of the same walks (walk_trace).
//
// Second-order walks (node2vec, Grover & Leskovec, KDD 2016; DGL's dgl.sampling.node2vec_random_walk on a homogeneous graph;
// coala_sampler_node2vec_walk), walk_length L in 1..127, W = num_walks in 1..64, by rejection sampling in exact integer arithmetic:
//   * thresholds: with m = max(1/p, 1, 1/q) the host passes thr_return = int((1/p) / m * 2^32), thr_near = int(1 / m * 2^32) and
//     thr_far = int((1/q) / m * 2^32): three integers in [0, 2^32], the largest exactly 2^32;
//   * keys: wkey = sample_key(seed, step, 0, v) ^ kN2vStream (0x1F83D9ABFB41BD6B: a stream of its own, not random_walk's), and walk w
//     of start node v uses kw = splitmix64(wkey + w): a function of (seed, step, v, w) alone, not of the batch or the grid;
//   * hop h (0-based) at node cur, having come from prev: deg(cur) == 0 ends the walk.  Attempts a = 0, 1, .. use c = 2 (256 h + a):
//     the candidate is x = indices[indptr[cur] + mulhi64(splitmix64(kw + c), deg)].  At h = 0 attempt 0 is taken.  At h >= 1 the
//     candidate's class picks the threshold t: return if x == prev, near if x occurs in row prev (indices[indptr[prev] ..
//     indptr[prev + 1])), far otherwise; it is taken when (splitmix64(kw + c + 1) >> 32) < t.  The first taken attempt wins; if the
//     attempts 0..255 all fail, attempt 255's candidate is taken: no walk loops without a bound.  A taken x outside [0, N) ends the
//     walk; an ended walk is padded with -1, and an out-of-range start node gives a row of -1;
//   * the near test is a binary search: ROWS MUST BE SORTED ASCENDING BY SOURCE ID when thr_near != thr_far (the caller's duty:
//     COALA_GNN.sampler.sort_csc_by_src, checked once per graph by the Python wrapper); with thr_near == thr_far row prev is never read.
//   Launch: node2vec_trace, a group of 16 lanes per walk: the group evaluates sixteen attempts of a hop at once and the first accepting
//   lane of its ballot wins -- the same sequential rule, with the dependent loads indptr -> indices -> search of sixteen attempts in
//   flight.  At p = q = 1 attempt 0 always wins and nothing is searched.
// Skip-gram batches (PyG's Node2Vec.pos_sample / neg_sample; coala_sampler_walk_batch): the walks above from n start nodes, and for
//   every walk K = num_neg (0..16) negative rows: column 0 is the walk's start node, column t >= 1 the node
//   mulhi64(splitmix64((kw ^ 0x6A09E667F3BCC909) + 128 j + t), N) of negative j.  input_nodes = the distinct ids of the item list
//   [start nodes | traces row-major | the negatives' columns 1.. row-major] in order of first appearance, an item of an invalid start
//   node or behind a walk's end being no node; pos int32 [n W, L + 1] and neg int32 [n W K, L + 1] hold every entry's index in it,
//   -1 for no node.  Three launches as an edge batch: walk_items (walks, negatives, hash insert), the layers' scan_assign, and
//   walk_relabel_clear; no memset, copy or host wait.  Limit: n W (L + 1) (1 + K) <= 8,388,608.
//
// Temporal layers (PyG's NeighborLoader(time_attr=, temporal_strategy='uniform' | 'last'), GraphBolt's temporal_sample_neighbors, TGN's
// "most recent neighbours"; coala_sampler_sample_layers_temporal), fan-out f in 1..32.  The graph carries an int64 timestamp per edge in CSC
// order, NON-DECREASING INSIDE EVERY ROW (the caller's duty; not verified here).  A destination item of a layer is a pair (v, t): node v
// as of query time t (int64).
//   * pair code: the n_slots distinct query times of a call sit in slot_time[n_slots], ascending; they never multiply, since a neighbour
//     inherits the query time of the row that reached it.  The pair is the int64 code slot << node_bits | v, node_bits the bit length of
//     num_nodes (so the value num_nodes fits the node field and names no node); the host refuses node_bits + bit_length(n_slots - 1) > 62.
//     The kernel decodes a code and then checks it: a negative code, slot >= n_slots or v >= num_nodes give an empty row.  The
//     destination's own hash insert follows the uniform rule: a negative code is not inserted, any other is, decoded or not;
//   * eligible edges of (v, t): the prefix [indptr[v], indptr[v] + m) of the row, m = the number of the row's edges with ts < t (a lower
//     bound; with `inclusive` ts <= t, an upper bound, PyG's rule).  Strict: an edge simultaneous with the query or later is out;
//   * strategy uniform: m <= f takes the m eligible edges in CSC order, then -1; otherwise sample_insert_kernel's Floyd loop with deg := m,
//     r(j) = splitmix64(key + j), key = sample_key(seed, step, layer, v) ^ splitmix64((uint64)t ^ kTemporalStream), kTemporalStream =
//     0xBB67AE8584CAA73B, t_c = mulhi64(r(c), m - f + c + 1), duplicate resolution and slot order as there.  The draws depend on (seed,
//     step, layer, v, t) only: not on the slot index, the batch, the grid or the order of the waves;
//   * strategy last: the min(m, f) most recent eligible edges, positions m - min(m, f) .. m - 1 ascending, then -1; nothing is drawn;
//   * the item of a slot is the code (the row's slot) << node_bits | indices[e], its edge id e (emit_fixed_slot); an indices[e] outside the
//     graph (a broken CSC) leaves the slot empty.  Source list (of codes), first appearance, nbr_local, the item limit and its refusal are a
//     uniform fixed layer's on codes; the destination codes of a call must be distinct, as seed nodes must be.  No owner bucketing (the
//     owner of a code is not the owner of its node), no -1 layers, no weights.
//   Launches: temporal_select<GS> replaces sample_insert (GS lanes per row find m by a GS-ary search over the timestamps, one ballot per
//   step, about log_GS(deg) dependent loads: the row is never walked, so there is no hub list and no ragged form), then scan_assign /
//   relabel_clear unchanged, which treat a key as opaque: three launches per layer, no memset, no host wait.
//
// Edge ids (coala_sampler_sample_layers_edge_ids), added to the contract of every layer kind above: with edge_ids_out[l] non-null the
// kernel that reads a neighbour also stores where it read it, eid[slot] = indptr[v] + j (the edge's position in `indices`), int64,
// laid out like the layer's nbr_local ([n_dst, f] or [E]); -1 where the slot holds no neighbour.  It is one 8-byte vector store from
// the lane that holds the position (sample_insert, weighted_select, weighted_select_hub, full_insert), behind a wave-uniform test
// of the pointer: no launch, no pass and no draw is added, and a null pointer leaves the kernels' memory traffic as it was.  A refused
// layer runs over 0 items and so stores nothing.  Bucketing permutes source indices, not slots: the ids are the same with it.
//
// Three launches per layer, nothing else on the stream (round 1: five launches + a memset per layer, a D2H copy and a stream
// synchronisation per call):
//   sample_insert   draw + hash insert;
//   scan_assign     first-occurrence flags -> positions in ONE pass: tiles are handed out by an atomic ticket and chained with a
//                   decoupled look-back over generation-tagged status words (no clearing pass, no second kernel for the tile sums);
//   relabel_clear   neighbour -> local index, and the hash table of the NEXT layer (or of the next call) is cleared alongside.
// Layer l+1 reads its destination count from device memory; the counts also go straight into pinned host memory from the kernel
// that produces them, and the host collects them by waiting on an event behind the last kernel -- never on the stream.
// (Tried and dropped: the whole call as one persistent kernel with grid barriers.  Every barrier needs a device-scope fence, i.e.
// an L2 write-back + invalidate issued by every block; 9 barriers cost more than the 10 kernel boundaries they replaced: 0.186 ms
// against 0.107 ms per 5,5 call.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <type_traits>

#include "../../include/coala_hip.h"
#include "coala_internal.h"
#include "coala_partition.h"

#define fail coala_fail_
#define HIPCHK COALA_HIPCHK

namespace {

constexpr long long kEmpty = -1;
constexpr int kItems = 4;                   // items per thread in the scan phases
constexpr int kTile = kBlock * kItems;      // items per block tile
constexpr int kMaxTiles = 8192;             // tiles per layer (8.4 M items): status words of the single-pass scan
constexpr int kRing = 8;                    // calls whose counts may be outstanding at once
constexpr int64_t kItemLimit = (int64_t)kMaxTiles * kTile;
constexpr int kFull = -1;                   // fan-out of a full layer: every in-edge
// device count words of layer l, relative to its base counts_dev + l: [0] n_dst, [kItemsOff] items, [kEdgesOff] edges of a full
// layer (both 0 when it was refused); counts_dev[l + 1] is layer l's source count, counts_dev[kMaxLayers + 1 ..] the bucket bases
constexpr int kItemsOff = COALA_SAMPLER_MAX_LAYERS + 1 + kMaxParts;
constexpr int kEdgesOff = kItemsOff + COALA_SAMPLER_MAX_LAYERS + 1;
constexpr int kCountsWords = kEdgesOff + COALA_SAMPLER_MAX_LAYERS + 1;
// pinned host words of a call, relative to the slot + l: [0] n_src, [kPinEdges] E, [kPinRefused] the layer was refused,
// [kPinOver] the fixed layers behind it were refused; the bucket sizes follow at kPinParts
constexpr int kPinEdges = COALA_SAMPLER_MAX_LAYERS, kPinRefused = 2 * COALA_SAMPLER_MAX_LAYERS, kPinOver = 3 * COALA_SAMPLER_MAX_LAYERS;
constexpr int kPinParts = 4 * COALA_SAMPLER_MAX_LAYERS;

__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__host__ __device__ inline uint64_t sample_key(uint64_t seed, uint64_t step, int layer, uint64_t v) {
    uint64_t h = splitmix64(seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(layer + 1)));
    h = splitmix64(h ^ (step * 0xD1B54A32D192ED03ull));
    return splitmix64(h ^ v);
}

__device__ __forceinline__ uint32_t hash_slot(int64_t key, uint32_t mask) { return (uint32_t)splitmix64((uint64_t)key) & mask; }

__device__ __forceinline__ int64_t item_key(const int64_t* dst, const int64_t* nbr, int64_t n_dst, int64_t p) {
    return p < n_dst ? dst[p] : nbr[p - n_dst];
}

__host__ __device__ inline uint32_t table_size(int64_t n_items) { // power of two, at most half full
    uint32_t t = 1024;
    while ((int64_t)t < 2 * n_items) t <<= 1;
    return t;
}

struct Graph {
    const int64_t* indptr;
    const int64_t* indices;
    int64_t num_nodes;
};

struct Table {
    long long* keys;          // [table] hash keys
    uint32_t* minpos;         // [table] first position of the key in the (dst..., neighbours...) item list
    uint32_t* local_of_slot;  // [table] index of the key in the source list
};

__device__ __forceinline__ void clear_table(const Table& t, uint32_t tbl) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < tbl; i += gridDim.x * blockDim.x) {
        t.keys[i] = kEmpty;
        t.minpos[i] = 0xFFFFFFFFu;
    }
}

// Item p (key k) into the hash table: CAS on the key, then atomicMin of the first position; k < 0 (no neighbour) is not inserted.
__device__ __forceinline__ void hash_insert(const Table& tb, uint32_t mask, int64_t k, int64_t p, uint32_t* __restrict__ slot_of_item) {
    if (k < 0) {
        slot_of_item[p] = 0xFFFFFFFFu;
    } else {
        uint32_t s = hash_slot(k, mask);
        while (true) {
            const long long cur = tb.keys[s];
            if (cur == k) break;
            if (cur == kEmpty) {
                const long long old = atomicCAS((unsigned long long*)(tb.keys + s), (unsigned long long)kEmpty, (unsigned long long)k);
                if (old == kEmpty || old == k) break;
            }
            s = (s + 1) & mask;
        }
        atomicMin(tb.minpos + s, (uint32_t)p);
        slot_of_item[p] = s;
    }
}

__device__ __forceinline__ uint32_t sat_add(uint32_t a, uint32_t b) { // degree sums saturate: past 2^32 - 1 a layer is refused anyway
    const uint32_t c = a + b;
    return c < a ? 0xFFFFFFFFu : c;
}

// The layer's destination count: from device memory behind an earlier layer, by value for the first layer.
__device__ __forceinline__ int64_t layer_n_dst(const int64_t* __restrict__ n_dst_dev, int64_t n_dst_value) { return n_dst_dev ? *n_dst_dev : n_dst_value; }

// Row header of the kernels that put a lane group on a destination row: GS lanes of a wave per row, `gl` the lane inside its group,
// `gbase` the group's first lane, `gmask` the group's lanes in a ballot.
struct LaneGroup {
    int gl, gbase;
    uint64_t gmask;
};

template <int GS>
__device__ __forceinline__ LaneGroup lane_group(int lane) {
    const int gl = lane % GS, gbase = lane - gl;
    return {gl, gbase, (GS == 64) ? ~0ull : (((1ull << GS) - 1ull) << gbase)};
}

struct Row { // destination d of a layer: its node, whether that is a node of the graph, and its in-edges indices[start .. start + deg)
    int64_t v;
    bool ok;
    int64_t start, deg;
};

// d >= n_dst (a lane past the layer) gives v = -1; that and any id outside the graph give an empty row: the one statement of the
// contract's "an out-of-range destination id gives an empty row".
__device__ __forceinline__ Row dst_row(const Graph& g, const int64_t* __restrict__ dst, int64_t d, int64_t n_dst) {
    const int64_t v = d < n_dst ? dst[d] : -1;
    const bool ok = v >= 0 && v < g.num_nodes;
    const int64_t start = ok ? g.indptr[v] : 0;
    return {v, ok, start, ok ? g.indptr[v + 1] - start : 0};
}

// A row that an earlier pass put on a hub list: d < n_dst and the id is valid (its degree was read), so the loads are unconditional.
__device__ __forceinline__ Row listed_row(const Graph& g, const int64_t* __restrict__ dst, int64_t d) {
    const int64_t v = dst[d];
    const int64_t start = g.indptr[v];
    return {v, true, start, g.indptr[v + 1] - start};
}

// Slot q = d * fanout + c of a fixed layer takes neighbour nb, read at CSC position e (nb < 0: the slot is empty); eid is nullable.
// The slot's hash insert (item n_dst + q) stays with the caller: sample_insert_kernel shares that loop with the node's own insert.
__device__ __forceinline__ void emit_fixed_slot(int64_t* __restrict__ nbr, int64_t* __restrict__ eid, int64_t q, int64_t nb, int64_t e) {
    nbr[q] = nb;
    if (eid) eid[q] = nb >= 0 ? e : -1;
}

// Sample + insert, a lane per sampled neighbour: GS lanes (16/32/64 >= fanout+1) work on one destination node.  Lane c < fanout
// draws Floyd's c-th candidate on its own, the duplicate resolution walks c = 0..fanout-1 with one shuffle + one ballot per
// step (bit-identical to the sequential loop of the CPU twin), then every lane loads ITS neighbour and inserts it into the
// hash table; lane `fanout` inserts the destination node itself.
template <int GS>
__global__ __launch_bounds__(kBlock) void sample_insert_kernel(Graph g, const int64_t* __restrict__ dst, const int64_t* __restrict__ n_dst_dev,
                                                               int64_t n_dst_value /* used when n_dst_dev is null: the first layer */, int fanout, uint64_t seed, uint64_t step, int layer, int64_t* __restrict__ nbr,
                                                               Table tb, uint32_t* __restrict__ slot_of_item, int64_t* __restrict__ eid) {
    constexpr int GPW = 64 / GS; // groups per wave
    const int64_t n_dst = layer_n_dst(n_dst_dev, n_dst_value);
    const uint32_t mask = table_size(n_dst * (fanout + 1)) - 1;
    const int lane = threadIdx.x & 63;
    const auto [gl, gbase, gmask] = lane_group<GS>(lane);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t d0 = wave * GPW; d0 < n_dst; d0 += n_waves * GPW) { // wave-uniform trip count: ballots below need every lane
        const int64_t d = d0 + lane / GS;
        const bool active = d < n_dst;
        const auto [v, okv, start, deg] = dst_row(g, dst, d, n_dst);
        // candidate of lane c = gl (Floyd step j = deg - fanout + c)
        const uint64_t key = sample_key(seed, step, layer, (uint64_t)v);
        const int64_t jmine = deg - fanout + gl;
        const int64_t t = (deg > fanout && gl < fanout) ? (int64_t)__umul64hi(splitmix64(key + (uint64_t)gl), (uint64_t)(jmine + 1)) : -1;
        int64_t chosen = -2;
        for (int c = 0; c < fanout; ++c) {
            const int64_t tc = __shfl(t, gbase + c);
            const uint64_t dupm = __ballot(gl < c && chosen == tc) & gmask;
            if (gl == c) chosen = dupm ? (deg - fanout + c) : tc;
        }
        int64_t pick = -1;
        if (gl < fanout) pick = (deg <= fanout) ? (gl < deg ? (int64_t)gl : -1) : chosen;
        const int64_t nb = (okv && pick >= 0) ? g.indices[start + pick] : kEmpty;
        if (active && gl < fanout) {
            emit_fixed_slot(nbr, eid, d * fanout + gl, nb, start + pick);
        }
        // ---- hash insert: neighbours at positions n_dst + d*fanout + gl, the node itself at position d
        int64_t k = kEmpty;
        int64_t p = -1;
        if (active && gl < fanout) { k = nb; p = n_dst + d * fanout + gl; }
        else if (active && gl == fanout) { k = v; p = d; }
        if (p >= 0) hash_insert(tb, mask, k, p, slot_of_item);
    }
}

// ---------------------------------------------------------------------------------------------------------- temporal layers
constexpr uint64_t kTemporalStream = 0xBB67AE8584CAA73Bull; // hashed with the query time into sample_key: the temporal draws' own stream

struct Temporal {
    const int64_t* ts;        // [num_edges] edge timestamps in CSC order, non-decreasing inside every row
    const int64_t* slot_time; // [n_slots] the distinct query times of the call, ascending
    int64_t n_slots;
    int node_bits;            // a pair is the code slot << node_bits | node
    bool last, inclusive;     // strategy 'last'; ts <= t instead of ts < t
};

struct TimedRow { // destination item (v, t) of a temporal layer: Row's fields, and the row's time slot and query time
    int64_t code, v;
    bool ok;
    int64_t start, deg, slot, t;
};

// Decode, then check: d >= n_dst, a negative code, a slot >= n_slots or a node >= num_nodes give an empty row.
__device__ __forceinline__ TimedRow timed_row(const Graph& g, const Temporal& tp, const int64_t* __restrict__ dst, int64_t d, int64_t n_dst) {
    const int64_t code = d < n_dst ? dst[d] : -1;
    const int64_t slot = code >> tp.node_bits, v = code & ((1ll << tp.node_bits) - 1);
    const bool ok = code >= 0 && slot < tp.n_slots && v < g.num_nodes;
    const int64_t start = ok ? g.indptr[v] : 0;
    return {code, v, ok, start, ok ? g.indptr[v + 1] - start : 0, slot, ok ? tp.slot_time[slot] : 0};
}

// Temporal fixed layer, in place of sample_insert_kernel: GS lanes (16/32/64 >= fanout + 1) per destination pair (v, t).  The group
// finds m, the number of the row's edges with ts < t (<= t: inclusive), by a GS-ary search: the range [lo, hi) that holds the
// boundary is cut into GS chunks of `step` positions, lane i probes the last position of chunk i, and one ballot counts the chunks
// that lie wholly in front of the boundary -- a 10^6-edge row takes 4 steps at GS = 32, and the row is never walked.  Every probe is a
// position of the row and lo <= hi <= deg whatever the timestamps hold, so unsorted times give a wrong m, never a read out of
// bounds.  Then sample_insert_kernel's draw with deg := m (strategy last: the positions m - fanout + c, no draw), the same slots, the
// same items and positions; a neighbour goes into the table as the code of (neighbour, the row's slot).
template <int GS>
__global__ __launch_bounds__(kBlock) void temporal_select_kernel(Graph g, Temporal tp, const int64_t* __restrict__ dst, const int64_t* __restrict__ n_dst_dev,
                                                                 int64_t n_dst_value, int fanout, uint64_t seed, uint64_t step, int layer,
                                                                 int64_t* __restrict__ nbr, Table tb, uint32_t* __restrict__ slot_of_item,
                                                                 int64_t* __restrict__ eid) {
    constexpr int GPW = 64 / GS;
    const int64_t n_dst = layer_n_dst(n_dst_dev, n_dst_value);
    const uint32_t mask = table_size(n_dst * (fanout + 1)) - 1;
    const int lane = threadIdx.x & 63;
    const auto [gl, gbase, gmask] = lane_group<GS>(lane);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t d0 = wave * GPW; d0 < n_dst; d0 += n_waves * GPW) { // wave-uniform trip count: ballots below need every lane
        const int64_t d = d0 + lane / GS;
        const bool active = d < n_dst;
        const TimedRow row = timed_row(g, tp, dst, d, n_dst);
        const int64_t start = row.start, t = row.t;
        int64_t lo = 0, hi = row.deg; // positions < lo are eligible, positions >= hi are not
        while (__ballot(lo < hi)) {   // wave-uniform: a group that is done probes nothing and keeps lo == hi
            const int64_t chunk = (hi - lo + GS - 1) / GS;
            const int64_t first = lo + gl * chunk; // lane gl's chunk [first, first + chunk), cut off at hi
            bool in = false;
            if (first < hi) {
                const int64_t x = tp.ts[start + min(first + chunk, hi) - 1];
                in = tp.inclusive ? x <= t : x < t;
            }
            const int64_t k = __popcll(__ballot(in) & gmask); // chunks wholly eligible; chunk k holds the boundary
            if (lo < hi) {
                const int64_t nlo = min(lo + k * chunk, hi);
                hi = min(nlo + chunk - 1, hi);
                lo = nlo;
            }
        }
        const int64_t m = lo;
        // candidate of lane c = gl (Floyd step j = m - fanout + c), as sample_insert_kernel with deg := m
        const uint64_t key = sample_key(seed, step, layer, (uint64_t)row.v) ^ splitmix64((uint64_t)t ^ kTemporalStream);
        const bool draw = !tp.last && m > fanout;
        const int64_t jmine = m - fanout + gl;
        const int64_t tc0 = (draw && gl < fanout) ? (int64_t)__umul64hi(splitmix64(key + (uint64_t)gl), (uint64_t)(jmine + 1)) : -1;
        int64_t chosen = -2;
        if (__ballot(draw)) { // wave-uniform: strategy last draws nothing
            for (int c = 0; c < fanout; ++c) {
                const int64_t tc = __shfl(tc0, gbase + c);
                const uint64_t dupm = __ballot(gl < c && chosen == tc) & gmask;
                if (gl == c) chosen = dupm ? (m - fanout + c) : tc;
            }
        }
        int64_t pick = -1;
        if (gl < fanout) pick = (m <= fanout) ? (gl < m ? (int64_t)gl : -1) : (tp.last ? jmine : chosen);
        const int64_t u = (row.ok && pick >= 0) ? g.indices[start + pick] : kEmpty;
        // the slot's item is the code of (u, the row's slot); an id outside the graph (a broken CSC) has no code: the slot stays empty
        const int64_t nb = (u >= 0 && u < g.num_nodes) ? (row.slot << tp.node_bits) | u : kEmpty;
        if (active && gl < fanout) emit_fixed_slot(nbr, eid, d * fanout + gl, nb, start + pick);
        // ---- hash insert: the neighbours' codes at positions n_dst + d*fanout + gl, the destination's own code at position d
        int64_t k = kEmpty;
        int64_t p = -1;
        if (active && gl < fanout) { k = nb; p = n_dst + d * fanout + gl; }
        else if (active && gl == fanout) { k = row.code; p = d; }
        if (p >= 0) hash_insert(tb, mask, k, p, slot_of_item);
    }
}

// ---------------------------------------------------------------------------------------------------------- weighted layers
constexpr uint64_t kWeightedStream = 0x6A09E667F3BCC909ull; // xor on sample_key: the weighted draws' own stream
constexpr int64_t kHubDegree = 4096;                          // rows with more in-edges go to weighted_select_hub
constexpr int kHubBlock = 1024;
constexpr int kHubWaves = kHubBlock / 64;
constexpr int kHubGrid = 256;
constexpr unsigned long long kNoKey = ~0ull; // above every fp64 key (+inf included): a weight-0 edge, or an empty slot
constexpr int64_t kNoPos = INT64_MAX;

// Bits of key_j (non-negative fp64, so its bits order like its value), or kNoKey for a weight of 0.  The weight's sign and
// magnitude are read from its bits: a denormal weight counts as positive whatever the float mode.
__device__ __forceinline__ unsigned long long weighted_key(uint64_t wkey, int64_t j, float wj) {
    if ((int32_t)__float_as_uint(wj) <= 0) return kNoKey;
    const uint64_t r = splitmix64(wkey + (uint64_t)j);
    const double u = (double)(r >> 11) * 0x1.0p-53;
    return (unsigned long long)__double_as_longlong(-log1p(-u) / (double)wj);
}

__device__ __forceinline__ bool kp_less(unsigned long long ak, int64_t ap, unsigned long long bk, int64_t bp) {
    return ak < bk || (ak == bk && ap < bp);
}

// One compare-exchange of a bitonic network across lanes lane ^ m (inside a GS-lane group): keep the smaller pair or the larger.
__device__ __forceinline__ void bitonic_step(unsigned long long& k, int64_t& p, int m, bool take_min) {
    const unsigned long long ok = __shfl_xor(k, m);
    const int64_t op = __shfl_xor(p, m);
    if (take_min == kp_less(ok, op, k, p)) {
        k = ok;
        p = op;
    }
}

template <int GS>
__device__ __forceinline__ void group_sort(unsigned long long& k, int64_t& p, int gl) { // ascending over the group's lanes
    for (int s = 2; s <= GS; s <<= 1)
        for (int m = s >> 1; m > 0; m >>= 1) bitonic_step(k, p, m, ((gl & s) == 0) == ((gl & m) == 0));
}

// The group's running best list (lane i holds the i-th smallest (key, pos) seen) takes one candidate per lane.  Nothing happens
// unless some candidate is below the f-th best; otherwise the candidates are sorted, merged against the list reversed (the lower
// half of a bitonic merge) and the list is re-sorted.  Every lane of the group must call it.
template <int GS>
__device__ __forceinline__ void group_offer(unsigned long long& bk, int64_t& bp, unsigned long long ck, int64_t cp, int gl, int gbase,
                                            uint64_t gmask, int fanout) {
    const unsigned long long tk = __shfl(bk, gbase + fanout - 1);
    const int64_t tp = __shfl(bp, gbase + fanout - 1);
    if (!(__ballot(kp_less(ck, cp, tk, tp)) & gmask)) return;
    group_sort<GS>(ck, cp, gl);
    const unsigned long long rk = __shfl(ck, gbase + GS - 1 - gl);
    const int64_t rp = __shfl(cp, gbase + GS - 1 - gl);
    if (kp_less(rk, rp, bk, bp)) {
        bk = rk;
        bp = rp;
    }
    for (int m = GS >> 1; m > 0; m >>= 1) bitonic_step(bk, bp, m, (gl & m) == 0);
}

// Lanes gl < fanout of the group: the gl-th chosen position in ascending order, or -1.  The winners are the lanes < fanout of
// the best list that hold a key; they are sorted by position.
template <int GS>
__device__ __forceinline__ int64_t group_picks(unsigned long long bk, int64_t bp, int gl, int fanout) {
    unsigned long long pk = (gl < fanout && bk != kNoKey) ? (unsigned long long)bp : (unsigned long long)kNoPos;
    int64_t unused = 0;
    group_sort<GS>(pk, unused, gl);
    return (gl < fanout && pk != (unsigned long long)kNoPos) ? (int64_t)pk : -1;
}

// Weighted fixed layer, in place of sample_insert_kernel: GS lanes (16/32/64 >= fanout + 1) per destination node stream its row in
// GS-edge chunks through group_offer, then lanes < fanout write and insert the chosen neighbours in position order, and lane
// `fanout` inserts the node itself -- the items and positions of sample_insert_kernel.  A row of more than kHubDegree in-edges is put
// on the hub list for weighted_select_hub_kernel (its node is still inserted here); when the list is full the group scans it itself.
template <int GS>
__global__ __launch_bounds__(kBlock) void weighted_select_kernel(Graph g, const float* __restrict__ w, const int64_t* __restrict__ dst,
                                                                 const int64_t* __restrict__ n_dst_dev, int64_t n_dst_value, int fanout,
                                                                 uint64_t seed, uint64_t step, int layer, int64_t* __restrict__ nbr, Table tb,
                                                                 uint32_t* __restrict__ slot_of_item, int64_t* __restrict__ hubs,
                                                                 unsigned long long* __restrict__ n_hubs, int64_t hub_cap,
                                                                 int64_t* __restrict__ eid) {
    constexpr int GPW = 64 / GS;
    const int64_t n_dst = layer_n_dst(n_dst_dev, n_dst_value);
    const uint32_t mask = table_size(n_dst * (fanout + 1)) - 1;
    const int lane = threadIdx.x & 63;
    const auto [gl, gbase, gmask] = lane_group<GS>(lane);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t d0 = wave * GPW; d0 < n_dst; d0 += n_waves * GPW) { // wave-uniform; the row loop below is group-uniform
        const int64_t d = d0 + lane / GS;
        const bool active = d < n_dst;
        const auto [v, okv, start, deg] = dst_row(g, dst, d, n_dst);
        unsigned long long hs = kNoKey;
        if (gl == 0 && deg > kHubDegree) {
            hs = atomicAdd(n_hubs, 1ull);
            if (hs < (unsigned long long)hub_cap) hubs[hs] = d;
        }
        hs = __shfl(hs, gbase);
        if (hs >= (unsigned long long)hub_cap) { // not a listed hub: this group selects the row
            const uint64_t wkey = sample_key(seed, step, layer, (uint64_t)v) ^ kWeightedStream;
            unsigned long long bk = kNoKey;
            int64_t bp = kNoPos;
            for (int64_t c0 = 0; c0 < deg; c0 += GS) {
                const int64_t j = c0 + gl;
                const unsigned long long ck = j < deg ? weighted_key(wkey, j, w[start + j]) : kNoKey;
                group_offer<GS>(bk, bp, ck, ck == kNoKey ? kNoPos : j, gl, gbase, gmask, fanout);
            }
            const int64_t pick = group_picks<GS>(bk, bp, gl, fanout);
            const int64_t nb = pick >= 0 ? g.indices[start + pick] : kEmpty;
            if (active && gl < fanout) {
                emit_fixed_slot(nbr, eid, d * fanout + gl, nb, start + pick);
                hash_insert(tb, mask, nb, n_dst + d * fanout + gl, slot_of_item);
            }
        }
        if (active && gl == fanout) hash_insert(tb, mask, v, d, slot_of_item);
    }
}

// The rows weighted_select_kernel listed: one block of kHubWaves waves per row (grid-stride over the list, whose length is read
// here).  Wave q streams chunks q, q + kHubWaves, ... of the row through its own best list; the waves' best f go to LDS, wave 0
// merges them, sorts the winners by position, writes the row and inserts it.  An empty list ends every block at once.
__global__ __launch_bounds__(kHubBlock) void weighted_select_hub_kernel(Graph g, const float* __restrict__ w, const int64_t* __restrict__ dst,
                                                                        const int64_t* __restrict__ n_dst_dev, int64_t n_dst_value, int fanout,
                                                                        uint64_t seed, uint64_t step, int layer, int64_t* __restrict__ nbr,
                                                                        Table tb, uint32_t* __restrict__ slot_of_item,
                                                                        const int64_t* __restrict__ hubs,
                                                                        const unsigned long long* __restrict__ n_hubs, int64_t hub_cap,
                                                                        int64_t* __restrict__ eid) {
    __shared__ unsigned long long s_k[kHubWaves * 32];
    __shared__ int64_t s_p[kHubWaves * 32];
    const unsigned long long cnt = min(*n_hubs, (unsigned long long)hub_cap);
    if ((unsigned long long)blockIdx.x >= cnt) return;
    const int64_t n_dst = layer_n_dst(n_dst_dev, n_dst_value);
    const uint32_t mask = table_size(n_dst * (fanout + 1)) - 1;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    for (unsigned long long i = blockIdx.x; i < cnt; i += gridDim.x) { // block-uniform
        const int64_t d = hubs[i];
        const auto [v, listed, start, deg] = listed_row(g, dst, d); // more than kHubDegree in-edges
        const uint64_t wkey = sample_key(seed, step, layer, (uint64_t)v) ^ kWeightedStream;
        unsigned long long bk = kNoKey;
        int64_t bp = kNoPos;
        for (int64_t c0 = (int64_t)q * 64; c0 < deg; c0 += kHubWaves * 64) { // wave-uniform
            const int64_t j = c0 + lane;
            const unsigned long long ck = j < deg ? weighted_key(wkey, j, w[start + j]) : kNoKey;
            group_offer<64>(bk, bp, ck, ck == kNoKey ? kNoPos : j, lane, 0, ~0ull, fanout);
        }
        __syncthreads(); // wave 0 has read the previous row's lists
        if (lane < fanout) {
            s_k[q * 32 + lane] = bk;
            s_p[q * 32 + lane] = bp;
        }
        __syncthreads();
        if (q == 0) {
            const int others = (kHubWaves - 1) * fanout; // the lists of waves 1.., fanout entries each
            for (int e0 = 0; e0 < others; e0 += 64) {
                const int e = e0 + lane;
                const int at = e < others ? (1 + e / fanout) * 32 + e % fanout : 0;
                group_offer<64>(bk, bp, e < others ? s_k[at] : kNoKey, e < others ? s_p[at] : kNoPos, lane, 0, ~0ull, fanout);
            }
            const int64_t pick = group_picks<64>(bk, bp, lane, fanout);
            if (lane < fanout) {
                const int64_t nb = pick >= 0 ? g.indices[start + pick] : kEmpty;
                emit_fixed_slot(nbr, eid, d * fanout + lane, nb, start + pick);
                hash_insert(tb, mask, nb, n_dst + d * fanout + lane, slot_of_item);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- random-walk layers
constexpr uint64_t kWalkStream = 0x3C6EF372FE94F82Bull; // xor on sample_key: the walks' own stream
constexpr int kMaxWalkLength = 16, kMaxWalks = 64, kMaxVisits = 512;
constexpr uint64_t kWalkThresholdMax = 1ull << 53; // term_threshold = floor(p * 2^53), p < 1

struct WalkParams {
    int T, W;     // hops per walk, walks per node
    uint64_t thr; // a hop h >= 1 ends the walk when (draw >> 11) < thr
};

// Walk w of node v (a node of the graph): visit(h, u) for every hop h < T, u the node the hop reached or -1 once the walk has ended.
// The draws are counters 2 (16 w + h) (termination) and 2 (16 w + h) + 1 (the step) on wkey.  A neighbour id outside the graph (a
// broken CSC) ends the walk instead of being followed.
template <typename F>
__device__ __forceinline__ void random_walk(const Graph& g, uint64_t wkey, int64_t v, int w, const WalkParams& wp, F&& visit) {
    int64_t u = v;
    bool ended = false;
    for (int h = 0; h < wp.T; ++h) {
        const uint64_t c = 2ull * (uint64_t)(kMaxWalkLength * w + h);
        if (!ended && h >= 1 && (splitmix64(wkey + c) >> 11) < wp.thr) ended = true;
        if (!ended) {
            const int64_t start = g.indptr[u];
            const int64_t deg = g.indptr[u + 1] - start;
            if (deg <= 0) {
                ended = true;
            } else {
                u = g.indices[start + (int64_t)__umul64hi(splitmix64(wkey + c + 1), (uint64_t)deg)];
                if (u < 0 || u >= g.num_nodes) ended = true;
            }
        }
        visit(h, ended ? kEmpty : u);
    }
}

// Walk layer, in place of sample_insert_kernel: GS lanes (16/32/64 >= max(W, fanout + 1)) per destination node, RPB = kBlock / GS rows
// per block step.  Lane w < W runs walk w and stores its visits at vis[w T + h] of the group's LDS array (-1 once ended): fixed
// positions, no atomics.  Behind a barrier every lane counts, for its entries i = gl, gl + GS, ..., how often the node occurs among
// all W T entries; the entry that is the node's first occurrence keeps the count, the others 0.  Then `fanout` rounds of a group
// arg-max on (count, -id) over the entries still standing: round j's winner goes to lane j, and its owner retires it.  Lanes
// < fanout write and insert their slots, lane `fanout` inserts the node itself -- the items and positions of sample_insert_kernel.
// The row loop is block-uniform (barriers), the rounds and their shuffles run for every lane of the wave.
// Dynamic LDS: RPB * W T int64 visits, then RPB * W T int32 counts.
template <int GS>
__global__ __launch_bounds__(kBlock) void walk_select_kernel(Graph g, const int64_t* __restrict__ dst, const int64_t* __restrict__ n_dst_dev,
                                                             int64_t n_dst_value, int fanout, WalkParams wp, uint64_t seed, uint64_t step, int layer,
                                                             int64_t* __restrict__ nbr, int32_t* __restrict__ visit_counts, Table tb,
                                                             uint32_t* __restrict__ slot_of_item) {
    constexpr int RPB = kBlock / GS; // rows per block step
    extern __shared__ int64_t s_walk[];
    const int n_vis = wp.W * wp.T;
    const int grp = (int)threadIdx.x / GS;
    int64_t* const vis = s_walk + (size_t)grp * n_vis;
    int32_t* const cnt = reinterpret_cast<int32_t*>(s_walk + (size_t)RPB * n_vis) + (size_t)grp * n_vis;
    const int64_t n_dst = layer_n_dst(n_dst_dev, n_dst_value);
    const uint32_t mask = table_size(n_dst * (fanout + 1)) - 1;
    const int gl = (int)threadIdx.x % GS;
    for (int64_t d0 = (int64_t)blockIdx.x * RPB; d0 < n_dst; d0 += (int64_t)gridDim.x * RPB) { // block-uniform
        const int64_t d = d0 + grp;
        const bool active = d < n_dst;
        const Row row = dst_row(g, dst, d, n_dst);
        const int64_t v = row.v;
        if (gl < wp.W) {
            if (row.ok) {
                const uint64_t wkey = sample_key(seed, step, layer, (uint64_t)v) ^ kWalkStream;
                random_walk(g, wkey, v, gl, wp, [&](int h, int64_t u) { vis[gl * wp.T + h] = u; });
            } else {
                for (int h = 0; h < wp.T; ++h) vis[gl * wp.T + h] = kEmpty;
            }
        }
        __syncthreads();
        for (int i = gl; i < n_vis; i += GS) {
            const int64_t x = vis[i];
            int32_t c = 0;
            if (x >= 0) {
                bool first = true;
                for (int j = 0; j < n_vis; ++j) {
                    const bool same = vis[j] == x;
                    c += same ? 1 : 0;
                    first = first && !(same && j < i);
                }
                if (!first) c = 0;
            }
            cnt[i] = c;
        }
        // fanout rounds of arg-max on (count, -id); an entry of count 0 never wins
        int64_t my_id = kEmpty;
        int32_t my_cnt = 0;
        for (int r = 0; r < fanout; ++r) { // wave-uniform: fanout is a kernel argument
            int32_t bc = 0;
            int64_t bid = kEmpty;
            int bi = -1;
            for (int i = gl; i < n_vis; i += GS) {
                const int32_t c = cnt[i];
                const int64_t x = vis[i];
                if (c > bc || (c == bc && c > 0 && x < bid)) { bc = c; bid = x; bi = i; }
            }
            for (int m = GS >> 1; m > 0; m >>= 1) {
                const int32_t oc = __shfl_xor(bc, m);
                const int64_t oid = __shfl_xor(bid, m);
                const int oi = __shfl_xor(bi, m);
                if (oc > bc || (oc == bc && oc > 0 && oid < bid)) { bc = oc; bid = oid; bi = oi; }
            }
            if (bi >= 0 && bi % GS == gl) cnt[bi] = 0; // the owner retires the winner: only this lane reads cnt[bi]
            if (gl == r) { my_id = bc > 0 ? bid : kEmpty; my_cnt = bc; }
        }
        if (active && gl < fanout) {
            const int64_t q = d * fanout + gl;
            emit_fixed_slot(nbr, nullptr, q, my_id, 0);
            if (visit_counts) visit_counts[q] = my_cnt;
            hash_insert(tb, mask, my_id, n_dst + q, slot_of_item);
        } else if (active && gl == fanout) {
            hash_insert(tb, mask, v, d, slot_of_item);
        }
        __syncthreads(); // every lane has read vis before the next step's walks overwrite it
    }
}

// coala_sampler_random_walk: one thread per (start node, walk); traces[i, w, 0] is the start node, then the hops, -1 once ended.
__global__ __launch_bounds__(kBlock) void walk_trace_kernel(Graph g, const int64_t* __restrict__ nodes, int64_t n, WalkParams wp, uint64_t seed,
                                                            uint64_t step, int layer, int64_t* __restrict__ traces) {
    const int64_t total = n * wp.W;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t / wp.W;
        const int w = (int)(t % wp.W);
        const int64_t v = nodes[i];
        int64_t* const row = traces + t * (wp.T + 1);
        if (v >= 0 && v < g.num_nodes) {
            row[0] = v;
            random_walk(g, sample_key(seed, step, layer, (uint64_t)v) ^ kWalkStream, v, w, wp, [&](int h, int64_t u) { row[1 + h] = u; });
        } else {
            for (int h = 0; h <= wp.T; ++h) row[h] = kEmpty;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- second-order walks
// node2vec's biased walk (the rule is in the header of this file).  kN2vGroup lanes run one walk.  A hop is a chain of dependent
// loads -- indptr, the candidate, then a binary search in the row of `prev` -- so the group tries kN2vGroup attempts at once, lane gl
// the attempt 16 r + gl of round r, and the first accepting lane of the group's ballot wins: the sequential rule, with the loads of
// sixteen attempts in flight.  At h = 0, and whenever every threshold is 2^32 (p = q = 1), attempt 0 wins: every lane computes it and
// nothing is searched or shuffled.  The row of `prev` is kept as (start, degree) from the hop before, and it is searched only when the
// near and far thresholds differ.  Every loop is bounded: L hops of at most 16 rounds of at most 64 search steps.  The groups of a
// wave diverge (their walks end, and accept, at different times); a ballot is read through the group's own bits and a shuffle reads
// a lane of the own group, all of whose lanes run together.
constexpr uint64_t kN2vStream = 0x1F83D9ABFB41BD6Bull;    // xor on sample_key: the second-order walks' own stream
constexpr uint64_t kN2vNegStream = 0x6A09E667F3BCC909ull; // xor on a walk's key: its negatives
constexpr int kN2vMaxLength = 127, kN2vAttempts = 256, kN2vMaxNeg = 16, kN2vGroup = 16;
constexpr uint64_t kN2vOne = 1ull << 32; // a threshold that accepts every draw
static_assert(kN2vAttempts % kN2vGroup == 0 && 64 % kN2vGroup == 0 && kBlock % kN2vGroup == 0, "a walk's lanes lie in one wave");

struct N2vParams {
    int L, W;                         // hops per walk, walks per start node
    uint64_t thr_ret, thr_near, thr_far; // in [0, 2^32]: a candidate is taken when (draw >> 32) < its class's threshold
};

__device__ __forceinline__ uint64_t n2v_walk_key(uint64_t seed, uint64_t step, int64_t v, int w) {
    return splitmix64((sample_key(seed, step, 0, (uint64_t)v) ^ kN2vStream) + (uint64_t)w);
}

// Does x occur in indices[start .. start + deg), a row sorted ascending?
__device__ __forceinline__ bool row_has(const int64_t* __restrict__ indices, int64_t start, int64_t deg, int64_t x) {
    int64_t lo = 0, hi = deg; // the first entry >= x lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (indices[start + mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < deg && indices[start + lo] == x;
}

// The walk with key kw from v (a node of the graph), run by the kN2vGroup lanes of a group together: every lane follows the walk, and
// lane 0 calls visit(h, u) for every hop h < L, u the node reached or -1 once the walk has ended.
template <typename F>
__device__ __forceinline__ void node2vec_walk(const Graph& g, uint64_t kw, int64_t v, const N2vParams& np, F&& visit) {
    const int gl = (int)threadIdx.x % kN2vGroup, gbase = (int)(threadIdx.x & 63) - gl;
    const bool search = np.thr_near != np.thr_far;
    const bool open = np.thr_ret == kN2vOne && np.thr_near == kN2vOne && np.thr_far == kN2vOne; // attempt 0 is always taken
    int64_t cur = v, prev = -1, prev_start = 0, prev_deg = 0;
    bool ended = false;
    for (int h = 0; h < np.L; ++h) {
        if (!ended) { // group-uniform: every lane of the group holds the same walk
            const int64_t start = g.indptr[cur];
            const int64_t deg = g.indptr[cur + 1] - start;
            if (deg <= 0) {
                ended = true;
            } else {
                int64_t x = kEmpty;
                if (h == 0 || open) {
                    x = g.indices[start + (int64_t)__umul64hi(splitmix64(kw + 2ull * (uint64_t)(kN2vAttempts * h)), (uint64_t)deg)];
                } else {
                    bool found = false;
                    for (int r = 0; r < kN2vAttempts / kN2vGroup && !found; ++r) {
                        const uint64_t c = 2ull * (uint64_t)(kN2vAttempts * h + r * kN2vGroup + gl);
                        const int64_t cand = g.indices[start + (int64_t)__umul64hi(splitmix64(kw + c), (uint64_t)deg)];
                        uint64_t t = np.thr_near;
                        if (cand == prev) t = np.thr_ret;
                        else if (search) t = row_has(g.indices, prev_start, prev_deg, cand) ? np.thr_near : np.thr_far;
                        const bool take = (splitmix64(kw + c + 1) >> 32) < t;
                        const uint32_t mine = (uint32_t)(__ballot(take) >> gbase) & ((1u << kN2vGroup) - 1u);
                        found = mine != 0;
                        // the first taking attempt; none: the round's last attempt, which in the last round is attempt 255
                        x = __shfl(cand, gbase + (found ? __builtin_ctz(mine) : kN2vGroup - 1));
                    }
                }
                if (x < 0 || x >= g.num_nodes) {
                    ended = true;
                } else {
                    prev = cur; prev_start = start; prev_deg = deg;
                    cur = x;
                }
            }
        }
        if (gl == 0) visit(h, ended ? kEmpty : cur);
    }
}

// coala_sampler_node2vec_walk: a lane group per (start node, walk); traces[i, w, 0] is the start node, then the hops, -1 once ended.
__global__ __launch_bounds__(kBlock) void node2vec_trace_kernel(Graph g, const int64_t* __restrict__ nodes, int64_t n, N2vParams np, uint64_t seed,
                                                                uint64_t step, int64_t* __restrict__ traces) {
    const int64_t total = n * np.W;
    const int gl = (int)threadIdx.x % kN2vGroup;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kN2vGroup; t < total; t += (int64_t)gridDim.x * blockDim.x / kN2vGroup) {
        const int64_t v = nodes[t / np.W];
        int64_t* const row = traces + t * (np.L + 1);
        if (v >= 0 && v < g.num_nodes) {
            if (gl == 0) row[0] = v;
            node2vec_walk(g, n2v_walk_key(seed, step, v, (int)(t % np.W)), v, np, [&](int h, int64_t u) { row[1 + h] = u; });
        } else {
            for (int h = gl; h <= np.L; h += kN2vGroup) row[h] = kEmpty;
        }
    }
}

// Skip-gram batches (coala_sampler_walk_batch).  The item list is [start nodes (n) | traces row-major (n W (L + 1)) | the negatives'
// columns 1..L row-major (n W K L)]; an item of an invalid start node is -1.  One launch makes the items and inserts them: a lane
// group per walk first, then a thread per negative entry.  traces (nullable) receives the global-id traces of node2vec_trace_kernel.
__host__ __device__ inline int64_t walk_batch_items(int64_t n, int W, int L, int K) { return n + n * W * (L + 1) + n * W * K * L; }

__global__ __launch_bounds__(kBlock) void walk_items_kernel(Graph g, const int64_t* __restrict__ nodes, int64_t n, N2vParams np, int K, uint64_t seed,
                                                            uint64_t step, int64_t* __restrict__ items, int64_t* __restrict__ traces, Table tb,
                                                            uint32_t* __restrict__ slot_of_item, unsigned long long* __restrict__ n_bad) {
    const int L = np.L, W = np.W;
    const int64_t n_walks = n * W, n_neg = n_walks * K * L;
    const int64_t pos0 = n, neg0 = n + n_walks * (L + 1);
    const uint32_t mask = table_size(walk_batch_items(n, W, L, K)) - 1;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n_thr = (int64_t)gridDim.x * blockDim.x;
    const int gl = (int)threadIdx.x % kN2vGroup;
    auto emit = [&](int64_t p, int64_t key) {
        items[p] = key;
        hash_insert(tb, mask, key, p, slot_of_item);
    };
    for (int64_t t = tid / kN2vGroup; t < n_walks; t += n_thr / kN2vGroup) {
        const int64_t i = t / W;
        const int w = (int)(t % W);
        const int64_t v = nodes[i];
        const bool ok = v >= 0 && v < g.num_nodes;
        const int64_t base = pos0 + t * (L + 1);
        int64_t* const row = traces ? traces + t * (L + 1) : nullptr;
        if (gl == 0) {
            if (w == 0) {
                emit(i, ok ? v : kEmpty);
                if (!ok) atomicAdd(n_bad, 1ull);
            }
            emit(base, ok ? v : kEmpty);
            if (row) row[0] = ok ? v : kEmpty;
        }
        if (ok) {
            node2vec_walk(g, n2v_walk_key(seed, step, v, w), v, np, [&](int h, int64_t u) {
                emit(base + 1 + h, u);
                if (row) row[1 + h] = u;
            });
        } else {
            for (int h = gl; h < L; h += kN2vGroup) {
                emit(base + 1 + h, kEmpty);
                if (row) row[1 + h] = kEmpty;
            }
        }
    }
    for (int64_t q = tid; q < n_neg; q += n_thr) { // entry (walk t, negative j, column c + 1)
        const int c = (int)(q % L);
        const int j = (int)((q / L) % K);
        const int64_t t = q / ((int64_t)L * K);
        const int64_t v = nodes[t / W];
        int64_t key = kEmpty;
        if (v >= 0 && v < g.num_nodes)
            key = (int64_t)__umul64hi(splitmix64((n2v_walk_key(seed, step, v, (int)(t % W)) ^ kN2vNegStream) + (uint64_t)(128 * j + c + 1)),
                                      (uint64_t)g.num_nodes);
        emit(neg0 + q, key);
    }
}

// item -> index in input_nodes (-1: no node); column 0 of a negative row is its walk's start node, the item of that node.  The table
// is cleared for the next call alongside, and the bad-start count goes to the host and back to 0.
__global__ __launch_bounds__(kBlock) void walk_relabel_clear_kernel(int64_t n, int W, int L, int K, const uint32_t* __restrict__ slot_of_item, Table tb,
                                                                    int32_t* __restrict__ pos, int32_t* __restrict__ neg,
                                                                    unsigned long long* __restrict__ n_bad, int64_t* __restrict__ n_bad_host,
                                                                    int64_t next_items) {
    const int64_t n_pos = n * W * (L + 1), n_neg_out = n * W * K * (L + 1);
    auto local = [&](int64_t p) {
        const uint32_t s = slot_of_item[p];
        return (s == 0xFFFFFFFFu) ? -1 : (int32_t)tb.local_of_slot[s];
    };
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_pos + n_neg_out; q += (int64_t)gridDim.x * blockDim.x) {
        if (q < n_pos) {
            pos[q] = local(n + q);
        } else {
            const int64_t r = q - n_pos;
            const int c = (int)(r % (L + 1));
            const int64_t row = r / (L + 1); // (walk t, negative j) = (row / K, row % K)
            neg[r] = c == 0 ? local(row / K / W) : local(n + n_pos + row * L + (c - 1));
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *n_bad_host = (int64_t)*n_bad;
        *n_bad = 0;
    }
    clear_table(tb, table_size(next_items));
}

// ---------------------------------------------------------------------------------------------------------- single-pass tile scan
// Single-pass scan over the tiles of a layer (degree_scan_kernel, labor_count_scan_kernel, scan_assign_kernel): a block takes the
// next tile with an atomic ticket (so every predecessor of its tile has already started), publishes the tile's count as an
// AGGREGATE, looks back over its predecessors until it meets an INCLUSIVE prefix and publishes its own INCLUSIVE prefix.  Status
// words carry the launch's generation: nothing to reset, and every scan of a handle shares the one ticket and the one status array.
//   word = gen << 34 | status << 32 | value          status: 1 = aggregate, 2 = inclusive prefix
// This is the only place where blocks wait on each other: relaxed agent-scope atomics on the status words, nothing else is ordered.
constexpr unsigned long long kAggregate = 1ull << 32, kInclusive = 2ull << 32;

struct TileScan {
    uint32_t excl;  // exclusive prefix of this thread's count over the whole layer
    uint32_t total; // inclusive total through this tile
    bool last;      // this block owns the layer's last tile
};

template <bool SAT> // degree sums saturate; first-occurrence counts stay below kItemLimit and add plainly
__device__ __forceinline__ uint32_t scan_add(uint32_t a, uint32_t b) {
    if constexpr (SAT) return sat_add(a, b);
    else return a + b;
}

// The block's tile: ticket order is start order.  Block-uniform; ends in a barrier.
__device__ __forceinline__ int64_t take_tile(unsigned long long* __restrict__ ticket, unsigned long long ticket_base) {
    __shared__ unsigned long long s_tile;
    if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1ull) - ticket_base;
    __syncthreads();
    return (int64_t)s_tile;
}

// Every thread of the block of `tile` (< n_tiles) calls it with its count c: wave inclusive scan, the waves combined through LDS,
// then thread 0 chains the tile to its predecessors.  Ends in a barrier.
template <bool SAT>
__device__ __forceinline__ TileScan tile_scan(unsigned long long* __restrict__ status, unsigned long long gen, int64_t tile, int64_t n_tiles,
                                              uint32_t c) {
    __shared__ uint32_t s_woff[kWavesPerBlock];
    __shared__ uint32_t s_prefix;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t incl = c; // inclusive scan inside the wave
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off);
        if (lane >= off) incl = scan_add<SAT>(incl, v);
    }
    if (lane == 63) s_woff[w] = incl;
    __syncthreads();
    uint32_t wbase = 0, total = 0;
    for (int q = 0; q < kWavesPerBlock; ++q) {
        if (q < w) wbase = scan_add<SAT>(wbase, s_woff[q]);
        total = scan_add<SAT>(total, s_woff[q]);
    }
    if (threadIdx.x == 0) {
        const unsigned long long tag = gen << 34;
        uint32_t prefix = 0;
        if (tile > 0) {
            __hip_atomic_store(status + tile, tag | kAggregate | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int64_t t = tile - 1; t >= 0;) { // decoupled look-back
                const unsigned long long v = __hip_atomic_load(status + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((v >> 34) != gen || !(v & (kAggregate | kInclusive))) { __builtin_amdgcn_s_sleep(1); continue; } // not published yet
                prefix = scan_add<SAT>(prefix, (uint32_t)v);
                if (v & kInclusive) break;
                --t;
            }
        }
        __hip_atomic_store(status + tile, tag | kInclusive | scan_add<SAT>(prefix, total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_prefix = prefix;
    }
    __syncthreads();
    const uint32_t prefix = s_prefix;
    return {scan_add<SAT>(prefix, scan_add<SAT>(wbase, incl - c)), scan_add<SAT>(prefix, total), tile == n_tiles - 1};
}

// Last tile of a ragged layer (full or LABOR), one thread: the layer's totals and the capacity check.  A refused layer publishes 0
// items and 0 edges, so every later kernel of the call does nothing; coala_sampler_wait_layers builds its message from the pinned words.
__device__ __forceinline__ void publish_ragged_layer(int64_t n_dst, int64_t edges, bool first_layer, int64_t item_cap, int64_t edge_cap,
                                                     int64_t* __restrict__ indptr_local, int64_t* __restrict__ base, int64_t* __restrict__ pin) {
    const int64_t items = n_dst + edges;
    const bool ok = items <= item_cap && edges <= edge_cap;
    indptr_local[n_dst] = edges;
    if (first_layer) base[0] = n_dst;
    base[kItemsOff] = ok ? items : 0;
    base[kEdgesOff] = ok ? edges : 0;
    pin[kPinEdges] = edges;
    pin[kPinRefused] = ok ? 0 : 1;
}

// A tile of `rows` destination nodes (row0 ..) whose edge counts sit in LDS (s_cnt, complete behind a barrier): degree_scan_kernel's
// scan over them -> indptr_local and, from the last tile, the layer's totals.  The tail of labor_count_scan_kernel and rel_count_scan_kernel.
__device__ __forceinline__ void scan_row_counts(const uint32_t* s_cnt, int rows, int64_t row0, int64_t n_dst, int64_t tile, int64_t n_tiles,
                                                unsigned long long* __restrict__ status, unsigned long long gen, bool first_layer,
                                                int64_t item_cap, int64_t edge_cap, int64_t* __restrict__ indptr_local,
                                                int64_t* __restrict__ base, int64_t* __restrict__ pin) {
    const int at = (int)threadIdx.x * kItems;
    const int64_t first = row0 + at;
    uint32_t dg[kItems];
    uint32_t c = 0;
    for (int i = 0; i < kItems; ++i) {
        dg[i] = (at + i < rows && first + i < n_dst) ? s_cnt[at + i] : 0;
        c = sat_add(c, dg[i]);
    }
    const TileScan ts = tile_scan<true>(status, gen, tile, n_tiles, c);
    if (ts.last && threadIdx.x == 0) publish_ragged_layer(n_dst, (int64_t)ts.total, first_layer, item_cap, edge_cap, indptr_local, base, pin);
    uint32_t run = ts.excl;
    for (int i = 0; i < kItems; ++i) {
        if (at + i < rows && first + i < n_dst) indptr_local[first + i] = (int64_t)run;
        run = sat_add(run, dg[i]);
    }
}

// Full layer, pass 1: degrees of the destination nodes -> indptr_local (exclusive scan) and E, by tile_scan.  The block of the last
// tile checks the layer against its capacities and publishes n_dst (first layer), the item and edge counts (publish_ragged_layer).
__global__ __launch_bounds__(kBlock) void degree_scan_kernel(Graph g, const int64_t* __restrict__ dst, const int64_t* __restrict__ n_dst_dev,
                                                             int64_t n_dst_value, int64_t* __restrict__ base, unsigned long long* __restrict__ status,
                                                             unsigned long long* __restrict__ ticket, unsigned long long ticket_base,
                                                             unsigned long long gen, int64_t* __restrict__ indptr_local, int64_t item_cap,
                                                             int64_t edge_cap, int64_t* __restrict__ pin) {
    const int64_t n_dst = layer_n_dst(n_dst_dev, n_dst_value);
    const int64_t n_tiles = n_dst > 0 ? (n_dst + kTile - 1) / kTile : 1; // tile 0 always runs: it publishes an empty layer too
    const int64_t tile = take_tile(ticket, ticket_base);
    if (tile >= n_tiles) return;
    const int64_t first = tile * kTile + (int64_t)threadIdx.x * kItems;
    uint32_t dg[kItems];
    uint32_t c = 0;
    for (int i = 0; i < kItems; ++i) {
        const int64_t deg = dst_row(g, dst, first + i, n_dst).deg;
        dg[i] = deg > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)deg;
        c = sat_add(c, dg[i]);
    }
    const TileScan ts = tile_scan<true>(status, gen, tile, n_tiles, c);
    if (ts.last && threadIdx.x == 0) publish_ragged_layer(n_dst, (int64_t)ts.total, !n_dst_dev, item_cap, edge_cap, indptr_local, base, pin);
    uint32_t run = ts.excl;
    for (int i = 0; i < kItems; ++i) {
        if (first + i < n_dst) indptr_local[first + i] = (int64_t)run;
        run = sat_add(run, dg[i]);
    }
}

// Full layer, pass 2: item p < n_dst is destination node p; item n_dst + q is edge q of the layer, whose destination a binary
// search in indptr_local finds (load-balanced over edges: a hub's edges are spread over the whole grid).  The edge's neighbour is
// stored (scan_assign reads it back) and inserted exactly as sample_insert_kernel inserts its items; eid (nullable) takes its position.
__global__ __launch_bounds__(kBlock) void full_insert_kernel(Graph g, const int64_t* __restrict__ dst, const int64_t* __restrict__ base,
                                                             const int64_t* __restrict__ indptr_local, int64_t* __restrict__ nbr, Table tb,
                                                             uint32_t* __restrict__ slot_of_item, int64_t* __restrict__ eid) {
    const int64_t n_dst = base[0];
    const int64_t n_items = base[kItemsOff];
    const uint32_t mask = table_size(n_items) - 1;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_items; p += (int64_t)gridDim.x * blockDim.x) {
        int64_t k;
        if (p < n_dst) {
            k = dst[p];
        } else {
            const int64_t q = p - n_dst;
            int64_t lo = 0, hi = n_dst - 1; // the last d with indptr_local[d] <= q (q < E, so d < n_dst and deg(d) > 0)
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (indptr_local[mid] <= q) lo = mid;
                else hi = mid - 1;
            }
            const int64_t e = g.indptr[dst[lo]] + (q - indptr_local[lo]);
            k = g.indices[e];
            nbr[q] = k;
            if (eid) eid[q] = e;
        }
        hash_insert(tb, mask, k, p, slot_of_item);
    }
}

// ---------------------------------------------------------------------------------------------------------- LABOR layers
constexpr uint64_t kLaborStream = 0xBB67AE8584CAA73Bull; // xor on the two outer rounds of sample_key: the LABOR draws' own stream
constexpr int kLaborGroup = 16;                           // lanes per destination row
constexpr int kLaborHubList = 32;                         // hub rows a block defers per pass; one more is counted by its group

__host__ __device__ inline uint64_t labor_key(uint64_t seed, uint64_t step, int layer, bool layer_dependency) {
    uint64_t h = splitmix64(layer_dependency ? seed : seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(layer + 1)));
    h = splitmix64(h ^ (step * 0xD1B54A32D192ED03ull));
    return h ^ kLaborStream;
}

// The LABOR test of an in-edge from source node t into a row of deg in-edges.
__device__ __forceinline__ bool labor_take(uint64_t lkey, int64_t t, int64_t deg, int fanout) {
    return deg <= fanout || __umul64hi(splitmix64(lkey ^ (uint64_t)t), (uint64_t)deg) < (uint64_t)fanout;
}

// A hub row of deg in-edges done by the whole block: wave w takes the contiguous share [hub_share(deg, w), hub_share(deg, w + 1)),
// whole 64-edge steps except at the row's end.
__device__ __forceinline__ int64_t hub_share(int64_t deg, int w) {
    return min(deg, w * (((deg + kWavesPerBlock - 1) / kWavesPerBlock + 63) & ~63ll));
}

// Taken edges among positions [from, to) of a row, by one wave: the wave-uniform total (trip count and ballots are wave-uniform).
__device__ __forceinline__ uint32_t labor_wave_count(const Graph& g, uint64_t lkey, int64_t start, int64_t deg, int fanout, int64_t from,
                                                     int64_t to, int lane) {
    uint32_t n = 0;
    for (int64_t c0 = from; c0 < to; c0 += 64) {
        const int64_t j = c0 + lane;
        const bool take = j < to && labor_take(lkey, g.indices[start + j], deg, fanout);
        n += (uint32_t)__builtin_popcountll(__ballot(take));
    }
    return n;
}

// LABOR layer, pass 1, where degree_scan_kernel stands: the count of taken edges of every destination node -> indptr_local
// (exclusive scan) and E.  A tile is `rows` destination nodes (a power of two, 64 .. kTile, chosen by the host so that the layer's
// capacity fits kMaxTiles tiles: small tiles spread the edge reads of a small batch over many blocks).  kLaborGroup lanes count a
// row, 64 / kLaborGroup rows per wave step; a row of more than kHubDegree in-edges is put on the block's list and counted by all its
// waves afterwards.  Then the scan, the capacity check and the published words of degree_scan_kernel, over the counts in LDS.
__global__ __launch_bounds__(kBlock) void labor_count_scan_kernel(Graph g, const int64_t* __restrict__ dst, const int64_t* __restrict__ n_dst_dev,
                                                                  int64_t n_dst_value, int rows, int fanout, uint64_t lkey,
                                                                  int64_t* __restrict__ base, unsigned long long* __restrict__ status,
                                                                  unsigned long long* __restrict__ ticket, unsigned long long ticket_base,
                                                                  unsigned long long gen, int64_t* __restrict__ indptr_local, int64_t item_cap,
                                                                  int64_t edge_cap, int64_t* __restrict__ pin) {
    constexpr int GS = kLaborGroup, GPB = kBlock / GS;
    __shared__ uint32_t s_cnt[kTile];
    __shared__ int s_hub[kLaborHubList];
    __shared__ int s_nhub;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t n_dst = layer_n_dst(n_dst_dev, n_dst_value);
    const int64_t n_tiles = n_dst > 0 ? (n_dst + rows - 1) / rows : 1; // tile 0 always runs: it publishes an empty layer too
    const int64_t tile = take_tile(ticket, ticket_base);
    if (tile >= n_tiles) return;
    const int64_t row0 = tile * rows;
    // ---- counts of the tile's rows
    const auto [gl, gbase, gmask] = lane_group<GS>(lane);
    for (int r0 = 0; r0 < rows; r0 += GPB * kLaborHubList) { // block-uniform: the list holds the hubs of one stretch of rows
        if (threadIdx.x == 0) s_nhub = 0;
        __syncthreads();
        const int r_end = min(rows, r0 + GPB * kLaborHubList);
        for (int r = r0 + (int)threadIdx.x / GS; r < r_end; r += GPB) { // wave-uniform trip count: r0, r_end are multiples of GPB
            const Row row = dst_row(g, dst, row0 + r, n_dst);
            int64_t deg = row.deg; // 0 once the row is deferred
            int at = kLaborHubList;
            if (gl == 0 && deg > kHubDegree) at = atomicAdd(&s_nhub, 1);
            at = __shfl(at, gbase);
            if (at < kLaborHubList) { // deferred to the whole block; a row that finds the list full is counted here
                if (gl == 0) s_hub[at] = r;
                deg = 0;
            }
            uint32_t n = 0;
            int64_t longest = deg; // the wave's rows run in step
            for (int off = GS; off < 64; off <<= 1) longest = max(longest, __shfl_xor(longest, off));
            for (int64_t c0 = 0; c0 < longest; c0 += GS) {
                const int64_t j = c0 + gl;
                const bool take = j < deg && labor_take(lkey, g.indices[row.start + j], deg, fanout);
                n += (uint32_t)__builtin_popcountll(__ballot(take) & gmask);
            }
            if (gl == 0) s_cnt[r] = n; // a deferred row: 0 for now
        }
        __syncthreads();
        const int n_hub = min(s_nhub, kLaborHubList);
        for (int i = 0; i < n_hub; ++i) { // block-uniform: every wave counts its share of the row
            const int r = s_hub[i];
            const Row hub = listed_row(g, dst, row0 + r);
            const uint32_t n = labor_wave_count(g, lkey, hub.start, hub.deg, fanout, hub_share(hub.deg, w), hub_share(hub.deg, w + 1), lane);
            if (lane == 0 && n) atomicAdd(&s_cnt[r], n);
        }
        __syncthreads();
    }
    scan_row_counts(s_cnt, rows, row0, n_dst, tile, n_tiles, status, gen, !n_dst_dev, item_cap, edge_cap, indptr_local, base, pin);
}

// Edge at position j of row d passed the test (take) or not: the survivors of the lanes in `among` go to slots slot0 + rank, rank by
// ballot prefix; the neighbour is stored (scan_assign reads it back), its edge id when asked, and it is inserted at item position
// n_dst + slot.  Returns the number of survivors among the lanes.  Every lane of the wave must call it.
__device__ __forceinline__ uint32_t labor_emit(bool take, uint64_t among, int lane, int64_t t, int64_t e, int64_t slot0, int64_t n_dst,
                                               int64_t* __restrict__ nbr, int64_t* __restrict__ eid, const Table& tb, uint32_t mask,
                                               uint32_t* __restrict__ slot_of_item) {
    const uint64_t m = __ballot(take) & among;
    if (take) {
        const int64_t q = slot0 + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        nbr[q] = t;
        if (eid) eid[q] = e;
        hash_insert(tb, mask, t, n_dst + q, slot_of_item);
    }
    return (uint32_t)__builtin_popcountll(m);
}

// LABOR layer, pass 2, where full_insert_kernel stands: item p < n_dst is destination node p; item n_dst + q is taken edge q of the
// layer.  kLaborGroup lanes walk a row, evaluate the test again and compact the survivors into the row's segment of nbr, which starts
// at indptr_local[d]; a block takes kBlock / kLaborGroup rows per step, and the rows of more than kHubDegree in-edges among them are
// then done by the whole block: every wave counts its contiguous share, the shares are ranked through LDS, and a second walk emits.
// A refused layer (0 items) does nothing.
__global__ __launch_bounds__(kBlock) void labor_insert_kernel(Graph g, const int64_t* __restrict__ dst, const int64_t* __restrict__ base,
                                                              const int64_t* __restrict__ indptr_local, int fanout, uint64_t lkey,
                                                              int64_t* __restrict__ nbr, Table tb, uint32_t* __restrict__ slot_of_item,
                                                              int64_t* __restrict__ eid) {
    constexpr int GS = kLaborGroup, GPB = kBlock / GS;
    __shared__ int64_t s_hub[GPB];
    __shared__ int s_nhub;
    __shared__ uint32_t s_wcnt[kWavesPerBlock];
    const int64_t n_dst = base[0];
    const int64_t n_items = base[kItemsOff];
    if (n_items == 0) return;
    const uint32_t mask = table_size(n_items) - 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const auto [gl, gbase, gmask] = lane_group<GS>(lane);
    for (int64_t d0 = (int64_t)blockIdx.x * GPB; d0 < n_dst; d0 += (int64_t)gridDim.x * GPB) { // block-uniform
        if (threadIdx.x == 0) s_nhub = 0;
        __syncthreads();
        const int64_t d = d0 + (int)threadIdx.x / GS;
        const bool active = d < n_dst;
        const Row row = dst_row(g, dst, d, n_dst);
        int64_t deg = row.deg; // 0 once the row is deferred
        if (deg > kHubDegree) { // at most GPB of them: the list cannot fill up
            if (gl == 0) s_hub[atomicAdd(&s_nhub, 1)] = d;
            deg = 0;
        }
        if (active && gl == 0) hash_insert(tb, mask, row.v, d, slot_of_item);
        int64_t slot = deg > 0 ? indptr_local[d] : 0;
        int64_t longest = deg;
        for (int off = GS; off < 64; off <<= 1) longest = max(longest, __shfl_xor(longest, off));
        for (int64_t c0 = 0; c0 < longest; c0 += GS) { // wave-uniform
            const int64_t j = c0 + gl;
            const int64_t t = j < deg ? g.indices[row.start + j] : -1;
            const bool take = j < deg && labor_take(lkey, t, deg, fanout);
            slot += labor_emit(take, gmask, lane, t, row.start + j, slot, n_dst, nbr, eid, tb, mask, slot_of_item);
        }
        __syncthreads();
        const int n_hub = s_nhub;
        for (int i = 0; i < n_hub; ++i) { // block-uniform
            const int64_t hd = s_hub[i];
            const Row hub = listed_row(g, dst, hd);
            const int64_t from = hub_share(hub.deg, w), to = hub_share(hub.deg, w + 1);
            const uint32_t mine = labor_wave_count(g, lkey, hub.start, hub.deg, fanout, from, to, lane);
            if (lane == 0) s_wcnt[w] = mine;
            __syncthreads();
            int64_t hslot = indptr_local[hd];
            for (int q = 0; q < w; ++q) hslot += s_wcnt[q];
            for (int64_t c0 = from; c0 < to; c0 += 64) { // wave-uniform
                const int64_t j = c0 + lane;
                const int64_t t = j < to ? g.indices[hub.start + j] : -1;
                const bool take = j < to && labor_take(lkey, t, hub.deg, fanout);
                hslot += labor_emit(take, ~0ull, lane, t, hub.start + j, hslot, n_dst, nbr, eid, tb, mask, slot_of_item);
            }
            __syncthreads(); // s_wcnt is rewritten for the next row
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- relation layers
constexpr int kMaxRels = 64;
constexpr int kRelHubList = kBlock; // a block step holds kBlock / GS rows of at most GS relations each: its deferred segments always fit

struct RelFan { // the fan-outs of one layer, by value in the kernel arguments
    int8_t f[kMaxRels]; // -1, 0, 1..32; 0 past num_rels
    int32_t num_rels;
};

struct RelSeg { // relation `gl` of a row, on lane gl of the row's group: its in-edges [s, s + deg) and how many of them the layer takes
    int64_t s, deg, take;
};

// First position in [lo, hi) whose type is not below `key` (hi when there is none).
__device__ __forceinline__ int64_t type_lower_bound(const int32_t* __restrict__ etype, int64_t lo, int64_t hi, int32_t key) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (etype[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Lane gl < num_rels of the group finds where relation gl ends; its start is the end of relation gl - 1 (the row's start for gl = 0).
// Every boundary lies inside the row whatever the types hold; a segment of negative length (types not sorted) counts as empty.
// Every lane of the wave must call it.
__device__ __forceinline__ RelSeg rel_segment(const int32_t* __restrict__ etype, const RelFan& fan, const Row& row, int gl, int gbase) {
    const bool mine = gl < fan.num_rels;
    const int64_t row_end = row.start + row.deg;
    const int64_t end = mine ? type_lower_bound(etype, row.start, row_end, gl + 1) : row_end;
    const int64_t prev = __shfl(end, gbase + (gl > 0 ? gl - 1 : 0));
    const int64_t s = gl > 0 ? prev : row.start;
    const int64_t deg = mine ? max(end - s, (int64_t)0) : 0;
    const int f = fan.f[gl];
    return {s, deg, (!mine || f == 0) ? 0 : (f < 0 || deg <= f) ? deg : (int64_t)f};
}

// Relation layer, pass 1, where degree_scan_kernel stands: the number of taken edges of every destination node -> indptr_local
// (exclusive scan) and E.  Tiles of `rows` destination nodes as in labor_count_scan_kernel; GS lanes per row (GS >= num_rels), the
// row's count is the sum of its relations' takes.  No row is walked: a hub costs its binary searches.
template <int GS>
__global__ __launch_bounds__(kBlock) void rel_count_scan_kernel(Graph g, const int32_t* __restrict__ etype, RelFan fan, const int64_t* __restrict__ dst,
                                                                const int64_t* __restrict__ n_dst_dev, int64_t n_dst_value, int rows,
                                                                int64_t* __restrict__ base, unsigned long long* __restrict__ status,
                                                                unsigned long long* __restrict__ ticket, unsigned long long ticket_base,
                                                                unsigned long long gen, int64_t* __restrict__ indptr_local, int64_t item_cap,
                                                                int64_t edge_cap, int64_t* __restrict__ pin) {
    constexpr int GPB = kBlock / GS;
    __shared__ uint32_t s_cnt[kTile];
    const int lane = threadIdx.x & 63;
    const int64_t n_dst = layer_n_dst(n_dst_dev, n_dst_value);
    const int64_t n_tiles = n_dst > 0 ? (n_dst + rows - 1) / rows : 1; // tile 0 always runs: it publishes an empty layer too
    const int64_t tile = take_tile(ticket, ticket_base);
    if (tile >= n_tiles) return;
    const int64_t row0 = tile * rows;
    const auto [gl, gbase, gmask] = lane_group<GS>(lane);
    for (int r = (int)threadIdx.x / GS; r < rows; r += GPB) { // wave-uniform trip count: rows is a multiple of GPB
        const Row row = dst_row(g, dst, row0 + r, n_dst);
        int64_t n = rel_segment(etype, fan, row, gl, gbase).take;
        for (int off = 1; off < GS; off <<= 1) n += __shfl_xor(n, off);
        if (gl == 0) s_cnt[r] = n > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)n;
    }
    __syncthreads();
    scan_row_counts(s_cnt, rows, row0, n_dst, tile, n_tiles, status, gen, !n_dst_dev, item_cap, edge_cap, indptr_local, base, pin);
}

// Relation layer, pass 2, where full_insert_kernel stands: item p < n_dst is destination node p; item n_dst + q is taken edge q of the
// layer.  GS lanes per row (GS >= num_rels and >= every fan-out) find the boundaries again; relation r's taken edges start at
// indptr_local[d] + the takes of the relations before it.  Then relation by relation (the fan-out is the layer's, so the branches are
// wave-uniform): a drawn relation runs sample_insert_kernel's Floyd loop on the segment with a lane per candidate and sorts the picks
// over the group's lanes (rows with deg_r <= f_r hold positions 0 .. deg_r - 1 there); a -1 relation is copied in lane strides, and
// a segment of more than kHubDegree edges goes on the block's list and is copied by all its threads afterwards.  A refused layer
// (0 items) does nothing.
template <int GS>
__global__ __launch_bounds__(kBlock) void rel_insert_kernel(Graph g, const int32_t* __restrict__ etype, RelFan fan, const int64_t* __restrict__ dst,
                                                            const int64_t* __restrict__ base, const int64_t* __restrict__ indptr_local,
                                                            uint64_t seed, uint64_t step, int layer, int64_t* __restrict__ nbr, Table tb,
                                                            uint32_t* __restrict__ slot_of_item, int64_t* __restrict__ eid) {
    constexpr int GPB = kBlock / GS;
    __shared__ int64_t s_hub[kRelHubList][3]; // first CSC position, length, first slot
    __shared__ int s_nhub;
    const int64_t n_dst = base[0];
    const int64_t n_items = base[kItemsOff];
    if (n_items == 0) return;
    const uint32_t mask = table_size(n_items) - 1;
    const int lane = threadIdx.x & 63;
    const auto [gl, gbase, gmask] = lane_group<GS>(lane);
    // slot q of the layer takes the edge at CSC position e: the neighbour is stored (scan_assign reads it back), its edge id when asked
    const auto emit = [&](int64_t q, int64_t e) {
        const int64_t t = g.indices[e];
        nbr[q] = t;
        if (eid) eid[q] = e;
        hash_insert(tb, mask, t, n_dst + q, slot_of_item);
    };
    for (int64_t d0 = (int64_t)blockIdx.x * GPB; d0 < n_dst; d0 += (int64_t)gridDim.x * GPB) { // block-uniform
        if (threadIdx.x == 0) s_nhub = 0;
        __syncthreads();
        const int64_t d = d0 + (int)threadIdx.x / GS;
        const Row row = dst_row(g, dst, d, n_dst);
        if (d < n_dst && gl == 0) hash_insert(tb, mask, row.v, d, slot_of_item);
        const RelSeg sg = rel_segment(etype, fan, row, gl, gbase);
        int64_t incl = sg.take; // inclusive scan of the takes over the group's lanes
        for (int off = 1; off < GS; off <<= 1) {
            const int64_t v = __shfl_up(incl, off);
            if (gl >= off) incl += v;
        }
        const int64_t slot0 = (row.deg > 0 ? indptr_local[d] : 0) + incl - sg.take;
        const uint64_t key = sample_key(seed, step, layer, (uint64_t)row.v);
        for (int r = 0; r < fan.num_rels; ++r) { // wave-uniform, and so is every branch on f
            const int f = fan.f[r];
            if (f == 0) continue;
            const int64_t s_r = __shfl(sg.s, gbase + r), deg_r = __shfl(sg.deg, gbase + r), q_r = __shfl(slot0, gbase + r);
            if (f < 0) { // taken whole, whatever its length
                int at = -1;
                if (gl == 0 && deg_r > kHubDegree) at = atomicAdd(&s_nhub, 1);
                at = __shfl(at, gbase);
                if (at >= 0) { // deferred to the whole block
                    if (gl == 0) {
                        s_hub[at][0] = s_r;
                        s_hub[at][1] = deg_r;
                        s_hub[at][2] = q_r;
                    }
                } else {
                    for (int64_t j = gl; j < deg_r; j += GS) emit(q_r + j, s_r + j);
                }
                continue;
            }
            // candidate of lane c = gl (Floyd step j = deg_r - f + c), positions relative to s_r
            const bool drawn = deg_r > f;
            const int64_t t = (drawn && gl < f) ? (int64_t)__umul64hi(splitmix64(key + (uint64_t)(kMaxRels * r + gl)), (uint64_t)(deg_r - f + gl + 1)) : -1;
            int64_t chosen = -2;
            for (int c = 0; c < f; ++c) {
                const int64_t tc = __shfl(t, gbase + c);
                const uint64_t dupm = __ballot(gl < c && chosen == tc) & gmask;
                if (gl == c) chosen = dupm ? (deg_r - f + c) : tc;
            }
            unsigned long long pk = (unsigned long long)kNoPos; // lane i ends up with the i-th smallest pick
            if (gl < f && (drawn || gl < deg_r)) pk = (unsigned long long)(drawn ? chosen : (int64_t)gl);
            int64_t unused = 0;
            group_sort<GS>(pk, unused, gl);
            if (gl < min(deg_r, (int64_t)f)) emit(q_r + gl, s_r + (int64_t)pk);
        }
        __syncthreads();
        const int n_hub = s_nhub;
        for (int i = 0; i < n_hub; ++i) // block-uniform
            for (int64_t j = threadIdx.x; j < s_hub[i][1]; j += kBlock) emit(s_hub[i][2] + j, s_hub[i][0] + j);
        __syncthreads(); // the list is rewritten in the next step
    }
}

// first layer full: its table size is known on the device only
__global__ __launch_bounds__(kBlock) void table_clear_kernel(Table tb, const int64_t* __restrict__ items_dev) { clear_table(tb, table_size(*items_dev)); }

__device__ __forceinline__ uint32_t first_flag(const uint32_t* __restrict__ slot_of_item, const uint32_t* __restrict__ minpos, int64_t p,
                                               int64_t n_items) {
    if (p >= n_items) return 0;
    const uint32_t s = slot_of_item[p];
    return (s != 0xFFFFFFFFu && minpos[s] == (uint32_t)p) ? 1u : 0u;
}

// First-occurrence flags -> positions in the source list, in one pass (tile_scan); the block of the last tile publishes the source
// count.  FULL (a fan-out -1 layer): n_dst and the item count come from the layer's device words (n_dst_dev = its base), and n_dst_value
// is the largest source count the fixed layers behind it accept: above it the next layers see 0 destination nodes.
template <bool FULL>
__global__ __launch_bounds__(kBlock) void scan_assign_kernel(const int64_t* __restrict__ dst, const int64_t* __restrict__ nbr,
                                                             const int64_t* __restrict__ n_dst_dev, int64_t n_dst_value, int fanout,
                                                             const uint32_t* __restrict__ slot_of_item, Table tb, unsigned long long* __restrict__ status,
                                                             unsigned long long* __restrict__ ticket, unsigned long long ticket_base,
                                                             unsigned long long gen, int64_t* __restrict__ src_nodes, int64_t* __restrict__ n_src_dev,
                                                             int64_t* __restrict__ n_src_host) {
    const int64_t n_dst = FULL ? *n_dst_dev : layer_n_dst(n_dst_dev, n_dst_value);
    const int64_t n_items = FULL ? n_dst_dev[kItemsOff] : n_dst * (fanout + 1);
    const int64_t n_tiles = (n_items + kTile - 1) / kTile;
    const int64_t tile = take_tile(ticket, ticket_base);
    if (tile >= n_tiles) { // launched for the capacity; the block that would own the first unused tile reports an empty layer
        if (tile == 0 && threadIdx.x == 0) {
            *n_src_dev = 0;
            *n_src_host = 0;
            if constexpr (FULL) n_src_host[kPinOver] = 0;
        }
        return;
    }
    const int64_t base = tile * kTile + (int64_t)threadIdx.x * kItems;
    uint32_t fl[kItems];
    uint32_t c = 0;
    for (int i = 0; i < kItems; ++i) { fl[i] = first_flag(slot_of_item, tb.minpos, base + i, n_items); c += fl[i]; }
    const TileScan ts = tile_scan<false>(status, gen, tile, n_tiles, c);
    if (ts.last && threadIdx.x == 0) { // layer l+1 (and the host) read the number of source nodes from here
        const int64_t n_src = (int64_t)ts.total;
        const bool over = FULL && n_src > n_dst_value;
        *n_src_dev = over ? 0 : n_src;
        *n_src_host = n_src;
        if constexpr (FULL) n_src_host[kPinOver] = over ? 1 : 0;
    }
    uint32_t run = ts.excl;
    for (int i = 0; i < kItems; ++i) {
        if (fl[i]) {
            const int64_t p = base + i;
            src_nodes[run] = item_key(dst, nbr, n_dst, p);
            tb.local_of_slot[slot_of_item[p]] = run;
            ++run;
        }
    }
}

// neighbour -> local index in the source list; alongside, the hash table for what comes next is cleared (keys / minpos are no
// longer read by this layer): next_items_dev != null -> the next layer's size is read from the device, else next_items (next call).
// FULL: this layer's edge count is read from its device words; NEXT_FULL: so is the next layer's item count (its degree_scan ran
// before this kernel).
template <bool FULL, bool NEXT_FULL>
__global__ __launch_bounds__(kBlock) void relabel_clear_kernel(const int64_t* __restrict__ n_dst_dev, int64_t n_dst_value, int fanout, const uint32_t* __restrict__ slot_of_item,
                                                               Table tb, int32_t* __restrict__ nbr_local, const int64_t* __restrict__ next_n_dst_dev,
                                                               int next_fanout, int64_t next_items) {
    const int64_t n_dst = layer_n_dst(n_dst_dev, n_dst_value);
    const int64_t n_nbr = FULL ? n_dst_dev[kEdgesOff] : n_dst * fanout;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_nbr; q += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t s = slot_of_item[n_dst + q];
        nbr_local[q] = (s == 0xFFFFFFFFu) ? -1 : (int32_t)tb.local_of_slot[s];
    }
    if constexpr (NEXT_FULL) clear_table(tb, table_size(next_n_dst_dev[kItemsOff]));
    else clear_table(tb, table_size(next_n_dst_dev ? *next_n_dst_dev * (next_fanout + 1) : next_items));
}

// ---------------------------------------------------------------------------------------------------------- owner bucketing
// Stable partition of the input nodes by owner = id % n_parts, then the last block is re-indexed through the permutation new_of_old.  The
// per-tile bodies are coala_partition.h's; the kernels here are the sampler's own shells over them: the list's length comes from the device
// (the layer's scan wrote it), and the bucket sizes also go to the call's pinned host words.
struct BucketSink {
    int64_t* __restrict__ bucketed;
    uint32_t* __restrict__ new_of_old;
    __device__ __forceinline__ void operator()(int64_t dest, int64_t i, int64_t id) const { bucketed[dest] = id, new_of_old[i] = (uint32_t)dest; }
};

__global__ __launch_bounds__(kBlock) void bucket_count_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ n_src_dev, uint32_t P,
                                                              int pshift, uint32_t* __restrict__ wave_counts) {
    const int64_t n_src = *n_src_dev;
    const int64_t n_wt = partition_tiles(n_src), n_waves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t wt = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); wt < n_wt; wt += n_waves)
        partition_count_tile(src, n_src, wt, P, pshift, wave_counts);
}

__global__ __launch_bounds__(1024) void bucket_scan_kernel(uint32_t* __restrict__ wave_counts, const int64_t* __restrict__ n_src_dev, uint32_t P,
                                                           int64_t* __restrict__ counts_out, int64_t* __restrict__ counts_host, int64_t* __restrict__ bases) {
    __shared__ int64_t totals[kMaxParts];
    partition_scan_columns(wave_counts, partition_tiles(*n_src_dev), P, totals);
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (uint32_t g = 0; g < P; ++g) {
            counts_out[g] = totals[g];
            counts_host[g] = totals[g];
            bases[g] = acc;
            acc += totals[g];
        }
    }
}

__global__ __launch_bounds__(kBlock) void bucket_scatter_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ n_src_dev, uint32_t P,
                                                                int pshift, const uint32_t* __restrict__ wave_offsets, const int64_t* __restrict__ bases,
                                                                int64_t* __restrict__ bucketed, uint32_t* __restrict__ new_of_old) {
    const int64_t n_src = *n_src_dev;
    const int64_t n_wt = partition_tiles(n_src), n_waves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t wt = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); wt < n_wt; wt += n_waves)
        partition_scatter_tile(src, n_src, wt, P, pshift, wave_offsets, bases, BucketSink{bucketed, new_of_old});
}

template <bool FULL>
__global__ __launch_bounds__(kBlock) void bucket_reindex_kernel(const int64_t* __restrict__ n_dst_dev, int64_t n_dst_value, int fanout,
                                                                const uint32_t* __restrict__ new_of_old, int32_t* __restrict__ nbr_local,
                                                                int32_t* __restrict__ dst_in_src) {
    const int64_t n_dst = layer_n_dst(n_dst_dev, n_dst_value);
    const int64_t n_nbr = FULL ? n_dst_dev[kEdgesOff] : n_dst * fanout;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_nbr; q += (int64_t)gridDim.x * blockDim.x) {
        const int32_t o = nbr_local[q];
        if (o >= 0) nbr_local[q] = (int32_t)new_of_old[o];
    }
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_dst; d += (int64_t)gridDim.x * blockDim.x)
        dst_in_src[d] = (int32_t)new_of_old[d]; // the dst nodes are the first n_dst entries of the unbucketed list
}

// ------------------------------------------------------------------------------------------------------- edge batches
// Seed EDGES of a link-prediction minibatch (DGL's as_edge_prediction_sampler with negative_sampler.Uniform(k);
// coala_sampler_edge_batch).  Seed edge e is a CSC position: its destination is the row v with indptr[v] <= e < indptr[v+1] (an
// upper-bound search, so a run of degree-0 rows around v is never chosen), its source indices[e].  Negative j of e is the pair
// (u, mulhi64(splitmix64(nkey + j), N)) with nkey = sample_key(seed, step, 0, e) ^ kNegStream: a function of (seed, step, e, j) alone.
// The item list [src_0.. | dst_0.. | v'_{0,0}..] stands where a layer's (dst..., neighbours...) list stands: item p is hashed by
// edge_items, scan_assign (as a layer of n(2+k) "destination nodes" and fan-out 0) gives the distinct ids in order of first
// appearance, and edge_relabel_clear writes every item's index in that list and leaves the table clean, as relabel_clear does.  An e
// outside [0, E) gives -1 in each of its items (no node) and is counted.
constexpr uint64_t kNegStream = 0xA54FF53A5F1D36F1ull; // xor on sample_key: the negative pairs' own stream
constexpr int kMaxNeg = 64;

__device__ __forceinline__ int64_t edge_row(const Graph& g, int64_t e) { // 0 <= e < indptr[num_nodes]
    int64_t lo = 0, hi = g.num_nodes; // indptr[lo] <= e < indptr[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (g.indptr[mid] > e) hi = mid;
        else lo = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void edge_items_kernel(Graph g, int64_t num_edges, const int64_t* __restrict__ eids, int64_t n, int k,
                                                            uint64_t seed, uint64_t step, int64_t* __restrict__ items, Table tb,
                                                            uint32_t* __restrict__ slot_of_item, unsigned long long* __restrict__ n_bad) {
    const int64_t n_items = n * (2 + k);
    const uint32_t mask = table_size(n_items) - 1;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_items; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = p < 2 * n ? (p < n ? p : p - n) : (p - 2 * n) / k;
        const int64_t e = eids[i];
        int64_t key = -1;
        if (e >= 0 && e < num_edges) {
            if (p < n) key = g.indices[e];
            else if (p < 2 * n) key = edge_row(g, e);
            else
                key = (int64_t)__umul64hi(splitmix64((sample_key(seed, step, 0, (uint64_t)e) ^ kNegStream) + (uint64_t)((p - 2 * n) % k)),
                                          (uint64_t)g.num_nodes);
        } else if (p < n) {
            atomicAdd(n_bad, 1ull);
        }
        items[p] = key;
        hash_insert(tb, mask, key, p, slot_of_item);
    }
}

// item -> index in seed_nodes (-1: the item of a bad edge); the table is cleared for the next call alongside, and the bad-edge count
// goes to the host and back to 0.
__global__ __launch_bounds__(kBlock) void edge_relabel_clear_kernel(int64_t n, int k, const uint32_t* __restrict__ slot_of_item, Table tb,
                                                                    int32_t* __restrict__ pos_src, int32_t* __restrict__ pos_dst,
                                                                    int32_t* __restrict__ neg_dst, unsigned long long* __restrict__ n_bad,
                                                                    int64_t* __restrict__ n_bad_host, int64_t next_items) {
    const int64_t n_items = n * (2 + k);
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_items; p += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t s = slot_of_item[p];
        const int32_t local = (s == 0xFFFFFFFFu) ? -1 : (int32_t)tb.local_of_slot[s];
        if (p < n) pos_src[p] = local;
        else if (p < 2 * n) pos_dst[p - n] = local;
        else neg_dst[p - 2 * n] = local;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *n_bad_host = (int64_t)*n_bad;
        *n_bad = 0;
    }
    clear_table(tb, table_size(next_items));
}

} // namespace

struct coala_sampler {
    struct RingInfo { // what coala_sampler_wait_layers needs of a call to read its counts and explain a refusal
        // a batch's slot holds n_nodes and n_bad, collected by coala_sampler_edge_batch_wait / coala_sampler_walk_batch_wait
        enum class Holds { sample, edge_batch, walk_batch } holds = Holds::sample;
        int n_layers = 0, n_parts = 0;
        bool all_ragged = false; // a LABOR or a relation call: every layer is ragged, whatever its fan-out
        int64_t n_seeds = 0;
        bool ragged(int l) const { return all_ragged || fanouts[l] == -1; } // CSR block, sizes known on the device only
        int32_t fanouts[COALA_SAMPLER_MAX_LAYERS] = {}; // of a relation call: -1 for a layer whose fan-outs are all -1, else 0
        int64_t src_cap[COALA_SAMPLER_MAX_LAYERS] = {}, edge_cap[COALA_SAMPLER_MAX_LAYERS] = {};
    };
    int device = 0;
    Graph g{};
    int64_t num_edges = 0;
    // workspace, grown on demand
    int64_t* nbr_global = nullptr;    uint64_t nbr_cap = 0;
    Table tb{};                       uint64_t table_cap = 0;
    uint64_t clean_items = 0;         // the table is clean for a first layer of at most this many items (0 = unknown)
    uint32_t* slot_of_item = nullptr; uint64_t item_cap = 0;
    uint32_t* wave_counts = nullptr;  uint64_t wc_cap = 0;
    uint32_t* new_of_old = nullptr;   uint64_t noo_cap = 0;
    unsigned long long* status = nullptr;  // [kMaxTiles] look-back status words (generation-tagged, never reset)
    unsigned long long* ticket = nullptr;  // tile ticket counter, monotonic across launches
    unsigned long long ticket_total = 0, scan_gen = 0;
    int64_t* counts_dev = nullptr;         // [kCountsWords]: source counts of the call in flight, bucket bases, full-layer words
    // weighted layers: the rows of more than kHubDegree in-edges of a layer (at most num_edges / (kHubDegree + 1) distinct nodes)
    int64_t* hubs = nullptr;               // [hub_cap] destination indices, reused layer after layer
    int64_t hub_cap = 0;
    unsigned long long* hub_count = nullptr; // [COALA_SAMPLER_MAX_LAYERS] list lengths of the call in flight
    unsigned long long* edge_bad = nullptr;  // out-of-range seed edges of the edge batch in flight; its last kernel puts it back to 0
    // pinned host ring: per call kSlot words (kPinEdges .. kPinParts), and an event recorded behind the last kernel
    int64_t* counts_pinned = nullptr; // host pointer
    int64_t* counts_pinned_dev = nullptr;
    hipEvent_t done[kRing] = {};
    RingInfo ring[kRing];
    uint64_t calls = 0;
    hipStream_t last_stream = nullptr; // stream of the previous call
};

namespace {
using RingInfo = coala_sampler::RingInfo;
using Holds = RingInfo::Holds;
constexpr int kSlot = kPinParts + kMaxParts; // int64 words per ring slot

// One sampling call, as its entry point hands it to sample_impl: its kind -- how a fixed layer picks its edges; the kinds exclude each
// other --, the arguments every entry point has, in the ABI's order, and below them the kinds' payloads, which an entry point sets by name.
enum class Kind { uniform, weighted, labor, rel, walk, temporal };
struct Call {
    Kind kind;
    const int64_t* seeds;   int64_t n_seeds; // of a temporal call: pair codes, as layers[l].src_nodes
    const int32_t* fanouts; int n_layers;    // of a relation call: -1 for a layer whose fan-outs are all -1, else 0
    uint64_t seed, step;
    const coala_sampler_layer_t* layers;
    int64_t* const* edge_ids; // null, or per layer: null or device int64[edge_cap], the CSC position of every neighbour slot
    int64_t *n_src_host, *n_edges_host;
    const coala_sampler_bucketing_t* bucketing;
    int64_t* ticket_out;
    hipStream_t st;
    const float* weights = nullptr;                                                   // weighted: the fp32 edge weights, CSC order
    bool layer_dependency = false;                                                    // labor: one key for every layer of the call
    const RelFan* rel = nullptr;                const int32_t* etype = nullptr;       // rel: every layer's fan-outs; the int32 edge types, CSC order
    WalkParams walk{};                          int32_t* const* visit_counts = nullptr; // walk; null, or per layer null or device int32[edge_cap]
    const Temporal* temporal = nullptr;                                               // temporal: seeds / src_nodes hold pair codes
    bool all_ragged() const { return kind == Kind::labor || kind == Kind::rel; } // every layer is ragged, whatever its fan-out
};

int check_n_layers(int n) {
    return n < 1 || n > COALA_SAMPLER_MAX_LAYERS ? fail(COALA_EINVAL, "n_layers must be 1..%d", COALA_SAMPLER_MAX_LAYERS) : COALA_OK;
}

// The layers of a kind that has fixed-stride layers only ("a <noun> layer <rule>").
int check_fixed_layers(const int32_t* fanouts, const coala_sampler_layer_t* layers, int n_layers, const char* noun, const char* rule) {
    for (int l = 0; l < n_layers; ++l) {
        if (fanouts[l] < 1 || fanouts[l] > 32) return fail(COALA_EINVAL, "fan-out %d outside 1..32 (a %s layer %s)", fanouts[l], noun, rule);
        if (layers[l].indptr_local) return fail(COALA_EINVAL, "layer %d: a %s layer is fixed-stride, indptr_local must be NULL", l, noun);
    }
    return COALA_OK;
}

int check_call(const coala_sampler_t* s, const Call& c) {
    if (!s || (!c.seeds && c.n_seeds > 0) || !c.fanouts) return fail(COALA_EINVAL, "null argument");
    if (int rc = check_n_layers(c.n_layers)) return rc;
    if (c.n_seeds < 0 || c.n_seeds > 0x7FFFFFFF) return fail(COALA_EINVAL, "bad n_seeds");
    const int n_parts = c.bucketing ? c.bucketing->n_parts : 0;
    if (n_parts < 0 || n_parts > kMaxParts) return fail(COALA_EINVAL, "bucketing: n_parts must be 0..%d", kMaxParts);
    if (n_parts > 0 && (!c.bucketing->bucketed_nodes || !c.bucketing->counts || !c.bucketing->dst_in_src)) return fail(COALA_EINVAL, "bucketing: null buffer");
    if (!c.layers) return fail(COALA_EINVAL, "null argument");
    for (int l = 0; l < c.n_layers; ++l) {
        const int f = c.fanouts[l];
        if (c.kind != Kind::rel && f != kFull && (f < 1 || f > 32)) return fail(COALA_EINVAL, "fan-out %d outside 1..32 (or -1: every in-edge)", f);
        const coala_sampler_layer_t& y = c.layers[l];
        if (!y.src_nodes || !y.nbr_local || ((c.all_ragged() || f == kFull) && !y.indptr_local)) return fail(COALA_EINVAL, "layer %d: null buffer", l);
        if (y.src_cap < 0 || y.edge_cap < 0) return fail(COALA_EINVAL, "layer %d: negative capacity", l);
    }
    return COALA_OK;
}

// A batch kind in the words of a refusal: "an edge batch" / "a walk batch", and the "edge" / "walk" of its entry points' names.
const char* batch_noun(Holds k) { return k == Holds::edge_batch ? "an edge batch" : "a walk batch"; }
const char* batch_stem(Holds k) { return k == Holds::edge_batch ? "edge" : "walk"; }

// What every wait begins with: the ring slot of one of the last kRing calls, which has to be a call of the kind this wait collects, and
// the event behind that call's last kernel.  A refused wait has waited for nothing.
int wait_slot(coala_sampler_t* s, int64_t ticket, Holds kind, int* slot) {
    if (!s) return fail(COALA_EINVAL, "null sampler");
    if (ticket < 0 || (uint64_t)ticket >= s->calls || s->calls - (uint64_t)ticket > kRing)
        return fail(COALA_EINVAL, "ticket %lld is not one of the last %d calls", (long long)ticket, kRing);
    *slot = (int)((uint64_t)ticket % kRing);
    const Holds holds = s->ring[*slot].holds;
    if (holds != kind && kind != Holds::sample) return fail(COALA_EINVAL, "ticket %lld is not %s", (long long)ticket, batch_noun(kind));
    if (holds != kind)
        return fail(COALA_EINVAL, "ticket %lld is %s: collect it with coala_sampler_%s_batch_wait", (long long)ticket, batch_noun(holds), batch_stem(holds));
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipEventSynchronize(s->done[*slot])); // the kernels behind this event stored the counts into pinned host memory
    return COALA_OK;
}

// Fixed layers behind full layer l (up to the next full layer) have a destination count known on the device only.  Layer j of them
// holds at most n_src_l * P_j destination nodes (P_j = product of (f + 1) of the fixed layers between), i.e. n_dst * (f_j + 1)
// items and n_dst * f_j neighbours.  With n_src >= 0: the first such layer that n_src overflows (-1: none), its worst-case item
// count in *items_out and its bound in *limit_out.  With n_src < 0: -1, and the largest n_src they all accept in *limit_out.
int fixed_run_check(const RingInfo& r, int l, int64_t n_src, int64_t* items_out, int64_t* limit_out, const char** what) {
    int64_t most = INT64_MAX;
    int64_t mult = 1; // P_j, capped above the item limit
    for (int j = l + 1; j < r.n_layers && !r.ragged(j); ++j) {
        const int64_t f = r.fanouts[j];
        const int64_t item_lim = std::min<int64_t>(kItemLimit, r.src_cap[j]);
        if (n_src >= 0) {
            const int64_t items = n_src * mult * (f + 1);
            if (items > item_lim || n_src * mult * f > r.edge_cap[j]) {
                *items_out = items;
                *limit_out = items > item_lim ? item_lim : r.edge_cap[j];
                *what = items > kItemLimit ? "the item limit" : items > item_lim ? "its src_cap" : "its edge_cap (neighbour entries)";
                return j;
            }
        } else {
            most = std::min(most, std::min(item_lim / (mult * (f + 1)), r.edge_cap[j] / (mult * f)));
        }
        mult = std::min<int64_t>(mult * (f + 1), kItemLimit + 1);
    }
    if (n_src < 0) *limit_out = most;
    return -1;
}

int batch_wait(coala_sampler_t* s, int64_t ticket, Holds kind, int64_t* n_nodes_host, int64_t* n_bad_host) {
    int slot;
    if (int rc = wait_slot(s, ticket, kind, &slot)) return rc;
    const int64_t* pin = s->counts_pinned + (size_t)slot * kSlot;
    if (n_nodes_host) *n_nodes_host = pin[0];
    if (n_bad_host) *n_bad_host = pin[kPinEdges];
    return COALA_OK;
}

int wait_impl(coala_sampler_t* s, int64_t ticket, int64_t* n_src_host, int64_t* n_edges_host, int64_t* bucket_counts_host) {
    int slot;
    if (int rc = wait_slot(s, ticket, Holds::sample, &slot)) return rc;
    const int64_t* pin = s->counts_pinned + (size_t)slot * kSlot;
    const RingInfo& r = s->ring[slot];
    if (n_src_host)
        for (int l = 0; l < r.n_layers; ++l) n_src_host[l] = pin[l];
    if (n_edges_host)
        for (int l = 0; l < r.n_layers; ++l)
            n_edges_host[l] = r.ragged(l) ? pin[kPinEdges + l] : (l ? pin[l - 1] : r.n_seeds) * r.fanouts[l];
    if (bucket_counts_host)
        for (int g = 0; g < r.n_parts; ++g) bucket_counts_host[g] = pin[kPinParts + g];
    for (int l = 0; l < r.n_layers; ++l) { // device-side refusals, in layer order: the first one is the cause
        if (!r.ragged(l)) continue;
        const int64_t n_dst = l ? pin[l - 1] : r.n_seeds;
        if (pin[kPinRefused + l]) {
            const long long e = pin[kPinEdges + l], items = n_dst + e;
            const bool limit = items > kItemLimit, src = items > r.src_cap[l];
            return fail(COALA_EINVAL, "layer %d holds %lld items (%lld destination nodes + %lld edges): over %s of %lld", l, items, (long long)n_dst, e,
                        limit ? "the limit" : src ? "its src_cap" : "its edge_cap", (long long)(limit ? kItemLimit : src ? r.src_cap[l] : r.edge_cap[l]));
        }
        if (pin[kPinOver + l]) {
            int64_t items = 0, lim = 0;
            const char* what = "";
            const int j = fixed_run_check(r, l, pin[l], &items, &lim, &what);
            return fail(COALA_EINVAL, "layer %d would hold %lld items (%lld source nodes of full layer %d, fan-out %d behind it): over %s of %lld", j,
                        (long long)items, (long long)pin[l], l, j >= 0 ? r.fanouts[j] : 0, what, (long long)lim);
        }
    }
    return COALA_OK;
}

// A template parameter chosen at run time: f gets the value as a std::integral_constant, so each templated launch is written once
// (the idiom of dispatch_geo in coala_cache.hip).  GS: lanes per destination row of sample_insert / weighted_select.
template <typename F>
void dispatch_group(int fanout, F&& f) {
    if (fanout < 16) f(std::integral_constant<int, 16>{});
    else if (fanout < 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}

template <typename F>
void dispatch_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// What the launches of a call are made from: the call, and what the host derives from it (plan_call).
struct Plan : Call {
    RingInfo info;       // n_seeds, the fan-outs, n_parts and the caller's capacities
    // layer l has at most dst_cap[l] dst nodes, items_cap[l] items (dst nodes + neighbour slots), nbr_cap[l] neighbour entries
    int64_t dst_cap[COALA_SAMPLER_MAX_LAYERS], items_cap[COALA_SAMPLER_MAX_LAYERS], nbr_cap[COALA_SAMPLER_MAX_LAYERS];
    uint64_t max_items, max_nbr;
    int64_t* pin_dev;     // the call's ring slot, as the device sees it
    uint64_t items0;      // what the last kernel leaves clean for the next call (launch_call)
};

// Capacities.  Up to the first full layer they are exact host bounds (cap_l * (f + 1)) and checked here; a full layer and the fixed
// layers behind it are checked on the device against the caller's capacities and the item limit.
int plan_call(Plan& p) {
    p.info.all_ragged = p.all_ragged();
    p.info.n_layers = p.n_layers;
    p.info.n_parts = p.bucketing ? p.bucketing->n_parts : 0;
    p.info.n_seeds = p.n_seeds;
    p.max_items = p.max_nbr = 0;
    int64_t cap = p.n_seeds;
    bool host_bound = true;
    for (int l = 0; l < p.n_layers; ++l) {
        const int f = p.fanouts[l];
        const coala_sampler_layer_t& y = p.layers[l];
        p.info.fanouts[l] = f;
        p.info.src_cap[l] = y.src_cap;
        p.info.edge_cap[l] = y.edge_cap;
        p.dst_cap[l] = cap;
        if (p.info.ragged(l)) {
            host_bound = false;
            p.items_cap[l] = std::min<int64_t>(kItemLimit, y.src_cap);
            p.nbr_cap[l] = std::min<int64_t>(kItemLimit, y.edge_cap);
        } else if (host_bound) {
            const uint64_t items = (uint64_t)cap * (uint64_t)(f + 1);
            if (items > (uint64_t)kItemLimit) return fail(COALA_EINVAL, "layer %d would hold %llu items (limit %d)", l, (unsigned long long)items, kMaxTiles * kTile);
            if ((uint64_t)y.src_cap < items || (uint64_t)y.edge_cap < (uint64_t)cap * f)
                return fail(COALA_EINVAL, "layer %d: src_cap %lld / edge_cap %lld below the %llu / %llu its fan-out of %d needs", l, (long long)y.src_cap,
                            (long long)y.edge_cap, (unsigned long long)items, (unsigned long long)cap * f, f);
            p.items_cap[l] = (int64_t)items;
            p.nbr_cap[l] = cap * f;
        } else {
            p.items_cap[l] = std::min(std::min<int64_t>(cap * (f + 1), kItemLimit), y.src_cap);
            p.nbr_cap[l] = std::min(std::min<int64_t>(cap * f, kItemLimit), y.edge_cap);
        }
        if ((uint64_t)p.items_cap[l] > p.max_items) p.max_items = (uint64_t)p.items_cap[l];
        if ((uint64_t)p.nbr_cap[l] > p.max_nbr) p.max_nbr = (uint64_t)p.nbr_cap[l];
        cap = p.items_cap[l];
    }
    return COALA_OK;
}

// The scratch of a call of at most max_items items and max_nbr neighbour entries in a layer, and cap source nodes in the last one.
int grow_workspace(coala_sampler_t* s, hipStream_t st, int n_parts, uint64_t cap, uint64_t max_items, uint64_t max_nbr) {
    int rc;
    const uint64_t table = table_size((int64_t)max_items);
    const uint64_t wave_tiles = (uint64_t)partition_tiles((int64_t)cap);
    if ((rc = grow((void**)&s->nbr_global, &s->nbr_cap, max_nbr ? max_nbr : 1, sizeof(int64_t), st))) return rc;
    if ((rc = grow((void**)&s->slot_of_item, &s->item_cap, max_items ? max_items : 1, sizeof(uint32_t), st))) return rc;
    if (n_parts > 0) {
        if ((rc = grow((void**)&s->wave_counts, &s->wc_cap, (wave_tiles + 1) * (uint64_t)n_parts, sizeof(uint32_t), st))) return rc;
        if ((rc = grow((void**)&s->new_of_old, &s->noo_cap, cap ? cap : 1, sizeof(uint32_t), st))) return rc;
    }
    if (table > s->table_cap) {
        HIPCHK(hipStreamSynchronize(st));
        for (void** q : {(void**)&s->tb.keys, (void**)&s->tb.local_of_slot})
            if (*q) { HIPCHK(hipFree(*q)); *q = nullptr; }
        HIPCHK(hipMalloc((void**)&s->tb.keys, table * (sizeof(long long) + sizeof(uint32_t)))); // keys, then the first-position words
        HIPCHK(hipMalloc((void**)&s->tb.local_of_slot, table * sizeof(uint32_t)));
        s->table_cap = table;
        s->tb.minpos = reinterpret_cast<uint32_t*>(s->tb.keys + table);
        s->clean_items = 0;
    }
    return COALA_OK;
}

// No seeds: nothing is launched; the counts are written from the host and the device-side outputs a caller reads are zeroed.
int empty_call(const Plan& p, int64_t* pin) {
    for (int l = 0; l < p.info.n_layers; ++l) {
        pin[l] = pin[kPinEdges + l] = pin[kPinRefused + l] = pin[kPinOver + l] = 0;
        if (p.info.ragged(l)) HIPCHK(hipMemsetAsync(p.layers[l].indptr_local, 0, sizeof(int64_t), p.st));
    }
    for (int g = 0; g < p.info.n_parts; ++g) pin[kPinParts + g] = 0;
    if (p.info.n_parts > 0) HIPCHK(hipMemsetAsync(p.bucketing->counts, 0, (size_t)p.info.n_parts * sizeof(int64_t), p.st));
    return COALA_OK;
}

// The generation tag of the next single-pass scan (degree_scan, scan_assign).
int next_gen(coala_sampler_t* s, hipStream_t st) {
    if ((++s->scan_gen & 0x3FFFFFFFull) == 0) { // 2^30 scans: the generation tag wraps -> clear the status words once
        HIPCHK(hipMemsetAsync(s->status, 0, kMaxTiles * sizeof(unsigned long long), st));
        s->scan_gen++;
    }
    return COALA_OK;
}

// Lanes per destination row of the relation kernels: one per relation, and one per candidate of the largest fan-out (dispatch_group's
// argument: it gives a group of more lanes than that).
int rel_group(const RelFan& fan) {
    int need = fan.num_rels;
    for (int r = 0; r < fan.num_rels; ++r) need = std::max<int>(need, fan.f[r]);
    return need - 1;
}

// Ragged layer l: degrees (full) or counts of taken edges (LABOR, relations) -> indptr_local, and its edge and item counts into its
// device words.
int degree_scan(coala_sampler_t* s, const Plan& p, int l, const int64_t* dst, const int64_t* n_dst_dev) {
    if (int rc = next_gen(s, p.st)) return rc;
    const bool full = p.info.fanouts[l] == kFull;
    int rows = full ? kTile : 64; // destination nodes per tile; LABOR, relations: the smallest power of two with which dst_cap fits kMaxTiles tiles
    while (rows < kTile && (p.dst_cap[l] + rows - 1) / rows > kMaxTiles) rows <<= 1;
    const int tiles = grid1d(p.dst_cap[l], rows, kMaxTiles);
    auto launch = [&](auto kernel, auto... head) { // the three kernels end alike: the scan state, the layer's indptr and its limits
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(kBlock), 0, p.st, s->g, head..., s->counts_dev + l, s->status, s->ticket, s->ticket_total,
                           s->scan_gen & 0x3FFFFFFFull, p.layers[l].indptr_local, p.items_cap[l],
                           std::min<int64_t>(kItemLimit, p.layers[l].edge_cap), p.pin_dev + l);
    };
    if (full)
        launch(degree_scan_kernel, dst, n_dst_dev, p.info.n_seeds);
    else if (p.kind == Kind::rel)
        dispatch_group(rel_group(p.rel[l]), [&](auto gs_c) {
            launch(rel_count_scan_kernel<decltype(gs_c)::value>, p.etype, p.rel[l], dst, n_dst_dev, p.info.n_seeds, rows);
        });
    else
        launch(labor_count_scan_kernel, dst, n_dst_dev, p.info.n_seeds, rows, p.info.fanouts[l], labor_key(p.seed, p.step, l, p.layer_dependency));
    s->ticket_total += (unsigned long long)tiles;
    return COALA_OK;
}

// Layer l over the destination nodes dst[0 .. *n_dst_dev) (n_dst_dev null: the seeds, whose count travels as a kernel argument).
int launch_layer(coala_sampler_t* s, const Plan& p, int l, const int64_t* dst, const int64_t* n_dst_dev) {
    const int64_t n_seeds = p.info.n_seeds;
    const int f = p.info.fanouts[l];
    const bool full = p.info.ragged(l); // the ragged form: a full layer, or a LABOR layer
    const int64_t cap_l = p.dst_cap[l];
    int64_t* base = s->counts_dev + l;
    int64_t* n_src_dev = s->counts_dev + l + 1;
    int64_t* const src_out = p.layers[l].src_nodes;
    int32_t* const nbr_out = p.layers[l].nbr_local;
    const dim3 blk(kBlock);
    const int tiles = grid1d(p.items_cap[l], kTile, kMaxTiles);
    const int64_t* rdev = full ? (const int64_t*)base : n_dst_dev; // a full layer reads n_dst and E from its base
    hipStream_t st = p.st;
    int64_t* const eid = p.edge_ids ? p.edge_ids[l] : nullptr;
    int rc;
    int64_t max_src = 0; // full layer: the most source nodes the fixed layers behind it accept
    if (full) {
        if (f == kFull)
            hipLaunchKernelGGL(full_insert_kernel, dim3(grid1d(p.items_cap[l], kBlock, 8192)), blk, 0, st, s->g, dst, (const int64_t*)base,
                               (const int64_t*)p.layers[l].indptr_local, s->nbr_global, s->tb, s->slot_of_item, eid);
        else if (p.kind == Kind::rel)
            dispatch_group(rel_group(p.rel[l]), [&](auto gs_c) {
                constexpr int GS = decltype(gs_c)::value;
                hipLaunchKernelGGL(rel_insert_kernel<GS>, dim3(grid1d(cap_l * GS, kBlock, 8192)), blk, 0, st, s->g, p.etype, p.rel[l], dst,
                                   (const int64_t*)base, (const int64_t*)p.layers[l].indptr_local, p.seed, p.step, l, s->nbr_global, s->tb,
                                   s->slot_of_item, eid);
            });
        else
            hipLaunchKernelGGL(labor_insert_kernel, dim3(grid1d(cap_l * kLaborGroup, kBlock, 8192)), blk, 0, st, s->g, dst, (const int64_t*)base,
                               (const int64_t*)p.layers[l].indptr_local, f, labor_key(p.seed, p.step, l, p.layer_dependency), s->nbr_global,
                               s->tb, s->slot_of_item, eid);
        int64_t unused_items = 0;
        const char* unused_what = nullptr;
        fixed_run_check(p.info, l, -1, &unused_items, &max_src, &unused_what);
    } else {
        unsigned long long* nh = s->hub_count + l;
        dispatch_group(p.kind == Kind::walk ? std::max(f, p.walk.W - 1) : f, [&](auto gs_c) { // a walk layer: a lane per walk too
            constexpr int GS = decltype(gs_c)::value;
            const dim3 gs(grid1d(cap_l * GS, kBlock, 8192));
            // a walk layer's dynamic LDS holds the visits (int64) and their counts (int32) of the kBlock / GS rows of a block
            const size_t walk_lds = (size_t)(kBlock / GS) * (size_t)(p.walk.W * p.walk.T) * (sizeof(int64_t) + sizeof(int32_t));
            if (p.kind == Kind::walk)
                hipLaunchKernelGGL(walk_select_kernel<GS>, gs, blk, walk_lds, st, s->g, dst, n_dst_dev, n_seeds, f, p.walk, p.seed, p.step, l,
                                   s->nbr_global, p.visit_counts ? p.visit_counts[l] : nullptr, s->tb, s->slot_of_item);
            else if (p.kind == Kind::temporal)
                hipLaunchKernelGGL(temporal_select_kernel<GS>, gs, blk, 0, st, s->g, *p.temporal, dst, n_dst_dev, n_seeds, f, p.seed, p.step, l,
                                   s->nbr_global, s->tb, s->slot_of_item, eid);
            else if (p.kind == Kind::weighted)
                hipLaunchKernelGGL(weighted_select_kernel<GS>, gs, blk, 0, st, s->g, p.weights, dst, n_dst_dev, n_seeds, f, p.seed, p.step, l,
                                   s->nbr_global, s->tb, s->slot_of_item, s->hubs, nh, s->hub_cap, eid);
            else
                hipLaunchKernelGGL(sample_insert_kernel<GS>, gs, blk, 0, st, s->g, dst, n_dst_dev, n_seeds, f, p.seed, p.step, l, s->nbr_global, s->tb,
                                   s->slot_of_item, eid);
        });
        if (p.kind == Kind::weighted && s->hub_cap > 0) // no launch on a graph that cannot hold a row of more than kHubDegree in-edges
            hipLaunchKernelGGL(weighted_select_hub_kernel, dim3((unsigned)std::min<int64_t>(std::min<int64_t>(kHubGrid, s->hub_cap), std::max<int64_t>(cap_l, 1))),
                               dim3(kHubBlock), 0, st, s->g, p.weights, dst, n_dst_dev, n_seeds, f, p.seed, p.step, l, s->nbr_global, s->tb,
                               s->slot_of_item, (const int64_t*)s->hubs, (const unsigned long long*)nh, s->hub_cap, eid);
    }
    if ((rc = next_gen(s, st))) return rc;
    dispatch_bool(full, [&](auto full_c) { // a full layer: n_dst from its base, and max_src in place of the seed count
        hipLaunchKernelGGL(scan_assign_kernel<decltype(full_c)::value>, dim3(tiles), blk, 0, st, dst, s->nbr_global, rdev, full ? max_src : n_seeds,
                           full ? 0 : f, s->slot_of_item, s->tb, s->status, s->ticket, s->ticket_total, s->scan_gen & 0x3FFFFFFFull, src_out,
                           n_src_dev, p.pin_dev + l);
    });
    s->ticket_total += (unsigned long long)tiles;
    const bool last = l + 1 == p.info.n_layers;
    const bool next_full = !last && p.info.ragged(l + 1);
    // a full next layer: its degree scan runs now, so that this layer's relabel_clear knows how much table to clear for it
    if (next_full && (rc = degree_scan(s, p, l + 1, src_out, n_src_dev))) return rc;
    const int64_t clear_cap = last ? (int64_t)table_size((int64_t)p.items0) : (int64_t)table_size(p.items_cap[l + 1]);
    const int64_t* next_dev = last ? (const int64_t*)nullptr : (const int64_t*)n_src_dev;
    const int next_f = last ? 0 : p.info.fanouts[l + 1];
    const dim3 gr(grid1d(std::max<int64_t>(p.nbr_cap[l], clear_cap), kBlock, 4096));
    dispatch_bool(full, [&](auto full_c) {
        dispatch_bool(next_full, [&](auto next_full_c) {
            hipLaunchKernelGGL((relabel_clear_kernel<decltype(full_c)::value, decltype(next_full_c)::value>), gr, blk, 0, st, rdev, n_seeds, f,
                               s->slot_of_item, s->tb, nbr_out, next_dev, next_f, (int64_t)p.items0);
        });
    });
    if (last && p.info.n_parts > 0) { // owner bucketing of the source list, and the block re-indexed through the permutation
        const uint32_t P = (uint32_t)p.info.n_parts;
        const int pshift = ilog2_exact((uint64_t)P);
        int64_t* bases = s->counts_dev + COALA_SAMPLER_MAX_LAYERS + 1;
        const dim3 gw = partition_grid(partition_tiles(p.items_cap[l]));
        hipLaunchKernelGGL(bucket_count_kernel, gw, blk, 0, st, src_out, n_src_dev, P, pshift, s->wave_counts);
        hipLaunchKernelGGL(bucket_scan_kernel, dim3(1), partition_scan_block(P), 0, st, s->wave_counts, n_src_dev, P, p.bucketing->counts,
                           p.pin_dev + kPinParts, bases);
        hipLaunchKernelGGL(bucket_scatter_kernel, gw, blk, 0, st, src_out, n_src_dev, P, pshift, (const uint32_t*)s->wave_counts, (const int64_t*)bases,
                           p.bucketing->bucketed_nodes, s->new_of_old);
        const dim3 gb(grid1d(full ? std::max(p.nbr_cap[l], cap_l) : cap_l * f, kBlock, 4096));
        dispatch_bool(full, [&](auto full_c) {
            hipLaunchKernelGGL(bucket_reindex_kernel<decltype(full_c)::value>, gb, blk, 0, st, rdev, n_seeds, f, s->new_of_old, nbr_out,
                               p.bucketing->dst_in_src);
        });
    }
    return COALA_OK;
}

// A new call's stream hand-over and ring slot.  The handle's scratch (hash table, scan state) is ordered by the stream of its calls.
int begin_call(coala_sampler_t* s, hipStream_t st, int* slot) {
    HIPCHK(hipSetDevice(s->device));
    if (s->calls > 0 && s->last_stream != st) HIPCHK(hipStreamWaitEvent(st, s->done[(s->calls - 1) % kRing], 0)); // behind the previous call's last kernel
    s->last_stream = st;
    *slot = (int)(s->calls % kRing);
    if (s->calls >= kRing) HIPCHK(hipEventSynchronize(s->done[*slot])); // the ring slot's previous user has finished writing it
    return COALA_OK;
}

// The call is committed: the event behind its last kernel, its record on the ring, and its ticket.  Until here the slot still describes
// ticket calls - kRing, which wait_slot accepts.
int end_call(coala_sampler_t* s, int slot, hipStream_t st, const RingInfo& info, int64_t* ticket_out) {
    HIPCHK(hipEventRecord(s->done[slot], st));
    s->ring[slot] = info;
    if (ticket_out) *ticket_out = (int64_t)s->calls;
    s->calls++;
    return COALA_OK;
}

// The table of a first layer of items0 items, a size the host knows: normally left clean by the previous call's last kernel.
int prepare_table(coala_sampler_t* s, uint64_t items0, hipStream_t st) {
    const bool stale = s->clean_items == 0 || table_size((int64_t)items0) > table_size((int64_t)s->clean_items);
    s->clean_items = 0; // from here on the table is written: a call that fails half-way leaves no clean extent behind
    if (stale) {
        const uint32_t t0 = table_size((int64_t)items0);
        HIPCHK(hipMemsetAsync(s->tb.keys, 0xFF, (size_t)t0 * sizeof(long long), st));
        HIPCHK(hipMemsetAsync(s->tb.minpos, 0xFF, (size_t)t0 * sizeof(uint32_t), st));
    }
    return COALA_OK;
}

// Every launch of a call with seeds: the layers, each reading its destination nodes from the one before.  The table of a fixed first
// layer is ring_call's business (p.items0); that of a ragged one is cleared here, by what its degree scan finds.
int launch_call(coala_sampler_t* s, Plan& p) {
    int rc;
    const bool first_full = p.info.ragged(0);
    if (first_full) {
        // what the last kernel leaves clean for the next call: the first layer's table of this call, or -- when that size is known on
        // the device only, as here -- the extent the previous call left clean
        p.items0 = std::max<uint64_t>(s->clean_items, 1);
        s->clean_items = 0;
    }
    if (p.kind == Kind::weighted && s->hub_cap > 0) HIPCHK(hipMemsetAsync(s->hub_count, 0, (size_t)p.n_layers * sizeof(unsigned long long), p.st));
    if (first_full) {
        if ((rc = degree_scan(s, p, 0, p.seeds, nullptr))) return rc;
        hipLaunchKernelGGL(table_clear_kernel, dim3(grid1d(table_size(p.items_cap[0]), kBlock, 4096)), dim3(kBlock), 0, p.st, s->tb,
                           (const int64_t*)(s->counts_dev + kItemsOff));
    }
    for (int l = 0; l < p.n_layers; ++l) // layer l > 0 reads its destination nodes and their count from layer l - 1's outputs
        if ((rc = launch_layer(s, p, l, l ? p.layers[l - 1].src_nodes : p.seeds, l ? s->counts_dev + l : nullptr))) return rc;
    s->clean_items = p.items0;
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

// One call on the handle's ring, the only place that takes and commits a slot: the stream hand-over and the slot, the scratch (cap,
// max_items, max_nbr: grow_workspace's) and the table of a first layer of items0 items (0: an empty call, or a ragged first layer, whose
// size the host does not know), then body(pin, pin_dev) -- every launch of the call, or the words an empty call writes from the host,
// given the slot's pinned words as the host and the device see them -- and the commit.  A call that fails on the way leaves the ring's
// records as they were.
template <typename F>
int ring_call(coala_sampler_t* s, hipStream_t st, const RingInfo& info, uint64_t cap, uint64_t max_items, uint64_t max_nbr, uint64_t items0,
              int64_t* ticket_out, F&& body) {
    int rc, slot;
    if ((rc = begin_call(s, st, &slot))) return rc;
    if ((rc = grow_workspace(s, st, info.n_parts, cap, max_items, max_nbr))) return rc;
    if (items0 > 0 && (rc = prepare_table(s, items0, st))) return rc;
    if ((rc = body(s->counts_pinned + (size_t)slot * kSlot, s->counts_pinned_dev + (size_t)slot * kSlot))) return rc;
    return end_call(s, slot, st, info, ticket_out);
}

int sample_impl(coala_sampler_t* s, const Call& c) {
    int rc;
    if ((rc = check_call(s, c))) return rc;
    Plan p{c};
    if ((rc = plan_call(p))) return rc;
    p.items0 = p.info.ragged(0) ? 0 : (uint64_t)c.n_seeds * (uint64_t)(c.fanouts[0] + 1);
    rc = ring_call(s, c.st, p.info, (uint64_t)p.items_cap[c.n_layers - 1], p.max_items, p.max_nbr, p.items0, c.ticket_out,
                   [&](int64_t* pin, int64_t* pin_dev) {
                       p.pin_dev = pin_dev;
                       return c.n_seeds == 0 ? empty_call(p, pin) : launch_call(s, p);
                   });
    if (rc == COALA_OK && (c.n_src_host || c.n_edges_host)) return wait_impl(s, (int64_t)s->calls - 1, c.n_src_host, c.n_edges_host, nullptr);
    return rc;
}

// What an edge batch and a walk batch have in common.  The batch's kernel writes an item list (endpoints and negatives; start nodes,
// traces and negatives); the list then goes through the handle's hash table and scan as the destination nodes of one fixed layer of
// fan-out 0 do, and comes out as the list of its distinct nodes and every item's place in it.
struct ItemBatch {
    Holds kind;
    int64_t items;      // 0: an empty batch, nothing is launched
    hipStream_t st;
    int64_t* nodes_out; // device int64[items]: the distinct nodes in order of first appearance
    int64_t* ticket_out;
};

// The batch takes a ring slot, the handle's scratch and its table as a sample of one fixed layer over `items` items does (what it records
// on the ring: no parts, one layer, `items` seeds): three launches -- the kind's items kernel (launch_items()), the layers' scan_assign,
// the kind's relabel-and-clear kernel (launch_relabel(grid, the slot's device word for n_bad)) --, n_nodes and n_bad into the slot's
// pinned words, and the table left clean for `items` items.
template <typename Items, typename Relabel>
int item_batch(coala_sampler_t* s, const ItemBatch& b, Items&& launch_items, Relabel&& launch_relabel) {
    const RingInfo info{b.kind, 1, 0, false, b.items};
    const uint64_t items = (uint64_t)b.items;
    return ring_call(s, b.st, info, items, items, items, items, b.ticket_out, [&](int64_t* pin, int64_t* pin_dev) -> int {
        if (b.items == 0) {
            pin[0] = pin[kPinEdges] = 0;
            return COALA_OK;
        }
        launch_items();
        if (int rc = next_gen(s, b.st)) return rc;
        const int tiles = grid1d(b.items, kTile, kMaxTiles);
        // the item list as the "destination nodes" of a layer of fan-out 0: n_items = items, item p is items[p]
        hipLaunchKernelGGL(scan_assign_kernel<false>, dim3(tiles), dim3(kBlock), 0, b.st, (const int64_t*)s->nbr_global,
                           (const int64_t*)s->nbr_global, (const int64_t*)nullptr, b.items, 0, (const uint32_t*)s->slot_of_item, s->tb, s->status,
                           s->ticket, s->ticket_total, s->scan_gen & 0x3FFFFFFFull, b.nodes_out, s->counts_dev + 1, pin_dev);
        s->ticket_total += (unsigned long long)tiles;
        launch_relabel(dim3(grid1d(std::max<int64_t>(b.items, table_size(b.items)), kBlock, 4096)), pin_dev + kPinEdges);
        s->clean_items = items;
        HIPCHK(hipGetLastError());
        return COALA_OK;
    });
}

// The frame of the two trace entry points around their own range checks: a kernel on the caller's stream, off the ring.
template <typename Check, typename Launch>
int trace_call(coala_sampler_t* s, const int64_t* nodes, int64_t n, const int64_t* traces_out, Check&& check_ranges, Launch&& launch) {
    if (!s || (n > 0 && (!nodes || !traces_out))) return fail(COALA_EINVAL, "null argument");
    if (n < 0 || n > 0x7FFFFFFF) return fail(COALA_EINVAL, "bad node count");
    if (int rc = check_ranges()) return rc;
    if (n == 0) return COALA_OK;
    HIPCHK(hipSetDevice(s->device));
    launch();
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

} // namespace

extern "C" {

int coala_sampler_edge_batch(coala_sampler_t* s, const int64_t* eids, int64_t n, int num_neg, uint64_t seed, uint64_t step,
                             const coala_edge_batch_t* out, int64_t* ticket_out, void* stream) {
    if (!s || !out || (!eids && n > 0)) return fail(COALA_EINVAL, "null argument");
    if (num_neg < 0 || num_neg > kMaxNeg) return fail(COALA_EINVAL, "num_neg %d outside 0..%d", num_neg, kMaxNeg);
    if (n < 0 || n > kItemLimit) return fail(COALA_EINVAL, "bad edge count");
    const int64_t items = n * (2 + num_neg);
    if (items > kItemLimit)
        return fail(COALA_EINVAL, "an edge batch of %lld edges and %d negatives each holds %lld items (limit %lld)", (long long)n, num_neg,
                    (long long)items, (long long)kItemLimit);
    if (n > 0 && (!out->seed_nodes || !out->pos_src || !out->pos_dst || (num_neg > 0 && !out->neg_dst))) return fail(COALA_EINVAL, "null buffer");
    hipStream_t st = (hipStream_t)stream;
    return item_batch(s, ItemBatch{Holds::edge_batch, items, st, out->seed_nodes, ticket_out},
        [&] {
            hipLaunchKernelGGL(edge_items_kernel, dim3(grid1d(items, kBlock, 8192)), dim3(kBlock), 0, st, s->g, s->num_edges, eids, n, num_neg, seed,
                               step, s->nbr_global, s->tb, s->slot_of_item, s->edge_bad);
        },
        [&](dim3 grid, int64_t* n_bad_pin) {
            hipLaunchKernelGGL(edge_relabel_clear_kernel, grid, dim3(kBlock), 0, st, n, num_neg, (const uint32_t*)s->slot_of_item, s->tb, out->pos_src,
                               out->pos_dst, out->neg_dst, s->edge_bad, n_bad_pin, items);
        });
}

int coala_sampler_edge_batch_wait(coala_sampler_t* s, int64_t ticket, int64_t* n_nodes_host, int64_t* n_bad_host) {
    return batch_wait(s, ticket, Holds::edge_batch, n_nodes_host, n_bad_host);
}

int coala_sampler_create(int device, const int64_t* indptr, const int64_t* indices, int64_t num_nodes, int64_t num_edges,
                         coala_sampler_t** out) {
    if (!out || !indptr || !indices || num_nodes <= 0 || num_edges < 0) return fail(COALA_EINVAL, "bad sampler arguments");
    HIPCHK(hipSetDevice(device));
    coala_sampler* s = new (std::nothrow) coala_sampler();
    if (!s) return fail(COALA_ENOMEM, "out of host memory");
    s->device = device;
    s->g = Graph{indptr, indices, num_nodes};
    s->num_edges = num_edges;
    s->hub_cap = std::min<int64_t>(num_nodes, num_edges / (kHubDegree + 1));
    auto zeroed = [](auto** p, size_t n) { return hipMalloc((void**)p, n * sizeof(**p)) == hipSuccess && hipMemset(*p, 0, n * sizeof(**p)) == hipSuccess; };
    bool ok = zeroed(&s->status, kMaxTiles) && zeroed(&s->ticket, 1) && zeroed(&s->counts_dev, kCountsWords) &&
              zeroed(&s->hub_count, COALA_SAMPLER_MAX_LAYERS) && zeroed(&s->edge_bad, 1) &&
              (s->hub_cap == 0 || hipMalloc((void**)&s->hubs, (size_t)s->hub_cap * sizeof(int64_t)) == hipSuccess) &&
              hipHostMalloc((void**)&s->counts_pinned, kRing * kSlot * sizeof(int64_t), hipHostMallocMapped) == hipSuccess &&
              hipHostGetDevicePointer((void**)&s->counts_pinned_dev, s->counts_pinned, 0) == hipSuccess;
    for (int i = 0; i < kRing && ok; ++i) ok = hipEventCreateWithFlags(&s->done[i], hipEventDisableTiming) == hipSuccess;
    if (!ok || hipDeviceSynchronize() != hipSuccess) {
        coala_sampler_destroy(s);
        return fail(COALA_ENOMEM, "sampler set-up failed: %s", hipGetErrorString(hipGetLastError()));
    }
    *out = s;
    return COALA_OK;
}

int coala_sampler_destroy(coala_sampler_t* s) {
    if (!s) return COALA_OK;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    void* ptrs[] = {s->nbr_global, s->tb.keys, s->tb.local_of_slot, s->slot_of_item, s->wave_counts, s->new_of_old, s->status, s->ticket, s->counts_dev,
                     s->hubs, s->hub_count, s->edge_bad};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (s->counts_pinned) (void)hipHostFree(s->counts_pinned);
    for (int i = 0; i < kRing; ++i)
        if (s->done[i]) (void)hipEventDestroy(s->done[i]);
    delete s;
    return COALA_OK;
}

int coala_sampler_wait(coala_sampler_t* s, int64_t ticket, int64_t* n_src_host, int64_t* bucket_counts_host) {
    return wait_impl(s, ticket, n_src_host, nullptr, bucket_counts_host);
}

int coala_sampler_wait_layers(coala_sampler_t* s, int64_t ticket, int64_t* n_src_host, int64_t* n_edges_host, int64_t* bucket_counts_host) {
    return wait_impl(s, ticket, n_src_host, n_edges_host, bucket_counts_host);
}

int coala_sampler_sample(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                         uint64_t seed, uint64_t step, int64_t* const* src_nodes_out, int32_t* const* nbr_local_out,
                         int64_t* n_src_host, const coala_sampler_bucketing_t* bucketing, int64_t* ticket_out, void* stream) {
    if (!s || (!seeds && n_seeds > 0) || !fanouts || !src_nodes_out || !nbr_local_out) return fail(COALA_EINVAL, "null argument");
    // fixed fan-outs only, into the dense buffers: cap_{l+1} = cap_l * (f + 1) source nodes, cap_l * f neighbour entries.  sample_impl
    // checks the rest from n_seeds itself; a cap it will refuse (negative, or past the item limit) is clamped so that no product overflows
    coala_sampler_layer_t layers[COALA_SAMPLER_MAX_LAYERS];
    int64_t cap = std::min(std::max<int64_t>(n_seeds, 0), kItemLimit + 1);
    for (int l = 0; l < n_layers && l < COALA_SAMPLER_MAX_LAYERS; ++l) {
        const int f = fanouts[l];
        if (f < 1 || f > 32) return fail(COALA_EINVAL, "fan-out %d outside 1..32", f);
        layers[l] = coala_sampler_layer_t{src_nodes_out[l], nbr_local_out[l], nullptr, cap * (f + 1), cap * f};
        cap = std::min(cap * (f + 1), kItemLimit + 1);
    }
    return sample_impl(s, Call{Kind::uniform, seeds, n_seeds, fanouts, n_layers, seed, step, layers, nullptr, n_src_host, nullptr, bucketing, ticket_out,
                               (hipStream_t)stream});
}

int coala_sampler_sample_layers(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts, int n_layers, uint64_t seed,
                                uint64_t step, const coala_sampler_layer_t* layers, int64_t* n_src_host, int64_t* n_edges_host,
                                const coala_sampler_bucketing_t* bucketing, int64_t* ticket_out, void* stream) {
    return coala_sampler_sample_layers_edge_ids(s, seeds, n_seeds, fanouts, n_layers, seed, step, layers, nullptr, nullptr, n_src_host, n_edges_host,
                                                bucketing, ticket_out, stream);
}

int coala_sampler_sample_layers_weighted(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                                         uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, const float* edge_weights,
                                         int64_t* n_src_host, int64_t* n_edges_host, const coala_sampler_bucketing_t* bucketing,
                                         int64_t* ticket_out, void* stream) {
    if (!edge_weights) return fail(COALA_EINVAL, "null edge_weights");
    return coala_sampler_sample_layers_edge_ids(s, seeds, n_seeds, fanouts, n_layers, seed, step, layers, edge_weights, nullptr, n_src_host,
                                                n_edges_host, bucketing, ticket_out, stream);
}

int coala_sampler_sample_layers_edge_ids(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                                         uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, const float* edge_weights,
                                         int64_t* const* edge_ids_out, int64_t* n_src_host, int64_t* n_edges_host,
                                         const coala_sampler_bucketing_t* bucketing, int64_t* ticket_out, void* stream) {
    Call c{edge_weights ? Kind::weighted : Kind::uniform, seeds, n_seeds, fanouts, n_layers, seed, step, layers, edge_ids_out, n_src_host, n_edges_host,
           bucketing, ticket_out, (hipStream_t)stream};
    c.weights = edge_weights;
    return sample_impl(s, c);
}

int coala_sampler_sample_layers_labor(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                                      uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, int64_t* const* edge_ids_out,
                                      int layer_dependency, int64_t* n_src_host, int64_t* n_edges_host,
                                      const coala_sampler_bucketing_t* bucketing, int64_t* ticket_out, void* stream) {
    Call c{Kind::labor, seeds, n_seeds, fanouts, n_layers, seed, step, layers, edge_ids_out, n_src_host, n_edges_host, bucketing, ticket_out,
           (hipStream_t)stream};
    c.layer_dependency = layer_dependency != 0;
    return sample_impl(s, c);
}

int coala_sampler_sample_layers_rel(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* rel_fanouts, int num_rels,
                                    int n_layers, uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, const int32_t* etype,
                                    int64_t* const* edge_ids_out, int64_t* n_src_host, int64_t* n_edges_host,
                                    const coala_sampler_bucketing_t* bucketing, int64_t* ticket_out, void* stream) {
    if (!rel_fanouts) return fail(COALA_EINVAL, "null argument");
    if (!etype) return fail(COALA_EINVAL, "null etype");
    if (num_rels < 1 || num_rels > kMaxRels) return fail(COALA_EINVAL, "num_rels must be 1..%d", kMaxRels);
    if (int rc = check_n_layers(n_layers)) return rc;
    RelFan fan[COALA_SAMPLER_MAX_LAYERS] = {};
    int32_t kind[COALA_SAMPLER_MAX_LAYERS]; // what the rest of the call needs of a layer: -1 (all -1: the full layer), else 0
    for (int l = 0; l < n_layers; ++l) {
        fan[l].num_rels = num_rels;
        bool all_full = true, some = false;
        for (int r = 0; r < num_rels; ++r) {
            const int f = rel_fanouts[(size_t)l * num_rels + r];
            if (f < -1 || f > 32) return fail(COALA_EINVAL, "layer %d, relation %d: fan-out %d outside 0..32 (or -1: every in-edge)", l, r, f);
            fan[l].f[r] = (int8_t)f;
            all_full = all_full && f == kFull;
            some = some || f != 0;
        }
        if (!some) return fail(COALA_EINVAL, "layer %d: every relation has fan-out 0", l);
        kind[l] = all_full ? kFull : 0;
    }
    Call c{Kind::rel, seeds, n_seeds, kind, n_layers, seed, step, layers, edge_ids_out, n_src_host, n_edges_host, bucketing, ticket_out,
           (hipStream_t)stream};
    c.rel = fan;
    c.etype = etype;
    return sample_impl(s, c);
}

int coala_sampler_sample_layers_walk(coala_sampler_t* s, const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                                     uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, const coala_sampler_walk_t* walk,
                                     int32_t* const* visit_counts_out, int64_t* n_src_host, int64_t* n_edges_host,
                                     const coala_sampler_bucketing_t* bucketing, int64_t* ticket_out, void* stream) {
    if (!fanouts || !layers || !walk) return fail(COALA_EINVAL, "null argument");
    if (int rc = check_n_layers(n_layers)) return rc;
    const int T = walk->num_traversals, W = walk->num_random_walks;
    if (T < 1 || T > kMaxWalkLength) return fail(COALA_EINVAL, "num_traversals %d outside 1..%d", T, kMaxWalkLength);
    if (W < 1 || W > kMaxWalks) return fail(COALA_EINVAL, "num_random_walks %d outside 1..%d", W, kMaxWalks);
    if (W * T > kMaxVisits) return fail(COALA_EINVAL, "num_random_walks * num_traversals = %d: over the limit of %d visits", W * T, kMaxVisits);
    if (walk->term_threshold >= kWalkThresholdMax) return fail(COALA_EINVAL, "term_threshold must be below 2^53 (termination_prob < 1)");
    if (int rc = check_fixed_layers(fanouts, layers, n_layers, "walk", "keeps 1..32 neighbours")) return rc;
    Call c{Kind::walk, seeds, n_seeds, fanouts, n_layers, seed, step, layers, nullptr, n_src_host, n_edges_host, bucketing, ticket_out,
           (hipStream_t)stream};
    c.walk = WalkParams{T, W, walk->term_threshold};
    c.visit_counts = visit_counts_out;
    return sample_impl(s, c);
}

int coala_sampler_sample_layers_temporal(coala_sampler_t* s, const int64_t* seed_codes, int64_t n_seeds, const int32_t* fanouts, int n_layers,
                                         uint64_t seed, uint64_t step, const coala_sampler_layer_t* layers, const int64_t* edge_ts,
                                         const int64_t* slot_time, int64_t n_slots, int strategy, int inclusive, int64_t* const* edge_ids_out,
                                         int64_t* n_src_host, int64_t* n_edges_host, int64_t* ticket_out, void* stream) {
    if (!fanouts || !layers) return fail(COALA_EINVAL, "null argument");
    if (!edge_ts) return fail(COALA_EINVAL, "null edge_ts");
    if (int rc = check_n_layers(n_layers)) return rc;
    if (strategy != 0 && strategy != 1) return fail(COALA_EINVAL, "strategy %d: 0 (uniform) or 1 (last)", strategy);
    if (n_slots < 0 || (n_slots > 0 && !slot_time)) return fail(COALA_EINVAL, "slot_time: %lld query times and a null table", (long long)n_slots);
    if (int rc = check_fixed_layers(fanouts, layers, n_layers, "temporal", "has a fixed fan-out")) return rc;
    if (!s) return fail(COALA_EINVAL, "null argument");
    int node_bits = 0, slot_bits = 0; // bit lengths of num_nodes and of n_slots - 1
    while ((s->g.num_nodes >> node_bits) != 0) ++node_bits;
    while (n_slots > 1 && ((n_slots - 1) >> slot_bits) != 0) ++slot_bits;
    if (node_bits + slot_bits > 62)
        return fail(COALA_EINVAL, "%lld query times on a graph of %lld nodes: a (node, time) pair takes %d + %d bits, over the 62 of a code",
                    (long long)n_slots, (long long)s->g.num_nodes, node_bits, slot_bits);
    const Temporal tp{edge_ts, slot_time, n_slots, node_bits, strategy == 1, inclusive != 0};
    Call c{Kind::temporal, seed_codes, n_seeds, fanouts, n_layers, seed, step, layers, edge_ids_out, n_src_host, n_edges_host, nullptr, ticket_out,
           (hipStream_t)stream};
    c.temporal = &tp;
    return sample_impl(s, c);
}

int coala_sampler_random_walk(coala_sampler_t* s, const int64_t* nodes, int64_t n, int num_walks, int length, uint64_t term_threshold,
                              uint64_t seed, uint64_t step, int layer, int64_t* traces_out, void* stream) {
    auto check_ranges = [&] {
        if (num_walks < 1 || num_walks > kMaxWalks) return fail(COALA_EINVAL, "num_walks %d outside 1..%d", num_walks, kMaxWalks);
        if (length < 1 || length > kMaxWalkLength) return fail(COALA_EINVAL, "length %d outside 1..%d", length, kMaxWalkLength);
        if (term_threshold >= kWalkThresholdMax) return fail(COALA_EINVAL, "term_threshold must be below 2^53 (restart_prob < 1)");
        if (layer < 0 || layer >= COALA_SAMPLER_MAX_LAYERS) return fail(COALA_EINVAL, "layer must be 0..%d", COALA_SAMPLER_MAX_LAYERS - 1);
        return COALA_OK;
    };
    return trace_call(s, nodes, n, traces_out, check_ranges, [&] {
        hipLaunchKernelGGL(walk_trace_kernel, dim3(grid1d(n * num_walks, kBlock, 8192)), dim3(kBlock), 0, (hipStream_t)stream, s->g, nodes, n,
                           WalkParams{length, num_walks, term_threshold}, seed, step, layer, traces_out);
    });
}

// The three thresholds of a second-order walk: each in [0, 2^32], the largest exactly 2^32 (the host normalises by max(1/p, 1, 1/q)).
static int check_n2v(int num_walks, int length, uint64_t thr_ret, uint64_t thr_near, uint64_t thr_far) {
    if (num_walks < 1 || num_walks > kMaxWalks) return fail(COALA_EINVAL, "num_walks %d outside 1..%d", num_walks, kMaxWalks);
    if (length < 1 || length > kN2vMaxLength) return fail(COALA_EINVAL, "walk_length %d outside 1..%d", length, kN2vMaxLength);
    if (std::max(thr_ret, std::max(thr_near, thr_far)) != kN2vOne)
        return fail(COALA_EINVAL, "thresholds %llu, %llu, %llu: each in [0, 2^32] and the largest 2^32", (unsigned long long)thr_ret,
                    (unsigned long long)thr_near, (unsigned long long)thr_far);
    return COALA_OK;
}

int coala_sampler_node2vec_walk(coala_sampler_t* s, const int64_t* nodes, int64_t n, int num_walks, int length, uint64_t thr_return,
                                uint64_t thr_near, uint64_t thr_far, uint64_t seed, uint64_t step, int64_t* traces_out, void* stream) {
    return trace_call(s, nodes, n, traces_out, [&] { return check_n2v(num_walks, length, thr_return, thr_near, thr_far); }, [&] {
        hipLaunchKernelGGL(node2vec_trace_kernel, dim3(grid1d(n * num_walks * kN2vGroup, kBlock, 8192)), dim3(kBlock), 0, (hipStream_t)stream, s->g, nodes,
                           n, N2vParams{length, num_walks, thr_return, thr_near, thr_far}, seed, step, traces_out);
    });
}

int coala_sampler_walk_batch(coala_sampler_t* s, const int64_t* nodes, int64_t n, int num_walks, int length, uint64_t thr_return,
                             uint64_t thr_near, uint64_t thr_far, int num_neg, uint64_t seed, uint64_t step, const coala_walk_batch_t* out,
                             int64_t* ticket_out, void* stream) {
    if (!s || !out || (!nodes && n > 0)) return fail(COALA_EINVAL, "null argument");
    if (int rc = check_n2v(num_walks, length, thr_return, thr_near, thr_far)) return rc;
    if (num_neg < 0 || num_neg > kN2vMaxNeg) return fail(COALA_EINVAL, "num_neg %d outside 0..%d", num_neg, kN2vMaxNeg);
    if (n < 0 || n > kItemLimit) return fail(COALA_EINVAL, "bad node count");
    const int64_t stated = n * num_walks * (length + 1) * (1 + num_neg); // the documented bound; the item list itself holds n more at num_neg 0
    const int64_t items = walk_batch_items(n, num_walks, length, num_neg);
    if (stated > kItemLimit || items > kItemLimit)
        return fail(COALA_EINVAL, "a walk batch of %lld start nodes, %d walks of %d hops and %d negatives holds %lld items (limit %lld)",
                    (long long)n, num_walks, length, num_neg, (long long)std::max(stated, items), (long long)kItemLimit);
    if (n > 0 && (!out->input_nodes || !out->pos || (num_neg > 0 && !out->neg))) return fail(COALA_EINVAL, "null buffer");
    hipStream_t st = (hipStream_t)stream;
    return item_batch(s, ItemBatch{Holds::walk_batch, items, st, out->input_nodes, ticket_out},
        [&] {
            const N2vParams np{length, num_walks, thr_return, thr_near, thr_far};
            const int64_t n_walks = n * num_walks;
            hipLaunchKernelGGL(walk_items_kernel, dim3(grid1d(std::max<int64_t>(n_walks * kN2vGroup, n_walks * num_neg * length / 4), kBlock, 8192)),
                               dim3(kBlock), 0, st, s->g, nodes, n, np, num_neg, seed, step, s->nbr_global, out->traces, s->tb, s->slot_of_item, s->edge_bad);
        },
        [&](dim3 grid, int64_t* n_bad_pin) {
            hipLaunchKernelGGL(walk_relabel_clear_kernel, grid, dim3(kBlock), 0, st, n, num_walks, length, num_neg, (const uint32_t*)s->slot_of_item, s->tb,
                               out->pos, out->neg, s->edge_bad, n_bad_pin, items);
        });
}

int coala_sampler_walk_batch_wait(coala_sampler_t* s, int64_t ticket, int64_t* n_nodes_host, int64_t* n_bad_host) {
    return batch_wait(s, ticket, Holds::walk_batch, n_nodes_host, n_bad_host);
}

} // extern "C"
