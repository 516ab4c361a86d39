// coala_cache.hip -- MI355X (gfx950 / CDNA4) feature cache: probe + hit gather, deterministic miss ranking, cold fill,
// owner routing and un-permute.  Hand-written HIP, wave64.  C ABI in include/coala_hip.h.
//
// Replaces (paths relative to /root/reference/COALA_GNN_Modules):
//   isolated_cache.h:335-475 get_data, :145-174 search_ways, :36-50 iso_warp_memcpy, :323-331 read_page_simulation
//   nvshmem_cache.h:336-480 (same table, distributed set index), seqlock.h (not needed: batch-synchronous design)
//   cache_kernel.cu:59-77 / :93-111 / :38-57 read kernels, :79-91 split, :113-137 gather, :139-143 stats
//   ssd_gnn_cache.cuh:84-109,227-360 host front-ends
//
// Design (DESIGN.md has the long form).  One call = one batch, two stream-ordered kernels, no same-address atomics:
//   K1 probe_gather : a wave takes R rows (4, or 8 for 512-B lines) per step of a grid-stride loop.  One 16-B load per
//                     lane fetches the 32 tags of eight sets at once (8 lanes x 4 tags of 32 bits per set; four sets of
//                     16 lanes x 2 tags with the reference's 64-bit tags); every lane ranks its own tags and a DPP minimum
//                     over the lanes of a row gives the lowest matching way -- all rows at once, nothing extracted row by
//                     row; hits are copied HBM line -> output row with nontemporal 16-B loads / plain stores, 4 row(-pair)s
//                     in flight per wave, with the next chunk's ids/tags prefetched behind them.  A miss is pushed on its
//                     set's chain (ONE atomicExch on the set's own head word, tagged with the batch generation so no
//                     clearing pass is needed); every row's verdict + chain link is one 4-byte word written per position.  For a whole
//                     read on a host tier the missed positions are also appended to the batch's miss list (64 lists, one atomic per chunk).
//   K2 miss_fill    : same chunking (ranged fills, HBM tier: verdict tiles; whole reads on a host tier: groups of R entries of the miss
//                     list, cold rows requested before the ranking).  For a missed row one lane walks the set's chain and counts the misses that precede
//                     it in batch order: its rank k.  way = (set_cnt_before + k) % 32 -- the reference's round robin
//                     executed in batch order, for any arrival order of the atomics; the first-ranked miss of a set advances
//                     the set's cursor (a generation-tagged 64-bit word, so that late readers still recover the value
//                     before the batch).  The last writer of a way (the
//                     "winner") publishes key, colour and line; every miss streams its row from the cold tier (pinned
//                     host over PCIe, or HBM) into the output.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/coala_hip.h"
#include "coala_internal.h"
#include "coala_partition.h"

namespace {

constexpr uint64_t kEmptyKey = 0xFFFFFFFFFFFFFFFFull; // isolated_cache.h:552
constexpr uint32_t kLinkMiss = 0x80000000u;            // miss_link: a miss (low 31 bits = chain link)
constexpr uint32_t kLinkBad = 0x7FFFFFFFu;             // miss_link: id outside [0, num_rows)
constexpr int kStatBlocks = 2048;                      // upper bound of K2's grid
constexpr int kFillSlots = 8;                          // fill launches of one batch that can deal their tiles dynamically (a ticket counter each, two batches' worth)

struct CacheDev {
    void* keys;            // [sets*32] tags: uint32_t when every id fits 32 bits (tag32: a set is ONE 128-B line), else uint64_t (256 B)
    uint64_t* set_cnt;     // [sets] : (gen << 32) | round-robin cursor.  gen == the current batch's generation: the cursor already
                           //          includes this batch's misses (K2 advanced it), otherwise it is the value before the batch
    uint32_t* color_meta;  // [sets*32]
    int32_t* color_counters; // [num_colors+1] or null
    const int32_t* node_color; // [num_rows] device copy or null
    float* lines;          // [sets*32*cache_dim]
    const float* cold;     // [num_rows*dim]
    uint64_t num_sets;
    uint64_t num_rows;
    uint32_t cache_dim;
    uint32_t dim;
    uint32_t n_gpus;
    int32_t gshift;        // log2(n_gpus) if power of two else -1
    int32_t sshift;        // log2(num_sets) if power of two else -1
    uint32_t distributed;
    uint32_t cold_partitioned; // cold row of id = id / n_gpus
    uint32_t tag32;            // 1: 32-bit tags (num_rows <= 2^32-1, empty = 0xFFFFFFFF); 0: 64-bit tags as in the reference
    // per-batch scratch, indexed by the row's POSITION in the batch (ranking never needs a compacted list; streaming may use one: miss_list)
    uint64_t* set_head;    // [sets] : (gen << 32) | (position + 1) of the most recently pushed miss of this set
    uint32_t* miss_link;   // [cap] K1's verdict for every position of the batch, rewritten by every probe (nothing to clear):
                           //       0 = hit, kLinkBad = rejected id, kLinkMiss | (position + 1 of the previously pushed miss of the set; 0 = end)
    unsigned long long* stats; // [kStatBlocks][2] running sums owned by K2's blocks: misses, rejected ids
    uint32_t* miss_list;   // [kListShards][list_sub] batch positions of the misses, appended by K1 in arrival order (read by K2's list form)
    uint32_t list_sub;     // entries per shard of miss_list; 0 in the copy a launch gets = this batch keeps no list (its fills are ranged: tile form)
};

// The miss list of a batch (K1 appends, K2's list form streams from it).  One counter for the whole batch would take one returning atomic per
// chunk with a miss on ONE word, and a word takes ~12 ns per atomic whoever sends it: 7 k chunks = 80 us under a 17-us probe.  So the list is
// kListShards lists, chunk k appends to list k % kListShards, and every counter has a 256-B stretch of its own; K2 reads all the counters with
// one load per lane and walks the lists as one dense index space through their prefix sums.  A shard holds the misses of at most
// ceil(chunks / kListShards) chunks of up to 32 rows: list_sub = cap / kListShards + 32 entries.
constexpr int kListShards = 64;        // = the lanes of a wave (K2's prefix sum)
constexpr int kListStride = 64;        // uint32_t words between two counters
// CacheDev::stats in 64-bit words: K2's per-block sums, its ticket counters (2 x kFillSlots x 4 B) and the two "something to fill" flags, then
constexpr int kStatWriteBad = 2 * kStatBlocks + kFillSlots + 1;   // rejected ids of the write kernel
constexpr int kStatProbeBad = kStatWriteBad + 1;                  // rejected ids of the batches that keep a list (K1 counts them: K2's list form never sees them)
constexpr int kStatHostWords = kStatProbeBad + 1;                 // what coala_cache_stats reads back
constexpr int kStatList = (kStatHostWords + 31) & ~31;            // the list counters: [2 parities of the generation][kListShards], kListStride words apart
constexpr int kStatWords = kStatList + 2 * kListShards * kListStride / 2;
__device__ __forceinline__ uint32_t* list_counter(const CacheDev& c, uint32_t parity, uint32_t shard) {
    return reinterpret_cast<uint32_t*>(c.stats + kStatList) + (parity * kListShards + shard) * kListStride;
}

__device__ __forceinline__ uint64_t set_of(const CacheDev& c, uint64_t id) {
    // isolated_cache.h:183-195 ; nvshmem_cache.h:191-196
    uint64_t k = id;
    if (c.distributed) {
        if (c.gshift >= 0) k = id >> c.gshift;
        else if ((id >> 32) == 0) k = (uint32_t)id / c.n_gpus;
        else k = id / c.n_gpus;
    }
    if (c.sshift >= 0) return k & (c.num_sets - 1);
    if ((k >> 32) == 0 && (c.num_sets >> 32) == 0) return (uint32_t)k % (uint32_t)c.num_sets;
    return k % c.num_sets;
}

__device__ __forceinline__ uint64_t cold_row_of(const CacheDev& c, uint64_t id) {
    if (!c.cold_partitioned) return id;
    if (c.gshift >= 0) return id >> c.gshift;
    return id / c.n_gpus;
}

// A union of disjoint batch-position ranges walked as one dense "virtual" index space (a serve split into several fills, a
// row exchange split into rounds: every round touches one slice of every peer's segment).  Lives in the kernarg segment.
constexpr int kMaxRanges = 64;
struct RangeSet {
    uint32_t n;                      // ranges in use
    uint32_t total;                  // rows in all ranges
    uint32_t begin[kMaxRanges];      // first position of range k
    uint32_t vstart[kMaxRanges + 1]; // exclusive prefix sums of the range lengths
};
// position of virtual row v (0xFFFFFFFF past the end).  Uniform trip count: the table is read with scalar loads.
__device__ __forceinline__ uint32_t pos_of(const RangeSet& rs, uint32_t v) {
    if (rs.n == 1) return v < rs.total ? rs.begin[0] + v : 0xFFFFFFFFu;
    uint32_t pos = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < rs.n; ++k) {
        const uint32_t a = rs.vstart[k], b = rs.vstart[k + 1];
        if (v >= a && v < b) pos = rs.begin[k] + (v - a);
    }
    return pos;
}
// Batch positions [begin, end) are delivered to out[row_map[pos - begin]] of ANOTHER buffer instead of row pos of the batch's
// own output: the requester's own shard of a distributed fetch goes straight into the caller's tensor, bypassing the exchange.
struct Redirect {
    int64_t begin, end;
    float* out;
    const int64_t* row_map; // null: row pos - begin
};

template <int CTRL> __device__ __forceinline__ uint32_t dpp_u32(uint32_t v) { // v of the lane the DPP control names (all lanes active)
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);   // (this form folds into the consuming v_min_u32: one instruction per step)
}
__device__ __forceinline__ uint32_t umin_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int src_lane) {
    uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, src_lane);
    uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src_lane);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// native clang vectors (not HIP's float4 struct) so the in-flight rows stay in VGPRs
typedef float vfloat4 __attribute__((ext_vector_type(4)));
typedef unsigned long long vu64x2 __attribute__((ext_vector_type(2)));
typedef unsigned int vu32x4 __attribute__((ext_vector_type(4)));

// How a wave reads tag sets: every lane loads 16 B.  The reference keeps 64-bit tags (isolated_cache.h:552: a set is 32 x 8 B = two
// 128-B lines, 16 lanes x 2 tags per set, 4 sets per wave-wide load).  No dataset the reference runs has 2^32 nodes, so whenever
// num_rows < 2^32 the table holds 32-bit tags instead: a set is ONE 128-B line (8 lanes x 4 tags, 8 sets per wave-wide load) -- half the
// probe bytes and half the random HBM lines per probed row.  coala_cache_dump widens them again, so the table state stays comparable
// with the oracle's bit for bit.
template <typename TAG> struct TagGeo;
template <> struct TagGeo<uint64_t> {
    using vec = vu64x2;
    static constexpr int KPL = 2;   // tags per lane
    static constexpr int LPS = 16;  // lanes per set
    static constexpr int SPL = 4;   // sets per wave-wide load
    static constexpr uint64_t EMPTY = 0xFFFFFFFFFFFFFFFFull;
};
template <> struct TagGeo<uint32_t> {
    using vec = vu32x4;
    static constexpr int KPL = 4;
    static constexpr int LPS = 8;
    static constexpr int SPL = 8;
    static constexpr uint32_t EMPTY = 0xFFFFFFFFu;
};
template <int VEC> struct VecT;
template <> struct VecT<4> { using type = vfloat4; };
template <> struct VecT<1> { using type = float; };

// Geometry of the row movers.  VEC = floats per lane access (4 -> 16-B accesses; 1 -> fallback for dim % 4 != 0).
template <int CD, int VEC, int NP = 4>
struct Geo {
    static constexpr int UNITS = CD / VEC;                    // accesses per full line
    static constexpr int LPR = UNITS >= 64 ? 64 : UNITS;      // lanes per row
    static constexpr int RPP = 64 / LPR;                      // rows per pass (2 for 512-B lines with 16-B accesses)
    static constexpr int VPL = UNITS / LPR;                   // accesses per lane per row
    static constexpr int PASSES = (VPL >= 16) ? 1 : NP;       // rows(-pairs) in flight per wave
    static constexpr int R = RPP * PASSES;                    // rows per chunk
};

// ---------------------------------------------------------------------------------------------------------- K1
// Probe R rows, copy the hits, mark the misses.  Software-pipelined over a wave's chunks: the ids of chunk k+2 and the
// tag sets of chunk k+1 are requested while the rows of chunk k are in flight, so a wave never sits on the
// id -> tag -> line dependency chain with nothing outstanding.  Lines and output rows are touched once per batch:
// nontemporal loads/stores keep them from displacing the tag sets in L2.
// Every per-miss record of the ranking is indexed by the row's position in the batch, and the per-set chain
// that K2 walks is pushed with one atomicExch on the set's own head word.  (Measured alternatives: a miss-list append
// per chunk or per wave on ONE counter serialises at ~12 ns per same-address atomic -- 4096 waves = 49 us, as long as the whole hit
// gather; a block-level append needs LDS staging and a trailing barrier and still costs 5-7 us.  The list K2's list form
// streams from is therefore kListShards lists with a counter each: ~110 atomics per counter on the default workload.)
constexpr int kK1MinWaves = 4; // waves per SIMD the register allocator must leave room for (5 on 4-KiB lines spills: 17.5 -> 20.9 us on the default workload)
// Row(-pair)s a wave keeps in flight (passes): 4 for every line size and both tag widths = 16 KiB of 4-KiB lines, 4 KiB of 512-B lines
// (8 rows).  More passes on short lines were measured in situ on the configs[3] shape (512-B lines, 16 GiB cache, 315 k rows per
// minibatch at 62 % hits; tools/k1_insitu.py, profiles/r03_k1_insitu_papers100m.txt): 2 / 4 / 8 / 16 passes -> 51.2 / 51.0 / 53.4 /
// (72 k rows) 44.5 us: a launch of this size is one chunk per wave, so its waves overlap each other, not their own chunks, and fewer,
// fatter waves lose more parallelism than they gain bytes in flight.
constexpr int kK1Passes = 4;
constexpr int64_t kK1SingleMaxChunks = 1 << 20; // launches up to this many chunks (4-8 M rows) get one wave per chunk (SINGLE)
constexpr int kK1Waves = 2; // waves per block (measured: 2048 x 128 threads beats 1024 x 256 and 256 x 1024 by 3-20 %)
#ifdef COALA_DEV_KNOBS          // development builds only (build.py --dev -> libcoala_hip_dev.so): launch geometry from the environment
constexpr int kK1MaxWaves = 4;
#else
constexpr int kK1MaxWaves = kK1Waves;
#endif

template <typename V> __device__ __forceinline__ V nt_load(const V* p) { return __builtin_nontemporal_load(p); }
template <typename V> __device__ __forceinline__ void nt_store(V v, V* p) { __builtin_nontemporal_store(v, p); }

// K1's row moves: nontemporal loads of the lines (touched once per batch: keeps them from displacing the tag sets; plain loads are
// 3 us slower on an all-hit batch and no faster at 32 % hits -- 17.4 us either way in situ, as is a per-chunk choice between the two), plain stores of the output rows (0.3-0.4 us faster than
// nontemporal ones in situ and on the all-hit batch, and the consumer reads them next).
// SINGLE: the grid has one wave per chunk (every launch up to kK1SingleMaxChunks chunks): no loop and no prefetch state for later
// chunks, which is what the software pipeline's registers are for (4-KiB lines: 76 instead of 110 VGPRs, 6 instead of 4 waves per SIMD) and
// whose id / tag loads a one-chunk wave issues for chunks it never has.  The product's choice for lines of 1 KiB and more; 512-B lines keep
// the looping kernel (8-row waves gain from the pipeline whenever a wave does run two chunks, and lose nothing when it does not).
// Round 4, the last K1 experiment (profiles/r04_k1_min_waves.txt): on 512-B lines the looping kernel needs 66 VGPRs = 7 waves per SIMD; bounded to 8
// waves the configs[3] variant fits 64 registers without a spill -- and is no faster in the product's block shape: 11.3 against
// 11.4 us at ~72 k rows, 44-48 against 49 us at ~289 k (the development build's 256-thread blocks gained 7 % at 72 k rows).  Not adopted.
template <int CD, int VEC, typename TAG, int NP, bool FULL, bool REDIR, bool SINGLE>
__global__ __launch_bounds__(64 * kK1MaxWaves, kK1MinWaves) void probe_gather_kernel(const int64_t* __restrict__ idx, float* __restrict__ out,
                                                                    int64_t n, uint32_t gen, uint32_t n_blocks, CacheDev c, Redirect rd) {
    // Argument order and the explicit block count are deliberate: with kernarg preloading (build.py: -mllvm -amdgpu-kernarg-preload-count=16)
    // the leading scalar arguments arrive in SGPRs, and with the compile-time block shape the first id load needs nothing from
    // the kernarg segment -- the s_loads of the CacheDev fields then overlap that load instead of preceding it.
    // FULL: dim == cache_dim, every lane of a row group moves data -> no per-lane bounds predicate around the row moves
    // REDIR: rows at positions [rd.begin, rd.end) go to rd.out[rd.row_map[..]] (own shard of a distributed fetch); the
    //        destination row travels with the id through the software pipeline, so no load sits in front of the stores
    using G = Geo<CD, VEC, NP>;
    using V = typename VecT<VEC>::type;
    using TG = TagGeo<TAG>;
    using TV = typename TG::vec;
    constexpr int R = G::R;
    static_assert(R <= 32, "per-chunk row masks are 32 bits wide");
    // the ticket counters of THIS batch's fill launches (K2's dynamic deal): the probe comes before every one of them, and the counters of this
    // parity were last used two batches ago
    if (blockIdx.x == 0 && threadIdx.x < kFillSlots) reinterpret_cast<uint32_t*>(c.stats + 2 * kStatBlocks)[(gen & 1u) * kFillSlots + threadIdx.x] = 0u;
    // ... and "this batch has something to fill" (set below by every wave that finds a miss or a rejected id): the flag of the NEXT batch's parity is
    // cleared here -- its last readers, the fills of the batch before this one, are done -- and this batch's was cleared by the previous probe
    uint32_t* fill_flag = reinterpret_cast<uint32_t*>(c.stats + 2 * kStatBlocks) + 2 * kFillSlots;
    if (blockIdx.x == 0 && threadIdx.x == kFillSlots) fill_flag[(gen + 1u) & 1u] = 0u;
    // ... and the miss-list counters: this batch adds to the ones of its own parity and clears the next batch's, which the fill of the batch
    // before this one was the last to read
    if (blockIdx.x == 0 && threadIdx.x < kListShards) *list_counter(c, (gen + 1u) & 1u, threadIdx.x) = 0u;
    constexpr int TSTEPS = (R + TG::SPL - 1) / TG::SPL; // tag loads per chunk: SPL sets per wave-wide 16-B load (LPS lanes x KPL tags per set)
    int lane = threadIdx.x & 63;
#ifdef COALA_DEV_KNOBS
    const int wpb = (int)(blockDim.x >> 6);
#else
    constexpr int wpb = kK1Waves;
#endif
    const int64_t wave = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)n_blocks * wpb;
    const int64_t n_chunks = (n + R - 1) / R;
    const uint32_t nunits = c.dim / VEC; // accesses per output row
    const TAG* __restrict__ keys = reinterpret_cast<const TAG*>(c.keys);

    // probe state of one chunk: lane l looks at row q = SPL*t + l/LPS, tags KPL*(l%LPS) .. KPL*(l%LPS)+KPL-1 of that row's set
    struct Ids { uint64_t id[TSTEPS]; bool valid[TSTEPS]; int32_t drow[REDIR ? TSTEPS : 1]; };
    struct Tags { uint64_t id[TSTEPS]; uint32_t set[TSTEPS]; TV kk[TSTEPS]; bool ok[TSTEPS]; bool valid[TSTEPS]; int32_t drow[REDIR ? TSTEPS : 1]; };
    auto load_ids = [&](int64_t chunk) {
        Ids r;
#pragma unroll
        for (int t = 0; t < TSTEPS; ++t) {
            const int q_l = t * TG::SPL + lane / TG::LPS;
            const int64_t i_l = chunk * R + q_l;
            r.valid[t] = (chunk < n_chunks) && (q_l < R) && (i_l < n);
            r.id[t] = r.valid[t] ? (uint64_t)idx[i_l] : 0;
            if (REDIR) { // destination: -1 = row i_l of the batch's own output, v >= 0 = row v of rd.out (a batch has < 2^31 rows)
                int32_t d = -1;
                if (r.valid[t] && i_l >= rd.begin && i_l < rd.end) d = (int32_t)(rd.row_map ? rd.row_map[i_l - rd.begin] : i_l - rd.begin);
                r.drow[t] = d;
            }
        }
        return r;
    };
    auto load_tags = [&](const Ids& ids) {
        Tags r;
#pragma unroll
        for (int t = 0; t < TSTEPS; ++t) {
            r.id[t] = ids.id[t];
            r.valid[t] = ids.valid[t];
            if (REDIR) r.drow[t] = ids.drow[t];
            r.ok[t] = ids.valid[t] && ids.id[t] < c.num_rows;
            r.set[t] = r.ok[t] ? (uint32_t)set_of(c, ids.id[t]) : 0u;
            r.kk[t] = TV(TG::EMPTY);
            if (r.ok[t]) r.kk[t] = *reinterpret_cast<const TV*>(keys + (uint64_t)r.set[t] * COALA_WAYS + (lane % TG::LPS) * TG::KPL);
        }
        return r;
    };

    int64_t chunk = wave;
    Ids ids_next = load_ids(chunk);
    Tags tags = load_tags(ids_next);
    if (!SINGLE) ids_next = load_ids(chunk + n_waves);

    for (; chunk < n_chunks; chunk += n_waves) {
        // (the lane index made opaque once per iteration: otherwise every lane-derived address and constant of the loop is hoisted into a VGPR of its
        //  own -- 72 -> 66 VGPRs on 512-B lines, 81 -> 67 in the redirecting variant: one more wave per SIMD -- for a loop most waves run once)
        asm volatile("" : "+v"(lane));
        const int64_t base = chunk * R;
        // ---- probe, all rows of a tag step at once: every lane ranks its own KPL tags, a DPP minimum over the LPS lanes of a row gives
        //      the lowest matching way (isolated_cache.h:165-172) to each of them, and the row's first lane keeps the books for it.  Nothing
        //      is extracted row by row into scalars (that was ~80 instructions per row: on short lines the launch was bound by instruction
        //      issue, 300 VALU + 340 SALU per 8-row wave -- profiles/r03_k1_sq_counters.txt); the copy loops read a row's slot with one
        //      v_readlane and its status from the ballots.
        uint32_t slot_v[TSTEPS];                // per lane: set*32 + way of the lane's row (meaningful where the row hits)
        int32_t drow_v[REDIR ? TSTEPS : 1];     // per lane: destination row of the lane's row in rd.out, -1 = not redirected
        uint64_t hit_b[TSTEPS], bad_b[TSTEPS];  // ballots: bit l = the row of lane l hits / carries a rejected id
        bool lead_l[TSTEPS], imiss_l[TSTEPS], bad_l[TSTEPS]; // the lane is the first of an existing row's lanes; ... and that row misses; ... is rejected
        unsigned long long prev[TSTEPS];
        const uint32_t lane_way0 = (uint32_t)((lane % TG::LPS) * TG::KPL);
#pragma unroll
        for (int t = 0; t < TSTEPS; ++t) {
            const TAG want = (TAG)tags.id[t];
            uint32_t way = 0xFFu;
#pragma unroll
            for (int k = TG::KPL - 1; k >= 0; --k)
                if (tags.kk[t][k] == want) way = lane_way0 + (uint32_t)k;
            if (!tags.ok[t]) way = 0xFFu; // (an id outside the table may equal the empty tag)
            way = umin_u32(way, dpp_u32<0xB1>(way));   // quad_perm [1,0,3,2]: lane ^ 1
            way = umin_u32(way, dpp_u32<0x4E>(way));   // quad_perm [2,3,0,1]: lane ^ 2
            way = umin_u32(way, dpp_u32<0x141>(way));  // row_half_mirror: the other quad of the 8 lanes
            if (TG::LPS == 16) way = umin_u32(way, dpp_u32<0x140>(way)); // row_mirror: the other half of the 16 lanes
            const bool hit = way != 0xFFu;
            slot_v[t] = tags.set[t] * COALA_WAYS + (way & (COALA_WAYS - 1));
            if (REDIR) drow_v[t] = tags.drow[t];
            hit_b[t] = __ballot(hit);
            bad_l[t] = tags.valid[t] && !tags.ok[t];
            bad_b[t] = __ballot(bad_l[t]);
            lead_l[t] = tags.valid[t] && (lane % TG::LPS) == 0;
            // ---- misses: push the row on its set's chain (the old head comes back behind the row loads)
            imiss_l[t] = lead_l[t] && tags.ok[t] && !hit;
            prev[t] = 0;
            if (imiss_l[t]) {
                const unsigned long long tag = ((unsigned long long)gen << 32) | (unsigned long long)(base + t * TG::SPL + lane / TG::LPS + 1);
                prev[t] = atomicExch(reinterpret_cast<unsigned long long*>(c.set_head + tags.set[t]), tag);
                // (the set's round-robin cursor, isolated_cache.h:203, is advanced by K2: an atomicAdd here cost 1.2 us per launch)
            }
        }
        {   // one store per wave that has work for K2 (a fill launch of a batch without any leaves at once: the steady state of a cache that holds the table)
            bool any = false;
#pragma unroll
            for (int t = 0; t < TSTEPS; ++t) any = any || imiss_l[t] || bad_l[t];
            if (__ballot(any) != 0 && lane == 0) fill_flag[gen & 1u] = 1u;   // (what the flag costs K1: profiles/r04_k2_dynamic_deal.txt)
        }
        // ---- the batch's miss list (a whole read on a host tier): ONE atomic per chunk with misses reserves their slots in the chunk's shard
        //      (the old count comes back behind the row loads; the positions are stored with the verdicts), and rejected ids are counted here
        const uint32_t shard = (uint32_t)chunk & (kListShards - 1);
        uint32_t list_at = 0;   // lane 0: the shard's count before this chunk
        if (c.list_sub) {
            uint32_t n_miss = 0, n_bad = 0;
#pragma unroll
            for (int t = 0; t < TSTEPS; ++t) {
                n_miss += (uint32_t)__builtin_popcountll(__ballot(imiss_l[t]));
                n_bad += (uint32_t)__builtin_popcountll(__ballot(bad_l[t] && lead_l[t]));
            }
            if (n_miss && lane == 0) list_at = atomicAdd(list_counter(c, gen & 1u, shard), n_miss);
            if (n_bad && lane == 0) atomicAdd(c.stats + kStatProbeBad, (unsigned long long)n_bad);
        }
        // row q of the chunk: its tag step, and the first of its lanes there
        auto row_slot = [&](int q) { return (uint32_t)__builtin_amdgcn_readlane((int)slot_v[q / TG::SPL], TG::LPS * (q % TG::SPL)); };
        auto row_hit = [&](int q) { return ((hit_b[q / TG::SPL] >> (TG::LPS * (q % TG::SPL))) & 1) != 0; };
        auto row_bad = [&](int q) { return ((bad_b[q / TG::SPL] >> (TG::LPS * (q % TG::SPL))) & 1) != 0; };
        // ids two chunks ahead (consumed by load_tags in the NEXT iteration: a full row round trip of slack)
        Ids ids_next2;
        if (!SINGLE) ids_next2 = load_ids(chunk + 2 * n_waves);

        // ---- hits: HBM line -> registers -> output row, PASSES row(-pair)s in flight, next chunk's tags requested in between.
        // (Measured alternatives that did not pay: unconditional loads through a dummy address so that the stores get counted
        // vmcnt(N) waits, and a predicate-free second path for all-hit chunks: DESIGN.md section 4.)
        const int sub = (G::RPP == 2) ? (lane >> 5) : 0;
        const int l_in = lane & (G::LPR - 1);
        V val[G::PASSES][G::VPL];
#pragma unroll
        for (int p = 0; p < G::PASSES; ++p) {
            // (both rows of a pass are read out BEFORE the per-lane choice: a readlane inside a divergent ?: becomes a branch per pass)
            const uint32_t s_a = row_slot(p * G::RPP), s_b = row_slot(p * G::RPP + (G::RPP - 1));
            const bool h_a = row_hit(p * G::RPP), h_b = row_hit(p * G::RPP + (G::RPP - 1));
            const uint32_t s = (G::RPP == 2 && sub) ? s_b : s_a;
            const bool h = (G::RPP == 2 && sub) ? h_b : h_a;
            const V* src = reinterpret_cast<const V*>(c.lines + (uint64_t)s * CD);
#pragma unroll
            for (int v = 0; v < G::VPL; ++v) {
                const uint32_t u = v * G::LPR + l_in;
                if (h && (FULL || u < nunits)) val[p][v] = nt_load(src + u);
            }
        }
        if (!SINGLE) {
            tags = load_tags(ids_next);
            ids_next = ids_next2;
        }
#pragma unroll
        for (int p = 0; p < G::PASSES; ++p) {
            const int q = p * G::RPP + sub;
            const bool h_a = row_hit(p * G::RPP), h_b = row_hit(p * G::RPP + (G::RPP - 1));
            const bool bad_a = row_bad(p * G::RPP), bad_b2 = row_bad(p * G::RPP + (G::RPP - 1));
            const bool h = (G::RPP == 2 && sub) ? h_b : h_a;
            const bool bad = (G::RPP == 2 && sub) ? bad_b2 : bad_a;
            V* dst = reinterpret_cast<V*>(out + (base + q) * (int64_t)c.dim);
            if (REDIR) {
                auto row_drow = [&](int r) { return (int32_t)__builtin_amdgcn_readlane(drow_v[r / TG::SPL], TG::LPS * (r % TG::SPL)); };
                const int32_t dr_a = row_drow(p * G::RPP), dr_b = row_drow(p * G::RPP + (G::RPP - 1));
                const int32_t dr = (G::RPP == 2 && sub) ? dr_b : dr_a;
                if (dr >= 0) dst = reinterpret_cast<V*>(rd.out + (int64_t)dr * (int64_t)c.dim);
            }
#pragma unroll
            for (int v = 0; v < G::VPL; ++v) {
                const uint32_t u = v * G::LPR + l_in;
                if (FULL || u < nunits) {
                    if (h) dst[u] = val[p][v];
                    else if (bad) dst[u] = V(0.0f); // rejected id: zero row (kept inline: hoisting it out costs 12 VGPRs and 10 % speed)
                }
            }
        }
        // ---- verdict for K2: one word per position, written for EVERY row of the chunk (one 4-byte store by the first lane of the
        //      row), so the array never needs clearing between batches
#pragma unroll
        for (int t = 0; t < TSTEPS; ++t) {
            if (lead_l[t]) {
                uint32_t w = 0u;
                if (imiss_l[t]) w = kLinkMiss | (((uint32_t)(prev[t] >> 32) == gen) ? (uint32_t)prev[t] : 0u);
                else if (bad_l[t]) w = kLinkBad;
                c.miss_link[base + t * TG::SPL + lane / TG::LPS] = w;
            }
        }
        if (c.list_sub) {   // the missed rows' positions, in the slots reserved above
            uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)list_at);
#pragma unroll
            for (int t = 0; t < TSTEPS; ++t) {
                const uint64_t mb = __ballot(imiss_l[t]);
                if (imiss_l[t]) c.miss_list[shard * c.list_sub + at + (uint32_t)__builtin_popcountll(mb & ((1ull << lane) - 1ull))] = (uint32_t)(base + t * TG::SPL + lane / TG::LPS);
                at += (uint32_t)__builtin_popcountll(mb);
            }
        }
        if (SINGLE) break;
    }
}

// ---------------------------------------------------------------------------------------------------------- KW
// Write-through row update (coala_cache_write_rows / _adagrad_rows / _adam_rows / _rowwise_adagrad_rows): one kernel over (line size, VEC, tag
// width, op); the ops are assign, add, element-wise Adagrad, Adam and row-wise Adagrad.
// A wave takes the SPL rows whose tag sets one wave-wide 16-B load fetches (8 with 32-bit tags, 4 with 64-bit ones), exactly as a tag step of
// K1: every lane compares its own KPL tags, and an OR over the LPS lanes of a row -- K1's DPP ladder with | in place of min -- leaves the row's
// whole 32-way match mask in each of them.  The rows are then moved RPP at a time: the old value comes from the lowest matching line when there is
// one (no host-link read) and from the cold row otherwise, the new one goes to the cold row and to EVERY line of the mask.  Nothing else of the
// table is written: no tag, cursor, colour or hit / miss counter, and no float of a line past `dim`.  Rejected ids add to one counter of their own
// (stats word kStatWriteBad: K2's per-block sums are tied to the rows a probe counted).
// Latency is hidden across waves, not inside one (a wave has one row(-pair) in flight): the grid is one wave per chunk up to the caps at the launch.
// Measured (tools/embedding_probe.py, profiles/r17_embedding_update.txt; pinned table, 24.6 k and 60.9 k rows): 512-B rows, all cached, go to the
// host at 53.4-53.9 GB/s in all three ops, 97-101 % of a pinned hipMemcpy of the same bytes in the same process; 4-KiB rows at 55 GB/s (assign,
// 97 %) and, with a third to three quarters of the old values read back over the link, 47-51 GB/s (add, Adagrad: 84-91 %).  An Adagrad state in
// pinned host memory adds a read and a write of the link per element: 23-24 GB/s of rows (41-43 %).
// Adam and row-wise Adagrad (profiles/r19_embedding_optimizers.txt, same shapes, alternating with Adagrad): 0.99-1.03 and 1.01-1.06 of Adagrad's time;
// the reduction's wait between a row's loads and its stores is hidden by the other waves.
// Adam (coala_cache_adam_rows) is a fourth element-wise op with two state rows; its step count t is the row's own counter (read by every lane
// of the row, stored back by the first) or the caller's, and the bias corrections 1 - beta^t = -expm1(t ln beta) are taken once per row in double.
// exp_avg is signed, so beta1 m and (1 - beta1) g can cancel: the product's rounding error is carried (one more fma) and added back after the
// sum, which keeps the error of the new exp_avg -- and of the step -- relative to the value itself.
// Row-wise Adagrad (coala_cache_rowwise_adagrad_rows) reduces over the row between its loads and its stores: every lane sums the squares of
// its own floats in load order (fma chain), an xor butterfly over the row's LPR lanes (1, 2, .. LPR / 2) adds the partial sums -- both
// partners of a step add the same two numbers, so all lanes end with the same bits and the result does not depend on the run.  The butterfly
// runs with all 64 lanes active: with two rows per pass a rejected row does not leave the iteration (its loads and stores are predicated off
// and it sums zeros), and a step never crosses the half-wave of its row.  Additions on the longest path from one square to the total:
// VPL * VEC - 1 in the lane, log2(LPR) across lanes -- at most 21 (1024-float lines).
enum { kOpAssign = 0, kOpAdd = 1, kOpAdagrad = 2, kOpAdam = 3, kOpRowAdagrad = 4 };

// What the last two ops need beyond (state, a, eps).  It trails the kernel's arguments: those of the first three ops are where they were.
struct WriteExtra {
    float* state2;       // Adam: exp_avg_sq (state: exp_avg)
    int32_t* row_step;   // Adam: per-row step counter, or null: t = step
    double ln_b1, ln_b2; // Adam: ln beta_i, from the fp32 beta_i
    double step;         // Adam: t of every row when row_step is null
    float b1, b2;        // Adam
    float omb1, omb1_lo; // Adam: 1 - beta1 as an fp32 pair (the low part is 0 for beta1 >= 0.5)
    float omb2;          // Adam: 1 - beta2
};
struct AdamRow { float step_size, rsbc2; };   // lr / bc1 and 1 / sqrt(bc2) of one row

__device__ __forceinline__ float adam_op(float g, float old, float& m, float& v, const WriteExtra& ex, const AdamRow& r, float eps) {
    const float p = ex.omb1 * g;
    float e = __builtin_fmaf(ex.omb1, g, -p);            // p + e == omb1 * g exactly
    e = __builtin_fmaf(ex.omb1_lo, g, e);
    const float mn = __builtin_fmaf(ex.b1, m, p) + e;
    const float vn = __builtin_fmaf(ex.b2, v, ex.omb2 * (g * g));
    m = mn;
    v = vn;
    return old - (r.step_size * mn) / __builtin_fmaf(__builtin_sqrtf(vn), r.rsbc2, eps);
}
__device__ __forceinline__ vfloat4 adam_op(vfloat4 g, vfloat4 old, vfloat4& m, vfloat4& v, const WriteExtra& ex, const AdamRow& r, float eps) {
    vfloat4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float mk = m[k], vk = v[k];
        o[k] = adam_op(g[k], old[k], mk, vk, ex, r, eps);
        m[k] = mk;
        v[k] = vk;
    }
    return o;
}
__device__ __forceinline__ float sq_acc(float x, float acc) { return __builtin_fmaf(x, x, acc); }
__device__ __forceinline__ float sq_acc(vfloat4 x, float acc) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = __builtin_fmaf(x[k], x[k], acc);
    return acc;
}
__device__ __forceinline__ float scaled_sub(float x, float old, float scale) { return __builtin_fmaf(-scale, x, old); }
__device__ __forceinline__ vfloat4 scaled_sub(vfloat4 x, vfloat4 old, float scale) {
    vfloat4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = __builtin_fmaf(-scale, x[k], old[k]);
    return o;
}

template <int OP> __device__ __forceinline__ float write_op(float x, float old, float& st, float a, float eps) {
    if (OP == kOpAssign) return x;
    if (OP == kOpAdd) return __builtin_fmaf(a, x, old);
    const float s = st + x * x;
    st = s;
    return old - a * x / (__builtin_sqrtf(s) + eps);
}
template <int OP> __device__ __forceinline__ vfloat4 write_op(vfloat4 x, vfloat4 old, vfloat4& st, float a, float eps) {
    vfloat4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float s = st[k];
        r[k] = write_op<OP>(x[k], old[k], s, a, eps);
        st[k] = s;
    }
    return r;
}

template <int CD, int VEC, typename TAG, int OP>
__global__ __launch_bounds__(256) void write_rows_kernel(const int64_t* __restrict__ ids, const float* __restrict__ src, float* __restrict__ state,
                                                         int64_t n, float a, float eps, CacheDev c, WriteExtra ex) {
    using G = Geo<CD, VEC, 1>;
    using V = typename VecT<VEC>::type;
    using TG = TagGeo<TAG>;
    using TV = typename TG::vec;
    constexpr int R = TG::SPL;            // rows per chunk: the sets of one wave-wide tag load
    static_assert(R % G::RPP == 0, "a chunk is a whole number of passes");
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int64_t n_chunks = (n + R - 1) / R;
    const uint32_t nunits = c.dim / VEC;
    const TAG* __restrict__ keys = reinterpret_cast<const TAG*>(c.keys);
    float* cold = const_cast<float*>(c.cold);   // (the header: a handle that is written to fronts a writable table)
    const int sub = (G::RPP == 2) ? (lane >> 5) : 0;
    const int l_in = lane & (G::LPR - 1);
    const uint32_t lane_way0 = (uint32_t)((lane % TG::LPS) * TG::KPL);

    for (int64_t chunk = wave; chunk < n_chunks; chunk += n_waves) {   // (wave-uniform trip count: every lane is active at the DPP steps)
        // ---- probe: lane l looks at row l / LPS of the chunk, tags KPL * (l % LPS) .. + KPL - 1 of that row's set
        const int64_t i_l = chunk * R + lane / TG::LPS;
        const bool valid = i_l < n;
        const uint64_t id_l = valid ? (uint64_t)ids[i_l] : 0;
        const bool ok = valid && id_l < c.num_rows;
        const uint32_t set_l = ok ? (uint32_t)set_of(c, id_l) : 0u;
        TV kk = TV(TG::EMPTY);
        if (ok) kk = *reinterpret_cast<const TV*>(keys + (uint64_t)set_l * COALA_WAYS + lane_way0);
        uint32_t mask = 0u;
#pragma unroll
        for (int k = 0; k < TG::KPL; ++k)
            if (kk[k] == (TAG)id_l) mask |= 1u << (lane_way0 + (uint32_t)k);
        if (!ok) mask = 0u;   // (an id outside the table may equal the empty tag)
        mask |= dpp_u32<0xB1>(mask);    // lane ^ 1
        mask |= dpp_u32<0x4E>(mask);    // lane ^ 2
        mask |= dpp_u32<0x141>(mask);   // the other quad of the 8 lanes
        if (TG::LPS == 16) mask |= dpp_u32<0x140>(mask);   // the other half of the 16 lanes
        const uint64_t bad_b = __ballot(valid && !ok && (lane % TG::LPS) == 0);
        if (bad_b && lane == 0) atomicAdd(c.stats + kStatWriteBad, (unsigned long long)__builtin_popcountll(bad_b));

        // ---- rows, RPP at a time: row q of the chunk lives in lane LPS * q of the probe
#pragma unroll 1
        for (int p = 0; p < R / G::RPP; ++p) {
            const int q = p * G::RPP + sub;
            const uint32_t m = (uint32_t)__shfl((int)mask, TG::LPS * q);
            const uint32_t set = (uint32_t)__shfl((int)set_l, TG::LPS * q);
            const uint64_t id = shfl64(id_l, TG::LPS * q);
            const bool live = __shfl((int)ok, TG::LPS * q) != 0;
            // (row-wise Adagrad: a wave-uniform exit only, so that the butterfly below runs with all 64 lanes; `act` predicates the dead half)
            if (OP == kOpRowAdagrad ? __ballot(live) == 0 : !live) continue;
            const bool act = OP == kOpRowAdagrad ? live : true;
            const int64_t i = chunk * R + q;
            const V* xs = reinterpret_cast<const V*>(src + i * (int64_t)c.dim);
            V* cold_row = reinterpret_cast<V*>(cold + id * (uint64_t)c.dim);   // (never partitioned: refused on the host)
            V* st_row = (OP == kOpAdagrad || OP == kOpAdam) ? reinterpret_cast<V*>(state + id * (uint64_t)c.dim) : nullptr;
            V* st2_row = OP == kOpAdam ? reinterpret_cast<V*>(ex.state2 + id * (uint64_t)c.dim) : nullptr;
            float* set_lines = c.lines + (uint64_t)set * COALA_WAYS * CD;
            const V* old_row = m ? reinterpret_cast<const V*>(set_lines + (uint64_t)__builtin_ctz(m) * CD) : cold_row;
            V x[G::VPL], old[G::VPL], st[G::VPL], st2[G::VPL];
#pragma unroll
            for (int v = 0; v < G::VPL; ++v) {
                const uint32_t u = v * G::LPR + l_in;
                x[v] = V(0.0f); old[v] = V(0.0f); st[v] = V(0.0f); st2[v] = V(0.0f);
                if (u < nunits && act) {
                    x[v] = nt_load(xs + u);
                    if (OP != kOpAssign) old[v] = old_row[u];
                    if (OP == kOpAdagrad || OP == kOpAdam) st[v] = st_row[u];
                    if (OP == kOpAdam) st2[v] = st2_row[u];
                }
            }
            AdamRow ar = {0.0f, 0.0f};
            if (OP == kOpAdam) {   // the row's step count and bias corrections, the same in every lane of the row
                double t = ex.step;
                if (ex.row_step) {
                    const int32_t t0 = ex.row_step[id];
                    const int32_t t1 = t0 < 0x7FFFFFFF ? t0 + 1 : t0;   // saturates
                    if (l_in == 0) ex.row_step[id] = t1;                // (after the read: it waits for t0; distinct ids, so no other wave's word)
                    t = (double)t1;
                }
                const double bc1 = -expm1(t * ex.ln_b1), bc2 = -expm1(t * ex.ln_b2);
                ar.step_size = (float)((double)a / bc1);
                ar.rsbc2 = (float)(1.0 / sqrt(bc2));
            }
            float scale = 0.0f;
            if (OP == kOpRowAdagrad) {
                float part = 0.0f;                                       // 0 in lanes past dim and in a dead half
#pragma unroll
                for (int v = 0; v < G::VPL; ++v) part = sq_acc(x[v], part);
#pragma unroll
                for (int d = 1; d < G::LPR; d <<= 1) part += __shfl_xor(part, d);   // all lanes active; d < LPR keeps a step inside the row
                float s = 0.0f;
                if (act) s = state[id] + part / (float)c.dim;
                if (act && l_in == 0) state[id] = s;
                scale = a / (__builtin_sqrtf(s) + eps);
            }
#pragma unroll
            for (int v = 0; v < G::VPL; ++v) {
                const uint32_t u = v * G::LPR + l_in;
                if (u < nunits && act) {
                    V nv;
                    if (OP == kOpAdam) {
                        nv = adam_op(x[v], old[v], st[v], st2[v], ex, ar, eps);
                        st_row[u] = st[v];
                        st2_row[u] = st2[v];
                    } else if (OP == kOpRowAdagrad) {
                        nv = scaled_sub(x[v], old[v], scale);
                    } else {
                        nv = write_op<OP>(x[v], old[v], st[v], a, eps);
                        if (OP == kOpAdagrad) st_row[u] = st[v];
                    }
                    cold_row[u] = nv;
                    for (uint32_t mm = m; mm; mm &= mm - 1)
                        reinterpret_cast<V*>(set_lines + (uint64_t)__builtin_ctz(mm) * CD)[u] = nv;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- K2
// Rank + fill. isolated_cache.h:197-210 (round robin in batch order), :417-474 (miss path), :323-331 (cold read).
// Hazard-free in ONE kernel: every reader of a set's cursor recovers the value before the batch whether or not the set's
// first-ranked miss has already advanced it (generation tag), every way touched in this batch has exactly one winner, and only
// winners touch keys / color_meta / lines.


// Rank the missed row at batch position `pos` inside its set, by ONE lane: walk the set's chain, count the misses before it in batch order,
// advance the set's cursor if it is the first of them, and publish tag and colour if it is the last writer of its way (the winner).
__device__ __forceinline__ void rank_row(const CacheDev& c, uint32_t gen, uint32_t pos, uint64_t id, uint32_t& slot, uint32_t& win) {
    const uint64_t set = set_of(c, id);
    uint32_t cur = (uint32_t)c.set_head[set]; // tagged with this generation: this row was pushed on it by K1
    uint32_t total = 0, rank = 0;
    while (cur) {
        const uint32_t p2 = cur - 1;
        ++total;
        rank += (p2 < pos) ? 1u : 0u;
        cur = c.miss_link[p2] & ~kLinkMiss;
    }
    // the cursor before this batch: the set's first-ranked miss advances it below, tagged with the generation
    const uint64_t cv = __hip_atomic_load(c.set_cnt + set, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t cnt0 = ((uint32_t)(cv >> 32) == gen) ? (uint32_t)cv - total : (uint32_t)cv;
    if (rank == 0) __hip_atomic_store(c.set_cnt + set, ((uint64_t)gen << 32) | (uint32_t)(cnt0 + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t way = (cnt0 + rank) & (COALA_WAYS - 1);              // isolated_cache.h:203
    slot = (uint32_t)(set * COALA_WAYS) + way;
    win = (rank + COALA_WAYS >= total) ? 1u : 0u;                       // nobody later in the batch lands here
    if (win) {
        if (c.tag32) reinterpret_cast<uint32_t*>(c.keys)[slot] = (uint32_t)id;   // isolated_cache.h:434 (a uniform branch)
        else reinterpret_cast<uint64_t*>(c.keys)[slot] = id;
        if (c.color_counters) {
            // the pre-batch occupant leaves (:427-429), the winner enters (:437-441); rows that were inserted
            // and overwritten again inside this batch cancel out
            const int32_t col = c.node_color[id];
            atomicSub(c.color_counters + c.color_meta[slot], 1);
            atomicAdd(c.color_counters + col, 1);
            c.color_meta[slot] = (uint32_t)col;
        }
    }
}
// The two halves of a group move (up to R missed rows, one per pass and half-wave): cold rows -> registers, registers -> output rows
// and, for winners, lines.  Between them the loads are in flight.
template <typename G, typename V>
__device__ __forceinline__ void cold_load(const CacheDev& c, const uint64_t (&id)[G::PASSES], const bool (&live)[G::PASSES], int l_in, uint32_t nunits,
                                          V (&val)[G::PASSES][G::VPL]) {
#pragma unroll
    for (int p = 0; p < G::PASSES; ++p) {
        const V* src = reinterpret_cast<const V*>(c.cold + cold_row_of(c, id[p]) * (uint64_t)c.dim); // cold stride = dim
#pragma unroll
        for (int v = 0; v < G::VPL; ++v) {
            const uint32_t u = v * G::LPR + l_in;
            if (live[p] && u < nunits) val[p][v] = nt_load(src + u);
        }
    }
}
template <int CD, typename G, typename V>
__device__ __forceinline__ void fill_store(const CacheDev& c, V* const (&dst)[G::PASSES], const uint32_t (&slot)[G::PASSES], const bool (&winner)[G::PASSES],
                                           const bool (&live)[G::PASSES], int l_in, uint32_t nunits, const V (&val)[G::PASSES][G::VPL]) {
#pragma unroll
    for (int p = 0; p < G::PASSES; ++p) {
        V* line = reinterpret_cast<V*>(c.lines + (uint64_t)slot[p] * CD);
#pragma unroll
        for (int v = 0; v < G::VPL; ++v) {
            const uint32_t u = v * G::LPR + l_in;
            if (live[p] && u < nunits) {
                nt_store(val[p][v], dst[p] + u);
                if (winner[p]) nt_store(val[p][v], line + u);
            }
        }
    }
}
// miss / rejected totals of a fill launch (isolated_cache.h:471-472): a running sum per block, owned by that block -- no atomics
__device__ __forceinline__ void add_block_stats(const CacheDev& c, uint32_t my_miss, uint32_t my_bad) {
    __shared__ uint32_t s_m[256 / 64], s_b[256 / 64];
    const int lane = threadIdx.x & 63;
    for (int off = 32; off > 0; off >>= 1) { my_miss += __shfl_down(my_miss, off); my_bad += __shfl_down(my_bad, off); }
    if (lane == 0) { s_m[threadIdx.x >> 6] = my_miss; s_b[threadIdx.x >> 6] = my_bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t m = 0, b = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { m += s_m[w]; b += s_b[w]; }
        if (m) c.stats[2 * blockIdx.x] += m;
        if (b) c.stats[2 * blockIdx.x + 1] += b;
    }
}

template <int CD, int VEC, bool REDIR = false, int NP = 4>
__global__ __launch_bounds__(256) void miss_fill_kernel(CacheDev c, const int64_t* __restrict__ idx, float* __restrict__ out,
                                                        int tile_rows, int sparse_max, uint32_t gen, RangeSet rs, Redirect rd, int dyn_slot) {
    // Works on the batch positions of `rs` (the whole batch = one range, or the slices of a serve split into several fills),
    // walked as one dense virtual index space.  A wave reads the verdicts of tile_rows rows at once (one byte per lane;
    // tile_rows = R or 64) and then works through the tile chunk by chunk (R rows), skipping chunks without a miss on a scalar
    // mask.  With tile_rows = R this is one verdict load per chunk: fine when the grid is wide (HBM cold tier).  Behind the
    // 16..64-block grid of the host tier it made a batch with few misses latency-bound (123,904 rows, all hits: 484 dependent
    // loads per wave = 220 us of nothing).
    using G = Geo<CD, VEC, NP>;
    using V = typename VecT<VEC>::type;
    constexpr int R = G::R;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int64_t n_tiles = ((int64_t)rs.total + tile_rows - 1) / tile_rows;
    const int chunks_per_tile = tile_rows / R;
    const uint32_t nunits = c.dim / VEC;
    const int sub = (G::RPP == 2) ? (lane >> 5) : 0;
    const int l_in = lane & (G::LPR - 1);
    uint32_t my_miss = 0, my_bad = 0;

    // U verdict loads in flight per wave: the scan of a batch without misses is a chain of load latencies, and with FEW misses every
    // group of U tiles is ranked and streamed as one (below) -- 8 tiles = 512 rows per step (4 until round 3: 2 % misses 56 -> 5x us)
    constexpr int U = 8;
    // Which tiles a wave takes.  Static (dyn_slot < 0): wave w takes tiles w, w + n_waves, ... -- with few waves behind a host tier and a miss count that
    // varies from tile to tile, the waves' shares of the launch differ by 15-30 % and the last ones stream alone.  Dynamic: a wave CLAIMS tiles from this
    // launch's ticket counter until they are gone (the probe of the batch zeroed the batch's counters; which wave streams which row never mattered to
    // the result).  A claim is as small as it may be while the wave finds misses -- ONE tile for a batch of a few tiles per wave, an eighth of a wave's
    // even share (up to U tiles) for the big ones -- and doubles, up to 4 U consecutive tiles scanned U at a time, with every claim that found none:
    // a batch, or a stretch of one, without misses is scanned about as fast as by the static deal, and a sparse one is still dealt finely.
    uint32_t* ticket = reinterpret_cast<uint32_t*>(c.stats + 2 * kStatBlocks) + (dyn_slot < 0 ? 0 : dyn_slot);
    const bool dyn = dyn_slot >= 0;
    // nothing to fill in the whole batch (the probe's waves set the flag when they find a miss or a rejected id): no scan at all
    if (reinterpret_cast<const uint32_t*>(c.stats + 2 * kStatBlocks)[2 * kFillSlots + (gen & 1u)] == 0u) return;
    const int64_t n_deal = dyn ? 1 : n_waves;
    const int64_t even8 = n_tiles / (n_waves * 8);
    const int claim_min = even8 < 1 ? 1 : (even8 > U ? U : (int)even8);
    int claim = claim_min;
    for (int64_t unit = dyn ? -1 : wave;;) {
      int64_t claim_end = n_tiles;          // static: the wave's tiles run to the end of the launch
      if (dyn) {
          uint32_t t = 0;
          if (lane == 0) t = atomicAdd(ticket, (uint32_t)claim);
          unit = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)t);
          if (unit >= n_tiles) break;
          claim_end = unit + claim < n_tiles ? unit + claim : n_tiles;
          claim = claim * 2 > 4 * U ? 4 * U : claim * 2;   // (back to claim_min below as soon as this claim turns out to hold a miss)
      } else if (unit >= n_tiles) break;
     for (int64_t tile0 = unit; tile0 < claim_end; tile0 += n_deal * U) {
      const int n_here = dyn ? (int)(claim_end - tile0 < U ? claim_end - tile0 : U) : U;   // tiles of this pass: tile0 + u * n_deal, u < n_here
      uint64_t st_pack = 0; // the U verdict bytes of this lane, one per tile
#pragma unroll
      for (int u = 0; u < U; ++u) {
          const int64_t tile = tile0 + u * n_deal;
          const uint32_t p = (u < n_here && tile < n_tiles && lane < tile_rows) ? pos_of(rs, (uint32_t)(tile * tile_rows + lane)) : 0xFFFFFFFFu;
          const uint32_t w = (p != 0xFFFFFFFFu) ? c.miss_link[p] : 0u;
          const uint64_t v = (w == 0u) ? 0u : ((w & kLinkMiss) ? 1u : 2u);
          st_pack |= v << (8 * u);
      }
      if (!__ballot(st_pack != 0)) continue; // nothing but hits in these U tiles
      // ---- per-lane state of ONE missed row (the lane "holds" it): rank inside its set, way, winner flag
      uint32_t slot_l = 0, win_l = 0;
      uint64_t id_l = 0;
      int64_t drow_l = 0;                    // destination row; < 0 encodes row -(v+1) of rd.out
      auto rank_at = [&](uint32_t pos) {
          id_l = (uint64_t)idx[pos];
          drow_l = (int64_t)pos;
          if (REDIR && (int64_t)pos >= rd.begin && (int64_t)pos < rd.end)
              drow_l = -((rd.row_map ? rd.row_map[(int64_t)pos - rd.begin] : (int64_t)pos - rd.begin) + 1);
          rank_row(c, gen, pos, id_l, slot_l, win_l);
      };
      // ---- stream up to R missed rows: pass p of this lane's half-wave moves the row held by lane srcl[p]
      auto move_group = [&](const int (&srcl)[G::PASSES], const bool (&live)[G::PASSES]) {
          V val[G::PASSES][G::VPL];
          uint32_t slot_[G::PASSES];
          uint64_t id[G::PASSES];
          int64_t drow[G::PASSES];
          bool winner[G::PASSES];
          V* dst[G::PASSES];
#pragma unroll
          for (int p = 0; p < G::PASSES; ++p) {
              slot_[p] = (uint32_t)__shfl((int)slot_l, srcl[p]);
              winner[p] = __shfl((int)win_l, srcl[p]) != 0;
              id[p] = shfl64(id_l, srcl[p]);
              drow[p] = (int64_t)shfl64((uint64_t)drow_l, srcl[p]);
          }
          cold_load<G>(c, id, live, l_in, nunits, val);
#pragma unroll
          for (int p = 0; p < G::PASSES; ++p)
              dst[p] = (REDIR && drow[p] < 0) ? reinterpret_cast<V*>(rd.out + (uint64_t)(-(drow[p] + 1)) * c.dim)
                                              : reinterpret_cast<V*>(out + (uint64_t)drow[p] * c.dim);
          fill_store<CD, G>(c, dst, slot_, winner, live, l_in, nunits, val);
      };
      // the rows held by the lanes of `holders` (each already ranked), streamed R at a time, compacted
      auto stream_holders = [&](uint64_t holders) {
          int srcl[G::PASSES];
          bool live[G::PASSES];
          while (holders) {
#pragma unroll
              for (int p = 0; p < G::PASSES; ++p) {
                  int l0 = -1, l1 = -1;
                  if (holders) { l0 = __builtin_ctzll(holders); holders &= holders - 1; }
                  if (G::RPP == 2 && holders) { l1 = __builtin_ctzll(holders); holders &= holders - 1; }
                  const int l = (G::RPP == 2 && sub) ? l1 : l0;
                  live[p] = l >= 0;
                  srcl[p] = l >= 0 ? l : 0;
              }
              move_group(srcl, live);
          }
      };
      // verdicts of the U tiles as wave-uniform masks
      uint64_t mmask[U];
      uint32_t total_miss = 0, worst = 0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
          const uint8_t st = (uint8_t)(st_pack >> (8 * u));
          mmask[u] = __ballot(st == 1);
          my_miss += (st == 1);
          my_bad += (st == 2);
          const uint32_t cnt = (uint32_t)__builtin_popcountll(mmask[u]);
          total_miss += cnt;
          worst = cnt > worst ? cnt : worst;
      }
      if (!total_miss) continue;
      claim = claim_min;
      if (total_miss <= 64 && (int)worst <= sparse_max) {
          // Few misses in ALL U tiles (the multi-GPU steady state: the caches of 8 GPUs hold most of the table).  Tile by tile a wave
          // would pay the whole dependency chain -- verdict -> id -> chain walk -> cursor -> PCIe read -> store, ~8 us -- once per
          // tile with one or two rows in flight (2 % misses: 56 us for 2.3 MB, latency- not link-bound).  Instead lane j takes the
          // j-th miss of the U tiles, all are ranked at once, and the rows stream R at a time.
          uint32_t k = (uint32_t)lane;
          int u_sel = -1;
          uint64_t m_sel = 0;
#pragma unroll
          for (int u = 0; u < U; ++u) {
              const uint32_t cnt = (uint32_t)__builtin_popcountll(mmask[u]);
              if (u_sel < 0) {
                  if (k < cnt) { u_sel = u; m_sel = mmask[u]; }
                  else k -= cnt;
              }
          }
          if (u_sel >= 0) {
              for (uint32_t i = 0; i < k; ++i) m_sel &= m_sel - 1;   // the k-th miss of that tile sits in lane ctz(m_sel)
              const uint32_t pos = pos_of(rs, (uint32_t)((tile0 + u_sel * n_deal) * tile_rows + __builtin_ctzll(m_sel)));
              rank_at(pos);
          }
          stream_holders(total_miss >= 64 ? ~0ull : ((1ull << total_miss) - 1ull));
          continue;
      }
#pragma nounroll
      for (int u = 0; u < U; ++u) {
        const uint8_t st = (uint8_t)(st_pack >> (8 * u));
        const uint64_t tile_mask = __ballot(st == 1);   // (recomputed: mmask[] must not be indexed by a run-time u)
        if (!tile_mask) continue;
        // a lane with a verdict has a valid position (recomputed: cheaper than keeping U of them alive across the loop)
        const uint32_t pos_l = st ? pos_of(rs, (uint32_t)((tile0 + u * n_deal) * tile_rows + lane)) : 0u;
        if (__builtin_popcountll(tile_mask) <= sparse_max) {
            // Few misses in this tile: rank every missed row of the tile at once, then stream them R at a time, compacted.
            if (st == 1) rank_at(pos_l);
            stream_holders(tile_mask);
        } else {
            int srcl[G::PASSES];
            bool live[G::PASSES];
            for (int ck = 0; ck < chunks_per_tile; ++ck) {
                const uint32_t live_mask = (uint32_t)(tile_mask >> (ck * R)) & ((1u << R) - 1u);
                if (!live_mask) continue;
                const int lane0 = ck * R;              // lanes lane0 .. lane0+R-1 hold this chunk's rows
                if (st == 1 && lane >= lane0 && lane < lane0 + R) rank_at(pos_l);
#pragma unroll
                for (int p = 0; p < G::PASSES; ++p) {
                    const int q = p * G::RPP + sub;
                    live[p] = (live_mask >> q) & 1;
                    srcl[p] = lane0 + q;
                }
                move_group(srcl, live);
            }
        }
      }
     }
      if (!dyn) break;           // static: the wave's own tiles are done
    }
    add_block_stats(c, my_miss, my_bad);
}

// K2, list form: every whole read on a host tier.  The probe has left the batch's misses in kListShards lists (list_counter); a wave reads all
// the counters at once, and with their prefix sums the lists are one dense index space of `total` entries, dealt R at a time: a wave's first
// group is its own index, the later ones come from the batch's first ticket counter.  For a group the cold rows are requested as soon as the ids
// are known -- a host read needs nothing else -- and the rows are ranked (rank_row, lanes 0..R-1) while those reads are in flight.  No verdict
// scan, no tiles, no sparse / dense split: every miss ratio takes this path, and a batch without misses leaves after the counter load.
template <int CD, int VEC, int NP = 4>
__global__ __launch_bounds__(256) void miss_fill_list_kernel(CacheDev c, const int64_t* __restrict__ idx, float* __restrict__ out, uint32_t gen) {
    using G = Geo<CD, VEC, NP>;
    using V = typename VecT<VEC>::type;
    constexpr int R = G::R;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    const uint32_t nunits = c.dim / VEC;
    const int sub = (G::RPP == 2) ? (lane >> 5) : 0;
    const int l_in = lane & (G::LPR - 1);
    static_assert(kListShards == 64, "one list counter per lane");
    const uint32_t cnt_l = __hip_atomic_load(list_counter(c, gen & 1u, (uint32_t)lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t incl = cnt_l;   // entries of the shards 0..lane
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    const uint32_t excl = incl - cnt_l;
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (total == 0) return;   // nothing missed in this batch
    const uint32_t n_groups = (total + R - 1) / R;
    uint32_t* ticket = reinterpret_cast<uint32_t*>(c.stats + 2 * kStatBlocks) + (gen & 1u) * kFillSlots;   // zeroed by the batch's probe
    uint32_t my_miss = 0;
    for (uint32_t g = wave; g < n_groups;) {
        // lane j < R holds entry g * R + j: its shard is the number of shards that end at or before it
        uint32_t pos_l = 0;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const uint32_t e = g * R + j;
            const uint32_t s = (uint32_t)__builtin_popcountll(__ballot(incl <= e)) & 63u;   // (e >= total: not read)
            const uint32_t off = e - (uint32_t)__builtin_amdgcn_readlane((int)excl, (int)s);
            if (lane == j && e < total) pos_l = c.miss_list[s * c.list_sub + off];
        }
        const bool have = lane < R && g * R + (uint32_t)lane < total;
        const uint64_t id_l = have ? (uint64_t)idx[pos_l] : 0;
        uint64_t id[G::PASSES];
        uint32_t pos[G::PASSES];
        bool live[G::PASSES];
        V val[G::PASSES][G::VPL];
#pragma unroll
        for (int p = 0; p < G::PASSES; ++p) {
            const int q = p * G::RPP + sub;   // the row of this half-wave in pass p is held by lane q
            live[p] = g * R + (uint32_t)q < total;
            id[p] = shfl64(id_l, q);
            pos[p] = (uint32_t)__shfl((int)pos_l, q);
        }
        cold_load<G>(c, id, live, l_in, nunits, val);
        uint32_t t = 0;   // the next group's ticket comes back behind the rows
        if (lane == 0) t = atomicAdd(ticket, 1u);
        uint32_t slot_l = 0, win_l = 0;
        if (have) rank_row(c, gen, pos_l, id_l, slot_l, win_l);
        uint32_t slot[G::PASSES];
        bool winner[G::PASSES];
        V* dst[G::PASSES];
#pragma unroll
        for (int p = 0; p < G::PASSES; ++p) {
            const int q = p * G::RPP + sub;
            slot[p] = (uint32_t)__shfl((int)slot_l, q);
            winner[p] = __shfl((int)win_l, q) != 0;
            dst[p] = reinterpret_cast<V*>(out + (uint64_t)pos[p] * c.dim);
        }
        fill_store<CD, G>(c, dst, slot, winner, live, l_in, nunits, val);
        if (lane == 0) my_miss += (total - g * R < (uint32_t)R) ? total - g * R : (uint32_t)R;
        g = n_waves + (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    }
    add_block_stats(c, my_miss, 0u);
}

// ---------------------------------------------------------------------------------------------------------- scatter
// out[map[r], :] = src[r, :]   (cache_kernel.cu:113-137)
template <int CD, int VEC, int NP = 4>
__global__ __launch_bounds__(256) void scatter_rows_kernel(float* __restrict__ out, const float* __restrict__ src,
                                                           const int64_t* __restrict__ map, RangeSet rs, uint32_t dim) {
    // rows r of `rs` (one range = the whole buffer; several = the slices one round of a split row exchange delivered)
    using G = Geo<CD, VEC, NP>;
    using V = typename VecT<VEC>::type;
    constexpr int R = G::R;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int64_t n_chunks = ((int64_t)rs.total + R - 1) / R;
    const uint32_t nunits = dim / VEC;
    const int sub = (G::RPP == 2) ? (lane >> 5) : 0;
    const int l_in = lane & (G::LPR - 1);
    for (int64_t chunk = wave; chunk < n_chunks; chunk += n_waves) {
        const int64_t base = chunk * R;
        V val[G::PASSES][G::VPL];
        int64_t d[G::PASSES];
#pragma unroll
        for (int p = 0; p < G::PASSES; ++p) {
            const int64_t vr = base + p * G::RPP + sub;
            const uint32_t r = (vr < (int64_t)rs.total) ? pos_of(rs, (uint32_t)vr) : 0xFFFFFFFFu;
            d[p] = (r != 0xFFFFFFFFu) ? map[r] : -1;
            const V* s = reinterpret_cast<const V*>(src + (int64_t)r * (int64_t)dim);
#pragma unroll
            for (int v = 0; v < G::VPL; ++v) {
                const uint32_t u = v * G::LPR + l_in;
                if (d[p] >= 0 && u < nunits) val[p][v] = nt_load(s + u);
            }
        }
#pragma unroll
        for (int p = 0; p < G::PASSES; ++p) {
            V* t = reinterpret_cast<V*>(out + d[p] * (int64_t)dim);
#pragma unroll
            for (int v = 0; v < G::VPL; ++v) {
                const uint32_t u = v * G::LPR + l_in;
                if (d[p] >= 0 && u < nunits) nt_store(val[p][v], t + u);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- route
// Stable bucketing by owner = id % n_parts: thin kernels over the per-tile bodies of coala_partition.h, grid-stride over the wave tiles.  A
// routed id goes to node_out with its position in the batch beside it in map_out.
struct RouteSink {
    int64_t* __restrict__ node_out;
    int64_t* __restrict__ map_out;
    __device__ __forceinline__ void operator()(int64_t dest, int64_t i, int64_t id) const { node_out[dest] = id, map_out[dest] = i; }
};

__global__ __launch_bounds__(kBlock) void route_count_kernel(const int64_t* __restrict__ idx, int64_t n, uint32_t n_parts, int pshift,
                                                             uint32_t* __restrict__ wave_counts) {
    const int64_t n_tiles = partition_tiles(n), n_waves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); tile < n_tiles; tile += n_waves)
        partition_count_tile(idx, n, tile, n_parts, pshift, wave_counts);
}

// thread 0: bucket totals and bases; bucket_stride > 0 places bucket g at g * bucket_stride (the [G][stride] layout) instead of packing
__global__ __launch_bounds__(1024) void route_scan_kernel(uint32_t* __restrict__ wave_counts, int64_t n, uint32_t n_parts, int64_t bucket_stride,
                                                          int64_t* __restrict__ counts_out, int64_t* __restrict__ offsets_out, int64_t* __restrict__ bases) {
    __shared__ int64_t totals[kMaxParts];
    partition_scan_columns(wave_counts, partition_tiles(n), n_parts, totals);
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (uint32_t g = 0; g < n_parts; ++g) {
            counts_out[g] = totals[g];
            const int64_t b = bucket_stride > 0 ? (int64_t)g * bucket_stride : acc;
            bases[g] = b;
            if (offsets_out) offsets_out[g] = b;
            acc += totals[g];
        }
        if (offsets_out) offsets_out[n_parts] = bucket_stride > 0 ? (int64_t)n_parts * bucket_stride : acc;
    }
}

__global__ __launch_bounds__(kBlock) void route_scatter_kernel(const int64_t* __restrict__ idx, int64_t n, uint32_t n_parts, int pshift,
                                                               const uint32_t* __restrict__ wave_offsets, const int64_t* __restrict__ bases,
                                                               int64_t* __restrict__ node_out, int64_t* __restrict__ map_out) {
    const int64_t n_tiles = partition_tiles(n), n_waves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); tile < n_tiles; tile += n_waves)
        partition_scatter_tile(idx, n, tile, n_parts, pshift, wave_offsets, bases, RouteSink{node_out, map_out});
}

} // namespace

// ============================================================================================================ host

#define fail coala_fail_
#define HIPCHK COALA_HIPCHK

namespace {

// How K1 and K2 are launched.  Fixed at handle creation: launch_shape() sets the product's choice, which development builds
// (build.py --dev -> libcoala_hip_dev.so, -DCOALA_DEV_KNOBS) then override from the environment (apply_dev_knobs).
struct LaunchShape {
    int k1_grid_cap;    // K1 blocks of the looping kernel
    int k1_waves;       // K1 waves per block
    bool k1_single;     // one wave per chunk, loop-free K1 (launches up to kK1SingleMaxChunks chunks)
    int k1_passes;      // development builds: rows(-pairs) in flight per wave in K1 (COALA_K1_PASSES = 2 | 4 | 8 | 16); 0 = kK1Passes
    int k2_grid_cap;    // K2 blocks
    int k2_tile_rows;   // rows per verdict tile of K2; 0 = one chunk
    int k2_sparse_max;  // tiles with at most this many misses are streamed compacted (0 = never)
    int k2_unit_tiles;  // 1 = K2 deals its tiles dynamically (0 = static: wave w takes tiles w, w + n_waves, ...)
};

LaunchShape launch_shape(uint32_t cache_dim, bool host_tier) {
    LaunchShape s;
    // K1 blocks: one chunk per wave up to 131,072 rows.  Measured (tools/k1_insitu.py, tools/k1_bench): 28.5 k rows at 32 %
    // hits in situ: 2048 blocks -> 22.3 us, 4096 -> 20.7, 8192 -> 20.6; all-hit 36,864 rows: 53.8 / 53.1 / 51.4 us;
    // all-hit 123,904 rows: 192.5 / 192.3 / 190.1 / 185.3 us at 2048 / 4096 / 8192 / 16384; 1.08 M x 512 B: 232 -> 227 us
    s.k1_grid_cap = 16384;
    s.k1_waves = kK1Waves;
    // one wave per chunk, no loop, no prefetch state for later chunks: with the lane-parallel probe it is ahead on every line of 1 KiB and more
    // (default workload 17.5 -> 16.35 us, its all-hit leg 58.8 -> 56.6 us, 262,144 x 1 KiB and 123,904 x 4 KiB at every hit ratio:
    // profiles/r03_k1_single_lane_parallel.txt) and behind on 512-B lines, whose 8-row waves need the software pipeline (12.3 vs 13.3 us at 72 k rows)
    s.k1_single = cache_dim >= 256;
    s.k1_passes = 0;
    // K2 blocks: 24-64 when the cold tier is host memory.  The link, not the chip, is the limit, and
    // what matters is the bytes of PCIe reads in flight (blocks x 4 waves x 16 KB): ~1 MB
    // already runs the link at 56.0 GB/s; 4 MB (64 blocks) gives 56.6 GB/s but queues every
    // other host access of the GPU -- AQL packets, kernargs, completion signals of kernels
    // on OTHER streams -- behind ~50 us of reads: a 9-kernel sampler call overlapping the
    // fill took 1.8 ms instead of 0.22 ms, and the prefetching epoch 11.7 s instead of 9.2 s.
    // Full grid: 53.7 GB/s; 8 blocks: 43.1 GB/s.
    // host tier: ~1 MB of reads in flight (blocks x 4 waves x rows-per-wave x line bytes).  A wave holds 16 KB of 4-KiB lines
    // but only 4 KB of 512-B or 1-KiB lines, and with short lines the per-chunk ranking latency dominates, so the
    // count scales with the line size: 24 / 32 / 64 / 64 blocks for cache_dim 1024 / 512 / 256 / 128
    // (measured at cache_dim 128, 111 M x 128 table: 32 / 64 / 128 blocks -> 42.9 / 55.2 / 52.7 GB/s; 16 -> 22.4).
    // 4-KiB lines: 16 / 20 / 24 / 32 blocks take 1417 / 1420 / 1445 / 1507 us per fill of the default workload on their own, and
    // 1.550-1.585 / 1.526 / 1.524 / 1.529 ms per step (fill + gap) beside a consumer's training kernels, which stretch the
    // fill by ~5 %: 20 blocks cost 0.2 % alone and give 1.5 % under load (profiles/r03_k2_grid_under_load.txt) -- that was the STATIC deal of tiles.
    // With the dynamic deal (below) a few more blocks cost nothing alone, and what counts is a multiple of the 8 XCDs, whose turn it is block by
    // block: 24 / 32 blocks run the loader's step in 1.438 / 1.441 ms alone and 1.452 / 1.450 beside the training kernels, 20 / 22 / 26 / 28 blocks in
    // 1.448 / 1.448 / 1.445 / 1.456 and 1.470-1.479 / 1.467 / 1.467 / 1.461; 40: 1.448 and 1.480 (profiles/r04_k2_grid_under_load.txt)
    const int host_blocks = std::min(64, std::max(24, 16 * 1024 / (int)cache_dim));
    s.k2_grid_cap = host_tier ? host_blocks : kStatBlocks;
    // verdict tile: 64 rows behind the narrow host-tier grid, one chunk behind the wide HBM-tier grid (miss_fill_kernel)
    s.k2_tile_rows = host_tier ? 64 : 0;
    // tiles with at most 32 of 64 rows missing are streamed compacted (tools/k2_sparse_probe.py, 28.5 k rows x 4 KiB: 32 % misses
    // 52.4 -> 55.2 GB/s, 16 %: 47.4 -> 54.6, 8 %: 42.5 -> 52.1, 4 %: 36 -> 47; the 68 % default batch is unchanged, 48 costs it 1 %)
    s.k2_sparse_max = host_tier ? 32 : 0;
    // host tier: the tiles are dealt dynamically (miss_fill_kernel).  With 80-256 waves and a miss count that varies from tile to tile a static deal
    // leaves the waves' shares 15-30 % apart and the last ones streaming alone (tools/k2_sparse_probe.py, 28.5 k rows x 4 KiB, static -> dynamic:
    // 100 % misses 52.4 -> 56.7 GB/s, 68 % (the default workload) 55.8 -> 56.3, 32 % 52.7 -> 55.9, 16 % (the 8-GPU steady state) 50.4 -> 54.8,
    // 8 % 49.7 -> 53.2, 2 % 42.7 -> 45.3; a launch with nothing to fill 4 -> 8 us: profiles/r04_k2_dynamic_deal.txt)
    s.k2_unit_tiles = host_tier ? 1 : 0;
    return s;
}

#ifdef COALA_DEV_KNOBS
void apply_dev_knobs(LaunchShape& s) {
    if (const char* e = getenv("COALA_K1_PASSES")) { int v = atoi(e); if (v == 2 || v == 4 || v == 8 || v == 16) s.k1_passes = v; }
    if (const char* e = getenv("COALA_K1_GRID")) { int g = atoi(e); if (g >= 1 && g <= 65535) s.k1_grid_cap = g; }
    if (const char* e = getenv("COALA_K1_WAVES")) { int w = atoi(e); if (w == 1 || w == 2 || w == 4) s.k1_waves = w; }
    if (const char* e = getenv("COALA_K1_SINGLE")) s.k1_single = atoi(e) != 0;
    if (const char* e = getenv("COALA_K2_TILE_ROWS")) { int t = atoi(e); if (t == 0 || t == 8 || t == 16 || t == 32 || t == 64) s.k2_tile_rows = t; }
    if (const char* e = getenv("COALA_K2_GRID")) { int g = atoi(e); if (g >= 1 && g <= kStatBlocks) s.k2_grid_cap = g; }
    if (const char* e = getenv("COALA_K2_SPARSE")) { int g = atoi(e); if (g >= 0 && g <= 64) s.k2_sparse_max = g; }
    if (const char* e = getenv("COALA_K2_UNIT_TILES")) { int g = atoi(e); if (g >= 0 && g <= 1) s.k2_unit_tiles = g; }   // 0: the static deal
}
#endif

// A batch that was probed (serve_probe) and still waits for its fills.  Until every position of [0, rows) was handed to a fill, exactly once, it
// owns the verdict words and the per-set miss chains: a second probe or a row write on top of it would overwrite them under the pending fills.
struct OpenBatch {
    using Ranges = std::vector<std::pair<int64_t, int64_t>>;
    int64_t rows = -1;
    Ranges filled;                               // position ranges already handed to a fill (sorted)
    int64_t filled_rows = 0;
    Redirect redirect{0, 0, nullptr, nullptr};   // set by the probe, reused by the fills

    bool is_open() const { return rows >= 0; }
    void open(int64_t n, const Redirect& rd) { rows = n; filled.clear(); filled_rows = 0; redirect = rd; }
    void close() { rows = -1; filled.clear(); filled_rows = 0; }
    int refuse_while_open() const {
        return fail(COALA_EINVAL, "a batch of %lld rows is still open (%lld filled): finish its serve_fill calls or call coala_cache_serve_abort",
                    (long long)rows, (long long)filled_rows);
    }
    // The ranges of one fill call: inside [0, rows), disjoint from each other and from earlier fills.  Refuses, or leaves in *claim what `filled`
    // becomes once the call's launches are enqueued (commit) and in *claim_rows the rows the call fills.
    int check_ranges(const int64_t* begins, const int64_t* ends, int n_ranges, Ranges* claim, int64_t* claim_rows) const {
        if (n_ranges < 0 || (n_ranges > 0 && (!begins || !ends))) return fail(COALA_EINVAL, "bad fill ranges");
        *claim = filled;
        *claim_rows = 0;
        for (int k = 0; k < n_ranges; ++k) {
            if (begins[k] < 0 || begins[k] > ends[k] || ends[k] > rows)
                return fail(COALA_EINVAL, "fill range [%lld, %lld) outside the batch of %lld rows", (long long)begins[k], (long long)ends[k], (long long)rows);
            if (ends[k] > begins[k]) claim->emplace_back(begins[k], ends[k]);
            *claim_rows += ends[k] - begins[k];
        }
        std::sort(claim->begin(), claim->end());
        for (size_t k = 1; k < claim->size(); ++k)
            if ((*claim)[k].first < (*claim)[k - 1].second)
                return fail(COALA_EINVAL, "fill range [%lld, %lld) overlaps positions that were already filled in this batch", (long long)(*claim)[k].first, (long long)(*claim)[k].second);
        return COALA_OK;
    }
    void commit(Ranges& claim, int64_t claim_rows) {
        filled.swap(claim);
        filled_rows += claim_rows;
        if (filled_rows == rows) close(); // [0, rows) covered once: the batch is complete
    }
};

} // namespace

struct coala_cache {
    coala_cache_config_t cfg;
    CacheDev d;
    uint64_t cap = 0;           // scratch capacity (rows)
    uint32_t gen = 0;           // generation: one per probe
    int fill_launches = 0;      // fill launches of this generation so far: each takes its own ticket counter (kFillSlots per batch)
    int32_t* node_color_dev = nullptr;
    // route scratch
    uint32_t* wave_counts = nullptr;
    uint64_t wave_counts_cap = 0;
    int64_t* route_bases = nullptr;
    // profiling
    struct EvPair { hipEvent_t a, b; int kind; uint64_t rows; };
    std::vector<EvPair> ev_live;
    EventPool ev_pool;
    coala_cache_profile_t prof{};
    hipStream_t last_stream = nullptr;    // stream of the last bracketed launch (for the empty-bracket calibration)
    // The handle's tables and scratch are ordered by the stream its calls are enqueued on.  A caller that moves to another stream
    // keeps that order: the new stream first waits for what the handle enqueued last on the old one (enter).
    StreamOrder order;
    uint64_t table_bytes = 0;
    LaunchShape shape;                    // K1 / K2 launch shapes (launch_shape)
    bool host_tier = false;               // the cold table is host memory (behind the host link)
    int32_t* color_pin = nullptr;         // pinned staging for coala_cache_color_counts
    int32_t* color_pin_async = nullptr;   // pinned staging + event of a pending coala_cache_color_counts_async
    hipEvent_t color_ev = nullptr;
    int32_t color_pending = -1;           // entries of the pending snapshot, -1 = none
    OpenBatch batch;                      // set by serve_probe, closed by its fills or by serve_abort
    uint64_t rows_total = 0;              // rows submitted since the last stats reset (hits = rows - misses - rejected)
    uint64_t cum_hit = 0, cum_miss = 0;   // totals folded in whenever coala_cache_stats resets the device counters
    uint64_t prof_hit0 = 0, prof_miss0 = 0; // totals at the last profile reset
    // coala_cache_fetch_events: a begin event on the first kernel and an end event on the last kernel of every read_feature call, attached
    // to the dispatches themselves (no packets of their own); a ring, so that a caller far ahead of the device can still read old pairs
    bool fetch_events = false;
    static constexpr int kFetchRing = 2048;
    std::vector<hipEvent_t> fev;          // [2 * kFetchRing], created on first use
    uint64_t fev_calls = 0;
    hipEvent_t last_begin = nullptr, last_end = nullptr;
};

namespace {

// How an entry point that enqueues work begins: on the handle's device and, unless it touches nothing the handle orders (follow = false), behind
// what the handle enqueued last, on whichever stream that was ...
int enter(coala_cache* h, hipStream_t s, bool follow = true) {
    HIPCHK(hipSetDevice(h->cfg.device));
    return follow ? h->order.follow(s) : COALA_OK;
}

// ... and how one that launched kernels ends: a launch that failed is reported, and a COALA_FLAG_SYNC handle waits for its work.
int leave(coala_cache* h, hipStream_t s) {
    HIPCHK(hipGetLastError());
    if (h->cfg.flags & COALA_FLAG_SYNC) HIPCHK(hipStreamSynchronize(s));
    return COALA_OK;
}

int ensure_scratch(coala_cache* h, uint64_t n, hipStream_t s) {
    const uint64_t cap_before = h->cap;
    if (int rc = grow((void**)&h->d.miss_link, &h->cap, n, sizeof(uint32_t), s)) return rc;   // written by every probe before any fill reads it
    if (h->cap == cap_before && h->d.miss_list) return COALA_OK;
    // the miss list follows the new capacity (a power of two >= 1024; a chunk has at most 32 rows), whatever it held before
    h->d.list_sub = (uint32_t)(h->cap / kListShards) + 32u;
    const uint64_t list_words = (uint64_t)kListShards * h->d.list_sub;   // entries below a shard's counter are written by the batch's probe
    uint64_t list_cap = 0;
    return grow((void**)&h->d.miss_list, &list_cap, list_words, sizeof(uint32_t), s, list_words);
}

void drain_events(coala_cache* h) {
    for (auto& p : h->ev_live) {
        float ms = 0.f;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            if (p.kind == 0) { h->prof.gather_ms += ms; h->prof.gather_launches++; h->prof.gather_rows += p.rows; }
            else { h->prof.fill_ms += ms; h->prof.fill_launches++; }
        }
        h->ev_pool.give(p.a);
        h->ev_pool.give(p.b);
    }
    h->ev_live.clear();
}

// COALA_FLAG_PROFILE: the kernel's own begin / end timestamps (hipExtLaunchKernelGGL attaches the two events to the dispatch
// itself), i.e. what rocprofv3 reports for the launch -- a separate hipEventRecord bracket adds the 2-5 us between two packets.
struct ProfScope {
    coala_cache* h; hipStream_t s; int kind; uint64_t rows; hipEvent_t a = nullptr, b = nullptr; bool on;
    hipEvent_t xa = nullptr, xb = nullptr; // without profiling: the caller's own begin / end event for this launch (coala_cache_fetch_events)
    ProfScope(coala_cache* h_, hipStream_t s_, int kind_, uint64_t rows_, hipEvent_t xa_ = nullptr, hipEvent_t xb_ = nullptr)
        : h(h_), s(s_), kind(kind_), rows(rows_), xa(xa_), xb(xb_) {
        on = (h->cfg.flags & COALA_FLAG_PROFILE) != 0;
        if (on) {
            if (h->ev_live.size() >= 8192) drain_events(h);
            a = h->ev_pool.take(); b = h->ev_pool.take();
            on = a && b;
            if (on) h->last_stream = s;
        }
    }
    template <typename K, typename... Args>
    void launch(K kernel, dim3 grid, dim3 block, Args... args) {
        if (on) hipExtLaunchKernelGGL(kernel, grid, block, 0, s, a, b, 0, args...);
        else if (xa || xb) hipExtLaunchKernelGGL(kernel, grid, block, 0, s, xa, xb, 0, args...);
        else hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
    }
    ~ProfScope() {
        if (on) h->ev_live.push_back({a, b, kind, rows});
    }
};

template <typename F>
int dispatch_geo(uint32_t cache_dim, bool vec4, F&& f) {
    switch (cache_dim) {
        case 128: return vec4 ? f(Geo<128, 4>{}) : f(Geo<128, 1>{});
        case 256: return vec4 ? f(Geo<256, 4>{}) : f(Geo<256, 1>{});
        case 512: return vec4 ? f(Geo<512, 4>{}) : f(Geo<512, 1>{});
        case 1024: return vec4 ? f(Geo<1024, 4>{}) : f(Geo<1024, 1>{});
    }
    return fail(COALA_EINVAL, "unsupported cache_dim %u", cache_dim);
}

template <int CD, int VEC> constexpr int geo_cd(Geo<CD, VEC>) { return CD; }
template <int CD, int VEC> constexpr int geo_vec(Geo<CD, VEC>) { return VEC; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Split `count` host ranges into RangeSets of at most kMaxRanges ranges each and call f(rs) for every one.
template <typename F>
int for_each_range_set(const int64_t* begins, const int64_t* ends, int count, F&& f) {
    RangeSet rs;
    rs.n = 0;
    rs.total = 0;
    rs.vstart[0] = 0;
    for (int k = 0; k < count; ++k) {
        if (ends[k] <= begins[k]) continue;
        rs.begin[rs.n] = (uint32_t)begins[k];
        rs.total += (uint32_t)(ends[k] - begins[k]);
        rs.vstart[++rs.n] = rs.total;
        if (rs.n == kMaxRanges) {
            if (int rc = f(rs)) return rc;
            rs.n = 0;
            rs.total = 0;
        }
    }
    if (rs.n) return f(rs);
    return COALA_OK;
}

// ---------------------------------------------------------------------------------------------------------- a read
enum { kPhaseProbe = 1, kPhaseFill = 2, kPhaseBoth = 3 };

// One read, as its entry point hands it to read_feature: the phases it runs and the arguments every entry point has, in the ABI's order, and
// below them what an entry point sets by name; then what the steps of read_feature work out, each from what stands above it.
struct FillRanges { const int64_t* begins; const int64_t* ends; int n; };
struct ReadCall {
    int phases;
    coala_cache* h; float* out; const int64_t* idx; int64_t n; hipStream_t stream;
    bool force_dist = true;                               // the owner-partitioned set index whatever the handle's flags say: every serve call
                                                          // (coala_cache_read_feature alone clears it)
    FillRanges ranges{nullptr, nullptr, 0};               // a fill alone: the batch positions it fills
    const coala_row_redirect_t* redirect = nullptr;       // a probe alone
    // Events to put ON the probe's launch (its begin) / on the LAST fill launch of this call (its end) instead of recording them behind it
    // (library-internal callers: the distributed fetch).  rode_begin / rode_end: the event that really rides on that launch: the caller's, or -- a
    // profiling handle uses the dispatches' event slots for its own pairs -- the handle's profiling event of that launch (good for a stream to wait
    // on; it returns to a pool later, so not for timing), or null when the call launched nothing there: the caller then records its event the plain way.
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    hipEvent_t rode_begin = nullptr, rode_end = nullptr;
    // check_read
    bool nothing_to_do = false;
    Redirect rd{0, 0, nullptr, nullptr};
    int64_t whole[2] = {0, 0};                            // a whole read fills the one range [0, n)
    OpenBatch::Ranges claim; int64_t fill_rows = 0;       // a fill alone: OpenBatch::check_ranges
    // choose_events
    bool own_ring = false;
    // kernel_args
    uint32_t gen; bool redir, vec4, list_form; CacheDev d;
};

// Every refusal, always in this order, and what the call fills.  No HIP call, and nothing of the handle's changes but last_begin / last_end.
int check_read(ReadCall& c) {
    coala_cache* h = c.h;
    if (!h) return fail(COALA_EINVAL, "null handle");
    h->last_begin = h->last_end = nullptr; // (set again by finish_read when this call launches a whole read with its events attached)
    if (c.n < 0 || c.n > 0x7FFFFFFFll) return fail(COALA_EINVAL, "n=%lld out of range", (long long)c.n);
    if (c.phases & kPhaseProbe) {
        if (h->batch.is_open()) return h->batch.refuse_while_open();
    } else if (h->batch.rows != c.n || h->gen == 0) {
        return fail(COALA_EINVAL, "serve_fill without a matching serve_probe (batch of %lld rows, probe saw %lld)", (long long)c.n, (long long)h->batch.rows);
    }
    c.nothing_to_do = c.n == 0;
    if (c.nothing_to_do) return COALA_OK;
    if (!c.idx || (!c.out && !(c.redirect && c.redirect->begin == 0 && c.redirect->end == c.n))) return fail(COALA_EINVAL, "null buffer");
    if (!(c.phases & kPhaseProbe)) {
        c.rd = h->batch.redirect;
    } else if (c.redirect && c.redirect->end > c.redirect->begin) {
        if (c.redirect->begin < 0 || c.redirect->end > c.n || !c.redirect->out)
            return fail(COALA_EINVAL, "redirect [%lld, %lld) outside the batch of %lld rows, or null destination", (long long)c.redirect->begin, (long long)c.redirect->end, (long long)c.n);
        c.rd = Redirect{c.redirect->begin, c.redirect->end, c.redirect->out, c.redirect->row_map};
    }
    if (c.phases == kPhaseBoth) {
        c.whole[1] = c.fill_rows = c.n;
        c.ranges = FillRanges{&c.whole[0], &c.whole[1], 1};
    } else if (c.phases == kPhaseFill) {
        if (int rc = h->batch.check_ranges(c.ranges.begins, c.ranges.ends, c.ranges.n, &c.claim, &c.fill_rows)) return rc;
        c.nothing_to_do = c.fill_rows == 0;
    }
    return COALA_OK;
}

// The events that ride on the launches: the handle's own pair of this call (coala_cache_fetch_events: a whole read = K1 + one K2 launch, begin on
// the first dispatch, end on the second), else the caller's.  A profiling handle keeps the dispatches' event slots for itself (ProfScope).
int choose_events(ReadCall& c) {
    coala_cache* h = c.h;
    if (h->cfg.flags & COALA_FLAG_PROFILE) {
        c.ev_begin = c.ev_end = nullptr;
    } else if (h->fetch_events && c.phases == kPhaseBoth) {
        if (h->fev.empty()) h->fev.assign(2 * (size_t)coala_cache::kFetchRing, nullptr);
        const size_t slot = (size_t)(h->fev_calls % coala_cache::kFetchRing);
        for (size_t k = 2 * slot; k < 2 * slot + 2; ++k)
            if (!h->fev[k]) HIPCHK(hipEventCreate(&h->fev[k]));
        c.ev_begin = h->fev[2 * slot];
        c.ev_end = h->fev[2 * slot + 1];
        c.own_ring = true;
    }
    return COALA_OK;
}

// A probe starts a generation.  One that runs alone leaves its batch open for the fills.
int next_generation(ReadCall& c) {
    coala_cache* h = c.h;
    h->fill_launches = 0;
    if (++h->gen == 0) { // generation wrapped: clear the chain heads and the generation tags of the cursors once
        HIPCHK(hipMemsetAsync(h->d.set_head, 0, h->d.num_sets * 8, c.stream));
        HIPCHK(hipMemset2DAsync(reinterpret_cast<char*>(h->d.set_cnt) + 4, 8, 0, 4, h->d.num_sets, c.stream));
        HIPCHK(hipMemsetAsync(h->d.stats + kStatList, 0, (size_t)(kStatWords - kStatList) * 8, c.stream));   // (generation 1 follows an odd one: its list counters were not cleared)
        h->gen = 1;
    }
    if (c.phases == kPhaseProbe) h->batch.open(c.n, c.rd);
    return COALA_OK;
}

// What the kernels of this call get, and which of them run: after ensure_scratch and next_generation, which change what is copied here.
void kernel_args(ReadCall& c) {
    const coala_cache* h = c.h;
    c.gen = h->gen;
    c.redir = c.rd.end > c.rd.begin;
    c.vec4 = (h->d.dim % 4 == 0) && aligned16(c.out) && aligned16(h->d.cold) && (!c.redir || aligned16(c.rd.out));
    c.d = h->d;
    if (c.force_dist) c.d.distributed = 1u;
    // a whole read on a host tier: the probe keeps the batch's miss list and the fill streams from it (ranged fills: the tile form, no list)
    c.list_form = c.phases == kPhaseBoth && h->host_tier;
    if (!c.list_form) c.d.list_sub = 0;
}

// K1's variants.  The redirecting one carries a destination per row: with 16 rows per chunk (512-B lines, 8 passes) it spills -> half the passes there.
template <int CD, int VEC, int NP> constexpr int kRedirectPasses = (Geo<CD, VEC, NP>::R > 8) ? NP / 2 : NP;
using ProbeKernel = void (*)(const int64_t*, float*, int64_t, uint32_t, uint32_t, CacheDev, Redirect);
template <int CD, int VEC, typename TAG, int NP>
ProbeKernel probe_kernel(bool full, bool redir, bool single) {
    constexpr int NPR = kRedirectPasses<CD, VEC, NP>;
    static constexpr ProbeKernel variant[2][2][2] = { // [redir][full][single]
        {{probe_gather_kernel<CD, VEC, TAG, NP, false, false, false>, probe_gather_kernel<CD, VEC, TAG, NP, false, false, true>},
         {probe_gather_kernel<CD, VEC, TAG, NP, true, false, false>, probe_gather_kernel<CD, VEC, TAG, NP, true, false, true>}},
        {{probe_gather_kernel<CD, VEC, TAG, NPR, false, true, false>, probe_gather_kernel<CD, VEC, TAG, NPR, false, true, true>},
         {probe_gather_kernel<CD, VEC, TAG, NPR, true, true, false>, probe_gather_kernel<CD, VEC, TAG, NPR, true, true, true>}}};
    return variant[redir][full][single];
}

// K1: 2-wave blocks, every wave resident; one wave per chunk, or grid-stride over the chunks
template <int CD, int VEC, typename TAG, int NP>
int launch_probe_as(ReadCall& c) {
    const LaunchShape& ls = c.h->shape;
    const int rows = c.redir ? Geo<CD, VEC, kRedirectPasses<CD, VEC, NP>>::R : Geo<CD, VEC, NP>::R;   // per chunk
    const int64_t chunks = (c.n + rows - 1) / rows;
    const bool full = (VEC == 4) && ((int)c.d.dim == CD);
    const bool single = ls.k1_single && chunks <= kK1SingleMaxChunks;
    const dim3 grid(grid1d(chunks, ls.k1_waves, single ? (int)((kK1SingleMaxChunks + ls.k1_waves - 1) / ls.k1_waves) : ls.k1_grid_cap)), block(64 * ls.k1_waves);
    ProfScope ps(c.h, c.stream, 0, (uint64_t)c.n, c.ev_begin, nullptr);
    c.rode_begin = ps.on ? ps.a : c.ev_begin;
    ps.launch(probe_kernel<CD, VEC, TAG, NP>(full, c.redir, single), grid, block, c.idx, c.out, c.n, c.gen, (uint32_t)grid.x, c.d, c.rd);
    return COALA_OK;
}

template <int CD, int VEC, typename TAG>
int launch_probe_of(ReadCall& c) {
#ifdef COALA_DEV_KNOBS
    switch (c.h->shape.k1_passes) { // development builds: rows in flight per wave from the environment
        case 0: break;
        case 2: return launch_probe_as<CD, VEC, TAG, 2>(c);
        case 8: return launch_probe_as<CD, VEC, TAG, 8>(c);
        case 16: return launch_probe_as<CD, VEC, TAG, (Geo<CD, VEC, 16>::R <= 32 ? 16 : 8)>(c);
        default: return launch_probe_as<CD, VEC, TAG, 4>(c);
    }
#endif
    return launch_probe_as<CD, VEC, TAG, kK1Passes>(c);
}

int launch_probe(ReadCall& c) {
    return dispatch_geo(c.d.cache_dim, c.vec4, [&](auto geo) -> int {
        constexpr int CD = geo_cd(geo);
        constexpr int VEC = geo_vec(geo);
        return c.d.tag32 ? launch_probe_of<CD, VEC, uint32_t>(c) : launch_probe_of<CD, VEC, uint64_t>(c);
    });
}

// K2 streaming from the miss list the batch's probe kept: one launch, which draws its groups from the batch's first ticket counter
template <int CD, int VEC>
int launch_fill_list(ReadCall& c) {
    constexpr int R = Geo<CD, VEC>::R;
    ProfScope ps(c.h, c.stream, 2, 0, nullptr, c.ev_end);
    c.rode_end = ps.on ? ps.b : c.ev_end;
    c.h->fill_launches++;
    ps.launch(miss_fill_list_kernel<CD, VEC>, dim3(grid1d((c.n + R - 1) / R, 4, c.h->shape.k2_grid_cap)), dim3(256), c.d, c.idx, c.out, c.gen);
    return COALA_OK;
}

// K2 over verdict tiles of the call's ranges: one launch per kMaxRanges ranges, the end event on the last one
template <int CD, int VEC>
int launch_fill_tiles(ReadCall& c) {
    coala_cache* h = c.h;
    const int tile_rows = h->shape.k2_tile_rows > 0 ? h->shape.k2_tile_rows : Geo<CD, VEC>::R;
    int live = 0, set_no = 0;
    for (int k = 0; k < c.ranges.n; ++k) live += c.ranges.ends[k] > c.ranges.begins[k];
    const int n_sets = (live + kMaxRanges - 1) / kMaxRanges;
    return for_each_range_set(c.ranges.begins, c.ranges.ends, c.ranges.n, [&](const RangeSet& rs) -> int {
        const bool last_set = ++set_no == n_sets;
        ProfScope ps(h, c.stream, 2, 0, nullptr, last_set ? c.ev_end : nullptr);
        if (last_set) c.rode_end = ps.on ? ps.b : c.ev_end;
        const int64_t tiles = ((int64_t)rs.total + tile_rows - 1) / tile_rows;
        const dim3 grid(grid1d(tiles, 4, h->shape.k2_grid_cap));
        // dynamic deal (host tier, more tiles than waves, one of the batch's first kFillSlots fill launches): this launch's ticket counter
        const int64_t waves = (int64_t)grid.x * 4;
        int dyn_slot = -1;
        if (h->shape.k2_unit_tiles > 0 && tiles > waves && tiles < 0x7FFFFFFF && h->fill_launches < kFillSlots)
            dyn_slot = (int)((c.gen & 1u) * kFillSlots) + h->fill_launches;
        h->fill_launches++;
        ps.launch(c.redir ? miss_fill_kernel<CD, VEC, true> : miss_fill_kernel<CD, VEC, false>, grid, dim3(256), c.d, c.idx, c.out, tile_rows,
                  h->shape.k2_sparse_max, c.gen, rs, c.rd, dyn_slot);
        return COALA_OK;
    });
}

// A whole read on a host tier fills from the list, every other one from verdict tiles (kernel_args)
int launch_fill(ReadCall& c) {
    return dispatch_geo(c.d.cache_dim, c.vec4, [&](auto geo) -> int {
        constexpr int CD = geo_cd(geo);
        constexpr int VEC = geo_vec(geo);
        return c.list_form ? launch_fill_list<CD, VEC>(c) : launch_fill_tiles<CD, VEC>(c);
    });
}

// What a read that was enqueued leaves on the handle.  (A fill's ranges count as filled from here on, not from check_read: a call that a HIP
// error ends before its launches leaves the batch as it found it, and the same fill can be sent again.)
int finish_read(ReadCall& c) {
    coala_cache* h = c.h;
    if (c.own_ring) {
        h->last_begin = c.ev_begin;
        h->last_end = c.ev_end;
        h->fev_calls++;
    }
    if (c.phases & kPhaseProbe) h->rows_total += (uint64_t)c.n;
    if (c.phases == kPhaseFill) h->batch.commit(c.claim, c.fill_rows);
    return leave(h, c.stream);
}

int read_feature(ReadCall& c) {
    if (int rc = check_read(c)) return rc;
    if (c.nothing_to_do) return COALA_OK;
    if (int rc = enter(c.h, c.stream)) return rc;
    if (int rc = ensure_scratch(c.h, (uint64_t)c.n, c.stream)) return rc;
    if (int rc = choose_events(c)) return rc;
    if (c.phases & kPhaseProbe)
        if (int rc = next_generation(c)) return rc;
    kernel_args(c);
    if (c.phases & kPhaseProbe)
        if (int rc = launch_probe(c)) return rc;
    if (c.fill_rows > 0)
        if (int rc = launch_fill(c)) return rc;   // launch_fill_list or launch_fill_tiles
    return finish_read(c);
}

} // namespace

extern "C" {

int coala_cache_dim(int dim) { // ssd_gnn_cache.cuh:34-44
    if (dim <= 0) return fail(COALA_EINVAL, "dim must be positive");
    if (dim <= 128) return 128;
    if (dim <= 256) return 256;
    if (dim <= 512) return 512;
    if (dim <= 1024) return 1024;
    return fail(COALA_EINVAL, "Only Feature Embedding Size less than 8KB is supported");
}

uint64_t coala_cache_num_sets(uint64_t cache_mb, int cache_dim) { // ssd_gnn_cache.cuh:96-97
    if (cache_dim <= 0) return 0;
    const uint64_t page = (uint64_t)cache_dim * sizeof(float);
    return (cache_mb * 1024ull * 1024ull / page) / COALA_WAYS;
}

int coala_cache_create(const coala_cache_config_t* cfg, coala_cache_t** out) {
    if (!cfg || !out) return fail(COALA_EINVAL, "null argument");
    *out = nullptr;
    const int cd = coala_cache_dim(cfg->dim);
    if (cd < 0) return cd;
    if (!cfg->cold_table) return fail(COALA_EINVAL, "cold_table is null (the NVMe/BaM tier is out of scope: pass the pinned feature table)");
    if (cfg->n_gpus < 1 || cfg->rank < 0 || cfg->rank >= cfg->n_gpus) return fail(COALA_EINVAL, "bad rank/n_gpus");
    const uint64_t sets = coala_cache_num_sets(cfg->cache_mb, cd);
    if (sets == 0) return fail(COALA_EINVAL, "cache_mb=%llu gives zero sets", (unsigned long long)cfg->cache_mb);
    if (sets * COALA_WAYS > 0xFFFFFFFFull) return fail(COALA_EINVAL, "cache too large: more than 2^32 lines");
    if (cfg->node_color && cfg->num_colors < 0) return fail(COALA_EINVAL, "num_colors < 0");
    HIPCHK(hipSetDevice(cfg->device));
    coala_cache* h = new (std::nothrow) coala_cache();
    if (!h) return fail(COALA_ENOMEM, "out of host memory");
    h->cfg = *cfg;
    CacheDev& d = h->d;
    memset(&d, 0, sizeof(d));
    const uint64_t slots = sets * COALA_WAYS;
    d.num_sets = sets;
    d.num_rows = cfg->num_rows;
    d.cache_dim = (uint32_t)cd;
    d.dim = (uint32_t)cfg->dim;
    d.n_gpus = (uint32_t)cfg->n_gpus;
    d.gshift = ilog2_exact((uint64_t)cfg->n_gpus);
    d.sshift = ilog2_exact(sets);
    d.distributed = (cfg->flags & COALA_FLAG_DISTRIBUTED) ? 1u : 0u;
    d.cold_partitioned = (cfg->flags & COALA_FLAG_COLD_PARTITIONED) ? 1u : 0u;
    d.cold = cfg->cold_table;
    // 32-bit tags whenever every id fits (0xFFFFFFFF is the empty tag): a set is then one 128-B line instead of two
    d.tag32 = (!(cfg->flags & COALA_FLAG_TAG64) && cfg->num_rows <= 0xFFFFFFFFull) ? 1u : 0u;
    const uint64_t tag_bytes = d.tag32 ? 4 : 8;
    int rc = COALA_OK;
    auto alloc = [&](void** p, uint64_t bytes) -> int {
        hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) return fail(COALA_ENOMEM, "hipMalloc(%llu) failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
        h->table_bytes += bytes;
        return COALA_OK;
    };
    do {
        if ((rc = alloc((void**)&d.keys, slots * tag_bytes))) break;
        if ((rc = alloc((void**)&d.set_cnt, sets * 8))) break;
        if ((rc = alloc((void**)&d.color_meta, slots * 4))) break;
        if ((rc = alloc((void**)&d.set_head, sets * 8))) break;
        if ((rc = alloc((void**)&d.stats, kStatWords * 8))) break;   // (the per-block sums and what lies behind them: kStatWriteBad ... kStatList)
        if ((rc = alloc((void**)&d.lines, slots * (uint64_t)cd * 4))) break;
        if ((rc = alloc((void**)&h->route_bases, (kMaxParts + 1) * sizeof(int64_t)))) break;
        if (hipMemset(d.keys, 0xFF, slots * tag_bytes) != hipSuccess || hipMemset(d.set_cnt, 0, sets * 8) != hipSuccess ||
            hipMemset(d.color_meta, 0, slots * 4) != hipSuccess || hipMemset(d.set_head, 0, sets * 8) != hipSuccess ||
            hipMemset(d.stats, 0, kStatWords * 8) != hipSuccess) {
            rc = fail(COALA_EHIP, "hipMemset failed");
            break;
        }
        if (cfg->node_color) {
            if ((rc = alloc((void**)&d.color_counters, ((uint64_t)cfg->num_colors + 1) * 4))) break;
            if (hipMemset(d.color_counters, 0, ((uint64_t)cfg->num_colors + 1) * 4) != hipSuccess) { rc = fail(COALA_EHIP, "hipMemset failed"); break; }
            if ((rc = alloc((void**)&h->node_color_dev, cfg->num_rows * 4))) break;
            // narrow int64 colours to int32 on the host in chunks, validating the range
            const uint64_t chunk = 1ull << 22;
            std::vector<int32_t> tmp((size_t)(cfg->num_rows < chunk ? cfg->num_rows : chunk));
            for (uint64_t off = 0; off < cfg->num_rows && rc == COALA_OK; off += chunk) {
                const uint64_t cnt = cfg->num_rows - off < chunk ? cfg->num_rows - off : chunk;
                for (uint64_t k = 0; k < cnt; ++k) {
                    const int64_t col = cfg->node_color[off + k];
                    if (col < 0 || col > cfg->num_colors) { rc = fail(COALA_EINVAL, "node_color[%llu]=%lld outside [0,%d]", (unsigned long long)(off + k), (long long)col, cfg->num_colors); break; }
                    tmp[k] = (int32_t)col;
                }
                if (rc == COALA_OK && hipMemcpy(h->node_color_dev + off, tmp.data(), cnt * 4, hipMemcpyHostToDevice) != hipSuccess)
                    rc = fail(COALA_EHIP, "colour upload failed");
            }
            if (rc) break;
            d.node_color = h->node_color_dev;
        }
        h->gen = 0;
        {
            hipPointerAttribute_t attr;
            const bool host_tier = hipPointerGetAttributes(&attr, cfg->cold_table) == hipSuccess && attr.type == hipMemoryTypeHost;
            (void)hipGetLastError(); // an unregistered pointer is reported as an error: not ours to keep
            h->host_tier = host_tier;
            h->shape = launch_shape(d.cache_dim, host_tier);
#ifdef COALA_DEV_KNOBS
            apply_dev_knobs(h->shape);
#endif
        }
        if (cfg->max_batch) rc = ensure_scratch(h, cfg->max_batch, nullptr);
    } while (0);
    if (rc == COALA_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(COALA_EHIP, "device sync failed after create");
    if (rc != COALA_OK) {
        coala_cache_destroy(h); // does not touch the recorded error
        return rc;
    }
    *out = h;
    return COALA_OK;
}

int coala_cache_destroy(coala_cache_t* h) {
    if (!h) return COALA_OK;
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();
    drain_events(h);   // (the pool's events, and the stream order's, go with the handle)
    for (auto e : h->fev)
        if (e) (void)hipEventDestroy(e);
    CacheDev& d = h->d;
    void* ptrs[] = {d.keys, d.set_cnt, d.color_meta, d.set_head, d.stats, d.lines, d.color_counters,
                    h->node_color_dev, d.miss_link, d.miss_list,
                    h->wave_counts, h->route_bases};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (h->color_pin) (void)hipHostFree(h->color_pin);
    if (h->color_pin_async) (void)hipHostFree(h->color_pin_async);
    if (h->color_ev) (void)hipEventDestroy(h->color_ev);
    delete h;
    return COALA_OK;
}

int64_t coala_cache_row_dim(const coala_cache_t* h) { return h ? (int64_t)h->d.dim : 0; }

int coala_cache_fetch_events(coala_cache_t* h, int enable) {
    if (!h) return fail(COALA_EINVAL, "null handle");
    h->fetch_events = enable != 0;
    if (!h->fetch_events) h->last_begin = h->last_end = nullptr;
    return COALA_OK;
}

int coala_cache_last_fetch_events(const coala_cache_t* h, void** begin_ev, void** end_ev) {
    if (!h) return fail(COALA_EINVAL, "null handle");
    if (begin_ev) *begin_ev = (void*)h->last_begin;
    if (end_ev) *end_ev = (void*)h->last_end;
    return COALA_OK;
}

int coala_stream_wait_event(void* stream, void* event) {
    if (!event) return fail(COALA_EINVAL, "null event");
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
    return COALA_OK;
}

int coala_event_elapsed_ms(void* begin_ev, void* end_ev, int wait, float* ms_out) {
    if (!begin_ev || !end_ev || !ms_out) return fail(COALA_EINVAL, "null argument");
    if (wait) HIPCHK(hipEventSynchronize((hipEvent_t)end_ev));
    else {
        const hipError_t q = hipEventQuery((hipEvent_t)end_ev);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();
            return 1; // not finished yet: no error, no message
        }
        if (q != hipSuccess) return fail(COALA_EHIP, "hipEventQuery failed: %s", hipGetErrorString(q));
    }
    HIPCHK(hipEventElapsedTime(ms_out, (hipEvent_t)begin_ev, (hipEvent_t)end_ev));
    return COALA_OK;
}

int coala_cache_geometry(const coala_cache_t* h, coala_cache_geometry_t* out) {
    if (!h || !out) return fail(COALA_EINVAL, "null argument");
    out->num_sets = h->d.num_sets;
    out->num_ways = COALA_WAYS;
    out->cache_dim = h->d.cache_dim;
    out->line_bytes = (uint64_t)h->d.cache_dim * 4;
    out->table_bytes = h->table_bytes;
    out->tag_set_bytes = h->d.tag32 ? COALA_WAYS * 4u : COALA_WAYS * 8u;
    out->reserved = 0;
    return COALA_OK;
}

int coala_cache_read_feature(coala_cache_t* h, float* out, const int64_t* idx, int64_t n, void* stream) {
    ReadCall c{kPhaseBoth, h, out, idx, n, (hipStream_t)stream};
    c.force_dist = false;
    return read_feature(c);
}

int coala_cache_serve(coala_cache_t* h, float* out, const int64_t* ids, int64_t n, void* stream) {
    ReadCall c{kPhaseBoth, h, out, ids, n, (hipStream_t)stream};
    return read_feature(c);
}

int coala_cache_serve_probe(coala_cache_t* h, float* out, const int64_t* ids, int64_t n, void* stream) {
    ReadCall c{kPhaseProbe, h, out, ids, n, (hipStream_t)stream};
    return read_feature(c);
}

int coala_cache_serve_probe_redirect(coala_cache_t* h, float* out, const int64_t* ids, int64_t n, const coala_row_redirect_t* redirect,
                                     void* stream) {
    ReadCall c{kPhaseProbe, h, out, ids, n, (hipStream_t)stream};
    c.redirect = redirect;
    return read_feature(c);
}

// library-internal (coala_internal.h): the split-phase serve with events on its launches
int coala_serve_probe_redirect_ev_(coala_cache_t* h, float* out, const int64_t* ids, int64_t n, const coala_row_redirect_t* redirect, void* stream,
                                   hipEvent_t begin_ev, hipEvent_t* rode) {
    ReadCall c{kPhaseProbe, h, out, ids, n, (hipStream_t)stream};
    c.redirect = redirect;
    c.ev_begin = begin_ev;
    const int rc = read_feature(c);
    if (rode) *rode = c.rode_begin;
    return rc;
}
int coala_serve_fill_ranges_ev_(coala_cache_t* h, float* out, const int64_t* ids, int64_t n, const int64_t* begins, const int64_t* ends, int n_ranges,
                                void* stream, hipEvent_t end_ev, hipEvent_t* rode) {
    ReadCall c{kPhaseFill, h, out, ids, n, (hipStream_t)stream};
    c.ranges = FillRanges{begins, ends, n_ranges};
    c.ev_end = end_ev;
    const int rc = read_feature(c);
    if (rode) *rode = c.rode_end;
    return rc;
}

int coala_cache_serve_fill(coala_cache_t* h, float* out, const int64_t* ids, int64_t n, int64_t begin, int64_t end, void* stream) {
    ReadCall c{kPhaseFill, h, out, ids, n, (hipStream_t)stream};
    c.ranges = FillRanges{&begin, &end, 1};
    return read_feature(c);
}

int coala_cache_serve_fill_ranges(coala_cache_t* h, float* out, const int64_t* ids, int64_t n, const int64_t* begins, const int64_t* ends,
                                  int n_ranges, void* stream) {
    ReadCall c{kPhaseFill, h, out, ids, n, (hipStream_t)stream};
    c.ranges = FillRanges{begins, ends, n_ranges};
    return read_feature(c);
}

int coala_cache_serve_abort(coala_cache_t* h, void* stream) {
    if (!h) return fail(COALA_EINVAL, "null handle");
    if (!h->batch.is_open()) return COALA_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    // nothing on the device to undo: the next probe starts a new generation and rewrites every verdict word it will read; rows
    // whose fill already ran are cached, the others are not
    (void)stream;
    h->batch.close();
    return COALA_OK;
}

int coala_cache_route(coala_cache_t* h, const int64_t* idx, int64_t n, int n_parts, int64_t bucket_stride,
                      int64_t* node_out, int64_t* map_out, int64_t* counts_out, int64_t* offsets_out, void* stream) {
    if (!h) return fail(COALA_EINVAL, "null handle");
    if (n < 0 || n_parts < 1 || n_parts > kMaxParts) return fail(COALA_EINVAL, "bad n or n_parts (1..64)");
    if (!node_out || !map_out || !counts_out || (n > 0 && !idx)) return fail(COALA_EINVAL, "null buffer");
    if (bucket_stride < 0) return fail(COALA_EINVAL, "negative bucket_stride");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = enter(h, s)) return rc;
    const int64_t n_tiles = partition_tiles(n);
    const uint64_t need = (uint64_t)(n_tiles > 0 ? n_tiles : 1) * (uint64_t)n_parts;
    if (int rc = grow((void**)&h->wave_counts, &h->wave_counts_cap, need, sizeof(uint32_t), s, 4096)) return rc;
    const int pshift = ilog2_exact((uint64_t)n_parts);
    const dim3 grid = partition_grid(n_tiles), blk(kBlock);
    if (n_tiles > 0) hipLaunchKernelGGL(route_count_kernel, grid, blk, 0, s, idx, n, (uint32_t)n_parts, pshift, h->wave_counts);
    hipLaunchKernelGGL(route_scan_kernel, dim3(1), partition_scan_block((uint32_t)n_parts), 0, s, h->wave_counts, n, (uint32_t)n_parts, bucket_stride,
                       counts_out, offsets_out, h->route_bases);
    if (n_tiles > 0)
        hipLaunchKernelGGL(route_scatter_kernel, grid, blk, 0, s, idx, n, (uint32_t)n_parts, pshift, (const uint32_t*)h->wave_counts,
                           (const int64_t*)h->route_bases, node_out, map_out);
    return leave(h, s);
}

int coala_cache_scatter_ranges(coala_cache_t* h, float* out, const float* src, const int64_t* map, const int64_t* begins,
                               const int64_t* ends, int n_ranges, void* stream) {
    if (!h) return fail(COALA_EINVAL, "null handle");
    if (n_ranges < 0 || (n_ranges > 0 && (!begins || !ends))) return fail(COALA_EINVAL, "bad ranges");
    int64_t rows = 0;
    for (int k = 0; k < n_ranges; ++k) {
        if (begins[k] < 0 || ends[k] < begins[k] || ends[k] > 0x7FFFFFFFll) return fail(COALA_EINVAL, "bad range [%lld, %lld)", (long long)begins[k], (long long)ends[k]);
        rows += ends[k] - begins[k];
    }
    if (rows == 0) return COALA_OK;
    if (!out || !src || !map) return fail(COALA_EINVAL, "null buffer");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = enter(h, s, false)) return rc;   // (touches nothing of the handle's on the device: no order to keep)
    const uint32_t dim = h->d.dim;
    const bool vec4 = (dim % 4 == 0) && aligned16(out) && aligned16(src);
    int rc = dispatch_geo(h->d.cache_dim, vec4, [&](auto geo) -> int {
        constexpr int CD = geo_cd(geo);
        constexpr int VEC = geo_vec(geo);
        using G = Geo<CD, VEC>;
        return for_each_range_set(begins, ends, n_ranges, [&](const RangeSet& rs) -> int {
            const int64_t chunks = ((int64_t)rs.total + G::R - 1) / G::R;
            hipLaunchKernelGGL((scatter_rows_kernel<CD, VEC>), dim3(grid1d(chunks, 4, 256 * 16)), dim3(256), 0, s, out, src, map, rs, dim);
            return COALA_OK;
        });
    });
    return rc ? rc : leave(h, s);
}

int coala_cache_scatter(coala_cache_t* h, float* out, const float* src, const int64_t* map, int64_t n, void* stream) {
    if (n < 0) return fail(COALA_EINVAL, "negative n");
    const int64_t b = 0;
    return coala_cache_scatter_ranges(h, out, src, map, &b, &n, 1, stream);
}

// coala_cache_write_rows / _adagrad_rows / _adam_rows / _rowwise_adagrad_rows: every refusal comes before the first launch; one kernel
// (write_rows_kernel).
static int write_rows_impl(coala_cache_t* h, const int64_t* ids, int64_t n, const float* src, float* state, int op, float a, float eps,
                           void* stream, const WriteExtra& ex = WriteExtra{}) {
    if (!h) return fail(COALA_EINVAL, "null handle");
    if (n < 0 || n > 0x7FFFFFFFll) return fail(COALA_EINVAL, "n=%lld out of range", (long long)n);
    if (op < kOpAssign || op > kOpRowAdagrad) return fail(COALA_EINVAL, "write mode %d outside 0..1", op);
    if (h->cfg.n_gpus != 1 || (h->cfg.flags & (COALA_FLAG_DISTRIBUTED | COALA_FLAG_COLD_PARTITIONED)))
        return fail(COALA_EINVAL, "row writes need an isolated cache of one GPU (n_gpus=%d, flags=0x%x): a second cache over the same table would keep stale lines",
                    h->cfg.n_gpus, h->cfg.flags);
    if (h->batch.is_open()) return h->batch.refuse_while_open();
    const bool elem_state = op == kOpAdagrad || op == kOpAdam;   // state tables of [num_rows, dim]
    if (n > 0 && (!ids || !src || (op >= kOpAdagrad && !state) || (op == kOpAdam && !ex.state2))) return fail(COALA_EINVAL, "null buffer");
    if (n == 0) return COALA_OK;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = enter(h, s)) return rc;
    const CacheDev& d = h->d;
    const bool vec4 = (d.dim % 4 == 0) && aligned16(d.cold) && aligned16(src) && (!elem_state || aligned16(state)) &&
                      (op != kOpAdam || aligned16(ex.state2));
    int rc = dispatch_geo(d.cache_dim, vec4, [&](auto geo) -> int {
        constexpr int CD = geo_cd(geo);
        constexpr int VEC = geo_vec(geo);
        auto launch = [&](auto tag_c) {
            using TAG = decltype(tag_c);
            const int64_t chunks = (n + TagGeo<TAG>::SPL - 1) / TagGeo<TAG>::SPL;
            // one wave per chunk up to 4096 waves behind a host tier (a wave has at most two rows of reads and writes on the link), 32768 on HBM
            const dim3 grid(grid1d(chunks, 4, h->host_tier ? 1024 : 8192)), block(256);
            auto k = op == kOpAssign    ? write_rows_kernel<CD, VEC, TAG, kOpAssign>
                     : op == kOpAdd     ? write_rows_kernel<CD, VEC, TAG, kOpAdd>
                     : op == kOpAdagrad ? write_rows_kernel<CD, VEC, TAG, kOpAdagrad>
                     : op == kOpAdam    ? write_rows_kernel<CD, VEC, TAG, kOpAdam>
                                        : write_rows_kernel<CD, VEC, TAG, kOpRowAdagrad>;
            hipLaunchKernelGGL(k, grid, block, 0, s, ids, src, state, n, a, eps, d, ex);
        };
        if (d.tag32) launch(uint32_t{}); else launch(uint64_t{});
        return COALA_OK;
    });
    return rc ? rc : leave(h, s);
}

int coala_cache_write_rows(coala_cache_t* h, const int64_t* ids, int64_t n, const float* src, int mode, float alpha, void* stream) {
    if (h && mode != 0 && mode != 1) return fail(COALA_EINVAL, "write mode %d outside 0..1", mode);
    return write_rows_impl(h, ids, n, src, nullptr, mode == 0 ? kOpAssign : kOpAdd, alpha, 0.0f, stream);
}

int coala_cache_adagrad_rows(coala_cache_t* h, const int64_t* ids, int64_t n, const float* grad, float* state, float lr, float eps,
                             void* stream) {
    return write_rows_impl(h, ids, n, grad, state, kOpAdagrad, lr, eps, stream);
}

int coala_cache_adam_rows(coala_cache_t* h, const int64_t* ids, int64_t n, const float* grad, float* exp_avg, float* exp_avg_sq,
                          int32_t* row_step, int64_t step, float lr, float beta1, float beta2, float eps, void* stream) {
    if (h && !(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f))
        return fail(COALA_EINVAL, "Adam: betas (%g, %g) outside [0, 1)", (double)beta1, (double)beta2);
    if (h && !row_step && step < 1) return fail(COALA_EINVAL, "Adam: step=%lld without a row_step vector, steps count from 1", (long long)step);
    WriteExtra ex{};
    ex.state2 = exp_avg_sq;
    ex.row_step = row_step;
    ex.ln_b1 = std::log((double)beta1);   // (-inf for beta = 0: -expm1(-inf) = 1, no correction)
    ex.ln_b2 = std::log((double)beta2);
    ex.step = (double)step;
    ex.b1 = beta1;
    ex.b2 = beta2;
    const double omb1 = 1.0 - (double)beta1;
    ex.omb1 = (float)omb1;
    ex.omb1_lo = (float)(omb1 - (double)ex.omb1);
    ex.omb2 = (float)(1.0 - (double)beta2);
    return write_rows_impl(h, ids, n, grad, exp_avg, kOpAdam, lr, eps, stream, ex);
}

int coala_cache_rowwise_adagrad_rows(coala_cache_t* h, const int64_t* ids, int64_t n, const float* grad, float* row_state, float lr,
                                     float eps, void* stream) {
    return write_rows_impl(h, ids, n, grad, row_state, kOpRowAdagrad, lr, eps, stream);
}

int coala_cache_color_counts(coala_cache_t* h, int32_t* dst, int32_t n_entries, void* stream) {
    if (!h || !dst) return fail(COALA_EINVAL, "null argument");
    if (n_entries < 0 || n_entries > h->cfg.num_colors + 1) return fail(COALA_EINVAL, "n_entries=%d exceeds num_colors+1=%d", n_entries, h->cfg.num_colors + 1);
    if (!h->d.color_counters) { memset(dst, 0, (size_t)n_entries * 4); return COALA_OK; }
    hipStream_t s = (hipStream_t)stream;
    if (int rc = enter(h, s)) return rc;
    // staged through pinned memory owned by the handle: a D2H copy into pageable memory waits for every queue of the device
    // (measured: 11 ms per call when a prefetching loader had run ahead), this one only for `stream`
    if (!h->color_pin) HIPCHK(hipHostMalloc((void**)&h->color_pin, ((size_t)h->cfg.num_colors + 1) * 4, hipHostMallocDefault));
    HIPCHK(hipMemcpyAsync(h->color_pin, h->d.color_counters, (size_t)n_entries * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memcpy(dst, h->color_pin, (size_t)n_entries * 4);
    return COALA_OK;
}

// The same snapshot without a host wait at the point of the call: _async enqueues the copy on `stream` (same position in the stream
// as the synchronous call) and returns; _finish, from any thread, waits for exactly that copy and hands the counters over.  The
// loader's scheduler reads the counters every refresh_counter steps and only feeds them to a helper thread: blocking the thread
// that enqueues the next fetch for the ~1.5 ms the previous fetch still runs cost an idle gap on the fetch stream every time.
int coala_cache_color_counts_async(coala_cache_t* h, int32_t n_entries, void* stream) {
    if (!h) return fail(COALA_EINVAL, "null argument");
    if (n_entries < 0 || n_entries > h->cfg.num_colors + 1) return fail(COALA_EINVAL, "n_entries=%d exceeds num_colors+1=%d", n_entries, h->cfg.num_colors + 1);
    if (h->color_pending >= 0) return fail(COALA_EINVAL, "a colour-counter snapshot is already pending: call coala_cache_color_counts_finish first");
    if (int rc = enter(h, (hipStream_t)stream)) return rc;
    if (h->d.color_counters) {
        if (!h->color_pin_async) HIPCHK(hipHostMalloc((void**)&h->color_pin_async, ((size_t)h->cfg.num_colors + 1) * 4, hipHostMallocDefault));
        if (!h->color_ev) HIPCHK(hipEventCreateWithFlags(&h->color_ev, hipEventDisableTiming));
        HIPCHK(hipMemcpyAsync(h->color_pin_async, h->d.color_counters, (size_t)n_entries * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIPCHK(hipEventRecord(h->color_ev, (hipStream_t)stream));
    }
    h->color_pending = n_entries;
    return COALA_OK;
}

int coala_cache_color_counts_finish(coala_cache_t* h, int32_t* dst, int32_t n_entries) {
    if (!h || !dst) return fail(COALA_EINVAL, "null argument");
    if (h->color_pending < 0 || n_entries != h->color_pending) return fail(COALA_EINVAL, "no pending snapshot of %d entries", n_entries);
    if (!h->d.color_counters) {
        memset(dst, 0, (size_t)n_entries * 4);
    } else {
        HIPCHK(hipSetDevice(h->cfg.device));
        HIPCHK(hipEventSynchronize(h->color_ev));
        memcpy(dst, h->color_pin_async, (size_t)n_entries * 4);
    }
    h->color_pending = -1;
    return COALA_OK;
}

static int read_stats(coala_cache_t* h, hipStream_t s, uint64_t* hit, uint64_t* miss, uint64_t* bad, bool reset) {
    std::vector<unsigned long long> part((size_t)kStatHostWords);   // (K2's tickets and flags come along: 72 bytes, and nothing here reads them)
    HIPCHK(hipMemcpyAsync(part.data(), h->d.stats, part.size() * 8, hipMemcpyDeviceToHost, s)); // end of epoch: a device-wide wait is fine
    if (reset) {
        HIPCHK(hipMemsetAsync(h->d.stats, 0, (size_t)kStatBlocks * 2 * 8, s));
        HIPCHK(hipMemsetAsync(h->d.stats + kStatWriteBad, 0, 2 * 8, s));   // (and kStatProbeBad behind it)
    }
    HIPCHK(hipStreamSynchronize(s));
    uint64_t m = 0, b = 0;
    for (int i = 0; i < kStatBlocks; ++i) { m += part[2 * i]; b += part[2 * i + 1]; }
    b += part[kStatProbeBad];   // rejected ids of the reads whose fill streamed from the miss list: counted by their probe
    *miss = m;
    *bad = b + part[kStatWriteBad];   // rejected ids of reads and of writes; only the reads' were counted in rows_total
    *hit = h->rows_total - m - b;
    if (reset) { h->cum_hit += *hit; h->cum_miss += m; h->rows_total = 0; }
    return COALA_OK;
}

int coala_cache_stats(coala_cache_t* h, uint64_t* hit, uint64_t* miss, uint64_t* range_errors, int reset, void* stream) {
    if (!h) return fail(COALA_EINVAL, "null handle");
    if (int rc = enter(h, (hipStream_t)stream)) return rc;
    uint64_t v0, v1, v2;
    int rc = read_stats(h, (hipStream_t)stream, &v0, &v1, &v2, reset != 0);
    if (rc) return rc;
    if (hit) *hit = v0;
    if (miss) *miss = v1;
    if (range_errors) *range_errors = v2;
    return COALA_OK;
}

int coala_cache_dump(coala_cache_t* h, uint64_t* keys, uint32_t* set_cnt, uint32_t* color_meta, void* stream) {
    if (!h) return fail(COALA_EINVAL, "null handle");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = enter(h, s)) return rc;
    const uint64_t slots = h->d.num_sets * COALA_WAYS;
    HIPCHK(hipStreamSynchronize(s));
    if (keys) {
        if (h->d.tag32) { // widened to the reference's 64-bit tags (empty = all ones), in place from the back
            uint32_t* narrow = reinterpret_cast<uint32_t*>(keys);
            HIPCHK(hipMemcpy(narrow, h->d.keys, slots * 4, hipMemcpyDeviceToHost));
            for (uint64_t k = slots; k-- > 0;) keys[k] = narrow[k] == 0xFFFFFFFFu ? kEmptyKey : (uint64_t)narrow[k];
        } else {
            HIPCHK(hipMemcpy(keys, h->d.keys, slots * 8, hipMemcpyDeviceToHost));
        }
    }
    if (set_cnt) HIPCHK(hipMemcpy2D(set_cnt, 4, h->d.set_cnt, 8, 4, h->d.num_sets, hipMemcpyDeviceToHost)); // the cursors without their generation tags
    if (color_meta) HIPCHK(hipMemcpy(color_meta, h->d.color_meta, slots * 4, hipMemcpyDeviceToHost));
    return COALA_OK;
}

int coala_cache_profile(coala_cache_t* h, coala_cache_profile_t* out, int reset) {
    if (!h || !out) return fail(COALA_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    drain_events(h);
    uint64_t v0, v1, v2;
    int rc = read_stats(h, nullptr, &v0, &v1, &v2, false);
    if (rc) return rc;
    const uint64_t th = h->cum_hit + v0, tm = h->cum_miss + v1;
    h->prof.gather_hits = th - h->prof_hit0;
    h->prof.fill_rows = tm - h->prof_miss0;
    if (h->cfg.flags & COALA_FLAG_PROFILE) { // empty brackets on the same stream: the cost of the measurement itself
        std::vector<float> gaps;
        for (int i = 0; i < 16; ++i) {
            hipEvent_t a = h->ev_pool.take(), b = h->ev_pool.take();
            if (!a || !b) break;
            float ms = 0.f;
            if (hipEventRecord(a, h->last_stream) == hipSuccess && hipEventRecord(b, h->last_stream) == hipSuccess &&
                hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess)
                gaps.push_back(ms);
            h->ev_pool.give(a);
            h->ev_pool.give(b);
        }
        if (!gaps.empty()) {
            std::sort(gaps.begin(), gaps.end());
            h->prof.event_overhead_us = gaps[gaps.size() / 2] * 1e3;
        }
    }
    *out = h->prof;
    if (reset) { h->prof = coala_cache_profile_t{}; h->prof_hit0 = th; h->prof_miss0 = tm; }
    return COALA_OK;
}

} // extern "C"
