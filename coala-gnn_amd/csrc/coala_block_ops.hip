// coala_block_ops.hip -- what a model computes on a sampled block (coala_sampler.hip makes the blocks), for gfx950: mean aggregation
// (DGL's SAGEConv "mean"), weighted sum aggregation (DGL's u_mul_e_sum: GraphConv / SAGEConv with edge_weight=), max aggregation
// (DGL's fn.max: SAGEConv "pool", GINConv "max"), the relation-typed sum (RelGraphConv's message step), GAT / GATv2 attention
// aggregation (GATConv's and GATv2Conv's message steps), scaled dot-product attention (DotGatConv's and HGTConv's message step) and
// relation-typed GAT attention (a softmax per destination and relation), forward and backward, on fixed blocks (nbr_local[n_dst, fanout], -1 = no
// neighbour) and on the CSR blocks of full layers; and, for link prediction, edge exclusion on both block forms and the dot-product
// scores of node pairs (forward and backward).  Stateless entry points: no handle, every launch on the caller's stream.
//
// Layout of the file: the device helpers every kernel walks a row with (which rows a wave takes, a row's bounds in either block form,
// the 64-index chunk load, the wave reductions); then one `template <bool CSR>` kernel per op and direction, each written out top to
// bottom on those helpers; then one `*_launch<CSR>` per kernel (shape check, n_dst == 0, null check, launch); then the C entry
// points, which only forward.  The fixed and the CSR instantiation of a kernel are the same code on the same lanes -- a fixed row of
// fan-out <= 32 is a row of one chunk -- so a row both forms can express gives the same bits in both.  A hub row is aggregated by one
// wave (splitting it is not done).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/coala_hip.h"
#include "coala_internal.h"

#define fail coala_fail_
#define HIPCHK COALA_HIPCHK

namespace {

// One wave per destination row: this thread's lane, its wave's first row and the stride to the wave's next row, for a grid of blocks
// of `waves` waves -- `const auto [lane, wave, n_waves] = wave_rows(); for (int64_t d = wave; d < n_dst; d += n_waves)`.
struct WaveRows {
    int lane;
    int64_t wave, n_waves;
};

__device__ __forceinline__ WaveRows wave_rows(int waves = kWavesPerBlock) {
    return {(int)(threadIdx.x & 63), (int64_t)blockIdx.x * waves + (threadIdx.x >> 6), (int64_t)gridDim.x * waves};
}

// Row d's indices: idx[beg .. end), nbr[d * fanout ..] for the fixed form, indices[indptr[d] .. indptr[d+1]) for the CSR form.
template <bool CSR>
__device__ __forceinline__ void row_range(const int64_t* indptr, int fanout, int64_t d, int64_t* beg, int64_t* end) {
    *beg = CSR ? indptr[d] : d * fanout;
    *end = CSR ? indptr[d + 1] : *beg + fanout;
}

// The chunk of a row at e0: lane j takes idx[e0 + j] into *mine, -1 past the row's end; -> the chunk's length, min(64, end - e0).
// The indices then go round by __shfl(mine, j), j < n, which every lane of the wave must execute.
__device__ __forceinline__ int load_chunk(const int32_t* idx, int64_t e0, int64_t end, int lane, int32_t* mine) {
    *mine = e0 + lane < end ? idx[e0 + lane] : -1;
    return end - e0 < 64 ? (int)(end - e0) : 64;
}

__device__ __forceinline__ void wave_lds_sync() { // LDS written by some lanes of a wave, read by others (rocPRIM's wave_barrier)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float wave_sum(float v) { // butterfly: every lane ends with the same bits
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int VEC, typename V>
__device__ __forceinline__ void axpy(V& acc, float a, const V& x) { // one fma per term
    for (int i = 0; i < VEC; ++i) acc[i] = __builtin_fmaf(a, x[i], acc[i]);
}

// Mean aggregation, the one dense-side primitive a consumer of these blocks needs (DGL's SAGEConv "mean" reduces to it): out[d] = the
// mean of the rows h_src[s_j] over the valid slots j of row d.  One wave per destination row, 16-B accesses, the row's indices read
// 64 at a time and broadcast by shuffle; the sum starts from +0 and runs in slot order, so a row both forms can express gives the
// same bits.  The first chunk stays in registers over the passes of a long feature row: a fixed row is that chunk alone, read once.
// The two forms divide differently: the fixed form by the number of valid entries, the CSR form by the row's length (the rule of
// Block.mean_aggregate_torch; a sampled CSR row holds no -1).  Replaces gather -> mask -> sum -> divide in eager torch (four passes
// over a [n_dst, fanout, dim] intermediate).
template <int VEC, bool CSR>
__global__ __launch_bounds__(kBlock) void mean_aggregate_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, int fanout,
                                                                const float* __restrict__ h_src, float* __restrict__ out, int64_t n_dst, int dim) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    const auto [lane, wave, n_waves] = wave_rows();
    const int units = dim / VEC;
    for (int64_t d = wave; d < n_dst; d += n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        int32_t mine0;
        const int n0 = load_chunk(idx, beg, end, lane, &mine0);
        const float cnt = CSR ? (float)(end - beg) : (float)__builtin_popcountll(__ballot(mine0 >= 0));
        const float inv = cnt > 0.0f ? 1.0f / cnt : 0.0f;
        for (int u0 = 0; u0 < units; u0 += 64) { // wave-uniform trip counts: the shuffles below need every lane
            const int u = u0 + lane;
            vf acc = vf(0.0f);
            for (int64_t e0 = beg; e0 < end; e0 += 64) {
                int32_t mine = mine0;
                int n = n0;
                if (e0 != beg) n = load_chunk(idx, e0, end, lane, &mine); // wave-uniform
                for (int j = 0; j < n; ++j) {
                    const int32_t s = __shfl(mine, j);
                    if (s >= 0 && u < units) acc += *reinterpret_cast<const vf*>(h_src + (int64_t)s * dim + (int64_t)u * VEC);
                }
            }
            if (u < units) *reinterpret_cast<vf*>(out + d * dim + (int64_t)u * VEC) = acc * inv;
        }
    }
}

// grad_src[s_j] += grad_out[d] / cnt(d) for the valid slots j of row d, cnt the forward's divisor (grad_src zeroed by the caller;
// hardware float atomics: summation order varies).  A lane per float: an atomic instruction of the wave covers 256 contiguous bytes.
template <bool CSR>
__global__ __launch_bounds__(kBlock) void mean_aggregate_backward_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                                         int fanout, const float* __restrict__ grad_out,
                                                                         float* __restrict__ grad_src, int64_t n_dst, int dim) {
    const auto [lane, wave, n_waves] = wave_rows();
    for (int64_t d = wave; d < n_dst; d += n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        int32_t mine0;
        const int n0 = load_chunk(idx, beg, end, lane, &mine0);
        const float cnt = CSR ? (float)(end - beg) : (float)__builtin_popcountll(__ballot(mine0 >= 0));
        if (!(cnt > 0.0f)) continue;
        const float inv = 1.0f / cnt;
        for (int c0 = 0; c0 < dim; c0 += 64) { // wave-uniform trip count: the shuffles below read lanes that are past `dim`
            const int c = c0 + lane;
            const float g = c < dim ? grad_out[d * dim + c] * inv : 0.0f;
            for (int64_t e0 = beg; e0 < end; e0 += 64) {
                int32_t mine = mine0;
                int n = n0;
                if (e0 != beg) n = load_chunk(idx, e0, end, lane, &mine); // wave-uniform
                for (int j = 0; j < n; ++j) {
                    const int32_t s = __shfl(mine, j);
                    if (s >= 0 && c < dim) unsafeAtomicAdd(grad_src + (int64_t)s * dim + c, g);
                }
            }
        }
    }
}

// GAT attention on a block (DGL GATConv's message step; its projections fc_src / fc_dst and the attn_l / attn_r products are dense
// and stay in torch).  For dst d, head h and the valid in-edges j of d (source s_j):
//   z_j = el[s_j, h] + er[d, h],  e_j = leaky_relu(z_j, slope),  a_j = softmax of e over the row,  out[d, h, :] = sum_j a_j feat[s_j, h, :]
// One wave per destination row, in both block forms.  Per chunk a lane per edge computes its edge's score for every head once, into
// LDS; the feature lanes then sum the rows with those weights, never writing a [n_dst, fanout, H, D] intermediate.  The softmax runs
// online over the chunks: running max m and sum l per head; the partial sum is rescaled by exp(m_old - m_new) when the max grows, and
// it waits in `out`, unnormalised, between the chunks of a row of more than 64 edges.  GATv2 and dot-product attention below differ
// only in how a chunk's scores come about and in which table is summed: the three are one kernel, attention_aggregate_kernel, over a
// score policy, and the softmax step, the weighted sum and the two ends of a row are the functions that follow.
constexpr int kGatMaxHeads = 16;
constexpr float kNegInf = -__builtin_inff();

// GAT's and RelGAT's score from z = el + er: the slope product is one rounded product in the forward and in the backward alike, never
// contracted into the subtraction that follows it (e - m, e - lse), so the backward's e_j is the forward's bit for bit (dot_score below
// is the same rule for the dot-product score).
__device__ __forceinline__ float leaky_score(float z, float slope) {
#pragma clang fp contract(off)
    return z > 0.0f ? z : z * slope;
}

// acc[h] += the sum of x over the lanes of head h, for the 64 floats c0 + lane of a [H * dim] row (a head's floats are contiguous):
// a segmented inclusive scan, then the last lane of each head's segment adds its total.  Every lane must call it.
__device__ __forceinline__ void head_segment_add(float* acc, float x, int lane, int c0, int dim, int hd) {
    const int c = c0 + lane;
    const int h = c < hd ? c / dim : 0;
    const int start = c < hd ? max(h * dim - c0, 0) : hd - c0; // first lane of this lane's segment in the pass
    for (int o = 1; o < 64; o <<= 1) {
        const float y = __shfl_up(x, o);
        if (lane - o >= start) x += y;
    }
    if (c < hd && (lane == 63 || c + 1 == hd || (c + 1) % dim == 0)) acc[h] += x;
}

// A wave's LDS in the attention forward kernels.
struct SoftmaxLds {
    float* w;     // [64][kGatMaxHeads], [edge][head]: exp(e_j - m) of the chunk
    float* m_run; // per head: the running max,
    float* l_run; // the running sum,
    float* scl;   // and the chunk's rescale factor
};

__device__ __forceinline__ SoftmaxLds softmax_lds(float* w, float* st) { return {w, st, st + kGatMaxHeads, st + 2 * kGatMaxHeads}; }

__device__ __forceinline__ void softmax_row_begin(const SoftmaxLds& s, int lane, int heads) {
    wave_lds_sync(); // the previous row has read m_run / l_run
    if (lane < heads) {
        s.m_run[lane] = kNegInf;
        s.l_run[lane] = 0.0f;
    }
}

// One head's step of the online softmax over a chunk: lane j brings edge j's score e (-inf and !valid: no edge in this lane) and
// leaves p_j = exp(e_j - m) in w; lane 0 updates the head's running max and sum and stores the factor that rescales the earlier
// chunks' sum.  Every lane must call it.
__device__ __forceinline__ void softmax_chunk_step(const SoftmaxLds& s, int h, float e, bool valid, int lane) {
    const float mo = s.m_run[h];
    const float mn = fmaxf(mo, wave_max(e));
    const float p = valid ? expf(e - mn) : 0.0f;
    const float sum = wave_sum(p);
    const float sc = mo == mn ? 1.0f : (mo == kNegInf ? 0.0f : expf(mo - mn));
    s.w[lane * kGatMaxHeads + h] = p;
    if (lane == 0) {
        s.m_run[h] = mn;
        s.l_run[h] = s.l_run[h] * sc + sum;
        s.scl[h] = sc;
    }
}

// out_row[h, :] = (first chunk ? 0 : out_row[h, :] * scl[h]) + sum over the chunk's valid edges j of w[j][h] * feat[s_j, h, :], divided
// by the row's sum on the last chunk.  A lane per VEC floats of the [H * dim] row.  FINAL: w holds finished weights a_j (RelGAT's second
// pass): nothing to rescale and nothing to divide, and of s only w is read.
template <int VEC, bool FINAL>
__device__ __forceinline__ void softmax_accumulate(const SoftmaxLds& s, float* out_row, const float* __restrict__ feat, int32_t mine, int n,
                                                   bool first, bool last, int lane, int hd, int units, int upl) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    for (int u0 = 0; u0 < units; u0 += 64) { // wave-uniform trip counts: the shuffles below need every lane
        const int u = u0 + lane;
        const int hu = u < units ? u / upl : 0;
        float* o = out_row + (int64_t)u * VEC;
        vf acc = vf(0.0f);
        if (!first && u < units) acc = FINAL ? *reinterpret_cast<const vf*>(o) : *reinterpret_cast<const vf*>(o) * s.scl[hu];
        for (int j = 0; j < n; ++j) {
            const int32_t src = __shfl(mine, j);
            if (src >= 0 && u < units) acc += s.w[j * kGatMaxHeads + hu] * *reinterpret_cast<const vf*>(feat + (int64_t)src * hd + (int64_t)u * VEC);
        }
        if (u < units) {
            if (!FINAL && last) acc *= s.l_run[hu] > 0.0f ? 1.0f / s.l_run[hu] : 0.0f;
            *reinterpret_cast<vf*>(o) = acc;
        }
    }
}

// A row's end: zeros when no chunk ran (an empty CSR row), and the log-sum-exp per head, which is all the backward keeps.
template <int VEC>
__device__ __forceinline__ void softmax_row_end(const SoftmaxLds& s, float* out_row, float* lse_row, bool empty, int lane, int heads, int units) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    if (empty)
        for (int u = lane; u < units; u += 64) *reinterpret_cast<vf*>(out_row + (int64_t)u * VEC) = vf(0.0f);
    wave_lds_sync();
    if (lane < heads) lse_row[lane] = s.l_run[lane] > 0.0f ? s.m_run[lane] + logf(s.l_run[lane]) : kNegInf;
}

// gout[h] += <g[h, :], o[h, :]> for the heads of one [H * dim] row, in head_segment_add's fixed order (the backward kernels' pre-pass
// over grad_out[d] and out[d]).  Every lane must call it.
__device__ __forceinline__ void head_dots(float* gout, const float* __restrict__ g, const float* __restrict__ o, int lane, int dim, int hd) {
    for (int c0 = 0; c0 < hd; c0 += 64) { // wave-uniform trip count
        const int c = c0 + lane;
        head_segment_add(gout, c < hd ? g[c] * o[c] : 0.0f, lane, c0, dim, hd);
    }
}

// GATv2 attention on a block (DGL GATv2Conv's message step; the projections fc_src / fc_dst stay in torch).  For dst d, head h and the
// valid in-edges j of d (source s_j):
//   z_jc = feat_src[s_j, h, c] + feat_dst[d, h, c],  e_j = sum_c attn[h, c] leaky_relu(z_jc, slope),  a_j = softmax of e over the row,
//   out[d, h, :] = sum_j a_j feat_src[s_j, h, :]
// The score does not split into a per-source and a per-destination scalar as GAT's does: it is a dot product over the [H * D] row per
// edge.  GAT's mapping and its online softmax, with one step in front of every chunk, the score pass: a lane per
// float of the row, 64 floats at a time, attn and feat_dst[d] of the pass in registers, the chunk's edges in the inner loop, and the
// per-head sums added into the LDS [edge][head] array by head_segment_add in a fixed order.  The weighted sum then reads the chunk's
// source rows a second time (at most 64 rows: from the cache), so the HBM bytes are GAT's plus feat_dst, and nothing of size E is
// written.
// e[j * kGatMaxHeads + h] += edge j's score of head h, for the n edges of a chunk; with DOT also dot[..] += <g[h, :], feat_src[s_j, h, :]>.
template <bool DOT>
__device__ __forceinline__ void gatv2_score_pass(float* e, float* dot, int32_t mine, int n, const float* __restrict__ feat_src,
                                                 const float* __restrict__ fd, const float* __restrict__ attn, const float* __restrict__ g,
                                                 int lane, int hd, int dim, float slope) {
    for (int c0 = 0; c0 < hd; c0 += 64) { // wave-uniform trip count: head_segment_add shuffles across every lane
        const int c = c0 + lane;
        const bool in = c < hd;
        const float a = in ? attn[c] : 0.0f;
        const float b = in ? fd[c] : 0.0f;
        const float gc = DOT && in ? g[c] : 0.0f;
        for (int j = 0; j < n; ++j) {
            const int32_t s = __shfl(mine, j);
            if (s < 0) continue; // wave-uniform
            const float f = in ? feat_src[(int64_t)s * hd + c] : 0.0f;
            const float z = f + b;
            head_segment_add(e + j * kGatMaxHeads, in ? a * (z > 0.0f ? z : z * slope) : 0.0f, lane, c0, dim, hd);
            if (DOT) head_segment_add(dot + j * kGatMaxHeads, gc * f, lane, c0, dim, hd);
        }
    }
}

// Scaled dot-product attention on a block (the message step of DGL's DotGatConv and HGTConv, PyG's TransformerConv without edge
// features; the projections stay in torch).  Every slot carries the row of k / v its edge reads (row, -1 = no edge; the block's own
// index array in the dense form).  For dst d, head h and the slots j of d with row_j >= 0:
//   e_j = scale <q[d, h, :], k[row_j, h, :]>,  a_j = softmax of e over the row,  out[d, h, :] = sum_j a_j v[row_j, h, :]
// GATv2's layout with another score pass: a lane per float of the [H * D] row, 64 floats at a time, q[d] of the pass in
// registers, the chunk's edges in the inner loop, the per-head sums added into the LDS [edge][head] array by head_segment_add in a
// fixed order; the scale is applied to the finished sum by dot_score, in both directions.  The weighted sum then reads the chunk's v rows.
// Nothing of size E is written.
//
// A slot's score from its finished dot product: one rounded product, never contracted into the subtraction that follows it (e - m in
// the forward, e - lse in the backward).  Fused, the backward's fma(scale, qk, -lse) would take the product unrounded while the
// forward's maximum and lse are made of rounded scores: a_j = exp(e_j - lse) is then off by u |e_j|, edge by edge, the a_j of a row no
// longer sum to what lse says, and sum_j t_j, zero in exact arithmetic, grows with the scores' common offset.
__device__ __forceinline__ float dot_score(float scale, float qk) {
#pragma clang fp contract(off)
    return scale * qk;
}

// e[j * kGatMaxHeads + h] += <q[d, h, :], k[row_j, h, :]> for the n slots of a chunk; with DOT also dot[..] += <g[h, :], v[row_j, h, :]>.
template <bool DOT>
__device__ __forceinline__ void dot_score_pass(float* e, float* dot, int32_t mine, int n, const float* __restrict__ k,
                                               const float* __restrict__ qd, const float* __restrict__ v, const float* __restrict__ g, int lane,
                                               int hd, int dim) {
    for (int c0 = 0; c0 < hd; c0 += 64) { // wave-uniform trip count: head_segment_add shuffles across every lane
        const int c = c0 + lane;
        const bool in = c < hd;
        const float qc = in ? qd[c] : 0.0f;
        const float gc = DOT && in ? g[c] : 0.0f;
        for (int j = 0; j < n; ++j) {
            const int32_t s = __shfl(mine, j);
            if (s < 0) continue; // wave-uniform
            head_segment_add(e + j * kGatMaxHeads, in ? qc * k[(int64_t)s * hd + c] : 0.0f, lane, c0, dim, hd);
            if (DOT) head_segment_add(dot + j * kGatMaxHeads, in ? gc * v[(int64_t)s * hd + c] : 0.0f, lane, c0, dim, hd);
        }
    }
}

// What tells GAT, GATv2 and dot-product attention apart, in the forward kernel and in the row front of their backward kernels: how a
// slot's score comes about, and which table holds the rows that are summed.  The kernels take an op's three tables as (a, b, c) and
// its one float as `param`.  A policy with kRowPass makes a chunk's scores by a pass over the [H * dim] rows into the LDS [edge][head]
// array (row_pass; with DOT also the dots <g, value row>), and score(e, lane, h, param) finishes lane j's own word e[lane][h]; one without
// makes the score from scalars, score(a, b, mine, d, heads, h, param).  Either way score() is where the rounding rule of leaky_score / dot_score is applied, forward and backward.
struct GatScore { // a = el, b = er, c = feat, param = slope
    static constexpr bool kRowPass = false;
    static __host__ __device__ const float* values(const float*, const float*, const float* feat) { return feat; }
    static __device__ __forceinline__ float score(const float* __restrict__ el, const float* __restrict__ er, int32_t mine, int64_t d, int heads, int h,
                                                  float slope) {
        return leaky_score(el[(int64_t)mine * heads + h] + er[d * heads + h], slope);
    }
};

struct Gatv2Score { // a = feat_src, b = feat_dst, c = attn, param = slope
    static constexpr bool kRowPass = true;
    static __host__ __device__ const float* values(const float* feat_src, const float*, const float*) { return feat_src; }
    template <bool DOT>
    static __device__ __forceinline__ void row_pass(float* e, float* dot, int32_t mine, int n, const float* __restrict__ feat_src,
                                                    const float* __restrict__ feat_dst, const float* __restrict__ attn, int64_t d,
                                                    const float* __restrict__ g, int lane, int hd, int dim, float slope) {
        gatv2_score_pass<DOT>(e, dot, mine, n, feat_src, feat_dst + d * hd, attn, g, lane, hd, dim, slope);
    }
    static __device__ __forceinline__ float score(const float* e, int lane, int h, float) {
        return e[lane * kGatMaxHeads + h]; // the finished sum
    }
};

struct DotScore { // a = q, b = k, c = v, param = scale
    static constexpr bool kRowPass = true;
    static __host__ __device__ const float* values(const float*, const float*, const float* v) { return v; }
    template <bool DOT>
    static __device__ __forceinline__ void row_pass(float* e, float* dot, int32_t mine, int n, const float* __restrict__ q,
                                                    const float* __restrict__ k, const float* __restrict__ v, int64_t d,
                                                    const float* __restrict__ g, int lane, int hd, int dim, float) {
        dot_score_pass<DOT>(e, dot, mine, n, k, q + d * hd, v, g, lane, hd, dim);
    }
    static __device__ __forceinline__ float score(const float* e, int lane, int h, float scale) {
        return dot_score(scale, e[lane * kGatMaxHeads + h]);
    }
};

// A chunk's row pass: lane j zeroes edge j's words of w (with DOT of dot too), then Score's pass adds into them.  The caller has
// synchronised: the previous chunk's readers of w / dot are done.
template <typename Score, bool DOT>
__device__ __forceinline__ void score_pass_chunk(float* w, float* dot, int32_t mine, int n, const float* __restrict__ a,
                                                 const float* __restrict__ b, const float* __restrict__ c, int64_t d,
                                                 const float* __restrict__ g, int lane, int heads, int hd, int dim, float param) {
    for (int h = 0; h < heads; ++h) {
        w[lane * kGatMaxHeads + h] = 0.0f;
        if (DOT) dot[lane * kGatMaxHeads + h] = 0.0f;
    }
    wave_lds_sync();
    Score::template row_pass<DOT>(w, dot, mine, n, a, b, c, d, g, lane, hd, dim, param);
    wave_lds_sync();
}

// The forward kernel of the three ops: out[d, h, :] = sum_j a_j values[s_j, h, :], a_j the softmax over row d of Score's e_j, and
// lse[d, h].  Without a row pass the score is a scalar per edge and head and goes straight into the softmax step; with one, w holds the
// chunk's scores first, and lane j reads and rewrites only edge j's words.
template <typename Score, int VEC, bool CSR>
__global__ __launch_bounds__(kBlock) void attention_aggregate_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, int fanout,
                                                                     const float* __restrict__ a, const float* __restrict__ b,
                                                                     const float* __restrict__ c, float* __restrict__ out,
                                                                     float* __restrict__ lse, int64_t n_dst, int heads, int dim, float param) {
    __shared__ float w_lds[kWavesPerBlock][64 * kGatMaxHeads];
    __shared__ float st_lds[kWavesPerBlock][3 * kGatMaxHeads];
    const auto [lane, wave, n_waves] = wave_rows();
    const SoftmaxLds s = softmax_lds(w_lds[threadIdx.x >> 6], st_lds[threadIdx.x >> 6]);
    const int hd = heads * dim, units = hd / VEC, upl = dim / VEC;
    for (int64_t d = wave; d < n_dst; d += n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        softmax_row_begin(s, lane, heads);
        for (int64_t e0 = beg; e0 < end; e0 += 64) { // wave-uniform trip counts: the shuffles below need every lane
            int32_t mine;
            const int n = load_chunk(idx, e0, end, lane, &mine);
            wave_lds_sync(); // the previous chunk has read w and scl; m_run / l_run are set
            if constexpr (Score::kRowPass) score_pass_chunk<Score, false>(s.w, nullptr, mine, n, a, b, c, d, nullptr, lane, heads, hd, dim, param);
            for (int h = 0; h < heads; ++h) {
                float e = kNegInf;
                if (mine >= 0) {
                    if constexpr (Score::kRowPass) e = Score::score(s.w, lane, h, param);
                    else e = Score::score(a, b, mine, d, heads, h, param);
                }
                softmax_chunk_step(s, h, e, mine >= 0, lane);
            }
            wave_lds_sync();
            softmax_accumulate<VEC, false>(s, out + d * hd, Score::values(a, b, c), mine, n, e0 == beg, e0 + 64 >= end, lane, hd, units, upl);
        }
        softmax_row_end<VEC>(s, out + d * hd, lse + d * heads, beg == end, lane, heads, units);
    }
}

// The backward kernels of the four attention ops recompute a weight as exp(e_j - lse) from the saved fp32 log-sum-exp.  Those sum over a
// softmax group to S = 1 + O(u |lse|), not to 1: lse is rounded at the scores' common offset.  Every backward therefore divides by the
// group's own S, summed in a fixed order (a wave_sum per 64-slot chunk, chunk after chunk), so that the weights sum to 1 within a few u
// whatever the offset, grad_feat / grad_v / grad_src add up over the table to grad_out, and an error of lse itself cancels.  A row of
// one chunk -- every fixed row -- takes S from the chunk already in registers; a longer row walks its scores once more in front.
__device__ __forceinline__ float normalised(float a, float sum) { return sum > 0.0f ? a / sum : 0.0f; }

// A row's front in the backward kernels of GAT and dot-product attention: gout[h] = <g[h, :], out[d, h, :]> (head_dots), and for a
// row of several chunks ssum[h] = S from a walk over its scores -- with a row pass of its own where Score has one, through w -- chunk
// after chunk, lane 0 alone touching ssum.  -> whether the row is one chunk (wave-uniform); its S is then the wave_sum of the a_j.
// The GATv2 backward has the same steps written out: moved in here, its RP = 8 CSR instantiation takes one VGPR more.
template <typename Score>
__device__ __forceinline__ bool backward_row_front(float* w, float* gout, float* ssum, const int32_t* __restrict__ idx, int64_t beg, int64_t end,
                                                   const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                   const float* __restrict__ out_row, const float* __restrict__ lse_row,
                                                   const float* __restrict__ g, int64_t d, int lane, int heads, int hd, int dim, float param) {
    wave_lds_sync(); // the previous row has read gout
    if (lane < heads) gout[lane] = ssum[lane] = 0.0f;
    wave_lds_sync();
    head_dots(gout, g, out_row, lane, dim, hd);
    const bool one = end - beg <= 64;
    if (!one) {
        for (int64_t e0 = beg; e0 < end; e0 += 64) {
            int32_t mine;
            const int n = load_chunk(idx, e0, end, lane, &mine);
            if constexpr (Score::kRowPass) {
                wave_lds_sync(); // the previous chunk has read w
                score_pass_chunk<Score, false>(w, nullptr, mine, n, a, b, c, d, nullptr, lane, heads, hd, dim, param);
            }
            for (int h = 0; h < heads; ++h) {
                float p = 0.0f;
                if (mine >= 0) {
                    if constexpr (Score::kRowPass) p = expf(Score::score(w, lane, h, param) - lse_row[h]);
                    else p = expf(Score::score(a, b, mine, d, heads, h, param) - lse_row[h]);
                }
                const float sum = wave_sum(p);
                if (lane == 0) ssum[h] += sum;
            }
        }
        wave_lds_sync();
    }
    return one;
}

// dot[j][h] += <g[h, :], feat[s_j, h, :]> for the n slots of a chunk whose weights a_j are in w: a lane per float of the [H * dim] row, 64
// at a time, the per-head sums by head_segment_add in a fixed order; with ADD also grad_feat[s_j, h, :] += a_j g[h, :] from the same
// lanes (GAT's and RelGAT's backward).
template <bool ADD>
__device__ __forceinline__ void dot_grad_feat_walk(const float* w, float* dot, int32_t mine, int n, const float* __restrict__ feat,
                                                   const float* __restrict__ g, float* __restrict__ grad_feat, int lane, int dim, int hd) {
    for (int c0 = 0; c0 < hd; c0 += 64) { // wave-uniform trip count: head_segment_add shuffles across every lane
        const int c = c0 + lane;
        const int hc = c < hd ? c / dim : 0;
        const float gc = c < hd ? g[c] : 0.0f;
        for (int j = 0; j < n; ++j) {
            const int32_t s = __shfl(mine, j);
            if (s < 0) continue; // wave-uniform
            float x = 0.0f;
            if (c < hd) {
                x = gc * feat[(int64_t)s * hd + c];
                if (ADD) unsafeAtomicAdd(grad_feat + (int64_t)s * hd + c, w[j * kGatMaxHeads + hc] * gc);
            }
            head_segment_add(dot + j * kGatMaxHeads, x, lane, c0, dim, hd);
        }
    }
}

// GAT backward, a_j = exp(e_j - lse[d, h]) / S recomputed from the saved log-sum-exp, S the row's sum of exp(e_j - lse[d, h]):
//   grad_feat[s_j, h, :] += a_j g[d, h, :],  t_j = a_j (<g[d, h, :], feat[s_j, h, :]> - <g[d, h, :], out[d, h, :]>) (z_j > 0 ? 1 : slope),
//   grad_el[s_j, h] += t_j,  grad_er[d, h] = sum_j t_j.
// A lane per float of the [H * dim] row, 64 at a time; the per-head dot products are summed by head_segment_add into LDS in a fixed
// order.  grad_feat and grad_el take hardware float atomics (zeroed by the caller); grad_er is written whole, one tree per chunk.
template <bool CSR>
__global__ __launch_bounds__(kBlock) void gat_aggregate_backward_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                                        int fanout, const float* __restrict__ el, const float* __restrict__ er,
                                                                        const float* __restrict__ feat, const float* __restrict__ out,
                                                                        const float* __restrict__ lse, const float* __restrict__ grad_out,
                                                                        float* __restrict__ grad_feat, float* __restrict__ grad_el,
                                                                        float* __restrict__ grad_er, int64_t n_dst, int heads, int dim, float slope) {
    __shared__ float w_lds[kWavesPerBlock][64 * kGatMaxHeads];   // a_j of the chunk, [edge][head]
    __shared__ float dot_lds[kWavesPerBlock][64 * kGatMaxHeads]; // <g, feat_j>, [edge][head]
    __shared__ float hs_lds[kWavesPerBlock][3 * kGatMaxHeads];   // per head: <g, out>, the sum of t_j so far, S of a row of several chunks
    const auto [lane, wave, n_waves] = wave_rows();
    float* w = w_lds[threadIdx.x >> 6];
    float* dot = dot_lds[threadIdx.x >> 6];
    float* gout = hs_lds[threadIdx.x >> 6];
    float* ter = gout + kGatMaxHeads;
    float* ssum = ter + kGatMaxHeads;
    const int hd = heads * dim;
    for (int64_t d = wave; d < n_dst; d += n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        const float* g = grad_out + d * hd;
        const bool one = backward_row_front<GatScore>(w, gout, ssum, idx, beg, end, el, er, feat, out + d * hd, lse + d * heads, g, d, lane, heads,
                                                      hd, dim, slope);
        if (lane < heads) ter[lane] = 0.0f; // the previous row's reader is past the front's syncs
        for (int64_t e0 = beg; e0 < end; e0 += 64) { // wave-uniform trip counts
            int32_t mine;
            const int n = load_chunk(idx, e0, end, lane, &mine);
            wave_lds_sync(); // the previous chunk has read w and dot
            for (int h = 0; h < heads; ++h) {
                float a = 0.0f;
                if (mine >= 0) a = expf(GatScore::score(el, er, mine, d, heads, h, slope) - lse[d * heads + h]);
                w[lane * kGatMaxHeads + h] = normalised(a, one ? wave_sum(a) : ssum[h]);
                dot[lane * kGatMaxHeads + h] = 0.0f;
            }
            wave_lds_sync();
            dot_grad_feat_walk<true>(w, dot, mine, n, feat, g, grad_feat, lane, dim, hd);
            wave_lds_sync();
            for (int h = 0; h < heads; ++h) {
                float t = 0.0f;
                if (mine >= 0) {
                    const float z = el[(int64_t)mine * heads + h] + er[d * heads + h];
                    t = w[lane * kGatMaxHeads + h] * (dot[lane * kGatMaxHeads + h] - gout[h]) * (z > 0.0f ? 1.0f : slope);
                    unsafeAtomicAdd(grad_el + (int64_t)mine * heads + h, t);
                }
                const float ts = wave_sum(t);
                if (lane == 0) ter[h] += ts;
            }
        }
        wave_lds_sync();
        if (lane < heads) grad_er[d * heads + lane] = ter[lane];
    }
}

// GATv2 backward, all three gradients in one launch, each of them optional (null).  a_j = exp(e_j - lse[d, h]) / S (`normalised` above) with e_j
// recomputed by a second score pass, which also sums dot_j = <g[d, h, :], feat_src[s_j, h, :]>; then per edge and head
// t_j = a_j (dot_j - <g, out>), and a third walk over the chunk's rows, a lane per float c, with k_jc = z_jc > 0 ? 1 : slope:
//   grad_src[s_j, c] += a_j g[d, c] + t_j attn[c] k_jc   hardware float atomics (zeroed by the caller), 256 contiguous bytes per wave
//                                                        instruction: the only atomics;
//   grad_dst[d, c]    = sum_j t_j attn[c] k_jc           summed in slot order in a register, stored once per chunk (a later chunk of a
//                                                        long row adds to what the earlier ones stored);
//   grad_attn[c]      = sum_d sum_j t_j leaky_relu(z_jc)  no atomics: lane c keeps the sum over its wave's rows, the waves of a block add
//                                                        theirs through LDS in wave order, and block b stores row b of the caller's
//                                                        partials [gridDim.x, H * D]; the caller sums the rows.  The same grid gives
//                                                        the same bits.
// RP > 0: the row is at most RP 64-float passes long and the grad_attn sums are RP registers.  RP == 0: any row length; a block is then
// one wave (the host launches 64 threads) and adds each pass's sum into its own partials row, the same lane at the same address.
template <int RP, bool CSR>
__global__ __launch_bounds__(kBlock) void gatv2_aggregate_backward_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                                          int fanout, const float* __restrict__ feat_src,
                                                                          const float* __restrict__ feat_dst, const float* __restrict__ attn,
                                                                          const float* __restrict__ out, const float* __restrict__ lse,
                                                                          const float* __restrict__ grad_out, float* __restrict__ grad_src,
                                                                          float* __restrict__ grad_dst, float* __restrict__ grad_attn_parts,
                                                                          int64_t n_dst, int heads, int dim, float slope) {
    __shared__ float w_lds[kWavesPerBlock][64 * kGatMaxHeads];   // the chunk's scores e_j, then a_j, [edge][head]
    __shared__ float dot_lds[kWavesPerBlock][64 * kGatMaxHeads]; // <g, feat_src_j>, then t_j, [edge][head]
    __shared__ float hs_lds[kWavesPerBlock][2 * kGatMaxHeads];   // per head: <g, out>, S of a row of several chunks
    static_assert(RP * 64 <= 64 * kGatMaxHeads, "the waves' grad_attn sums are combined through w_lds");
    const int wv = threadIdx.x >> 6, wpb = blockDim.x >> 6; // one wave a block at RP == 0
    const WaveRows wr = wave_rows(wpb);
    const int lane = wr.lane; // a lambda below captures it
    float* w = w_lds[wv];
    float* dot = dot_lds[wv];
    float* gout = hs_lds[wv];
    float* ssum = gout + kGatMaxHeads;
    const int hd = heads * dim;
    float* prow = grad_attn_parts ? grad_attn_parts + (int64_t)blockIdx.x * hd : nullptr;
    float ga_reg[RP > 0 ? RP : 1];
    for (int p = 0; p < (RP > 0 ? RP : 1); ++p) ga_reg[p] = 0.0f;
    if (RP == 0 && prow)
        for (int c = lane; c < hd; c += 64) prow[c] = 0.0f;
    for (int64_t d = wr.wave; d < n_dst; d += wr.n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        const float* g = grad_out + d * hd;
        const float* fd = feat_dst + d * hd;
        wave_lds_sync(); // the previous row has read gout
        if (lane < heads) gout[lane] = ssum[lane] = 0.0f;
        wave_lds_sync();
        head_dots(gout, g, out + d * hd, lane, dim, hd);
        const bool one = end - beg <= 64; // wave-uniform: the row is one chunk
        if (!one) {                       // S per head from a score pass of its own, chunk after chunk (lane 0 alone touches ssum)
            for (int64_t e0 = beg; e0 < end; e0 += 64) {
                int32_t mine;
                const int n = load_chunk(idx, e0, end, lane, &mine);
                wave_lds_sync(); // the previous chunk has read w
                for (int h = 0; h < heads; ++h) w[lane * kGatMaxHeads + h] = 0.0f;
                wave_lds_sync();
                gatv2_score_pass<false>(w, nullptr, mine, n, feat_src, fd, attn, nullptr, lane, hd, dim, slope);
                wave_lds_sync();
                for (int h = 0; h < heads; ++h) {
                    const float sum = wave_sum(mine >= 0 ? expf(w[lane * kGatMaxHeads + h] - lse[d * heads + h]) : 0.0f);
                    if (lane == 0) ssum[h] += sum;
                }
            }
            wave_lds_sync();
        }
        for (int64_t e0 = beg; e0 < end; e0 += 64) { // wave-uniform trip counts
            int32_t mine;
            const int n = load_chunk(idx, e0, end, lane, &mine);
            const bool first = e0 == beg;
            wave_lds_sync(); // the previous chunk has read w and dot
            for (int h = 0; h < heads; ++h) {
                w[lane * kGatMaxHeads + h] = 0.0f;
                dot[lane * kGatMaxHeads + h] = 0.0f;
            }
            wave_lds_sync();
            gatv2_score_pass<true>(w, dot, mine, n, feat_src, fd, attn, g, lane, hd, dim, slope);
            wave_lds_sync();
            for (int h = 0; h < heads; ++h) { // lane j reads and rewrites only edge j's words
                float a = 0.0f, t = 0.0f;
                if (mine >= 0) a = expf(w[lane * kGatMaxHeads + h] - lse[d * heads + h]);
                a = normalised(a, one ? wave_sum(a) : ssum[h]);
                if (mine >= 0) t = a * (dot[lane * kGatMaxHeads + h] - gout[h]);
                w[lane * kGatMaxHeads + h] = a;
                dot[lane * kGatMaxHeads + h] = t;
            }
            wave_lds_sync();
            auto pass = [&](int c0, float& ga_sum) {
                const int c = c0 + lane;
                const bool in = c < hd;
                const int hc = in ? c / dim : 0;
                const float at = in ? attn[c] : 0.0f;
                const float b = in ? fd[c] : 0.0f;
                const float gc = in ? g[c] : 0.0f;
                float gd = 0.0f, ga = 0.0f;
                for (int j = 0; j < n; ++j) {
                    const int32_t s = __shfl(mine, j);
                    if (s >= 0 && in) { // every lane takes the shuffle above
                        const float z = feat_src[(int64_t)s * hd + c] + b;
                        const float tj = dot[j * kGatMaxHeads + hc];
                        const float u = tj * at * (z > 0.0f ? 1.0f : slope);
                        if (grad_src) unsafeAtomicAdd(grad_src + (int64_t)s * hd + c, w[j * kGatMaxHeads + hc] * gc + u);
                        gd += u;
                        ga += tj * (z > 0.0f ? z : z * slope);
                    }
                }
                if (in && grad_dst) grad_dst[d * hd + c] = first ? gd : grad_dst[d * hd + c] + gd;
                ga_sum += ga;
            };
            if constexpr (RP > 0) {
#pragma unroll
                for (int p = 0; p < RP; ++p)
                    if (p * 64 < hd) pass(p * 64, ga_reg[p]);
            } else {
                for (int c0 = 0; c0 < hd; c0 += 64) {
                    float ga = 0.0f;
                    pass(c0, ga);
                    if (prow && c0 + lane < hd) prow[c0 + lane] += ga;
                }
            }
        }
        if (beg == end && grad_dst) // no chunk ran: an empty CSR row
            for (int c = lane; c < hd; c += 64) grad_dst[d * hd + c] = 0.0f;
    }
    if constexpr (RP > 0) {
        if (!prow) return; // block-uniform
        __syncthreads(); // every wave of the block is past its rows: w_lds is free
#pragma unroll
        for (int p = 0; p < RP; ++p) w[p * 64 + lane] = ga_reg[p];
        __syncthreads();
        for (int c = threadIdx.x; c < hd; c += kBlock) {
            float sum = w_lds[0][c];
            for (int k = 1; k < kWavesPerBlock; ++k) sum += w_lds[k][c];
            prow[c] = sum;
        }
    }
}

// Dot-product backward, all three gradients in one launch, each of them optional (null).  A second score pass gives the dot products again and
// dot_j = <g[d, h, :], v[row_j, h, :]>; then per edge and head a_j = exp(e_j - lse[d, h]) / S (`normalised` above), e_j the forward's bit for bit (dot_score), and
// t_j = a_j (dot_j - <g, out>), and a third walk over the chunk's rows, a lane per float c:
//   grad_v[row_j, c] += a_j g[d, c]             hardware float atomics (zeroed by the caller), 256 contiguous bytes per wave instruction;
//   grad_k[row_j, c] += scale t_j q[d, c]       the same;
//   grad_q[d, c]      = scale sum_j t_j k[row_j, c]   summed in slot order in a register, scaled and stored once per chunk (a later
//                                               chunk of a long row adds to what the earlier ones stored): no atomics.
template <bool CSR>
__global__ __launch_bounds__(kBlock) void dot_gat_aggregate_backward_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ row,
                                                                            int fanout, const float* __restrict__ q, const float* __restrict__ k,
                                                                            const float* __restrict__ v, const float* __restrict__ out,
                                                                            const float* __restrict__ lse, const float* __restrict__ grad_out,
                                                                            float* __restrict__ grad_q, float* __restrict__ grad_k,
                                                                            float* __restrict__ grad_v, int64_t n_dst, int heads, int dim,
                                                                            float scale) {
    __shared__ float w_lds[kWavesPerBlock][64 * kGatMaxHeads];   // the chunk's dot products <q, k_j>, then a_j, [edge][head]
    __shared__ float dot_lds[kWavesPerBlock][64 * kGatMaxHeads]; // <g, v_j>, then t_j, [edge][head]
    __shared__ float hs_lds[kWavesPerBlock][2 * kGatMaxHeads];   // per head: <g, out>, S of a row of several chunks
    const auto [lane, wave, n_waves] = wave_rows();
    float* w = w_lds[threadIdx.x >> 6];
    float* dot = dot_lds[threadIdx.x >> 6];
    float* gout = hs_lds[threadIdx.x >> 6];
    float* ssum = gout + kGatMaxHeads;
    const int hd = heads * dim;
    for (int64_t d = wave; d < n_dst; d += n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        const float* g = grad_out + d * hd;
        const float* qd = q + d * hd;
        const bool one = backward_row_front<DotScore>(w, gout, ssum, row, beg, end, q, k, v, out + d * hd, lse + d * heads, g, d, lane, heads, hd, dim,
                                                      scale);
        for (int64_t e0 = beg; e0 < end; e0 += 64) { // wave-uniform trip counts
            int32_t mine;
            const int n = load_chunk(row, e0, end, lane, &mine);
            wave_lds_sync(); // the previous chunk has read w and dot
            score_pass_chunk<DotScore, true>(w, dot, mine, n, q, k, v, d, g, lane, heads, hd, dim, scale);
            for (int h = 0; h < heads; ++h) { // lane j reads and rewrites only edge j's words
                float a = 0.0f, t = 0.0f;
                if (mine >= 0) a = expf(dot_score(scale, w[lane * kGatMaxHeads + h]) - lse[d * heads + h]);
                a = normalised(a, one ? wave_sum(a) : ssum[h]);
                if (mine >= 0) t = a * (dot[lane * kGatMaxHeads + h] - gout[h]);
                w[lane * kGatMaxHeads + h] = a;
                dot[lane * kGatMaxHeads + h] = t;
            }
            wave_lds_sync();
            for (int c0 = 0; c0 < hd; c0 += 64) { // wave-uniform trip count: the shuffles below need every lane
                const int c = c0 + lane;
                const bool in = c < hd;
                const int hc = in ? c / dim : 0;
                const float gc = in ? g[c] : 0.0f;
                const float qc = in ? qd[c] : 0.0f;
                float gq = 0.0f;
                for (int j = 0; j < n; ++j) {
                    const int32_t s = __shfl(mine, j);
                    if (s >= 0 && in) { // every lane takes the shuffle above
                        const float tj = dot[j * kGatMaxHeads + hc];
                        if (grad_v) unsafeAtomicAdd(grad_v + (int64_t)s * hd + c, w[j * kGatMaxHeads + hc] * gc);
                        if (grad_k) unsafeAtomicAdd(grad_k + (int64_t)s * hd + c, scale * tj * qc);
                        if (grad_q) gq = __builtin_fmaf(tj, k[(int64_t)s * hd + c], gq);
                    }
                }
                if (in && grad_q) grad_q[d * hd + c] = e0 == beg ? scale * gq : grad_q[d * hd + c] + scale * gq;
            }
        }
        if (beg == end && grad_q) // no chunk ran: an empty CSR row
            for (int c = lane; c < hd; c += 64) grad_q[d * hd + c] = 0.0f;
    }
}

// Weighted sum aggregation (DGL's u_mul_e_sum, what GraphConv / SAGEConv compute with edge_weight=): out[d] = sum over the valid edges
// j of row d of w_j * h_src[s_j], one weight per neighbour slot (w is laid out like the block's index array).  The mean kernel's
// mapping: one wave per destination row, a lane per 16 bytes of the row, the row's indices and weights read 64 at a time (a fixed row
// of fan-out <= 32 is one chunk) and broadcast by shuffle; the sum runs in slot order with one fma per term.  A byte mover like the
// mean: per row it reads deg * (dim * 4 + 8) bytes and writes dim * 4.  The fixed and the CSR kernels are the same code on the same
// lanes, so a row both forms can express gives the same bits.
template <int VEC, bool CSR>
__global__ __launch_bounds__(kBlock) void weighted_sum_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                              const float* __restrict__ w, int fanout, const float* __restrict__ h_src,
                                                              float* __restrict__ out, int64_t n_dst, int dim) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    const auto [lane, wave, n_waves] = wave_rows();
    const int units = dim / VEC;
    for (int64_t d = wave; d < n_dst; d += n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        for (int u0 = 0; u0 < units; u0 += 64) { // wave-uniform trip counts: the shuffles below need every lane
            const int u = u0 + lane;
            vf acc = vf(0.0f);
            for (int64_t e0 = beg; e0 < end; e0 += 64) {
                int32_t mine;
                const int n = load_chunk(idx, e0, end, lane, &mine);
                const float wm = e0 + lane < end ? w[e0 + lane] : 0.0f;
                for (int j = 0; j < n; ++j) {
                    const int32_t s = __shfl(mine, j);
                    const float wj = __shfl(wm, j);
                    if (s >= 0 && u < units) axpy<VEC>(acc, wj, *reinterpret_cast<const vf*>(h_src + (int64_t)s * dim + (int64_t)u * VEC));
                }
            }
            if (u < units) *reinterpret_cast<vf*>(out + d * dim + (int64_t)u * VEC) = acc;
        }
    }
}

// Both gradients of the weighted sum in one launch, either of them optional (null):
//   grad_src[s_j] += w_j * grad_out[d]          hardware float atomics into a buffer the caller zeroed: summation order varies;
//   grad_w[slot j] = <grad_out[d], h_src[s_j]>   each lane sums its 16-byte units of the row with fmas, a butterfly adds the 64 lanes
//                                               (a fixed order), and lane j of the chunk keeps edge j's value; 0 on a padding slot.
// One wave per row; per edge it reads the row of h_src (grad_w only) and adds into the row of grad_src; grad_out[d] stays in
// registers when the row is at most 64 units long and comes from the cache otherwise.  Measured: with a lane per 16 bytes an atomic
// instruction of the wave touches 64 floats 16 bytes apart, and the grad_src part runs at a quarter of the mean backward's rate
// (361 against 89 us on the 5,5 input block at dim 1024); giving the atomics the mean backward's lane-per-float mapping is the
// known next step (profiles/r08_edge_ids_weighted_sum.txt).
template <int VEC, bool CSR>
__global__ __launch_bounds__(kBlock) void weighted_sum_backward_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                                       const float* __restrict__ w, int fanout, const float* __restrict__ h_src,
                                                                       const float* __restrict__ grad_out, float* __restrict__ grad_src,
                                                                       float* __restrict__ grad_w, int64_t n_dst, int dim) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    const auto [lane, wave, n_waves] = wave_rows();
    const int units = dim / VEC;
    for (int64_t d = wave; d < n_dst; d += n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        const float* g = grad_out + d * dim;
        const vf g0 = lane < units ? *reinterpret_cast<const vf*>(g + (int64_t)lane * VEC) : vf(0.0f);
        for (int64_t e0 = beg; e0 < end; e0 += 64) { // wave-uniform trip counts
            const bool have = e0 + lane < end;
            int32_t mine;
            const int n = load_chunk(idx, e0, end, lane, &mine);
            const float wm = have ? w[e0 + lane] : 0.0f;
            float gw = 0.0f;
            for (int j = 0; j < n; ++j) {
                const int32_t s = __shfl(mine, j);
                if (s < 0) continue; // wave-uniform
                const float wj = __shfl(wm, j);
                float part = 0.0f;
                for (int u0 = 0; u0 < units; u0 += 64) {
                    const int u = u0 + lane;
                    if (u < units) {
                        const vf gv = u0 == 0 ? g0 : *reinterpret_cast<const vf*>(g + (int64_t)u * VEC);
                        const int64_t at = (int64_t)s * dim + (int64_t)u * VEC;
                        if (grad_src)
                            for (int i = 0; i < VEC; ++i) unsafeAtomicAdd(grad_src + at + i, wj * gv[i]);
                        if (grad_w) {
                            const vf hv = *reinterpret_cast<const vf*>(h_src + at);
                            for (int i = 0; i < VEC; ++i) part = __builtin_fmaf(gv[i], hv[i], part);
                        }
                    }
                }
                if (grad_w) { // wave-uniform
                    const float tot = wave_sum(part);
                    if (lane == j) gw = tot;
                }
            }
            if (grad_w && have) grad_w[e0 + lane] = gw;
        }
    }
}

// Max aggregation (DGL's fn.max reducer, what SAGEConv "pool" and GINConv "max" compute): out[d, c] = max over the valid edges j of row
// d of h_src[s_j, c], and arg[d, c] = the s_j of the winning edge (int32, the local source index), which is all the backward needs.
// The weighted sum's mapping: one wave per destination row, a lane per 16 bytes of the row, the row's indices read 64 at a time (a
// fixed row of fan-out <= 32 is one chunk) and broadcast by shuffle.  The rule, torch.max(dim)'s: the running maximum starts from the
// first valid slot, a later slot replaces it when v > best, or when v is NaN and best is not -- ties (+-0 included) keep the first slot
// in slot order, a NaN propagates with arg at the first NaN, a row of -inf gives -inf and a valid arg.  A row without a valid edge
// gives out = 0 and arg = -1 (DGL's max reducer at zero in-degree).  arg may be null (inference): nothing is stored for it.  A
// maximum rounds nothing, and the fixed and the CSR kernels are the same code on the same lanes: both forms give the same bits.
// A byte mover like the mean: per row it reads deg * (dim * 4 + 4) bytes and writes dim * 4 (dim * 8 with arg).
template <int VEC, bool CSR>
__global__ __launch_bounds__(kBlock) void max_aggregate_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, int fanout,
                                                               const float* __restrict__ h_src, float* __restrict__ out,
                                                               int32_t* __restrict__ arg, int64_t n_dst, int dim) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    typedef int32_t vi __attribute__((ext_vector_type(VEC)));
    const auto [lane, wave, n_waves] = wave_rows();
    const int units = dim / VEC;
    for (int64_t d = wave; d < n_dst; d += n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        for (int u0 = 0; u0 < units; u0 += 64) { // wave-uniform trip counts: the shuffles below need every lane
            const int u = u0 + lane;
            vf best = vf(0.0f);
            vi at = vi(-1);
            bool any = false; // wave-uniform: a valid slot has been seen
            for (int64_t e0 = beg; e0 < end; e0 += 64) {
                int32_t mine;
                const int n = load_chunk(idx, e0, end, lane, &mine);
                for (int j = 0; j < n; ++j) {
                    const int32_t s = __shfl(mine, j);
                    if (s < 0) continue; // wave-uniform
                    if (u < units) {
                        const vf v = *reinterpret_cast<const vf*>(h_src + (int64_t)s * dim + (int64_t)u * VEC);
                        for (int i = 0; i < VEC; ++i) { // selects, no branches: the lanes of a wave disagree element by element
                            const bool take = !any | (v[i] > best[i]) | ((v[i] != v[i]) & (best[i] == best[i]));
                            best[i] = take ? v[i] : best[i];
                            at[i] = take ? s : at[i];
                        }
                    }
                    any = true;
                }
            }
            if (u < units) {
                *reinterpret_cast<vf*>(out + d * dim + (int64_t)u * VEC) = best;
                if (arg) *reinterpret_cast<vi*>(arg + d * dim + (int64_t)u * VEC) = at;
            }
        }
    }
}

// grad_src[arg[d, c], c] += grad_out[d, c] wherever arg[d, c] >= 0 (grad_src zeroed by the caller; hardware float atomics: summation
// order varies).  One kernel for both block forms: it needs no neighbour list.  The mean backward's mapping, a lane per float: lane c
// reads arg[d, c] and grad_out[d, c] coalesced and issues one atomic, where the mean backward issues deg.  Per row it reads dim * 8
// bytes and adds dim * 4 through atomics.
__global__ __launch_bounds__(kBlock) void max_aggregate_backward_kernel(const int32_t* __restrict__ arg, const float* __restrict__ grad_out,
                                                                        float* __restrict__ grad_src, int64_t n_dst, int dim) {
    const auto [lane, wave, n_waves] = wave_rows();
    for (int64_t d = wave; d < n_dst; d += n_waves)
        for (int c = lane; c < dim; c += 64) {
            const int32_t s = arg[d * dim + c];
            if (s >= 0) unsafeAtomicAdd(grad_src + (int64_t)s * dim + c, grad_out[d * dim + c]);
        }
}

// Relation-typed sum (DGL RelGraphConv's message step, before its weights): out[d, r, :] = sum over the valid edges j of row d with
// etype_j == r of w_j * h_src[s_j, :], so that out.view(n_dst, R * dim) @ W.view(R * dim, out_dim) is sum_j w_j W[etype_j] h[s_j] in one
// GEMM.  etype is laid out like the block's index array, and so is w (null: every weight is 1).  The weighted sum's mapping and its
// arithmetic: one wave per destination row, a lane per 16 bytes, indices / types / weights read 64 at a time; a relation's sum runs in
// slot order with one fma per term from +0, so out[:, r, :] has the bits of weighted_sum_kernel with w * [etype == r] (a term of weight
// 0 leaves a finite fma accumulator as it is).  A wave cannot hold R * dim accumulators, so it walks r = 0 .. R-1: every lane ORs the
// types of its slots into a 64-bit mask (hence R <= 64) and a ballot tells whether r is in the row; an absent relation stores zeros, a
// present one takes the ballot of its edges in each chunk and visits only those, in ascending slot order.  A row of at most 64 slots
// keeps its (index, type, weight) words in registers; a longer one streams them again per present relation (12 bytes an edge).  Every
// h_src row is read once.  A valid slot whose type is outside [0, R) matches no r: it contributes nothing, and its type is only
// ever compared.  Per row of deg edges: reads deg * (4 dim + 12), writes 4 dim R.
template <int VEC, bool CSR>
__global__ __launch_bounds__(kBlock) void rel_sum_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                         const int32_t* __restrict__ etype, const float* __restrict__ w, int fanout,
                                                         const float* __restrict__ h_src, float* __restrict__ out, int64_t n_dst, int num_rels,
                                                         int dim) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    const auto [lane, wave, n_waves] = wave_rows();
    const int units = dim / VEC;
    for (int64_t d = wave; d < n_dst; d += n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        // the first chunk stays in registers; -1 as a type matches no relation (padding, past the end, out of range)
        int32_t mine0 = -1, t0 = -1;
        float w0 = 1.0f;
        uint64_t seen = 0; // the relations among this lane's slots
        for (int64_t e0 = beg; e0 < end; e0 += 64) {
            if (e0 + lane >= end) continue;
            const int32_t s = idx[e0 + lane];
            int32_t t = s >= 0 ? etype[e0 + lane] : -1;
            if (t < 0 || t >= num_rels) t = -1;
            if (t >= 0) seen |= 1ull << t;
            if (e0 == beg) {
                mine0 = s, t0 = t;
                if (w && t >= 0) w0 = w[e0 + lane];
            }
        }
        for (int r = 0; r < num_rels; ++r) {
            float* o = out + (d * num_rels + r) * dim;
            if (!__ballot((seen >> r) & 1)) { // wave-uniform
                for (int u = lane; u < units; u += 64) *reinterpret_cast<vf*>(o + (int64_t)u * VEC) = vf(0.0f);
                continue;
            }
            for (int u0 = 0; u0 < units; u0 += 64) { // wave-uniform trip counts: the shuffles below need every lane
                const int u = u0 + lane;
                vf acc = vf(0.0f);
                for (int64_t e0 = beg; e0 < end; e0 += 64) {
                    int32_t mine = mine0, t = t0;
                    float wm = w0;
                    if (e0 != beg) { // wave-uniform
                        load_chunk(idx, e0, end, lane, &mine);
                        t = mine >= 0 ? etype[e0 + lane] : -1;
                        wm = w && t == r ? w[e0 + lane] : 1.0f;
                    }
                    uint64_t hit = __ballot(t == r); // t == r >= 0 only on a valid slot
                    while (hit) {
                        const int j = __builtin_ctzll(hit);
                        hit &= hit - 1;
                        const int32_t s = __shfl(mine, j);
                        const float wj = __shfl(wm, j);
                        if (u < units) axpy<VEC>(acc, wj, *reinterpret_cast<const vf*>(h_src + (int64_t)s * dim + (int64_t)u * VEC));
                    }
                }
                if (u < units) *reinterpret_cast<vf*>(o + (int64_t)u * VEC) = acc;
            }
        }
    }
}

// Both gradients of the relation-typed sum in one launch, either of them optional (null); with g_j = grad_out[d, etype_j, :]:
//   grad_src[s_j] += w_j * g_j          hardware float atomics into a buffer the caller zeroed, a lane per float (the mean backward's
//                                       mapping: an atomic instruction of the wave covers 256 contiguous bytes); the order varies;
//   grad_w[slot j] = <g_j, h_src[s_j]>   the weighted sum backward's arithmetic on its lanes -- each lane sums its 16-byte units with
//                                       fmas, a butterfly adds the 64 lanes, lane j of the chunk keeps edge j's value -- so with R = 1
//                                       it gives that kernel's bits; 0 on a padding slot and on a type outside [0, R).
// One wave per row; only the edges with a type in range are visited.  g_j is read from the cache per edge, in each of the two layouts.
template <int VEC, bool CSR>
__global__ __launch_bounds__(kBlock) void rel_sum_backward_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                                  const int32_t* __restrict__ etype, const float* __restrict__ w, int fanout,
                                                                  const float* __restrict__ h_src, const float* __restrict__ grad_out,
                                                                  float* __restrict__ grad_src, float* __restrict__ grad_w, int64_t n_dst,
                                                                  int num_rels, int dim) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    const auto [lane, wave, n_waves] = wave_rows();
    const int units = dim / VEC;
    for (int64_t d = wave; d < n_dst; d += n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        for (int64_t e0 = beg; e0 < end; e0 += 64) { // wave-uniform trip counts
            const bool have = e0 + lane < end;
            int32_t mine;
            load_chunk(idx, e0, end, lane, &mine);
            int32_t t = mine >= 0 ? etype[e0 + lane] : -1;
            if (t < 0 || t >= num_rels) t = -1;
            const float wm = w && t >= 0 ? w[e0 + lane] : 1.0f;
            float gw = 0.0f;
            uint64_t todo = __ballot(t >= 0);
            while (todo) {
                const int j = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int32_t s = __shfl(mine, j);
                const float* g = grad_out + (d * num_rels + __shfl(t, j)) * dim;
                if (grad_src) { // wave-uniform
                    const float wj = __shfl(wm, j);
                    for (int c = lane; c < dim; c += 64) unsafeAtomicAdd(grad_src + (int64_t)s * dim + c, wj * g[c]);
                }
                if (grad_w) { // wave-uniform
                    float part = 0.0f;
                    for (int u = lane; u < units; u += 64) {
                        const vf gv = *reinterpret_cast<const vf*>(g + (int64_t)u * VEC);
                        const vf hv = *reinterpret_cast<const vf*>(h_src + (int64_t)s * dim + (int64_t)u * VEC);
                        for (int i = 0; i < VEC; ++i) part = __builtin_fmaf(gv[i], hv[i], part);
                    }
                    const float tot = wave_sum(part);
                    if (lane == j) gw = tot;
                }
            }
            if (grad_w && have) grad_w[e0 + lane] = gw;
        }
    }
}

// Relation-typed GAT attention on a block (the message step of DGL's HeteroGraphConv over one GATConv per edge type, aggregate='sum', on
// a homogenised block): the softmax runs per (destination, relation), and the relations' results are summed.  Every slot carries the
// row of el / feat its edge reads (row, -1 = padding; it stands where nbr / indices stand in the other ops) and its type.  For dst d,
// head h, relation r and the slots j of d with row_j >= 0 and etype_j == r:
//   e_j = leaky_relu(el[row_j, h] + er[d, r, h], slope),  a_j = softmax of e over those j,  out[d, h, :] = sum_r sum_j a_j feat[row_j, h, :]
// One wave per destination row.  The scores are scalars per edge and head, so a first pass over the row's chunks costs no feature
// traffic: it keeps the running max and sum of every (relation, head) in LDS (hence R * H <= kRelGatMaxStates), visiting per chunk
// only the relations present in it -- a ballot on the first live lane's type peels them off one by one -- with a masked wave_max /
// wave_sum each.  The second pass then knows every group's max m and sum l: a_j = exp(e_j - m) / l, and the sum over edges and
// relations is one plain weighted sum into out[d]: softmax_accumulate with FINAL weights, nothing to rescale.  A row of at most 64
// slots (every fixed row) keeps its (row, type) words in registers between the passes.  A slot whose type is outside [0, R) is
// treated as padding.  lse[d, r, h] = m + log(l), -inf where (d, r) has no edge, is all the backward keeps.
constexpr int kRelGatMaxStates = 256;

// load_chunk for a typed row: lane j also takes slot e0 + j's type into *t; a padding slot, a slot past the row's end and a slot whose
// type is outside [0, num_rels) all leave with *mine == *t == -1.
__device__ __forceinline__ int load_rel_chunk(const int32_t* row, const int32_t* etype, int64_t e0, int64_t end, int lane, int num_rels,
                                              int32_t* mine, int32_t* t) {
    const int n = load_chunk(row, e0, end, lane, mine);
    *t = *mine >= 0 ? etype[e0 + lane] : -1;
    if (*t < 0 || *t >= num_rels) *t = *mine = -1;
    return n;
}

template <int VEC, bool CSR>
__global__ __launch_bounds__(kBlock) void rel_gat_aggregate_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ row,
                                                                   const int32_t* __restrict__ etype, int fanout, const float* __restrict__ el,
                                                                   const float* __restrict__ er, const float* __restrict__ feat,
                                                                   float* __restrict__ out, float* __restrict__ lse, int64_t n_dst, int num_rels,
                                                                   int heads, int dim, float slope) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    __shared__ float w_lds[kWavesPerBlock][64 * kGatMaxHeads];   // a_j of the chunk, [edge][head]
    __shared__ float st_lds[kWavesPerBlock][2 * kRelGatMaxStates]; // per (relation, head): the running max; the running sum, then 1 / sum
    const auto [lane, wave, n_waves] = wave_rows();
    float* w = w_lds[threadIdx.x >> 6];
    float* m_run = st_lds[threadIdx.x >> 6];
    float* l_run = m_run + kRelGatMaxStates;
    const int hd = heads * dim, units = hd / VEC, upl = dim / VEC, rh = num_rels * heads;
    for (int64_t d = wave; d < n_dst; d += n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        const float* er_d = er + d * rh;
        wave_lds_sync(); // the previous row has read m_run / l_run
        for (int i = lane; i < rh; i += 64) {
            m_run[i] = kNegInf;
            l_run[i] = 0.0f;
        }
        int32_t mine0 = -1, t0 = -1; // the first chunk stays in registers
        for (int64_t e0 = beg; e0 < end; e0 += 64) { // wave-uniform trip counts: the ballots and shuffles below need every lane
            int32_t mine, t;
            load_rel_chunk(row, etype, e0, end, lane, num_rels, &mine, &t);
            if (e0 == beg) mine0 = mine, t0 = t;
            wave_lds_sync(); // m_run / l_run are set
            uint64_t todo = __ballot(t >= 0);
            while (todo) { // the relations present in the chunk, by first slot
                const int r = __shfl(t, __builtin_ctzll(todo));
                const bool in = t == r;
                todo &= ~__ballot(in);
                for (int h = 0; h < heads; ++h) { // an online softmax step of group (r, h): lane 0 keeps its max and sum
                    float e = kNegInf;
                    if (in) e = leaky_score(el[(int64_t)mine * heads + h] + er_d[r * heads + h], slope);
                    const float mo = m_run[r * heads + h];
                    const float mn = fmaxf(mo, wave_max(e));
                    const float sum = wave_sum(in ? expf(e - mn) : 0.0f);
                    if (lane == 0) {
                        m_run[r * heads + h] = mn;
                        l_run[r * heads + h] = l_run[r * heads + h] * (mo == mn ? 1.0f : (mo == kNegInf ? 0.0f : expf(mo - mn))) + sum;
                    }
                }
            }
        }
        wave_lds_sync();
        for (int i = lane; i < rh; i += 64) {
            const float l = l_run[i];
            lse[d * rh + i] = l > 0.0f ? m_run[i] + logf(l) : kNegInf;
            l_run[i] = l > 0.0f ? 1.0f / l : 0.0f;
        }
        if (beg == end) // no chunk runs: an empty CSR row
            for (int u = lane; u < units; u += 64) *reinterpret_cast<vf*>(out + d * hd + (int64_t)u * VEC) = vf(0.0f);
        for (int64_t e0 = beg; e0 < end; e0 += 64) {
            int32_t mine = mine0, t = t0;
            int n = end - beg < 64 ? (int)(end - beg) : 64;
            if (e0 != beg) n = load_rel_chunk(row, etype, e0, end, lane, num_rels, &mine, &t); // wave-uniform
            wave_lds_sync(); // 1 / l is stored; the previous chunk has read w
            for (int h = 0; h < heads; ++h) {
                float a = 0.0f;
                if (t >= 0)
                    a = expf(leaky_score(el[(int64_t)mine * heads + h] + er_d[t * heads + h], slope) - m_run[t * heads + h]) * l_run[t * heads + h];
                w[lane * kGatMaxHeads + h] = a;
            }
            wave_lds_sync();
            softmax_accumulate<VEC, true>(SoftmaxLds{w, nullptr, nullptr, nullptr}, out + d * hd, feat, mine, n, e0 == beg, false, lane, hd, units, upl);
        }
    }
}

// One chunk of the backward below: lane j takes slot e0 + j's (row, type), and leaves in LDS, for every head, a_j = exp(e_j - lse) in w,
// divided by its group's S[type_j, h] where S is given, and <g[h, :], feat[row_j, h, :]> in dot (dot_grad_feat_walk, GAT's); with ADD
// also grad_feat[row_j, h, :] += a_j g[h, :].  -> the chunk's length.
template <bool ADD>
__device__ __forceinline__ int rel_gat_chunk_dots(float* w, float* dot, const int32_t* __restrict__ row, const int32_t* __restrict__ etype,
                                                  int64_t e0, int64_t end, int lane, int num_rels, int heads, int dim,
                                                  const float* __restrict__ el, const float* __restrict__ er_d,
                                                  const float* __restrict__ lse_d, const float* S, const float* __restrict__ feat,
                                                  const float* __restrict__ g, float* __restrict__ grad_feat, float slope, int32_t* mine_out,
                                                  int32_t* t_out) {
    int32_t mine, t;
    const int n = load_rel_chunk(row, etype, e0, end, lane, num_rels, &mine, &t);
    wave_lds_sync(); // the previous chunk has read w and dot
    for (int h = 0; h < heads; ++h) {
        float a = 0.0f;
        if (t >= 0) {
            a = expf(leaky_score(el[(int64_t)mine * heads + h] + er_d[t * heads + h], slope) - lse_d[t * heads + h]);
            if (S) a = normalised(a, S[t * heads + h]);
        }
        w[lane * kGatMaxHeads + h] = a;
        dot[lane * kGatMaxHeads + h] = 0.0f;
    }
    wave_lds_sync();
    dot_grad_feat_walk<ADD>(w, dot, mine, n, feat, g, grad_feat, lane, dim, heads * dim);
    wave_lds_sync();
    *mine_out = mine, *t_out = t;
    return n;
}

// Backward, p_j = exp(e_j - lse[d, etype_j, h]) recomputed from the saved log-sum-exp; with dot_j = <g[d, h, :], feat[row_j, h, :]>,
// G[r, h] = sum over the edges j of relation r of p_j dot_j -- relation r's <g, out_r>, which the stored out, summed over relations,
// cannot give -- S[r, h] = sum of p_j over the same edges, and a_j = p_j / S[etype_j, h] (`normalised` above):
//   grad_feat[row_j, h, :] += a_j g[d, h, :],  t_j = a_j (dot_j - G[etype_j, h] / S[etype_j, h]) (z_j > 0 ? 1 : slope),
//   grad_el[row_j, h] += t_j,  grad_er[d, r, h] = sum of t_j over relation r's edges.
// S is 1 but for the rounding of lse and of expf.  Without the division of G the sum of a group's p_j (dot_j - G), zero in exact
// arithmetic, is (1 - S) G, an error of one sign per group that whatever sums the t_j over edges afterwards (the gradients of attn_l
// and attn_r) does not cancel; without that of p_j a group's grad_feat adds up to S g.
// A first walk over the row's chunks gives p and dot and adds every group's G and S in LDS (two masked wave_sums per relation present
// and head, in chunk order).  A row of one chunk -- every fixed row -- then divides the p still in LDS, adds grad_feat from them and forms
// t; a longer row walks its source rows a second time, now with S, for grad_feat and t.  grad_feat and grad_el take hardware float atomics (zeroed by the caller); grad_er is summed
// in LDS in a fixed order and written whole.
template <bool CSR>
__global__ __launch_bounds__(kBlock) void rel_gat_aggregate_backward_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ row, const int32_t* __restrict__ etype, int fanout,
    const float* __restrict__ el, const float* __restrict__ er, const float* __restrict__ feat, const float* __restrict__ lse,
    const float* __restrict__ grad_out, float* __restrict__ grad_feat, float* __restrict__ grad_el, float* __restrict__ grad_er, int64_t n_dst,
    int num_rels, int heads, int dim, float slope) {
    __shared__ float w_lds[kWavesPerBlock][64 * kGatMaxHeads];     // a_j of the chunk, [edge][head]
    __shared__ float dot_lds[kWavesPerBlock][64 * kGatMaxHeads];   // <g, feat_j>, [edge][head]
    __shared__ float gs_lds[kWavesPerBlock][3 * kRelGatMaxStates]; // per (relation, head): G, then G / S; the sum of t_j so far; S
    const WaveRows wr = wave_rows();
    const int lane = wr.lane; // a lambda below captures it
    float* w = w_lds[threadIdx.x >> 6];
    float* dot = dot_lds[threadIdx.x >> 6];
    float* G = gs_lds[threadIdx.x >> 6];
    float* ter = G + kRelGatMaxStates;
    float* S = ter + kRelGatMaxStates;
    const int hd = heads * dim, rh = num_rels * heads;
    for (int64_t d = wr.wave; d < n_dst; d += wr.n_waves) {
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        const float* g = grad_out + d * hd;
        const float* er_d = er + d * rh;
        const float* lse_d = lse + d * rh;
        wave_lds_sync(); // the previous row has read G / ter
        for (int i = lane; i < rh; i += 64) {
            G[i] = 0.0f;
            ter[i] = 0.0f;
            S[i] = 0.0f;
        }
        // t_j of the chunk whose a and dot are in LDS, into grad_el and ter
        auto t_step = [&](int32_t mine, int32_t t) {
            uint64_t todo = __ballot(t >= 0);
            while (todo) {
                const int r = __shfl(t, __builtin_ctzll(todo));
                const bool in = t == r;
                todo &= ~__ballot(in);
                for (int h = 0; h < heads; ++h) {
                    float tv = 0.0f;
                    if (in) {
                        const float z = el[(int64_t)mine * heads + h] + er_d[r * heads + h];
                        tv = w[lane * kGatMaxHeads + h] * (dot[lane * kGatMaxHeads + h] - G[r * heads + h]) * (z > 0.0f ? 1.0f : slope);
                        unsafeAtomicAdd(grad_el + (int64_t)mine * heads + h, tv);
                    }
                    const float ts = wave_sum(tv);
                    if (lane == 0) ter[r * heads + h] += ts;
                }
            }
        };
        int32_t mine = -1, t = -1;
        for (int64_t e0 = beg; e0 < end; e0 += 64) { // wave-uniform trip counts
            rel_gat_chunk_dots<false>(w, dot, row, etype, e0, end, lane, num_rels, heads, dim, el, er_d, lse_d, nullptr, feat, g, nullptr, slope, &mine,
                                      &t);
            uint64_t todo = __ballot(t >= 0);
            while (todo) {
                const int r = __shfl(t, __builtin_ctzll(todo));
                const bool in = t == r;
                todo &= ~__ballot(in);
                for (int h = 0; h < heads; ++h) {
                    const float a = in ? w[lane * kGatMaxHeads + h] : 0.0f;
                    const float gs = wave_sum(a * dot[lane * kGatMaxHeads + h]);
                    const float ss = wave_sum(a);
                    if (lane == 0) {
                        G[r * heads + h] += gs;
                        S[r * heads + h] += ss;
                    }
                }
            }
        }
        wave_lds_sync(); // G and S are whole
        for (int i = lane; i < rh; i += 64) G[i] = S[i] > 0.0f ? G[i] / S[i] : 0.0f; // a group without an edge is never read
        wave_lds_sync();
        if (end - beg <= 64) { // wave-uniform: the one chunk's p and dot are still in LDS; lane j divides its own words
            const int n = (int)(end - beg);
            if (t >= 0)
                for (int h = 0; h < heads; ++h) w[lane * kGatMaxHeads + h] = normalised(w[lane * kGatMaxHeads + h], S[t * heads + h]);
            wave_lds_sync();
            for (int c0 = 0; c0 < hd; c0 += 64) { // wave-uniform trip count: the shuffles below need every lane
                const int c = c0 + lane;
                const int hc = c < hd ? c / dim : 0;
                const float gc = c < hd ? g[c] : 0.0f;
                for (int j = 0; j < n; ++j) {
                    const int32_t s = __shfl(mine, j);
                    if (s >= 0 && c < hd) unsafeAtomicAdd(grad_feat + (int64_t)s * hd + c, w[j * kGatMaxHeads + hc] * gc);
                }
            }
            t_step(mine, t);
        } else {
            for (int64_t e0 = beg; e0 < end; e0 += 64) {
                rel_gat_chunk_dots<true>(w, dot, row, etype, e0, end, lane, num_rels, heads, dim, el, er_d, lse_d, S, feat, g, grad_feat, slope, &mine,
                                         &t);
                t_step(mine, t);
            }
        }
        wave_lds_sync();
        for (int i = lane; i < rh; i += 64) grad_er[d * rh + i] = ter[i];
    }
}

// 16-B accesses need a row length of whole float4s and both row arrays on a 16-B boundary
bool vec4_ok(int dim, const void* a, const void* b) {
    return dim % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0;
}

// f(std::integral_constant<int, VEC>): the float4 instantiation of a kernel, or its scalar one
template <typename F>
void dispatch_vec(bool vec4, F&& f) {
    if (vec4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 1>{});
}

dim3 row_grid(int64_t n_dst) { return dim3(grid1d(n_dst * 64, kBlock, 8192)); } // one wave per destination row

// Every launch below runs the same checks in the same order: the shape, then n_dst == 0 is done, then the null buffers.  The fixed
// form of an entry passes indptr = nullptr and its fan-out, the CSR form fanout = 0.
template <bool CSR>
bool fanout_ok(int fanout) { return CSR || (fanout >= 1 && fanout <= 32); }

template <bool CSR>
int shape_check(int64_t n_dst, int fanout, int dim) {
    if (n_dst >= 0 && dim >= 1 && fanout_ok<CSR>(fanout)) return COALA_OK;
    return CSR ? fail(COALA_EINVAL, "bad block shape") : fail(COALA_EINVAL, "bad block shape (fan-out 1..32)");
}

template <bool CSR>
int gat_shape_check(int64_t n_dst, int fanout, int heads, int dim) {
    if (!fanout_ok<CSR>(fanout)) return fail(COALA_EINVAL, "bad block shape (fan-out 1..32)");
    if (n_dst < 0 || heads < 1 || heads > kGatMaxHeads || dim < 1 || (int64_t)heads * dim > INT32_MAX)
        return fail(COALA_EINVAL, "bad block shape (heads 1..%d, dim >= 1, n_dst >= 0)", kGatMaxHeads);
    return COALA_OK;
}

constexpr int kMaxRels = 64; // a row's relations are a 64-bit mask

template <bool CSR>
int rel_shape_check(int64_t n_dst, int fanout, int num_rels, int dim) {
    if (n_dst >= 0 && dim >= 1 && num_rels >= 1 && num_rels <= kMaxRels && fanout_ok<CSR>(fanout)) return COALA_OK;
    return CSR ? fail(COALA_EINVAL, "bad block shape (relations 1..%d)", kMaxRels)
               : fail(COALA_EINVAL, "bad block shape (fan-out 1..32, relations 1..%d)", kMaxRels);
}

template <bool CSR>
int rel_gat_shape_check(int64_t n_dst, int fanout, int num_rels, int heads, int dim) {
    if (int rc = gat_shape_check<CSR>(n_dst, fanout, heads, dim)) return rc;
    if (num_rels < 1 || num_rels > kMaxRels || num_rels * heads > kRelGatMaxStates)
        return fail(COALA_EINVAL, "bad block shape (relations 1..%d, relations * heads <= %d)", kMaxRels, kRelGatMaxStates);
    return COALA_OK;
}

template <bool CSR>
int mean_launch(int device, const int64_t* indptr, const int32_t* idx, int fanout, const float* h_src, float* out, int64_t n_dst, int dim,
                void* stream) {
    if (int rc = shape_check<CSR>(n_dst, fanout, dim)) return rc;
    if (n_dst == 0) return COALA_OK;
    if ((CSR && !indptr) || !idx || !h_src || !out) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    dispatch_vec(vec4_ok(dim, h_src, out), [&](auto vec) {
        hipLaunchKernelGGL((mean_aggregate_kernel<decltype(vec)::value, CSR>), row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr, idx,
                           fanout, h_src, out, n_dst, dim);
    });
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

template <bool CSR>
int mean_backward_launch(int device, const int64_t* indptr, const int32_t* idx, int fanout, const float* grad_out, float* grad_src, int64_t n_dst,
                         int dim, void* stream) {
    if (int rc = shape_check<CSR>(n_dst, fanout, dim)) return rc;
    if (n_dst == 0) return COALA_OK;
    if ((CSR && !indptr) || !idx || !grad_out || !grad_src) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(mean_aggregate_backward_kernel<CSR>, row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr, idx, fanout, grad_out,
                       grad_src, n_dst, dim);
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

// The forward of GAT, GATv2 and dot-product attention: (a, b, c) and param as Score names them; 16-B accesses go to Score's value table.
template <typename Score, bool CSR>
int attention_launch(int device, const int64_t* indptr, const int32_t* idx, int fanout, const float* a, const float* b, const float* c, float* out,
                     float* lse, int64_t n_dst, int heads, int dim, float param, void* stream) {
    if (int rc = gat_shape_check<CSR>(n_dst, fanout, heads, dim)) return rc;
    if (n_dst == 0) return COALA_OK;
    if ((CSR && !indptr) || !idx || !a || !b || !c || !out || !lse) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    dispatch_vec(vec4_ok(dim, Score::values(a, b, c), out), [&](auto vec) {
        hipLaunchKernelGGL((attention_aggregate_kernel<Score, decltype(vec)::value, CSR>), row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream,
                           indptr, idx, fanout, a, b, c, out, lse, n_dst, heads, dim, param);
    });
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

template <bool CSR>
int gat_backward_launch(int device, const int64_t* indptr, const int32_t* idx, int fanout, const float* el, const float* er, const float* feat,
                        const float* out, const float* lse, const float* grad_out, float* grad_feat, float* grad_el, float* grad_er,
                        int64_t n_dst, int heads, int dim, float slope, void* stream) {
    if (int rc = gat_shape_check<CSR>(n_dst, fanout, heads, dim)) return rc;
    if (n_dst == 0) return COALA_OK;
    if ((CSR && !indptr) || !idx || !el || !er || !feat || !out || !lse || !grad_out || !grad_feat || !grad_el || !grad_er)
        return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(gat_aggregate_backward_kernel<CSR>, row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr, idx, fanout, el, er, feat,
                       out, lse, grad_out, grad_feat, grad_el, grad_er, n_dst, heads, dim, slope);
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

// The grad_attn partials rule: with a partials buffer the grid is exactly `parts` blocks and block b stores row b.  The sums of a row
// of at most 1024 floats stay in registers (RP = 1, 2, 4, 8 or 16 passes of 64 floats, four waves a block); a longer row takes the
// RP = 0 kernel, one wave a block.  Without a partials buffer the grid is that of the other block ops.
template <bool CSR>
int gatv2_backward_launch(int device, const int64_t* indptr, const int32_t* idx, int fanout, const float* feat_src, const float* feat_dst,
                          const float* attn, const float* out, const float* lse, const float* grad_out, float* grad_src, float* grad_dst,
                          float* grad_attn_parts, int parts, int64_t n_dst, int heads, int dim, float slope, void* stream) {
    if (int rc = gat_shape_check<CSR>(n_dst, fanout, heads, dim)) return rc;
    if (grad_attn_parts && parts < 1) return fail(COALA_EINVAL, "bad block shape (parts >= 1)");
    if (n_dst == 0 || (!grad_src && !grad_dst && !grad_attn_parts)) return COALA_OK;
    if ((CSR && !indptr) || !idx || !feat_src || !feat_dst || !attn || !out || !lse || !grad_out) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    const int passes = (heads * dim + 63) / 64;
    const bool regs = grad_attn_parts && passes <= kGatMaxHeads;
    const dim3 grid(grad_attn_parts ? dim3(parts) : row_grid(n_dst)), blk(grad_attn_parts && !regs ? 64 : kBlock);
    auto launch = [&](auto rp) {
        hipLaunchKernelGGL((gatv2_aggregate_backward_kernel<decltype(rp)::value, CSR>), grid, blk, 0, (hipStream_t)stream, indptr, idx, fanout,
                           feat_src, feat_dst, attn, out, lse, grad_out, grad_src, grad_dst, grad_attn_parts, n_dst, heads, dim, slope);
    };
    if (!regs) launch(std::integral_constant<int, 0>{});
    else if (passes <= 1) launch(std::integral_constant<int, 1>{});
    else if (passes <= 2) launch(std::integral_constant<int, 2>{});
    else if (passes <= 4) launch(std::integral_constant<int, 4>{});
    else if (passes <= 8) launch(std::integral_constant<int, 8>{});
    else launch(std::integral_constant<int, 16>{});
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

template <bool CSR>
int dot_gat_backward_launch(int device, const int64_t* indptr, const int32_t* row, int fanout, const float* q, const float* k, const float* v,
                            const float* out, const float* lse, const float* grad_out, float* grad_q, float* grad_k, float* grad_v,
                            int64_t n_dst, int heads, int dim, float scale, void* stream) {
    if (int rc = gat_shape_check<CSR>(n_dst, fanout, heads, dim)) return rc;
    if (n_dst == 0 || (!grad_q && !grad_k && !grad_v)) return COALA_OK;
    if ((CSR && !indptr) || !row || !q || !k || !v || !out || !lse || !grad_out) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(dot_gat_aggregate_backward_kernel<CSR>, row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr, row, fanout, q, k, v,
                       out, lse, grad_out, grad_q, grad_k, grad_v, n_dst, heads, dim, scale);
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

template <bool CSR>
int weighted_sum_launch(int device, const int64_t* indptr, const int32_t* idx, const float* w, int fanout, const float* h_src, float* out,
                        int64_t n_dst, int dim, void* stream) {
    if (int rc = shape_check<CSR>(n_dst, fanout, dim)) return rc;
    if (n_dst == 0) return COALA_OK;
    if ((CSR && !indptr) || !idx || !w || !h_src || !out) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    dispatch_vec(vec4_ok(dim, h_src, out), [&](auto vec) {
        hipLaunchKernelGGL((weighted_sum_kernel<decltype(vec)::value, CSR>), row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr, idx, w,
                           fanout, h_src, out, n_dst, dim);
    });
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

template <bool CSR>
int weighted_sum_backward_launch(int device, const int64_t* indptr, const int32_t* idx, const float* w, int fanout, const float* h_src,
                                 const float* grad_out, float* grad_src, float* grad_w, int64_t n_dst, int dim, void* stream) {
    if (int rc = shape_check<CSR>(n_dst, fanout, dim)) return rc;
    if (n_dst == 0 || (!grad_src && !grad_w)) return COALA_OK;
    if ((CSR && !indptr) || !idx || !w || !grad_out || (grad_w && !h_src)) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    dispatch_vec(vec4_ok(dim, grad_out, grad_w ? h_src : nullptr), [&](auto vec) {
        hipLaunchKernelGGL((weighted_sum_backward_kernel<decltype(vec)::value, CSR>), row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr,
                           idx, w, fanout, h_src, grad_out, grad_src, grad_w, n_dst, dim);
    });
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

template <bool CSR>
int max_launch(int device, const int64_t* indptr, const int32_t* idx, int fanout, const float* h_src, float* out, int32_t* arg, int64_t n_dst,
               int dim, void* stream) {
    if (int rc = shape_check<CSR>(n_dst, fanout, dim)) return rc;
    if (n_dst == 0) return COALA_OK;
    if ((CSR && !indptr) || !idx || !h_src || !out) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    dispatch_vec(vec4_ok(dim, h_src, out) && vec4_ok(dim, arg, nullptr), [&](auto vec) {
        hipLaunchKernelGGL((max_aggregate_kernel<decltype(vec)::value, CSR>), row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr, idx,
                           fanout, h_src, out, arg, n_dst, dim);
    });
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

int max_backward_launch(int device, const int32_t* arg, const float* grad_out, float* grad_src, int64_t n_dst, int dim, void* stream) {
    if (int rc = shape_check<true>(n_dst, 0, dim)) return rc; // one kernel for both forms: no neighbour list, no fan-out
    if (n_dst == 0) return COALA_OK;
    if (!arg || !grad_out || !grad_src) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(max_aggregate_backward_kernel, row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, arg, grad_out, grad_src, n_dst, dim);
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

template <bool CSR>
int rel_sum_launch(int device, const int64_t* indptr, const int32_t* idx, const int32_t* etype, const float* w, int fanout, const float* h_src,
                   float* out, int64_t n_dst, int num_rels, int dim, void* stream) {
    if (int rc = rel_shape_check<CSR>(n_dst, fanout, num_rels, dim)) return rc;
    if (n_dst == 0) return COALA_OK;
    if ((CSR && !indptr) || !idx || !etype || !h_src || !out) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    dispatch_vec(vec4_ok(dim, h_src, out), [&](auto vec) {
        hipLaunchKernelGGL((rel_sum_kernel<decltype(vec)::value, CSR>), row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr, idx, etype, w,
                           fanout, h_src, out, n_dst, num_rels, dim);
    });
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

template <bool CSR>
int rel_sum_backward_launch(int device, const int64_t* indptr, const int32_t* idx, const int32_t* etype, const float* w, int fanout,
                            const float* h_src, const float* grad_out, float* grad_src, float* grad_w, int64_t n_dst, int num_rels, int dim,
                            void* stream) {
    if (int rc = rel_shape_check<CSR>(n_dst, fanout, num_rels, dim)) return rc;
    if (n_dst == 0 || (!grad_src && !grad_w)) return COALA_OK;
    if ((CSR && !indptr) || !idx || !etype || !grad_out || (grad_w && !h_src)) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    dispatch_vec(vec4_ok(dim, grad_out, grad_w ? h_src : nullptr), [&](auto vec) { // the weighted sum backward's choice: the same bits at R = 1
        hipLaunchKernelGGL((rel_sum_backward_kernel<decltype(vec)::value, CSR>), row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr, idx,
                           etype, w, fanout, h_src, grad_out, grad_src, grad_w, n_dst, num_rels, dim);
    });
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

template <bool CSR>
int rel_gat_launch(int device, const int64_t* indptr, const int32_t* row, const int32_t* etype, int fanout, const float* el, const float* er,
                   const float* feat, float* out, float* lse, int64_t n_dst, int num_rels, int heads, int dim, float slope, void* stream) {
    if (int rc = rel_gat_shape_check<CSR>(n_dst, fanout, num_rels, heads, dim)) return rc;
    if (n_dst == 0) return COALA_OK;
    if ((CSR && !indptr) || !row || !etype || !el || !er || !feat || !out || !lse) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    dispatch_vec(vec4_ok(dim, feat, out), [&](auto vec) {
        hipLaunchKernelGGL((rel_gat_aggregate_kernel<decltype(vec)::value, CSR>), row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr, row,
                           etype, fanout, el, er, feat, out, lse, n_dst, num_rels, heads, dim, slope);
    });
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

template <bool CSR>
int rel_gat_backward_launch(int device, const int64_t* indptr, const int32_t* row, const int32_t* etype, int fanout, const float* el,
                            const float* er, const float* feat, const float* lse, const float* grad_out, float* grad_feat, float* grad_el,
                            float* grad_er, int64_t n_dst, int num_rels, int heads, int dim, float slope, void* stream) {
    if (int rc = rel_gat_shape_check<CSR>(n_dst, fanout, num_rels, heads, dim)) return rc;
    if (n_dst == 0) return COALA_OK;
    if ((CSR && !indptr) || !row || !etype || !el || !er || !feat || !lse || !grad_out || !grad_feat || !grad_el || !grad_er)
        return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(rel_gat_aggregate_backward_kernel<CSR>, row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr, row, etype, fanout,
                       el, er, feat, lse, grad_out, grad_feat, grad_el, grad_er, n_dst, num_rels, heads, dim, slope);
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

// ------------------------------------------------------------------------------------------------------------ edge exclusion
// Take edges out of a block by their edge id (link prediction: the seed edges must not be in the message-flow blocks).  excl is a
// sorted int64 list of CSC positions, a few thousand at most: every slot binary-searches its id in it.  Survivors keep their order.

__device__ __forceinline__ bool listed(const int64_t* __restrict__ list, int64_t n, int64_t e) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (list[mid] < e) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && list[lo] == e;
}

// Fixed form: 32 lanes per row (fan-out <= 32), a lane per slot; the survivors are ballot-compacted to the front of the row of the
// output arrays and -1 fills both behind them ("valid entries first").  Out of place: nbr_out / eid_out are not the inputs.
__global__ __launch_bounds__(kBlock) void exclude_edges_kernel(const int32_t* __restrict__ nbr, const int64_t* __restrict__ eid, int fanout,
                                                               const int64_t* __restrict__ excl, int64_t n_excl, int32_t* __restrict__ nbr_out,
                                                               int64_t* __restrict__ eid_out, int64_t n_dst) {
    const auto [lane, wave, n_waves] = wave_rows();
    const int gl = lane & 31, gbase = lane - gl;
    for (int64_t d0 = wave * 2; d0 < n_dst; d0 += n_waves * 2) { // wave-uniform trip count: the ballot needs every lane
        const int64_t d = d0 + (lane >> 5);
        const bool slot = d < n_dst && gl < fanout;
        const int64_t q = d * fanout + gl;
        const int32_t s = slot ? nbr[q] : -1;
        const int64_t e = s >= 0 ? eid[q] : -1;
        const bool keep = s >= 0 && !listed(excl, n_excl, e);
        const uint32_t m = (uint32_t)(__ballot(keep) >> gbase);
        const int cnt = __builtin_popcount(m);
        if (keep) {
            const int64_t at = d * fanout + __builtin_popcount(m & ((1u << gl) - 1u));
            nbr_out[at] = s;
            eid_out[at] = e;
        }
        if (slot && gl >= cnt) {
            nbr_out[q] = -1;
            eid_out[q] = -1;
        }
    }
}

// CSR form, one wave per row, two passes of one kernel: COUNT writes the row's surviving edges to counts[d]; the caller scans them
// into new_indptr, and the compact pass writes the survivors of row d from new_indptr[d] on.
template <bool COUNT>
__global__ __launch_bounds__(kBlock) void exclude_edges_csr_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                                   const int64_t* __restrict__ eid, const int64_t* __restrict__ excl, int64_t n_excl,
                                                                   int64_t* __restrict__ counts, const int64_t* __restrict__ new_indptr,
                                                                   int32_t* __restrict__ indices_out, int64_t* __restrict__ eid_out, int64_t n_dst) {
    const auto [lane, wave, n_waves] = wave_rows();
    for (int64_t d = wave; d < n_dst; d += n_waves) {
        const int64_t beg = indptr[d], end = indptr[d + 1];
        int64_t run = COUNT ? 0 : new_indptr[d];
        for (int64_t e0 = beg; e0 < end; e0 += 64) { // wave-uniform
            const int64_t i = e0 + lane;
            const int64_t e = i < end ? eid[i] : -1;
            const bool keep = i < end && !listed(excl, n_excl, e);
            const uint64_t m = __ballot(keep);
            if constexpr (!COUNT) {
                if (keep) {
                    const int64_t at = run + __builtin_popcountll(m & ((1ull << lane) - 1ull));
                    indices_out[at] = indices[i];
                    eid_out[at] = e;
                }
            }
            run += __builtin_popcountll(m);
        }
        if (COUNT && lane == 0) counts[d] = run;
    }
}

int exclude_launch(int device, const int32_t* nbr, const int64_t* eid, int fanout, const int64_t* excl, int64_t n_excl, int32_t* nbr_out,
                   int64_t* eid_out, int64_t n_dst, void* stream) {
    if (n_dst < 0 || n_excl < 0 || !fanout_ok<false>(fanout)) return fail(COALA_EINVAL, "bad block shape (fan-out 1..32)");
    if (n_dst == 0) return COALA_OK;
    if (!nbr || !eid || !nbr_out || !eid_out || (n_excl > 0 && !excl)) return fail(COALA_EINVAL, "null buffer");
    if (nbr == nbr_out || eid == eid_out) return fail(COALA_EINVAL, "edge exclusion is out of place");
    HIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(exclude_edges_kernel, dim3(grid1d(n_dst * 32, kBlock, 8192)), dim3(kBlock), 0, (hipStream_t)stream, nbr, eid, fanout, excl,
                       n_excl, nbr_out, eid_out, n_dst);
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

int exclude_csr_launch(int device, const int64_t* indptr, const int32_t* indices, const int64_t* eid, const int64_t* excl, int64_t n_excl,
                       int64_t* counts, const int64_t* new_indptr, int32_t* indices_out, int64_t* eid_out, int64_t n_dst, void* stream) {
    if (n_dst < 0 || n_excl < 0) return fail(COALA_EINVAL, "bad block shape");
    if (n_dst == 0) return COALA_OK;
    const bool count = new_indptr == nullptr;
    if (!indptr || !eid || (n_excl > 0 && !excl) || (count ? !counts : (!indices || !indices_out || !eid_out))) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    if (count)
        hipLaunchKernelGGL(exclude_edges_csr_kernel<true>, row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr, indices, eid, excl, n_excl,
                           counts, new_indptr, indices_out, eid_out, n_dst);
    else
        hipLaunchKernelGGL(exclude_edges_csr_kernel<false>, row_grid(n_dst), dim3(kBlock), 0, (hipStream_t)stream, indptr, indices, eid, excl, n_excl,
                           counts, new_indptr, indices_out, eid_out, n_dst);
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

// ---------------------------------------------------------------------------------------------------------------- pair scores
// out[p, hd] = <h[src_p, hd, :], h[dst_p, hd, :]> (DGL's fn.u_dot_v on a pair graph; a link predictor's score).  GS lanes -- a wave,
// or a lane group for a small dim -- take one (pair, head): two row reads, lane gl multiplies the columns gl, gl + GS, ... with one
// fma per term, then a butterfly sum, so every lane of the group ends with the same bits; no [P, dim] intermediate.  A pair with an
// index < 0 scores 0.  The backward adds g h[dst_p] into grad_h[src_p] and g h[src_p] into grad_h[dst_p] with hardware float atomics
// (grad_h zeroed by the caller; the order varies); a pair with an index < 0 adds nothing.
template <int GS>
__global__ __launch_bounds__(kBlock) void pair_dot_kernel(const float* __restrict__ h, const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                          float* __restrict__ out, int64_t n_units, int heads, int dim) {
    constexpr int GPW = 64 / GS;
    const auto [lane, wave, n_waves] = wave_rows();
    const int gl = lane % GS;
    const int64_t row = (int64_t)heads * dim;
    for (int64_t u0 = wave * GPW; u0 < n_units; u0 += n_waves * GPW) { // wave-uniform trip count: the shuffles need every lane
        const int64_t unit = u0 + lane / GS;
        const bool ok = unit < n_units;
        const int64_t p = ok ? unit / heads : 0;
        const int hd = ok ? (int)(unit % heads) : 0;
        const int32_t a = ok ? src[p] : -1, b = ok ? dst[p] : -1;
        float acc = 0.0f;
        if (a >= 0 && b >= 0) {
            const float* ha = h + (int64_t)a * row + (int64_t)hd * dim;
            const float* hb = h + (int64_t)b * row + (int64_t)hd * dim;
            for (int c = gl; c < dim; c += GS) acc = __builtin_fmaf(ha[c], hb[c], acc);
        }
        for (int o = GS / 2; o; o >>= 1) acc += __shfl_xor(acc, o);
        if (ok && gl == 0) out[unit] = acc;
    }
}

template <int GS>
__global__ __launch_bounds__(kBlock) void pair_dot_backward_kernel(const float* __restrict__ h, const int32_t* __restrict__ src,
                                                                   const int32_t* __restrict__ dst, const float* __restrict__ grad_out,
                                                                   float* __restrict__ grad_h, int64_t n_units, int heads, int dim) {
    const int64_t group = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / GS, n_groups = (int64_t)gridDim.x * kBlock / GS;
    const int gl = threadIdx.x % GS;
    const int64_t row = (int64_t)heads * dim;
    for (int64_t unit = group; unit < n_units; unit += n_groups) {
        const int64_t p = unit / heads;
        const int32_t a = src[p], b = dst[p];
        if (a < 0 || b < 0) continue;
        const int64_t oa = (int64_t)a * row + (unit % heads) * dim, ob = (int64_t)b * row + (unit % heads) * dim;
        const float g = grad_out[unit];
        for (int c = gl; c < dim; c += GS) {
            unsafeAtomicAdd(grad_h + oa + c, g * h[ob + c]);
            unsafeAtomicAdd(grad_h + ob + c, g * h[oa + c]);
        }
    }
}

template <typename F>
void dispatch_pair_group(int dim, F&& f) { // lanes per (pair, head)
    if (dim <= 16) f(std::integral_constant<int, 16>{});
    else if (dim <= 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}

int pair_dot_launch(int device, const float* h, const int32_t* src, const int32_t* dst, const float* grad_out, float* out, int64_t n_pairs,
                    int heads, int dim, void* stream) {
    if (n_pairs < 0 || heads < 1 || dim < 1 || (int64_t)heads * dim > INT32_MAX) return fail(COALA_EINVAL, "bad pair shape (heads >= 1, dim >= 1, n_pairs >= 0)");
    if (n_pairs == 0) return COALA_OK;
    if (!h || !src || !dst || !out) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    const int64_t n_units = n_pairs * heads;
    dispatch_pair_group(dim, [&](auto gs_c) {
        constexpr int GS = decltype(gs_c)::value;
        const dim3 grid(grid1d(n_units * GS, kBlock, 8192));
        if (grad_out)
            hipLaunchKernelGGL(pair_dot_backward_kernel<GS>, grid, dim3(kBlock), 0, (hipStream_t)stream, h, src, dst, grad_out, out, n_units, heads, dim);
        else
            hipLaunchKernelGGL(pair_dot_kernel<GS>, grid, dim3(kBlock), 0, (hipStream_t)stream, h, src, dst, out, n_units, heads, dim);
    });
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

// ---------------------------------------------------------------------------------------------------------- skip-gram window loss
// Walk tables rows int32 [R, len] (-1 = no node) over h fp32 [N, dim]: the pairs of a row are (a, a + j) for every window start a in
// 0 .. len - C and j in 1 .. C - 1, valid when both indices are >= 0; a pair's score is s = <h[rows[r, a]], h[rows[r, a + j]]> and its
// loss softplus(sign * s) (PyG's Node2Vec.loss: sign -1 on the positive walks, +1 on the negatives).  GS lanes -- a wave, or a group of
// 16 / 32 lanes for a small dim, as pair_dot -- take one row: together they copy its len embedding rows into LDS once (a row of no
// node as zeros), a lane per column.  A block holds as many groups as fit 64 KB of LDS (len * dim <= 16384 floats: at least one; a
// shape near that budget runs one wave per block).
// Forward: a lane owns whole PAIRS, gl, gl + GS, ... in pair order: it forms its pair's dot product alone, one fma per column,
// starting at column (its lane index) and wrapping round, so that the lanes of a wave read different LDS banks although they read
// different rows, computes the softplus once, and sums its losses in a double; the group's sums are added by a butterfly: partial[r]
// and count[r] are deterministic.
// Backward: position t of a row is the start of the pairs (t, t + j) and the partner of the pairs (i, t), t - C < i < t, i <= len - C:
// at most 254 partners.  Pass 1 recomputes the score of every partner m from LDS with all lanes of the group on one dot and a
// butterfly sum (a position has a couple of dozen partners in practice: a lane per partner would leave most of a wave idle), and lane
// m % GS keeps d loss / d s = sign * sigmoid(sign * s) in its register m / GS.  Pass 2 forms the position's whole gradient row,
// sum_m coef_m h[partner_m], a lane per column with the coefficients going round by shuffle, in a double, multiplies it by the double
// `scale` and adds it with ONE atomic per (position, element) -- not one per pair -- to the DOUBLE buffer grad_acc (zeroed by the
// caller, who rounds it to fp32 once).  A node of a batch collects hundreds of such additions: in fp32 their rounding, not the
// kernel's arithmetic, would set the gradient's error, and the order of the atomics would show in it; in a double neither does.  The
// partner loops depend on (t, len, C) alone and a group's lanes agree on which positions hold a node, so every shuffle reads a lane
// that runs the same code.
constexpr int kSkipMaxLen = 128, kSkipMaxFloats = 16384;

__device__ __forceinline__ float softplusf(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoidf(float x) {
    const float e = expf(-fabsf(x));
    return (x >= 0.0f ? 1.0f : e) / (1.0f + e);
}

struct SkipRow { // a group's row: its index (-1: the group is past the table) and which of its positions hold a node
    int64_t r;
    uint64_t m0, m1;
    __device__ __forceinline__ bool has(int t) const { return ((t < 64 ? m0 >> t : m1 >> (t - 64)) & 1ull) != 0; }
};

// Stage row r0 + (the lane's group) into the group's LDS slice; -> the row and its validity mask.  Ends with the wave's LDS fence.
template <int GS>
__device__ __forceinline__ SkipRow skip_stage(const float* __restrict__ h, const int32_t* __restrict__ rows, int64_t r0, int64_t n_rows, int len,
                                              int dim, float* __restrict__ sh, int gl) {
    const int64_t r = r0 + (int)threadIdx.x / GS;
    SkipRow row{r < n_rows ? r : -1, 0, 0};
    if (row.r >= 0) {
        for (int t = 0; t < len; ++t) {
            const int32_t s = rows[row.r * len + t];
            if (s >= 0) {
                if (t < 64) row.m0 |= 1ull << t;
                else row.m1 |= 1ull << (t - 64);
            }
            for (int c = gl; c < dim; c += GS) sh[t * dim + c] = s >= 0 ? h[(int64_t)s * dim + c] : 0.0f;
        }
    }
    wave_lds_sync();
    return row;
}

// <sh[a], sh[k]> by one lane: dim fmas from +0, the columns taken from `rot` on and wrapping round.
__device__ __forceinline__ float skip_dot(const float* __restrict__ sh, int a, int k, int dim, int rot) {
    const float* const x = sh + a * dim;
    const float* const y = sh + k * dim;
    float acc = 0.0f;
    int c = rot % dim;
    for (int i = 0; i < dim; ++i) {
        acc = __builtin_fmaf(x[c], y[c], acc);
        c = c + 1 == dim ? 0 : c + 1;
    }
    return acc;
}

// The same dot by the GS lanes of a group together: lane gl the columns gl, gl + GS, ..., then a butterfly sum, so every lane of the
// group ends with the same bits.  Every lane of the group must call it (valid is group-uniform).
template <int GS>
__device__ __forceinline__ float skip_dot_group(const float* __restrict__ sh, int a, int k, int dim, int gl, bool valid) {
    float acc = 0.0f;
    if (valid)
        for (int c = gl; c < dim; c += GS) acc = __builtin_fmaf(sh[a * dim + c], sh[k * dim + c], acc);
    for (int o = GS / 2; o; o >>= 1) acc += __shfl_xor(acc, o);
    return acc;
}

template <int GS>
__global__ __launch_bounds__(kBlock) void skipgram_loss_kernel(const float* __restrict__ h, const int32_t* __restrict__ rows, float* __restrict__ partial,
                                     int32_t* __restrict__ count, int64_t n_rows, int len, int C, int dim, float sign) {
    extern __shared__ float s_skip[];
    const int G = (int)blockDim.x / GS, gl = (int)threadIdx.x % GS;
    float* const sh = s_skip + (size_t)((int)threadIdx.x / GS) * len * dim;
    const int n_pairs = (len - C + 1) * (C - 1);
    for (int64_t r0 = (int64_t)blockIdx.x * G; r0 < n_rows; r0 += (int64_t)gridDim.x * G) { // block-uniform trip count
        const SkipRow row = skip_stage<GS>(h, rows, r0, n_rows, len, dim, sh, gl);
        double sum = 0.0; // a lane adds up to 16129 / GS terms, the group 16129: a double keeps the row's sum at one fp32 rounding
        int32_t cnt = 0;
        if (row.r >= 0) {
            for (int q = gl; q < n_pairs; q += GS) {
                const int a = q / (C - 1), k = a + 1 + q % (C - 1);
                if (row.has(a) && row.has(k)) {
                    sum += (double)softplusf(sign * skip_dot(sh, a, k, dim, gl));
                    ++cnt;
                }
            }
        }
        for (int o = GS / 2; o; o >>= 1) { // every lane of the wave: a group past the table adds zeros
            sum += __shfl_xor(sum, o);
            cnt += __shfl_xor(cnt, o);
        }
        if (row.r >= 0 && gl == 0) {
            partial[row.r] = (float)sum;
            count[row.r] = cnt;
        }
        wave_lds_sync(); // every lane has read the slice before the next row overwrites it
    }
}

template <int GS>
__global__ __launch_bounds__(kBlock) void skipgram_loss_backward_kernel(const float* __restrict__ h, const int32_t* __restrict__ rows, double* __restrict__ grad_acc,
                                              const double* __restrict__ scale_dev, int64_t n_rows, int len, int C, int dim, float sign) {
    constexpr int NCH = 256 / GS; // a position has at most 2 (C - 1) <= 254 partners: partner m's coefficient is coef[m / GS] of lane m % GS
    extern __shared__ float s_skip[];
    const int G = (int)blockDim.x / GS, gl = (int)threadIdx.x % GS, gbase = (int)(threadIdx.x & 63) - gl;
    float* const sh = s_skip + (size_t)((int)threadIdx.x / GS) * len * dim;
    const double scale = *scale_dev;
    for (int64_t r0 = (int64_t)blockIdx.x * G; r0 < n_rows; r0 += (int64_t)gridDim.x * G) { // block-uniform trip count
        const SkipRow row = skip_stage<GS>(h, rows, r0, n_rows, len, dim, sh, gl);
        for (int t = 0; t < len; ++t) {
            if (row.r < 0 || !row.has(t)) continue; // group-uniform: the shuffles below stay inside the group
            const int nf = t + C <= len ? C - 1 : 0;                 // pairs (t, t + 1 + m)
            const int lo = t - C + 1 > 0 ? t - C + 1 : 0;            // pairs (i, t), lo <= i <= hi
            const int hi = t - 1 < len - C ? t - 1 : len - C;
            const int n_part = nf + (hi >= lo ? hi - lo + 1 : 0);
            auto partner = [&](int m) { return m < nf ? t + 1 + m : lo + (m - nf); };
            float coef[NCH];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) coef[ch] = 0.0f;
            for (int m = 0; m < n_part; ++m) { // group-uniform
                const int k = partner(m);
                const bool valid = row.has(k);
                const float s = skip_dot_group<GS>(sh, t, k, dim, gl, valid);
                const float cf = valid ? sign * sigmoidf(sign * s) : 0.0f;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch)
                    if (m / GS == ch && m % GS == gl) coef[ch] = cf;
            }
            const int64_t node = rows[row.r * len + t];
            for (int c0 = 0; c0 < dim; c0 += GS) { // group-uniform trip count: the shuffles below need every lane of the group
                const int c = c0 + gl;
                double g = 0.0;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    if (ch * GS < n_part) {
                        const int n = n_part - ch * GS < GS ? n_part - ch * GS : GS;
                        for (int j = 0; j < n; ++j) {
                            const float cf = __shfl(coef[ch], gbase + j);
                            if (c < dim) g = __builtin_fma((double)cf, (double)sh[partner(ch * GS + j) * dim + c], g);
                        }
                    }
                }
                if (c < dim) unsafeAtomicAdd(grad_acc + node * dim + c, g * scale);
            }
        }
        wave_lds_sync(); // every lane has read the slice before the next row overwrites it
    }
}

int skipgram_launch(int device, const float* h, const int32_t* rows, float* partial, int32_t* count, double* grad_h, const double* scale,
                    int64_t n_rows, int len, int C, int dim, float sign, void* stream) {
    if (n_rows < 0 || len < 2 || len > kSkipMaxLen || C < 2 || C > len || dim < 1 || (int64_t)len * dim > kSkipMaxFloats)
        return fail(COALA_EINVAL, "bad walk table shape (len 2..%d, context 2..len, dim >= 1, len * dim <= %d)", kSkipMaxLen, kSkipMaxFloats);
    if (sign != 1.0f && sign != -1.0f) return fail(COALA_EINVAL, "sign must be +1 or -1");
    if (n_rows == 0) return COALA_OK;
    if (!h || !rows || (grad_h ? !scale : (!partial || !count))) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    dispatch_pair_group(dim, [&](auto gs_c) {
        constexpr int GS = decltype(gs_c)::value;
        const int fit = kSkipMaxFloats / (len * dim);                          // groups whose slices fit 64 KB
        const int G = fit < kBlock / GS ? fit : kBlock / GS;                    // >= 1 by the shape check
        const size_t lds = (size_t)G * len * dim * sizeof(float);
        const dim3 grid(grid1d(n_rows, G, 8192)), blk(G * GS);
        if (grad_h)
            hipLaunchKernelGGL(skipgram_loss_backward_kernel<GS>, grid, blk, lds, (hipStream_t)stream, h, rows, grad_h, scale, n_rows, len, C, dim, sign);
        else
            hipLaunchKernelGGL(skipgram_loss_kernel<GS>, grid, blk, lds, (hipStream_t)stream, h, rows, partial, count, n_rows, len, C, dim, sign);
    });
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

} // namespace

// The C ABI (include/coala_hip.h): every entry forwards to its launch, the fixed form with <false>, a null indptr and its fan-out, the
// CSR form with <true> and fan-out 0.
extern "C" {

int coala_block_mean_aggregate(int device, const int32_t* nbr, const float* h_src, float* out, int64_t n_dst, int fanout, int dim, void* stream) {
    return mean_launch<false>(device, nullptr, nbr, fanout, h_src, out, n_dst, dim, stream);
}

int coala_block_mean_aggregate_backward(int device, const int32_t* nbr, const float* grad_out, float* grad_src, int64_t n_dst, int fanout,
                                        int dim, void* stream) {
    return mean_backward_launch<false>(device, nullptr, nbr, fanout, grad_out, grad_src, n_dst, dim, stream);
}

int coala_block_mean_aggregate_csr(int device, const int64_t* indptr, const int32_t* indices, const float* h_src, float* out, int64_t n_dst, int dim,
                                   void* stream) {
    return mean_launch<true>(device, indptr, indices, 0, h_src, out, n_dst, dim, stream);
}

int coala_block_mean_aggregate_csr_backward(int device, const int64_t* indptr, const int32_t* indices, const float* grad_out, float* grad_src,
                                            int64_t n_dst, int dim, void* stream) {
    return mean_backward_launch<true>(device, indptr, indices, 0, grad_out, grad_src, n_dst, dim, stream);
}

int coala_block_gat_aggregate(int device, const int32_t* nbr, const float* el, const float* er, const float* feat, float* out, float* lse,
                              int64_t n_dst, int fanout, int heads, int dim, float negative_slope, void* stream) {
    return attention_launch<GatScore, false>(device, nullptr, nbr, fanout, el, er, feat, out, lse, n_dst, heads, dim, negative_slope, stream);
}

int coala_block_gat_aggregate_backward(int device, const int32_t* nbr, const float* el, const float* er, const float* feat, const float* out,
                                       const float* lse, const float* grad_out, float* grad_feat, float* grad_el, float* grad_er, int64_t n_dst,
                                       int fanout, int heads, int dim, float negative_slope, void* stream) {
    return gat_backward_launch<false>(device, nullptr, nbr, fanout, el, er, feat, out, lse, grad_out, grad_feat, grad_el, grad_er, n_dst, heads, dim,
                                      negative_slope, stream);
}

int coala_block_gat_aggregate_csr(int device, const int64_t* indptr, const int32_t* indices, const float* el, const float* er, const float* feat,
                                  float* out, float* lse, int64_t n_dst, int heads, int dim, float negative_slope, void* stream) {
    return attention_launch<GatScore, true>(device, indptr, indices, 0, el, er, feat, out, lse, n_dst, heads, dim, negative_slope, stream);
}

int coala_block_gat_aggregate_csr_backward(int device, const int64_t* indptr, const int32_t* indices, const float* el, const float* er,
                                           const float* feat, const float* out, const float* lse, const float* grad_out, float* grad_feat,
                                           float* grad_el, float* grad_er, int64_t n_dst, int heads, int dim, float negative_slope, void* stream) {
    return gat_backward_launch<true>(device, indptr, indices, 0, el, er, feat, out, lse, grad_out, grad_feat, grad_el, grad_er, n_dst, heads, dim,
                                     negative_slope, stream);
}

int coala_block_gatv2_aggregate(int device, const int32_t* nbr, const float* feat_src, const float* feat_dst, const float* attn, float* out,
                                float* lse, int64_t n_dst, int fanout, int heads, int dim, float negative_slope, void* stream) {
    return attention_launch<Gatv2Score, false>(device, nullptr, nbr, fanout, feat_src, feat_dst, attn, out, lse, n_dst, heads, dim, negative_slope, stream);
}

int coala_block_gatv2_aggregate_backward(int device, const int32_t* nbr, const float* feat_src, const float* feat_dst, const float* attn,
                                         const float* out, const float* lse, const float* grad_out, float* grad_src, float* grad_dst,
                                         float* grad_attn_parts, int parts, int64_t n_dst, int fanout, int heads, int dim, float negative_slope,
                                         void* stream) {
    return gatv2_backward_launch<false>(device, nullptr, nbr, fanout, feat_src, feat_dst, attn, out, lse, grad_out, grad_src, grad_dst,
                                        grad_attn_parts, parts, n_dst, heads, dim, negative_slope, stream);
}

int coala_block_gatv2_aggregate_csr(int device, const int64_t* indptr, const int32_t* indices, const float* feat_src, const float* feat_dst,
                                    const float* attn, float* out, float* lse, int64_t n_dst, int heads, int dim, float negative_slope,
                                    void* stream) {
    return attention_launch<Gatv2Score, true>(device, indptr, indices, 0, feat_src, feat_dst, attn, out, lse, n_dst, heads, dim, negative_slope, stream);
}

int coala_block_gatv2_aggregate_csr_backward(int device, const int64_t* indptr, const int32_t* indices, const float* feat_src,
                                             const float* feat_dst, const float* attn, const float* out, const float* lse, const float* grad_out,
                                             float* grad_src, float* grad_dst, float* grad_attn_parts, int parts, int64_t n_dst, int heads,
                                             int dim, float negative_slope, void* stream) {
    return gatv2_backward_launch<true>(device, indptr, indices, 0, feat_src, feat_dst, attn, out, lse, grad_out, grad_src, grad_dst,
                                       grad_attn_parts, parts, n_dst, heads, dim, negative_slope, stream);
}

int coala_block_dot_gat_aggregate(int device, const int32_t* row, const float* q, const float* k, const float* v, float* out, float* lse,
                                  int64_t n_dst, int fanout, int heads, int dim, float scale, void* stream) {
    return attention_launch<DotScore, false>(device, nullptr, row, fanout, q, k, v, out, lse, n_dst, heads, dim, scale, stream);
}

int coala_block_dot_gat_aggregate_backward(int device, const int32_t* row, const float* q, const float* k, const float* v, const float* out,
                                           const float* lse, const float* grad_out, float* grad_q, float* grad_k, float* grad_v, int64_t n_dst,
                                           int fanout, int heads, int dim, float scale, void* stream) {
    return dot_gat_backward_launch<false>(device, nullptr, row, fanout, q, k, v, out, lse, grad_out, grad_q, grad_k, grad_v, n_dst, heads, dim, scale,
                                          stream);
}

int coala_block_dot_gat_aggregate_csr(int device, const int64_t* indptr, const int32_t* row, const float* q, const float* k, const float* v,
                                      float* out, float* lse, int64_t n_dst, int heads, int dim, float scale, void* stream) {
    return attention_launch<DotScore, true>(device, indptr, row, 0, q, k, v, out, lse, n_dst, heads, dim, scale, stream);
}

int coala_block_dot_gat_aggregate_csr_backward(int device, const int64_t* indptr, const int32_t* row, const float* q, const float* k,
                                               const float* v, const float* out, const float* lse, const float* grad_out, float* grad_q,
                                               float* grad_k, float* grad_v, int64_t n_dst, int heads, int dim, float scale, void* stream) {
    return dot_gat_backward_launch<true>(device, indptr, row, 0, q, k, v, out, lse, grad_out, grad_q, grad_k, grad_v, n_dst, heads, dim, scale,
                                         stream);
}

int coala_block_weighted_sum(int device, const int32_t* nbr, const float* w, const float* h_src, float* out, int64_t n_dst, int fanout, int dim,
                             void* stream) {
    return weighted_sum_launch<false>(device, nullptr, nbr, w, fanout, h_src, out, n_dst, dim, stream);
}

int coala_block_weighted_sum_backward(int device, const int32_t* nbr, const float* w, const float* h_src, const float* grad_out, float* grad_src,
                                      float* grad_w, int64_t n_dst, int fanout, int dim, void* stream) {
    return weighted_sum_backward_launch<false>(device, nullptr, nbr, w, fanout, h_src, grad_out, grad_src, grad_w, n_dst, dim, stream);
}

int coala_block_weighted_sum_csr(int device, const int64_t* indptr, const int32_t* indices, const float* w, const float* h_src, float* out,
                                 int64_t n_dst, int dim, void* stream) {
    return weighted_sum_launch<true>(device, indptr, indices, w, 0, h_src, out, n_dst, dim, stream);
}

int coala_block_weighted_sum_csr_backward(int device, const int64_t* indptr, const int32_t* indices, const float* w, const float* h_src,
                                          const float* grad_out, float* grad_src, float* grad_w, int64_t n_dst, int dim, void* stream) {
    return weighted_sum_backward_launch<true>(device, indptr, indices, w, 0, h_src, grad_out, grad_src, grad_w, n_dst, dim, stream);
}

int coala_block_max_aggregate(int device, const int32_t* nbr, const float* h_src, float* out, int32_t* arg, int64_t n_dst, int fanout, int dim,
                              void* stream) {
    return max_launch<false>(device, nullptr, nbr, fanout, h_src, out, arg, n_dst, dim, stream);
}

int coala_block_max_aggregate_csr(int device, const int64_t* indptr, const int32_t* indices, const float* h_src, float* out, int32_t* arg,
                                  int64_t n_dst, int dim, void* stream) {
    return max_launch<true>(device, indptr, indices, 0, h_src, out, arg, n_dst, dim, stream);
}

int coala_block_max_aggregate_backward(int device, const int32_t* arg, const float* grad_out, float* grad_src, int64_t n_dst, int dim,
                                       void* stream) {
    return max_backward_launch(device, arg, grad_out, grad_src, n_dst, dim, stream);
}

int coala_block_rel_sum(int device, const int32_t* nbr, const int32_t* etype, const float* w, const float* h_src, float* out, int64_t n_dst,
                        int fanout, int num_rels, int dim, void* stream) {
    return rel_sum_launch<false>(device, nullptr, nbr, etype, w, fanout, h_src, out, n_dst, num_rels, dim, stream);
}

int coala_block_rel_sum_backward(int device, const int32_t* nbr, const int32_t* etype, const float* w, const float* h_src, const float* grad_out,
                                 float* grad_src, float* grad_w, int64_t n_dst, int fanout, int num_rels, int dim, void* stream) {
    return rel_sum_backward_launch<false>(device, nullptr, nbr, etype, w, fanout, h_src, grad_out, grad_src, grad_w, n_dst, num_rels, dim, stream);
}

int coala_block_rel_sum_csr(int device, const int64_t* indptr, const int32_t* indices, const int32_t* etype, const float* w, const float* h_src,
                            float* out, int64_t n_dst, int num_rels, int dim, void* stream) {
    return rel_sum_launch<true>(device, indptr, indices, etype, w, 0, h_src, out, n_dst, num_rels, dim, stream);
}

int coala_block_rel_sum_csr_backward(int device, const int64_t* indptr, const int32_t* indices, const int32_t* etype, const float* w,
                                     const float* h_src, const float* grad_out, float* grad_src, float* grad_w, int64_t n_dst, int num_rels,
                                     int dim, void* stream) {
    return rel_sum_backward_launch<true>(device, indptr, indices, etype, w, 0, h_src, grad_out, grad_src, grad_w, n_dst, num_rels, dim, stream);
}

int coala_block_rel_gat_aggregate(int device, const int32_t* row, const int32_t* etype, const float* el, const float* er, const float* feat,
                                  float* out, float* lse, int64_t n_dst, int fanout, int num_rels, int heads, int dim, float negative_slope,
                                  void* stream) {
    return rel_gat_launch<false>(device, nullptr, row, etype, fanout, el, er, feat, out, lse, n_dst, num_rels, heads, dim, negative_slope, stream);
}

int coala_block_rel_gat_aggregate_backward(int device, const int32_t* row, const int32_t* etype, const float* el, const float* er,
                                           const float* feat, const float* lse, const float* grad_out, float* grad_feat, float* grad_el,
                                           float* grad_er, int64_t n_dst, int fanout, int num_rels, int heads, int dim, float negative_slope,
                                           void* stream) {
    return rel_gat_backward_launch<false>(device, nullptr, row, etype, fanout, el, er, feat, lse, grad_out, grad_feat, grad_el, grad_er, n_dst,
                                          num_rels, heads, dim, negative_slope, stream);
}

int coala_block_rel_gat_aggregate_csr(int device, const int64_t* indptr, const int32_t* row, const int32_t* etype, const float* el,
                                      const float* er, const float* feat, float* out, float* lse, int64_t n_dst, int num_rels, int heads, int dim,
                                      float negative_slope, void* stream) {
    return rel_gat_launch<true>(device, indptr, row, etype, 0, el, er, feat, out, lse, n_dst, num_rels, heads, dim, negative_slope, stream);
}

int coala_block_rel_gat_aggregate_csr_backward(int device, const int64_t* indptr, const int32_t* row, const int32_t* etype, const float* el,
                                               const float* er, const float* feat, const float* lse, const float* grad_out, float* grad_feat,
                                               float* grad_el, float* grad_er, int64_t n_dst, int num_rels, int heads, int dim,
                                               float negative_slope, void* stream) {
    return rel_gat_backward_launch<true>(device, indptr, row, etype, 0, el, er, feat, lse, grad_out, grad_feat, grad_el, grad_er, n_dst, num_rels,
                                         heads, dim, negative_slope, stream);
}

int coala_block_exclude_edges(int device, const int32_t* nbr, const int64_t* eid, const int64_t* excluded, int64_t n_excluded, int32_t* nbr_out,
                              int64_t* eid_out, int64_t n_dst, int fanout, void* stream) {
    return exclude_launch(device, nbr, eid, fanout, excluded, n_excluded, nbr_out, eid_out, n_dst, stream);
}

int coala_block_exclude_edges_csr(int device, const int64_t* indptr, const int32_t* indices, const int64_t* eid, const int64_t* excluded,
                                  int64_t n_excluded, int64_t* counts_out, const int64_t* new_indptr, int32_t* indices_out, int64_t* eid_out,
                                  int64_t n_dst, void* stream) {
    return exclude_csr_launch(device, indptr, indices, eid, excluded, n_excluded, counts_out, new_indptr, indices_out, eid_out, n_dst, stream);
}

int coala_block_pair_dot(int device, const float* h, const int32_t* src, const int32_t* dst, float* out, int64_t n_pairs, int heads, int dim,
                         void* stream) {
    return pair_dot_launch(device, h, src, dst, nullptr, out, n_pairs, heads, dim, stream);
}

int coala_block_pair_dot_backward(int device, const float* h, const int32_t* src, const int32_t* dst, const float* grad_out, float* grad_h,
                                  int64_t n_pairs, int heads, int dim, void* stream) {
    if (n_pairs > 0 && !grad_out) return fail(COALA_EINVAL, "null buffer");
    return pair_dot_launch(device, h, src, dst, grad_out, grad_h, n_pairs, heads, dim, stream);
}

int coala_block_skipgram_loss(int device, const float* h, const int32_t* rows, float* partial, int32_t* count, int64_t n_rows, int len,
                              int context, int dim, float sign, void* stream) {
    return skipgram_launch(device, h, rows, partial, count, nullptr, nullptr, n_rows, len, context, dim, sign, stream);
}

int coala_block_skipgram_loss_backward(int device, const float* h, const int32_t* rows, double* grad_acc, const double* scale, int64_t n_rows,
                                       int len, int context, int dim, float sign, void* stream) {
    if (n_rows > 0 && !grad_acc) return fail(COALA_EINVAL, "null buffer");
    return skipgram_launch(device, h, rows, nullptr, nullptr, grad_acc, scale, n_rows, len, context, dim, sign, stream);
}

} // extern "C"
