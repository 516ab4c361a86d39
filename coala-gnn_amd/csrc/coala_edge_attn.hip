// coala_edge_attn.hip -- dot-product attention on a sampled block whose edges carry a feature row (PyG's TransformerConv(edge_dim=), TGN's
// raw messages), for gfx950, forward and backward, on fixed blocks of any fan-out and on the CSR blocks of full layers.  With the edge
// projection W_e added to the key and to the value of every edge,
//   <q, k_s + W_e x_j> = <q, k_s> + <W_e^T q, x_j>        sum_j a_j (v_s + W_e x_j) = sum_j a_j v_s + W_e sum_j a_j x_j,
// so the per-edge work is on the raw F-float edge row x_j and nothing of shape [E, H, D] exists: the caller brings qe[d, h] = W_e[h]^T q[d, h]
// and takes eagg[d, h] = sum_j a_j x_j back.  For dst d, head h and the slots j of d that hold an edge (source s_j):
//   e_j = scale (<q[d, h, :], k[s_j, h, :]> + <qe[d, h, :], x_j>),  a_j = softmax of e over the row,
//   out[d, h, :] = sum_j a_j v[s_j, h, :],  eagg[d, h, :] = sum_j a_j x_j.
// x_j = efeat[eids_j] with an id per slot (int32 or int64, read as it is), or efeat's row of the slot itself.
//
// One wave per destination row, rows dealt by a grid-stride loop, a row walked in chunks of 64 slots with the online softmax of the
// dot-product kernels (running max and sum per head, the partial sums rescaled when the max grows).  Every row takes that one path: a
// chunk without an edge leaves max, sum and partial sums as they are (the rescale factor is exactly 1), so a ragged row and the same row
// padded with -1 to any fan-out give the same bits.  What is new is the edge row: it is data, so it cannot be recomputed per lane as a
// time encoding can, and its two sums want opposite lane mappings --
//   score  <qe[d, h], x_j>: a lane per slot, t in the loop, qe[d, h, t] wave-uniform (scalar loads), one fma per head into registers;
//   eagg / grad_qe / grad_x: a lane per channel t, the slots in the loop, the [slot][head] weights from LDS, x_j[t] a coalesced read
// -- neither reduces across lanes.  The score's mapping reads a row per lane, which from memory would be 64 strided streams: the rows are
// staged instead, a lane per channel (each row one coalesced F-float read), into LDS as [slot][F | 1].  The odd row stride makes the
// lane-per-slot reader conflict-free (lane j reads word j * stride + t), the lane-per-channel reader and the writer touch consecutive
// words.  A wave's stage is kStageFloats = 64 * 17 floats: a whole chunk for F <= 16, which the lane-per-channel pass then reads from
// LDS too (the rows come from memory once per chunk); a wider row is staged kStageFloats / (F | 1) slots at a time (8 at F = 128) for the
// score, and the lane-per-channel pass reads it from memory a second time, coalesced (once per pass).
//
// The helpers of coala_block_ops.hip that a row walk needs (which rows a wave takes, the 64-index chunk load, the wave reductions, the
// segmented per-head sum, the softmax steps, the rounded scale product) are duplicated here, with the LDS [slot][head] arrays at a
// stride of HB | 1 words instead of 16: that file is left as it is, so its kernels compile to the code they had.
// No matrix instructions: per destination this is matrix-vector work (one q against a row's k, one qe against a row's x).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/coala_hip.h"
#include "coala_internal.h"

#define fail coala_fail_
#define HIPCHK COALA_HIPCHK

namespace {

constexpr int kMaxHeads = 16, kMaxEdgeDim = 128;
constexpr int kStageFloats = 64 * 17; // a wave's stage of edge rows
constexpr int kMaxGrid = 2048;        // blocks: 8192 rows a pass of the grid
constexpr float kNegInf = -__builtin_inff();

struct WaveRows {
    int lane;
    int64_t wave, n_waves;
};

__device__ __forceinline__ WaveRows wave_rows() {
    return {(int)(threadIdx.x & 63), (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), (int64_t)gridDim.x * kWavesPerBlock};
}

template <bool CSR>
__device__ __forceinline__ void row_range(const int64_t* indptr, int fanout, int64_t d, int64_t* beg, int64_t* end) {
    *beg = CSR ? indptr[d] : d * fanout;
    *end = CSR ? indptr[d + 1] : *beg + fanout;
}

// lane j takes idx[e0 + j] into *mine, -1 past the row's end; -> the chunk's length
__device__ __forceinline__ int load_chunk(const int32_t* idx, int64_t e0, int64_t end, int lane, int32_t* mine) {
    *mine = e0 + lane < end ? idx[e0 + lane] : -1;
    return end - e0 < 64 ? (int)(end - e0) : 64;
}

// The edge row of the slot at e: efeat's row eids[e], or row e without ids; -1 where the slot holds no edge (ids are not read there).
__device__ __forceinline__ int64_t slot_edge_row(const void* eids, int eid_is_64, int64_t e, bool valid) {
    if (!valid) return -1;
    if (!eids) return e;
    return eid_is_64 ? static_cast<const int64_t*>(eids)[e] : (int64_t) static_cast<const int32_t*>(eids)[e];
}

__device__ __forceinline__ void wave_lds_sync() { // LDS written by some lanes of a wave, read by others
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

// x is the same in every lane: say so, and what it addresses is read by scalar loads.
__device__ __forceinline__ int64_t wave_uniform(int64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// One rounded product, never contracted into the subtraction that follows it: the backward's e_j is the forward's bit for bit.
__device__ __forceinline__ float dot_score(float scale, float qk) {
#pragma clang fp contract(off)
    return scale * qk;
}

__device__ __forceinline__ float normalised(float a, float sum) { return sum > 0.0f ? a / sum : 0.0f; }

// acc[h] += the sum of x over the lanes of head h, for the 64 floats c0 + lane of a [H * dim] row: a segmented inclusive scan, then the
// last lane of each head's segment adds its total.  Every lane must call it.
__device__ __forceinline__ void head_segment_add(float* acc, float x, int lane, int c0, int dim, int hd) {
    const int c = c0 + lane;
    const int h = c < hd ? c / dim : 0;
    const int start = c < hd ? max(h * dim - c0, 0) : hd - c0;
    for (int o = 1; o < 64; o <<= 1) {
        const float y = __shfl_up(x, o);
        if (lane - o >= start) x += y;
    }
    if (c < hd && (lane == 63 || c + 1 == hd || (c + 1) % dim == 0)) acc[h] += x;
}

// gout[h] += <g[h, :], o[h, :]> for the heads of one [H * dim] row, in a fixed order.  Every lane must call it.
__device__ __forceinline__ void head_dots(float* gout, const float* __restrict__ g, const float* __restrict__ o, int lane, int dim, int hd) {
    for (int c0 = 0; c0 < hd; c0 += 64) {
        const int c = c0 + lane;
        head_segment_add(gout, c < hd ? g[c] * o[c] : 0.0f, lane, c0, dim, hd);
    }
}

// w[j * HS + h] = <q[d, h, :], k[s_j, h, :]> for the n slots of a chunk, with DOT also dot[..] = <g[h, :], v[s_j, h, :]>: lane j zeroes
// slot j's words, then a lane per float of the [H * D] row, 64 at a time, the per-head sums by head_segment_add.  The caller has
// synchronised: the previous chunk's readers of w / dot are done.
template <int HS, bool DOT>
__device__ __forceinline__ void node_score_pass(float* w, float* dot, int32_t mine, int n, const float* __restrict__ k, const float* __restrict__ qd,
                                                const float* __restrict__ v, const float* __restrict__ g, int lane, int heads, int hd, int dim) {
    for (int h = 0; h < heads; ++h) {
        w[lane * HS + h] = 0.0f;
        if (DOT) dot[lane * HS + h] = 0.0f;
    }
    wave_lds_sync();
    for (int c0 = 0; c0 < hd; c0 += 64) { // wave-uniform trip count: head_segment_add shuffles across every lane
        const int c = c0 + lane;
        const bool in = c < hd;
        const float qc = in ? qd[c] : 0.0f;
        const float gc = DOT && in ? g[c] : 0.0f;
        for (int j = 0; j < n; ++j) {
            const int32_t s = __shfl(mine, j);
            if (s < 0) continue; // wave-uniform
            head_segment_add(w + j * HS, in ? qc * k[(int64_t)s * hd + c] : 0.0f, lane, c0, dim, hd);
            if (DOT) head_segment_add(dot + j * HS, in ? gc * v[(int64_t)s * hd + c] : 0.0f, lane, c0, dim, hd);
        }
    }
    wave_lds_sync();
}

// Eight channels t0 .. t0 + 7 of a lane's staged row x against the wave-uniform rows qr and gr ([H, F], scalar loads): per head the eight
// products are summed in fp32 from zero (one fma per term), and that block sum is added to te[h] in fp64, to tr[h] in fp32.  FULL: all
// eight channels exist; otherwise nt < 8 do and the others are neither read nor added.
template <int HB, bool DOT, bool FULL>
__device__ __forceinline__ void edge_dot_block(double (&te)[HB], float (&tr)[HB], const float* x, const float* __restrict__ qr,
                                               const float* __restrict__ gr, int nt, int heads, int F) {
    float xv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) xv[i] = FULL || i < nt ? x[i] : 0.0f;
#pragma unroll
    for (int h = 0; h < HB; ++h) {
        if (h < heads) { // wave-uniform
            float pq = 0.0f, pg = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (FULL || i < nt) { // wave-uniform
                    pq = __builtin_fmaf(qr[h * F + i], xv[i], pq);
                    if (DOT) pg = __builtin_fmaf(gr[h * F + i], xv[i], pg);
                }
            }
            te[h] += (double)pq;
            if (DOT) tr[h] += pg;
        }
    }
}

// The edge part of a chunk's scores, a lane per slot: te[h] = <qe_row[h, :], x_lane>, with DOT also tr[h] = <ge_row[h, :], x_lane>.  The
// score goes through an exponential, and a chain of F fp32 additions at the sum's own size would be its largest error: te is summed in
// blocks of eight channels (edge_dot_block), the block sums added in fp64 and the total rounded to fp32 once -- the same order forward
// and backward, so the backward's te is the forward's bit for bit.  The rows go through the stage `depth` slots at a time: a lane per
// channel reads a row (coalesced) and writes stage[slot * stride + t]; then the lanes of those slots read their rows back.  qe_row and
// ge_row are wave-uniform: scalar loads.  -> whether the whole chunk is in the stage when this returns (row j at stage + j * stride, for
// the slots with an edge), which holds until the next call.  Every lane must call it.
template <int HB, bool DOT>
__device__ __forceinline__ bool edge_score_pass(float (&te)[HB], float (&tr)[HB], float* stage, const float* __restrict__ efeat, int64_t xrow,
                                                int n, const float* __restrict__ qe_row, const float* __restrict__ ge_row, int heads, int F,
                                                int stride, int depth, int lane) {
    double te64[HB];
#pragma unroll
    for (int h = 0; h < HB; ++h) te64[h] = 0.0, tr[h] = 0.0f;
    for (int s0 = 0; s0 < n; s0 += depth) { // wave-uniform
        const int cnt = n - s0 < depth ? n - s0 : depth;
        wave_lds_sync(); // the stage's readers are done
        for (int jj = 0; jj < cnt; ++jj) {
            const int64_t r = __shfl(xrow, s0 + jj);
            if (r < 0) continue; // wave-uniform
            for (int t = lane; t < F; t += 64) stage[jj * stride + t] = efeat[r * F + t];
        }
        wave_lds_sync();
        const int jj = lane - s0;
        if (jj >= 0 && jj < cnt && xrow >= 0) {
            const float* x = stage + jj * stride;
            int t0 = 0;
            for (; t0 + 8 <= F; t0 += 8) edge_dot_block<HB, DOT, true>(te64, tr, x + t0, qe_row + t0, ge_row + t0, 8, heads, F);
            if (t0 < F) edge_dot_block<HB, DOT, false>(te64, tr, x + t0, qe_row + t0, ge_row + t0, F - t0, heads, F);
        }
    }
#pragma unroll
    for (int h = 0; h < HB; ++h) te[h] = (float)te64[h];
    return n <= depth;
}

// A wave's softmax state in LDS: w [64][HS] (exp(e_j - m) of the chunk, [slot][head]), and per head the running max, the running sum and
// the chunk's rescale factor.
struct SoftmaxLds {
    float *w, *m_run, *l_run, *scl;
};

// One head's step of the online softmax over a chunk: lane j brings slot j's score e (-inf and !valid: no edge) and leaves
// p_j = exp(e - m) in w; lane 0 updates the head's running max and sum and stores the factor that rescales the earlier chunks' sums (1
// exactly when the max did not move: a chunk without an edge changes nothing).  Every lane must call it.
template <int HS>
__device__ __forceinline__ void softmax_chunk_step(const SoftmaxLds& s, int h, float e, bool valid, int lane) {
    const float mo = s.m_run[h];
    const float mn = fmaxf(mo, wave_max(e));
    const float p = valid ? expf(e - mn) : 0.0f;
    const float sum = wave_sum(p);
    const float sc = mo == mn ? 1.0f : (mo == kNegInf ? 0.0f : expf(mo - mn));
    s.w[lane * HS + h] = p;
    if (lane == 0) {
        s.m_run[h] = mn;
        s.l_run[h] = s.l_run[h] * sc + sum;
        s.scl[h] = sc;
    }
}

// out_row[h, :] = (first chunk ? 0 : out_row[h, :] * scl[h]) + sum over the chunk's edges j of w[j][h] * v[s_j, h, :], divided by the
// row's sum on the last chunk: a lane per VEC floats of the [H * dim] row; the partial sum waits in out_row between chunks.
template <int VEC, int HS>
__device__ __forceinline__ void value_accumulate(const SoftmaxLds& s, float* out_row, const float* __restrict__ v, int32_t mine, int n, bool first,
                                                 bool last, int lane, int hd, int units, int upl) {
    typedef float vf __attribute__((ext_vector_type(VEC)));
    for (int u0 = 0; u0 < units; u0 += 64) { // wave-uniform trip counts: the shuffles below need every lane
        const int u = u0 + lane;
        const int hu = u < units ? u / upl : 0;
        float* o = out_row + (int64_t)u * VEC;
        vf acc = vf(0.0f);
        if (!first && u < units) acc = *reinterpret_cast<const vf*>(o) * s.scl[hu];
        for (int j = 0; j < n; ++j) {
            const int32_t src = __shfl(mine, j);
            if (src >= 0 && u < units) acc += s.w[j * HS + hu] * *reinterpret_cast<const vf*>(v + (int64_t)src * hd + (int64_t)u * VEC);
        }
        if (u < units) {
            if (last) acc *= s.l_run[hu] > 0.0f ? 1.0f / s.l_run[hu] : 0.0f;
            *reinterpret_cast<vf*>(o) = acc;
        }
    }
}

// eagg_row[h, t] likewise over the chunk's edge rows: a lane per channel t, an accumulator per head, x_j[t] from the stage when the
// chunk is resident there and from memory (coalesced) otherwise.
template <int HB, int HS>
__device__ __forceinline__ void edge_accumulate(const SoftmaxLds& s, float* eagg_row, const float* stage, bool resident,
                                                const float* __restrict__ efeat, int64_t xrow, int n, bool first, bool last, int lane, int heads,
                                                int F, int stride) {
    for (int t0 = 0; t0 < F; t0 += 64) { // wave-uniform trip count
        const int t = t0 + lane;
        const bool in = t < F;
        float acc[HB];
#pragma unroll
        for (int h = 0; h < HB; ++h) acc[h] = !first && in && h < heads ? eagg_row[h * F + t] * s.scl[h] : 0.0f;
        for (int j = 0; j < n; ++j) {
            const int64_t r = __shfl(xrow, j);
            if (r < 0) continue; // wave-uniform
            const float x = in ? (resident ? stage[j * stride + t] : efeat[r * F + t]) : 0.0f;
#pragma unroll
            for (int h = 0; h < HB; ++h)
                if (h < heads) acc[h] = __builtin_fmaf(s.w[j * HS + h], x, acc[h]);
        }
#pragma unroll
        for (int h = 0; h < HB; ++h) {
            if (h < heads && in) {
                if (last) acc[h] *= s.l_run[h] > 0.0f ? 1.0f / s.l_run[h] : 0.0f;
                eagg_row[h * F + t] = acc[h];
            }
        }
    }
}

// HB: the head count rounded up to 1, 2, 4, 8 or 16, the length of the per-head register arrays; the LDS [slot][head] arrays have rows
// of HS = HB | 1 words (an odd stride: the lane-per-slot accesses spread over the banks).
template <int HB, int VEC, bool CSR>
__global__ __launch_bounds__(kBlock) void edge_attn_aggregate_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, int fanout,
                                                                     const void* __restrict__ eids, int eid_is_64, const float* __restrict__ q,
                                                                     const float* __restrict__ k, const float* __restrict__ v,
                                                                     const float* __restrict__ qe, const float* __restrict__ efeat,
                                                                     float* __restrict__ out, float* __restrict__ eagg, float* __restrict__ lse,
                                                                     int64_t n_dst, int heads, int dim, int F, float scale) {
    constexpr int HS = HB | 1;
    __shared__ float w_lds[kWavesPerBlock][64 * HS];
    __shared__ float st_lds[kWavesPerBlock][3 * HB];
    __shared__ float x_lds[kWavesPerBlock][kStageFloats];
    const auto [lane, wave, n_waves] = wave_rows();
    const int wv = threadIdx.x >> 6;
    const SoftmaxLds s = {w_lds[wv], st_lds[wv], st_lds[wv] + HB, st_lds[wv] + 2 * HB};
    float* stage = x_lds[wv];
    const int hd = heads * dim, hf = heads * F, units = hd / VEC, upl = dim / VEC;
    const int stride = F | 1, depth = kStageFloats / stride < 64 ? kStageFloats / stride : 64;
    for (int64_t d0 = wave; d0 < n_dst; d0 += n_waves) {
        const int64_t d = wave_uniform(d0);
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        wave_lds_sync(); // the previous row has read m_run / l_run
        if (lane < heads) {
            s.m_run[lane] = kNegInf;
            s.l_run[lane] = 0.0f;
        }
        for (int64_t e0 = beg; e0 < end; e0 += 64) { // wave-uniform trip counts: the shuffles below need every lane
            int32_t mine;
            const int n = load_chunk(idx, e0, end, lane, &mine);
            const int64_t xrow = slot_edge_row(eids, eid_is_64, e0 + lane, mine >= 0);
            wave_lds_sync(); // the previous chunk has read w and scl; m_run / l_run are set
            node_score_pass<HS, false>(s.w, nullptr, mine, n, k, q + d * hd, nullptr, nullptr, lane, heads, hd, dim);
            float te[HB], unused[HB];
            const bool resident = edge_score_pass<HB, false>(te, unused, stage, efeat, xrow, n, qe + d * hf, nullptr, heads, F, stride, depth, lane);
#pragma unroll
            for (int h = 0; h < HB; ++h) {
                if (h < heads) // wave-uniform: softmax_chunk_step shuffles across every lane
                    softmax_chunk_step<HS>(s, h, mine >= 0 ? dot_score(scale, s.w[lane * HS + h] + te[h]) : kNegInf, mine >= 0, lane);
            }
            wave_lds_sync();
            const bool first = e0 == beg, last = e0 + 64 >= end;
            value_accumulate<VEC, HS>(s, out + d * hd, v, mine, n, first, last, lane, hd, units, upl);
            edge_accumulate<HB, HS>(s, eagg + d * hf, stage, resident, efeat, xrow, n, first, last, lane, heads, F, stride);
        }
        if (beg == end) { // no chunk ran: an empty CSR row
            for (int c = lane; c < hd; c += 64) out[d * hd + c] = 0.0f;
            for (int c = lane; c < hf; c += 64) eagg[d * hf + c] = 0.0f;
        }
        wave_lds_sync();
        if (lane < heads) lse[d * heads + lane] = s.l_run[lane] > 0.0f ? s.m_run[lane] + logf(s.l_run[lane]) : kNegInf;
    }
}

// Backward, every gradient in one launch, each of them optional (null).  Per row: gout[h] = <g_out[h], out[d, h]> + <g_eagg[h], eagg[d, h]>;
// a row of several chunks first walks its scores once for S[h] = sum_j exp(e_j - lse[d, h]), chunk after chunk in a fixed order (a row of
// one chunk takes S from the chunk in registers; a chunk without an edge adds exactly 0, so both block forms give the same S).  Then per
// chunk the two score passes run again, now also summing <g_out, v_j> and <g_eagg, x_j>, and per slot and head
//   a_j = exp(e_j - lse[d, h]) / S,   ds_j = a_j (<g_out, v_j> + <g_eagg, x_j> - gout[h]).
// The node walk is the dot-product backward's, a lane per float c of the [H * D] row:
//   grad_v[s_j, c] += a_j g_out[d, c]   grad_k[s_j, c] += scale ds_j q[d, c]   (float atomics)   grad_q[d, c] = scale sum_j ds_j k[s_j, c]
// and the edge walk takes a lane per channel t over the chunk's slots, x_j[t] from the stage or from memory as in the forward:
//   grad_qe[d, h, t] = scale sum_j ds_j[h] x_j[t]                                 an accumulator per head;
//   grad_x_j[t] = sum_h (scale ds_j[h] qe[d, h, t] + a_j[h] g_eagg[d, h, t])      stored at the slot's own row without ids (0 in a slot
//                                                                                 without an edge), a float atomic at row eids_j with them.
// grad_q and grad_qe are summed in slot order and stored once per chunk (a later chunk adds to what the earlier ones stored): no atomics.
template <int HB, bool CSR>
__global__ __launch_bounds__(kBlock) void edge_attn_aggregate_backward_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, int fanout, const void* __restrict__ eids, int eid_is_64,
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const float* __restrict__ qe,
    const float* __restrict__ efeat, const float* __restrict__ out, const float* __restrict__ eagg, const float* __restrict__ lse,
    const float* __restrict__ grad_out, const float* __restrict__ grad_eagg, float* __restrict__ grad_q, float* __restrict__ grad_k,
    float* __restrict__ grad_v, float* __restrict__ grad_qe, float* __restrict__ grad_efeat, int64_t n_dst, int heads, int dim, int F,
    float scale) {
    constexpr int HS = HB | 1;
    __shared__ float w_lds[kWavesPerBlock][64 * HS];   // the chunk's <q, k_j>, then a_j, [slot][head]
    __shared__ float dot_lds[kWavesPerBlock][64 * HS]; // <g_out, v_j>, then ds_j, [slot][head]
    __shared__ float hs_lds[kWavesPerBlock][2 * HB];   // per head: gout, S of a row of several chunks
    __shared__ float x_lds[kWavesPerBlock][kStageFloats];
    const auto [lane, wave, n_waves] = wave_rows();
    const int wv = threadIdx.x >> 6;
    float* w = w_lds[wv];
    float* dot = dot_lds[wv];
    float* gout = hs_lds[wv];
    float* ssum = gout + HB;
    float* stage = x_lds[wv];
    const int hd = heads * dim, hf = heads * F;
    const int stride = F | 1, depth = kStageFloats / stride < 64 ? kStageFloats / stride : 64;
    for (int64_t d0 = wave; d0 < n_dst; d0 += n_waves) {
        const int64_t d = wave_uniform(d0);
        int64_t beg, end;
        row_range<CSR>(indptr, fanout, d, &beg, &end);
        const float* g = grad_out + d * hd;
        const float* ge = grad_eagg + d * hf;
        const float* qd = q + d * hd;
        const float* qed = qe + d * hf;
        wave_lds_sync(); // the previous row has read gout and ssum
        if (lane < heads) gout[lane] = ssum[lane] = 0.0f;
        wave_lds_sync();
        head_dots(gout, g, out + d * hd, lane, dim, hd);
        wave_lds_sync();
        head_dots(gout, ge, eagg + d * hf, lane, F, hf);
        const bool one = end - beg <= 64; // wave-uniform: the row is one chunk
        if (!one) {
            for (int64_t e0 = beg; e0 < end; e0 += 64) {
                int32_t mine;
                const int n = load_chunk(idx, e0, end, lane, &mine);
                const int64_t xrow = slot_edge_row(eids, eid_is_64, e0 + lane, mine >= 0);
                wave_lds_sync(); // the previous chunk has read w
                node_score_pass<HS, false>(w, nullptr, mine, n, k, qd, nullptr, nullptr, lane, heads, hd, dim);
                float te[HB], unused[HB];
                edge_score_pass<HB, false>(te, unused, stage, efeat, xrow, n, qed, nullptr, heads, F, stride, depth, lane);
#pragma unroll
                for (int h = 0; h < HB; ++h) {
                    if (h < heads) { // wave-uniform: wave_sum shuffles across every lane
                        const float sum = wave_sum(mine >= 0 ? expf(dot_score(scale, w[lane * HS + h] + te[h]) - lse[d * heads + h]) : 0.0f);
                        if (lane == 0) ssum[h] += sum;
                    }
                }
            }
        }
        wave_lds_sync();
        for (int64_t e0 = beg; e0 < end; e0 += 64) { // wave-uniform trip counts
            int32_t mine;
            const int n = load_chunk(idx, e0, end, lane, &mine);
            const int64_t xrow = slot_edge_row(eids, eid_is_64, e0 + lane, mine >= 0);
            const bool first = e0 == beg;
            wave_lds_sync(); // the previous chunk has read w and dot
            node_score_pass<HS, true>(w, dot, mine, n, k, qd, v, g, lane, heads, hd, dim);
            float te[HB], tr[HB];
            const bool resident = edge_score_pass<HB, true>(te, tr, stage, efeat, xrow, n, qed, ge, heads, F, stride, depth, lane);
#pragma unroll
            for (int h = 0; h < HB; ++h) { // lane j reads and rewrites only slot j's words
                if (h < heads) {           // wave-uniform: wave_sum shuffles across every lane
                    float a = 0.0f, t = 0.0f;
                    if (mine >= 0) a = expf(dot_score(scale, w[lane * HS + h] + te[h]) - lse[d * heads + h]);
                    a = normalised(a, one ? wave_sum(a) : ssum[h]);
                    if (mine >= 0) t = a * (dot[lane * HS + h] + tr[h] - gout[h]);
                    w[lane * HS + h] = a;
                    dot[lane * HS + h] = t;
                }
            }
            wave_lds_sync();
            if (grad_q || grad_k || grad_v) { // grid-uniform
                for (int c0 = 0; c0 < hd; c0 += 64) { // wave-uniform trip count: the shuffles below need every lane
                    const int c = c0 + lane;
                    const bool in = c < hd;
                    const int hc = in ? c / dim : 0;
                    const float gc = in ? g[c] : 0.0f;
                    const float qc = in ? qd[c] : 0.0f;
                    float gq = 0.0f;
                    for (int j = 0; j < n; ++j) {
                        const int32_t src = __shfl(mine, j);
                        if (src >= 0 && in) { // every lane takes the shuffle above
                            const float tj = dot[j * HS + hc];
                            if (grad_v) unsafeAtomicAdd(grad_v + (int64_t)src * hd + c, w[j * HS + hc] * gc);
                            if (grad_k) unsafeAtomicAdd(grad_k + (int64_t)src * hd + c, scale * tj * qc);
                            if (grad_q) gq = __builtin_fmaf(tj, k[(int64_t)src * hd + c], gq);
                        }
                    }
                    if (in && grad_q) grad_q[d * hd + c] = first ? scale * gq : grad_q[d * hd + c] + scale * gq;
                }
            }
            if (!grad_qe && !grad_efeat) continue; // grid-uniform
            for (int t0 = 0; t0 < F; t0 += 64) {   // wave-uniform trip count
                const int t = t0 + lane;
                const bool in = t < F;
                float qer[HB], ger[HB], gq[HB];
#pragma unroll
                for (int h = 0; h < HB; ++h) {
                    qer[h] = in && h < heads ? scale * qed[h * F + t] : 0.0f;
                    ger[h] = in && h < heads ? ge[h * F + t] : 0.0f;
                    gq[h] = 0.0f;
                }
                for (int j = 0; j < n; ++j) {
                    const int64_t r = __shfl(xrow, j);
                    if (r < 0) { // wave-uniform; without ids the slot's own row takes a zero
                        if (grad_efeat && !eids && in) grad_efeat[(e0 + j) * F + t] = 0.0f;
                        continue;
                    }
                    const float x = in ? (resident ? stage[j * stride + t] : efeat[r * F + t]) : 0.0f;
                    float gx = 0.0f;
#pragma unroll
                    for (int h = 0; h < HB; ++h) {
                        if (h < heads) {
                            const float tj = dot[j * HS + h];
                            gq[h] = __builtin_fmaf(tj, x, gq[h]);
                            gx = __builtin_fmaf(tj, qer[h], __builtin_fmaf(w[j * HS + h], ger[h], gx));
                        }
                    }
                    if (grad_efeat && in) {
                        if (eids) unsafeAtomicAdd(grad_efeat + r * F + t, gx);
                        else grad_efeat[r * F + t] = gx;
                    }
                }
                if (grad_qe) {
#pragma unroll
                    for (int h = 0; h < HB; ++h)
                        if (h < heads && in) grad_qe[d * hf + h * F + t] = first ? scale * gq[h] : grad_qe[d * hf + h * F + t] + scale * gq[h];
                }
            }
        }
        if (beg == end) { // no chunk ran: an empty CSR row
            if (grad_q)
                for (int c = lane; c < hd; c += 64) grad_q[d * hd + c] = 0.0f;
            if (grad_qe)
                for (int c = lane; c < hf; c += 64) grad_qe[d * hf + c] = 0.0f;
        }
    }
}

// 16-B accesses need a row length of whole float4s and both row arrays on a 16-B boundary
bool vec4_ok(int dim, const void* a, const void* b) {
    return dim % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0;
}

// f(std::integral_constant<int, HB>): the instantiation for `heads` heads
template <typename F>
void dispatch_heads(int heads, F&& f) {
    if (heads <= 1) f(std::integral_constant<int, 1>{});
    else if (heads <= 2) f(std::integral_constant<int, 2>{});
    else if (heads <= 4) f(std::integral_constant<int, 4>{});
    else if (heads <= 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

template <bool CSR>
int shape_check(int64_t n_dst, int fanout, int heads, int dim, int edge_dim) {
    if (!CSR && fanout < 1) return fail(COALA_EINVAL, "bad block shape (fan-out >= 1)");
    if (n_dst < 0 || heads < 1 || heads > kMaxHeads || dim < 1 || (int64_t)heads * dim > INT32_MAX || edge_dim < 1 || edge_dim > kMaxEdgeDim)
        return fail(COALA_EINVAL, "bad block shape (heads 1..%d, dim >= 1, edge_dim 1..%d, n_dst >= 0)", kMaxHeads, kMaxEdgeDim);
    return COALA_OK;
}

// The checks of every launch in the order of the other block ops: the shape, then n_dst == 0 is done, then the null buffers.
template <bool CSR>
int forward_launch(int device, const int64_t* indptr, const int32_t* idx, int fanout, const void* eids, int eid_is_64, const float* q,
                   const float* k, const float* v, const float* qe, const float* efeat, float* out, float* eagg, float* lse, int64_t n_dst,
                   int heads, int dim, int edge_dim, float scale, void* stream) {
    if (int rc = shape_check<CSR>(n_dst, fanout, heads, dim, edge_dim)) return rc;
    if (n_dst == 0) return COALA_OK;
    if ((CSR && !indptr) || !idx || !q || !k || !v || !qe || !efeat || !out || !eagg || !lse) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    const dim3 grid(grid1d(n_dst * 64, kBlock, kMaxGrid));
    dispatch_heads(heads, [&](auto hb) {
        auto launch = [&](auto vec) {
            hipLaunchKernelGGL((edge_attn_aggregate_kernel<decltype(hb)::value, decltype(vec)::value, CSR>), grid, dim3(kBlock), 0,
                               (hipStream_t)stream, indptr, idx, fanout, eids, eid_is_64, q, k, v, qe, efeat, out, eagg, lse, n_dst, heads, dim,
                               edge_dim, scale);
        };
        if (vec4_ok(dim, v, out)) launch(std::integral_constant<int, 4>{});
        else launch(std::integral_constant<int, 1>{});
    });
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

template <bool CSR>
int backward_launch(int device, const int64_t* indptr, const int32_t* idx, int fanout, const void* eids, int eid_is_64, const float* q,
                    const float* k, const float* v, const float* qe, const float* efeat, const float* out, const float* eagg, const float* lse,
                    const float* grad_out, const float* grad_eagg, float* grad_q, float* grad_k, float* grad_v, float* grad_qe, float* grad_efeat,
                    int64_t n_dst, int heads, int dim, int edge_dim, float scale, void* stream) {
    if (int rc = shape_check<CSR>(n_dst, fanout, heads, dim, edge_dim)) return rc;
    if (n_dst == 0 || (!grad_q && !grad_k && !grad_v && !grad_qe && !grad_efeat)) return COALA_OK;
    if ((CSR && !indptr) || !idx || !q || !k || !v || !qe || !efeat || !out || !eagg || !lse || !grad_out || !grad_eagg)
        return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    const dim3 grid(grid1d(n_dst * 64, kBlock, kMaxGrid));
    dispatch_heads(heads, [&](auto hb) {
        hipLaunchKernelGGL((edge_attn_aggregate_backward_kernel<decltype(hb)::value, CSR>), grid, dim3(kBlock), 0, (hipStream_t)stream, indptr, idx,
                           fanout, eids, eid_is_64, q, k, v, qe, efeat, out, eagg, lse, grad_out, grad_eagg, grad_q, grad_k, grad_v, grad_qe,
                           grad_efeat, n_dst, heads, dim, edge_dim, scale);
    });
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

} // namespace

extern "C" {

int coala_block_edge_attn_aggregate(int device, const int32_t* nbr, const void* eids, int eid_is_64, const float* q, const float* k,
                                    const float* v, const float* qe, const float* efeat, float* out, float* eagg, float* lse, int64_t n_dst,
                                    int fanout, int heads, int dim, int edge_dim, float scale, void* stream) {
    return forward_launch<false>(device, nullptr, nbr, fanout, eids, eid_is_64, q, k, v, qe, efeat, out, eagg, lse, n_dst, heads, dim, edge_dim,
                                 scale, stream);
}

int coala_block_edge_attn_aggregate_backward(int device, const int32_t* nbr, const void* eids, int eid_is_64, const float* q, const float* k,
                                             const float* v, const float* qe, const float* efeat, const float* out, const float* eagg,
                                             const float* lse, const float* grad_out, const float* grad_eagg, float* grad_q, float* grad_k,
                                             float* grad_v, float* grad_qe, float* grad_efeat, int64_t n_dst, int fanout, int heads, int dim,
                                             int edge_dim, float scale, void* stream) {
    return backward_launch<false>(device, nullptr, nbr, fanout, eids, eid_is_64, q, k, v, qe, efeat, out, eagg, lse, grad_out, grad_eagg, grad_q,
                                  grad_k, grad_v, grad_qe, grad_efeat, n_dst, heads, dim, edge_dim, scale, stream);
}

int coala_block_edge_attn_aggregate_csr(int device, const int64_t* indptr, const int32_t* indices, const void* eids, int eid_is_64,
                                        const float* q, const float* k, const float* v, const float* qe, const float* efeat, float* out,
                                        float* eagg, float* lse, int64_t n_dst, int heads, int dim, int edge_dim, float scale, void* stream) {
    return forward_launch<true>(device, indptr, indices, 0, eids, eid_is_64, q, k, v, qe, efeat, out, eagg, lse, n_dst, heads, dim, edge_dim,
                                scale, stream);
}

int coala_block_edge_attn_aggregate_csr_backward(int device, const int64_t* indptr, const int32_t* indices, const void* eids, int eid_is_64,
                                                 const float* q, const float* k, const float* v, const float* qe, const float* efeat,
                                                 const float* out, const float* eagg, const float* lse, const float* grad_out,
                                                 const float* grad_eagg, float* grad_q, float* grad_k, float* grad_v, float* grad_qe,
                                                 float* grad_efeat, int64_t n_dst, int heads, int dim, int edge_dim, float scale, void* stream) {
    return backward_launch<true>(device, indptr, indices, 0, eids, eid_is_64, q, k, v, qe, efeat, out, eagg, lse, grad_out, grad_eagg, grad_q,
                                 grad_k, grad_v, grad_qe, grad_efeat, n_dst, heads, dim, edge_dim, scale, stream);
}

} // extern "C"
