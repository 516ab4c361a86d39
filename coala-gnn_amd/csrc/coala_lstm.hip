// coala_lstm.hip -- LSTM neighbour aggregation on a sampled block (DGL's SAGEConv 'lstm', PyG's LSTMAggregation) on the fp32 matrix
// units of gfx950.  Row d of the block starts from h = c = 0 and takes its valid slots in slot order; a step with source s is
//     z = xg[s] + h @ w_hh^T,   i, f, o = sigmoid(z_i, z_f, z_o),   g = tanh(z_g),   c = f c + i g,   h = o tanh(c),
// and the row's result is its last h.  xg [n_src, 4H] holds the input-side gate pre-activations of every SOURCE NODE (x @ W_ih^T + b_ih
// + b_hh, made once per node by the caller, torch's gate order i, f, g, o); w_hh is [4H, H].  Stateless entry points, every launch on the
// caller's stream, no host read.  Native range: H % 32 == 0, 32 <= H <= 256.
//
// Forward, one launch.  A block owns a tile of 32 destination rows and has H / 32 waves.  Wave w owns the hidden units [32 w, 32 w + 32)
// and holds all four gates of that slice as four 32 x 32 accumulators of v_mfma_f32_32x32x2_f32 (lane l: a = A[l % 32][l / 32], b =
// B[l / 32][l % 32]; accumulator register r is C[8 (r / 4) + 4 (l / 32) + r % 4][l % 32], see coala_typed_mm.hip), so a lane has the i, f,
// g and o of the same 16 (row, unit) pairs and the cell update is local to it: c and the lane's copy of h never leave registers.  The
// h of the tile, the A operand of every wave, lies in LDS unit-major (hs[u][row], row stride 40) and is double-buffered: a step reads
// the old h while every wave writes its slice of the new one; one barrier per step, which also tells the block whether any row goes
// on (__syncthreads_or).  The accumulators start from 0 and xg[s] of each row's current slot, gathered straight into the accumulator
// layout (a half wave reads 128 consecutive bytes), is added once behind the product: started FROM xg[s] the chain rounds every
// one of its H / 2 steps at the magnitude of z instead of that of the partial product, which measured 2 to 3 times the error of a
// library GEMM followed by one addition (out 2.0e-07 against 1.0e-07, grad_xg 8.6e-07 against 2.8e-07 at H = 96).  w_hh streams from L2 every step (256 KB at H = 128: it does not fit LDS): a lane reads
// 16 bytes along k of its own row of w_hh per gate and 8 reduction steps; to let it use them the lane halves split each 8 steps as
// k = 8 c + {0..3} (lanes 0-31) and 8 c + {4..7} (lanes 32-63).  The first step of a tile, where every h is 0, skips the product.  The
// rows of a tile are aligned at their first slot; lanes 0-31 of wave 0 each walk one row's slots (-1 entries are skipped wherever
// they stand) and post the next step's source and slot position in LDS; a row whose slots are used up keeps h and c, and the tile
// runs to its longest row.  Every output element is one chain of fused multiply-adds over k in a fixed order, plus xg[s]: the
// forward is bitwise reproducible, the same in both block forms and independent of the other rows of the tile.  With gates != NULL the
// forward stores per live slot the activated gates [S, 4H] and c [S, H] (S = slots of the block: n_dst * fanout, or indptr[n_dst]).
//
// Backward, one launch, same tiling, the rows aligned at their LAST slot and walked in reverse.  dh and dc of a (row, unit) pair stay
// in the registers of the lane that owns it: the product below leaves dh in the very layout the cell step reads.  A step forms the
// pre-activation gradients dz [32, 4H] from the saved gates and c, writes them over the saved gates in place, adds them into
// grad_xg[s] with float atomics (a lane per float: a half wave covers 128 consecutive bytes; the mapping of rel_sum_backward) and to
// LDS k-major (dzs[n][row], row stride 32, 128 KB at H = 256); then dh_{t-1} = dz @ w_hh on the matrix units, reduction length 4H,
// two interleaved accumulators, w_hh read row-wise (128 consecutive bytes per half wave).  It also leaves h_prev [S, H], the h each
// slot started from (recomputed as o tanh(c) of the slot before), and zeroes the dz and h_prev rows of -1 slots, so that
// grad_w_hh = dz^T @ h_prev is ONE dense GEMM over the two buffers for the caller.  Two barriers per step (dzs is single-buffered).
//
// A hub row of a ragged block is walked serially by its tile; splitting it is not done.
//
// hipcc -O3 for gfx950 reports: forward 158 VGPRs, no AGPRs, no scratch, 3 waves per SIMD, 1 KB static + 320 H bytes dynamic LDS (80 KB
// at H = 256); backward 110 VGPRs, no scratch, 4 waves per SIMD, 2 KB static + 512 H bytes dynamic LDS (128 KB at H = 256, which is
// why dzs has row stride 32 and one buffer).  Above 48 KB the launch raises the kernel's dynamic LDS limit first.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/coala_hip.h"
#include "coala_internal.h"

#define fail coala_fail_
#define HIPCHK COALA_HIPCHK

namespace {

constexpr int kTile = 32;        // destination rows of a tile
constexpr int kLDH = 40;         // row stride of the forward's hs[u][row]: the two lane halves, 4 rows of hs apart, read disjoint banks
constexpr int kMinH = 32, kMaxH = 256;
constexpr int kMaxThreads = 64 * (kMaxH / 32);

typedef float floatx16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float sigmoid_(float x) { return 1.0f / (1.0f + expf(-x)); }   // expf(-x) = inf gives 0: no NaN at any x

// tile row of accumulator register r in a lane of the upper (kh = 1) or lower half wave
__device__ __forceinline__ int acc_row(int r, int kh) { return 8 * (r >> 2) + 4 * kh + (r & 3); }

template <bool CSR>
__device__ __forceinline__ void tile_row_range(const int64_t* indptr, int fanout, int64_t d, int64_t n_dst, int64_t* beg, int64_t* end) {
    *beg = *end = 0;
    if (d < n_dst) {
        *beg = CSR ? indptr[d] : d * fanout;
        *end = CSR ? indptr[d + 1] : *beg + fanout;
    }
}

template <bool VEC>
__device__ __forceinline__ float4 load_w4(const float* p) {
    if (VEC) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

// ------------------------------------------------------------------------------------------------------------------------ forward
template <bool CSR, bool VEC>
__global__ __launch_bounds__(kMaxThreads) void lstm_forward_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, int fanout,
                                                                   const float* __restrict__ xg, const float* __restrict__ w_hh,
                                                                   float* __restrict__ out, float* __restrict__ gates, float* __restrict__ cell,
                                                                   int64_t n_dst, int H) {
    extern __shared__ __attribute__((aligned(16))) float hs[];   // [2][H][kLDH]
    __shared__ int32_t s_src[2][kTile];                          // the step's source of every tile row, -1: the row rests
    __shared__ int64_t s_pos[2][kTile];                          // and its slot position
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, kh = lane >> 5;
    const int64_t d0 = (int64_t)blockIdx.x * kTile;
    const int u = 32 * wave + l32;                               // this lane's hidden unit
    const int64_t G = 4 * (int64_t)H;

    int64_t e = 0, end = 0;                                      // lanes 0-31 of wave 0: the cursor of tile row tid
    int32_t s = -1;
    const bool walker = tid < kTile;
    if (walker) {
        tile_row_range<CSR>(indptr, fanout, d0 + tid, n_dst, &e, &end);
        while (e < end && (s = idx[e]) < 0) ++e;
        if (e >= end) s = -1;
        s_src[0][tid] = s;
        s_pos[0][tid] = e;
    }
    int any = __syncthreads_or(walker && s >= 0);

    floatx16 h = {0}, c = {0};
    int cur = 0;
    for (int t = 0; any; ++t) {
        const float* hc = hs + cur * H * kLDH;
        float* hn = hs + (cur ^ 1) * H * kLDH;
        floatx16 acc[4] = {{0}, {0}, {0}, {0}};
        if (t > 0) {                                             // the first step's h is 0 in every row
            const float* w = w_hh + (int64_t)u * H + 4 * kh;     // gate g: + g * H * H
            const int64_t HH = (int64_t)H * H;
            for (int k0 = 0; k0 < H; k0 += 8) {
                float4 b[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) b[g] = load_w4<VEC>(w + g * HH + k0);
                const float* a = hc + (k0 + 4 * kh) * kLDH + l32;
                const float a0 = a[0], a1 = a[kLDH], a2 = a[2 * kLDH], a3 = a[3 * kLDH];
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[g].x, acc[g], 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[g].y, acc[g], 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b[g].z, acc[g], 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b[g].w, acc[g], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, kh);
            const int32_t sr = s_src[cur][row];
            if (sr >= 0) {
                const float* x = xg + (int64_t)sr * G + u;       // gathered straight into the accumulator layout
                const float gi = sigmoid_(x[0] + acc[0][r]), gf = sigmoid_(x[H] + acc[1][r]);
                const float gg = tanhf(x[2 * H] + acc[2][r]), go = sigmoid_(x[3 * H] + acc[3][r]);
                c[r] = __builtin_fmaf(gf, c[r], gi * gg);
                h[r] = go * tanhf(c[r]);
                if (gates) {
                    const int64_t p = s_pos[cur][row];
                    float* gp = gates + p * G + u;
                    gp[0] = gi, gp[H] = gf, gp[2 * H] = gg, gp[3 * H] = go;
                    cell[p * H + u] = c[r];
                }
            }
            hn[u * kLDH + row] = h[r];
        }
        bool more = false;
        if (walker) {
            if (s >= 0) ++e;
            while (e < end && (s = idx[e]) < 0) ++e;
            if (e >= end) s = -1;
            s_src[cur ^ 1][tid] = s;
            s_pos[cur ^ 1][tid] = e;
            more = s >= 0;
        }
        any = __syncthreads_or(more);
        cur ^= 1;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t d = d0 + acc_row(r, kh);
        if (d < n_dst) out[d * H + u] = h[r];
    }
}

// ----------------------------------------------------------------------------------------------------------------------- backward
template <bool CSR>
__global__ __launch_bounds__(kMaxThreads) void lstm_backward_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, int fanout,
                                                                    const float* __restrict__ w_hh, const float* __restrict__ grad_out,
                                                                    float* __restrict__ gates, const float* __restrict__ cell,
                                                                    float* __restrict__ h_prev, float* __restrict__ grad_xg, int64_t n_dst, int H) {
    extern __shared__ __attribute__((aligned(16))) float dzs[];  // [4H][kTile]
    __shared__ int64_t s_e[2][3][kTile];                         // per tile row: the slot after the step's (0), the step's (1), the one before (2); -1: none
    __shared__ int32_t s_src[2][kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6, l32 = lane & 31, kh = lane >> 5;
    const int64_t d0 = (int64_t)blockIdx.x * kTile;
    const int u = 32 * wave + l32;
    const int64_t G = 4 * (int64_t)H;

    // the dz and h_prev rows of -1 slots: zeros, for the caller's dz^T @ h_prev.  A wave per row, 64 slots at a time.
    for (int row = wave; row < kTile; row += n_waves) {
        int64_t beg, end;
        tile_row_range<CSR>(indptr, fanout, d0 + row, n_dst, &beg, &end);
        for (int64_t e0 = beg; e0 < end; e0 += 64) {
            uint64_t pad = __ballot(e0 + lane < end && idx[e0 + lane] < 0);
            while (pad) {
                const int64_t p = e0 + __builtin_ctzll(pad);
                pad &= pad - 1;
                for (int i = lane; i < G; i += 64) gates[p * G + i] = 0.0f;
                if (h_prev)
                    for (int i = lane; i < H; i += 64) h_prev[p * H + i] = 0.0f;
            }
        }
    }

    int64_t beg = 0, ec = -1, ep = -1;                           // lanes 0-31 of wave 0: the cursor of tile row tid, walking down
    const bool walker = tid < kTile;
    if (walker) {
        int64_t end;
        tile_row_range<CSR>(indptr, fanout, d0 + tid, n_dst, &beg, &end);
        ec = end - 1;
        while (ec >= beg && idx[ec] < 0) --ec;
        if (ec < beg) ec = -1;
        ep = ec < 0 ? -1 : ec - 1;
        while (ep >= beg && idx[ep] < 0) --ep;
        if (ep < beg) ep = -1;
        s_e[0][0][tid] = -1, s_e[0][1][tid] = ec, s_e[0][2][tid] = ep;
        s_src[0][tid] = ec < 0 ? -1 : idx[ec];
    }
    floatx16 dh, dc = {0};
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t d = d0 + acc_row(r, kh);
        dh[r] = d < n_dst ? grad_out[d * H + u] : 0.0f;
    }
    int any = __syncthreads_or(walker && ec >= 0);

    int cur = 0;
    while (any) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, kh);
            const int64_t p = s_e[cur][1][row];
            float di = 0.0f, df = 0.0f, dg = 0.0f, dout = 0.0f;
            if (p >= 0) {
                const int64_t pn = s_e[cur][0][row], pp = s_e[cur][2][row];
                float* gp = gates + p * G + u;
                const float gi = gp[0], gf = gp[H], gg = gp[2 * H], go = gp[3 * H];
                const float cp = pp >= 0 ? cell[pp * H + u] : 0.0f;
                const float tc = tanhf(cell[p * H + u]);
                if (h_prev) {
                    if (pn >= 0) h_prev[pn * H + u] = go * tc;   // what the slot after this one started from
                    if (pp < 0) h_prev[p * H + u] = 0.0f;        // the row's first slot starts from 0
                }
                dout = dh[r] * tc * go * (1.0f - go);
                const float dcr = __builtin_fmaf(dh[r] * go, 1.0f - tc * tc, dc[r]);
                di = dcr * gg * gi * (1.0f - gi);
                dg = dcr * gi * (1.0f - gg * gg);
                df = dcr * cp * gf * (1.0f - gf);
                dc[r] = dcr * gf;
                gp[0] = di, gp[H] = df, gp[2 * H] = dg, gp[3 * H] = dout;
                if (grad_xg) {
                    float* gx = grad_xg + (int64_t)s_src[cur][row] * G + u;
                    unsafeAtomicAdd(gx, di);
                    unsafeAtomicAdd(gx + H, df);
                    unsafeAtomicAdd(gx + 2 * H, dg);
                    unsafeAtomicAdd(gx + 3 * H, dout);
                }
            }
            dzs[u * kTile + row] = di;
            dzs[(H + u) * kTile + row] = df;
            dzs[(2 * H + u) * kTile + row] = dg;
            dzs[(3 * H + u) * kTile + row] = dout;
        }
        bool more = false;
        if (walker) {
            const int64_t en = ec;
            ec = ep;
            ep = ec < 0 ? -1 : ec - 1;
            while (ep >= beg && idx[ep] < 0) --ep;
            if (ep < beg) ep = -1;
            s_e[cur ^ 1][0][tid] = en, s_e[cur ^ 1][1][tid] = ec, s_e[cur ^ 1][2][tid] = ep;
            s_src[cur ^ 1][tid] = ec < 0 ? -1 : idx[ec];
            more = ec >= 0;
        }
        any = __syncthreads_or(more);
        if (!any) break;                                         // no row has a slot before this one: its dh is not needed
        floatx16 acc0 = {0}, acc1 = {0};
        const float* a = dzs + kh * kTile + l32;
        const float* b = w_hh + (int64_t)kh * H + u;
        for (int k = 0; k < 4 * H; k += 4) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k * kTile], b[(int64_t)k * H], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[(k + 2) * kTile], b[(int64_t)(k + 2) * H], acc1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (s_e[cur ^ 1][1][acc_row(r, kh)] >= 0) dh[r] = acc0[r] + acc1[r];
        __syncthreads();                                         // dzs is read out before the next step writes it
        cur ^= 1;
    }
}

// ------------------------------------------------------------------------------------------------------------------------- launch
int check_shape(int64_t n_dst, int fanout, bool csr, int H) {
    if (H < kMinH || H > kMaxH || H % 32 != 0)
        return fail(COALA_EINVAL, "bad lstm hidden size %d (a multiple of 32 in %d..%d)", H, kMinH, kMaxH);
    if (n_dst < 0 || (n_dst + kTile - 1) / kTile > INT32_MAX) return fail(COALA_EINVAL, "bad lstm block: n_dst %lld", (long long)n_dst);
    if (!csr && (fanout < 1 || fanout > 32)) return fail(COALA_EINVAL, "bad lstm block: fan-out %d (1..32)", fanout);
    return COALA_OK;
}

// a kernel that asks for more than the default 64 KB of dynamic LDS has to be told so once per call
template <class K>
int allow_lds(K kernel, size_t bytes) {
    if (bytes > 48 * 1024) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return COALA_OK;
}

template <bool CSR>
int forward_launch(int device, const int64_t* indptr, const int32_t* idx, int fanout, const float* xg, const float* w_hh, float* out, float* gates,
                   float* cell, int64_t n_dst, int H, void* stream) {
    if (int rc = check_shape(n_dst, fanout, CSR, H)) return rc;
    if (!idx || (CSR && !indptr) || !xg || !w_hh || !out || (gates == nullptr) != (cell == nullptr))
        return fail(COALA_EINVAL, "null buffer (gates and cell: both or neither)");
    if (n_dst == 0) return COALA_OK;
    HIPCHK(hipSetDevice(device));
    const dim3 grid((unsigned)((n_dst + kTile - 1) / kTile)), block(64 * (H / 32));
    const size_t lds = 2 * (size_t)H * kLDH * sizeof(float);
    const bool vec = ((uintptr_t)w_hh & 15) == 0;
    auto kernel = vec ? lstm_forward_kernel<CSR, true> : lstm_forward_kernel<CSR, false>;
    if (int rc = allow_lds(kernel, lds)) return rc;
    hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)stream, indptr, idx, fanout, xg, w_hh, out, gates, cell, n_dst, H);
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

template <bool CSR>
int backward_launch(int device, const int64_t* indptr, const int32_t* idx, int fanout, const float* w_hh, const float* grad_out, float* gates,
                    const float* cell, float* h_prev, float* grad_xg, int64_t n_dst, int H, void* stream) {
    if (int rc = check_shape(n_dst, fanout, CSR, H)) return rc;
    if (!idx || (CSR && !indptr) || !w_hh || !grad_out || !gates || !cell) return fail(COALA_EINVAL, "null buffer");
    if (n_dst == 0) return COALA_OK;
    HIPCHK(hipSetDevice(device));
    const dim3 grid((unsigned)((n_dst + kTile - 1) / kTile)), block(64 * (H / 32));
    const size_t lds = 4 * (size_t)H * kTile * sizeof(float);
    if (int rc = allow_lds(lstm_backward_kernel<CSR>, lds)) return rc;
    hipLaunchKernelGGL(lstm_backward_kernel<CSR>, grid, block, lds, (hipStream_t)stream, indptr, idx, fanout, w_hh, grad_out, gates, cell, h_prev,
                       grad_xg, n_dst, H);
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

} // namespace

extern "C" {

int coala_block_lstm_aggregate(int device, const int32_t* nbr, const float* xg, const float* w_hh, float* out, float* gates, float* cell,
                               int64_t n_dst, int fanout, int hidden, void* stream) {
    return forward_launch<false>(device, nullptr, nbr, fanout, xg, w_hh, out, gates, cell, n_dst, hidden, stream);
}

int coala_block_lstm_aggregate_csr(int device, const int64_t* indptr, const int32_t* indices, const float* xg, const float* w_hh, float* out,
                                   float* gates, float* cell, int64_t n_dst, int hidden, void* stream) {
    return forward_launch<true>(device, indptr, indices, 0, xg, w_hh, out, gates, cell, n_dst, hidden, stream);
}

int coala_block_lstm_aggregate_backward(int device, const int32_t* nbr, const float* w_hh, const float* grad_out, float* gates, const float* cell,
                                        float* h_prev, float* grad_xg, int64_t n_dst, int fanout, int hidden, void* stream) {
    return backward_launch<false>(device, nullptr, nbr, fanout, w_hh, grad_out, gates, cell, h_prev, grad_xg, n_dst, hidden, stream);
}

int coala_block_lstm_aggregate_backward_csr(int device, const int64_t* indptr, const int32_t* indices, const float* w_hh, const float* grad_out,
                                            float* gates, const float* cell, float* h_prev, float* grad_xg, int64_t n_dst, int hidden,
                                            void* stream) {
    return backward_launch<true>(device, indptr, indices, 0, w_hh, grad_out, gates, cell, h_prev, grad_xg, n_dst, hidden, stream);
}

} // extern "C"
