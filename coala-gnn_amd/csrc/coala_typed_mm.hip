// coala_typed_mm.hip -- the typed linear step of the relation- and node-typed layers on the fp32 matrix units of gfx950 (DGL's
// gather_mm / segment_mm, dgl.nn.TypedLinear):  C[i] = A[g(i)] @ op(W[type_i]).  Stateless entry points, every launch on the caller's
// stream, no host read.
//
// Three steps, one C entry each:
//   plan        types (and rows, for the -1 rule) -> order int32 [M], the row indices grouped by type in list order, and seg int32
//               [T + 1], the groups' offsets; rows that send nothing lie behind seg[T].  Ballot ranks and prefix sums, no atomics:
//               count per 256-row wave tile, one-block column scan (coala_partition.h's), scatter.
//   product     one block per (type, 64-row tile, 128-column tile).  The tile's rows are gathered through order (and rows) straight
//               from A into LDS; no sorted copy of A exists.  The forward and grad_x are this one kernel: grad_x is the transposed
//               case on grad_y, stored directly or added with float atomics through rows.
//   grad_W      grad_W[t] = sum over the rows of type t of P[p(i)]^T (x) Q[q(i)]: the same matrix step with the segment's rows as the
//               reduction dimension, a segment cut into chunks of kChunk rows, one block per (type, chunk, 64 x 128 tile), added
//               with float atomics into a zeroed grad_W.
//
// The matrix step.  v_mfma_f32_32x32x2_f32: lane l holds a = A[l % 32][l / 32] and b = B[l / 32][l % 32] of a 32 x 2 by 2 x 32
// product and 16 accumulators, register r being C[8 (r / 4) + 4 (l / 32) + r % 4][l % 32].  A block of 4 waves holds a 64 x 128
// tile, wave w the rows 32 (w & 1) .. and the columns 64 (w >> 1) .. as two 32 x 32 accumulators that stay in registers over the whole
// reduction.  Both operands lie in LDS reduction-index-major, As[k][row] (row stride 68) and Bs[k][column] (row stride 132), 16
// reduction steps per tile, so a lane's operand read is 32 consecutive floats per half wave in every case: free of bank conflicts.
// A tile is filled either "direct" (a source row runs along the LDS row: W plain, and both operands of grad_W) or "transposing" (a
// source row runs along k: the gathered rows of A, and W transposed; thread t takes 4 consecutive k of source row t / 4, and with
// the strides 68 and 132, both 4 mod 16, its four scalar stores hit 64 different banks per wave).  Edges are zeros in LDS; nothing
// is read past a row's end.  16-byte loads are used when both operands' pointers and row lengths allow, 4-byte loads otherwise.
// The loads of reduction step k + 1 are issued into registers before the matrix instructions of step k.
//
// One output element is one chain of fused multiply-adds over k = 0, 1, 2, ... in that order (the padding adds +0 * 0), so the
// product's direct-store form is bitwise reproducible and an element's bits do not depend on which rows share its tile.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/coala_hip.h"
#include "coala_internal.h"
#include "coala_partition.h"

#define fail coala_fail_
#define HIPCHK COALA_HIPCHK

namespace {

constexpr int kTM = 64;      // rows of a tile (the gathered rows; in-features for grad_W)
constexpr int kTN = 128;     // columns of a tile
constexpr int kKS = 16;      // reduction steps per LDS tile
constexpr int kLDA = 68;     // LDS row strides: 4 mod 16 (see above), multiples of 4 for the 16-byte stores
constexpr int kLDB = 132;
constexpr int kChunk = 2048; // rows of a segment one grad_W block reduces
constexpr int kMaxTypes = 64;

typedef float floatx16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------------------------------------ plan
// bucket of list entry i: its type, or T for an entry that sends nothing
__device__ __forceinline__ int plan_bucket(const int32_t* __restrict__ types, const int32_t* __restrict__ rows, int64_t i, int T) {
    const int32_t t = types[i];
    return (t < 0 || t >= T || (rows && rows[i] < 0)) ? T : t;
}

// counts[tile * (T + 1) + g] = entries of bucket g in the wave tile; lane g counts bucket g, bucket T is counted by every lane
__global__ __launch_bounds__(kBlock) void plan_count_kernel(const int32_t* __restrict__ types, const int32_t* __restrict__ rows, int64_t M, int T,
                                                            uint32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t n_tiles = partition_tiles(M);
    for (int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * kWavesPerBlock) {
        uint32_t mine = 0, tail = 0;
        for (int j = 0; j < kPartItems; ++j) {
            const int64_t i = tile * kPartTile + j * 64 + lane;
            const int o = i < M ? plan_bucket(types, rows, i, T) : -1;
            for (int g = 0; g < T; ++g) {
                const uint64_t m = __ballot(o == g);
                if (lane == g) mine += (uint32_t)__builtin_popcountll(m);
            }
            tail += (uint32_t)__builtin_popcountll(__ballot(o == T));
        }
        if (lane < T) counts[tile * (T + 1) + lane] = mine;
        if (lane == 0) counts[tile * (T + 1) + T] = tail;
    }
}

// one block: counts becomes every tile's exclusive offset inside its bucket; seg[g] = the first slot of bucket g, g = 0 .. T
__global__ __launch_bounds__(kBlock) void plan_scan_kernel(uint32_t* __restrict__ counts, int64_t n_tiles, int T, int32_t* __restrict__ seg) {
    __shared__ int64_t totals[kMaxTypes + 1];
    partition_scan_columns(counts, n_tiles, (uint32_t)(T + 1), totals);
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int g = 0; g <= T; ++g) {
            seg[g] = (int32_t)run;
            run += totals[g];
        }
    }
}

__global__ __launch_bounds__(kBlock) void plan_scatter_kernel(const int32_t* __restrict__ types, const int32_t* __restrict__ rows, int64_t M, int T,
                                                              const uint32_t* __restrict__ offsets, const int32_t* __restrict__ seg,
                                                              int32_t* __restrict__ order) {
    const int lane = threadIdx.x & 63;
    const int64_t n_tiles = partition_tiles(M);
    const uint64_t below = (1ull << lane) - 1ull;
    for (int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * kWavesPerBlock) {
        int64_t off = 0; // lane g: the next free slot of bucket g for this tile
        if (lane < T) off = (int64_t)seg[lane] + offsets[tile * (T + 1) + lane];
        int64_t tail_off = (int64_t)seg[T] + offsets[tile * (T + 1) + T];
        for (int j = 0; j < kPartItems; ++j) {
            const int64_t i = tile * kPartTile + j * 64 + lane;
            const int o = i < M ? plan_bucket(types, rows, i, T) : -1;
            int64_t dest = -1;
            for (int g = 0; g < T; ++g) {
                const uint64_t m = __ballot(o == g);
                const int64_t bg = __shfl(off, g);
                if (o == g) dest = bg + __builtin_popcountll(m & below);
                if (lane == g) off += __builtin_popcountll(m);
            }
            const uint64_t m = __ballot(o == T);
            if (o == T) dest = tail_off + __builtin_popcountll(m & below);
            tail_off += __builtin_popcountll(m);
            if (i < M) order[dest] = (int32_t)i;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ tile fills
// four floats of a source row from column c on: zeros for a missing row (p == nullptr) and past the row's n columns
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ p, int c, int n) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!p) return v;
    if (VEC) {               // n % 4 == 0 and c % 4 == 0: in or out as a whole
        if (c < n) v = *reinterpret_cast<const float4*>(p + c);
    } else {
        if (c < n) v.x = p[c];
        if (c + 1 < n) v.y = p[c + 1];
        if (c + 2 < n) v.z = p[c + 2];
        if (c + 3 < n) v.w = p[c + 3];
    }
    return v;
}

// "direct" fill of a [kKS][W] tile: tile row r is the source row row(r) from column c0 on (n columns in all).  Thread t takes 4 columns
// of row t / (W / 4) (+ 256 / (W / 4) for the second pass of the wide tile): a source row is read in consecutive 16-byte pieces.
template <int W, bool VEC, class Row>
__device__ __forceinline__ void fetch_direct(float4 (&reg)[W / 64], const Row& row, int c0, int n) {
    constexpr int Q = W / 4, RP = kBlock / Q;
#pragma unroll
    for (int j = 0; j < W / 64; ++j) reg[j] = load4<VEC>(row((int)threadIdx.x / Q + j * RP), c0 + 4 * ((int)threadIdx.x % Q), n);
}

template <int W, int LD>
__device__ __forceinline__ void stash_direct(float* __restrict__ tile, const float4 (&reg)[W / 64]) {
    constexpr int Q = W / 4, RP = kBlock / Q;
#pragma unroll
    for (int j = 0; j < W / 64; ++j)
        *reinterpret_cast<float4*>(tile + ((int)threadIdx.x / Q + j * RP) * LD + 4 * ((int)threadIdx.x % Q)) = reg[j];
}

// "transposing" fill of a [kKS][R] tile: tile column r is the source row row(r), tile row k its column k0 + k (n columns in all).
// Thread t takes the columns k0 + 4 (t % 4) .. + 3 of row t / 4 (+ 64 for the wide tile): 64 consecutive bytes of a row per 4 lanes.
template <int R, bool VEC, class Row>
__device__ __forceinline__ void fetch_trans(float4 (&reg)[R / 64], const Row& row, int k0, int n) {
#pragma unroll
    for (int j = 0; j < R / 64; ++j) reg[j] = load4<VEC>(row((int)threadIdx.x / 4 + j * 64), k0 + 4 * ((int)threadIdx.x % 4), n);
}

template <int R, int LD>
__device__ __forceinline__ void stash_trans(float* __restrict__ tile, const float4 (&reg)[R / 64]) {
#pragma unroll
    for (int j = 0; j < R / 64; ++j) {
        float* d = tile + 4 * ((int)threadIdx.x % 4) * LD + (int)threadIdx.x / 4 + j * 64;
        d[0] = reg[j].x, d[LD] = reg[j].y, d[2 * LD] = reg[j].z, d[3 * LD] = reg[j].w;
    }
}

// the kKS reduction steps of one LDS tile pair on this wave's 32 x 64 part: k ascending, two k per instruction (lanes 0-31 the even)
__device__ __forceinline__ void mma_tile(const float* __restrict__ As, const float* __restrict__ Bs, int arow, int bcol, floatx16& acc0, floatx16& acc1) {
    const int lane = threadIdx.x & 63, l32 = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int kk = 0; kk < kKS / 2; ++kk) {
        const int k = 2 * kk + kh;
        const float a = As[k * kLDA + arow + l32];
        const float b0 = Bs[k * kLDB + bcol + l32], b1 = Bs[k * kLDB + bcol + 32 + l32];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
    }
}

// this lane's 2 x 16 accumulators: sink(tile row, tile column, value)
template <class Sink>
__device__ __forceinline__ void drain(const floatx16& acc0, const floatx16& acc1, int arow, int bcol, const Sink& sink) {
    const int lane = threadIdx.x & 63, l32 = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = arow + 8 * (r / 4) + 4 * kh + (r % 4);
        sink(i, bcol + l32, acc0[r]);
        sink(i, bcol + 32 + l32, acc1[r]);
    }
}

// the block's share of the segments: block b of the grid takes unit (b - units before segment t) of the first segment t whose units
// reach past b; a segment of c rows has ceil(c / per) units.  seg has `n_seg` segments, the last one ending at M.  -> false past the end
__device__ __forceinline__ bool find_unit(const int32_t* __restrict__ seg, int n_seg, int64_t M, int per, int64_t b, int* t_out, int64_t* beg, int64_t* end) {
    for (int t = 0; t < n_seg; ++t) {
        const int64_t s = seg[t], e = t + 1 < n_seg ? (int64_t)seg[t + 1] : M;
        const int64_t units = (e - s + per - 1) / per;
        if (b < units) {
            *t_out = t;
            *beg = s + b * per;
            *end = e < *beg + per ? e : *beg + per;
            return true;
        }
        b -= units;
    }
    return false;
}

// --------------------------------------------------------------------------------------------------------------------- product
// C[c(m)] (+)= A[a(m)] @ op(W[t]) for the rows m = order[p] of one 64-row tile of segment t and 128 columns from blockIdx.y * 128:
// a(m) = a_rows ? a_rows[m] : m, c(m) likewise with c_rows; with c_rows the sums are added with float atomics.  A is [., K], C is
// [., N]; W[t] is [K, N], or [N, K] with TRANS.  The segments are seg's T types and the tail [seg[T], M): its rows get zeros when
// they are stored directly and nothing when they are added.
template <bool TRANS, bool VEC>
__global__ __launch_bounds__(kBlock) void gather_mm_kernel(const float* __restrict__ A, const float* __restrict__ W, const int32_t* __restrict__ order,
                                                           const int32_t* __restrict__ seg, const int32_t* __restrict__ a_rows,
                                                           const int32_t* __restrict__ c_rows, float* __restrict__ C, int64_t M, int T, int K, int N) {
    __shared__ __attribute__((aligned(16))) float As[kKS * kLDA];
    __shared__ __attribute__((aligned(16))) float Bs[kKS * kLDB];
    __shared__ int32_t s_a[kTM], s_c[kTM];
    int t;
    int64_t beg, end;
    if (!find_unit(seg, T + 1, M, kTM, blockIdx.x, &t, &beg, &end)) return;
    const int n0 = blockIdx.y * kTN;
    if (t == T) { // rows that send nothing
        if (c_rows) return;
        for (int e = threadIdx.x; e < kTM * kTN; e += kBlock) {
            const int64_t p = beg + e / kTN;
            const int n = n0 + e % kTN;
            if (p < end && n < N) C[(int64_t)order[p] * N + n] = 0.0f;
        }
        return;
    }
    if (threadIdx.x < kTM) {
        const int64_t p = beg + threadIdx.x;
        const int32_t m = p < end ? order[p] : -1;
        s_a[threadIdx.x] = m < 0 ? -1 : (a_rows ? a_rows[m] : m);
        s_c[threadIdx.x] = m < 0 ? -1 : (c_rows ? c_rows[m] : m);
    }
    __syncthreads();
    const float* Wt = W + (int64_t)t * K * N;
    int k0 = 0;
    const auto a_row = [&](int r) -> const float* { return s_a[r] < 0 ? nullptr : A + (int64_t)s_a[r] * K; };
    const auto w_k = [&](int r) -> const float* { return k0 + r < K ? Wt + (int64_t)(k0 + r) * N : nullptr; };   // plain: tile row = W's row k
    const auto w_n = [&](int r) -> const float* { return n0 + r < N ? Wt + (int64_t)(n0 + r) * K : nullptr; };   // TRANS: tile column = W's row n
    float4 ra[1], rb[2];
    const auto fetch = [&]() {
        fetch_trans<kTM, VEC>(ra, a_row, k0, K);
        if (TRANS) fetch_trans<kTN, VEC>(rb, w_n, k0, K);
        else fetch_direct<kTN, VEC>(rb, w_k, n0, N);
    };
    const auto stash = [&]() {
        stash_trans<kTM, kLDA>(As, ra);
        if (TRANS) stash_trans<kTN, kLDB>(Bs, rb);
        else stash_direct<kTN, kLDB>(Bs, rb);
    };
    const int wave = threadIdx.x >> 6, arow = 32 * (wave & 1), bcol = 64 * (wave >> 1);
    floatx16 acc0 = {0}, acc1 = {0};
    fetch();
    stash();
    __syncthreads();
    while (true) {
        const bool more = k0 + kKS < K;
        if (more) {
            k0 += kKS;
            fetch();          // the next step's global loads fly under this step's matrix instructions
        }
        mma_tile(As, Bs, arow, bcol, acc0, acc1);
        if (!more) break;
        __syncthreads();
        stash();
        __syncthreads();
    }
    const bool add = c_rows != nullptr;
    drain(acc0, acc1, arow, bcol, [&](int i, int j, float v) {
        const int32_t ci = s_c[i];
        const int n = n0 + j;
        if (ci < 0 || n >= N) return;
        float* dst = C + (int64_t)ci * N + n;
        if (add) unsafeAtomicAdd(dst, v);
        else *dst = v;
    });
}

// ---------------------------------------------------------------------------------------------------------------------- grad_W
// GW[t][k][n] += sum over the rows m = order[p] of one kChunk-row chunk of segment t of P[p(m)][k] Q[q(m)][n], k in the 64-row tile
// blockIdx.y, n in the 128-column tile blockIdx.z; p(m) = p_rows ? p_rows[m] : m, q(m) likewise.  P is [., K], Q is [., N].
template <bool VEC>
__global__ __launch_bounds__(kBlock) void gather_mm_wgrad_kernel(const float* __restrict__ P, const int32_t* __restrict__ p_rows, const float* __restrict__ Q,
                                                                 const int32_t* __restrict__ q_rows, const int32_t* __restrict__ order,
                                                                 const int32_t* __restrict__ seg, float* __restrict__ GW, int64_t M, int T, int K, int N) {
    __shared__ __attribute__((aligned(16))) float As[kKS * kLDA];
    __shared__ __attribute__((aligned(16))) float Bs[kKS * kLDB];
    int t;
    int64_t beg, end;
    if (!find_unit(seg, T, seg[T], kChunk, blockIdx.x, &t, &beg, &end)) return;
    const int i0 = blockIdx.y * kTM, n0 = blockIdx.z * kTN;
    int64_t r0 = beg;
    const auto p_row = [&](int r) -> const float* {
        if (r0 + r >= end) return nullptr;
        const int32_t m = order[r0 + r];
        return P + (int64_t)(p_rows ? p_rows[m] : m) * K;
    };
    const auto q_row = [&](int r) -> const float* {
        if (r0 + r >= end) return nullptr;
        const int32_t m = order[r0 + r];
        return Q + (int64_t)(q_rows ? q_rows[m] : m) * N;
    };
    float4 ra[1], rb[2];
    const auto fetch = [&]() {
        fetch_direct<kTM, VEC>(ra, p_row, i0, K);
        fetch_direct<kTN, VEC>(rb, q_row, n0, N);
    };
    const auto stash = [&]() {
        stash_direct<kTM, kLDA>(As, ra);
        stash_direct<kTN, kLDB>(Bs, rb);
    };
    const int wave = threadIdx.x >> 6, arow = 32 * (wave & 1), bcol = 64 * (wave >> 1);
    floatx16 acc0 = {0}, acc1 = {0};
    fetch();
    stash();
    __syncthreads();
    while (true) {
        const bool more = r0 + kKS < end;
        if (more) {
            r0 += kKS;
            fetch();
        }
        mma_tile(As, Bs, arow, bcol, acc0, acc1);
        if (!more) break;
        __syncthreads();
        stash();
        __syncthreads();
    }
    float* G = GW + (int64_t)t * K * N;
    drain(acc0, acc1, arow, bcol, [&](int i, int j, float v) {
        if (i0 + i < K && n0 + j < N) unsafeAtomicAdd(G + (int64_t)(i0 + i) * N + n0 + j, v);
    });
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_shape(int64_t M, int T, int K, int N) {
    if (M < 0 || M > INT32_MAX || T < 1 || T > kMaxTypes || K < 1 || N < 1 || K > 65535 * kTM || N > 65535 * kTM)   // a grid's y and z hold 65535 tiles
        return fail(COALA_EINVAL, "bad typed product shape (types 1..%d, 1 <= in, out <= %d, 0 <= M < 2^31)", kMaxTypes, 65535 * kTM);
    return COALA_OK;
}

} // namespace

extern "C" {

int64_t coala_block_gather_mm_plan_work(int64_t M, int T) { return M <= 0 || T < 1 ? 0 : partition_tiles(M) * (T + 1); }

int coala_block_gather_mm_plan(int device, const int32_t* types, const int32_t* rows, int64_t M, int T, int32_t* order, int32_t* seg, int32_t* work,
                               void* stream) {
    if (int rc = check_shape(M, T, 1, 1)) return rc;
    if (M == 0) return COALA_OK;
    if (!types || !order || !seg || !work) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    const int64_t n_tiles = partition_tiles(M);
    const dim3 grid = partition_grid(n_tiles);
    uint32_t* counts = reinterpret_cast<uint32_t*>(work);
    hipLaunchKernelGGL(plan_count_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, types, rows, M, T, counts);
    hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, counts, n_tiles, T, seg);
    hipLaunchKernelGGL(plan_scatter_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, types, rows, M, T, (const uint32_t*)counts, (const int32_t*)seg, order);
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

int coala_block_gather_mm(int device, const float* a, const float* w, const int32_t* order, const int32_t* seg, const int32_t* a_rows,
                          const int32_t* c_rows, float* c, int64_t M, int T, int K, int N, int transposed, void* stream) {
    if (int rc = check_shape(M, T, K, N)) return rc;
    if (M == 0) return COALA_OK;
    if (!a || !w || !order || !seg || !c) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    // every segment, the tail included, ends in at most one ragged tile
    const dim3 grid((unsigned)(M / kTM + T + 1), (unsigned)((N + kTN - 1) / kTN));
    const bool vec = aligned16(a) && aligned16(w) && K % 4 == 0 && (transposed || N % 4 == 0);
#define COALA_GMM(TR, VE) \
    hipLaunchKernelGGL((gather_mm_kernel<TR, VE>), grid, dim3(kBlock), 0, (hipStream_t)stream, a, w, order, seg, a_rows, c_rows, c, M, T, K, N)
    if (transposed) {
        if (vec) COALA_GMM(true, true);
        else COALA_GMM(true, false);
    } else {
        if (vec) COALA_GMM(false, true);
        else COALA_GMM(false, false);
    }
#undef COALA_GMM
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

int coala_block_gather_mm_backward_w(int device, const float* p, const int32_t* p_rows, const float* q, const int32_t* q_rows, const int32_t* order,
                                     const int32_t* seg, float* grad_w, int64_t M, int T, int K, int N, void* stream) {
    if (int rc = check_shape(M, T, K, N)) return rc;
    if (M == 0) return COALA_OK;
    if (!p || !q || !order || !seg || !grad_w) return fail(COALA_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(device));
    const dim3 grid((unsigned)(M / kChunk + T), (unsigned)((K + kTM - 1) / kTM), (unsigned)((N + kTN - 1) / kTN));
    const bool vec = aligned16(p) && aligned16(q) && K % 4 == 0 && N % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(gather_mm_wgrad_kernel<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, p, p_rows, q, q_rows, order, seg, grad_w, M, T, K, N);
    else
        hipLaunchKernelGGL(gather_mm_wgrad_kernel<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, p, p_rows, q, q_rows, order, seg, grad_w, M, T, K, N);
    HIPCHK(hipGetLastError());
    return COALA_OK;
}

} // extern "C"
