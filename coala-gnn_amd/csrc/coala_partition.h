// coala_partition.h -- stable partition of an id list by owner = id % n_parts, shared by coala_cache.hip (coala_cache_route) and
// coala_sampler.hip (owner bucketing of the input nodes).  Not part of the ABI.  Wave ballots + prefix sums instead of atomics
// (cache_kernel.cu:79-91, :4-17), so the slot order inside a bucket is the list order on every run.  Three launches: count (lane g of a wave
// counts owner g over the wave's tile), scan (one block: per owner an exclusive scan over the tiles, then totals and bases), scatter (ballot
// ranks).  Here: owner_of, the tile constants and the per-tile __device__ bodies, once.  Each caller has thin __global__ shells of its own
// over them (the route takes n by value, the sampler reads it from the device): profiles/r26_owner_partition.txt.
#ifndef COALA_PARTITION_H
#define COALA_PARTITION_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coala_internal.h"

namespace {

constexpr int kPartItems = 4;               // ids per lane
constexpr int kPartTile = 64 * kPartItems;  // ids per wave tile
constexpr int kMaxParts = 64;               // one lane per owner

__device__ __forceinline__ uint32_t owner_of(uint64_t id, uint32_t n_parts, int pshift) {
    if (pshift >= 0) return (uint32_t)id & (n_parts - 1);
    if ((id >> 32) == 0) return (uint32_t)id % n_parts;
    return (uint32_t)(id % n_parts);
}

__host__ __device__ constexpr int64_t partition_tiles(int64_t n) { return (n + kPartTile - 1) / kPartTile; }

// count, one wave tile: lane g counts owner g, wave_counts[tile * P + g] is stored
__device__ __forceinline__ void partition_count_tile(const int64_t* __restrict__ ids, int64_t n, int64_t tile, uint32_t P, int pshift,
                                                     uint32_t* __restrict__ wave_counts) {
    const int lane = threadIdx.x & 63;
    uint32_t mine = 0; // lane g accumulates the count of owner g
    for (int j = 0; j < kPartItems; ++j) {
        const int64_t i = tile * kPartTile + j * 64 + lane;
        const uint32_t o = (i < n) ? owner_of((uint64_t)ids[i], P, pshift) : 0xFFFFFFFFu;
        for (uint32_t g = 0; g < P; ++g) {
            const uint64_t m = __ballot(o == g);
            if ((uint32_t)lane == g) mine += (uint32_t)__builtin_popcountll(m);
        }
    }
    if ((uint32_t)lane < P) wave_counts[tile * P + lane] = mine;
}

// scan, the whole (single) block: one wave per owner column (looping when there are more owners than waves), wave-level exclusive scan of
// wave_counts over the tiles with a running carry; totals[g] = size of bucket g, visible to every thread on return
__device__ __forceinline__ void partition_scan_columns(uint32_t* __restrict__ wave_counts, int64_t n_tiles, uint32_t P, int64_t* totals) {
    const int lane = threadIdx.x & 63;
    for (uint32_t g = threadIdx.x >> 6; g < P; g += blockDim.x >> 6) {
        uint32_t carry = 0;
        for (int64_t t0 = 0; t0 < n_tiles; t0 += 64) {
            const int64_t t = t0 + lane;
            const uint32_t c = (t < n_tiles) ? wave_counts[t * P + g] : 0u;
            uint32_t incl = c;
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t v = __shfl_up(incl, off);
                if (lane >= off) incl += v;
            }
            if (t < n_tiles) wave_counts[t * P + g] = carry + incl - c; // exclusive offset of this tile inside bucket g
            carry += __shfl(incl, 63);
        }
        if (lane == 0) totals[g] = (int64_t)carry;
    }
    __syncthreads();
}

// scatter, one wave tile: sink(dest, i, id) for every id = ids[i] of the tile, dest its slot in the partitioned list
template <class Sink>
__device__ __forceinline__ void partition_scatter_tile(const int64_t* __restrict__ ids, int64_t n, int64_t tile, uint32_t P, int pshift,
                                                       const uint32_t* __restrict__ wave_offsets, const int64_t* __restrict__ bases, const Sink& sink) {
    const int lane = threadIdx.x & 63;
    int64_t off = 0; // lane g: next free slot of bucket g for this wave tile
    if ((uint32_t)lane < P) off = bases[lane] + (int64_t)wave_offsets[tile * P + lane];
    for (int j = 0; j < kPartItems; ++j) {
        const int64_t i = tile * kPartTile + j * 64 + lane;
        const bool valid = i < n;
        const int64_t id = valid ? ids[i] : 0;
        const uint32_t o = valid ? owner_of((uint64_t)id, P, pshift) : 0xFFFFFFFFu;
        int64_t dest = -1;
        for (uint32_t g = 0; g < P; ++g) {
            const uint64_t m = __ballot(o == g);
            const int64_t bg = __shfl(off, (int)g);
            if (o == g) dest = bg + __builtin_popcountll(m & ((1ull << lane) - 1ull));
            if ((uint32_t)lane == g) off += __builtin_popcountll(m);
        }
        if (valid) sink(dest, i, id);
    }
}

// launch shapes: count and scatter grid-stride over at most max_tiles wave tiles, one wave each; the scan's single block has one wave per owner
inline dim3 partition_grid(int64_t max_tiles) { return dim3(grid1d(max_tiles * 64, kBlock, 4096)); }
inline dim3 partition_scan_block(uint32_t P) { return dim3(64 * (P < 16 ? P : 16)); }

} // namespace
#endif
