// What the tile rasterisers share (draw.hip: draw_raster_kernel, label_raster_kernel; heat.hip: heat_raster_kernel): one
// 256-thread block per 32 x 32 tile of every canvas of the call's DrawFrame table, a thread per 2 x 2 block; the tile's frame, and
// the order-keeping compaction the tiles cull their people with.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"

namespace hrn {

constexpr int kDrawThreads = 256;
constexpr int kDrawWaves = kDrawThreads / 64;
static_assert(kDrawTile == 32 && kDrawThreads == (kDrawTile / 2) * (kDrawTile / 2), "one thread per 2 x 2 block of the tile");

// Order-keeping compaction over the block: the threads whose `pred` holds call write(position) with consecutive positions in
// thread order; returns their number.  Three barriers: the first also ends every earlier read of what `write` overwrites, the
// last publishes what it wrote.
template <class Write>
__device__ __forceinline__ int block_compact(bool pred, int *wave_count, const Write &write) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(pred);
    const int rank = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wave_count[wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kDrawWaves; ++k) {
        const int c = wave_count[k];
        if (k < wave) before += c;
        total += c;
    }
    if (pred) write(before + rank);
    __syncthreads();
    return total;
}

// the frame of a tile: the last one whose first tile is not behind it (every frame of the table has tiles)
__device__ __forceinline__ int frame_of_tile(const DrawFrame *frames, int nframes, int tile) {
    int lo = 0, hi = nframes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (frames[mid].tile_start <= tile) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace hrn
