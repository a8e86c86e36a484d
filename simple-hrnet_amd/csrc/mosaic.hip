// The face mosaic on the GPU (include/hrnet_mi355.h: hrn_mosaic_dev; every rule: mosaic_math.h): a square around chosen joints
// of every person, or a given box, pixelated in place, as two launches per call, whatever the number of frames and people.
//
//   mosaic_build_kernel   joints: one wave per person -- lanes stride the joints, the extents of the listed and of all live joints
//                         by wave minimum / maximum, as draw_build_kernel; boxes: one thread per person.  Reads pts or boxes where
//                         they lie and writes the clipped region (or an empty one) and the status.
//   mosaic_raster_kernel  draw_raster_kernel's geometry (draw_tile.h): one 256-thread block per 32 x 32 tile of every canvas
//                         somebody refers to, a thread per 2 x 2 block (one 4:2:0 chroma sample).  A tile culls its canvas's people
//                         by region 256 at a time, by wave-ballot compaction into LDS; thread t owns cell t of the tile's
//                         (32 / s)^2 <= 256 cells and ORs every chunk's survivors into its mark before the next chunk is read: no
//                         list exists that can overflow.  The marks become a bit mask in LDS.  A tile with an empty mask returns
//                         having read no frame byte.  Then a thread whose cell is marked loads its 2 x 2 block and forms three
//                         integer sums (B, G, R, or Y, U, V); the sums of a cell are reduced across lanes with __shfl_xor over the
//                         lane bits a wave holds (the four column bits, two row bits) and, for s = 16 and 32, across waves through
//                         LDS; every thread then writes its own block from its cell's means.
//
// A cell (s a power of two <= 32, canvas-aligned) lies inside one tile, so inside one block: its owner reads it whole before it
// writes it, which is why in place is safe, and each byte has one writer.  Integer sums: any reduction order gives the same bits.
// No atomics, no scratch of frame size.
//
// Thread geometry: tid = row * 16 + col of the 2 x 2 block, a wave holds four block rows (8 pixel rows of the tile).  A cell is
// s / 2 blocks wide and high: its columns are lane bits 0 .. log2(s / 2) - 1, its rows tid bits 4 .. 4 + log2(s / 2) - 1, of which
// bits 4 and 5 are lane bits and bits 6 and 7 the wave number.
//
// Accesses are bytes.  A thread's piece of a row is 6 bytes of BGR at a multiple of 6, or 2 bytes of Y: no dword fits it, and the
// call is bound by its two launches at every measured size (profiles/mosaic.txt, profiles/EXPERIMENTS.md).
#include <hip/hip_runtime.h>

#include "draw_tile.h"
#include "kernels.h"
#include "mosaic_math.h"

namespace hrn {

namespace {
__device__ __forceinline__ int wave_min_i(int v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
}  // namespace

// joints: blockIdx.x = person, 64 lanes; boxes: one thread per person
__global__ __launch_bounds__(64) void mosaic_build_kernel(MosaicArgs a) {
    const int lane = threadIdx.x;
    int out[4];
    if (a.boxes) {
        const int i = blockIdx.x * 64 + lane;
        if (i >= a.n) return;
        const DrawFrame &f = a.frames[a.person_frame[i]];
        const int st = mosaic_region_of_box(a.boxes + 4 * (size_t)i, f.height, f.width, out);
        a.region[i] = make_int4(out[0], out[1], out[2], out[3]);
        if (a.status) a.status[i] = st;
        return;
    }
    const int i = blockIdx.x;
    MosaicExtent listed = mosaic_extent_empty(), person = mosaic_extent_empty();
    for (int j = lane; j < a.J; j += 64) {
        int X = 0, Y = 0;
        if (!mosaic_joint_live(a.pts + ((size_t)i * a.J + j) * 3, a.threshold, &X, &Y)) continue;
        mosaic_extent_add(person, X, Y);
        if ((a.listed[j >> 5] >> (j & 31)) & 1u) mosaic_extent_add(listed, X, Y);
    }
    // (minimum and maximum of integers: exact in any order; an empty lane holds the neutral elements)
    listed.x0 = wave_min_i(listed.x0), listed.y0 = wave_min_i(listed.y0), listed.x1 = wave_max_i(listed.x1), listed.y1 = wave_max_i(listed.y1);
    person.x0 = wave_min_i(person.x0), person.y0 = wave_min_i(person.y0), person.x1 = wave_max_i(person.x1), person.y1 = wave_max_i(person.y1);
    if (lane == 0) {
        const DrawFrame &f = a.frames[a.person_frame[i]];
        const int st = mosaic_region(listed, person, a.scale_num, a.scale_den, a.min_half, f.height, f.width, out);
        a.region[i] = make_int4(out[0], out[1], out[2], out[3]);
        if (a.status) a.status[i] = st;
    }
}

__global__ __launch_bounds__(kDrawThreads) void mosaic_raster_kernel(MosaicArgs a) {
    __shared__ int4 regions[kDrawThreads];      // the regions of the current chunk that meet the tile
    __shared__ int wave_count[kDrawWaves];
    __shared__ unsigned mask[kDrawThreads / 32];   // bit t: cell t of the tile is marked
    __shared__ int part[kDrawWaves][2][3];      // s >= 16: a wave's sums of the (at most two) cells it holds a part of
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const int tile = blockIdx.x;
    const DrawFrame f = a.frames[frame_of_tile(a.frames, a.nframes, tile)];
    const int local = tile - f.tile_start, trow = local / f.tiles_x, tcol = local - trow * f.tiles_x;
    const int tx0 = tcol * kDrawTile, ty0 = trow * kDrawTile, tx1 = tx0 + kDrawTile - 1, ty1 = ty0 + kDrawTile - 1;
    const int s = f.radius;                     // the canvas's cell size: 2, 4, 8, 16 or 32
    const int shift = 31 - __clz(s);            // log2(s)
    const int g = kDrawTile >> shift;           // cells per side of the tile; cell t = row * g + col

    // ---- cull and mark: thread t owns cell t ----
    const bool owner = tid < g * g;
    const int ox0 = tx0 + ((tid & (g - 1)) << shift), oy0 = ty0 + ((tid / g) << shift);   // (beyond the canvas's edge: no clipped region meets it)
    bool marked = false;
    for (int base = 0; base < f.person_count; base += kDrawThreads) {
        const int pi = base + tid;
        int4 r = make_int4(0, 0, 0, 0);
        bool meets = false;
        if (pi < f.person_count) {
            r = a.region[a.order[f.person_start + pi]];
            meets = r.z > r.x && r.w > r.y && r.x <= tx1 && r.z > tx0 && r.y <= ty1 && r.w > ty0;   // (x2, y2: exclusive)
        }
        const int np = block_compact(meets, wave_count, [&](int at) { regions[at] = r; });
        if (owner && !marked)
            for (int k = 0; k < np && !marked; ++k) {
                const int4 q = regions[k];
                marked = mosaic_meets(q.x, q.y, q.z, q.w, ox0, oy0, s);
            }
    }
    const unsigned long long b = __ballot(marked);
    if (lane == 0) mask[2 * wave] = (unsigned)b;
    if (lane == 1) mask[2 * wave + 1] = (unsigned)(b >> 32);
    if (__syncthreads_or(marked) == 0) return;  // (the barrier also publishes the mask)

    // ---- this thread's 2 x 2 block, its cell, its sums ----
    const int bx = tid & 15, by = tid >> 4;     // block column and row in the tile
    const int px = tx0 + 2 * bx, py = ty0 + 2 * by;
    const int ccol = (2 * bx) >> shift, crow = (2 * by) >> shift, cell = crow * g + ccol;
    const bool mine = (mask[cell >> 5] >> (cell & 31)) & 1u;
    const bool in_x0 = px < f.width, in_x1 = px + 1 < f.width, in_y0 = py < f.height, in_y1 = py + 1 < f.height;   // (an odd BGR frame's edge)
    const bool bgr = f.format == 0;             // HRN_PIX_BGR
    const size_t crow_at = (size_t)(py >> 1) * f.pitch1;
    unsigned char *up = nullptr, *vp = nullptr; // this block's chroma sample (YUV; sides are even: the block is whole)
    if (!bgr) {
        up = f.format == 1 ? f.p1 + crow_at + px : f.p1 + crow_at + (px >> 1);        // HRN_PIX_NV12: interleaved U, V
        vp = f.format == 1 ? f.p1 + crow_at + px + 1 : f.p2 + crow_at + (px >> 1);    // HRN_PIX_I420: planes of their own
    }
    int s0 = 0, s1 = 0, s2 = 0;
    if (mine && in_x0 && in_y0) {
        if (bgr) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (!((p & 1) ? in_x1 : in_x0) || !((p >> 1) ? in_y1 : in_y0)) continue;
                const unsigned char *src = f.p0 + (size_t)(py + (p >> 1)) * f.pitch0 + (size_t)(px + (p & 1)) * 3;
                s0 += src[0], s1 += src[1], s2 += src[2];
            }
        } else {
            const unsigned char *y0 = f.p0 + (size_t)py * f.pitch0 + px, *y1 = y0 + f.pitch0;
            s0 = y0[0] + y0[1] + y1[0] + y1[1];
            s1 = *up, s2 = *vp;
        }
    }

    // ---- reduce over the cell: columns and the rows a wave holds by shuffle, the rest through LDS (s is uniform in the block) ----
    const int half = s >> 1;                    // blocks per side of a cell: 1, 2, 4, 8 or 16
    for (int o = 1; o < half && o < 16; o <<= 1) s0 += __shfl_xor(s0, o), s1 += __shfl_xor(s1, o), s2 += __shfl_xor(s2, o);
    for (int o = 1; o < half && o < 4; o <<= 1) {
        s0 += __shfl_xor(s0, 16 * o), s1 += __shfl_xor(s1, 16 * o), s2 += __shfl_xor(s2, 16 * o);
    }
    if (half > 4) {                             // s = 16: a cell spans two waves, a wave holds parts of two cells; s = 32: four and one
        const int slot = half == 8 ? (bx >> 3) : 0;
        if ((lane & (half - 1)) == 0 && (lane >> 4) == 0) part[wave][slot][0] = s0, part[wave][slot][1] = s1, part[wave][slot][2] = s2;
        __syncthreads();
        const int waves = half >> 2, first = wave & ~(waves - 1);
        s0 = s1 = s2 = 0;
        for (int w = first; w < first + waves; ++w) s0 += part[w][slot][0], s1 += part[w][slot][1], s2 += part[w][slot][2];
    }
    if (!(mine && in_x0 && in_y0)) return;

    // ---- every thread writes its own block from its cell's means ----
    const int c = mosaic_cell_count(tx0 + (ccol << shift), ty0 + (crow << shift), s, f.height, f.width);
    if (bgr) {
        const unsigned char m0 = (unsigned char)mosaic_mean(s0, c), m1 = (unsigned char)mosaic_mean(s1, c), m2 = (unsigned char)mosaic_mean(s2, c);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (!((p & 1) ? in_x1 : in_x0) || !((p >> 1) ? in_y1 : in_y0)) continue;
            unsigned char *dst = f.p0 + (size_t)(py + (p >> 1)) * f.pitch0 + (size_t)(px + (p & 1)) * 3;
            dst[0] = m0, dst[1] = m1, dst[2] = m2;
        }
        return;
    }
    const unsigned char my = (unsigned char)mosaic_mean(s0, c);
    unsigned char *y0 = f.p0 + (size_t)py * f.pitch0 + px, *y1 = y0 + f.pitch0;
    y0[0] = my, y0[1] = my, y1[0] = my, y1[1] = my;
    *up = (unsigned char)mosaic_mean(s1, c >> 2), *vp = (unsigned char)mosaic_mean(s2, c >> 2);   // (even sides: c / 4 chroma samples)
}

hipError_t launch_mosaic(const MosaicArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.total_tiles <= 0) return hipSuccess;
    const unsigned blocks = a.boxes ? (unsigned)((a.n + 63) / 64) : (unsigned)a.n;
    hipLaunchKernelGGL(mosaic_build_kernel, dim3(blocks), dim3(64), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mosaic_raster_kernel, dim3((unsigned)a.total_tiles), dim3(kDrawThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace hrn
