// Heat-map overlays on the GPU (include/hrnet_mi355.h: hrn_draw_heatmaps_dev; every rule: heat_math.h): what the network sees,
// blended into the frame, as two launches per call, whatever the number of frames and people.
//
//   heat_reduce_kernel   one thread per (person, cell): the maximum over the masked joints, quantised to a byte.  The one pass
//                        over the (n, J, hq, wq) fp32 tensor, each value read once, a wave reading 256 contiguous bytes of a row
//                        of cells per joint; Q (n, hq, wq) goes into the call's scratch.
//   heat_raster_kernel   draw_raster_kernel's geometry (draw_tile.h): one 256-thread block per 32 x 32 tile of every canvas
//                        somebody refers to, a thread per 2 x 2 block (one 4:2:0 chroma sample).  A tile culls its canvas's people
//                        by box 256 at a time, by wave-ballot compaction into LDS, and folds every chunk's survivors into the
//                        running maximum V of each thread's four pixels before the next chunk is read: no number of boxes on a
//                        tile loses anybody, and a maximum has no order.  Then every thread blends and stores once.  No atomics,
//                        no scratch of frame size; each byte of a canvas is read and written by one thread, and only when its
//                        pixel is written.  A tile nobody's box touches returns after the cull.
//
// Q is read through L1 / L2 where it lies, not staged in LDS: a tile's window of a person's map is a few dozen bytes (a 64 x 48
// map under a 256 x 192 box has one cell per four pixels), neighbouring threads read the same or adjacent bytes, and a person's
// whole map is 3 KiB.  The colour table (1 KiB) is staged: it is indexed by value, in no order.
//
// Integer ranges: a canvas pixel is in [0, 8191] and a drawn box starts at -8192 or later, so a pixel's offset in its box is at
// most 16383 and heat_coord's 32-bit product holds (heat_math.h); a sample's sum is at most 255 * 2^16 < 2^24.
#include <hip/hip_runtime.h>

#include "draw_tile.h"
#include "heat_math.h"
#include "kernels.h"

namespace hrn {

namespace {
constexpr int kReduceThreads = 256;
}

__global__ __launch_bounds__(kReduceThreads) void heat_reduce_kernel(HeatArgs a) {
    const int cells = a.hq * a.wq;                        // <= 2^20
    const int cell = blockIdx.y * kReduceThreads + threadIdx.x;
    if (cell >= cells) return;
    const size_t person = blockIdx.x;
    const float *m = a.maps + person * (size_t)a.J * cells + cell;
    float v = __builtin_nanf("");
    for (int i0 = 0; i0 < a.njoints; i0 += 4) {           // four loads in flight; a repeated joint does not change a maximum
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = m[(size_t)a.joints[min(i0 + u, a.njoints - 1)] * cells];
#pragma unroll
        for (int u = 0; u < 4; ++u) v = heat_max(v, x[u]);
    }
    a.q[person * cells + cell] = (unsigned char)heat_quantise(v, a.lo, a.k);
}

__global__ __launch_bounds__(kDrawThreads) void heat_raster_kernel(HeatArgs a) {
    __shared__ int4 boxes[kDrawThreads];    // the people of the current chunk whose box meets the tile
    __shared__ int who[kDrawThreads];
    __shared__ unsigned lut[256];
    __shared__ int wave_count[kDrawWaves];
    const int tid = threadIdx.x;
    lut[tid] = a.lut[tid];                   // (published by the cull's barriers: every frame of the table has people)

    const int tile = blockIdx.x;
    const DrawFrame f = a.frames[frame_of_tile(a.frames, a.nframes, tile)];
    const int local = tile - f.tile_start, trow = local / f.tiles_x, tcol = local - trow * f.tiles_x;
    const int tx0 = tcol * kDrawTile, ty0 = trow * kDrawTile, tx1 = tx0 + kDrawTile - 1, ty1 = ty0 + kDrawTile - 1;
    const int px = tx0 + 2 * (tid & 15), py = ty0 + 2 * (tid >> 4);   // this thread's 2 x 2 block: pixel k = (px + (k & 1), py + (k >> 1))
    const bool in_x0 = px < f.width, in_x1 = px + 1 < f.width, in_y0 = py < f.height, in_y1 = py + 1 < f.height;   // (an odd BGR frame's edge)

    const int cells = a.hq * a.wq;
    int v0 = 0, v1 = 0, v2 = 0, v3 = 0;     // V of the four pixels
    bool touched = false;                   // somebody's box meets the tile (the same in every thread)
    for (int base = 0; base < f.person_count; base += kDrawThreads) {
        const int pi = base + tid;
        int person = 0;
        int4 b = make_int4(0, 0, 0, 0);
        bool meets = false;
        if (pi < f.person_count) {
            person = a.order[f.person_start + pi];
            const int *src = a.boxes + 4 * (size_t)person;
            b = make_int4(src[0], src[1], src[2], src[3]);
            meets = heat_box_drawn(b.x, b.y, b.z, b.w) && b.x <= tx1 && b.z > tx0 && b.y <= ty1 && b.w > ty0;   // (x2, y2: exclusive)
        }
        const int np = block_compact(meets, wave_count, [&](int at) { boxes[at] = b, who[at] = person; });
        touched = touched || np > 0;
        for (int k = 0; k < np; ++k) {
            const int4 box = boxes[k];
            const bool cx0 = in_x0 && px >= box.x && px < box.z, cx1 = in_x1 && px + 1 >= box.x && px + 1 < box.z;
            const bool cy0 = in_y0 && py >= box.y && py < box.w, cy1 = in_y1 && py + 1 >= box.y && py + 1 < box.w;
            if (!((cx0 || cx1) && (cy0 || cy1))) continue;
            const unsigned char *q = a.q + (size_t)who[k] * cells;
            const int bw = box.z - box.x, bh = box.w - box.y;
            const int ux0 = cx0 ? heat_coord(px - box.x, a.wq, bw) : 0, ux1 = cx1 ? heat_coord(px + 1 - box.x, a.wq, bw) : 0;
            const int uy0 = cy0 ? heat_coord(py - box.y, a.hq, bh) : 0, uy1 = cy1 ? heat_coord(py + 1 - box.y, a.hq, bh) : 0;
            if (cx0 && cy0) v0 = max(v0, heat_sample(q, a.hq, a.wq, ux0, uy0));
            if (cx1 && cy0) v1 = max(v1, heat_sample(q, a.hq, a.wq, ux1, uy0));
            if (cx0 && cy1) v2 = max(v2, heat_sample(q, a.hq, a.wq, ux0, uy1));
            if (cx1 && cy1) v3 = max(v3, heat_sample(q, a.hq, a.wq, ux1, uy1));
        }
    }
    if (!touched) return;

    const int V[4] = {v0, v1, v2, v3};
    if (f.format == 0) {   // HRN_PIX_BGR
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            int al;
            if (!heat_written(V[p], a.alpha, a.mode, a.cutoff, &al)) continue;   // (a pixel beyond the frame's edge has V = 0)
            unsigned char *dst = f.p0 + (size_t)(py + (p >> 1)) * f.pitch0 + (size_t)(px + (p & 1)) * 3;
            const unsigned c = lut[V[p]];
            dst[0] = (unsigned char)heat_blend(dst[0], (int)(c & 255u), al);
            dst[1] = (unsigned char)heat_blend(dst[1], (int)((c >> 8) & 255u), al);
            dst[2] = (unsigned char)heat_blend(dst[2], (int)((c >> 16) & 255u), al);
        }
        return;
    }
    bool any = false;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        int al;
        if (!heat_written(V[p], a.alpha, a.mode, a.cutoff, &al)) continue;
        unsigned char *dst = f.p0 + (size_t)(py + (p >> 1)) * f.pitch0 + px + (p & 1);
        *dst = (unsigned char)heat_blend(*dst, (int)(lut[V[p]] & 255u), al);
        any = true;
    }
    if (!any) return;
    const int vc = heat_block_value(v0, v1, v2, v3), ac = heat_alpha(vc, a.alpha, a.mode);
    if (ac <= 0) return;
    const unsigned c = lut[vc];
    const size_t crow = (size_t)(py >> 1) * f.pitch1;
    unsigned char *u = f.format == 1 ? f.p1 + crow + px : f.p1 + crow + (px >> 1);           // HRN_PIX_NV12: interleaved U, V
    unsigned char *v = f.format == 1 ? f.p1 + crow + px + 1 : f.p2 + crow + (px >> 1);       // HRN_PIX_I420: planes of their own
    *u = (unsigned char)heat_blend(*u, (int)((c >> 8) & 255u), ac);
    *v = (unsigned char)heat_blend(*v, (int)((c >> 16) & 255u), ac);
}

hipError_t launch_draw_heatmaps(const HeatArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.total_tiles <= 0) return hipSuccess;
    const int cells = a.hq * a.wq;
    hipLaunchKernelGGL(heat_reduce_kernel, dim3((unsigned)a.n, (unsigned)((cells + kReduceThreads - 1) / kReduceThreads)),
                       dim3(kReduceThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(heat_raster_kernel, dim3((unsigned)a.total_tiles), dim3(kDrawThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace hrn
