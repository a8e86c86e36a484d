// Pose overlays on the GPU (include/hrnet_mi355.h: hrn_draw_poses): the reference's per-person cv2.line / cv2.circle loop
// (misc/visualization.py:71-192, scripts/live-demo.py:135-138) as two launches per call, whatever the number of frames and people.
//
//   draw_build_kernel    one wave per person: live mask, truncated coordinates and the grown bounding box of the live joints, read
//                        from the joints where the decode left them (no host synchronisation)
//   draw_raster_kernel   one 256-thread block per 32 x 32 tile of every canvas somebody is drawn on; a thread owns one 2 x 2 pixel
//                        block (and so, on a 4:2:0 canvas, one chroma sample)
//
// Every primitive is ONE shape here: a capsule around the segment P0 P1 with the squared diameter q2 --
//   bone   P0, P1 = the two joints, q2 = T^2;
//   disc   P0 = P1 = the joint,     q2 = 4 (r^2 + r): with d = 0 the capsule test reads 4 |w|^2 <= q2, which is |w|^2 <= r^2 + r.
// Integer ranges (frame sides <= 8192, live coordinates in [-8192, 16383]): |w| components <= 16383 < 2^14, |d| components
// <= 24575 < 2^14.6; t = w.d and L2 = d.d are below 2^30.3 (int32); 4 |w|^2 <= 2 147 221 512 (uint32); cross < 2^29.6, so
// 4 cross^2 < 2^61.2 and q2 L2 < 2^44.3 (int64).
//
// The tile's primitive list is built LAST PRIMITIVE FIRST, in chunks: people of the frame are culled by box 256 at a time from the
// end of the call order, the primitives of the survivors 256 at a time from the end of each person (joints J-1 .. 0, then bones
// K-1 .. 0), both by wave-ballot compaction that keeps the order.  The list (512 entries of LDS) is resolved whenever the next
// chunk might not fit, and at the end: each thread walks it from the front -- the highest-numbered primitive -- and stops once
// its four pixels have a colour; the block stops once every thread has.  Nothing is dropped, no atomics, no scratch of frame
// size; each byte of a canvas is written by at most one thread, and only when a primitive covers its pixel.
//
// Person labels (hrn_draw_labels_dev) follow at the end of the file: label_build_kernel and label_raster_kernel, on the same tile
// geometry, frame table and writer.
#include <hip/hip_runtime.h>

#include "draw_labels_math.h"
#include "draw_tile.h"   // block_compact, frame_of_tile: shared with heat.hip
#include "kernels.h"

namespace hrn {

namespace {

constexpr int kThreads = kDrawThreads;
constexpr int kWaves = kDrawWaves;
constexpr int kList = 512;   // entries of the tile's primitive list: two chunks, so that a chunk always fits after a resolve

__device__ __forceinline__ int wave_min(int v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// trunc(v) when it is finite and lies in [-8192, 16383] (int() of the reference: -0.7 -> 0); false otherwise (NaN fails both tests)
__device__ __forceinline__ bool live_coordinate(float v, int *out) {
    const float t = truncf(v);
    if (!(t >= -8192.0f && t <= 16383.0f)) return false;
    *out = (int)t;
    return true;
}

// the capsule test of include/hrnet_mi355.h, literally
__device__ __forceinline__ bool covers(int px, int py, int x0, int y0, int x1, int y1, int q2) {
    const int dx = x1 - x0, dy = y1 - y0, wx = px - x0, wy = py - y0;
    const int l2 = dx * dx + dy * dy, t = wx * dx + wy * dy;
    if (t <= 0) return 4u * (unsigned)(wx * wx + wy * wy) <= (unsigned)q2;
    if (t >= l2) {
        const int ux = px - x1, uy = py - y1;
        return 4u * (unsigned)(ux * ux + uy * uy) <= (unsigned)q2;
    }
    const long long cross = (long long)wx * dy - (long long)wy * dx;
    return 4 * cross * cross <= (long long)q2 * l2;
}

// what a thread writes of its 2 x 2 block at (px, py): the pixels of `drawn` in their colours; on a 4:2:0 canvas the block's
// chroma sample from `first`, the colour of the highest primitive on any of the four
__device__ __forceinline__ void write_block(const DrawFrame &f, int px, int py, unsigned drawn, const unsigned (&colour)[4], unsigned first) {
    if (drawn == 0) return;
    if (f.format == 0) {   // HRN_PIX_BGR
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if ((drawn >> p) & 1u) {
                unsigned char *dst = f.p0 + (size_t)(py + (p >> 1)) * f.pitch0 + (size_t)(px + (p & 1)) * 3;
                dst[0] = (unsigned char)colour[p], dst[1] = (unsigned char)(colour[p] >> 8), dst[2] = (unsigned char)(colour[p] >> 16);
            }
        return;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
        if ((drawn >> p) & 1u) f.p0[(size_t)(py + (p >> 1)) * f.pitch0 + px + (p & 1)] = (unsigned char)colour[p];
    const size_t crow = (size_t)(py >> 1) * f.pitch1;
    if (f.format == 1) {   // HRN_PIX_NV12: interleaved U, V
        f.p1[crow + px] = (unsigned char)(first >> 8), f.p1[crow + px + 1] = (unsigned char)(first >> 16);
    } else {               // HRN_PIX_I420
        f.p1[crow + (px >> 1)] = (unsigned char)(first >> 8), f.p2[crow + (px >> 1)] = (unsigned char)(first >> 16);
    }
}

}  // namespace

__global__ __launch_bounds__(64) void draw_build_kernel(DrawArgs a) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const DrawFrame &f = a.frames[a.person_frame[i]];
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -0x7fffffff, y1 = -0x7fffffff;
    for (int j0 = 0; j0 < a.J; j0 += 64) {
        const int j = j0 + lane;
        bool live = false;
        int X = 0, Y = 0;
        if (j < a.J) {
            const float *p = a.pts + ((size_t)i * a.J + j) * 3;   // (y, x, confidence)
            live = p[2] > a.threshold;                           // (equality and NaN: not live)
            live = live_coordinate(p[1], &X) && live;
            live = live_coordinate(p[0], &Y) && live;
            a.xy[(size_t)i * a.J + j] = make_short2((short)X, (short)Y);
        }
        if (live) x0 = min(x0, X), y0 = min(y0, Y), x1 = max(x1, X), y1 = max(y1, Y);
        const unsigned long long b = __ballot(live);
        if (lane == 0) a.live[(size_t)i * (kMaxJoints / 32) + j0 / 32] = (unsigned)b;
        if (lane == 1) a.live[(size_t)i * (kMaxJoints / 32) + j0 / 32 + 1] = (unsigned)(b >> 32);
    }
    x0 = wave_min(x0), y0 = wave_min(y0), x1 = wave_max(x1), y1 = wave_max(y1);
    if (lane == 0) {
        const int grow = max(f.radius, (a.thickness + 1) / 2);
        a.box[i] = x1 < x0 ? make_int4(1, 1, 0, 0) : make_int4(x0 - grow, y0 - grow, x1 + grow, y1 + grow);   // nobody live: empty
    }
}

__global__ __launch_bounds__(kThreads) void draw_raster_kernel(DrawArgs a) {
    __shared__ uint4 list[kList];      // x: x0 | y0 << 16, y: x1 | y1 << 16 (int16 each), z: q2 | reach << 16, w: the colour's three bytes
    __shared__ int people[kThreads];   // the people of the current chunk whose box meets the tile, last first
    __shared__ int wave_count[kWaves];
    const int tid = threadIdx.x;

    const int tile = blockIdx.x;
    const DrawFrame f = a.frames[frame_of_tile(a.frames, a.nframes, tile)];
    const int local = tile - f.tile_start, trow = local / f.tiles_x, tcol = local - trow * f.tiles_x;
    const int tx0 = tcol * kDrawTile, ty0 = trow * kDrawTile, tx1 = tx0 + kDrawTile - 1, ty1 = ty0 + kDrawTile - 1;
    const int px = tx0 + 2 * (tid & 15), py = ty0 + 2 * (tid >> 4);   // this thread's 2 x 2 block: pixel k = (px + (k & 1), py + (k >> 1))

    unsigned outside = 0;   // pixels beyond an odd BGR frame's edge count as finished and are never written
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (px + (k & 1) >= f.width || py + (k >> 1) >= f.height) outside |= 1u << k;
    unsigned done = outside, colour[4] = {0, 0, 0, 0}, first = 0;   // first: the colour of the highest primitive on any of the four

    const auto resolve = [&](int count) {
        for (int k = 0; k < count && done != 15u; ++k) {
            const uint4 e = list[k];
            const int x0 = (short)(e.x & 0xffffu), y0 = (short)(e.x >> 16), x1 = (short)(e.y & 0xffffu), y1 = (short)(e.y >> 16);
            const int q2 = (int)(e.z & 0xffffu), reach = (int)(e.z >> 16);
            if (min(x0, x1) - reach > px + 1 || max(x0, x1) + reach < px || min(y0, y1) - reach > py + 1 || max(y0, y1) + reach < py) continue;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if ((done >> p) & 1u) continue;
                if (covers(px + (p & 1), py + (p >> 1), x0, y0, x1, y1, q2)) {
                    if (done == outside) first = e.w;
                    colour[p] = e.w;
                    done |= 1u << p;
                }
            }
        }
    };

    const int Q = a.K + a.J;
    int held = 0;            // entries in the list (the same in every thread)
    bool finished = false;   // every pixel of the tile has its colour
    for (int pend = f.person_count; pend > 0 && !finished; pend -= kThreads) {
        const int pi = pend - 1 - tid;   // people of the frame from the last backwards
        int person = 0;
        bool meets = false;
        if (pi >= 0) {
            person = a.order[f.person_start + pi];
            const int4 b = a.box[person];
            meets = b.x <= tx1 && b.z >= tx0 && b.y <= ty1 && b.w >= ty0;
        }
        const int np = block_compact(meets, wave_count, [&](int at) { people[at] = person; });
        const int total = np * Q;        // (np <= 256, Q <= 65535 + 256: the host bounds K)
        for (int e0 = 0; e0 < total; e0 += kThreads) {
            if (held > kList - kThreads) {
                resolve(held);
                held = 0;
                if (__syncthreads_count(done != 15u) == 0) {
                    finished = true;
                    break;
                }
            }
            const int e = e0 + tid;
            bool keep = false;
            uint4 entry = make_uint4(0, 0, 0, 0);
            if (e < total) {
                const int s = e / Q, q = Q - 1 - (e - s * Q);   // the person's primitives from the last backwards
                const int who = people[s];
                const unsigned *lv = a.live + (size_t)who * (kMaxJoints / 32);
                const short2 *xy = a.xy + (size_t)who * a.J;
                int ja, jb, q2, reach;
                unsigned c;
                if (q >= a.K) {   // joint q - K
                    ja = jb = q - a.K;
                    q2 = 4 * (f.radius * f.radius + f.radius), reach = f.radius;
                    c = a.point_colour[ja % a.Cp];
                } else {
                    const unsigned pair = a.skeleton[q];
                    ja = (int)(pair & 0xffffu), jb = (int)(pair >> 16);
                    q2 = a.thickness * a.thickness, reach = (a.thickness + 1) / 2;
                    c = a.bone_colour[who];
                }
                if (((lv[ja >> 5] >> (ja & 31)) & (lv[jb >> 5] >> (jb & 31)) & 1u) != 0) {
                    const short2 p0 = xy[ja], p1 = xy[jb];
                    keep = min(p0.x, p1.x) - reach <= tx1 && max(p0.x, p1.x) + reach >= tx0 && min(p0.y, p1.y) - reach <= ty1 &&
                           max(p0.y, p1.y) + reach >= ty0;
                    entry = make_uint4((unsigned)(unsigned short)p0.x | ((unsigned)(unsigned short)p0.y << 16),
                                       (unsigned)(unsigned short)p1.x | ((unsigned)(unsigned short)p1.y << 16),
                                       (unsigned)q2 | ((unsigned)reach << 16), c);
                }
            }
            held += block_compact(keep, wave_count, [&](int at) { list[held + at] = entry; });
        }
    }
    if (!finished && held > 0) resolve(held);

    write_block(f, px, py, done & ~outside, colour, first);
}

hipError_t launch_draw(const DrawArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.total_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(draw_build_kernel, dim3((unsigned)a.n), dim3(64), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(draw_raster_kernel, dim3((unsigned)a.total_tiles), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

// ---- person labels (include/hrnet_mi355.h: hrn_draw_labels_dev; every rule: draw_labels_math.h) -----------------------------------
//   label_build_kernel    one thread per person: the record (outline, plate, cells, colours) and its reach, from box / id / score
//                         where they lie on the device
//   label_raster_kernel   draw_raster_kernel's geometry.  A tile culls its frame's people 256 at a time from the end of the call
//                         order -- first by reach, then by what of the record really meets the tile (a tile inside a box's interior
//                         holds no outline) -- and keeps the survivors' records in LDS, last person first; every thread walks them
//                         from the front and stops once its four pixels have a colour, the block once every thread has.  A chunk is
//                         resolved before the next is read, so no number of people on a tile loses anybody.
__global__ __launch_bounds__(kThreads) void label_build_kernel(LabelArgs a) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    const int32_t box[4] = {a.boxes[4 * (size_t)i], a.boxes[4 * (size_t)i + 1], a.boxes[4 * (size_t)i + 2], a.boxes[4 * (size_t)i + 3]};
    const int id = a.ids ? a.ids[i] : 0;
    const float score = a.scores ? a.scores[(size_t)i * a.score_stride] : 0.0f;
    LabelRecord r = label_layout(box, a.ids != nullptr, id, a.scores != nullptr, score, a.frames[a.person_frame[i]].radius, a.thickness);
    if (r.drawn) {
        const int c = label_colour_index(a.ids ? id : i, a.Cb);
        r.colour = a.colour[c], r.text_colour = a.text_colour[c];
    }
    a.records[i] = r;
    int32_t reach[4];
    label_reach(r, reach);
    a.reach[i] = make_int4(reach[0], reach[1], reach[2], reach[3]);
}

__global__ __launch_bounds__(kThreads) void label_raster_kernel(LabelArgs a) {
    __shared__ LabelRecord recs[kThreads];   // the people of the current chunk that meet the tile, last first
    __shared__ int wave_count[kWaves];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const DrawFrame f = a.frames[frame_of_tile(a.frames, a.nframes, tile)];
    const int local = tile - f.tile_start, trow = local / f.tiles_x, tcol = local - trow * f.tiles_x;
    const int tx0 = tcol * kDrawTile, ty0 = trow * kDrawTile, tx1 = tx0 + kDrawTile - 1, ty1 = ty0 + kDrawTile - 1;
    const int px = tx0 + 2 * (tid & 15), py = ty0 + 2 * (tid >> 4);   // this thread's 2 x 2 block: pixel k = (px + (k & 1), py + (k >> 1))

    unsigned outside = 0;   // pixels beyond an odd BGR frame's edge count as finished and are never written
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (px + (k & 1) >= f.width || py + (k >> 1) >= f.height) outside |= 1u << k;
    unsigned done = outside, c0 = 0, c1 = 0, c2 = 0, c3 = 0, first = 0;   // first: the colour of the highest primitive on any of the four

    for (int pend = f.person_count; pend > 0; pend -= kThreads) {
        const int pi = pend - 1 - tid;   // people of the frame from the last backwards
        bool meets = false;
        int person = 0;
        if (pi >= 0) {
            person = a.order[f.person_start + pi];
            const int4 b = a.reach[person];
            if (b.x <= tx1 && b.z >= tx0 && b.y <= ty1 && b.w >= ty0) {
                const LabelRecord rec = a.records[person];
                const int T = rec.thickness;
                const bool plate = rec.ncells > 0 && rec.left <= tx1 && rec.left + rec.width - 1 >= tx0 && rec.top <= ty1 &&
                                   rec.top + rec.height - 1 >= ty0;
                const bool outer = T > 0 && rec.x1 <= tx1 && rec.x2 >= tx0 && rec.y1 <= ty1 && rec.y2 >= ty0;
                const bool interior = tx0 >= rec.x1 + T && tx1 <= rec.x2 - T && ty0 >= rec.y1 + T && ty1 <= rec.y2 - T;
                meets = plate || (outer && !interior);
            }
        }
        const int np = block_compact(meets, wave_count, [&](int at) { recs[at] = a.records[person]; });   // (read again: it is in cache)
        for (int k = 0; k < np && done != 15u; ++k) {
            const LabelRecord &r = recs[k];
            unsigned now = 0;
            int best = LABEL_NONE;   // ink outnumbers plate and outline of the same person
            const auto pixel = [&](int p, unsigned &c) {
                if ((done >> p) & 1u) return;
                const int cls = label_covers(r, px + (p & 1), py + (p >> 1));
                if (cls == LABEL_NONE) return;
                c = cls == LABEL_TEXT ? r.text_colour : r.colour;
                now |= 1u << p;
                best = max(best, cls);
            };
            pixel(0, c0), pixel(1, c1), pixel(2, c2), pixel(3, c3);
            if (now != 0 && done == outside) first = best == LABEL_TEXT ? r.text_colour : r.colour;
            done |= now;
        }
        if (__syncthreads_count(done != 15u) == 0) break;
    }
    const unsigned colour[4] = {c0, c1, c2, c3};
    write_block(f, px, py, done & ~outside, colour, first);
}

hipError_t launch_draw_labels(const LabelArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.total_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(label_build_kernel, dim3((unsigned)((a.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(label_raster_kernel, dim3((unsigned)a.total_tiles), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace hrn
