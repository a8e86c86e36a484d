// BGR frames to 4:2:0 YCbCr frames on the GPU (include/hrnet_mi355.h: hrn_bgr_to_yuv_frames): the way back from the frame the
// overlays draw on to the layout an encoder consumes -- NV12 / NV21, I420 and 10-bit P010 / I010.  The arithmetic is yuv_fwd.h's, the
// text the host form (hrn_bgr_to_yuv_blocks) compiles.
//
//   bgr_to_yuv_kernel   ONE launch for all frames of a call: one 256-thread block per 256 x 8-pixel tile of a frame, found by
//                       binary search in the call's frame table (one frame: it sits in the kernel arguments).  A thread owns a group
//                       of 2 rows x 4 pixels -- two 2x2 blocks: it reads 12 bytes of each of its two source rows (three dwords when
//                       the source's base and pitch are multiples of 4: a group starts at byte 12 g of its row; a wavefront then
//                       reads 768 consecutive bytes per row), converts the eight pixels and the two block sums, and writes
//                         Y       4 samples per row: one dword (8 bit) or two (10 bit)
//                         chroma  its two samples: NV12 / NV21 one dword (U V U V / V U V U); I420 one 16-bit store per plane;
//                                 P010 two dwords (the four words U V U V); I010 one dword per plane
//                       A width is even, not a multiple of 4: the last group of a row may hold 2 pixels, and goes in bytes (16-bit
//                       words for 10 bit).  So does every group of a plane whose base or pitch is not a multiple of 4 (I420's
//                       chroma: not even) -- three choices per frame (source, Y, chroma), each uniform over the block, as the layout is.
// Nothing outside a row's samples is read or written: a dword is used only where all its bytes are samples of the row, so pitch
// padding keeps its bytes; every sample byte has exactly one writer; no atomics, no LDS, no scratch.  Offsets inside a plane are
// 32-bit (the host refuses pitch * rows >= 2^31).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "yuv_fwd.h"
#include "yuv_px.h"

namespace hrn {

namespace {

constexpr int kYuvOutThreads = 256;
constexpr int kYuvOutGroupsX = kYuvOutTileW / 4;   // 64
static_assert(kYuvOutGroupsX * (kYuvOutTileH / 2) == kYuvOutThreads, "one group per thread");

struct alignas(4) Dwords2 {
    unsigned a, b;
};
struct alignas(4) Dwords3 {
    unsigned a, b, c;
};

__device__ __forceinline__ unsigned pack_bytes(int a, int b, int c, int d) {
    return (unsigned)a | ((unsigned)b << 8) | ((unsigned)c << 16) | ((unsigned)d << 24);
}
__device__ __forceinline__ unsigned pack_words(int lo, int hi) { return (unsigned)lo | ((unsigned)hi << 16); }

// the group (gx, gy) of frame f: pixels 4 gx .. 4 gx + ne - 1 of the rows 2 gy and 2 gy + 1
template <int FMT>
__device__ __forceinline__ void bgr_to_yuv_group(const YuvOutFrame &f, int gx, int gy, bool swide, bool ywide, bool cwide) {
    constexpr bool ten = yuv_is10<FMT>();
    constexpr int SB = ten ? 2 : 1;                              // bytes of a stored sample
    const int x0 = 4 * gx, ne = min(4, f.width - x0);            // 4, or 2 at the end of a row
    const bool whole = ne == 4;
    int rs[2] = {0, 0}, gs[2] = {0, 0}, bs[2] = {0, 0};          // the sums of the group's two 2x2 blocks
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        const int i = 2 * gy + row;
        const unsigned char *s = f.src + i * f.spitch + 3 * x0;
        int b[4], g[4], r[4];
        if (swide && whole) {   // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
            const Dwords3 d = *(const Dwords3 *)s;
            b[0] = d.a & 255, g[0] = (d.a >> 8) & 255, r[0] = (d.a >> 16) & 255, b[1] = d.a >> 24;
            g[1] = d.b & 255, r[1] = (d.b >> 8) & 255, b[2] = (d.b >> 16) & 255, g[2] = d.b >> 24;
            r[2] = d.c & 255, b[3] = (d.c >> 8) & 255, g[3] = (d.c >> 16) & 255, r[3] = d.c >> 24;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = e < ne;   // (a pixel beyond the row is not read)
                b[e] = in ? s[3 * e] : 0, g[e] = in ? s[3 * e + 1] : 0, r[e] = in ? s[3 * e + 2] : 0;
            }
        }
        int y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            y[e] = yuv_fwd_luma(f.coef, ten, r[e], g[e], b[e]);
            if (FMT == kPixP010) y[e] <<= 6;
            rs[e >> 1] += r[e], gs[e >> 1] += g[e], bs[e >> 1] += b[e];
        }
        unsigned char *o = f.y + i * f.pitch_y + x0 * SB;
        if (ywide && whole) {
            if (ten) *(Dwords2 *)o = Dwords2{pack_words(y[0], y[1]), pack_words(y[2], y[3])};
            else *(unsigned *)o = pack_bytes(y[0], y[1], y[2], y[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= ne) continue;
                if (ten) ((unsigned short *)o)[e] = (unsigned short)y[e];
                else o[e] = (unsigned char)y[e];
            }
        }
    }
    int u[2], v[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        u[k] = yuv_fwd_chroma(f.coef + 4, ten, rs[k], gs[k], bs[k]);
        v[k] = yuv_fwd_chroma(f.coef + 7, ten, rs[k], gs[k], bs[k]);
        if (FMT == kPixP010) u[k] <<= 6, v[k] <<= 6;
    }
    const int ns = ne >> 1;   // chroma samples of the group: 2, or 1
    if (FMT == kPixNV12 || FMT == kPixNV21 || FMT == kPixP010) {   // one plane of pairs: the group's start is pair 2 gx
        const int *first = FMT == kPixNV21 ? v : u, *second = FMT == kPixNV21 ? u : v;
        unsigned char *o = f.u + gy * f.pitch_c + 4 * gx * SB;
        if (cwide && whole) {
            if (ten) *(Dwords2 *)o = Dwords2{pack_words(first[0], second[0]), pack_words(first[1], second[1])};
            else *(unsigned *)o = pack_bytes(first[0], second[0], first[1], second[1]);
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (k >= ns) continue;
                if (ten) ((unsigned short *)o)[2 * k] = (unsigned short)first[k], ((unsigned short *)o)[2 * k + 1] = (unsigned short)second[k];
                else o[2 * k] = (unsigned char)first[k], o[2 * k + 1] = (unsigned char)second[k];
            }
        }
    } else {   // I420 / I010: a U and a V plane, the group's start is sample 2 gx of each
        const int off = gy * f.pitch_c + 2 * gx * SB;
        unsigned char *ou = f.u + off, *ov = f.v + off;
        if (cwide && whole) {   // (I420: cwide asks for even addresses only)
            if (ten) *(unsigned *)ou = pack_words(u[0], u[1]), *(unsigned *)ov = pack_words(v[0], v[1]);
            else *(unsigned short *)ou = (unsigned short)(u[0] | (u[1] << 8)), *(unsigned short *)ov = (unsigned short)(v[0] | (v[1] << 8));
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (k >= ns) continue;
                if (ten) ((unsigned short *)ou)[k] = (unsigned short)u[k], ((unsigned short *)ov)[k] = (unsigned short)v[k];
                else ou[k] = (unsigned char)u[k], ov[k] = (unsigned char)v[k];
            }
        }
    }
}

template <int FMT>
__device__ __forceinline__ void bgr_to_yuv_tile(const YuvOutFrame &f, int tx, int ty) {
    const int gx = tx * kYuvOutGroupsX + (threadIdx.x & (kYuvOutGroupsX - 1));
    const int gy = ty * (kYuvOutTileH / 2) + (threadIdx.x / kYuvOutGroupsX);
    if (4 * gx >= f.width || 2 * gy >= f.height) return;
    const bool planar = FMT == kPixI420 || FMT == kPixI010;
    const size_t chroma = (size_t)f.u | (unsigned)f.pitch_c | (planar ? (size_t)f.v : 0);
    const bool swide = ((((size_t)f.src) | (unsigned)f.spitch) & 3) == 0;
    const bool ywide = ((((size_t)f.y) | (unsigned)f.pitch_y) & 3) == 0;
    const bool cwide = (chroma & (FMT == kPixI420 ? 1 : 3)) == 0;
    bgr_to_yuv_group<FMT>(f, gx, gy, swide, ywide, cwide);
}

}  // namespace

__global__ __launch_bounds__(kYuvOutThreads) void bgr_to_yuv_kernel(YuvOutArgs a) {
    const int tile = blockIdx.x;
    YuvOutFrame frame = a.one;
    if (a.table) {   // the last frame whose first tile is not beyond this one
        int lo = 0, hi = a.nframes - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.table[mid].tile_start <= tile) lo = mid; else hi = mid - 1;
        }
        frame = a.table[lo];
    }
    const int local = tile - frame.tile_start, ty = local / frame.tiles_x, tx = local - ty * frame.tiles_x;
    switch (frame.format) {
    case kPixNV12: bgr_to_yuv_tile<kPixNV12>(frame, tx, ty); break;
    case kPixNV21: bgr_to_yuv_tile<kPixNV21>(frame, tx, ty); break;
    case kPixI420: bgr_to_yuv_tile<kPixI420>(frame, tx, ty); break;
    case kPixP010: bgr_to_yuv_tile<kPixP010>(frame, tx, ty); break;
    case kPixI010: bgr_to_yuv_tile<kPixI010>(frame, tx, ty); break;
    default: break;
    }
}

hipError_t launch_bgr_to_yuv(const YuvOutArgs &a, hipStream_t s) {
    if (a.nframes <= 0 || a.total_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(bgr_to_yuv_kernel, dim3((unsigned)a.total_tiles), dim3(kYuvOutThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace hrn
