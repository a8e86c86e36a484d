// Frame rotation on the GPU (include/hrnet_mi355.h: hrn_rotate_frames, hrn_rotate_people_dev): cv2.rotate -- a pure permutation of
// elements -- for BGR, NV12 / NV21, I420 and 10-bit P010 / I010 frames, and people between the two orientations.
//
//   rotate_kernel          ONE launch for all planes of all frames of a call: one 256-thread block per 64 x 64-element tile of a
//                          plane (64 x 16 at 180 degrees), found by binary search in the call's plane table (one frame: its planes sit in the kernel
//                          arguments).  An element is 1 byte (Y, U, V), 2 (NV12's UV / NV21's VU pair; a 10-bit Y, U or V word), 3 (a BGR
//                          pixel) or 4 (P010's UV word pair), its bytes kept in order -- so a 10-bit word travels with all 16 bits.
//                          90 degrees: the tile's source rows go into LDS as they lie -- coalesced, in dwords when the plane's
//                          base and pitch are multiples of 4 (a tile's first column is a multiple of 64 elements, so its rows then
//                          start on a dword), in bytes otherwise and for a row's last bytes.  A thread then gathers four elements
//                          of one destination row -- four LDS rows, one column -- and stores them as `es` dwords (aligned likewise:
//                          destination tiles start at multiples of 64 columns), or in bytes.  The LDS pitch is 64 es + 4 bytes, an
//                          ODD number of dwords: the four-row steps of neighbouring threads fall on 8 banks, two threads each.
//                          Tiles are anchored where alignment matters: on the source's columns and on the destination's columns
//                          (for a quarter turn these are different axes of the tile); rows need none.
//                          180 degrees needs no LDS: a thread loads four consecutive elements of a source row (dwords when base,
//                          pitch and the row's bytes are multiples of 4), reverses the ELEMENTS in registers and stores them.
//                          Nothing outside a plane's rows is read or written: a dword is used only where all four bytes are
//                          elements of the row.  Offsets inside a plane are 32-bit (the host refuses pitch * rows >= 2^31).
//   rotate_people_kernel   one thread per joint and per box: rotate_math.h's arithmetic, the host form's text.
// No atomics; every byte has one writer.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "rotate_math.h"

namespace hrn {

namespace {

constexpr int kRotThreads = 256;

// four elements (ne of them real) to `o`: es dwords when all four are there and the address allows it, bytes otherwise
template <int ES>
__device__ __forceinline__ void rot_store_group(unsigned char *o, const unsigned char (&px)[4 * ES], int ne, bool wide) {
    if (wide && ne == 4) {
        unsigned *o4 = (unsigned *)o;
#pragma unroll
        for (int k = 0; k < ES; ++k)
            o4[k] = (unsigned)px[4 * k] | ((unsigned)px[4 * k + 1] << 8) | ((unsigned)px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4 * ES; ++k)
            if (k < ne * ES) o[k] = px[k];
    }
}

// codes 0 and 2.  Tile (tx, ty): destination columns j0 .. j0 + th - 1 (= th source rows) of the destination rows that the
// source columns c0 .. c0 + tw - 1 become.
template <int ES>
__device__ __forceinline__ void rotate90_tile(const RotPlane &p, int tx, int ty, unsigned *lds32) {
    constexpr int LP = kRotTile * ES + 4;   // LDS bytes between the tile's rows: LP / 4 is odd
    unsigned char *lds = (unsigned char *)lds32;
    const int tid = threadIdx.x;
    const int j0 = tx * kRotTile, th = min(kRotTile, p.hs - j0);
    const int c0 = ty * kRotTile, tw = min(kRotTile, p.ws - c0);
    const int rs0 = p.code == 0 ? p.hs - j0 - th : j0;   // the tile's first source row
    const int nb = tw * ES;                               // bytes of a source row inside the tile
    const unsigned char *s0 = p.src + rs0 * p.spitch + c0 * ES;
    const bool swide = ((((size_t)p.src) | (unsigned)p.spitch) & 3) == 0;
    const int ndw = swide ? nb >> 2 : 0;
    for (int idx = tid; idx < th * ndw; idx += kRotThreads) {
        const int r = idx / ndw, d = idx - r * ndw;
        lds32[r * (LP / 4) + d] = *(const unsigned *)(s0 + r * p.spitch + 4 * d);
    }
    const int rest = nb - 4 * ndw;
    for (int idx = tid; idx < th * rest; idx += kRotThreads) {
        const int r = idx / rest, k = 4 * ndw + (idx - r * rest);
        lds[r * LP + k] = s0[r * p.spitch + k];
    }
    __syncthreads();
    const bool dwide = ((((size_t)p.dst) | (unsigned)p.dpitch) & 3) == 0;
    const int ng = (th + 3) >> 2;
    for (int idx = tid; idx < tw * ng; idx += kRotThreads) {
        const int c = idx / ng, g = idx - c * ng;
        const int ne = min(4, th - 4 * g);
        unsigned char px[4 * ES];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int jl = 4 * g + e;
            const int jc = min(jl, th - 1);                   // (an element beyond the tile is not read: its address stays inside)
            const int rl = p.code == 0 ? th - 1 - jc : jc;   // dst(i, j) = src(Hs-1-j, i)  /  src(j, Ws-1-i)
#pragma unroll
            for (int b = 0; b < ES; ++b) px[e * ES + b] = e < ne ? lds[rl * LP + c * ES + b] : (unsigned char)0;
        }
        const int i = p.code == 0 ? c0 + c : p.ws - 1 - c0 - c;
        rot_store_group<ES>(p.dst + i * p.dpitch + (j0 + 4 * g) * ES, px, ne, dwide);
    }
}

// code 1.  Tile (tx, ty): 64 destination columns j0 .. of the 16 rows i0 .. -- one four-element group per thread, four times the
// blocks of a square tile: nothing is shared here, and a 1080p frame alone then fills the machine; dst(i, j) = src(Hs-1-i, Ws-1-j)
template <int ES>
__device__ __forceinline__ void rotate180_tile(const RotPlane &p, int tx, int ty) {
    const int tid = threadIdx.x;
    const int j0 = tx * kRotTile, tw = min(kRotTile, p.ws - j0);
    const int i0 = ty * kRotRows180, th = min(kRotRows180, p.hs - i0);
    const bool swide = ((((size_t)p.src) | (unsigned)p.spitch | (unsigned)(p.ws * ES)) & 3) == 0;
    const bool dwide = ((((size_t)p.dst) | (unsigned)p.dpitch) & 3) == 0;
    const int ng = (tw + 3) >> 2;
    for (int idx = tid; idx < th * ng; idx += kRotThreads) {
        const int r = idx / ng, g = idx - r * ng;
        const int j = j0 + 4 * g, ne = min(4, p.ws - j);
        const int i = i0 + r;
        const unsigned char *srow = p.src + (p.hs - 1 - i) * p.spitch;
        unsigned char px[4 * ES];
        if (swide && ne == 4) {   // the source elements Ws-j-4 .. Ws-j-1 in whole dwords, reversed element by element
            const unsigned *s4 = (const unsigned *)(srow + (p.ws - j - 4) * ES);
            unsigned char in[4 * ES];
#pragma unroll
            for (int k = 0; k < ES; ++k) {
                const unsigned v = s4[k];
                in[4 * k] = (unsigned char)v, in[4 * k + 1] = (unsigned char)(v >> 8);
                in[4 * k + 2] = (unsigned char)(v >> 16), in[4 * k + 3] = (unsigned char)(v >> 24);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int b = 0; b < ES; ++b) px[e * ES + b] = in[(3 - e) * ES + b];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int b = 0; b < ES; ++b) px[e * ES + b] = e < ne ? srow[(p.ws - 1 - j - e) * ES + b] : (unsigned char)0;
        }
        rot_store_group<ES>(p.dst + i * p.dpitch + j * ES, px, ne, dwide);
    }
}

}  // namespace

__global__ __launch_bounds__(kRotThreads) void rotate_kernel(RotArgs a) {
    __shared__ unsigned lds32[kRotTile * (kRotTile * 4 + 4) / 4];   // the widest element: 4 bytes
    const int tile = blockIdx.x;
    RotPlane p;
    if (a.table) {   // the last plane whose first tile is not beyond this one
        int lo = 0, hi = a.nplanes - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.table[mid].tile_start <= tile) lo = mid; else hi = mid - 1;
        }
        p = a.table[lo];
    } else {
        p = a.one[0];
        if (a.nplanes > 1 && tile >= a.one[1].tile_start) p = a.one[1];
        if (a.nplanes > 2 && tile >= a.one[2].tile_start) p = a.one[2];
    }
    const int local = tile - p.tile_start, ty = local / p.tiles_x, tx = local - ty * p.tiles_x;
    if (p.code == 1) {
        if (p.es == 1) rotate180_tile<1>(p, tx, ty);
        else if (p.es == 2) rotate180_tile<2>(p, tx, ty);
        else if (p.es == 3) rotate180_tile<3>(p, tx, ty);
        else if (p.es == 4) rotate180_tile<4>(p, tx, ty);
    } else {
        if (p.es == 1) rotate90_tile<1>(p, tx, ty, lds32);
        else if (p.es == 2) rotate90_tile<2>(p, tx, ty, lds32);
        else if (p.es == 3) rotate90_tile<3>(p, tx, ty, lds32);
        else if (p.es == 4) rotate90_tile<4>(p, tx, ty, lds32);
    }
}

hipError_t launch_rotate(const RotArgs &a, hipStream_t s) {
    if (a.nplanes <= 0 || a.total_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(rotate_kernel, dim3((unsigned)a.total_tiles), dim3(kRotThreads), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void rotate_people_kernel(RotPeopleArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long joints = a.pts ? (long)a.n * a.J : 0;
    const long total = joints + (a.boxes ? a.n : 0);
    if (idx >= total) return;
    const bool joint = idx < joints;
    const int i = joint ? (int)(idx / a.J) : (int)(idx - joints);
    const int hs = a.frame_hw ? a.frame_hw[2 * (size_t)i] : a.hs, ws = a.frame_hw ? a.frame_hw[2 * (size_t)i + 1] : a.ws;
    const int code = a.codes ? a.codes[i] : a.code;
    if (joint) rotate_joint(code, hs, ws, a.pts + (size_t)idx * 3, a.pts_out + (size_t)idx * 3);
    else rotate_box(code, hs, ws, a.boxes + (size_t)i * 4, a.boxes_out + (size_t)i * 4);
}

hipError_t launch_rotate_people(const RotPeopleArgs &a, hipStream_t s) {
    const long total = (a.pts ? (long)a.n * a.J : 0) + (a.boxes ? a.n : 0);
    if (a.n <= 0 || total <= 0) return hipSuccess;
    hipLaunchKernelGGL(rotate_people_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace hrn
