// The detector link on the GPU (include/hrnet_mi355.h: hrn_letterbox_frames, hrn_letterbox_frames_yuv,
// hrn_detections_to_frame_dev): what the reference runs on the host around its person detector.
//
//   letterbox_kernel        frames (BGR or YUV 4:2:0, 8- or 10-bit, of differing sizes) -> the detector tensor, ONE launch for all frames of a
//                           call (blockIdx.y = frame).  An interior pixel is cv2.resize(INTER_LINEAR)'s: resize_taps.h's window
//                           per axis, computed by the thread (two short double expressions: no tap table, no scratch, no second
//                           launch), the 2 x 2 taps, VResizeLinear -- bit for bit resize_frames_kernel with interp == 1 -- or a
//                           copy when the size does not change, or the 2 x 2 mean (a + b + c + d + 2) >> 2 when the frame is
//                           exactly twice the resized size in both axes (cv2's INTER_AREA fast path, restated from resize.cpp
//                           without a cv2 build to check against: UNPINNED like the other cv2 paths).  A padding pixel takes pad[c]
//                           and reads no frame byte.
//                           Thread -> pixel map: x fastest.  Planar float forms: one pixel per thread, so a wave stores 64
//                           consecutive elements of each plane.  HRN_LB_U8_HWC: four pixels per thread = 12 bytes = three dword
//                           stores where the address allows it (as yuv_to_bgr_kernel), bytes otherwise.
//   detections_kernel       one 256-thread block per frame: status per row, the inverse of letterbox_math.h on kept rows, zero rows
//                           for the others; with compaction the kept rows of a frame move to the front in their order (ballot +
//                           prefix count, chunk by chunk with a running base, as assoc.hip numbers new people).
// No atomics; every byte has one writer.
#include <hip/hip_runtime.h>

#include "elem.h"
#include "kernels.h"
#include "letterbox_math.h"
#include "resize_taps.h"
#include "yuv_px.h"

namespace hrn {

namespace {

constexpr int kSrcBgr = 0;   // the frame's layout: HRN_PIX_BGR; yuv_px.h's kPix* are the others

struct Bgr {
    int b, g, r;
};

template <int SRC>
__device__ __forceinline__ Bgr lb_src_px(const LetterboxFrame &f, int y, int x) {
    if constexpr (SRC == kSrcBgr) {
        const unsigned char *px = f.bgr + ((size_t)y * f.src_w + x) * 3;
        return Bgr{px[0], px[1], px[2]};
    } else {
        const Rgb p = yuv_frame_px<SRC>(f.yuv, y, x);
        return Bgr{p.b, p.g, p.r};
    }
}

// interior pixel (dy, dx) of the resized frame, 0 <= dy < new_h, 0 <= dx < new_w
template <int SRC>
__device__ __forceinline__ Bgr lb_interior(const LetterboxFrame &f, int dy, int dx) {
    if (f.mode == LB_MODE_COPY) return lb_src_px<SRC>(f, dy, dx);
    if (f.mode == LB_MODE_AREA) {   // src == 2 * new in both axes: rows 2 dy, 2 dy + 1 and columns 2 dx, 2 dx + 1 exist
        const Bgr a = lb_src_px<SRC>(f, 2 * dy, 2 * dx), b = lb_src_px<SRC>(f, 2 * dy, 2 * dx + 1);
        const Bgr c = lb_src_px<SRC>(f, 2 * dy + 1, 2 * dx), d = lb_src_px<SRC>(f, 2 * dy + 1, 2 * dx + 1);
        return Bgr{(a.b + b.b + c.b + d.b + 2) >> 2, (a.g + b.g + c.g + d.g + 2) >> 2, (a.r + b.r + c.r + d.r + 2) >> 2};
    }
    const ResizeTaps tx = resize_tap_of(dx, f.src_w, f.scale_x, 1, true), ty = resize_tap_of(dy, f.src_h, f.scale_y, 1, false);
    int hor[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        int y = ty.ofs + r;
        y = y < 0 ? 0 : y > f.src_h - 1 ? f.src_h - 1 : y;                 // replicate border
        int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            int x = tx.ofs + k;
            x = x < 0 ? 0 : x > f.src_w - 1 ? f.src_w - 1 : x;
            const Bgr p = lb_src_px<SRC>(f, y, x);
            const int a = tx.c[k];
            s0 += p.b * a, s1 += p.g * a, s2 += p.r * a;
        }
        hor[r][0] = s0, hor[r][1] = s1, hor[r][2] = s2;
    }
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int o = vresize_linear(ty.c[0], hor[0][c], ty.c[1], hor[1][c]);
        v[c] = o < 0 ? 0 : o > 255 ? 255 : o;
    }
    return Bgr{v[0], v[1], v[2]};
}

// output pixel (y, x) in OUTPUT channel order
template <int SRC>
__device__ __forceinline__ void lb_pixel(const LetterboxArgs &a, const LetterboxFrame &f, int y, int x, int v[3]) {
    const int dy = y - f.top, dx = x - f.left;
    if (dy < 0 || dy >= f.new_h || dx < 0 || dx >= f.new_w) {   // padding: no frame byte is read
        v[0] = a.pad[0], v[1] = a.pad[1], v[2] = a.pad[2];
        return;
    }
    const Bgr p = lb_interior<SRC>(f, dy, dx);
    if (a.order == 0) v[0] = p.r, v[1] = p.g, v[2] = p.b;   // HRN_LB_RGB
    else v[0] = p.b, v[1] = p.g, v[2] = p.r;
}

template <int FORM>
__device__ __forceinline__ void lb_store(void *base, size_t idx, float x);
template <>
__device__ __forceinline__ void lb_store<0>(void *base, size_t idx, float x) { ((float *)base)[idx] = x; }
template <>
__device__ __forceinline__ void lb_store<1>(void *base, size_t idx, float x) { ((unsigned short *)base)[idx] = Tr<DT_F16>::st(x); }
template <>
__device__ __forceinline__ void lb_store<2>(void *base, size_t idx, float x) { ((unsigned short *)base)[idx] = Tr<DT_BF16>::st(x); }


// FORM = HRN_LB_F32 / _F16 / _BF16: (n, 3, out_h, out_w) planar, one pixel per thread
template <int FORM, int SRC>
__device__ __forceinline__ void letterbox_planar(const LetterboxArgs &a, const LetterboxFrame &f, long idx, long plane) {
    const int y = (int)(idx / a.out_w), x = (int)(idx - (long)y * a.out_w);
    int v[3];
    lb_pixel<SRC>(a, f, y, x, v);
    const size_t o = (size_t)blockIdx.y * 3 * plane + (size_t)idx;
#pragma unroll
    for (int c = 0; c < 3; ++c) lb_store<FORM>(a.out, o + (size_t)c * plane, (float)v[c] / 255.0f);   // ToTensor: true division
}

// HRN_LB_U8_HWC: (n, out_h, out_w, 3), a run of four pixels of a row per thread
constexpr int kLbRun = 4;
template <int SRC>
__device__ __forceinline__ void letterbox_u8(const LetterboxArgs &a, const LetterboxFrame &f, long idx, int runs) {
    const int y = (int)(idx / runs), x0 = (int)(idx - (long)y * runs) * kLbRun;
    const int npx = a.out_w - x0 < kLbRun ? a.out_w - x0 : kLbRun;
    unsigned char px[3 * kLbRun];
#pragma unroll
    for (int k = 0; k < kLbRun; ++k) {
        int v[3] = {0, 0, 0};
        if (k < npx) lb_pixel<SRC>(a, f, y, x0 + k, v);
        px[3 * k] = (unsigned char)v[0], px[3 * k + 1] = (unsigned char)v[1], px[3 * k + 2] = (unsigned char)v[2];
    }
    unsigned char *o = (unsigned char *)a.out + (((size_t)blockIdx.y * a.out_h + y) * a.out_w + x0) * 3;
    if (npx == kLbRun && ((size_t)o & 3) == 0) {
        unsigned *o4 = (unsigned *)o;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = (unsigned)px[4 * k] | ((unsigned)px[4 * k + 1] << 8) | ((unsigned)px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * npx; ++k) o[k] = px[k];
    }
}

}  // namespace

// One kernel per (form, kind of frames).  YUV frames of all five layouts (NV12, I420, NV21, P010, I010) may share a call: the
// branch on the frame's layout is uniform over a block (blockIdx.y is the frame).  KIND: kLbBgr; kLbYuv8 -- every frame of the
// call is NV12 or I420: the two-way kernel, with the registers and the occupancy it has always had; kLbYuvAny -- some frame has one
// of the other layouts: the five-way kernel (the 10-bit bodies cost the u8 form 13 VGPRs and two waves of occupancy).  The host has
// refused every other value of `format`: such a frame writes nothing.
constexpr int kLbBgr = 0, kLbYuv8 = 1, kLbYuvAny = 2;

template <int FORM, int KIND>
__global__ __launch_bounds__(256) void letterbox_kernel(LetterboxArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const LetterboxFrame &f = a.n == 1 ? a.one : a.table[blockIdx.y];
    if (FORM == 3) {   // HRN_LB_U8_HWC
        const int runs = (a.out_w + kLbRun - 1) / kLbRun;
        if (idx >= (long)a.out_h * runs) return;
        if (KIND == kLbBgr) {
            letterbox_u8<kSrcBgr>(a, f, idx, runs);
        } else if (KIND == kLbYuv8) {
            if (f.yuv.format == kPixNV12) letterbox_u8<kPixNV12>(a, f, idx, runs);
            else if (f.yuv.format == kPixI420) letterbox_u8<kPixI420>(a, f, idx, runs);
        } else {
            switch (f.yuv.format) {
                case kPixNV12: letterbox_u8<kPixNV12>(a, f, idx, runs); break;
                case kPixI420: letterbox_u8<kPixI420>(a, f, idx, runs); break;
                case kPixNV21: letterbox_u8<kPixNV21>(a, f, idx, runs); break;
                case kPixP010: letterbox_u8<kPixP010>(a, f, idx, runs); break;
                case kPixI010: letterbox_u8<kPixI010>(a, f, idx, runs); break;
                default: break;
            }
        }
    } else {
        const long plane = (long)a.out_h * a.out_w;
        if (idx >= plane) return;
        constexpr int F = FORM == 3 ? 0 : FORM;
        if (KIND == kLbBgr) {
            letterbox_planar<F, kSrcBgr>(a, f, idx, plane);
        } else if (KIND == kLbYuv8) {
            if (f.yuv.format == kPixNV12) letterbox_planar<F, kPixNV12>(a, f, idx, plane);
            else if (f.yuv.format == kPixI420) letterbox_planar<F, kPixI420>(a, f, idx, plane);
        } else {
            switch (f.yuv.format) {
                case kPixNV12: letterbox_planar<F, kPixNV12>(a, f, idx, plane); break;
                case kPixI420: letterbox_planar<F, kPixI420>(a, f, idx, plane); break;
                case kPixNV21: letterbox_planar<F, kPixNV21>(a, f, idx, plane); break;
                case kPixP010: letterbox_planar<F, kPixP010>(a, f, idx, plane); break;
                case kPixI010: letterbox_planar<F, kPixI010>(a, f, idx, plane); break;
                default: break;
            }
        }
    }
}

namespace {
template <int KIND>
void launch_letterbox_kind(const LetterboxArgs &a, hipStream_t s) {
    const long threads = a.form == 3 ? (long)a.out_h * ((a.out_w + kLbRun - 1) / kLbRun) : (long)a.out_h * a.out_w;
    const dim3 g((unsigned)((threads + 255) / 256), (unsigned)a.n);
    switch (a.form) {
        case 0: hipLaunchKernelGGL((letterbox_kernel<0, KIND>), g, dim3(256), 0, s, a); break;
        case 1: hipLaunchKernelGGL((letterbox_kernel<1, KIND>), g, dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL((letterbox_kernel<2, KIND>), g, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((letterbox_kernel<3, KIND>), g, dim3(256), 0, s, a);
    }
}
}  // namespace

// a.yuv: 0 -- BGR frames; 1 -- YUV frames, all NV12 or I420; 2 -- YUV frames of any of the five layouts
hipError_t launch_letterbox(const LetterboxArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.yuv == 2) launch_letterbox_kind<kLbYuvAny>(a, s);
    else if (a.yuv) launch_letterbox_kind<kLbYuv8>(a, s);
    else launch_letterbox_kind<kLbBgr>(a, s);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void detections_kernel(DetArgs a, DetFrame one, DetFilter q) {
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const DetFrame f = a.P == 1 ? one : a.table[blockIdx.x];
    const int ds = q.det_stride;
    int base = 0;   // kept rows of the chunks before this one: the same in every thread
    for (int i0 = 0; i0 < f.n; i0 += 256) {
        const int i = i0 + tid;
        const bool in = i < f.n;
        const float *row = a.dets + (size_t)(f.first + (in ? i : 0)) * ds;
        const int st = in ? det_status(row, q) : DET_BELOW;
        const bool kept = in && st == DET_KEPT;
        const unsigned long long ballot = __ballot(kept);
        if (lane == 0) s_cnt[wave] = __popcll(ballot);
        __syncthreads();
        int rank = __popcll(ballot & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) rank += s_cnt[w];
            total += s_cnt[w];
        }
        if (in) {
            a.status[f.first + i] = st;
            if (kept) {
                det_map_row(row, f, ds, a.out + (size_t)(f.first + (a.compact ? base + rank : i)) * ds);
            } else if (!a.compact) {
                float *o = a.out + (size_t)(f.first + i) * ds;
                for (int k = 0; k < ds; ++k) o[k] = 0.0f;
            }
        }
        base += total;
        __syncthreads();   // s_cnt is rewritten by the next chunk
    }
    if (a.compact) {      // the zero rows behind the kept ones
        float *o = a.out + (size_t)(f.first + base) * ds;
        const long cells = (long)(f.n - base) * ds;
        for (long k = tid; k < cells; k += 256) o[k] = 0.0f;
    }
    if (tid == 0) a.counts[blockIdx.x] = base;
}

hipError_t launch_detections_to_frame(const DetArgs &a, const DetFrame &one, const DetFilter &q, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    hipLaunchKernelGGL(detections_kernel, dim3((unsigned)a.P), dim3(256), 0, s, a, one, q);
    return hipGetLastError();
}

}  // namespace hrn
