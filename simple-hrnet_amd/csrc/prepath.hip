// Crop pre-path of SimpleHRNet.predict(), single image / multi-person (SimpleHRNet.py:236-278) and the stack path
// (SimpleHRNet.py:383-412), on the GPU: every frame crosses PCIe once as uint8 and every person's crop is cut, zero-padded,
// resized and normalised here, straight into the (n,3,H,W) fp32 batch the stem reads.  A person's record names its frame
// (base pointer, width, height), so the people of many frames -- of differing sizes -- go through one pair of launches.
//
// The resize is Pillow's (torchvision Resize on a PIL image = Image.resize(BILINEAR); libImaging/Resample.c):
//   two separable 8-bit passes, horizontal then vertical, rounded and clipped to uint8 in between;
//   per output sample: center = (xx + 0.5) * scale, support = max(scale, 1), taps [xmin, xmin + n),
//   weights = triangle((x + xmin - center + 0.5) / max(scale, 1)) normalised to sum 1 in double, then
//   22-bit fixed point: kk = (int)(0.5 + k * 2^22); sample = clip8((2^21 + sum src * kk) >> 22).
// The coefficients are recomputed per thread in double with the same operation order (fp contraction off), so the
// result is bit-identical to Pillow's; ToTensor / Normalize are the float32 operations torchvision performs
// (v / 255, then (x - mean) / std).  A pass whose size does not change is the identity, as in Pillow.
#include "kernels.h"
#include "resize_taps.h"
#include "yuv_px.h"

namespace hrn {

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

struct Taps {
    int xmin, n;
    double scale, support, ss;
};

#pragma clang fp contract(off)
__device__ __forceinline__ Taps taps_of(int xx, int in_size, int out_size) {
    Taps t;
    t.scale = (double)in_size / out_size;
    const double filterscale = t.scale < 1.0 ? 1.0 : t.scale;
    t.support = 1.0 * filterscale;
    t.ss = 1.0 / filterscale;
    const double center = (xx + 0.5) * t.scale;
    int xmin = (int)(center - t.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + t.support + 0.5);
    if (xmax > in_size) xmax = in_size;
    t.xmin = xmin, t.n = xmax - xmin;
    return t;
}

#pragma clang fp contract(off)
__device__ __forceinline__ double tri(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// weight k of output sample xx, normalised and quantised exactly as precompute_coeffs + normalize_coeffs_8bpc
#pragma clang fp contract(off)
__device__ __forceinline__ void weights_of(const Taps &t, int xx, double *ww_out) {
    const double center = (xx + 0.5) * t.scale;
    double ww = 0.0;
    for (int x = 0; x < t.n; ++x) ww += tri((x + t.xmin - center + 0.5) * t.ss);
    *ww_out = ww;
}
#pragma clang fp contract(off)
__device__ __forceinline__ int coeff(const Taps &t, int xx, int x, double ww) {
    const double center = (xx + 0.5) * t.scale;
    double k = tri((x + t.xmin - center + 0.5) * t.ss);
    if (ww != 0.0) k /= ww;
    return (int)(0.5 + k * (double)(1 << PRECISION_BITS));
}

__device__ __forceinline__ int clip8(int v) {
    v >>= PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// padded-crop pixel (y, x) of channel c (RGB order) -- zero in the padding, the person's BGR frame flipped elsewhere
__device__ __forceinline__ int crop_px(const CropParams &cp, int y, int x, int c) {
    const int yy = y - cp.pad_top, xx = x - cp.pad_left;
    if (yy < 0 || yy >= cp.h_crop || xx < 0 || xx >= cp.w_crop) return 0;
    return cp.frame[((size_t)(cp.y1 + yy) * cp.frame_w + cp.x1 + xx) * 3 + (2 - c)];
}

}  // namespace

// pass 1: rows of the padded crop -> W output columns (uint8 RGB, row-major [h_pad][W][3] per crop); every crop reads the
// frame its record names, so one launch serves the people of any number of frames, of any sizes
__global__ __launch_bounds__(256) void prepath_horizontal_kernel(const CropParams *crops, unsigned char *tmp, int W) {
    const CropParams cp = crops[blockIdx.y];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)cp.h_pad * W) return;
    const int y = (int)(idx / W), xx = (int)(idx - (long)y * W);
    unsigned char *o = tmp + cp.tmp_off + ((size_t)y * W + xx) * 3;
    if (cp.w_pad == W) {  // no horizontal pass in Pillow either
        for (int c = 0; c < 3; ++c) o[c] = (unsigned char)crop_px(cp, y, xx, c);
        return;
    }
    const Taps t = taps_of(xx, cp.w_pad, W);
    double ww;
    weights_of(t, xx, &ww);
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < t.n; ++x) {
        const int k = coeff(t, xx, x, ww);
        s0 += crop_px(cp, y, t.xmin + x, 0) * k;
        s1 += crop_px(cp, y, t.xmin + x, 1) * k;
        s2 += crop_px(cp, y, t.xmin + x, 2) * k;
    }
    o[0] = (unsigned char)clip8(s0), o[1] = (unsigned char)clip8(s1), o[2] = (unsigned char)clip8(s2);
}

// pass 2: h_pad rows -> H output rows, then ToTensor + Normalize into the (n,3,H,W) fp32 batch
__global__ __launch_bounds__(256) void prepath_vertical_kernel(const CropParams *crops, const unsigned char *tmp, float *images,
                                                               int H, int W) {
    const CropParams cp = crops[blockIdx.y];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int yy = (int)(idx / W), xx = (int)(idx - (long)yy * W);
    const unsigned char *src = tmp + cp.tmp_off;
    int v[3];
    if (cp.h_pad == H) {
        for (int c = 0; c < 3; ++c) v[c] = src[((size_t)yy * W + xx) * 3 + c];
    } else {
        const Taps t = taps_of(yy, cp.h_pad, H);
        double ww;
        weights_of(t, yy, &ww);
        int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
        for (int y = 0; y < t.n; ++y) {
            const int k = coeff(t, yy, y, ww);
            const unsigned char *px = src + ((size_t)(t.xmin + y) * W + xx) * 3;
            s0 += px[0] * k, s1 += px[1] * k, s2 += px[2] * k;
        }
        v[0] = clip8(s0), v[1] = clip8(s1), v[2] = clip8(s2);
    }
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};  // SimpleHRNet.py:171
    float *o = images + (size_t)blockIdx.y * 3 * H * W + (size_t)yy * W + xx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = (float)v[c] / 255.0f;           // ToTensor
        o[(size_t)c * H * W] = (x - mean[c]) / stdv[c];  // Normalize
    }
}

hipError_t launch_prepath(const CropParams *crops_dev, int n, int max_h_pad, unsigned char *tmp_dev, float *images_dev, int H, int W,
                          hipStream_t s) {
    constexpr int kMaxGridY = 65535;   // blockIdx.y is the crop: more people than that go out in slices
    for (int lo = 0; lo < n; lo += kMaxGridY) {
        const int nb = n - lo < kMaxGridY ? n - lo : kMaxGridY;
        dim3 g1((unsigned)(((long)max_h_pad * W + 255) / 256), nb);
        hipLaunchKernelGGL(prepath_horizontal_kernel, g1, dim3(256), 0, s, crops_dev + lo, tmp_dev, W);
        dim3 g2((unsigned)(((long)H * W + 255) / 256), nb);
        hipLaunchKernelGGL(prepath_vertical_kernel, g2, dim3(256), 0, s, crops_dev + lo, (const unsigned char *)tmp_dev,
                           images_dev + (size_t)lo * 3 * H * W, H, W);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// The same pre-path from 4:2:0 YCbCr frames (NV12 / I420), as decoders deliver them: the frame crosses PCIe at 1.5 bytes per
// pixel and is never converted as a whole.  A tap is read through the conversion of cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420):
// the chroma sample of a 2x2 block is shared (nearest), 20-bit fixed point in int32 (coef = y0, CY, CUB, CUG, CVG, CVR):
//   yy = max(0, Y - y0) * CY;  u = U - 128;  v = V - 128;  h = 1 << 19
//   B = clip8((yy + h + CUB*u) >> 20);  G = clip8((yy + h + CVG*v + CUG*u) >> 20);  R = clip8((yy + h + CVR*v) >> 20)
// Everything behind the tap is the BGR path's arithmetic, so a crop equals, bit for bit, the BGR path's crop of the converted
// frame (tests/yuv_ref.py restates the conversion; tests/test_yuv_gpu.py holds both equalities).
// NV21 (the pair is V, U) and the 10-bit layouts P010 / I010 (16-bit words, one rounding from the 10-bit samples: yuv_px.h) are
// further instantiations of the same body (tests/yuv10_ref.py, tests/test_yuv10_gpu.py).
namespace {

// (the conversion of one pixel: yuv_px.h, shared with letterbox.hip)
// padded-crop pixel (y, x), all three channels: RGB 0 in the padding (zero AFTER the conversion, as np.pad of the RGB crop)
template <int FMT>
__device__ __forceinline__ Rgb crop_px_yuv(const CropParams &cp, const YuvSource &ys, int y, int x) {
    const int yy = y - cp.pad_top, xx = x - cp.pad_left;
    if (yy < 0 || yy >= cp.h_crop || xx < 0 || xx >= cp.w_crop) return Rgb{0, 0, 0};
    return yuv_frame_px<FMT>(ys, cp.y1 + yy, cp.x1 + xx);
}

// prepath_horizontal_kernel's body for one output sample, its taps read from a frame of layout FMT
template <int FMT>
__device__ __forceinline__ void horizontal_yuv(const CropParams &cp, const YuvSource &ys, unsigned char *o, int y, int xx, int W) {
    if (cp.w_pad == W) {  // no horizontal pass in Pillow either
        const Rgb p = crop_px_yuv<FMT>(cp, ys, y, xx);
        o[0] = (unsigned char)p.r, o[1] = (unsigned char)p.g, o[2] = (unsigned char)p.b;
        return;
    }
    const Taps t = taps_of(xx, cp.w_pad, W);
    double ww;
    weights_of(t, xx, &ww);
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < t.n; ++x) {
        const int k = coeff(t, xx, x, ww);
        const Rgb p = crop_px_yuv<FMT>(cp, ys, y, t.xmin + x);
        s0 += p.r * k, s1 += p.g * k, s2 += p.b * k;
    }
    o[0] = (unsigned char)clip8(s0), o[1] = (unsigned char)clip8(s1), o[2] = (unsigned char)clip8(s2);
}

// four bytes at p (p + 3 readable): one dword where the address allows it
__device__ __forceinline__ unsigned load4(const unsigned char *p) {
    if (((size_t)p & 3) == 0) return *(const unsigned *)p;
    return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
}

}  // namespace

// pass 1 from YUV frames: the layout is the crop's (one crop per blockIdx.y, so the branch is uniform over the block)
__global__ __launch_bounds__(256) void prepath_horizontal_yuv_kernel(const CropParams *crops, const YuvSource *srcs, unsigned char *tmp,
                                                                    int W) {
    const CropParams cp = crops[blockIdx.y];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)cp.h_pad * W) return;
    const YuvSource ys = srcs[blockIdx.y];
    const int y = (int)(idx / W), xx = (int)(idx - (long)y * W);
    unsigned char *o = tmp + cp.tmp_off + ((size_t)y * W + xx) * 3;
    switch (ys.format) {
        case kPixNV12: horizontal_yuv<kPixNV12>(cp, ys, o, y, xx, W); break;
        case kPixI420: horizontal_yuv<kPixI420>(cp, ys, o, y, xx, W); break;
        case kPixNV21: horizontal_yuv<kPixNV21>(cp, ys, o, y, xx, W); break;
        case kPixP010: horizontal_yuv<kPixP010>(cp, ys, o, y, xx, W); break;
        case kPixI010: horizontal_yuv<kPixI010>(cp, ys, o, y, xx, W); break;
        default: o[0] = o[1] = o[2] = 0;   // (the host refuses every other value: nothing of such a frame is read)
    }
}

hipError_t launch_prepath_yuv(const CropParams *crops_dev, const YuvSource *src_dev, int n, int max_h_pad, unsigned char *tmp_dev,
                              float *images_dev, int H, int W, hipStream_t s) {
    constexpr int kMaxGridY = 65535;   // as launch_prepath
    for (int lo = 0; lo < n; lo += kMaxGridY) {
        const int nb = n - lo < kMaxGridY ? n - lo : kMaxGridY;
        dim3 g1((unsigned)(((long)max_h_pad * W + 255) / 256), nb);
        hipLaunchKernelGGL(prepath_horizontal_yuv_kernel, g1, dim3(256), 0, s, crops_dev + lo, src_dev + lo, tmp_dev, W);
        dim3 g2((unsigned)(((long)H * W + 255) / 256), nb);
        hipLaunchKernelGGL(prepath_vertical_kernel, g2, dim3(256), 0, s, crops_dev + lo, (const unsigned char *)tmp_dev,
                           images_dev + (size_t)lo * 3 * H * W, H, W);
    }
    return hipGetLastError();
}

// A whole frame to contiguous (height, width, 3) BGR, for the consumer that needs BGR (the detector).  One thread converts a
// run of 4 pixels of a row PAIR: 2 x 4 Y samples and the 2 chroma pairs they share, out as 2 x 12 bytes = three dword stores per
// row where the row's address allows it (always when width % 4 == 0), bytes otherwise and in a last run of 2 pixels.
// 8-bit layouts: 4 Y bytes per row and 4 (NV12 / NV21) or 2 x 2 (I420) chroma bytes.  10-bit layouts: 8 bytes of Y per row and
// 8 (P010) or 2 x 4 (I010) bytes of chroma, in dwords where the address is a multiple of 4, in 16-bit words otherwise (the host
// guarantees even addresses).  The output is 8-bit BGR whatever the layout.
constexpr int kYuvRun = 4;

namespace {
// four / two 16-bit words at p (an even address, the words readable)
__device__ __forceinline__ void load4w(const unsigned char *p, unsigned (&w)[4]) {
    if (((size_t)p & 3) == 0) {
        const unsigned a = ((const unsigned *)p)[0], b = ((const unsigned *)p)[1];
        w[0] = a & 0xffffu, w[1] = a >> 16, w[2] = b & 0xffffu, w[3] = b >> 16;
    } else {
        const unsigned short *q = (const unsigned short *)p;
        w[0] = q[0], w[1] = q[1], w[2] = q[2], w[3] = q[3];
    }
}
__device__ __forceinline__ void load2w(const unsigned char *p, unsigned (&w)[2]) {
    if (((size_t)p & 3) == 0) {
        const unsigned a = *(const unsigned *)p;
        w[0] = a & 0xffffu, w[1] = a >> 16;
    } else {
        const unsigned short *q = (const unsigned short *)p;
        w[0] = q[0], w[1] = q[1];
    }
}
}  // namespace

template <int FMT>
__global__ __launch_bounds__(256) void yuv_to_bgr_kernel(YuvSource ys, int height, int width, unsigned char *bgr) {
    constexpr bool T10 = yuv_is10<FMT>();
    const int runs = (width + kYuvRun - 1) / kYuvRun;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)(height / 2) * runs) return;
    const int yp = (int)(idx / runs), x0 = (int)(idx - (long)yp * runs) * kYuvRun;
    const int npx = width - x0 < kYuvRun ? width - x0 : kYuvRun;   // 4, or 2 at the end of a row (width is even)
    int U[2], V[2];
    if (FMT == kPixNV12 || FMT == kPixNV21) {
        const unsigned char *c = ys.u + (size_t)yp * ys.pitch_c + x0;
        if (npx == kYuvRun) {
            const unsigned q = load4(c);
            U[0] = q & 255, V[0] = (q >> 8) & 255, U[1] = (q >> 16) & 255, V[1] = q >> 24;
        } else {
            U[0] = U[1] = c[0], V[0] = V[1] = c[1];
        }
        if (FMT == kPixNV21) {   // the pair is (V, U)
            const int t0 = U[0], t1 = U[1];
            U[0] = V[0], U[1] = V[1], V[0] = t0, V[1] = t1;
        }
    } else if (FMT == kPixP010) {
        const unsigned char *c = ys.u + (size_t)yp * ys.pitch_c + 2 * x0;
        if (npx == kYuvRun) {
            unsigned w[4];
            load4w(c, w);
            U[0] = yuv_sample10<FMT>(w[0]), V[0] = yuv_sample10<FMT>(w[1]), U[1] = yuv_sample10<FMT>(w[2]), V[1] = yuv_sample10<FMT>(w[3]);
        } else {
            unsigned w[2];
            load2w(c, w);
            U[0] = U[1] = yuv_sample10<FMT>(w[0]), V[0] = V[1] = yuv_sample10<FMT>(w[1]);
        }
    } else if (FMT == kPixI010) {
        const size_t off = (size_t)yp * ys.pitch_c + x0;   // chroma column x0 / 2, two bytes each
        if (npx == kYuvRun) {
            unsigned wu[2], wv[2];
            load2w(ys.u + off, wu), load2w(ys.v + off, wv);
            U[0] = yuv_sample10<FMT>(wu[0]), U[1] = yuv_sample10<FMT>(wu[1]), V[0] = yuv_sample10<FMT>(wv[0]), V[1] = yuv_sample10<FMT>(wv[1]);
        } else {
            U[0] = U[1] = yuv_sample10<FMT>(*(const unsigned short *)(ys.u + off));
            V[0] = V[1] = yuv_sample10<FMT>(*(const unsigned short *)(ys.v + off));
        }
    } else {
        const size_t off = (size_t)yp * ys.pitch_c + (x0 >> 1);
        const int last = npx == kYuvRun ? 1 : 0;
        U[0] = ys.u[off], V[0] = ys.v[off], U[1] = ys.u[off + last], V[1] = ys.v[off + last];
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int fy = 2 * yp + r;
        const unsigned char *yrow = ys.y + (size_t)fy * ys.pitch_y + (T10 ? 2 : 1) * x0;
        unsigned char *o = bgr + ((size_t)fy * width + x0) * 3;
        if (npx == kYuvRun) {
            int Ys[4];
            if (T10) {
                unsigned w[4];
                load4w(yrow, w);
#pragma unroll
                for (int k = 0; k < 4; ++k) Ys[k] = yuv_sample10<FMT>(w[k]);
            } else {
                const unsigned q = load4(yrow);
#pragma unroll
                for (int k = 0; k < 4; ++k) Ys[k] = (q >> (8 * k)) & 255;
            }
            unsigned char px[12];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const Rgb p = yuv_rgb_of<FMT>(ys.coef, Ys[k], U[k >> 1], V[k >> 1]);
                px[3 * k] = (unsigned char)p.b, px[3 * k + 1] = (unsigned char)p.g, px[3 * k + 2] = (unsigned char)p.r;
            }
            if (((size_t)o & 3) == 0) {
                unsigned *o4 = (unsigned *)o;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    o4[k] = (unsigned)px[4 * k] | ((unsigned)px[4 * k + 1] << 8) | ((unsigned)px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) o[k] = px[k];
            }
        } else {
            for (int k = 0; k < npx; ++k) {
                const int Yk = T10 ? yuv_sample10<FMT>(((const unsigned short *)yrow)[k]) : (int)yrow[k];
                const Rgb p = yuv_rgb_of<FMT>(ys.coef, Yk, U[0], V[0]);
                o[3 * k] = (unsigned char)p.b, o[3 * k + 1] = (unsigned char)p.g, o[3 * k + 2] = (unsigned char)p.r;
            }
        }
    }
}

// (the host has refused every other layout: an unknown value launches nothing and is an error)
hipError_t launch_yuv_to_bgr(const YuvSource &src, int height, int width, unsigned char *bgr_dev, hipStream_t s) {
    const long threads = (long)(height / 2) * ((width + kYuvRun - 1) / kYuvRun);
    dim3 g((unsigned)((threads + 255) / 256));
    switch (src.format) {
        case kPixNV12: hipLaunchKernelGGL(yuv_to_bgr_kernel<kPixNV12>, g, dim3(256), 0, s, src, height, width, bgr_dev); break;
        case kPixI420: hipLaunchKernelGGL(yuv_to_bgr_kernel<kPixI420>, g, dim3(256), 0, s, src, height, width, bgr_dev); break;
        case kPixNV21: hipLaunchKernelGGL(yuv_to_bgr_kernel<kPixNV21>, g, dim3(256), 0, s, src, height, width, bgr_dev); break;
        case kPixP010: hipLaunchKernelGGL(yuv_to_bgr_kernel<kPixP010>, g, dim3(256), 0, s, src, height, width, bgr_dev); break;
        case kPixI010: hipLaunchKernelGGL(yuv_to_bgr_kernel<kPixI010>, g, dim3(256), 0, s, src, height, width, bgr_dev); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Single-person pre-path: cv2.resize(frame, (W, H), interpolation) + BGR -> RGB + ToTensor + Normalize
// (SimpleHRNet.py:213-222, 355-366) for 8-bit 3-channel frames.  OpenCV is a third-party dependency of the reference that is
// not in this image: the arithmetic below follows the published generic path of modules/imgproc/src/resize.cpp (fixed-point
// coefficients of 11 bits, int32 passes; see oracle/cv2_resize_oracle.py, which this kernel matches bit for bit) -- parity
// with cv2 itself is UNPINNED.  It is OpenCV's SCALAR path: the SIMD builds of the stock wheels run the cubic vertical pass in
// float32 (VResizeCubicVec_32s8u) and can differ from it by one grey level on some pixels;
// tests/golden/make_cv2_golden.py makes the pin wherever opencv-python is installed.
// Tap tables are formed on the device (no host staging): one thread per output column / row.
__global__ __launch_bounds__(256) void resize_taps_kernel(int src_w, int src_h, int W, int H, double scale_x, double scale_y,
                                                          int interp, ResizeTaps *taps) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= W + H) return;
    const bool is_x = t < W;
    // (the arithmetic: resize_taps.h, shared with letterbox.hip)
    taps[t] = resize_tap_of(is_x ? t : t - W, is_x ? src_w : src_h, is_x ? scale_x : scale_y, interp, is_x);
}

__global__ __launch_bounds__(256) void resize_frames_kernel(const unsigned char *frames, int src_h, int src_w, const ResizeTaps *taps,
                                                            int interp, float *images, int H, int W) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int yy = (int)(idx / W), xx = (int)(idx - (long)yy * W);
    const unsigned char *src = frames + (size_t)blockIdx.y * src_h * src_w * 3;
    const ResizeTaps tx = taps[xx], ty = taps[W + yy];
    const int K = interp == 2 ? 4 : interp == 1 ? 2 : 1;
    int hor[4][3];
    for (int r = 0; r < K; ++r) {
        int y = ty.ofs + r;
        y = y < 0 ? 0 : y > src_h - 1 ? src_h - 1 : y;                 // replicate border
        int s0 = 0, s1 = 0, s2 = 0;
        for (int k = 0; k < K; ++k) {
            int x = tx.ofs + k;
            x = x < 0 ? 0 : x > src_w - 1 ? src_w - 1 : x;
            const unsigned char *px = src + ((size_t)y * src_w + x) * 3;
            const int a = tx.c[k];
            s0 += px[0] * a, s1 += px[1] * a, s2 += px[2] * a;
        }
        hor[r][0] = s0, hor[r][1] = s1, hor[r][2] = s2;
    }
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int o;
        if (interp == 2) {        // VResizeCubic + FixedPtCast<int, uchar, 22>
            o = (hor[0][c] * ty.c[0] + hor[1][c] * ty.c[1] + hor[2][c] * ty.c[2] + hor[3][c] * ty.c[3] + (1 << 21)) >> 22;
        } else if (interp == 1) { // VResizeLinear<uchar, int, short>
            o = vresize_linear(ty.c[0], hor[0][c], ty.c[1], hor[1][c]);
        } else {
            o = hor[0][c] >> 11;
        }
        v[c] = o < 0 ? 0 : o > 255 ? 255 : o;
    }
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};  // SimpleHRNet.py:171
    float *o = images + (size_t)blockIdx.y * 3 * H * W + (size_t)yy * W + xx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = (float)v[2 - c] / 255.0f;       // BGR -> RGB, ToTensor
        o[(size_t)c * H * W] = (x - mean[c]) / stdv[c];  // Normalize
    }
}

hipError_t launch_resize_frames(const unsigned char *frames_dev, int n, int src_h, int src_w, int interp, ResizeTaps *taps_dev,
                                float *images_dev, int H, int W, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const double scale_x = resize_scale(W, src_w), scale_y = resize_scale(H, src_h);
    hipLaunchKernelGGL(resize_taps_kernel, dim3((W + H + 255) / 256), dim3(256), 0, s, src_w, src_h, W, H, scale_x, scale_y, interp, taps_dev);
    dim3 g((unsigned)(((long)H * W + 255) / 256), n);
    hipLaunchKernelGGL(resize_frames_kernel, g, dim3(256), 0, s, frames_dev, src_h, src_w, taps_dev, interp, images_dev, H, W);
    return hipGetLastError();
}

}  // namespace hrn
