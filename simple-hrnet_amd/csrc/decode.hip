// Heat-map to joint-coordinate kernels for gfx950: every decode of the head's arg-max (include/hrnet_mi355.h: hrn_forward,
// hrn_forward_refined, hrn_forward_flip_tta, hrn_refine_coords).
//
//   decode_kernel<MODE>   arg-max merge of the head's slab candidates (first maximum wins), the MODE offset of the arg-max read from
//                         the head's heat-maps (none for RF_NONE), then the box scaling in fp64, SimpleHRNet.py:297-308.
//   refine_coords_kernel  the same offset for integer (x, y) coordinates given by the caller (flip-TTA's averaged maps).
//   tta_decode_kernel     flip-TTA: average with the mirrored pass, arg-max, and (post_processing) the quarter-cell offset.
//
// The per-joint kernels run one thread per (crop, joint): ~4 k joints per 256-crop pass, DARK reads a 15 x 15 window each -- no LDS,
// no MFMA.
// QUARTER is get_final_preds's rule (misc/utils.py:154-175).
// DARK (Zhang et al., CVPR 2020) is evaluated in fp64: the 13 blurred values it needs, their logarithms, a Newton step.
#include "kernels.h"
#include "argmax.h"

namespace hrn {

// Offset (ox, oy), in cells, of the integer arg-max (px, py) of one h x w map; (0, 0) where the mode does not apply.
__device__ __forceinline__ void subpixel_offset(const float *hm, int h, int w, int px, int py, int mode, double &ox, double &oy) {
    ox = 0., oy = 0.;
    if (mode == RF_QUARTER) {
        if (1 < px && px < w - 1 && 1 < py && py < h - 1) {
            const float dx = hm[py * w + px + 1] - hm[py * w + px - 1];
            const float dy = hm[(py + 1) * w + px] - hm[(py - 1) * w + px];
            ox = dx > 0.f ? 0.25 : (dx < 0.f ? -0.25 : 0.);
            oy = dy > 0.f ? 0.25 : (dy < 0.f ? -0.25 : 0.);
        }
        return;
    }
    if (mode != RF_DARK || px < 2 || px > w - 3 || py < 2 || py > h - 3) return;
    // B = H blurred by the separable 11-tap Gaussian of sigma 2, g[k] = exp(-k^2 / 8) / sum (cv2.getGaussianKernel(11, 0)), H = 0
    // outside the map.  Only B at the 13 points |cx| + |cy| <= 2 around (px, py) is needed: b[cy + 2][cx + 2], from rows
    // py - 7 .. py + 7 blurred horizontally at columns px - 2 .. px + 2.
    double g[11], gs = 0.;
#pragma unroll
    for (int k = 0; k < 11; ++k) g[k] = exp(-(double)((k - 5) * (k - 5)) / 8.), gs += g[k];
#pragma unroll
    for (int k = 0; k < 11; ++k) g[k] /= gs;
    double b[5][5];
#pragma unroll
    for (int cy = 0; cy < 5; ++cy)
#pragma unroll
        for (int cx = 0; cx < 5; ++cx) b[cy][cx] = 0.;
#pragma unroll
    for (int r = -7; r <= 7; ++r) {
        const int y = py + r;
        if (y < 0 || y >= h) continue;
        const float *row = hm + (size_t)y * w;
        double v[15];   // columns px - 7 .. px + 7
#pragma unroll
        for (int c = 0; c < 15; ++c) {
            const int x = px - 7 + c;
            v[c] = x >= 0 && x < w ? (double)row[x] : 0.;
        }
#pragma unroll
        for (int cx = -2; cx <= 2; ++cx) {
            const int ay = 2 - (cx < 0 ? -cx : cx);   // the points of this column: |cy| <= ay; this row reaches those with |r - cy| <= 5
            if (r < -ay - 5 || r > ay + 5) continue;
            double rb = 0.;
#pragma unroll
            for (int k = 0; k < 11; ++k) rb += g[k] * v[cx + k + 2];
#pragma unroll
            for (int cy = -2; cy <= 2; ++cy)
                if ((cy < 0 ? -cy : cy) <= ay && r - cy >= -5 && r - cy <= 5) b[cy + 2][cx + 2] += g[r - cy + 5] * rb;
        }
    }
    // L = ln(max(B, 1e-10)) (a NaN stays NaN and then fails the definiteness test, as numpy's maximum would have it)
    double L[5][5];
#pragma unroll
    for (int cy = -2; cy <= 2; ++cy)
#pragma unroll
        for (int cx = -2; cx <= 2; ++cx) {
            const double x = b[cy + 2][cx + 2];
            L[cy + 2][cx + 2] = (cx < 0 ? -cx : cx) + (cy < 0 ? -cy : cy) <= 2 ? log(x < 1e-10 ? 1e-10 : x) : 0.;
        }
    const double dx = (L[2][3] - L[2][1]) / 2., dy = (L[3][2] - L[1][2]) / 2.;
    const double dxx = (L[2][4] - 2. * L[2][2] + L[2][0]) / 4., dyy = (L[4][2] - 2. * L[2][2] + L[0][2]) / 4.;
    const double dxy = (L[3][3] - L[1][3] - L[3][1] + L[1][1]) / 4.;
    const double det = dxx * dyy - dxy * dxy;
    if (!(dxx < 0. && det > 0.)) return;   // the Newton step only where L is concave (a maximum)
    const double sx = -(dyy * dx - dxy * dy) / det, sy = -(dxx * dy - dxy * dx) / det;
    ox = sx < -1. ? -1. : (sx > 1. ? 1. : sx);
    oy = sy < -1. ? -1. : (sy > 1. ? 1. : sy);
}

// Decode (SimpleHRNet.py:297-308): merge the slab candidates (lowest flat index among equal maxima = np.argmax), move the arg-max
// by the MODE offset, then  y = (py + oy) * 1. / h * (y2 - y1) + y1,  x = (px + ox) * 1. / w * (x2 - x1) + x1  evaluated in float64
// exactly as numpy does (box difference first, in the boxes' own dtype), stored as fp32.  The offset keeps its own fp contraction
// (subpixel_offset is outside this kernel's contract(off)).  Launch bounds: 1024 (the default) for RF_NONE, 64 for the refined modes.
template <int MODE>
__global__ __launch_bounds__(MODE == RF_NONE ? 1024 : 64) void decode_kernel(const DecodeArgs p) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.n * p.joints) return;
    const int n = t / p.joints;
    float v = -INFINITY;
    int i = kNoIdx;
    for (int s = 0; s < p.slabs; ++s) {
        const float ov = p.part_val[(size_t)t * p.slabs + s];
        const int oi = p.part_idx[(size_t)t * p.slabs + s];
        if (better(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
    if (i == kNoIdx) i = 0;  // (unreachable with h*w >= 1; never form coordinates from the sentinel)
    const int py = i / p.w, px = i - py * p.w;
    double ox = 0., oy = 0.;
    if constexpr (MODE != RF_NONE) subpixel_offset(p.heatmaps + (size_t)t * p.h * p.w, p.h, p.w, px, py, MODE, ox, oy);
    double x1, y1, dx, dy;
    if (p.box_is_float) {
        const float *b = (const float *)p.boxes + 4 * (size_t)n;
        x1 = b[0], y1 = b[1];
        dx = (double)(b[2] - b[0]);  // fp32 subtraction first, like numpy float32 scalars
        dy = (double)(b[3] - b[1]);
    } else {
        const int *b = (const int *)p.boxes + 4 * (size_t)n;
        x1 = b[0], y1 = b[1];
        dx = (double)(b[2] - b[0]);
        dy = (double)(b[3] - b[1]);
    }
    float *o = p.pts + (size_t)t * 3;
    o[0] = (float)(((double)py + oy) * 1. / (double)p.h * dy + y1);
    o[1] = (float)(((double)px + ox) * 1. / (double)p.w * dx + x1);
    o[2] = v;
}

__global__ __launch_bounds__(64) void refine_coords_kernel(const DecodeArgs p) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.n * p.joints) return;
    float *c = p.coords + (size_t)t * 2;
    const float x = c[0], y = c[1];
    if (!(x >= 0.f && x <= (float)(p.w - 1) && y >= 0.f && y <= (float)(p.h - 1))) return;   // off the map (or NaN): unchanged
    double ox, oy;
    subpixel_offset(p.heatmaps + (size_t)t * p.h * p.w, p.h, p.w, (int)x, (int)y, p.mode, ox, oy);
    c[0] = (float)((double)x + ox);
    c[1] = (float)((double)y + oy);
}

// RF_NONE: 128-thread blocks.  QUARTER / DARK: 64-thread blocks, so that a 256-crop pass of 17 joints spreads over 68 CUs instead of 34.
hipError_t launch_decode(const DecodeArgs &a, hipStream_t s) {
    if (a.mode != RF_NONE && !a.heatmaps) return hipErrorInvalidValue;   // the offset reads the maps the head wrote
    const int total = a.n * a.joints;
    if (total <= 0) return hipSuccess;
    if (a.mode == RF_NONE)
        hipLaunchKernelGGL(decode_kernel<RF_NONE>, dim3((total + 127) / 128), dim3(128), 0, s, a);
    else if (a.mode == RF_QUARTER)
        hipLaunchKernelGGL(decode_kernel<RF_QUARTER>, dim3((total + 63) / 64), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL(decode_kernel<RF_DARK>, dim3((total + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_refine_coords(const DecodeArgs &a, hipStream_t s) {
    const int total = a.n * a.joints;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(refine_coords_kernel, dim3((total + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}

// Flip-TTA combine + decode (testing/Test.py:134-140, misc/utils.py:19-29, 125-175): per (crop, joint)
//   avg = (hm[j] + mirror(hm_flipped[pair(j)])) * 0.5     written back over hm
//   (max, first arg-max) of avg -> x = idx % w, y = idx / w, zeroed when max <= 0   (get_max_preds)
//   post_processing: +-0.25 px towards the higher neighbour when 1 < x < w-1 and 1 < y < h-1   (get_final_preds)
__global__ __launch_bounds__(256) void tta_decode_kernel(const TtaArgs p) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int j = blockIdx.x, n = blockIdx.y, hw = p.h * p.w;
    float *hm = p.hm + ((size_t)n * p.joints + j) * hw;
    const float *hf = p.hm_flipped + ((size_t)n * p.joints + p.pair[j]) * hw;
    float bv = -INFINITY;
    int bi = kNoIdx;
    for (int px = threadIdx.x; px < hw; px += 256) {
        const int y = px / p.w, x = px - y * p.w;
        const float v = (hm[px] + hf[y * p.w + (p.w - 1 - x)]) * 0.5f;
        hm[px] = v;
        if (takes(v, bv, bi)) bv = v, bi = px;  // px grows: strict > keeps the first maximum
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (better(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = bv, si[threadIdx.x >> 6] = bi;
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (better(sv[w], si[w], bv, bi)) bv = sv[w], bi = si[w];
        float x = (float)(bi % p.w), y = (float)(bi / p.w);
        if (!(bv > 0.f)) x = 0.f, y = 0.f;
        if (p.post_processing) {   // x, y are integer valued: x + ox in fp64 rounds to x + 0.25f, bit for bit
            double ox, oy;
            subpixel_offset(hm, p.h, p.w, (int)x, (int)y, RF_QUARTER, ox, oy);
            x = (float)((double)x + ox), y = (float)((double)y + oy);
        }
        p.preds[((size_t)n * p.joints + j) * 2 + 0] = x;
        p.preds[((size_t)n * p.joints + j) * 2 + 1] = y;
        p.maxvals[(size_t)n * p.joints + j] = bv;
    }
}

hipError_t launch_tta_decode(const TtaArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(tta_decode_kernel, dim3(a.joints, a.n), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace hrn
