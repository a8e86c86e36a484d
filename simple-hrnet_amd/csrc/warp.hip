// Evaluation pre-path (testing/Test.py through datasets/COCO.py:290-304, misc/utils.py:99-107) on the GPU: every person is
// cut out of its uint8 BGR frame by cv2.warpAffine(image, trans, (W, H), flags=cv2.INTER_LINEAR), then ToTensor + Normalize,
// straight into the (n,3,H,W) fp32 batch the stem reads.
//
// The arithmetic is warpAffine's classic 8-bit INTER_LINEAR path, integer throughout (modules/imgproc/src/imgwarp.cpp):
//   the host inverts the forward matrix in float64 (hrnet_mi355.cpp) and sends M0..M5 of the INVERSE per crop;
//   X = (rint((M1*y + M2) * 1024) + 16 + rint(M0*x * 1024)) >> 5, Y likewise with M4, M5, M3   (1/32 pixel; rint = half to even,
//   each product and sum rounded on its own: no fused multiply-add);  sx = X >> 5, fx = X & 31, likewise sy, fy;
//   v = (p00*(32-fx)*(32-fy) + p01*fx*(32-fy) + p10*(32-fx)*fy + p11*fx*fy + 512) >> 10, a tap outside the frame reads 0
//   (BORDER_CONSTANT, value 0).  This is OpenCV's 15-bit coefficient table for 5-bit fractions without the table: its
//   entries are exact multiples of 32.
// OpenCV saturates sx, sy to int16; the host refuses frames with a side above 32 766, where a saturated coordinate is
// outside the frame with and without the saturation.  Parity with a cv2 build is UNPINNED (tests/golden/make_warp_golden.py
// makes the pin wherever opencv-python is installed); the kernel equals tests/warp_affine_ref.py bit for bit.
//
// Shape: the work is a gather of 4 x 3 bytes and three float stores per output pixel, so the stores decide it.  A wave owns
// 64 consecutive x of one output row: each of its three plane stores is one contiguous 256-byte run.  The taps of
// neighbouring lanes are neighbouring or identical bytes of the frame and come from L1 / L2.
#include "kernels.h"

namespace hrn {

namespace {
constexpr int WARP_ROWS = 4;   // output rows (= waves) per block
}

// (contraction off for the whole kernel, with plain operators: an operation inlined from a header keeps the flags it was
// compiled under and could still be fused with its neighbour)
#pragma clang fp contract(off)
__global__ __launch_bounds__(64 * WARP_ROWS) void warp_crops_kernel(const unsigned char *frames, int frame_h, int frame_w,
                                                                    const WarpParams *params, float *images, int H, int W,
                                                                    int tiles_x, int tiles_y) {
#pragma clang fp contract(off)
    const unsigned tiles = (unsigned)tiles_x * tiles_y;
    const unsigned crop = blockIdx.x / tiles, t = blockIdx.x - crop * tiles;
    const int ty = (int)(t / tiles_x), tx = (int)(t - (unsigned)ty * tiles_x);
    const int y = ty * WARP_ROWS + threadIdx.y, x = tx * 64 + threadIdx.x;
    if (y >= H || x >= W) return;
    const WarpParams p = params[crop];
    // row term (the same for the whole wave), column term per lane; rounded product, rounded sum, as the reference's loops.
    // The rounded terms are integers below 2^32 in magnitude (the host bounds the coordinates): their sum, the + 16 and the
    // >> 5 (floor of a division by 32) are exact in float64, and X, Y fit an int
    const double xr = rint((p.m[1] * (double)y + p.m[2]) * 1024.0) + 16.0;
    const double yr = rint((p.m[4] * (double)y + p.m[5]) * 1024.0) + 16.0;
    const int X = (int)floor((xr + rint(p.m[0] * (double)x * 1024.0)) * 0.03125);
    const int Y = (int)floor((yr + rint(p.m[3] * (double)x * 1024.0)) * 0.03125);
    const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
    const bool x0_in = sx >= 0 && sx < frame_w, x1_in = sx >= -1 && sx < frame_w - 1;
    const bool y0_in = sy >= 0 && sy < frame_h, y1_in = sy >= -1 && sy < frame_h - 1;
    const unsigned char *src = frames + (size_t)p.frame * frame_h * frame_w * 3;
    int p00[3] = {0, 0, 0}, p01[3] = {0, 0, 0}, p10[3] = {0, 0, 0}, p11[3] = {0, 0, 0};
    if (y0_in) {
        const unsigned char *row = src + (size_t)sy * frame_w * 3;
        if (x0_in) p00[0] = row[sx * 3], p00[1] = row[sx * 3 + 1], p00[2] = row[sx * 3 + 2];
        if (x1_in) p01[0] = row[sx * 3 + 3], p01[1] = row[sx * 3 + 4], p01[2] = row[sx * 3 + 5];
    }
    if (y1_in) {
        const unsigned char *row = src + (size_t)(sy + 1) * frame_w * 3;
        if (x0_in) p10[0] = row[sx * 3], p10[1] = row[sx * 3 + 1], p10[2] = row[sx * 3 + 2];
        if (x1_in) p11[0] = row[sx * 3 + 3], p11[1] = row[sx * 3 + 4], p11[2] = row[sx * 3 + 5];
    }
    const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};  // SimpleHRNet.py:171
    float *o = images + (size_t)crop * 3 * H * W + (size_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int k = 2 - c;                                // BGR -> RGB
        const int v = (p00[k] * w00 + p01[k] * w01 + p10[k] * w10 + p11[k] * w11 + 512) >> 10;
        const float f = (float)v / 255.0f;                  // ToTensor
        o[(size_t)c * H * W] = (f - mean[c]) / stdv[c];     // Normalize
    }
}

hipError_t launch_warp_crops(const unsigned char *frames_dev, int frame_h, int frame_w, const WarpParams *params_dev, int n,
                             float *images_dev, int H, int W, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int tiles_x = (W + 63) / 64, tiles_y = (H + WARP_ROWS - 1) / WARP_ROWS;
    const long long blocks = (long long)n * tiles_x * tiles_y;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(warp_crops_kernel, dim3((unsigned)blocks), dim3(64, WARP_ROWS), 0, s, frames_dev, frame_h, frame_w,
                       params_dev, images_dev, H, W, tiles_x, tiles_y);
    return hipGetLastError();
}

}  // namespace hrn
