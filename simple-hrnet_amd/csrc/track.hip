// The tracking link of a video loop on the GPU (include/hrnet_mi355.h: hrn_boxes_from_poses, hrn_preprocess_frames_dev): between
// two detector runs the next frame's crops are cut from the previous frame's joints, pts(k) -> boxes -> crop records ->
// crops(k+1) -> pass -> pts(k+1), stream-ordered and without a host read.
//
//   pose_boxes_kernel     one wave per person: the extent of the live joints and the mean of their confidences as a detection
//                         row (x1, y1, x2, y2, score), read from the joints where the decode left them
//   crop_records_kernel   one thread per person: the box arithmetic of the crop pre-path (hrn_crop_geometry's) on a detection
//                         row in device memory; writes the CropParams record the host path would have uploaded, the box the
//                         decode scales by and a status.  prepath.hip's kernels then run unchanged on those records.
//
// The arithmetic of both is track_geometry.h's, the text the host entries compile: double, fixed order, no contraction.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "track_geometry.h"

namespace hrn {

namespace {

__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

}  // namespace

__global__ __launch_bounds__(64) void pose_boxes_kernel(PoseBoxArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x, lane = threadIdx.x;
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY, sum = 0.0;
    int nlive = 0;
    for (int j0 = 0; j0 < a.J; j0 += 64) {
        const int j = j0 + lane;
        bool live = false;
        float c = 0.0f;
        if (j < a.J) {
            const float *p = a.pts + ((size_t)i * a.J + j) * 3;   // (y, x, confidence)
            const float y = p[0], x = p[1];
            c = p[2];
            live = pose_joint_live(y, x, c, a.threshold);
            if (live) {   // (no zero is negative here and nothing is NaN: minimum and maximum are exact in any order)
                const double yd = pose_coordinate(y), xd = pose_coordinate(x);
                xmin = xd < xmin ? xd : xmin, xmax = xd > xmax ? xd : xmax;
                ymin = yd < ymin ? yd : ymin, ymax = yd > ymax ? yd : ymax;
            }
        }
        // the confidences are summed in joint order, as the definition says: every lane walks the live lanes of the ballot
        unsigned long long b = __ballot(live);
        nlive += __popcll(b);
        while (b) {
            const int k = __ffsll((long long)b) - 1;
            sum = sum + (double)__shfl(c, k);
            b &= b - 1;
        }
    }
    xmin = wave_min(xmin), xmax = wave_max(xmax), ymin = wave_min(ymin), ymax = wave_max(ymax);
    if (lane == 0) {
        const int fh = a.frame_hw ? a.frame_hw[2 * (size_t)i] : a.frame_h, fw = a.frame_hw ? a.frame_hw[2 * (size_t)i + 1] : a.frame_w;
        float row[5];
        pose_box_finish(xmin, xmax, ymin, ymax, sum, nlive, a.min_joints, fh, fw, a.scale, a.min_side, row);
        float *o = a.dets + (size_t)i * 5;
        for (int k = 0; k < 5; ++k) o[k] = row[k];
    }
}

hipError_t launch_pose_boxes(const PoseBoxArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pose_boxes_kernel, dim3((unsigned)a.n), dim3(64), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void crop_records_kernel(CropRecordArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const TrackFrame &f = a.frame_index ? a.frames[a.frame_index[i]] : a.frame0;
    const float *d = a.dets + (size_t)i * a.det_stride;
    CropParams cp{};
    int32_t box[4] = {0, 0, 0, 0};
    long pad_hw[2] = {0, 0};
    int status = CROP_OK;
    for (int k = 0; k < 4; ++k)   // (NaN fails the comparison)
        if (!(fabsf(d[k]) <= 1073741824.0f)) status = CROP_NOT_FINITE;
    if (status == CROP_OK) status = crop_geometry_one(d, f.height, f.width, a.H, a.W, a.variant, cp, box, pad_hw);
    if (status == CROP_OK && pad_hw[0] > crop_hcap(f.height, f.width, a.H, a.W)) status = CROP_TOO_TALL;
    if (status != CROP_OK) {   // the all-padding crop: nothing of the frame is read, H x W zeros go through an identity resize
        cp = CropParams{};
        cp.h_pad = a.H, cp.w_pad = a.W;
        box[0] = box[1] = box[2] = box[3] = 0;
    }
    cp.tmp_off = (long long)i * a.slot_bytes;
    cp.frame = f.bgr, cp.frame_w = f.width, cp.frame_h = f.height;
    a.crops[i] = cp;
    if (a.yuv) a.srcs[i] = f.yuv;
    for (int k = 0; k < 4; ++k) a.boxes[(size_t)i * 4 + k] = box[k];
    a.status[i] = status;
}

hipError_t launch_crop_records(const CropRecordArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(crop_records_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace hrn
