// Joints over time on the GPU (include/hrnet_mi355.h: hrn_filter_poses_dev): the One-Euro filter of every joint of this frame and
// the prediction of the next one, with the state following the people through hrn_associate_people_dev's `match` where it lies
// -- the step that would otherwise take the joints through the host after every frame.  ONE launch, one thread per (person,
// joint), 256-thread blocks:
//
//   read      the joint's (y, x, confidence), the person's match and (P > 1) its segment; with a match inside the segment, the age
//             and the six state values of the same joint of the previous person
//   compute   temporal_math.h's temporal_joint: the text the host entry compiles, so the results equal its bit for bit
//   write     the filtered joint (possibly over the input: each thread has read its joint before it writes it), the prediction
//             when asked for, six state values, the age
//
// Consecutive threads hold consecutive joints: a wave reads 768 and writes up to 3328 consecutive bytes, and the gather reads
// runs of whole joints of one previous person.  No atomics, no scratch, no LDS; every byte has one writer.  This is a latency link,
// not a throughput kernel: a video frame has some hundred joints.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "temporal_math.h"

namespace hrn {

__global__ __launch_bounds__(256) void temporal_kernel(TemporalArgs a, TemporalParams prm) {
#pragma clang fp contract(off)
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (unsigned)a.total) return;
    const unsigned i = t / (unsigned)a.J, j = t - i * (unsigned)a.J;
    const size_t person = (size_t)a.first + i, at = (size_t)a.first * a.J + t;   // the joint's place in the (n, J, .) arrays
    const float v[3] = {a.pts[at * 3], a.pts[at * 3 + 1], a.pts[at * 3 + 2]};
    const TemporalSegment seg = a.table ? a.table[i] : a.one;
    const long long before = a.match ? temporal_previous(a.match[person], seg.prev0, seg.m) : -1;
    float prev[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int prev_age = 0;
    if (before >= 0) {
        const size_t q = (size_t)before * a.J + j;
        prev_age = a.prev_age[q];
        if (prev_age > 0)
            for (int k = 0; k < 6; ++k) prev[k] = a.prev_state[q * 6 + k];
    }
    const TemporalJoint r = temporal_joint(v, prev_age > 0, prev, prev_age, prm);
    a.pts_out[at * 3] = r.out[0], a.pts_out[at * 3 + 1] = r.out[1], a.pts_out[at * 3 + 2] = v[2];
    if (a.pred_out) a.pred_out[at * 3] = r.pred[0], a.pred_out[at * 3 + 1] = r.pred[1], a.pred_out[at * 3 + 2] = v[2];
    for (int k = 0; k < 6; ++k) a.state[at * 6 + k] = r.state[k];
    a.age[at] = r.age;
}

hipError_t launch_temporal(const TemporalArgs &a, const TemporalParams &prm, hipStream_t s) {
    if (a.total <= 0) return hipSuccess;
    hipLaunchKernelGGL(temporal_kernel, dim3(((unsigned)a.total + 255u) / 256u), dim3(256), 0, s, a, prm);
    return hipGetLastError();
}

}  // namespace hrn
