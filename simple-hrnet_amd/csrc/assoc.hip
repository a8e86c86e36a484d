// Person re-identification between two frames on the GPU (include/hrnet_mi355.h: hrn_associate_people_dev): who of the previous
// frame is who of this one -- the last step of a video loop that forced the joints through the host.  One launch per call, one
// 256-thread block per problem (one video: one problem; a camera wall: one per stream):
//
//   phase 1   threads stride over the (current, previous) pairs; each runs assoc_math.h's similarity and blend serially over the
//             joints (numpy's pairwise summation order forbids splitting a pair across lanes) and writes cost and similarity to
//             the engine's scratch
//   phase 2   ONE wave runs hrn_assignment's shortest augmenting paths (assoc_assign.h, shared with tracks.hip).  u, v, minv, p,
//             way and used live in LDS; lane l owns the columns l + 1, l + 65, ... in ascending order, and the wave's minimum
//             keeps the lower column on equal values, so every step is elementwise or that argmin: the matching is
//             hrn_assignment's by construction, not by tolerance
//   phase 3   the block applies the threshold, carries ids over, numbers new people in index order (ballot + prefix count),
//             smooths matched boxes and joints, updates next_id and writes the status
//
// No atomics; every byte has one writer.  This is a latency link, not a throughput kernel: phase 2 is serial in the rows and in
// the steps of each augmenting path, and one wave of one CU runs it.
#include <hip/hip_runtime.h>

#include "assoc_assign.h"
#include "assoc_math.h"
#include "kernels.h"

namespace hrn {

__global__ __launch_bounds__(256) void assoc_kernel(AssocArgs a) {
#pragma clang fp contract(off)
    __shared__ AssignLds s_assign;
    __shared__ double s_vars[17];
    __shared__ int s_col[kMaxTracked], s_cnt[4], s_max[4];
    __shared__ int s_fail;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const AssocProblem pr = a.P == 1 ? a.one : a.table[blockIdx.x];
    const int n = pr.n, m = pr.m, J = a.J;   // n, m <= kMaxTracked: the entry refuses more
    if (n == 0) {                            // nobody here: next_id stays
        if (tid == 0) a.status[blockIdx.x] = 0;
        return;
    }
    const AssocParams prm = assoc_params(a.pose_alpha, a.similarity_threshold, a.smoothing_alpha);
    double *cost = (double *)(a.scratch + pr.scratch);
    float *sim = (float *)(cost + (size_t)n * m);

    // ---- phase 1: cost and similarity of every pair ----
    if (tid < 17) s_vars[tid] = assoc_coco_var(tid);
    s_col[tid] = -1;
    if (tid == 0) s_fail = 0;
    __syncthreads();
    int replaced = 0;
    for (int pair = tid; pair < n * m; pair += 256) {
        const int i = pair / m, k = pair - i * m;
        replaced |= assoc_pair(a.pts + (size_t)(pr.cur0 + i) * J * 3, a.prev_pts + (size_t)(pr.prev0 + k) * J * 3, J,
                               a.boxes + (size_t)(pr.cur0 + i) * 4, a.prev_boxes + (size_t)(pr.prev0 + k) * 4, s_vars, prm, &cost[pair],
                               &sim[pair]);
    }
    int status = __syncthreads_or(replaced) ? 1 : 0;   // (the barrier also publishes the scratch to the block)

    // ---- phase 2: the assignment, one wave (hrn_assignment, postproc.cpp, step for step) ----
    if (wave == 0 && m > 0 && !a.no_assign) {   // (assoc_assign.h: the text tracks.hip runs too)
        if (!assoc_assign_wave(cost, n, m, lane, s_assign, s_col) && lane == 0) s_fail = 1;
    }
    __syncthreads();
    if (s_fail) status |= 2;

    // ---- phase 3: threshold, ids, smoothing ----
    const int next = a.next_id[blockIdx.x];
    int id = -1, col = -1;
    if (tid < n) {
        const int c = s_col[tid];
        if (c >= 0 && assoc_accepted(sim[(size_t)tid * m + c], prm)) col = c, id = a.prev_ids[pr.prev0 + c];
    }
    const bool fresh = tid < n && id == -1;
    const unsigned long long ballot = __ballot(fresh);
    if (lane == 0) s_cnt[wave] = __popcll(ballot);
    s_col[tid] = col;                                        // from here on: the accepted previous index
    __syncthreads();
    if (fresh) {
        int rank = __popcll(ballot & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) rank += s_cnt[w];
        id = assoc_fresh_id(next, rank);
    }
    if (tid < n) a.ids[pr.cur0 + tid] = id, a.match[pr.cur0 + tid] = col;
    int mx = tid < n ? id : (-2147483647 - 1);
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(mx, o);
        mx = w > mx ? w : mx;
    }
    if (lane == 0) s_max[wave] = mx;
    if (prm.smoothing != 0.0) {
        if (col >= 0)
            for (int k = 0; k < 4; ++k) {
                int *b = a.boxes + (size_t)(pr.cur0 + tid) * 4 + k;
                *b = assoc_smooth_box(*b, a.prev_boxes[(size_t)(pr.prev0 + col) * 4 + k], prm);
            }
        const int per = J * 3;
        for (int idx = tid; idx < n * per; idx += 256) {
            const int i = idx / per, e = idx - i * per, c = s_col[i];
            if (c < 0) continue;
            float *p = a.pts + (size_t)(pr.cur0 + i) * per + e;
            *p = assoc_smooth_joint(*p, a.prev_pts[(size_t)(pr.prev0 + c) * per + e], prm);
        }
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) mx = s_max[w] > mx ? s_max[w] : mx;
        a.next_id[blockIdx.x] = assoc_next_id(next, mx);
        a.status[blockIdx.x] = status;
    }
}

hipError_t launch_assoc(const AssocArgs &a, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    hipLaunchKernelGGL(assoc_kernel, dim3((unsigned)a.P), dim3(256), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void bone_ids_kernel(const int *ids, int n, const unsigned *palette, int Cb, unsigned *bone) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long id = ids[i];
    bone[i] = palette[((id % Cb) + Cb) % Cb];   // Python's modulo
}

hipError_t launch_bone_ids(const int *ids, int n, const unsigned *palette, int Cb, unsigned *bone, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(bone_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, n, palette, Cb, bone);
    return hipGetLastError();
}

}  // namespace hrn
