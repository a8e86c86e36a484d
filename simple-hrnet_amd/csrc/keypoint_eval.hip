// COCO keypoint AP / AR on the GPU (include/hrnet_mi355.h: hrn_keypoint_eval_dev): the last step of the evaluation chain -- OKS
// matching of detections to ground truth per image, precision / recall accumulation over the set, the ten statistics.  Four
// launches on the caller's stream; the arithmetic is keypoint_eval_math.h's, the text the host form compiles:
//
//   match    one 256-thread block per image.  Scores, the people's k1 / crowd / ig flags into LDS; every detection's position by
//            counting who comes before it (the first 20 are the slots); the people's orders of the three ranges on three lanes;
//            the slots x people OKS matrix into LDS, one thread per pair, serial over the joints (numpy's pairwise summation order
//            forbids splitting a pair across lanes); then the 30 (range, threshold) matchings on 30 lanes, each serial over at most
//            20 x 256 LDS values.  Writes the slot records, npig and status.
//   rank     one thread per slot: its place in the set-wide order = the number of slots that come before it (descending score,
//            ties by slot index, NaN last), the scores going through LDS in tiles of 256.  O(S^2) compares, no sort; every place has
//            one writer.
//   curve    one block per (range, threshold).  npig and the total tp / fp counts by block sums; then ONE pass over the slots in set
//            order from the end, 256 at a time: a block scan of the exact integer counts gives each slot's tp / fp, a block scan of
//            the maximum its enveloped precision, and the slot that owns a recall threshold (eval_owns) writes its precision.
//   finish   one block: the ten statistics (eval_stat), one lane each.
//
// No atomics; every byte has one writer; nothing depends on scheduling.  LDS of the match kernel: 40 KiB of OKS, 7.5 KiB of taken
// flags, about 7 KiB of scores, variances, flags and orders.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "keypoint_eval_math.h"

namespace hrn {

__global__ __launch_bounds__(256) void keypoint_eval_match_kernel(KeypointEvalArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_oks[kEvalMaxDet * kMaxTracked];
    __shared__ double s_sc[kMaxTracked], s_vars[kAssocMaxJoints], s_darea[kEvalMaxDet];
    __shared__ int s_slot[kEvalMaxDet], s_npig[kEvalAreas];
    __shared__ short s_k1[kMaxTracked];
    __shared__ unsigned char s_taken[kEvalAreas * kEvalThrs][kMaxTracked];
    __shared__ unsigned char s_ig[kEvalAreas][kMaxTracked], s_order[kEvalAreas][kMaxTracked], s_crowd[kMaxTracked];
    const int tid = threadIdx.x, J = a.J;
    const EvalImage im = a.images[blockIdx.x];   // dt_n, gt_n <= kMaxTracked, J <= kAssocMaxJoints: the entry refuses more
    const size_t dt_first = (size_t)im.dt_first, gt_first = (size_t)im.gt_first;

    // ---- scores, variances, the people's flags ----
    if (tid < J) s_vars[tid] = pose_nms_var(a.sigmas, tid);
    double sc = 0.0;
    if (tid < im.dt_n) s_sc[tid] = sc = a.dt_scores[dt_first + tid];
    if (tid < im.gt_n) {
        const int k1 = eval_k1(a.gt_kpts + (gt_first + tid) * J * 3, J);
        const bool crowd = a.gt_iscrowd[gt_first + tid] != 0;
        const double area = a.gt_area[gt_first + tid];
        s_k1[tid] = (short)k1, s_crowd[tid] = crowd;
        for (int r = 0; r < kEvalAreas; ++r) s_ig[r][tid] = eval_gt_ig(crowd || k1 == 0, area, r);
    }
    const int status = __syncthreads_or(tid < im.dt_n && sc != sc) ? 1 : 0;

    // ---- the slots; the people's orders ----
    if (tid < im.dt_n) {
        const int r = pose_nms_rank(s_sc, im.dt_n, tid);
        if (r < im.slots) s_slot[r] = tid;
    }
    if (tid >= 64 && tid < 64 + kEvalAreas) s_npig[tid - 64] = eval_gt_order(s_ig[tid - 64], im.gt_n, s_order[tid - 64]);
    __syncthreads();

    // ---- the slot records and the OKS matrix ----
    if (tid < im.slots) {
        const size_t d = dt_first + s_slot[tid];
        a.slot_person[im.slot_first + tid] = (int)d, a.slot_score[im.slot_first + tid] = s_sc[s_slot[tid]];
        s_darea[tid] = eval_dt_area(a.dt_kpts + d * J * 3, J);
    }
    int bad = 0;
    for (int idx = tid; idx < im.slots * im.gt_n; idx += 256) {
        const int s = idx / im.gt_n, g = idx - s * im.gt_n;
        s_oks[idx] = eval_oks(a.dt_kpts + (dt_first + s_slot[s]) * J * 3, a.gt_kpts + (gt_first + g) * J * 3, J, s_k1[g],
                              a.gt_bbox + (gt_first + g) * 4, a.gt_area[gt_first + g], s_vars, &bad);
    }
    bad = __syncthreads_or(bad);

    // ---- the 30 matchings ----
    if (tid < kEvalAreas * kEvalThrs) {
        const int r = tid / kEvalThrs, t = tid - r * kEvalThrs;
        const size_t out = (size_t)tid * a.S + im.slot_first;
        eval_match(s_oks, im.slots, im.gt_n, s_order[r], s_ig[r], s_crowd, s_darea, r, kEvalIouThrs[t], im.gt_first, s_taken[tid],
                   a.dt_match + out, a.dt_ignore + out);
    }
    if (tid >= 64 && tid < 64 + kEvalAreas) a.npig[(size_t)blockIdx.x * kEvalAreas + (tid - 64)] = s_npig[tid - 64];
    if (tid == 128) a.status[blockIdx.x] = status | (bad ? 2 : 0);
}

__global__ __launch_bounds__(256) void keypoint_eval_rank_kernel(KeypointEvalArgs a) {
    __shared__ double s_tile[256];
    const int tid = threadIdx.x, S = a.S;
    const int me = blockIdx.x * 256 + tid;
    const double mine = me < S ? a.slot_score[me] : 0.0;
    int place = 0;
    for (int base = 0; base < S; base += 256) {
        if (base + tid < S) s_tile[tid] = a.slot_score[base + tid];
        __syncthreads();
        const int n = S - base < 256 ? S - base : 256;
        if (me < S)
            for (int k = 0; k < n; ++k) place += pose_nms_before(s_tile[k], base + k, mine, me) ? 1 : 0;
        __syncthreads();
    }
    if (me < S) a.set_order[place] = me;
}

// inclusive scan of v over the block's 256 threads (a sum from thread 0 up); buf[255] holds the total afterwards.  The caller
// puts a barrier between its last read of buf and the next use.
__device__ inline int block_scan_sum(int v, int *buf, int tid) {
    buf[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int add = tid >= off ? buf[tid - off] : 0;
        __syncthreads();
        buf[tid] += add;
        __syncthreads();
    }
    return buf[tid];
}
// the maximum of v over this thread and every later one; buf[0] holds the block's maximum afterwards
__device__ inline double block_scan_max_from_end(double v, double *buf, int tid) {
    buf[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const double other = tid + off < 256 ? buf[tid + off] : v;
        __syncthreads();
        if (other > buf[tid]) buf[tid] = other;
        __syncthreads();
    }
    return buf[tid];
}

__global__ __launch_bounds__(256) void keypoint_eval_curve_kernel(KeypointEvalArgs a) {
#pragma clang fp contract(off)
    __shared__ int s_int[256];
    __shared__ double s_dbl[256], s_prec[kEvalRecs];
    const int tid = threadIdx.x, S = a.S, at = blockIdx.x, range = at / kEvalThrs;
    double *prec = a.precision + (size_t)at * kEvalRecs;

    int part = 0;
    for (int p = tid; p < a.P; p += 256) part += a.npig[(size_t)p * kEvalAreas + range];
    block_scan_sum(part, s_int, tid);
    const int npig = s_int[255];
    __syncthreads();
    if (npig == 0) {   // (block-uniform)
        if (tid < kEvalRecs) prec[tid] = -1.0;
        if (tid == 0) a.recall[at] = -1.0;
        return;
    }
    const int *match = a.dt_match + (size_t)at * S;
    const unsigned char *ignore = a.dt_ignore + (size_t)at * S;

    // ---- the totals ----
    int my_tp = 0, my_fp = 0;
    for (int i = tid; i < S; i += 256) {
        const int s = a.set_order[i];
        if (!ignore[s]) (match[s] >= 0 ? my_tp : my_fp) += 1;
    }
    block_scan_sum(my_tp, s_int, tid);
    int end_tp = s_int[255];
    __syncthreads();
    block_scan_sum(my_fp, s_int, tid);
    int end_fp = s_int[255];
    if (tid < kEvalRecs) s_prec[tid] = 0.0;
    if (tid == 0) a.recall[at] = S ? eval_recall(end_tp, npig) : 0.0;
    __syncthreads();

    // ---- from the end: counts, envelope, look-ups (end_tp / end_fp: the counts at the last slot of the chunk) ----
    double later = -1.0;   // the maximum of pr over every later chunk
    for (int chunk = (S + 255) / 256 - 1; chunk >= 0; --chunk) {
        const int i = chunk * 256 + tid;
        int is_tp = 0, is_fp = 0;
        if (i < S) {
            const int s = a.set_order[i];
            if (!ignore[s]) (match[s] >= 0 ? is_tp : is_fp) = 1;
        }
        const int upto = block_scan_sum(is_tp | (is_fp << 16), s_int, tid);   // at most 256 of each: the halves cannot carry
        const int total = s_int[255];
        const int tp = end_tp - (total & 0xffff) + (upto & 0xffff), fp = end_fp - (total >> 16) + (upto >> 16);
        const double pr = i < S ? eval_precision(tp, fp) : -1.0;
        double env = block_scan_max_from_end(pr, s_dbl, tid);
        const double chunk_max = s_dbl[0];
        env = later > env ? later : env;
        if (i < S && (is_tp || i == 0))
            for (int r = 0; r < kEvalRecs; ++r)
                if (eval_owns(tp, tp - is_tp, i == 0, npig, r)) s_prec[r] = env;
        end_tp -= total & 0xffff, end_fp -= total >> 16;
        later = chunk_max > later ? chunk_max : later;
        __syncthreads();
    }
    if (tid < kEvalRecs) prec[tid] = s_prec[tid];
}

__global__ __launch_bounds__(64) void keypoint_eval_finish_kernel(KeypointEvalArgs a) {
    if (threadIdx.x < 10) a.stats[threadIdx.x] = eval_stat(a.precision, a.recall, threadIdx.x);
}

hipError_t launch_keypoint_eval(const KeypointEvalArgs &a, hipStream_t s) {
    if (a.P > 0) hipLaunchKernelGGL(keypoint_eval_match_kernel, dim3((unsigned)a.P), dim3(256), 0, s, a);
    if (a.S > 0) hipLaunchKernelGGL(keypoint_eval_rank_kernel, dim3((unsigned)((a.S + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(keypoint_eval_curve_kernel, dim3(kEvalAreas * kEvalThrs), dim3(256), 0, s, a);
    hipLaunchKernelGGL(keypoint_eval_finish_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace hrn
