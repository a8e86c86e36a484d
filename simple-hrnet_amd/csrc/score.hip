// Scoring of an evaluation batch on the GPU (include/hrnet_mi355.h: hrn_score_heatmaps, hrn_generate_targets): what
// testing/Test.py:141-157 computes per batch -- loss_fn(output, target, target_weight) (losses/loss.py) and
// evaluate_pck_accuracy(output, target) (misc/utils.py:125-151, 185-244) -- from the (n,J,h,w) fp32 heat-maps the head wrote.
//
//   score_kernel<MAPS>   one pass over the output maps.  A block of 256 threads owns whole maps (grid-strided), reads them with
//                        16-byte loads and produces per map: L = 0.5 / (h*w) * sum_p (double(o)*w - double(t)*w)^2 in fp64, the
//                        arg-max of o in the order of torch.max (argmax.h), its value, and get_max_preds' coordinates.
//                        MAPS = false: t is the Gaussian of datasets/COCO.py:460-515 looked up in the handle's table at
//                        (x - mu_x)^2 + (y - mu_y)^2 inside the window |x - mu_x|, |y - mu_y| <= 3 sigma -- nothing of target
//                        size is read or written.  MAPS = true: t is read from a second tensor whose arg-max is taken too.
//   score_finish_kernel  one block: the losses from the (n,J) matrix L in fp64, the PCK in float32 with the reference's operations.
//   targets_kernel       the analytic targets written out as (n,J,h,w) fp32.
//
// Order of the fp64 sum of a map: thread k adds the float4 groups k, k + 256, ... in that order, element by element; the 64
// lanes of a wave are combined by a butterfly, the 4 waves in wave order.  It depends on (h, w) alone: a map's L is the same
// bits in any batch, at any position, in both target modes.  No floating-point atomics.
#include "kernels.h"
#include "argmax.h"

namespace hrn {

namespace {
constexpr int SCORE_THREADS = 256;
constexpr int SCORE_WAVES = SCORE_THREADS / 64;
constexpr int SCORE_MAX_BLOCKS = 2048;   // 8 blocks per CU; more maps than that are walked grid-strided
}

// (contraction off for the whole file: the loss terms are a rounded difference and a rounded square in both target modes, and
// the distances of the PCK are torch's separate float32 operations)
#pragma clang fp contract(off)

// the target value of cell (x, y): table[dx^2 + dy^2] inside the window of a drawn joint, 0 everywhere else
__device__ __forceinline__ float analytic_target(const ScoreJoint &jt, const float *table, int t, int x, int y) {
    const int dx = x - jt.mu_x, dy = y - jt.mu_y;
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    return (jt.draw && ax <= t && ay <= t) ? table[dx * dx + dy * dy] : 0.f;
}

// block-wide arg-max in the order of `better`; the result is valid in thread 0
__device__ __forceinline__ void block_argmax(float &bv, int &bi, float *sv, int *si) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (better(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = bv, si[threadIdx.x >> 6] = bi;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < SCORE_WAVES; ++k)
            if (better(sv[k], si[k], bv, bi)) bv = sv[k], bi = si[k];
    __syncthreads();
}

// get_max_preds (misc/utils.py:143-150): (idx % w, idx / w) as floats, zeroed where the maximum is not > 0 (a NaN is not)
__device__ __forceinline__ void store_pred(float *dst, float bv, int bi, int w) {
    const bool pos = bv > 0.f;
    dst[0] = pos ? (float)(bi % w) : 0.f;
    dst[1] = pos ? (float)(bi / w) : 0.f;
}

template <bool MAPS>
__global__ __launch_bounds__(SCORE_THREADS) void score_kernel(const ScoreArgs p) {
#pragma clang fp contract(off)
    __shared__ double ssum[SCORE_WAVES];
    __shared__ float sv[SCORE_WAVES];
    __shared__ int si[SCORE_WAVES];
    const int hw = p.h * p.w, groups = hw >> 2, total = p.n * p.J;
    for (int m = blockIdx.x; m < total; m += gridDim.x) {
        const ScoreJoint jt = p.joints[m];
        const double wd = (double)jt.weight;
        const float4 *o4 = (const float4 *)(p.heatmaps + (size_t)m * hw);
        const float4 *t4 = MAPS ? (const float4 *)(p.targets + (size_t)m * hw) : nullptr;
        double acc = 0.;
        float bv = -INFINITY, tv = -INFINITY;
        int bi = kNoIdx, ti = kNoIdx;
        for (int q = threadIdx.x; q < groups; q += SCORE_THREADS) {
            const float4 o = o4[q];
            const int px = q << 2, y = px / p.w, x = px - y * p.w;   // w is a multiple of 4: the four cells share a row
            float4 t;
            if constexpr (MAPS) {
                t = t4[q];
            } else {
                t.x = analytic_target(jt, p.table, p.t, x, y), t.y = analytic_target(jt, p.table, p.t, x + 1, y);
                t.z = analytic_target(jt, p.table, p.t, x + 2, y), t.w = analytic_target(jt, p.table, p.t, x + 3, y);
            }
            const float ov[4] = {o.x, o.y, o.z, o.w}, tt[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)ov[e] * wd - (double)tt[e] * wd;   // both products are exact in fp64
                acc = acc + d * d;
                if (takes(ov[e], bv, bi)) bv = ov[e], bi = px + e;
                if constexpr (MAPS)
                    if (takes(tt[e], tv, ti)) tv = tt[e], ti = px + e;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off);
        if ((threadIdx.x & 63) == 0) ssum[threadIdx.x >> 6] = acc;
        block_argmax(bv, bi, sv, si);   // (its barriers publish ssum too)
        if constexpr (MAPS) block_argmax(tv, ti, sv, si);
        if (threadIdx.x == 0) {
            double s = ssum[0];
            for (int k = 1; k < SCORE_WAVES; ++k) s = s + ssum[k];
            p.map_loss[m] = 0.5 * s / (double)hw;
            p.maxvals[m] = bv;
            store_pred(p.preds + (size_t)m * 2, bv, bi == kNoIdx ? 0 : bi, p.w);
            float *tp = p.target_preds + (size_t)m * 2;
            if constexpr (MAPS) {
                store_pred(tp, tv, ti == kNoIdx ? 0 : ti, p.w);
            } else {   // the arg-max of a drawn Gaussian is the cell nearest to its centre; an empty map gives (0, 0)
                tp[0] = jt.draw ? (float)min(max(jt.mu_x, 0), p.w - 1) : 0.f;
                tp[1] = jt.draw ? (float)min(max(jt.mu_y, 0), p.h - 1) : 0.f;
            }
        }
        __syncthreads();   // ssum / sv / si are rewritten by the next map
    }
}

// sum of one value per thread in a fixed order (butterfly per wave, then the waves in order); valid in every thread
__device__ __forceinline__ double block_sum(double v, double *s) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = s[0];
    for (int k = 1; k < SCORE_WAVES; ++k) r = r + s[k];
    return r;
}

// a before b in torch.topk's order: larger first, a NaN is larger than everything
__device__ __forceinline__ bool larger(double a, double b) { return a > b || (a != a && b == b); }

// float32 division and square root, correctly rounded, through fp64: the quotient (root) of two floats rounded to 53 bits and
// then to 24 is the correctly rounded float (53 >= 2 * 24 + 2), so these equal torch's float32 `/` and `sqrt` bit for bit
// without the float32 expansion of the division, which is built from fused multiply-adds
// (the empty asm hides the widening from the optimiser, which would otherwise narrow the expression back to the float32 operation)
__device__ __forceinline__ double opaque(double x) {
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ float div32(float a, float b) { return (float)(opaque((double)a) / (double)b); }
__device__ __forceinline__ float sqrt32(float a) { return (float)sqrt(opaque((double)a)); }

// losses/loss.py: JointsMSELoss = mean(L); JointsOHKMMSELoss = mean over persons of the mean of the topk largest L[i, :].
// misc/utils.py:185-244: dists (J, n), acc (J), avg_acc, cnt.
__global__ __launch_bounds__(SCORE_THREADS) void score_finish_kernel(const ScoreArgs p) {
#pragma clang fp contract(off)
    __shared__ double ssum[SCORE_WAVES];
    const int n = p.n, J = p.J;
    // ---- losses: thread k owns persons k, k + 256, ...; a person's row is summed in joint order
    double mse = 0., ohkm = 0.;
    for (int i = threadIdx.x; i < n; i += SCORE_THREADS) {
        const double *L = p.map_loss + (size_t)i * J;
        double row = 0.;
        for (int j = 0; j < J; ++j) row = row + L[j];
        mse = mse + row;
        if (p.ohkm_topk > 0) {   // the topk largest of the row, largest first
            // No "already taken" set: the row is totally ordered by (value in topk's order, then joint index), and pick k is the
            // first element of that order behind pick k - 1.  Among equal values the lower joint goes first, as a scan that
            // skipped taken joints had it; any J, any topk <= J, O(topk * J) reads of a row that sits in the cache.
            double top = 0., pv = 0.;
            int pj = -1;
            for (int k = 0; k < p.ohkm_topk; ++k) {
                int best = -1;
                double bv = 0.;
                for (int j = 0; j < J; ++j) {
                    const double v = L[j];
                    const bool behind = pj < 0 || larger(pv, v) || (!larger(v, pv) && j > pj);   // v comes after the last pick
                    if (behind && (best < 0 || larger(v, bv))) best = j, bv = v;
                }
                pv = bv, pj = best;
                top = top + bv;
            }
            ohkm = ohkm + top / (double)p.ohkm_topk;
        }
    }
    mse = block_sum(mse, ssum);
    ohkm = block_sum(ohkm, ssum);
    if (threadIdx.x == 0) {
        *p.loss_mse = mse / ((double)n * (double)J);
        *p.loss_ohkm = p.ohkm_topk > 0 ? ohkm / (double)n : __longlong_as_double(0x7ff8000000000000LL);
    }
    // ---- PCK: wave k owns joints k, k + 4, ...; its lanes the persons.  norm = (h / 10, w / 10) in float32, x divided by
    // the first and y by the second, as evaluate_pck_accuracy and calc_dists have it
    const float norm_x = div32((float)p.h, 10.f), norm_y = div32((float)p.w, 10.f);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < J; j += SCORE_WAVES) {
        int below = 0, valid = 0;
        for (int i = lane; i < n; i += 64) {
            const float *pr = p.preds + ((size_t)i * J + j) * 2, *tg = p.target_preds + ((size_t)i * J + j) * 2;
            float d = -1.f;
            if (tg[0] > 1.f && tg[1] > 1.f) {
                const float dx = div32(pr[0], norm_x) - div32(tg[0], norm_x), dy = div32(pr[1], norm_y) - div32(tg[1], norm_y);
                d = sqrt32(dx * dx + dy * dy);
            }
            p.dists[(size_t)j * n + i] = d;
            valid += d != -1.f;
            below += d != -1.f && d < p.pck_thr;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) below += __shfl_xor(below, off), valid += __shfl_xor(valid, off);
        if (lane == 0) p.acc[j] = valid > 0 ? div32((float)below, (float)valid) : -1.f;
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.f;
        int cnt = 0;
        for (int j = 0; j < J; ++j)
            if (p.acc[j] >= 0.f) sum = sum + p.acc[j], ++cnt;
        *p.avg_acc = cnt ? div32(sum, (float)cnt) : 0.f;
        *p.cnt = cnt;
    }
}

__global__ __launch_bounds__(SCORE_THREADS) void targets_kernel(const ScoreArgs p, float *targets) {
    const int hw = p.h * p.w, groups = hw >> 2, total = p.n * p.J;
    for (int m = blockIdx.x; m < total; m += gridDim.x) {
        const ScoreJoint jt = p.joints[m];
        float4 *o4 = (float4 *)(targets + (size_t)m * hw);
        for (int q = threadIdx.x; q < groups; q += SCORE_THREADS) {
            const int px = q << 2, y = px / p.w, x = px - y * p.w;
            float4 t;
            t.x = analytic_target(jt, p.table, p.t, x, y), t.y = analytic_target(jt, p.table, p.t, x + 1, y);
            t.z = analytic_target(jt, p.table, p.t, x + 2, y), t.w = analytic_target(jt, p.table, p.t, x + 3, y);
            o4[q] = t;
        }
    }
}

namespace {
// every map is h*w floats read as float4 groups that do not straddle a row
bool score_shape_ok(const ScoreArgs &a) {
    return a.n >= 0 && a.J > 0 && a.J <= kMaxJoints && a.h > 0 && a.w > 0 && a.w % 4 == 0 && (long long)a.n * a.J <= 0x7fffffffLL;
}
}  // namespace

hipError_t launch_score(const ScoreArgs &a, hipStream_t s) {
    if (!score_shape_ok(a)) return hipErrorInvalidValue;
    const int total = a.n * a.J;
    if (total > 0) {
        const unsigned blocks = (unsigned)(total < SCORE_MAX_BLOCKS ? total : SCORE_MAX_BLOCKS);
        if (a.targets)
            hipLaunchKernelGGL(score_kernel<true>, dim3(blocks), dim3(SCORE_THREADS), 0, s, a);
        else
            hipLaunchKernelGGL(score_kernel<false>, dim3(blocks), dim3(SCORE_THREADS), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(score_finish_kernel, dim3(1), dim3(SCORE_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_targets(const ScoreArgs &a, float *targets_out, hipStream_t s) {
    if (!score_shape_ok(a)) return hipErrorInvalidValue;
    const int total = a.n * a.J;
    if (total == 0) return hipSuccess;
    const unsigned blocks = (unsigned)(total < SCORE_MAX_BLOCKS ? total : SCORE_MAX_BLOCKS);
    hipLaunchKernelGGL(targets_kernel, dim3(blocks), dim3(SCORE_THREADS), 0, s, a, targets_out);
    return hipGetLastError();
}

}  // namespace hrn
