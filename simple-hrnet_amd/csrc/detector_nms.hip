// Detector NMS on the GPU (include/hrnet_mi355.h: hrn_detector_nms_dev): the raw (B, N, 5 + C) output of a YOLO head to kept rows
// without a host step -- the one link of the video loop between the detector network and hrn_detections_to_frame_dev.  Two
// launches; the arithmetic is detector_nms_math.h's, the text the host form compiles.
//
//   the scoring launch   grid (ceil(N / 256), images), 256 threads, one row of pred per thread.  pred is read ONCE: the obj column
//                        first (one 4-byte load per row); then, for the rows whose obj passes -- a few hundred of 25 200 at
//                        deployment thresholds -- the classes, one wave per row with a lane per class (rows are 20 + 4C bytes and
//                        not 16-byte aligned: the loads are single elements, a wave's 64 of them contiguous), reduced to the first
//                        maximum over the wave; the row's own lane then reads the box and judges the candidate.  The block's
//                        candidates are compacted in row order (ballot + popcount within a wave, the four wave counts through
//                        LDS) into the block's slice of the scratch; its count and its NaN flag go to chunk_info.
//   the per-image launch one 1024-thread block per image.
//     phase 1  exclusive scan of the image's chunk counts -> chunk_off (global: up to 65 536 chunks), the number M that qualified
//     phase 2  M > max_candidates only: the key of the max_candidates-th candidate by a radix select over the key bits (four
//              passes of 256 integer histogram counts in LDS), and how many of the candidates with exactly that key take part
//     phase 3  the candidates that take part, in ROW order, into LDS: their 64-bit order keys and where they lie.  Without a
//              selection candidate i is found by bisection in chunk_off (one thread per candidate); with one, an ordered
//              compaction (block scans) that gives the equal keys at the cut to the lowest rows
//     phase 4  the order by counting: a candidate's position is the number of order keys below its own (no two are equal)
//     phase 5  boxes, areas, weights and classes in order into LDS (the keys' space is reused)
//     phase 6  the sweep, as pose_nms.hip runs it: a block-uniform loop over the order; each kept candidate computes ONE row of
//              IoUs across the block's threads against the candidates still alive.  No K x K mask exists anywhere.
//     phase 7  the rows and their indices: YOLOV5 one thread per kept candidate; YOLOV3 one wave per kept candidate, which finds the
//              candidates it suppressed by ballot and adds them in ascending position; then the zero rows, the -1s, the count
//              and the status
//
// LDS: 33 bytes per candidate of max_candidates (4096: 132 KiB of gfx950's 160).  No floating-point atomics, no atomics on
// global memory; the LDS histogram counts are integers whose arrival order cannot reach an output.  Every output byte has one
// writer.
#include <hip/hip_runtime.h>

#include "detector_nms_math.h"
#include "kernels.h"

namespace hrn {

namespace {

constexpr int kImageThreads = 1024, kImageWaves = kImageThreads / 64;
constexpr int kNanBit = 1 << 30;   // of chunk_info

__global__ __launch_bounds__(kDnmsChunk) void dnms_score_kernel(DetectorNmsArgs a) {
#pragma clang fp contract(off)
    __shared__ int s_wave[kDnmsChunk / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x;
    const size_t stride = (size_t)5 + a.C;
    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        const int row = chunk * kDnmsChunk + tid;
        const size_t at = ((size_t)b * a.N + row) * stride;   // (read only when row < N)
        float obj = 0.0f;
        bool pass = false;
        if (row < a.N) {
            obj = dnms_load(a.pred, a.dtype, at + 4);
            pass = dnms_obj_passes(a.rule, obj, a.conf_thres);
        }
        // the best class of every row of this wave that passed: the wave takes them one by one, a lane per class
        unsigned long long todo = __ballot(pass);
        float my_conf = 0.0f;
        int my_best = 0;
        while (todo) {   // (wave-uniform)
            const int owner = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const size_t cls = ((size_t)b * a.N + (chunk * kDnmsChunk + wave * 64 + owner)) * stride + 5;
            DnmsBest best{0.0f, 0, false};
            float first = 0.0f;
            for (int c = lane; c < a.C; c += 64) {
                const float v = dnms_load(a.pred, a.dtype, cls + c);
                if (c == 0) first = v;
                if (v == v) best = dnms_best_join(best, DnmsBest{v, c, true});
            }
            for (int off = 32; off; off >>= 1) {
                DnmsBest o;
                o.v = __shfl_xor(best.v, off), o.idx = __shfl_xor(best.idx, off), o.present = __shfl_xor((int)best.present, off) != 0;
                best = dnms_best_join(best, o);
            }
            first = __shfl(first, 0);
            if (first != first) best.v = first, best.idx = 0;   // a NaN cls_0 stays
            if (lane == owner) my_conf = best.v, my_best = best.idx;
        }
        DnmsCand c;
        int what = 0;
        if (pass)
            what = dnms_candidate(a.rule, a.conf_thres, dnms_load(a.pred, a.dtype, at), dnms_load(a.pred, a.dtype, at + 1),
                                  dnms_load(a.pred, a.dtype, at + 2), dnms_load(a.pred, a.dtype, at + 3), obj, my_conf, my_best, row, &c);
        // the block's candidates in row order
        const unsigned long long mine = __ballot(what == 1);
        const int nan_key = __syncthreads_or(what == 2);
        if (lane == 0) s_wave[wave] = __popcll(mine);
        __syncthreads();
        int base = 0, total = 0;
        for (int w = 0; w < kDnmsChunk / 64; ++w) {
            const int n = s_wave[w];
            if (w < wave) base += n;
            total += n;
        }
        if (what == 1) a.cand[(size_t)b * a.N + chunk * kDnmsChunk + base + __popcll(mine & ((1ull << lane) - 1))] = c;
        if (tid == 0) a.chunk_info[(size_t)b * a.nchunks + chunk] = total | (nan_key ? kNanBit : 0);
        __syncthreads();   // s_wave is rewritten for the next image
    }
}

// exclusive scan of one int per thread over the block, and the block's total; every thread calls it
__device__ inline int dnms_block_scan(int v, int *s_part, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    __syncthreads();   // the previous call's readers are done with s_part
    if (lane == 63) s_part[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < kImageWaves; ++w) {
        const int n = s_part[w];
        if (w < wave) base += n;
        tot += n;
    }
    *total = tot;
    return base + inc - v;
}

__host__ __device__ inline int dnms_lds_slots(int max_candidates) { return (max_candidates + 15) & ~15; }

__global__ __launch_bounds__(kImageThreads) void dnms_image_kernel(DetectorNmsArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem_dnms[];
    __shared__ int s_part[kImageWaves];
    __shared__ unsigned s_hist[256], s_pick[2];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Kc = dnms_lds_slots(a.max_candidates);
    float4 *s_box = (float4 *)smem_dnms;                                  // phase 5 on; before it, its space holds:
    unsigned long long *s_key = (unsigned long long *)smem_dnms;          //   the order keys in row order
    unsigned *s_loc = (unsigned *)(smem_dnms + (size_t)8 * Kc);           //   and where those candidates lie in the scratch
    float *s_area = (float *)(smem_dnms + (size_t)16 * Kc), *s_w = s_area + Kc;
    unsigned *s_src = (unsigned *)(s_w + Kc);                             // where the candidate at each position lies
    unsigned short *s_cls = (unsigned short *)(s_src + Kc), *s_sup = s_cls + Kc;
    unsigned char *s_state = (unsigned char *)(s_sup + Kc);               // 1 alive, 0 suppressed (s_sup: by the keeper at that
                                                                          // position), 2 kept (s_sup: its output row)
    const int *info = a.chunk_info + (size_t)b * a.nchunks;
    int *chunk_off = a.chunk_off + (size_t)b * a.nchunks;
    const DnmsCand *cand = a.cand + (size_t)b * a.N;
    const int rule = a.rule;
    const bool agnostic = (a.flags & kDnmsAgnostic) != 0;

    // ---- phase 1: the scan of the chunk counts ----
    int M = 0, nan_key = 0;
    for (int c0 = 0; c0 < a.nchunks; c0 += kImageThreads) {
        const int c = c0 + tid;
        int v = 0;
        if (c < a.nchunks) {
            const int i = info[c];
            v = i & ~kNanBit, nan_key |= i & kNanBit;
        }
        int tot;
        const int before = dnms_block_scan(v, s_part, &tot);
        if (c < a.nchunks) chunk_off[c] = M + before;
        M += tot;
    }
    int status = __syncthreads_or(nan_key) ? kDnmsNanKey : 0;   // (the barrier behind which chunk_off is read)

    // ---- phase 2: more qualified than take part: the key at the cut ----
    const bool select = M > a.max_candidates;
    unsigned cut = 0;
    int need_equal = 0;
    if (select) {   // (block-uniform)
        status |= kDnmsTruncated;
        unsigned prefix = 0;
        int remaining = a.max_candidates;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            const unsigned above_mask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
            for (int c0 = 0; c0 < a.nchunks; c0 += kImageThreads / kDnmsChunk) {
                const int c = c0 + tid / kDnmsChunk, slot = tid % kDnmsChunk;
                if (c < a.nchunks && slot < (info[c] & ~kNanBit)) {
                    const unsigned kb = dnms_key_bits(dnms_key(cand[c * kDnmsChunk + slot]));
                    if ((kb & above_mask) == prefix) atomicAdd(&s_hist[(kb >> shift) & 255u], 1u);
                }
            }
            __syncthreads();
            if (tid == 0) {   // the digit in which the `remaining`-th largest key lies (at least `remaining` keys carry the prefix)
                int d = 255;
                unsigned above = 0;
                while (d > 0 && above + s_hist[d] < (unsigned)remaining) above += s_hist[d], --d;
                s_pick[0] = prefix | ((unsigned)d << shift), s_pick[1] = (unsigned)remaining - above;
            }
            __syncthreads();
            prefix = s_pick[0], remaining = (int)s_pick[1];
        }
        cut = prefix, need_equal = remaining;
    }
    const int K = select ? a.max_candidates : M;

    // ---- phase 3: who takes part, in row order ----
    if (!select) {
        // everybody takes part: candidate i of the image lies in the last chunk whose offset is <= i (an empty chunk shares its
        // offset with the next one), found by bisection in chunk_off
        for (int i = tid; i < M; i += kImageThreads) {
            int lo = 0, hi = a.nchunks - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (chunk_off[mid] <= i) lo = mid;
                else hi = mid - 1;
            }
            unsigned loc = (unsigned)(lo * kDnmsChunk + (i - chunk_off[lo]));
            if (loc >= (unsigned)a.N) loc = (unsigned)a.N - 1;   // (cannot happen; never read beyond the image)
            const DnmsCand &q = cand[loc];
            s_key[i] = dnms_order_key(dnms_key_bits(dnms_key(q)), q.row), s_loc[i] = loc;
        }
    } else {
        // an ordered compaction over all candidates, four chunks at a time: the keys above the cut, and of those at the cut the
        // first need_equal in row order
        int taken = 0, equal_seen = 0;
        for (int c0 = 0; c0 < a.nchunks; c0 += kImageThreads / kDnmsChunk) {
            const int c = c0 + tid / kDnmsChunk, slot = tid % kDnmsChunk;
            const bool valid = c < a.nchunks && slot < (info[c] & ~kNanBit);
            const unsigned loc = (unsigned)(c * kDnmsChunk + slot);
            unsigned kb = 0;
            int row = 0;
            if (valid) {
                const DnmsCand &q = cand[loc];
                kb = dnms_key_bits(dnms_key(q)), row = q.row;
            }
            const bool equal = valid && kb == cut;
            int n_equal, n_take;
            const int equal_rank = equal_seen + dnms_block_scan(equal ? 1 : 0, s_part, &n_equal);
            const bool take = valid && (kb > cut || (equal && equal_rank < need_equal));
            const int pos = taken + dnms_block_scan(take ? 1 : 0, s_part, &n_take);
            if (take && pos < K) s_key[pos] = dnms_order_key(kb, row), s_loc[pos] = loc;
            equal_seen += n_equal, taken += n_take;
        }
    }
    __syncthreads();

    // ---- phase 4: the order ----
    for (int i = tid; i < K; i += kImageThreads) {
        const unsigned long long k = s_key[i];
        int r = 0;
        for (int j = 0; j < K; ++j) r += s_key[j] < k ? 1 : 0;
        s_src[r] = s_loc[i];
    }
    __syncthreads();

    // ---- phase 5: the candidates in order ----
    for (int p = tid; p < K; p += kImageThreads) {
        if (s_src[p] >= (unsigned)a.N) s_src[p] = 0;   // (cannot happen: the positions are a permutation; never read beyond the image)
        const DnmsCand q = cand[s_src[p]];
        s_box[p] = make_float4(q.x1, q.y1, q.x2, q.y2);
        s_area[p] = dnms_area(rule, q), s_w[p] = q.obj;
        s_cls[p] = (unsigned short)q.best, s_sup[p] = 0xFFFFu, s_state[p] = 1;
    }
    __syncthreads();

    // ---- phase 6: the sweep (block-uniform: every wave finds the same next candidate, behind the barrier of the previous keeper) ----
    int kept = 0;
    bool more = false;
    const int lane = tid & 63;
    for (int p = 0;; ++p) {
        while (p < K) {   // the next candidate still alive, 64 positions at a time
            const int j = p + lane;
            const unsigned long long alive = __ballot(j < K && s_state[j] == 1);
            if (alive) {
                p += __ffsll((long long)alive) - 1;
                break;
            }
            p += 64;
        }
        if (p >= K) break;
        if (kept == a.max_det) {
            more = true;
            break;
        }
        const float4 g = s_box[p];
        const float g_area = s_area[p];
        const unsigned short g_cls = s_cls[p];
        for (int q = p + 1 + tid; q < K; q += kImageThreads) {
            if (s_state[q] != 1 || !(agnostic || s_cls[q] == g_cls)) continue;
            const float4 d = s_box[q];
            if (dnms_iou(rule, g.x, g.y, g.z, g.w, g_area, d.x, d.y, d.z, d.w, s_area[q]) > a.iou_thres)
                s_state[q] = 0, s_sup[q] = (unsigned short)p;
        }
        __syncthreads();
        if (tid == 0) s_state[p] = 2, s_sup[p] = (unsigned short)kept;   // (nobody reads position p again before phase 7)
        ++kept;
    }
    __syncthreads();

    // ---- phase 7: the outputs ----
    const int F = dnms_row_floats(rule);
    float *out = a.rows + (size_t)b * a.max_det * F;
    int *index = a.index + (size_t)b * a.max_det;
    if (rule == kDnmsYoloV3) {
        // one WAVE per kept candidate (all lanes hold the same sums): the members of its merge set by ballot, 64 positions at a time,
        // added in ascending position
        for (int p = tid >> 6; p < K; p += kImageWaves) {
            if (s_state[p] != 2) continue;   // (wave-uniform)
            const DnmsCand q = cand[s_src[p]];
            float acc[4], sum;
            dnms_merge_first(q.obj, q.x1, q.y1, q.x2, q.y2, acc, sum);
            for (int j0 = (p + 1) & ~63; j0 < K; j0 += 64) {
                const int j = j0 + lane;
                unsigned long long members = __ballot(j > p && j < K && s_state[j] == 0 && s_sup[j] == p);
                while (members) {
                    const int m = j0 + __ffsll((long long)members) - 1;
                    members &= members - 1;
                    const float4 d = s_box[m];
                    dnms_merge_add(s_w[m], d.x, d.y, d.z, d.w, acc, sum);
                }
            }
            if (lane == 0) {
                float row[7];
                dnms_write_row(rule, q, acc, sum, row);
                const int slot = s_sup[p];
                for (int f = 0; f < 7; ++f) out[(size_t)slot * 7 + f] = row[f];
                index[slot] = q.row;
            }
        }
    } else {
        for (int p = tid; p < K; p += kImageThreads) {
            if (s_state[p] != 2) continue;
            const DnmsCand q = cand[s_src[p]];
            const float none[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            float row[7];
            dnms_write_row(rule, q, none, 0.0f, row);
            const int slot = s_sup[p];
            for (int f = 0; f < 6; ++f) out[(size_t)slot * 6 + f] = row[f];
            index[slot] = q.row;
        }
    }
    for (int k = kept * F + tid; k < a.max_det * F; k += kImageThreads) out[k] = 0.0f;
    for (int k = kept + tid; k < a.max_det; k += kImageThreads) index[k] = -1;
    if (tid == 0) a.counts[b] = kept, a.status[b] = status | (more ? kDnmsMaxDetHit : 0);
}

}  // namespace

size_t detector_nms_lds_bytes(int max_candidates) { return (size_t)33 * dnms_lds_slots(max_candidates); }

hipError_t launch_detector_nms(const DetectorNmsArgs &a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (a.nchunks > 0) {
        hipLaunchKernelGGL(dnms_score_kernel, dim3((unsigned)a.nchunks, (unsigned)(a.B < 65535 ? a.B : 65535)), dim3(kDnmsChunk), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_large_lds<dnms_image_kernel>((int)detector_nms_lds_bytes(kDnmsMaxCandidates), dim3((unsigned)a.B), dim3(kImageThreads),
                                               (int)detector_nms_lds_bytes(a.max_candidates), s, a);
}

}  // namespace hrn
