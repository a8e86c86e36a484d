// The person track table on the GPU (include/hrnet_mi355.h: hrn_track_people_dev): one update of a per-stream table that lives in
// device memory -- who of the tracks (seen or lost for a while) is who of this frame's rows.  One launch per call, one 256-thread
// block per stream; the block owns its stream's table and updates it in place:
//
//   phase 1   thread = slot: liveness, the column rank (counting over the keys in LDS: tracks_math.h's order), the compared state
//             (coast: boxes and joints written to the handle's scratch; otherwise the slot arrays are read where they lie).
//             thread = row: presence, and the compaction of the present rows (ballot + prefix count)
//   phase 2   threads stride over the (present row, live column) pairs through assoc_math.h's assoc_pair; cost and similarity go
//             to the scratch, dense with pitch m
//   phase 3   ONE wave runs the assignment: assoc_assign.h, the text assoc_kernel runs
//   phase 4   acceptance by row; new rows and free slots ranked by ballot + prefix counts; then every slot is written by its own
//             thread (scalars, box, velocity) and the joints by a loop over (slot, component), each with its row
//
// m (live columns) and np (present rows) are block-uniform values in LDS; no barrier sits under a condition, so an empty stream
// reaches every one of them.  No atomics; every byte has one writer.  Every loop but the shared assignment is bounded by C, n * C
// or C * J * 3.  A latency link, like assoc.hip.
#include <hip/hip_runtime.h>

#include "assoc_assign.h"
#include "kernels.h"
#include "tracks_math.h"

namespace hrn {

namespace {
enum { kUntouched = 0, kAccepted = 1, kNew = 2, kFreed = 3, kAged = 4 };   // what this update does to a slot
constexpr long long kDeadKey = 0x7fffffffffffffffLL;
}  // namespace

__global__ __launch_bounds__(256) void tracks_kernel(TracksArgs a) {
#pragma clang fp contract(off)
    __shared__ AssignLds s_assign;
    __shared__ double s_vars[17], s_k[kMaxTracked];
    __shared__ long long s_key[kMaxTracked];
    __shared__ float s_vel[kMaxTracked][2];
    __shared__ int s_prow[kMaxTracked], s_cslot[kMaxTracked], s_col[kMaxTracked], s_rowofcol[kMaxTracked], s_newrow[kMaxTracked];
    __shared__ int s_slotofnew[kMaxTracked], s_kind[kMaxTracked], s_src[kMaxTracked], s_oldid[kMaxTracked], s_oldrow[kMaxTracked];
    __shared__ int s_cnt_rows[4], s_cnt_fresh[4], s_cnt_free[4], s_max[4], s_m, s_np, s_fail;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const TrackProblem pr = a.P == 1 ? a.one : a.table[blockIdx.x];
    const int n = pr.n, C = a.C, J = a.J, per = J * 3;   // n, C <= kMaxTracked: the entry refuses more
    const size_t sb = (size_t)blockIdx.x * C;            // this stream's first slot
    const AssocParams prm = assoc_params(a.pose_alpha, a.similarity_threshold, a.smoothing_alpha);
    double *cost = (double *)(a.scratch + pr.scratch);
    float *sim = (float *)(cost + (size_t)n * C);
    int *cmp_boxes = (int *)(sim + (size_t)n * C);
    float *cmp_pts = (float *)(cmp_boxes + (size_t)C * 4);
    const unsigned long long below = (1ull << lane) - 1ull;

    // ---- phase 1: slots and rows ----
    int id_s = -1, lost_s = 0, hits_s = 0, row_s = -1, box_s[4] = {0, 0, 0, 0};
    float vel_s[2] = {0.0f, 0.0f};
    if (tid < C) {
        id_s = a.slot_id[sb + tid], lost_s = a.slot_lost[sb + tid], hits_s = a.slot_hits[sb + tid], row_s = a.slot_row[sb + tid];
        vel_s[0] = a.slot_vel[(sb + tid) * 2], vel_s[1] = a.slot_vel[(sb + tid) * 2 + 1];
        for (int c = 0; c < 4; ++c) box_s[c] = a.slot_boxes[(sb + tid) * 4 + c];
    }
    const bool live = id_s >= 0;
    const long long key = live ? track_column_key(lost_s, row_s, tid) : kDeadKey;
    const double k_s = track_k(a.coast, lost_s);
    s_key[tid] = key, s_k[tid] = k_s, s_vel[tid][0] = vel_s[0], s_vel[tid][1] = vel_s[1];
    s_oldid[tid] = id_s, s_oldrow[tid] = lost_s == 0 ? row_s : -1;
    if (live && a.coast)
        for (int c = 0; c < 4; ++c) cmp_boxes[tid * 4 + c] = track_compared_box(box_s[c], track_box_axis(vel_s, c), k_s);
    const bool present = tid < n && track_present(a.boxes + (size_t)(pr.cur0 + tid) * 4);
    const unsigned long long rows_here = __ballot(present);
    if (lane == 0) s_cnt_rows[wave] = __popcll(rows_here);
    if (tid < 17) s_vars[tid] = assoc_coco_var(tid);
    s_col[tid] = -1, s_rowofcol[tid] = -1, s_kind[tid] = kUntouched, s_src[tid] = -1;
    if (tid == 0) s_fail = 0;
    __syncthreads();
    int myr = -1;                                        // this row among the present ones
    if (present) {
        myr = __popcll(rows_here & below);
        for (int w = 0; w < wave; ++w) myr += s_cnt_rows[w];
        s_prow[myr] = tid;
    }
    int rank = 0, live_slots = 0;
    for (int t = 0; t < C; ++t) {
        const long long kt = s_key[t];
        live_slots += kt != kDeadKey ? 1 : 0;
        rank += kt < key ? 1 : 0;                        // (a dead key is below nothing)
    }
    const int mycol = live ? rank : -1;
    if (live) s_cslot[mycol] = tid;
    if (tid == 0) s_m = live_slots, s_np = s_cnt_rows[0] + s_cnt_rows[1] + s_cnt_rows[2] + s_cnt_rows[3];
    if (a.coast)                                         // the compared joints of the live slots
        for (int idx = tid; idx < C * per; idx += 256) {
            const int s = idx / per, e = idx - s * per;
            if (s_key[s] != kDeadKey) cmp_pts[idx] = track_compared_joint(a.slot_pts[sb * per + idx], s_vel[s], e % 3, s_k[s]);
        }
    __syncthreads();                                     // (also publishes the compared state in the scratch to the block)
    const int m = s_m, np = s_np;
    const int *d_boxes = a.coast ? cmp_boxes : a.slot_boxes + sb * 4;
    const float *d_pts = a.coast ? cmp_pts : a.slot_pts + sb * per;

    // ---- phase 2: cost and similarity of every (present row, live column) pair ----
    int replaced = 0;
    for (int pair = tid; pair < np * m; pair += 256) {
        const int r = pair / m, k = pair - r * m, i = s_prow[r], s = s_cslot[k];
        replaced |= assoc_pair(a.pts + (size_t)(pr.cur0 + i) * per, d_pts + (size_t)s * per, J, a.boxes + (size_t)(pr.cur0 + i) * 4,
                               d_boxes + (size_t)s * 4, s_vars, prm, &cost[pair], &sim[pair]);
    }
    int status = __syncthreads_or(replaced) ? 1 : 0;     // (the barrier also publishes the scratch to the block)

    // ---- phase 3: the assignment, one wave ----
    if (wave == 0 && m > 0 && np > 0) {
        if (!assoc_assign_wave(cost, np, m, lane, s_assign, s_col) && lane == 0) s_fail = 1;
    }
    __syncthreads();
    if (s_fail) status |= 2;

    // ---- phase 4: acceptance, ranks, and the writes ----
    const int next = a.next_id[blockIdx.x];
    int col = -1;
    if (present) {
        const int c = s_col[myr];
        if (c >= 0 && assoc_accepted(sim[(size_t)myr * m + c], prm)) col = c, s_rowofcol[c] = tid;
    }
    const bool fresh = present && col < 0;
    const unsigned long long fresh_here = __ballot(fresh);
    if (lane == 0) s_cnt_fresh[wave] = __popcll(fresh_here);
    __syncthreads();
    int fr = -1;                                         // this row among the new people
    if (fresh) {
        fr = __popcll(fresh_here & below);
        for (int w = 0; w < wave; ++w) fr += s_cnt_fresh[w];
        s_newrow[fr] = tid;
    }
    const int nnew = s_cnt_fresh[0] + s_cnt_fresh[1] + s_cnt_fresh[2] + s_cnt_fresh[3];
    int kind = kUntouched, src = -1;
    if (live) {
        src = s_rowofcol[mycol];
        kind = src >= 0 ? kAccepted : track_retired(lost_s, a.max_lost) ? kFreed : kAged;
    }
    const bool is_free = tid < C && (!live || kind == kFreed);
    const unsigned long long free_here = __ballot(is_free);
    if (lane == 0) s_cnt_free[wave] = __popcll(free_here);
    __syncthreads();
    const int nfree = s_cnt_free[0] + s_cnt_free[1] + s_cnt_free[2] + s_cnt_free[3];
    int q = -1;                                          // this slot among the free ones
    if (is_free) {
        q = __popcll(free_here & below);
        for (int w = 0; w < wave; ++w) q += s_cnt_free[w];
        if (q < nnew) kind = kNew, src = s_newrow[q], s_slotofnew[q] = tid;
    }
    s_kind[tid] = kind, s_src[tid] = src;
    if (nnew > nfree) status |= kTrackStatusFull;
    __syncthreads();

    // thread = row: ids, match_row, slot
    int id = -2147483647 - 1;
    if (tid < n) {
        int mr = -1, sl = -1;
        if (!present) {
            id = -1;
        } else if (col >= 0) {
            sl = s_cslot[col], id = s_oldid[sl], mr = s_oldrow[sl];
        } else {
            id = assoc_fresh_id(next, fr), sl = fr < nfree ? s_slotofnew[fr] : -1;
        }
        a.ids[pr.cur0 + tid] = id, a.match_row[pr.cur0 + tid] = mr, a.slot[pr.cur0 + tid] = sl;
        if (!present) id = -2147483647 - 1;              // an absent row's -1 is nobody's id
    }
    int mx = id;
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(mx, o);
        mx = w > mx ? w : mx;
    }
    if (lane == 0) s_max[wave] = mx;

    // thread = slot: scalars, box, velocity
    if (kind == kAccepted) {
        int box[4];
        for (int c = 0; c < 4; ++c) box[c] = a.boxes[(size_t)(pr.cur0 + src) * 4 + c];
        track_accept_box(box, box_s, vel_s, lost_s, hits_s, a.coast, a.velocity_alpha, prm);
        for (int c = 0; c < 4; ++c) {
            if (prm.smoothing != 0.0) a.boxes[(size_t)(pr.cur0 + src) * 4 + c] = box[c];
            a.slot_boxes[(sb + tid) * 4 + c] = box_s[c];
        }
        a.slot_vel[(sb + tid) * 2] = vel_s[0], a.slot_vel[(sb + tid) * 2 + 1] = vel_s[1];
        a.slot_lost[sb + tid] = 0, a.slot_hits[sb + tid] = track_hits(hits_s), a.slot_row[sb + tid] = src;
    } else if (kind == kNew) {
        for (int c = 0; c < 4; ++c) a.slot_boxes[(sb + tid) * 4 + c] = a.boxes[(size_t)(pr.cur0 + src) * 4 + c];
        a.slot_vel[(sb + tid) * 2] = 0.0f, a.slot_vel[(sb + tid) * 2 + 1] = 0.0f;
        a.slot_id[sb + tid] = assoc_fresh_id(next, q);
        a.slot_lost[sb + tid] = 0, a.slot_hits[sb + tid] = 1, a.slot_row[sb + tid] = src;
    } else if (kind == kFreed) {
        for (int c = 0; c < 4; ++c) a.slot_boxes[(sb + tid) * 4 + c] = 0;
        a.slot_vel[(sb + tid) * 2] = 0.0f, a.slot_vel[(sb + tid) * 2 + 1] = 0.0f;
        a.slot_id[sb + tid] = -1, a.slot_lost[sb + tid] = 0, a.slot_hits[sb + tid] = 0, a.slot_row[sb + tid] = -1;
    } else if (kind == kAged) {
        a.slot_lost[sb + tid] = lost_s + 1, a.slot_row[sb + tid] = -1;
    }

    // the joints of every slot this update writes, each element with its row's
    for (int idx = tid; idx < C * per; idx += 256) {
        const int s = idx / per, kd = s_kind[s];
        if (kd == kUntouched || kd == kAged) continue;
        float v = 0.0f;
        if (kd != kFreed) {
            float *p = a.pts + (size_t)(pr.cur0 + s_src[s]) * per + (idx - s * per);
            v = *p;
            if (kd == kAccepted && prm.smoothing != 0.0) {
                v = assoc_smooth_joint(v, d_pts[idx], prm);
                *p = v;
            }
        }
        a.slot_pts[sb * per + idx] = v;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) mx = s_max[w] > mx ? s_max[w] : mx;
        if (np > 0) a.next_id[blockIdx.x] = assoc_next_id(next, mx);
        a.status[blockIdx.x] = status;
    }
}

hipError_t launch_tracks(const TracksArgs &a, hipStream_t s) {
    if (a.P <= 0) return hipSuccess;
    hipLaunchKernelGGL(tracks_kernel, dim3((unsigned)a.P), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace hrn
