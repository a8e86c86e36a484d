// The arithmetic and the table logic of the person track table (include/hrnet_mi355.h: hrn_track_people, hrn_track_people_dev),
// written ONCE for the host and the device: every function here is compiled into the host entry (postproc.cpp) and into the kernel
// of tracks.hip, so the two sides cannot drift apart.  Plain C++, fp contraction off, no fast-math, no library call.  Similarity,
// acceptance, smoothing and numbering are assoc_math.h's, unchanged; what this header adds is what a table needs beyond two frames:
//   present     a row is a person iff x2 > x1 && y2 > y1 (the library's "nobody" row is all zeros)
//   order       the columns of the cost matrix: live slots seen in the latest update (slot_lost == 0) by (slot_row, slot index),
//               then the other live slots by slot index -- track_column_key below is that order as one integer
//   compared    where a slot is compared: k = coast ? slot_lost + 1 : 0 updates ahead along its velocity, in fp64, rounded once
//               (box: truncated towards zero after a clamp to the int32 range, NaN: the stored value; joint: to float32).  k == 0
//               is the stored bits themselves.  k is formed in fp64 ((double)slot_lost + 1), so no slot_lost overflows it
//   velocity    of the box centre, (dy, dx) per update, from the RAW current box and the STORED box: d = (c_now - c_stored) /
//               ((double)old_lost + 1); the first one (old hits == 1) is (float)d, later ones (float)(v + va * (d - v)) in fp64; a
//               non-finite component becomes +0.0f
//   ageing      an unaccepted live slot is freed iff slot_lost >= max_lost (that is, slot_lost + 1 > max_lost), else slot_lost + 1
//   hits        min(hits + 1, 2^30), written so that no value overflows
#pragma once

#include "assoc_math.h"

namespace hrn {

constexpr int kTrackHitsCap = 1 << 30;
constexpr int kTrackMaxLost = 1 << 20;
constexpr int kTrackStatusFull = 4;   // status bit 2: a new person found no free slot

__host__ __device__ inline bool track_present(const int32_t *b) { return b[2] > b[0] && b[3] > b[1]; }

// the column order as one key: smaller first.  Seen slots: slot_row * 256 + slot (|slot_row| < 2^31: below 2^40 in size); the
// others: 2^62 + slot
__host__ __device__ inline long long track_column_key(int32_t lost, int32_t row, int slot) {
    return lost == 0 ? (long long)row * kMaxTracked + slot : (1LL << 62) + slot;
}

// k of a slot, as the double every expression uses
__host__ __device__ inline double track_k(int coast, int32_t lost) {
#pragma clang fp contract(off)
    return coast ? (double)lost + 1.0 : 0.0;
}

__host__ __device__ inline int32_t track_compared_box(int32_t b, float v, double k) {
#pragma clang fp contract(off)
    if (k == 0.0) return b;
    const double step = (double)v * k;
    double t = (double)b + step;
    if (t != t) return b;
    if (t < -2147483648.0) t = -2147483648.0;
    if (t > 2147483647.0) t = 2147483647.0;
    return (int32_t)t;
}

// component e of a joint (0: y, 1: x, 2: confidence) `k` updates ahead; vel = (dy, dx)
__host__ __device__ inline float track_compared_joint(float c, const float *vel, int e, double k) {
#pragma clang fp contract(off)
    if (k == 0.0 || e == 2) return c;
    const double step = (double)vel[e] * k;
    return (float)((double)c + step);
}

// box component c (x1, y1, x2, y2) moves along dx for c even, dy for c odd
__host__ __device__ inline float track_box_axis(const float *vel, int c) { return vel[(c & 1) ? 0 : 1]; }

__host__ __device__ inline double track_centre(int32_t lo, int32_t hi) {
#pragma clang fp contract(off)
    return ((double)lo + (double)hi) / 2;
}

__host__ __device__ inline float track_velocity(float vel, double c_now, double c_stored, int32_t old_lost, int32_t old_hits, double va) {
#pragma clang fp contract(off)
    const double d = (c_now - c_stored) / ((double)old_lost + 1.0);
    float v;
    if (old_hits == 1) {
        v = (float)d;
    } else {
        const double corr = va * (d - (double)vel);
        v = (float)((double)vel + corr);
    }
    return v - v == 0.0f ? v : 0.0f;
}

__host__ __device__ inline int32_t track_hits(int32_t hits) { return hits >= kTrackHitsCap - 1 ? kTrackHitsCap : hits + 1; }
__host__ __device__ inline bool track_retired(int32_t lost, int max_lost) { return lost >= max_lost; }

// An accepted pair's box work, one text for both sides: the new velocity from the raw box, then the smoothed box (against the
// compared one) into `box` (the row, in / out) and `slot_box`; vel = (dy, dx) in / out
__host__ __device__ inline void track_accept_box(int32_t *box, int32_t *slot_box, float *vel, int32_t old_lost, int32_t old_hits, int coast,
                                                 double va, const AssocParams &prm) {
#pragma clang fp contract(off)
    const double k = track_k(coast, old_lost);
    int32_t cmp[4];
    for (int c = 0; c < 4; ++c) cmp[c] = track_compared_box(slot_box[c], track_box_axis(vel, c), k);
    const float vy = track_velocity(vel[0], track_centre(box[1], box[3]), track_centre(slot_box[1], slot_box[3]), old_lost, old_hits, va);
    const float vx = track_velocity(vel[1], track_centre(box[0], box[2]), track_centre(slot_box[0], slot_box[2]), old_lost, old_hits, va);
    vel[0] = vy, vel[1] = vx;
    for (int c = 0; c < 4; ++c) {
        const int32_t b = prm.smoothing != 0.0 ? assoc_smooth_box(box[c], cmp[c], prm) : box[c];
        box[c] = b, slot_box[c] = b;
    }
}

// ---- what is wrong with the arguments of the two entries, or nullptr; needs no device -------------------------------------------
inline const char *track_fault(int P, const int32_t *cur_start, int C, int J, const void *boxes, const void *pts, const void *slot_id,
                               const void *slot_lost, const void *slot_hits, const void *slot_row, const void *slot_boxes,
                               const void *slot_pts, const void *slot_vel, const void *next_id, double pose_alpha,
                               double similarity_threshold, double smoothing_alpha, int max_lost, int coast, double velocity_alpha,
                               const void *ids, const void *match_row, const void *slot, const void *status) {
    if (P < 0) return "P is negative";
    if (J < 1 || J > kAssocMaxJoints) return "J must be in [1, HRN_MAX_JOINTS]";
    if (!(pose_alpha - pose_alpha == 0.0) || !(similarity_threshold - similarity_threshold == 0.0))
        return "pose_alpha and similarity_threshold must be finite";
    if (!(smoothing_alpha >= 0.0 && smoothing_alpha <= 1.0)) return "smoothing_alpha must be in [0, 1]";
    if (C < 1 || C > kMaxTracked) return "the table capacity C must be in [1, HRN_MAX_TRACKED]";
    if (max_lost < 0 || max_lost > kTrackMaxLost) return "max_lost must be in [0, 2^20]";
    if (coast != 0 && coast != 1) return "coast must be 0 or 1";
    if (!(velocity_alpha > 0.0 && velocity_alpha <= 1.0)) return "velocity_alpha must be in (0, 1]";
    if (P == 0) return nullptr;
    if (!cur_start || !next_id || !status) return "null segment table / next_id / status";
    if (cur_start[0] < 0) return "a segment table starts below zero";
    for (int p = 0; p < P; ++p) {
        if (cur_start[p + 1] < cur_start[p]) return "a segment table decreases";
        if (cur_start[p + 1] - cur_start[p] > kMaxTracked) return "more than HRN_MAX_TRACKED rows in one stream";
    }
    if (!slot_id || !slot_lost || !slot_hits || !slot_row || !slot_boxes || !slot_pts || !slot_vel) return "null track table arrays";
    if (cur_start[P] > cur_start[0] && (!boxes || !pts || !ids || !match_row || !slot)) return "null boxes / pts / ids / match_row / slot";
    return nullptr;
}

}  // namespace hrn
