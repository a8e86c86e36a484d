// The arithmetic of joints over time (include/hrnet_mi355.h: hrn_filter_poses, hrn_filter_poses_dev): the One-Euro filter
// (Casiez, Roussel, Vogel, CHI 2012) per joint and axis, and the motion lookahead its derivative estimate gives -- written ONCE
// for the host and the device: every function here is compiled into the host entry (postproc.cpp) and into the kernel of
// temporal.hip, so the two sides cannot drift apart.  Plain C++, fp contraction off, doubles, a fixed operation order, no library
// call: every operation is one correctly rounded IEEE operation, the same bits on both sides.
//
//   state    (n, J, 6) float32 = (y_raw, x_raw, y_hat, x_hat, dy_hat, dx_hat);  age (n, J) int32: 0 no state, 1 initialised by this
//            update, otherwise the previous age + 1, saturating at 2^30
//   alpha    alpha(fc) = 1.0 / (1.0 + (1.0 / (TWO_PI * fc)) / dt), TWO_PI = 6.283185307179586, in exactly this order
//   LIVE     confidence > threshold (a float32 compare: equality and NaN are not live) and y, x finite -- hrn_pose_boxes' predicate
//   PRIOR    the person's match lies in [0, m) of its problem and that previous person's age[j] > 0
//   not live             outputs carry the input through bit for bit; the six state values are +0.0f, age 0
//   live, no prior       raw = hat = the input's bits, d_hat = +0.0f, age 1; output and prediction equal the input
//   live with a prior    per axis, y then x, with x = (double)v and r, p, d the previous raw, hat, d_hat widened:
//                            raw_d = (x - r) / dt                      the derivative of RAW samples, as in the paper's reference code
//                            dh    = d + alpha(d_cutoff) * (raw_d - d)
//                            fc    = min_cutoff + beta * fabs(dh)
//                            xh    = p + alpha(fc) * (x - p)           the lerp form: a constant input is a fixed point, exactly
//                            store (float)xh, (float)dh, raw = v;  age = min(previous age + 1, 2^30)
//                            pred  = (float)(x + (double)(float)dh * lookahead)
//                        (float)xh or (float)dh of either axis not finite: the whole joint is re-initialised as "live, no prior"
//                        (a stored state is therefore always finite); a non-finite pred component becomes the input's
//   The confidence is copied untouched into both outputs.  The prediction starts from the RAW position on purpose: on steady
//   motion the filtered position lags (the filter's known trade, tuned by beta) while raw + velocity converges to zero error.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace hrn {

constexpr int kTemporalMaxJoints = 256;        // = HRN_MAX_JOINTS
constexpr int32_t kTemporalMaxAge = 1 << 30;

// the parameters of one call as the expressions above use them; alpha(d_cutoff) is the same for every joint
struct TemporalParams {
    double dt, min_cutoff, beta, lookahead, alpha_d;
    float threshold;
};

__host__ __device__ inline double temporal_alpha(double fc, double dt) {
#pragma clang fp contract(off)
    return 1.0 / (1.0 + (1.0 / (6.283185307179586 * fc)) / dt);
}

inline TemporalParams temporal_params(double dt, double min_cutoff, double beta, double d_cutoff, float threshold, double lookahead) {
    TemporalParams p;
    p.dt = dt, p.min_cutoff = min_cutoff, p.beta = beta, p.lookahead = lookahead, p.threshold = threshold;
    p.alpha_d = temporal_alpha(d_cutoff, dt);
    return p;
}

__host__ __device__ inline bool temporal_finite(float v) { return v - v == 0.0f; }   // (inf - inf and NaN - NaN are NaN)

__host__ __device__ inline bool temporal_live(const float *v, const TemporalParams &prm) {
    return v[2] > prm.threshold && temporal_finite(v[0]) && temporal_finite(v[1]);
}

// one axis of a live joint with a prior: the filtered position, the filtered derivative and the prediction
struct TemporalAxis {
    float hat, dhat, pred;
};
__host__ __device__ inline TemporalAxis temporal_axis(float v, float r, float p, float d, const TemporalParams &prm) {
#pragma clang fp contract(off)
    const double x = (double)v, pd = (double)p, dd = (double)d;
    const double raw_d = (x - (double)r) / prm.dt;
    const double dh = dd + prm.alpha_d * (raw_d - dd);
    const double fc = prm.min_cutoff + prm.beta * __builtin_fabs(dh);
    const double xh = pd + temporal_alpha(fc, prm.dt) * (x - pd);
    TemporalAxis a;
    a.hat = (float)xh, a.dhat = (float)dh;
    a.pred = (float)(x + (double)a.dhat * prm.lookahead);
    if (!temporal_finite(a.pred)) a.pred = v;
    return a;
}

// what one joint of this frame becomes: v = its (y, x, confidence); prev / prev_age = the matched previous person's state and age
// of this joint (read only when has_prior)
struct TemporalJoint {
    float out[2], pred[2], state[6];
    int32_t age;
};
__host__ __device__ inline TemporalJoint temporal_joint(const float *v, bool has_prior, const float *prev, int32_t prev_age,
                                                         const TemporalParams &prm) {
    TemporalJoint t;
    t.out[0] = t.pred[0] = v[0], t.out[1] = t.pred[1] = v[1];
    if (!temporal_live(v, prm)) {
        for (int k = 0; k < 6; ++k) t.state[k] = 0.0f;
        t.age = 0;
        return t;
    }
    if (has_prior) {
        const TemporalAxis y = temporal_axis(v[0], prev[0], prev[2], prev[4], prm), x = temporal_axis(v[1], prev[1], prev[3], prev[5], prm);
        if (temporal_finite(y.hat) && temporal_finite(y.dhat) && temporal_finite(x.hat) && temporal_finite(x.dhat)) {
            t.out[0] = y.hat, t.out[1] = x.hat, t.pred[0] = y.pred, t.pred[1] = x.pred;
            t.state[0] = v[0], t.state[1] = v[1], t.state[2] = y.hat, t.state[3] = x.hat, t.state[4] = y.dhat, t.state[5] = x.dhat;
            t.age = prev_age >= kTemporalMaxAge ? kTemporalMaxAge : prev_age + 1;
            return t;
        }
    }
    t.state[0] = t.state[2] = v[0], t.state[1] = t.state[3] = v[1], t.state[4] = t.state[5] = 0.0f;
    t.age = 1;
    return t;
}

// the previous person of current person with `match` inside a problem with m previous people from prev0, or -1
__host__ __device__ inline long long temporal_previous(int match, int prev0, int m) {
    return match >= 0 && match < m ? (long long)prev0 + match : -1;
}

// ---- what is wrong with the arguments of the two entries, or nullptr; needs no device, reads only the two tables -------------------
inline bool temporal_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

inline const char *temporal_fault(int P, const int32_t *cur_start, const int32_t *prev_start, int J, const void *pts, const void *match,
                                  const void *prev_state, const void *prev_age, double dt, double min_cutoff, double beta, double d_cutoff,
                                  double lookahead, const void *pts_out, const void *state, const void *age) {
    if (P < 0) return "P is negative";
    if (J < 1 || J > kTemporalMaxJoints) return "J must be in [1, HRN_MAX_JOINTS]";
    if (!(dt - dt == 0.0 && dt > 0.0) || !(min_cutoff - min_cutoff == 0.0 && min_cutoff > 0.0) ||
        !(d_cutoff - d_cutoff == 0.0 && d_cutoff > 0.0))
        return "dt, min_cutoff and d_cutoff must be finite and positive";
    if (!(beta - beta == 0.0 && beta >= 0.0) || !(lookahead - lookahead == 0.0 && lookahead >= 0.0))
        return "beta and lookahead must be finite and not negative";
    if (P == 0) return nullptr;
    if (!cur_start || !prev_start) return "null segment tables";
    if (cur_start[0] < 0 || prev_start[0] < 0) return "a segment table starts below zero";
    for (int p = 0; p < P; ++p)
        if (cur_start[p + 1] < cur_start[p] || prev_start[p + 1] < prev_start[p]) return "a segment table decreases";
    const size_t n = (size_t)(cur_start[P] - cur_start[0]), m = (size_t)(prev_start[P] - prev_start[0]);
    if (n == 0) return nullptr;
    if (!pts || !pts_out || !state || !age) return "null pts / pts_out / state / age";
    if (n * (size_t)J > 2147483647u) return "more than 2^31 - 1 (person, joint) pairs in one call";
    const size_t per = (size_t)J;
    const char *s0 = (const char *)state + (size_t)cur_start[0] * per * 24, *a0 = (const char *)age + (size_t)cur_start[0] * per * 4;
    const char *ps0 = prev_state ? (const char *)prev_state + (size_t)prev_start[0] * per * 24 : nullptr;
    const char *pa0 = prev_age ? (const char *)prev_age + (size_t)prev_start[0] * per * 4 : nullptr;
    if (temporal_overlap(s0, n * per * 24, ps0, m * per * 24) || temporal_overlap(s0, n * per * 24, pa0, m * per * 4) ||
        temporal_overlap(a0, n * per * 4, ps0, m * per * 24) || temporal_overlap(a0, n * per * 4, pa0, m * per * 4))
        return "state / age overlap prev_state / prev_age";
    if (match && m > 0 && (!prev_state || !prev_age)) return "null prev_state / prev_age beside a match";
    return nullptr;
}

}  // namespace hrn
