// Host-side pose post-processing of the reference, behind the same C ABI (include/hrnet_mi355.h):
//   * OKS non-maximum suppression, hard and soft      misc/nms/nms.py:75-180   (evaluation: datasets/COCO.py:371-374)
//   * tracker: box-IoU / OKS similarity matrices and the optimal assignment   misc/utils.py:251-429
//     (live demo: scripts/live-demo.py:120-123)
//   * person ids and pose NMS in the arithmetic their kernels compile (assoc_math.h, pose_nms_math.h): the host forms of
//     hrn_associate_people_dev and hrn_pose_nms_dev, equal to them bit for bit
//   * joints over time (temporal_math.h): the One-Euro filter and the motion lookahead, the host form of hrn_filter_poses_dev
// These are O(people^2 * joints) on a handful of skeletons: they are host code in the reference (numpy + the munkres
// package) and stay host code here -- a kernel launch costs more than the whole computation.  What matters is that the
// numbers are the reference's: float64 arithmetic in numpy's operation order (its pairwise summation included), float32
// where the reference's arrays are float32, and the reference's quirks kept (the visibility mask that only looks at the
// candidate, `e <= 2^32 - 1` read by Python as `e <= 29`).  No fused multiply-adds: numpy has none.
#include "../../include/hrnet_mi355.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "assoc_math.h"
#include "letterbox_math.h"
#include "pose_nms_math.h"
#include "detector_nms_math.h"
#include "keypoint_eval_math.h"
#include "rotate_math.h"
#include "temporal_math.h"
#include "tracks_math.h"

#pragma clang fp contract(off)

namespace {

const double kCocoSigmas[17] = {.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89};
const double kSpacing1 = 2.220446049250313e-16;  // np.spacing(1)

// numpy's pairwise summation for n <= 128 contiguous doubles (numpy/core/src/umath/loops_utils.h.src: pairwise_sum)
double np_sum(const double *a, int n) {
    if (n < 8) {
        double res = 0.;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int k = 0; k < 8; ++k) r[k] = a[k];
        int i;
        for (i = 8; i < n - (n % 8); i += 8)
            for (int k = 0; k < 8; ++k) r[k] += a[i + k];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_sum(a, n2) + np_sum(a + n2, n - n2);
}

// misc/nms/nms.py:75-94: OKS of skeleton g against skeleton d, both flat (x, y, v) * J, float64
double oks_flat(const double *g, const double *d, double a_g, double a_d, const double *vars, int J, bool use_vis, double vis,
                std::vector<double> &tmp) {
    tmp.clear();
    const double denom = (a_g + a_d) / 2 + kSpacing1;
    for (int j = 0; j < J; ++j) {
        const double dx = d[3 * j] - g[3 * j], dy = d[3 * j + 1] - g[3 * j + 1];
        const double e = (dx * dx + dy * dy) / vars[j] / denom / 2;
        // `list(vg > t) and list(vd > t)` is the SECOND list whenever the first is non-empty: the mask is the candidate's
        if (use_vis && !(d[3 * j + 2] > vis)) continue;
        tmp.push_back(std::exp(-e));
    }
    return tmp.empty() ? 0.0 : np_sum(tmp.data(), (int)tmp.size()) / (double)tmp.size();
}

void make_vars(const double *sigmas, int J, std::vector<double> &vars) {
    vars.resize(J);
    for (int j = 0; j < J; ++j) {
        const double s = sigmas ? sigmas[j] : kCocoSigmas[j] / 10.0;
        vars[j] = (s * 2) * (s * 2);
    }
}

}  // namespace

extern "C" {

int hrn_oks_nms(int32_t *keep_out, int32_t *num_out, const double *kpts, const double *areas, const int32_t *order, int n, int J,
                double thresh, const double *sigmas, double in_vis_thre) {
    if (!keep_out || !num_out || n < 0 || J <= 0 || (n && (!kpts || !areas || !order)) || (!sigmas && J != 17)) return 1;
    std::vector<double> vars, tmp;
    make_vars(sigmas, J, vars);
    const bool use_vis = !std::isnan(in_vis_thre);
    std::vector<int> cur(order, order + n), nxt;
    int kept = 0;
    while (!cur.empty()) {
        const int i = cur[0];
        keep_out[kept++] = i;
        nxt.clear();
        for (size_t k = 1; k < cur.size(); ++k) {
            const int c = cur[k];
            const double o = oks_flat(kpts + (size_t)i * 3 * J, kpts + (size_t)c * 3 * J, areas[i], areas[c], vars.data(), J, use_vis,
                                      in_vis_thre, tmp);
            if (o <= thresh) nxt.push_back(c);
        }
        cur.swap(nxt);
    }
    *num_out = kept;
    return 0;
}

int hrn_soft_oks_nms(int32_t *keep_out, int32_t *num_out, const double *kpts, const double *areas, const double *scores_sorted,
                     const int32_t *order, int n, int J, double thresh, const double *sigmas, double in_vis_thre) {
    if (!keep_out || !num_out || n < 0 || J <= 0 || (n && (!kpts || !areas || !order || !scores_sorted)) || (!sigmas && J != 17))
        return 1;
    std::vector<double> vars, tmp;
    make_vars(sigmas, J, vars);
    const bool use_vis = !std::isnan(in_vis_thre);
    std::vector<int> cur(order, order + n);
    std::vector<double> sc(scores_sorted, scores_sorted + n);
    const int max_dets = 20;  // misc/nms/nms.py:156
    int kept = 0;
    while (!cur.empty() && kept < max_dets) {
        const int i = cur[0];
        const size_t m = cur.size() - 1;
        std::vector<int> rest(cur.begin() + 1, cur.end());
        std::vector<double> rs(m);
        for (size_t k = 0; k < m; ++k) {
            const int c = rest[k];
            const double o = oks_flat(kpts + (size_t)i * 3 * J, kpts + (size_t)c * 3 * J, areas[i], areas[c], vars.data(), J, use_vis,
                                      in_vis_thre, tmp);
            rs[k] = sc[k + 1] * std::exp(-(o * o) / thresh);  // rescore(..., type='gaussian')
        }
        std::vector<int> idx(m);
        std::iota(idx.begin(), idx.end(), 0);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return rs[a] > rs[b]; });  // argsort()[::-1]
        cur.resize(m), sc.resize(m);
        for (size_t k = 0; k < m; ++k) cur[k] = rest[idx[k]], sc[k] = rs[idx[k]];
        keep_out[kept++] = i;
    }
    *num_out = kept;
    return 0;
}

// misc/utils.py:372-384 (compute_similarity_matrices) with bbox_iou (:318-334) and oks_iou (:341-369)
int hrn_pose_similarity(const double *boxes_a, const float *poses_a, int na, const double *boxes_b, const float *poses_b, int nb, int J,
                        float *sim_bbox, float *sim_pose) {
    if (na < 0 || nb < 0 || J <= 0 || (na && (!boxes_a || !poses_a)) || (nb && (!boxes_b || !poses_b)) ||
        (na && nb && (!sim_bbox || !sim_pose)))
        return 1;
    auto area = [](const double *b) { return (b[2] - b[0]) * (b[3] - b[1]); };
    // sigmas: COCO's as float64 for 17 joints, float32 ones / 10 otherwise (:343-348) -- the dtype decides where the
    // first division is rounded
    const bool coco = J == 17;
    std::vector<double> vars64(J);
    std::vector<float> vars32(J);
    for (int j = 0; j < J; ++j) {
        const double s = kCocoSigmas[j % 17] / 10.0;
        vars64[j] = (s * 2) * (s * 2);
        const float s32 = 1.0f / 10.0f;
        vars32[j] = (s32 * 2) * (s32 * 2);
    }
    std::vector<double> tmp;
    for (int i = 0; i < na; ++i) {
        const float *g = poses_a + (size_t)i * J * 3;
        const double a_g = area(boxes_a + 4 * i);
        for (int k = 0; k < nb; ++k) {
            const float *d = poses_b + (size_t)k * J * 3;
            const double denom = (a_g + area(boxes_b + 4 * k)) / 2 + kSpacing1;
            tmp.clear();
            for (int j = 0; j < J; ++j) {
                const float dy = d[3 * j] - g[3 * j], dx = d[3 * j + 1] - g[3 * j + 1];   // (y, x, v) float32 arrays
                const float sq = dx * dx + dy * dy;
                const double e = (coco ? (double)sq / vars64[j] : (double)(sq / vars32[j])) / denom / 2;
                if (e <= 29) tmp.push_back(std::exp(-e));   // `e[e <= 2^32 - 1]`: ^ is XOR in Python, 2 ^ 31 == 29
            }
            sim_pose[(size_t)i * nb + k] = (float)(tmp.empty() ? 0.0 : np_sum(tmp.data(), (int)tmp.size()) / (double)tmp.size());
            // box IoU: intersection limits, zero area when disjoint, union = a + b - i (:269-334)
            const double *p = boxes_a + 4 * i, *q = boxes_b + 4 * k;
            const double x1 = std::max(p[0], q[0]), x2 = std::min(p[2], q[2]), y1 = std::max(p[1], q[1]), y2 = std::min(p[3], q[3]);
            const double area_i = (x2 < x1 || y2 < y1) ? 0.0 : (x2 - x1) * (y2 - y1);
            const double area_u = area(p) + area(q) - area_i;
            sim_bbox[(size_t)i * nb + k] = (float)(area_i / area_u);
        }
    }
    return 0;
}

// Minimum-cost assignment of a rows x cols matrix (what Munkres().compute() returns, misc/utils.py:406-407): every row gets
// a column when rows <= cols, otherwise every column gets a row; row_to_col[r] = column or -1.  Shortest augmenting paths
// with potentials, O(n^2 m).
int hrn_assignment(const double *cost, int rows, int cols, int32_t *row_to_col) {
    if (rows < 0 || cols < 0 || (rows && !row_to_col) || (rows && cols && !cost)) return 1;
    for (int r = 0; r < rows; ++r) row_to_col[r] = -1;
    if (rows == 0 || cols == 0) return 0;
    const bool transposed = rows > cols;
    const int n = transposed ? cols : rows, m = transposed ? rows : cols;  // n <= m
    auto c = [&](int i, int j) { return transposed ? cost[(size_t)j * cols + i] : cost[(size_t)i * cols + j]; };
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> u(n + 1, 0.0), v(m + 1, 0.0), minv(m + 1);
    std::vector<int> p(m + 1, 0), way(m + 1, 0);
    std::vector<char> used(m + 1);
    for (int i = 1; i <= n; ++i) {
        p[0] = i;
        int j0 = 0;
        std::fill(minv.begin(), minv.end(), inf);
        std::fill(used.begin(), used.end(), 0);
        do {
            used[j0] = 1;
            const int i0 = p[j0];
            double delta = inf;
            int j1 = 0;
            for (int j = 1; j <= m; ++j)
                if (!used[j]) {
                    const double cur = c(i0 - 1, j - 1) - u[i0] - v[j];
                    if (cur < minv[j]) minv[j] = cur, way[j] = j0;
                    if (minv[j] < delta) delta = minv[j], j1 = j;
                }
            if (j1 == 0) return 2;  // NaN / inf costs: no augmenting path
            for (int j = 0; j <= m; ++j)
                if (used[j])
                    u[p[j]] += delta, v[j] -= delta;
                else
                    minv[j] -= delta;
            j0 = j1;
        } while (p[j0] != 0);
        do {
            const int j1 = way[j0];
            p[j0] = p[j1];
            j0 = j1;
        } while (j0);
    }
    for (int j = 1; j <= m; ++j)
        if (p[j]) {
            const int small = p[j] - 1, big = j - 1;
            if (transposed)
                row_to_col[big] = small;
            else
                row_to_col[small] = big;
        }
    return 0;
}

// Person re-identification between two frames on the host: P independent problems, each postproc.find_person_id_associations
// followed by the demo's next_id update (scripts/live-demo.py:120-124), in assoc_math.h's arithmetic -- the text the kernel of
// assoc.hip compiles, so hrn_associate_people_dev equals this bit for bit.
namespace {
thread_local std::string g_associate_error;
}

int hrn_associate_people(int P, const int32_t *cur_start, const int32_t *prev_start, int J, int32_t *boxes, float *pts,
                         const int32_t *prev_boxes, const float *prev_pts, const int32_t *prev_ids, int32_t *next_id, double pose_alpha,
                         double similarity_threshold, double smoothing_alpha, int32_t *ids, int32_t *match, int32_t *status) {
    using namespace hrn;
    if (const char *fault = assoc_fault(P, cur_start, prev_start, J, boxes, pts, prev_boxes, prev_pts, prev_ids, next_id, pose_alpha,
                                        similarity_threshold, smoothing_alpha, ids, match, status)) {
        g_associate_error = fault;
        return 7;
    }
    const AssocParams prm = assoc_params(pose_alpha, similarity_threshold, smoothing_alpha);
    double vars[17];
    for (int j = 0; j < 17; ++j) vars[j] = assoc_coco_var(j);
    std::vector<double> cost;
    std::vector<float> sim;
    std::vector<int32_t> col;
    const size_t per = (size_t)J * 3;
    for (int p = 0; p < P; ++p) {
        const int cur0 = cur_start[p], n = cur_start[p + 1] - cur0, prev0 = prev_start[p], m = prev_start[p + 1] - prev0;
        status[p] = 0;
        if (n == 0) continue;   // nobody here: next_id stays
        cost.assign((size_t)n * m, 0.0), sim.assign((size_t)n * m, 0.0f), col.assign(n, -1);
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < m; ++k)
                status[p] |= assoc_pair(pts + (cur0 + i) * per, prev_pts + (prev0 + k) * per, J, boxes + (size_t)(cur0 + i) * 4,
                                        prev_boxes + (size_t)(prev0 + k) * 4, vars, prm, &cost[(size_t)i * m + k], &sim[(size_t)i * m + k]);
        if (m > 0 && hrn_assignment(cost.data(), n, m, col.data()) != 0) {   // (cannot happen: every cost is finite)
            col.assign(n, -1);
            status[p] |= 2;
        }
        int rank = 0;
        int32_t max_id = std::numeric_limits<int32_t>::min();
        for (int i = 0; i < n; ++i) {
            const int c = col[i];
            const bool accepted = c >= 0 && assoc_accepted(sim[(size_t)i * m + c], prm);
            int32_t id = accepted ? prev_ids[prev0 + c] : -1;
            if (id == -1) id = assoc_fresh_id(next_id[p], rank++);
            ids[cur0 + i] = id, match[cur0 + i] = accepted ? c : -1;
            max_id = std::max(max_id, id);
            if (accepted && prm.smoothing != 0.0) {
                for (int k = 0; k < 4; ++k) {
                    int32_t *b = boxes + (size_t)(cur0 + i) * 4 + k;
                    *b = assoc_smooth_box(*b, prev_boxes[(size_t)(prev0 + c) * 4 + k], prm);
                }
                for (size_t e = 0; e < per; ++e) {
                    float *q = pts + (cur0 + i) * per + e;
                    *q = assoc_smooth_joint(*q, prev_pts[(prev0 + c) * per + e], prm);
                }
            }
        }
        next_id[p] = assoc_next_id(next_id[p], max_id);
    }
    return 0;
}

const char *hrn_associate_people_last_error(void) { return g_associate_error.c_str(); }

// One update of P per-stream track tables on the host (include/hrnet_mi355.h states the eight steps), in tracks_math.h's and
// assoc_math.h's arithmetic -- the text the kernel of tracks.hip compiles, so hrn_track_people_dev equals this bit for bit.
namespace {
thread_local std::string g_track_people_error;
}

int hrn_track_people(int P, const int32_t *cur_start, int C, int J, int32_t *boxes, float *pts, int32_t *slot_id, int32_t *slot_lost,
                     int32_t *slot_hits, int32_t *slot_row, int32_t *slot_boxes, float *slot_pts, float *slot_vel, int32_t *next_id,
                     double pose_alpha, double similarity_threshold, double smoothing_alpha, int max_lost, int coast,
                     double velocity_alpha, int32_t *ids, int32_t *match_row, int32_t *slot, int32_t *status) {
    using namespace hrn;
    if (const char *fault = track_fault(P, cur_start, C, J, boxes, pts, slot_id, slot_lost, slot_hits, slot_row, slot_boxes, slot_pts,
                                        slot_vel, next_id, pose_alpha, similarity_threshold, smoothing_alpha, max_lost, coast,
                                        velocity_alpha, ids, match_row, slot, status)) {
        g_track_people_error = fault;
        return 7;
    }
    const AssocParams prm = assoc_params(pose_alpha, similarity_threshold, smoothing_alpha);
    double vars[17];
    for (int j = 0; j < 17; ++j) vars[j] = assoc_coco_var(j);
    const size_t per = (size_t)J * 3;
    std::vector<double> cost;
    std::vector<float> sim, cmp_pts((size_t)C * per);
    std::vector<int32_t> col, cmp_boxes((size_t)C * 4);
    std::vector<int> rows, cols, row_of_slot(C);
    std::vector<std::pair<long long, int>> order;
    for (int p = 0; p < P; ++p) {
        const int cur0 = cur_start[p], n = cur_start[p + 1] - cur0;
        int32_t *sid = slot_id + (size_t)p * C, *slost = slot_lost + (size_t)p * C, *shits = slot_hits + (size_t)p * C;
        int32_t *srow = slot_row + (size_t)p * C, *sbox = slot_boxes + (size_t)p * C * 4;
        float *spts = slot_pts + (size_t)p * C * per, *svel = slot_vel + (size_t)p * C * 2;
        status[p] = 0;
        // steps 1-3: the present rows, the live columns in order, their compared state
        rows.clear(), order.clear(), cols.clear();
        for (int i = 0; i < n; ++i) {
            ids[cur0 + i] = match_row[cur0 + i] = slot[cur0 + i] = -1;
            if (track_present(boxes + (size_t)(cur0 + i) * 4)) rows.push_back(i);
        }
        for (int s = 0; s < C; ++s)
            if (sid[s] >= 0) order.emplace_back(track_column_key(slost[s], srow[s], s), s);
        std::sort(order.begin(), order.end());
        for (const auto &o : order) cols.push_back(o.second);
        for (int s : cols) {
            const double k = track_k(coast, slost[s]);
            for (int c = 0; c < 4; ++c) cmp_boxes[(size_t)s * 4 + c] = track_compared_box(sbox[(size_t)s * 4 + c], track_box_axis(svel + s * 2, c), k);
            for (size_t e = 0; e < per; ++e) cmp_pts[s * per + e] = track_compared_joint(spts[s * per + e], svel + s * 2, (int)(e % 3), k);
        }
        // step 4: the association
        const int np = (int)rows.size(), m = (int)cols.size();
        cost.assign((size_t)np * m, 0.0), sim.assign((size_t)np * m, 0.0f), col.assign(np, -1);
        for (int r = 0; r < np; ++r)
            for (int k = 0; k < m; ++k)
                status[p] |= assoc_pair(pts + (cur0 + rows[r]) * per, &cmp_pts[cols[k] * per], J, boxes + (size_t)(cur0 + rows[r]) * 4,
                                        &cmp_boxes[(size_t)cols[k] * 4], vars, prm, &cost[(size_t)r * m + k], &sim[(size_t)r * m + k]);
        if (np > 0 && m > 0 && hrn_assignment(cost.data(), np, m, col.data()) != 0) {   // (cannot happen: every cost is finite)
            col.assign(np, -1);
            status[p] |= 2;
        }
        // step 5: accepted pairs
        std::fill(row_of_slot.begin(), row_of_slot.end(), -1);
        int32_t max_id = std::numeric_limits<int32_t>::min();
        for (int r = 0; r < np; ++r) {
            const int c = col[r], i = rows[r];
            if (c < 0 || !assoc_accepted(sim[(size_t)r * m + c], prm)) continue;
            const int s = cols[c];
            row_of_slot[s] = i;
            ids[cur0 + i] = sid[s], match_row[cur0 + i] = slost[s] == 0 ? srow[s] : -1, slot[cur0 + i] = s;
            max_id = std::max(max_id, sid[s]);
            int32_t *box = boxes + (size_t)(cur0 + i) * 4;
            track_accept_box(box, sbox + (size_t)s * 4, svel + s * 2, slost[s], shits[s], coast, velocity_alpha, prm);
            for (size_t e = 0; e < per; ++e) {
                float *q = pts + (cur0 + i) * per + e;
                if (prm.smoothing != 0.0) *q = assoc_smooth_joint(*q, cmp_pts[s * per + e], prm);
                spts[s * per + e] = *q;
            }
            slost[s] = 0, shits[s] = track_hits(shits[s]), srow[s] = i;
        }
        // step 6: unaccepted live slots age or are freed
        for (int s : cols) {
            if (row_of_slot[s] >= 0) continue;
            if (track_retired(slost[s], max_lost)) {
                sid[s] = -1, slost[s] = 0, shits[s] = 0, srow[s] = -1, svel[s * 2] = svel[s * 2 + 1] = 0.0f;
                for (int c = 0; c < 4; ++c) sbox[(size_t)s * 4 + c] = 0;
                for (size_t e = 0; e < per; ++e) spts[s * per + e] = 0.0f;
            } else {
                slost[s] += 1, srow[s] = -1;
            }
        }
        // step 7: new people into the free slots, both in ascending order
        int rank = 0, s = 0;
        for (int r = 0; r < np; ++r) {
            const int i = rows[r];
            if (slot[cur0 + i] != -1) continue;   // accepted
            const int32_t id = assoc_fresh_id(next_id[p], rank++);
            ids[cur0 + i] = id;
            max_id = std::max(max_id, id);
            while (s < C && sid[s] >= 0) ++s;
            if (s == C) {
                status[p] |= kTrackStatusFull;
                continue;
            }
            sid[s] = id, slost[s] = 0, shits[s] = 1, srow[s] = i, svel[s * 2] = svel[s * 2 + 1] = 0.0f;
            for (int c = 0; c < 4; ++c) sbox[(size_t)s * 4 + c] = boxes[(size_t)(cur0 + i) * 4 + c];
            for (size_t e = 0; e < per; ++e) spts[s * per + e] = pts[(cur0 + i) * per + e];
            slot[cur0 + i] = s;
        }
        // step 8
        if (np > 0) next_id[p] = assoc_next_id(next_id[p], max_id);
    }
    return 0;
}

const char *hrn_track_people_last_error(void) { return g_track_people_error.c_str(); }

// the (n, m) costs and blended similarities of ONE problem as both entries compute them (assoc_math.h's assoc_pair: the
// similarity is NaN where the blend was not finite), for measuring them against the reference's matrices; returns 0 or 7
int hrn_associate_similarity(const int32_t *boxes, const float *pts, int n, const int32_t *prev_boxes, const float *prev_pts, int m, int J,
                             double pose_alpha, double *cost_out, float *sim_out) {
    using namespace hrn;
    if (n < 0 || m < 0 || J < 1 || J > kAssocMaxJoints || !(pose_alpha - pose_alpha == 0.0) || (n && (!boxes || !pts)) ||
        (m && (!prev_boxes || !prev_pts)) || (n && m && (!cost_out || !sim_out)))
        return 7;
    const AssocParams prm = assoc_params(pose_alpha, 0.0, 0.0);
    double vars[17];
    for (int j = 0; j < 17; ++j) vars[j] = assoc_coco_var(j);
    const size_t per = (size_t)J * 3;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < m; ++k)
            (void)assoc_pair(pts + i * per, prev_pts + k * per, J, boxes + (size_t)i * 4, prev_boxes + (size_t)k * 4, vars, prm,
                             &cost_out[(size_t)i * m + k], &sim_out[(size_t)i * m + k]);
    return 0;
}

// assoc_math.h's exp, n values (its error is measured through this entry)
int hrn_assoc_exp(const double *x, int n, double *out) {
    if (n < 0 || (n && (!x || !out))) return 7;
    for (int i = 0; i < n; ++i) out[i] = hrn::assoc_exp(x[i]);
    return 0;
}

// Pose NMS on the host: P independent problems (the images of an evaluation set, the streams of a camera wall), each rescoring,
// ordering and hard or soft OKS NMS in pose_nms_math.h's arithmetic -- the text the kernel of pose_nms.hip compiles, so
// hrn_pose_nms_dev equals this bit for bit.  (hrn_oks_nms / hrn_soft_oks_nms above keep their libm exp and the caller's order.)
namespace {
thread_local std::string g_pose_nms_error;

hrn::PoseNmsPeople pose_nms_people(int J, int flags, const void *kpts, const void *areas, const void *scores, double in_vis_thre,
                                   double rescore_thre) {
    hrn::PoseNmsPeople p{};
    p.engine = (flags & hrn::kPoseNmsEngine) != 0, p.J = J, p.vis = in_vis_thre, p.rescore = rescore_thre;
    if (p.engine)
        p.pts = (const float *)kpts, p.boxes = (const int32_t *)areas, p.det_scores = (const float *)scores;
    else
        p.kpts = (const double *)kpts, p.areas = (const double *)areas, p.scores = (const double *)scores;
    return p;
}
}  // namespace

int hrn_pose_nms(int P, const int32_t *start, int J, int flags, void *kpts, void *areas, const void *scores, double thresh,
                 double in_vis_thre, double rescore_thre, const double *sigmas, int32_t *keep, int32_t *num, double *scores_out,
                 int32_t *suppressor, int32_t *status) {
    using namespace hrn;
    if (const char *fault = pose_nms_fault(P, start, J, flags, kpts, areas, scores, thresh, sigmas, keep, num, scores_out, suppressor,
                                           status)) {
        g_pose_nms_error = fault;
        return 7;
    }
    const PoseNmsPeople ppl = pose_nms_people(J, flags, kpts, areas, scores, in_vis_thre, rescore_thre);
    std::vector<double> vars(J), gx(J), gy(J), sc, rs, sc2;
    std::vector<int> ord, ord2;
    std::vector<char> alive;
    for (int j = 0; j < J; ++j) vars[j] = pose_nms_var(sigmas, j);
    auto stage = [&](size_t g) {
        for (int j = 0; j < J; ++j) gx[j] = pose_nms_x(ppl, g, j), gy[j] = pose_nms_y(ppl, g, j);
    };
    for (int p = 0; p < P; ++p) {
        const size_t first = (size_t)start[p];
        const int n = start[p + 1] - start[p];
        int st = 0, bad = 0, kept = 0;
        sc.resize(n), ord.resize(n), sc2.resize(n), ord2.resize(n), rs.resize(n), alive.assign(n, 1);
        for (int i = 0; i < n; ++i) {
            sc[i] = scores_out[first + i] = pose_nms_score(ppl, first + i);
            if (sc[i] != sc[i]) st |= 1;
            suppressor[first + i] = -1;
        }
        for (int i = 0; i < n; ++i) ord[pose_nms_rank(sc.data(), n, i)] = i;
        if (!(flags & kPoseNmsSoft)) {
            for (int pos = 0; pos < n; ++pos) {
                const int i = ord[pos];
                if (!alive[i]) continue;
                keep[first + kept++] = i;
                stage(first + i);
                const double a_g = pose_nms_area(ppl, first + i);
                for (int q = pos + 1; q < n; ++q) {
                    const int c = ord[q];
                    if (!alive[c]) continue;
                    const double o = pose_nms_oks(ppl, gx.data(), gy.data(), a_g, first + c, pose_nms_area(ppl, first + c), vars.data(), &bad);
                    if (o > thresh) alive[c] = 0, suppressor[first + c] = i;
                }
            }
        } else {
            int m = n;
            for (int q = 0; q < n; ++q) sc2[q] = sc[ord[q]];   // the scores by position
            while (m > 0 && kept < kPoseNmsMaxKeep) {
                const int i = ord[0];
                keep[first + kept++] = i;
                stage(first + i);
                const double a_g = pose_nms_area(ppl, first + i);
                for (int q = 1; q < m; ++q) {
                    const int c = ord[q];
                    const double o = pose_nms_oks(ppl, gx.data(), gy.data(), a_g, first + c, pose_nms_area(ppl, first + c), vars.data(), &bad);
                    rs[q - 1] = pose_nms_soften(sc2[q], o, thresh);
                }
                for (int q = 1; q < m; ++q) {
                    const int r = pose_nms_rank(rs.data(), m - 1, q - 1);
                    ord2[r] = ord[q], sc[r] = rs[q - 1];
                }
                --m;
                std::copy(ord2.begin(), ord2.begin() + m, ord.begin());
                std::copy(sc.begin(), sc.begin() + m, sc2.begin());
            }
            for (int q = 0; q < m; ++q) suppressor[first + ord[q]] = -2;
        }
        for (int q = kept; q < n; ++q) keep[first + q] = -1;
        num[p] = kept, status[p] = st | (bad ? 2 : 0);
        if (flags & kPoseNmsSuppress)   // a person who is not kept: what track_frame gives a lost person
            for (int i = 0; i < n; ++i) {
                if (suppressor[first + i] == -1) continue;
                for (int j = 0; j < J; ++j) ((float *)kpts)[((first + i) * J + j) * 3 + 2] = 0.0f;
                for (int k = 0; k < 4; ++k) ((int32_t *)areas)[(first + i) * 4 + k] = 0;
            }
    }
    return 0;
}

const char *hrn_pose_nms_last_error(void) { return g_pose_nms_error.c_str(); }

// ---- detector NMS on the host (detector_nms_math.h: the text the kernels of detector_nms.hip compile) -----------------------------
// One image after the other, everything sequential: the candidates in row order, the order by sorting the 64-bit order keys (no two
// are equal), the greedy sweep, the YOLOV3 merge in ascending position.  hrn_detector_nms_dev equals this bit for bit.
static thread_local std::string g_detector_nms_error;

int hrn_detector_nms(const void *pred, int dtype, int B, int N, int C, int rule, int flags, float conf_thres, float iou_thres,
                     int max_candidates, int max_det, float *rows, int32_t *index, int32_t *counts, int32_t *status) {
    using namespace hrn;
    if (const char *fault = dnms_fault(pred, dtype, B, N, C, rule, flags, conf_thres, iou_thres, max_candidates, max_det, rows, index,
                                       counts, status)) {
        g_detector_nms_error = fault;
        return 7;
    }
    const int F = dnms_row_floats(rule);
    const size_t stride = (size_t)5 + C;
    const bool agnostic = (flags & kDnmsAgnostic) != 0;
    std::vector<DnmsCand> cand;
    std::vector<std::pair<uint64_t, int>> order;   // (order key, index into cand)
    std::vector<DnmsCand> s;
    std::vector<float> area;
    std::vector<int> state, sup;   // state: 1 alive, 0 suppressed, 2 kept; sup: the position of the keeper that suppressed it
    for (int b = 0; b < B; ++b) {
        int st = 0;
        cand.clear();
        for (int r = 0; r < N; ++r) {
            const size_t at = ((size_t)b * N + r) * stride;
            const float obj = dnms_load(pred, dtype, at + 4);
            if (!dnms_obj_passes(rule, obj, conf_thres)) continue;
            float v = dnms_load(pred, dtype, at + 5);
            int best = 0;
            for (int c = 1; c < C; ++c) dnms_best_step(v, best, dnms_load(pred, dtype, at + 5 + c), c);
            DnmsCand q;
            const int what = dnms_candidate(rule, conf_thres, dnms_load(pred, dtype, at), dnms_load(pred, dtype, at + 1),
                                            dnms_load(pred, dtype, at + 2), dnms_load(pred, dtype, at + 3), obj, v, best, r, &q);
            if (what == 1) cand.push_back(q);
            else if (what == 2) st |= kDnmsNanKey;
        }
        order.resize(cand.size());
        for (size_t i = 0; i < cand.size(); ++i) order[i] = {dnms_order_key(dnms_key_bits(dnms_key(cand[i])), cand[i].row), (int)i};
        std::sort(order.begin(), order.end());
        if ((int)order.size() > max_candidates) st |= kDnmsTruncated, order.resize((size_t)max_candidates);
        const int K = (int)order.size();
        s.resize(K), area.resize(K), state.assign(K, 1), sup.assign(K, -1);
        for (int p = 0; p < K; ++p) s[p] = cand[order[p].second], area[p] = dnms_area(rule, s[p]);
        float *out = rows + (size_t)b * max_det * F;
        int32_t *idx = index + (size_t)b * max_det;
        int kept = 0;
        for (int p = 0; p < K; ++p) {
            if (!state[p]) continue;
            if (kept == max_det) {
                st |= kDnmsMaxDetHit;
                break;
            }
            state[p] = 2, sup[p] = kept++;
            for (int q = p + 1; q < K; ++q) {
                if (state[q] != 1 || !(agnostic || s[q].best == s[p].best)) continue;
                const float o = dnms_iou(rule, s[p].x1, s[p].y1, s[p].x2, s[p].y2, area[p], s[q].x1, s[q].y1, s[q].x2, s[q].y2, area[q]);
                if (o > iou_thres) state[q] = 0, sup[q] = p;
            }
        }
        for (int p = 0; p < K; ++p) {
            if (state[p] != 2) continue;
            float acc[4] = {0, 0, 0, 0}, sum = 0;
            if (rule == kDnmsYoloV3) {
                dnms_merge_first(s[p].obj, s[p].x1, s[p].y1, s[p].x2, s[p].y2, acc, sum);
                for (int q = p + 1; q < K; ++q)
                    if (state[q] == 0 && sup[q] == p) dnms_merge_add(s[q].obj, s[q].x1, s[q].y1, s[q].x2, s[q].y2, acc, sum);
            }
            dnms_write_row(rule, s[p], acc, sum, out + (size_t)sup[p] * F);
            idx[sup[p]] = s[p].row;
        }
        for (int k = kept; k < max_det; ++k) {
            for (int f = 0; f < F; ++f) out[(size_t)k * F + f] = 0.0f;
            idx[k] = -1;
        }
        counts[b] = kept, status[b] = st;
    }
    return 0;
}

const char *hrn_detector_nms_last_error(void) { return g_detector_nms_error.c_str(); }

// ---- COCO keypoint AP / AR on the host (keypoint_eval_math.h: the text the kernels of keypoint_eval.hip compile) ------------------
static thread_local std::string g_keypoint_eval_error;

int hrn_keypoint_eval(int P, const int32_t *dt_start, const int32_t *gt_start, int J, const double *dt_kpts, const double *dt_scores,
                      const double *gt_kpts, const double *gt_area, const double *gt_bbox, const int32_t *gt_iscrowd,
                      const double *sigmas, double *stats, double *precision, double *recall, int32_t *slot_person,
                      double *slot_score, int32_t *dt_match, uint8_t *dt_ignore, int32_t *npig, int32_t *status) {
    using namespace hrn;
    g_keypoint_eval_error.clear();
    if (const char *fault = keypoint_eval_fault(P, dt_start, gt_start, J, dt_kpts, dt_scores, gt_kpts, gt_area, gt_bbox, gt_iscrowd, sigmas,
                                                stats, precision, recall, slot_person, slot_score, dt_match, dt_ignore, npig, status)) {
        g_keypoint_eval_error = fault;
        return 7;
    }
    std::vector<EvalImage> images((size_t)P);
    const size_t S = (size_t)keypoint_eval_images(P, dt_start, gt_start, images.data());
    std::vector<double> vars(J), oks((size_t)kEvalMaxDet * kMaxTracked), dt_area(kEvalMaxDet);
    std::vector<int> k1(kMaxTracked), slot(kEvalMaxDet);
    std::vector<unsigned char> ig((size_t)kEvalAreas * kMaxTracked), order((size_t)kEvalAreas * kMaxTracked), crowd(kMaxTracked),
        taken(kMaxTracked);
    for (int j = 0; j < J; ++j) vars[j] = pose_nms_var(sigmas, j);

    // ---- per image: the slots, the OKS matrix, the 30 matchings ----
    for (int p = 0; p < P; ++p) {
        const EvalImage &im = images[p];
        int st = 0, bad = 0;
        const double *sc = dt_scores + im.dt_first;
        for (int d = 0; d < im.dt_n; ++d) {
            if (sc[d] != sc[d]) st |= 1;
            const int r = pose_nms_rank(sc, im.dt_n, d);
            if (r < im.slots) slot[r] = d;
        }
        for (int g = 0; g < im.gt_n; ++g) {
            const size_t at = (size_t)im.gt_first + g;
            k1[g] = eval_k1(gt_kpts + at * J * 3, J);
            crowd[g] = gt_iscrowd[at] != 0;
            for (int a = 0; a < kEvalAreas; ++a) ig[(size_t)a * kMaxTracked + g] = eval_gt_ig(crowd[g] || k1[g] == 0, gt_area[at], a);
        }
        for (int a = 0; a < kEvalAreas; ++a)
            npig[(size_t)p * kEvalAreas + a] = eval_gt_order(&ig[(size_t)a * kMaxTracked], im.gt_n, &order[(size_t)a * kMaxTracked]);
        for (int s = 0; s < im.slots; ++s) {
            const size_t d = (size_t)im.dt_first + slot[s];
            slot_person[im.slot_first + s] = (int32_t)d, slot_score[im.slot_first + s] = dt_scores[d];
            dt_area[s] = eval_dt_area(dt_kpts + d * J * 3, J);
            for (int g = 0; g < im.gt_n; ++g) {
                const size_t at = (size_t)im.gt_first + g;
                oks[(size_t)s * im.gt_n + g] = eval_oks(dt_kpts + d * J * 3, gt_kpts + at * J * 3, J, k1[g], gt_bbox + at * 4, gt_area[at],
                                                        vars.data(), &bad);
            }
        }
        for (int a = 0; a < kEvalAreas; ++a)
            for (int t = 0; t < kEvalThrs; ++t) {
                const size_t out = (size_t)(a * kEvalThrs + t) * S + im.slot_first;
                eval_match(oks.data(), im.slots, im.gt_n, &order[(size_t)a * kMaxTracked], &ig[(size_t)a * kMaxTracked], crowd.data(),
                           dt_area.data(), a, kEvalIouThrs[t], im.gt_first, taken.data(), dt_match + out, dt_ignore + out);
            }
        status[p] = st | (bad ? 2 : 0);
    }

    // ---- over the set: the order, then per (a, t) the counts from the front and the envelope and look-ups from the end ----
    std::vector<int32_t> set_order(S);
    std::iota(set_order.begin(), set_order.end(), 0);
    std::stable_sort(set_order.begin(), set_order.end(), [&](int32_t x, int32_t y) {
        const double sx = slot_score[x], sy = slot_score[y];
        return (sx == sx && sy != sy) || sx > sy;
    });
    std::vector<int> tps(S);
    for (int a = 0; a < kEvalAreas; ++a) {
        long long total = 0;
        for (int p = 0; p < P; ++p) total += npig[(size_t)p * kEvalAreas + a];
        const int npig_a = (int)total;
        for (int t = 0; t < kEvalThrs; ++t) {
            double *prec = precision + (size_t)(a * kEvalThrs + t) * kEvalRecs;
            if (npig_a == 0) {
                for (int r = 0; r < kEvalRecs; ++r) prec[r] = -1.0;
                recall[a * kEvalThrs + t] = -1.0;
                continue;
            }
            const int32_t *match = dt_match + (size_t)(a * kEvalThrs + t) * S;
            const uint8_t *ignore = dt_ignore + (size_t)(a * kEvalThrs + t) * S;
            int tp = 0, fp = 0;
            for (size_t i = 0; i < S; ++i) {
                const int32_t s = set_order[i];
                if (!ignore[s]) (match[s] >= 0 ? tp : fp) += 1;
                tps[i] = tp;
            }
            recall[a * kEvalThrs + t] = S ? eval_recall(tp, npig_a) : 0.0;
            for (int r = 0; r < kEvalRecs; ++r) prec[r] = 0.0;
            double env = -1.0;
            for (size_t i = S; i-- > 0;) {
                const double pr = eval_precision(tp, fp);
                env = pr > env ? pr : env;
                const int before = i ? tps[i - 1] : 0;
                if (i == 0 || before != tp)
                    for (int r = 0; r < kEvalRecs; ++r)
                        if (eval_owns(tp, before, i == 0, npig_a, r)) prec[r] = env;
                const int32_t s = set_order[i];
                if (!ignore[s]) (match[s] >= 0 ? tp : fp) -= 1;
            }
        }
    }
    for (int k = 0; k < 10; ++k) stats[k] = eval_stat(precision, recall, k);
    return 0;
}

const char *hrn_keypoint_eval_last_error(void) { return g_keypoint_eval_error.c_str(); }

int hrn_keypoint_eval_oks(int n_d, int n_g, int J, const double *dt_kpts, const double *gt_kpts, const double *gt_area,
                          const double *gt_bbox, const double *sigmas, double *oks_out) {
    using namespace hrn;
    if (n_d < 0 || n_g < 0 || n_d > kMaxTracked || n_g > kMaxTracked || J < 1 || J > kAssocMaxJoints || (!sigmas && J != 17)) return 7;
    if (n_d && n_g && (!dt_kpts || !gt_kpts || !gt_area || !gt_bbox || !oks_out)) return 7;
    std::vector<double> vars(J);
    for (int j = 0; j < J; ++j) vars[j] = pose_nms_var(sigmas, j);
    int bad = 0;
    for (int g = 0; g < n_g; ++g) {
        const int k1 = eval_k1(gt_kpts + (size_t)g * J * 3, J);
        for (int d = 0; d < n_d; ++d)
            oks_out[(size_t)d * n_g + g] =
                eval_oks(dt_kpts + (size_t)d * J * 3, gt_kpts + (size_t)g * J * 3, J, k1, gt_bbox + (size_t)g * 4, gt_area[g], vars.data(), &bad);
    }
    return 0;
}

int hrn_keypoint_eval_constants(double *iou_thrs, double *rec_thrs, double *area_ranges) {
    using namespace hrn;
    if (!iou_thrs || !rec_thrs || !area_ranges) return 7;
    for (int t = 0; t < kEvalThrs; ++t) iou_thrs[t] = kEvalIouThrs[t];
    for (int r = 0; r < kEvalRecs; ++r) rec_thrs[r] = kEvalRecThrs[r];
    for (int a = 0; a < kEvalAreas; ++a) area_ranges[2 * a] = kEvalAreaLo[a], area_ranges[2 * a + 1] = kEvalAreaHi[a];
    return 0;
}

// ---- the detector link on the host: letterbox geometry and the detector's boxes back in frame coordinates (letterbox_math.h) ----
static thread_local std::string g_letterbox_error;

int hrn_letterbox_geometry(int rule, const int32_t *frame_hw, int n, int out_h, int out_w, hrn_letterbox *out) {
    using namespace hrn;
    g_letterbox_error.clear();
    if (n < 0 || (n > 0 && (!frame_hw || !out))) {
        g_letterbox_error = "bad frame sizes / output / n";
        return 7;
    }
    for (int i = 0; i < n; ++i) {
        const int code = letterbox_geometry_one(rule, frame_hw[2 * (size_t)i], frame_hw[2 * (size_t)i + 1], out_h, out_w, &out[i], nullptr);
        if (code == LB_OK) continue;
        g_letterbox_error = code == LB_BAD_RULE || code == LB_NOT_SQUARE
                                ? std::string(letterbox_fault_text(code))
                                : "frame " + std::to_string(i) + " (" + std::to_string(frame_hw[2 * (size_t)i]) + " x " +
                                      std::to_string(frame_hw[2 * (size_t)i + 1]) + ") " + letterbox_fault_text(code);
        return 7;
    }
    return 0;
}

const char *hrn_letterbox_last_error(void) { return g_letterbox_error.c_str(); }

int hrn_detections_to_frame(int rule, const float *dets, int det_stride, const int32_t *start, int P, const hrn_letterbox *geometry,
                            const int32_t *frame_hw, int out_h, int out_w, int conf_col, float conf_thres, int class_col,
                            const int32_t *classes, int nclasses, int flags, float *dets_out, int32_t *counts_out, int32_t *status_out) {
    using namespace hrn;
    g_letterbox_error.clear();
    DetFilter q{};
    if (const char *fault = det_fault(rule, dets, det_stride, start, P, geometry, frame_hw, out_h, out_w, conf_col, conf_thres, class_col,
                                      classes, nclasses, flags, dets_out, counts_out, status_out, q)) {
        g_letterbox_error = fault;
        return 7;
    }
    for (int p = 0; p < P; ++p) {
        const DetFrame f = det_frame(rule, geometry[p], frame_hw[2 * (size_t)p], frame_hw[2 * (size_t)p + 1], out_h, out_w, start[p],
                                     start[p + 1] - start[p]);
        counts_out[p] = det_frame_host(dets, f, q, (flags & kDetCompact) != 0, dets_out, status_out);
    }
    return 0;
}

// ---- people between a frame and its rotation, on the host (rotate_math.h: the text rotate_people_kernel compiles) -----------------
static thread_local std::string g_rotate_people_error;

int hrn_rotate_people(int n, int J, const int32_t *frame_hw, int per_person_hw, const int32_t *codes, int per_person_code, const float *pts,
                      const int32_t *boxes, float *pts_out, int32_t *boxes_out) {
    using namespace hrn;
    g_rotate_people_error.clear();
    if (const char *fault = rotate_people_fault(n, J, frame_hw, per_person_hw, codes, per_person_code, pts, boxes, pts_out, boxes_out)) {
        g_rotate_people_error = fault;
        return 7;
    }
    for (int i = 0; i < n; ++i) {
        const int32_t *hw = frame_hw + (per_person_hw ? (size_t)i * 2 : 0);
        const int code = codes[per_person_code ? i : 0];
        if (pts)
            for (int j = 0; j < J; ++j) rotate_joint(code, hw[0], hw[1], pts + ((size_t)i * J + j) * 3, pts_out + ((size_t)i * J + j) * 3);
        if (boxes) rotate_box(code, hw[0], hw[1], boxes + (size_t)i * 4, boxes_out + (size_t)i * 4);
    }
    return 0;
}

const char *hrn_rotate_people_last_error(void) { return g_rotate_people_error.c_str(); }

// ---- joints over time on the host: the One-Euro filter and the motion lookahead (temporal_math.h: the text temporal_kernel compiles) --
static thread_local std::string g_filter_poses_error;

int hrn_filter_poses(int P, const int32_t *cur_start, const int32_t *prev_start, int J, const float *pts, const int32_t *match,
                     const float *prev_state, const int32_t *prev_age, double dt, double min_cutoff, double beta, double d_cutoff,
                     float threshold, double lookahead, float *pts_out, float *pred_out, float *state, int32_t *age) {
    using namespace hrn;
    g_filter_poses_error.clear();
    if (const char *fault = temporal_fault(P, cur_start, prev_start, J, pts, match, prev_state, prev_age, dt, min_cutoff, beta, d_cutoff,
                                           lookahead, pts_out, state, age)) {
        g_filter_poses_error = fault;
        return 7;
    }
    const TemporalParams prm = temporal_params(dt, min_cutoff, beta, d_cutoff, threshold, lookahead);
    for (int p = 0; p < P; ++p) {
        const int prev0 = prev_start[p], m = prev_start[p + 1] - prev0;
        for (size_t i = (size_t)cur_start[p]; i < (size_t)cur_start[p + 1]; ++i) {
            const long long before = match ? temporal_previous(match[i], prev0, m) : -1;
            for (int j = 0; j < J; ++j) {
                const size_t at = i * J + j;
                const float v[3] = {pts[at * 3], pts[at * 3 + 1], pts[at * 3 + 2]};
                const size_t q = before >= 0 ? (size_t)before * J + j : 0;
                const int32_t before_age = before >= 0 ? prev_age[q] : 0;
                const TemporalJoint r = temporal_joint(v, before_age > 0, before_age > 0 ? prev_state + q * 6 : nullptr, before_age, prm);
                pts_out[at * 3] = r.out[0], pts_out[at * 3 + 1] = r.out[1], pts_out[at * 3 + 2] = v[2];
                if (pred_out) pred_out[at * 3] = r.pred[0], pred_out[at * 3 + 1] = r.pred[1], pred_out[at * 3 + 2] = v[2];
                for (int k = 0; k < 6; ++k) state[at * 6 + k] = r.state[k];
                age[at] = r.age;
            }
        }
    }
    return 0;
}

const char *hrn_filter_poses_last_error(void) { return g_filter_poses_error.c_str(); }

// the OKS of all n people of ONE problem against its person g, exactly as both entries compute it (a non-finite value as 0.0),
// for measuring it against the reference's oks_iou; returns 0 or 7
int hrn_pose_nms_oks_row(int n, int J, int flags, const void *kpts, const void *areas, int g, double in_vis_thre, const double *sigmas,
                         double *oks_out) {
    using namespace hrn;
    if (n < 1 || n > kMaxTracked || J < 1 || J > kAssocMaxJoints || (flags & ~kPoseNmsEngine) || g < 0 || g >= n || !kpts || !areas ||
        !oks_out || (!sigmas && J != 17))
        return 7;
    const PoseNmsPeople ppl = pose_nms_people(J, flags, kpts, areas, nullptr, in_vis_thre, __builtin_nan(""));
    std::vector<double> vars(J), gx(J), gy(J);
    for (int j = 0; j < J; ++j) vars[j] = pose_nms_var(sigmas, j), gx[j] = pose_nms_x(ppl, g, j), gy[j] = pose_nms_y(ppl, g, j);
    int bad = 0;
    for (int d = 0; d < n; ++d)
        oks_out[d] = pose_nms_oks(ppl, gx.data(), gy.data(), pose_nms_area(ppl, g), d, pose_nms_area(ppl, d), vars.data(), &bad);
    return 0;
}

}  // extern "C"
