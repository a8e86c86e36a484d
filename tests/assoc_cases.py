"""Inputs shared by tests/test_assoc_host.py and tests/test_assoc_gpu.py: synthetic people, the margins of a case computed from
the EXISTING functions (postproc.compute_similarity_matrices / the blend of find_person_id_associations), the demo loop
(scripts/live-demo.py:114-130) restated on find_person_id_associations, and the six-step sequence the tracker tests follow."""
import itertools

import numpy as np

from conftest import load_pkg

PARAMS = [(0.2, 0.4, 0.1), (0.5, 0.5, 0.0), (0.8, 0.3, 0.5)]      # (pose_alpha, similarity_threshold, smoothing_alpha)
DEMO = (0.2, 0.4, 0.1)                                            # live-demo.py:122


def people(rng, n, j, jitter=0.0, base=None, frame=(480, 640)):
    """n synthetic skeletons (n, j, 3) float32 (y, x, confidence) with their int32 boxes (x1, y1, x2, y2); with `base`, jittered
    copies of those skeletons"""
    if base is None:
        cy, cx = rng.uniform(80, frame[0] - 80, n), rng.uniform(80, frame[1] - 80, n)
        sz = rng.uniform(40, 160, n)
        pts = np.empty((n, j, 3), np.float32)
        pts[:, :, 0] = cy[:, None] + rng.normal(0, 1, (n, j)) * sz[:, None] * 0.4
        pts[:, :, 1] = cx[:, None] + rng.normal(0, 1, (n, j)) * sz[:, None] * 0.25
        pts[:, :, 2] = rng.uniform(0.05, 1.0, (n, j))
    else:
        pts = base.copy()
        pts[:, :, :2] += rng.normal(0, jitter, pts[:, :, :2].shape).astype(np.float32)
    if n == 0:
        return pts, np.zeros((0, 4), np.int32)
    boxes = np.stack([pts[:, :, 1].min(1) - 5, pts[:, :, 0].min(1) - 5, pts[:, :, 1].max(1) + 5, pts[:, :, 0].max(1) + 5], 1)
    return pts, np.round(boxes).astype(np.int32)


def make_case(seed, n, m, j, jitter=3.0):
    """m previous people; the n current ones are jittered copies of some of them plus strangers, shuffled; previous ids are a
    random draw from 0..39 (0..2m-1 for crowds) and next_id lies above them"""
    rng = np.random.default_rng(seed)
    prev_pts, prev_boxes = people(rng, m, j)
    common = min(n, m)
    cur_pts, cur_boxes = people(rng, common, j, jitter=jitter, base=prev_pts[rng.permutation(m)[:common]])
    if n > common:
        extra_pts, extra_boxes = people(rng, n - common, j)
        cur_pts, cur_boxes = np.concatenate([cur_pts, extra_pts]), np.concatenate([cur_boxes, extra_boxes])
    order = rng.permutation(n)
    prev_ids = rng.permutation(max(40, 2 * m))[:m].astype(np.int32)
    return dict(boxes=np.ascontiguousarray(cur_boxes[order]), pts=np.ascontiguousarray(cur_pts[order]), prev_boxes=prev_boxes,
                prev_pts=prev_pts, prev_ids=prev_ids, next_id=int(prev_ids.max()) + 1 if m else 0)


def margins(case, pose_alpha, threshold, brute_limit=6):
    """(distance of the nearest blended similarity from the threshold, gap between the best and the second-best complete
    assignment in total cost -- inf where there is no second one or a side exceeds `brute_limit`), from the existing functions"""
    pp = load_pkg("postproc")
    n, m = len(case["boxes"]), len(case["prev_boxes"])
    if n == 0 or m == 0:
        return np.inf, np.inf
    sim_box, sim_pose = pp.compute_similarity_matrices(case["boxes"], case["prev_boxes"], case["pts"], case["prev_pts"])
    sim = sim_pose * pose_alpha + sim_box * (1 - pose_alpha)
    near = float(np.abs(sim.astype(np.float64) - threshold).min())
    if max(n, m) > brute_limit:
        return near, np.inf
    cost = np.asarray((1 - sim).tolist())
    if n > m:
        cost = cost.T
    rows = np.arange(cost.shape[0])
    totals = sorted(float(cost[rows, list(cols)].sum()) for cols in itertools.permutations(range(cost.shape[1]), cost.shape[0]))
    return near, (totals[1] - totals[0] if len(totals) > 1 else np.inf)


def demo_loop(frames, params=DEMO):
    """scripts/live-demo.py:114-130 over (boxes, pts) frames, with postproc.find_person_id_associations: per frame
    (boxes, pts, ids, next_id)"""
    pp = load_pkg("postproc")
    prev_boxes = prev_pts = prev_ids = None
    next_id, out = 0, []
    for boxes, pts in frames:
        boxes, pts = boxes.copy(), pts.copy()
        if len(pts) > 0:
            if prev_pts is None and prev_ids is None:
                ids = np.arange(next_id, len(pts) + next_id, dtype=np.int32)
                next_id = len(pts) + 1
            else:
                boxes, pts, ids = pp.find_person_id_associations(boxes, pts, prev_boxes, prev_pts, prev_ids, next_person_id=next_id,
                                                                 pose_alpha=params[0], similarity_threshold=params[1],
                                                                 smoothing_alpha=params[2])
                next_id = max(next_id, int(np.max(ids)) + 1)
        else:
            ids = np.array((), dtype=np.int32)
        prev_boxes, prev_pts, prev_ids = boxes.copy(), pts.copy(), ids
        out.append((boxes, pts, ids, next_id))
    return out


def sequence(j=17, seed=5):
    """six frames: three people; the same, moved a little; one has left; nobody; two are back and one enters; the same, moved"""
    rng = np.random.default_rng(seed)
    first, _ = people(rng, 3, j)
    second, _ = people(rng, 3, j, jitter=2.0, base=first)
    third, _ = people(rng, 2, j, jitter=2.0, base=second[[2, 0]])
    stranger, _ = people(rng, 1, j)
    fifth = np.concatenate([people(rng, 2, j, jitter=2.0, base=third)[0], stranger])[[1, 2, 0]]
    sixth, _ = people(rng, 3, j, jitter=2.0, base=fifth)
    frames = []
    for pts in (first, second, third, np.zeros((0, j, 3), np.float32), fifth, sixth):
        frames.append((people(rng, len(pts), j, base=pts)[1], np.ascontiguousarray(pts)))
    return frames
