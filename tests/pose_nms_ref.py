"""Pose NMS restated in numpy and plain loops (csrc/pose_nms_math.h's definition; misc/nms/nms.py:75-177 and
datasets/COCO.py:360-372 of the reference), with ``math.exp`` and numpy's own ``sum``: an independent text, so its OKS values may
differ from the library's in the last places (the library's exp is within 1 ulp of libm's) while every decision that is not
knife-edge is the same.  COCO layout throughout: kpts (n, J, 3) float64 (x, y, score); ``engine_to_coco`` widens the other one."""
import math

import numpy as np

COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
MAX_KEEP = 20


def engine_to_coco(pts, boxes, det_scores=None):
    """float32 (y, x, c) + int32 boxes (+ float32 scores) -> (kpts, areas, scores) float64, every value widened exactly"""
    pts = np.asarray(pts, np.float32).astype(np.float64)
    b = np.asarray(boxes, np.int32).astype(np.float64).reshape(-1, 4)
    kpts = np.stack([pts[:, :, 1], pts[:, :, 0], pts[:, :, 2]], 2) if len(pts) else np.zeros((0, pts.shape[1], 3))
    areas = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    scores = np.ones(len(b)) if det_scores is None else np.asarray(det_scores, np.float32).astype(np.float64)
    return np.ascontiguousarray(kpts), areas, scores


def rescore(kpts, scores, thre):
    out = []
    for person, box_score in zip(kpts, scores):
        kpt_score, valid = 0.0, 0
        for j in range(len(person)):
            if person[j][2] > thre:
                kpt_score = kpt_score + float(person[j][2])
                valid += 1
        if valid != 0:
            kpt_score = kpt_score / valid
        out.append(kpt_score * float(box_score))
    return np.asarray(out, np.float64).reshape(-1)


def stable_order(scores):
    """descending, equal scores in index order, NaN last in index order"""
    return sorted(range(len(scores)), key=lambda i: (1, 0.0) if scores[i] != scores[i] else (0, -scores[i]))


def oks(g, d, a_g, a_d, variances, vis):
    terms = []
    denom = (a_g + a_d) / 2 + float(np.spacing(1))
    for j in range(len(g)):
        if vis is not None and not d[j][2] > vis:          # the candidate's mask only
            continue
        dx, dy = float(d[j][0]) - float(g[j][0]), float(d[j][1]) - float(g[j][1])
        e = (dx * dx + dy * dy) / float(variances[j]) / denom / 2
        terms.append(math.exp(-e) if -e < 700 else (math.inf if e == e else math.nan))
    o = float(np.sum(np.asarray(terms, np.float64))) / len(terms) if terms else 0.0
    return o


def pose_nms(kpts, areas, scores, thresh, in_vis_thre=None, rescore_thre=None, soft=False, sigmas=None):
    """one problem; returns dict(keep, num, scores, suppressor, status, gap): ``gap`` is the smallest |OKS - thresh| met (hard) or
    the smallest relative distance between two scores that were ordered against each other (soft) -- how far from a knife edge"""
    kpts, areas = np.asarray(kpts, np.float64), np.asarray(areas, np.float64)
    n = len(areas)
    sg = COCO_SIGMAS if sigmas is None else np.asarray(sigmas, np.float64)
    variances = (sg * 2) * (sg * 2)
    sc = np.asarray(scores, np.float64).copy() if rescore_thre is None else rescore(kpts, scores, rescore_thre)
    status = 1 if any(s != s for s in sc) else 0
    order = stable_order(sc)
    keep, suppressor, gap = [], [-1] * n, math.inf

    def overlap(i, c):
        nonlocal status
        o = oks(kpts[i], kpts[c], float(areas[i]), float(areas[c]), variances, in_vis_thre)
        if not math.isfinite(o):
            status |= 2
            return 0.0
        return o

    def closest(values):
        v = sorted(x for x in values if x == x)
        return min([abs(a - b) / max(abs(a), abs(b), 1e-300) for a, b in zip(v, v[1:]) if a != b], default=math.inf)

    if not soft:
        alive = [True] * n
        for pos, i in enumerate(order):
            if not alive[i]:
                continue
            keep.append(i)
            for c in order[pos + 1:]:
                if alive[c]:
                    o = overlap(i, c)
                    gap = min(gap, abs(o - thresh))
                    if o > thresh:
                        alive[c], suppressor[c] = False, i
    else:
        cur, cs = list(order), [sc[i] for i in order]
        gap = closest(cs)
        while cur and len(keep) < MAX_KEEP:
            i = cur[0]
            rs = []
            for c, s in zip(cur[1:], cs[1:]):
                o = overlap(i, c)
                rs.append(s * math.exp(-(o * o) / thresh))
            gap = min(gap, closest(rs))
            idx = stable_order(rs)
            cur, cs = [cur[1:][k] for k in idx], [rs[k] for k in idx]
            keep.append(i)
        for c in cur:
            suppressor[c] = -2
    return dict(keep=np.asarray(keep + [-1] * (n - len(keep)), np.int32), num=len(keep), scores=sc,
                suppressor=np.asarray(suppressor, np.int32), status=status, gap=gap)


def clustered(seed, n, j, jitter=4.0, groups=None):
    """n people in the engine layout as tests/golden/make_tracking_golden.py builds its NMS cases: jittered copies of
    max(1, n // 3) skeletons (or `groups` of them), confidences jittered too, detection scores uniform in [0.1, 1)"""
    from assoc_cases import people

    rng = np.random.default_rng(seed)
    if n == 0:
        return np.zeros((0, j, 3), np.float32), np.zeros((0, 4), np.int32), np.zeros((0,), np.float32)
    base, _ = people(rng, groups or max(1, n // 3), j)
    pts, boxes = people(rng, n, j, jitter=jitter, base=base[rng.integers(0, len(base), n)])
    pts[:, :, 2] = np.clip(pts[:, :, 2] + rng.normal(0, 0.05, pts.shape[:2]), 0.01, 1).astype(np.float32)
    return np.ascontiguousarray(pts), np.ascontiguousarray(boxes), rng.uniform(0.1, 1.0, n).astype(np.float32)


def random_sigmas(seed, j):
    return np.random.default_rng(seed).uniform(0.025, 0.107, j)


def tie_case():
    """six people twice over (exact ties: duplicates), one NaN score, a pair all of whose joints are masked, and a zero-area
    pair of identical skeletons"""
    pts, boxes, det = clustered(31, 6, 17, jitter=30.0, groups=6)
    pts, boxes, det = np.concatenate([pts, pts]), np.concatenate([boxes, boxes]), np.concatenate([det, det])
    det[7] = np.nan
    pts[2, :, 2] = pts[8, :, 2] = 0.05                                               # below every in_vis_thre used: OKS 0.0 as a candidate
    boxes[4] = boxes[10] = 0                                                # person 4 and its duplicate: zero areas, distance 0
    return np.ascontiguousarray(pts), np.ascontiguousarray(boxes), det
