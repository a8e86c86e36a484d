"""The COCO keypoint evaluation restated in numpy and plain Python from the TEXT of csrc/keypoint_eval_math.h's header (not from
its C++): np.exp and np.sum for the OKS, np.argsort(kind="mergesort") for the two orders, np.cumsum / np.searchsorted for the
curves, loops for the matching and the means.  tests/test_keypoint_eval_host.py holds the host form to it."""
import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0, 1, 101)
AREA_RANGES = ((0.0, 1e10), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
MAX_DET = 20
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
EPS = np.spacing(1)


def descending(scores):
    """descending and stable, NaN last: mergesort of the negated scores (NaN sorts to the end, equal keys keep their order)"""
    return np.argsort(-np.asarray(scores, np.float64), kind="mergesort")


def dt_area(k):
    """(max x - min x) * (max y - min y) over all joints, max / min by `v > m ? v : m` from the first joint on"""
    if np.isfinite(k[:, :2]).all():
        return (k[:, 0].max() - k[:, 0].min()) * (k[:, 1].max() - k[:, 1].min())
    x0 = x1 = k[0, 0]
    y0 = y1 = k[0, 1]
    for x, y in k[1:, :2]:
        x0, x1 = (x if x < x0 else x0), (x if x > x1 else x1)
        y0, y1 = (y if y < y0 else y0), (y if y > y1 else y1)
    return (x1 - x0) * (y1 - y0)


def oks_matrix(dts, gts, area, bbox, sigmas=None):
    """(n_d, n_g) OKS and whether any value was non-finite (counted as 0.0)"""
    var = (np.asarray(COCO_SIGMAS if sigmas is None else sigmas, np.float64) * 2) ** 2
    out, bad = np.zeros((len(dts), len(gts))), False
    if len(dts) == 0:
        return out, bad
    xd, yd = dts[:, :, 0], dts[:, :, 1]
    with np.errstate(all="ignore"):
        for g in range(len(gts)):
            xg, yg, vg = gts[g, :, 0], gts[g, :, 1], gts[g, :, 2]
            k1 = int(np.count_nonzero(vg > 0))
            if k1 > 0:
                dx, dy = xd - xg, yd - yg
            else:
                x0, x1 = bbox[g, 0] - bbox[g, 2], bbox[g, 0] + 2 * bbox[g, 2]
                y0, y1 = bbox[g, 1] - bbox[g, 3], bbox[g, 1] + 2 * bbox[g, 3]
                pos = lambda v: np.where(v > 0, v, 0.0)   # noqa: E731
                dx, dy = pos(x0 - xd) + pos(xd - x1), pos(y0 - yd) + pos(yd - y1)
            e = (dx * dx + dy * dy) / var / (area[g] + EPS) / 2
            if k1 > 0:
                e = e[:, vg > 0]
            for d in range(len(dts)):
                o = np.sum(np.exp(-np.ascontiguousarray(e[d]))) / e.shape[1]
                if not np.isfinite(o):
                    o, bad = 0.0, True
                out[d, g] = o
    return out, bad


def keypoint_eval(dt_kpts, dt_scores, dt_image, gt_kpts, gt_area, gt_bbox, gt_iscrowd, gt_image, sigmas=None):
    dt_image, gt_image = np.asarray(dt_image, np.int64).reshape(-1), np.asarray(gt_image, np.int64).reshape(-1)
    joints = np.shape(dt_kpts)[1] if len(dt_image) else (np.shape(gt_kpts)[1] if len(gt_image) else 17)
    dt_kpts, dt_scores = np.asarray(dt_kpts, np.float64).reshape(-1, joints, 3), np.asarray(dt_scores, np.float64).reshape(-1)
    gt_kpts, gt_area = np.asarray(gt_kpts, np.float64).reshape(-1, joints, 3), np.asarray(gt_area, np.float64).reshape(-1)
    gt_bbox, gt_iscrowd = np.asarray(gt_bbox, np.float64).reshape(-1, 4), np.asarray(gt_iscrowd).reshape(-1)
    images = sorted(set(dt_image.tolist()) | set(gt_image.tolist()))
    T = len(IOU_THRS)
    slot_person, slot_score, status, npig, oks_all = [], [], [], [], []
    match = [[[] for _ in range(T)] for _ in AREA_RANGES]
    ignore = [[[] for _ in range(T)] for _ in AREA_RANGES]
    for image in images:
        di, gi = np.flatnonzero(dt_image == image), np.flatnonzero(gt_image == image)
        st = 1 if np.isnan(dt_scores[di]).any() else 0
        slots = di[descending(dt_scores[di])[:MAX_DET]]
        slot_person += slots.tolist()
        slot_score += dt_scores[slots].tolist()
        oks, bad = oks_matrix(dt_kpts[slots], gt_kpts[gi], gt_area[gi], gt_bbox[gi], sigmas)
        status.append(st | (2 if bad else 0))
        oks_all.append(oks)
        rows = oks.tolist()
        areas_d = [float(dt_area(dt_kpts[s])) for s in slots]
        crowd = [bool(c) for c in gt_iscrowd[gi]]
        k1 = [int(np.count_nonzero(gt_kpts[g, :, 2] > 0)) for g in gi]
        per_range = []
        for a, (lo, hi) in enumerate(AREA_RANGES):
            ig = [bool(crowd[q] or k1[q] == 0 or gt_area[g] < lo or gt_area[g] > hi) for q, g in enumerate(gi)]
            order = [q for q in range(len(gi)) if not ig[q]] + [q for q in range(len(gi)) if ig[q]]
            per_range.append(sum(1 for q in ig if not q))
            for t, thr in enumerate(IOU_THRS.tolist()):
                taken = [False] * len(gi)
                for s in range(len(slots)):
                    best, m = min(thr, 1 - 1e-10), -1
                    for q in order:
                        if taken[q] and not crowd[q]:
                            continue
                        if m >= 0 and not ig[m] and ig[q]:
                            break
                        if rows[s][q] < best:
                            continue
                        best, m = rows[s][q], q
                    if m >= 0:
                        taken[m] = True
                        match[a][t].append(int(gi[m]))
                        ignore[a][t].append(1 if ig[m] else 0)
                    else:
                        match[a][t].append(-1)
                        ignore[a][t].append(1 if (areas_d[s] < lo or areas_d[s] > hi) else 0)
        npig.append(per_range)
    S = len(slot_person)
    dt_match = np.array(match, np.int32).reshape(len(AREA_RANGES), T, S)
    dt_ignore = np.array(ignore, np.uint8).reshape(len(AREA_RANGES), T, S)
    npig = np.array(npig, np.int32).reshape(len(images), len(AREA_RANGES))
    precision, recall = -np.ones((len(AREA_RANGES), T, len(REC_THRS))), -np.ones((len(AREA_RANGES), T))
    order = descending(slot_score)
    for a in range(len(AREA_RANGES)):
        total = int(npig[:, a].sum())
        if total == 0:
            continue
        for t in range(T):
            m, ig = dt_match[a, t, order] >= 0, dt_ignore[a, t, order] != 0
            tp = np.cumsum(np.logical_and(m, ~ig)).astype(np.float64)
            fp = np.cumsum(np.logical_and(~m, ~ig)).astype(np.float64)
            rc = tp / total
            pr = tp / (fp + tp + EPS)
            recall[a, t] = rc[-1] if S else 0.0
            pr = np.maximum.accumulate(pr[::-1])[::-1]
            at = np.searchsorted(rc, REC_THRS, side="left")
            precision[a, t] = [pr[i] if i < S else 0.0 for i in at]

    def mean(values):
        total, count = 0.0, 0
        for v in np.asarray(values).reshape(-1).tolist():
            if v > -1:
                total, count = total + v, count + 1
        return total / count if count else -1.0

    stats = [mean(precision[0]), mean(precision[0, 0]), mean(precision[0, 5]), mean(precision[1]), mean(precision[2]),
             mean(recall[0]), mean(recall[0, 0]), mean(recall[0, 5]), mean(recall[1]), mean(recall[2])]
    return dict(stats=np.array(stats), precision=precision, recall=recall, slot_person=np.array(slot_person, np.int32),
                slot_score=np.array(slot_score, np.float64), dt_match=dt_match, dt_ignore=dt_ignore, npig=npig,
                status=np.array(status, np.int32), images=np.array(images, np.int64), oks=oks_all)
