"""Detector NMS restated in numpy float32 from the text of include/hrnet_mi355.h (hrn_detector_nms), plus the float64 evaluations
and the case builders the host and GPU tests share.

Every float operation below is an ELEMENTWISE float32 numpy operation (add, subtract, multiply, divide, compare, where): IEEE
fixes their results, so the library's host form must agree bit for bit.  The sweep and the merge are explicit loops in the
stated order; nothing is summed by a numpy reduction.
"""
import numpy as np

F32 = np.float32
QNAN = 0x7FC00000
RULES = ("yolov3", "yolov5")


def _max(a, b):
    """the header's max: a > b ? a : b (a NaN operand gives b)"""
    return np.where(a > b, a, b).astype(F32)


def _min(a, b):
    return np.where(a < b, a, b).astype(F32)


def _iou_row(rule, box_a, area_a, boxes_b, area_b):
    """IoU of the kept box a against the boxes b, float32, in the header's operation order"""
    dw = _min(box_a[2], boxes_b[:, 2]) - _max(box_a[0], boxes_b[:, 0])
    dh = _min(box_a[3], boxes_b[:, 3]) - _max(box_a[1], boxes_b[:, 1])
    if rule == "yolov3":
        inter = _max(dw + F32(1), F32(0)) * _max(dh + F32(1), F32(0))
        return inter / (area_a + area_b - inter + F32(1e-16))
    inter = _max(dw, F32(0)) * _max(dh, F32(0))
    return inter / (area_a + area_b - inter)


def candidates(image, rule, conf_thres):
    """one image (N, 5 + C) float32: (rows of the candidates in row order, boxes (n, 4), obj, cls_conf, best, key, NaN-key flag)"""
    t = F32(conf_thres)
    obj, cls = image[:, 4], image[:, 5:]
    conf, best = cls[:, 0].copy(), np.zeros(len(image), np.int64)
    for c in range(1, cls.shape[1]):            # the FIRST maximum: a later class wins only when it is greater
        upd = cls[:, c] > conf
        best[upd], conf[upd] = c, cls[upd, c]
    key = obj * conf
    cand = (obj > t) & (key > t) if rule == "yolov5" else obj >= t
    nan = cand & np.isnan(key)
    rows = np.flatnonzero(cand & ~nan)
    x = image[rows]
    hw, hh = x[:, 2] / F32(2), x[:, 3] / F32(2)
    boxes = np.stack([x[:, 0] - hw, x[:, 1] - hh, x[:, 0] + hw, x[:, 1] + hh], 1).astype(F32).reshape(-1, 4)
    return rows, boxes, obj[rows], conf[rows], best[rows], key[rows], bool(nan.any())


def order_of(key):
    """descending key, equal keys (-0 == +0) in row order: Python's sort is stable"""
    return sorted(range(len(key)), key=lambda i: -float(key[i]))


def detector_nms_ref(pred, rule, conf_thres, iou_thres, max_det=300, max_candidates=4096, agnostic=False, details=None):
    """(rows, counts, index, status) as postproc.detector_nms returns them.  ``details``: a list that receives, per image, a dict
    with the kept positions, the merge sets and the ordered candidates (for the float64 checks)."""
    pred = np.asarray(pred)
    p = pred.astype(F32)                          # float16 widens exactly
    B, width = p.shape[0], 7 if rule == "yolov3" else 6
    rows = np.zeros((B, max_det, width), F32)
    index = np.full((B, max_det), -1, np.int32)
    counts, status = np.zeros(B, np.int32), np.zeros(B, np.int32)
    thr = F32(iou_thres)
    with np.errstate(all="ignore"):
        for b in range(B):
            r, boxes, obj, conf, best, key, nan = candidates(p[b], rule, conf_thres)
            st = 4 if nan else 0
            order = order_of(key)
            if len(order) > max_candidates:
                st |= 1
                order = order[:max_candidates]
            order = np.asarray(order, np.int64)
            r, boxes, obj, conf, best, key = r[order], boxes[order], obj[order], conf[order], best[order], key[order]
            K = len(r)
            if rule == "yolov3":
                area = (boxes[:, 2] - boxes[:, 0] + F32(1)) * (boxes[:, 3] - boxes[:, 1] + F32(1))
            else:
                area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
            alive, sup, kept = np.ones(K, bool), np.full(K, -1, np.int64), []
            for pos in range(K):                  # the greedy sweep
                if not alive[pos]:
                    continue
                if len(kept) == max_det:
                    st |= 2
                    break
                kept.append(pos)
                alive[pos] = False                # the keeper always leaves the list
                q = np.flatnonzero(alive[pos + 1:]) + pos + 1
                if not agnostic:
                    q = q[best[q] == best[pos]]
                iou = _iou_row(rule, boxes[pos], area[pos], boxes[q], area[q])
                hit = q[iou > thr]                # a NaN never suppresses
                alive[hit], sup[hit] = False, pos
            sets = []
            for slot, pos in enumerate(kept):
                members = [pos] + [int(q) for q in np.flatnonzero(sup == pos)]
                sets.append(members)
                if rule == "yolov3":              # the merge: ascending position, product and sum rounded separately
                    acc, total = obj[pos] * boxes[pos], obj[pos]
                    for q in members[1:]:
                        acc, total = acc + obj[q] * boxes[q], total + obj[q]
                    rows[b, slot] = np.concatenate([acc / total, [obj[pos], conf[pos], F32(best[pos])]])
                else:
                    rows[b, slot] = np.concatenate([boxes[pos], [key[pos], F32(best[pos])]])
                index[b, slot] = r[pos]
            counts[b], status[b] = len(kept), st
            if details is not None:
                details.append(dict(kept=kept, sets=sets, rows=r, boxes=boxes, obj=obj, best=best, key=key))
    rows.view(np.uint32)[np.isnan(rows)] = QNAN
    return rows, counts, index, status


def greedy_f64(boxes, best, iou_thres, max_det, agnostic, pixel=False):
    """plain greedy NMS in float64 over candidates already in order: (kept positions, smallest |IoU - threshold| met)"""
    b = boxes.astype(np.float64)
    one = 1.0 if pixel else 0.0
    area = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    alive, kept, margin = np.ones(len(b), bool), [], np.inf
    for pos in range(len(b)):
        if not alive[pos]:
            continue
        if len(kept) == max_det:
            break
        kept.append(pos)
        alive[pos] = False
        q = np.flatnonzero(alive[pos + 1:]) + pos + 1
        if not agnostic:
            q = q[best[q] == best[pos]]
        if len(q) == 0:
            continue
        iw = np.maximum(np.minimum(b[pos, 2], b[q, 2]) - np.maximum(b[pos, 0], b[q, 0]) + one, 0)
        ih = np.maximum(np.minimum(b[pos, 3], b[q, 3]) - np.maximum(b[pos, 1], b[q, 1]) + one, 0)
        iou = iw * ih / (area[pos] + area[q] - iw * ih + (1e-16 if pixel else 0.0))
        margin = min(margin, float(np.abs(iou - float(iou_thres)).min()))
        alive[q[iou > float(iou_thres)]] = False
    return kept, margin


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def random_pred(rng, B, N, C, passing=0.3, conf_thres=0.25):
    """a head output whose passing rows cluster: each cluster has a box and a favourite class; its members are that box moved and
    resized by a few pixels.  Coordinates and sizes lie on a 1/64 grid below 1024, so x1 .. y2 and the intersections are exact in
    float32 and a float32 IoU is within a few 2^-24 of its float64 value (the float64 check's margin of 1e-6 rests on that)."""
    pred = np.zeros((B, N, 5 + C), F32)
    for b in range(B):
        n_pass = int(round(N * passing))
        clusters = max(1, int(round(n_pass / rng.uniform(2.0, 4.0))))
        centre = rng.uniform(60, 580, (clusters, 2))
        size = rng.uniform(30, 160, (clusters, 2))
        fav = rng.integers(0, C, clusters)
        k = rng.integers(0, clusters, N)
        grid = lambda v: np.round(v * 64) / 64    # noqa: E731
        pred[b, :, 0:2] = grid(centre[k] + rng.normal(0, 1, (N, 2)) * size[k] * 0.12)
        pred[b, :, 2:4] = grid(size[k] * rng.uniform(0.8, 1.25, (N, 2)))
        passes = rng.permutation(N) < n_pass
        pred[b, :, 4] = np.where(passes, rng.uniform(conf_thres + 0.3, 1.0, N), rng.uniform(0.0, conf_thres * 0.9, N))
        cls = rng.uniform(0.0, 0.3, (N, C))
        own = np.where(rng.uniform(size=N) < 0.8, fav[k], rng.integers(0, C, N))
        cls[np.arange(N), own] = rng.uniform(0.9, 1.0, N)
        pred[b, :, 5:] = cls
    return pred


def random_cases(seed, count=300):
    """the `count` random cases of one rule: (pred, conf_thres, iou_thres, agnostic)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        B, N, C = int(rng.integers(1, 4)), int(rng.integers(0, 601)), int(rng.choice([1, 2, 80]))
        out.append((random_pred(rng, B, N, C), 0.25, float(rng.choice([0.45, 0.5, 0.6])), bool(i & 1)))
    return out


def _rows(rows, C):
    """rows given as (cx, cy, w, h, obj, {class: score}) to an (1, n, 5 + C) array"""
    out = np.zeros((1, len(rows), 5 + C), F32)
    for i, (cx, cy, w, h, obj, cls) in enumerate(rows):
        out[0, i, :5] = cx, cy, w, h, obj
        for c, v in cls.items():
            out[0, i, 5 + c] = v
    return out


def designed_cases():
    """name -> (pred, rule, conf_thres, iou_thres, max_det, max_candidates, agnostic): the cases the issue names, for both rules
    where the rule matters.  What each one must give is asserted in test_detector_nms_host.py; the GPU test only compares."""
    nan, inf = float("nan"), float("inf")
    cases = {}
    for rule in RULES:
        # equal keys: four identical-score boxes far apart, and two overlapping ones with equal keys -- the lower row wins
        eq = [(100 + 200 * (i % 3), 100 + 200 * (i // 3), 40, 40, 0.5, {0: 0.5}) for i in range(4)]
        eq += [(400, 400, 40, 40, 0.5, {0: 0.5}), (402, 400, 40, 40, 0.25, {0: 1.0}), (398, 400, 40, 40, 1.0, {0: 0.25})]
        cases["equal_keys_" + rule] = (_rows(eq, 2), rule, 0.1, 0.5, 300, 4096, False)
        # obj exactly at conf_thres: kept under v3 (>=), dropped under v5 (>)
        cases["obj_at_threshold_" + rule] = (_rows([(50, 50, 20, 20, 0.25, {0: 1.0}), (150, 50, 20, 20, 0.5, {1: 1.0})], 2), rule, 0.25,
                                             0.5, 300, 4096, False)
        # NaN, inf and -0.0 in boxes, obj and classes
        odd = [(nan, 50, 20, 20, 0.9, {0: 0.9}), (50, 50, inf, 20, 0.9, {0: 0.8}), (50, 50, 20, 20, nan, {0: 0.9}),
               (60, 50, 20, 20, 0.9, {0: nan, 1: 0.9}), (70, 50, 20, 20, 0.9, {0: 0.1, 1: nan}), (-0.0, -0.0, 20, 20, 0.9, {0: 0.7}),
               (80, 50, 20, 20, inf, {0: 0.9}), (80, 50, 20, 20, inf, {0: 0.0, 1: -0.0}), (90, 50, 20, 20, 0.9, {0: inf}),
               (90, 50, 20, 20, 0.9, {0: -0.0, 1: 0.0}), (-inf, 50, 20, 20, 0.9, {1: 0.6}), (50, 50, -20, -20, 0.9, {0: 0.5}),
               (50, 50, 20, 20, -0.0, {0: 0.5}), (52, 50, 20, 20, 0.9, {0: 0.95})]
        cases["nonfinite_" + rule] = (_rows(odd, 2), rule, 0.25, 0.5, 300, 4096, False)
        cases["nonfinite_negative_threshold_" + rule] = (_rows(odd, 2), rule, -1.0, 0.5, 300, 4096, True)
        # zero-area boxes: identical points, a point inside a box, a line
        zero = [(50, 50, 0, 0, 0.9, {0: 0.9}), (50, 50, 0, 0, 0.8, {0: 0.9}), (50, 50, 20, 20, 0.7, {0: 0.9}), (50, 50, 20, 0, 0.6, {0: 0.9}),
                (50, 50, 20, 20, 0.5, {0: 0.9})]
        cases["zero_area_" + rule] = (_rows(zero, 1), rule, 0.25, 0.5, 300, 4096, False)
        # max_candidates below the number that qualify, ties at the cut: keys 0.5 x 6 around it; the lowest rows take part
        cut = [(40 + 60 * (i % 10), 40 + 60 * (i // 10), 30, 30, 0.5 if 10 <= i < 16 else (0.9 if i < 10 else 0.3), {0: 1.0}) for i in range(24)]
        cut = [cut[i] for i in (16, 10, 0, 17, 11, 1, 18, 12, 2, 19, 13, 3, 20, 14, 4, 21, 15, 5, 22, 6, 23, 7, 8, 9)]
        cases["cut_ties_" + rule] = (_rows(cut, 1), rule, 0.1, 0.5, 13, 13, False)
        # max_det reached with a survivor left, and reached exactly
        far = [(40 + 60 * i, 40, 30, 30, 0.9 - 0.01 * i, {0: 1.0}) for i in range(6)]
        cases["max_det_survivors_" + rule] = (_rows(far, 1), rule, 0.1, 0.5, 4, 4096, False)
        cases["max_det_exact_" + rule] = (_rows(far[:4] + [(40, 40, 30, 30, 0.5, {0: 1.0})], 1), rule, 0.1, 0.5, 4, 4096, False)
        # classes: overlapping boxes of two classes, with and without agnostic
        two = [(100, 100, 50, 50, 0.9, {0: 0.9}), (102, 100, 50, 50, 0.8, {1: 0.9}), (101, 101, 50, 50, 0.7, {0: 0.9})]
        cases["two_classes_" + rule] = (_rows(two, 2), rule, 0.25, 0.5, 300, 4096, False)
        cases["two_classes_agnostic_" + rule] = (_rows(two, 2), rule, 0.25, 0.5, 300, 4096, True)
        cases["no_rows_" + rule] = (np.zeros((2, 0, 7), F32), rule, 0.25, 0.5, 300, 4096, False)
        cases["no_images_" + rule] = (np.zeros((0, 5, 7), F32), rule, 0.25, 0.5, 300, 4096, False)
    # an IoU that equals iou_thres exactly, from integer boxes: it must not suppress.
    # yolov5: boxes (0,0)-(20,10) and (10,0)-(30,10): inter 100, union 300 -> 1/3; with (0,0)-(30,10) against (0,0)-(15,10): 150/300 = 0.5
    exact5 = [(15, 5, 30, 10, 0.9, {0: 1.0}), (7.5, 5, 15, 10, 0.8, {0: 1.0}), (215, 5, 30, 10, 0.7, {0: 1.0}), (208.5, 5, 17, 10, 0.6, {0: 1.0})]
    cases["iou_at_threshold_yolov5"] = (_rows(exact5, 1), "yolov5", 0.25, 0.5, 300, 4096, False)
    # yolov3 (pixel convention): (0,0)-(31,9) has area 32 x 10 = 320, (0,0)-(15,9) has 160 = the intersection: 160 / (320 + 160 - 160 +
    # 1e-16f) = 0.5 in float32; the second pair overlaps by one column more on the smaller box's side: above the threshold
    exact3 = [(15.5, 4.5, 31, 9, 0.9, {0: 1.0}), (7.5, 4.5, 15, 9, 0.8, {0: 1.0}), (215.5, 4.5, 31, 9, 0.7, {0: 1.0}),
              (208.5, 4.5, 17, 9, 0.6, {0: 1.0})]
    cases["iou_at_threshold_yolov3"] = (_rows(exact3, 1), "yolov3", 0.25, 0.5, 300, 4096, False)
    return cases
