"""Evaluation sets for the keypoint AP / AR tests (host and GPU): designed sets with closed-form answers and random sets.  A set is
the dict of `postproc.keypoint_eval`'s arguments."""
import numpy as np

EPS = float(np.spacing(1))
ONE = 1.0 / (1.0 + EPS)            # tp / (fp + tp + spacing(1)) with tp = 1, fp = 0
UNIFORM = np.full(17, 0.5)         # sigmas with (2 sigma)^2 = 1


def skeleton(cx, cy, size, joints=17, v=2.0):
    """a (J, 3) person whose joints span exactly the size x size square centred at (cx, cy): its detection area is size^2"""
    u = (np.arange(joints) * 7 % joints) / max(joints - 1, 1)
    w = (np.arange(joints) * 3 % joints) / max(joints - 1, 1)
    return np.stack([cx + size * (u - 0.5), cy + size * (w - 0.5), np.full(joints, v)], axis=1)


def make_set(dts, gts, sigmas=None, joints=17):
    """dts: (image, score, (J, 3)); gts: (image, (J, 3), area, iscrowd) or (image, (J, 3), area, iscrowd, bbox)"""
    out = dict(dt_kpts=np.array([d[2] for d in dts], np.float64).reshape(-1, joints, 3), dt_scores=np.array([d[1] for d in dts], np.float64),
               dt_image=np.array([d[0] for d in dts], np.int64), gt_kpts=np.array([g[1] for g in gts], np.float64).reshape(-1, joints, 3),
               gt_area=np.array([g[2] for g in gts], np.float64), gt_iscrowd=np.array([g[3] for g in gts], np.int32),
               gt_image=np.array([g[0] for g in gts], np.int64), sigmas=sigmas)
    boxes = []
    for g in gts:
        k = np.asarray(g[1], np.float64)
        boxes.append(g[4] if len(g) > 4 else (k[:, 0].min(), k[:, 1].min(), k[:, 0].max() - k[:, 0].min(), k[:, 1].max() - k[:, 1].min()))
    out["gt_bbox"] = np.array(boxes, np.float64).reshape(-1, 4)
    return out


def shifted(k, dx, dy=0.0):
    k = np.array(k, np.float64)
    k[:, 0] += dx
    k[:, 1] += dy
    return k


def designed():
    """name -> set"""
    cases = {}
    small, medium, large = skeleton(100, 100, 20), skeleton(400, 100, 60), skeleton(300, 500, 150)
    three = [(1, small, 500.0, 0), (1, medium, 4000.0, 0), (2, large, 20000.0, 0)]
    cases["exact"] = make_set([(1, .9, small), (1, .8, medium), (2, .7, large)], three)
    cases["no_medium"] = make_set([(1, .9, small), (2, .7, large)], [three[0], three[2]])
    a, b = skeleton(100, 100, 100), skeleton(600, 100, 100)
    cases["hit_miss_hit"] = make_set([(1, .9, a), (1, .8, shifted(a, 5000, 5000)), (1, .7, b)], [(1, a, 10000.0, 0), (1, b, 10000.0, 0)])
    cases["shift72"] = make_set([(1, .9, shifted(a, 72))], [(1, a, 10000.0, 0)], UNIFORM)
    cases["shift80"] = make_set([(1, .9, shifted(a, 80))], [(1, a, 10000.0, 0)], UNIFORM)
    cases["crowd_twice"] = make_set([(1, .9, a), (1, .8, shifted(a, 1)), (1, .7, b)], [(1, a, 10000.0, 1), (1, b, 10000.0, 0)])
    # the detection sits on the crowd (OKS 1) and 66 px from the counted person (OKS exp(-4356 / 20000) = 0.804)
    cases["counted_first"] = make_set([(1, .9, shifted(a, 66))], [(1, a, 10000.0, 0), (1, shifted(a, 66), 10000.0, 1)], UNIFORM)
    cases["stray_large"] = make_set([(1, .9, medium), (1, .8, skeleton(3000, 3000, 200))], [(1, medium, 4000.0, 0)])
    empty = skeleton(125, 180, 40, v=0.0)
    cases["empty_person"] = make_set([(1, .9, skeleton(125, 140, 100)), (1, .8, skeleton(400, 140, 100)), (1, .7, b)],
                                     [(1, empty, 4000.0, 0, (100.0, 100.0, 50.0, 80.0)), (1, b, 10000.0, 0)])
    cases["tie_across_images"] = make_set([(7, .5, a), (3, .5, shifted(a, 5000))], [(3, a, 10000.0, 0), (7, a, 10000.0, 0)])
    cases["twenty_five"] = make_set([(1, 0.01 * (k * 7 % 25), shifted(a, 3.0 * k)) for k in range(25)], [(1, a, 10000.0, 0)])
    nan_xy = np.array(a)
    nan_xy[3, 0] = np.nan
    cases["nan_zero"] = make_set([(1, np.nan, a), (1, .8, nan_xy), (1, .7, b), (1, .6, shifted(b, 1))],
                                 [(1, a, 10000.0, 0), (1, b, 0.0, 0)])
    return cases


def random_set(seed, joints=17, max_images=40, max_dt=25, max_gt=12, counts=None):
    """1 .. max_images images with 0 .. max_dt detections and 0 .. max_gt people each: detections are jittered copies of people
    plus strays, crowds and people without a visible joint are mixed in, scores partly quantised so that ties occur.  `counts`: the
    (detections, people) of each image instead of random numbers of them"""
    rng = np.random.default_rng(seed)
    dts, gts = [], []
    for at, image in enumerate(rng.permutation(rng.integers(1, max_images + 1) if counts is None else len(counts)) + 100):
        people = []
        for _ in range(rng.integers(0, max_gt + 1) if counts is None else counts[at][1]):
            size = float(np.exp(rng.uniform(np.log(10.0), np.log(300.0))))
            cx, cy = rng.uniform(0, 640), rng.uniform(0, 480)
            k = np.stack([cx + size * (rng.random(joints) - .5), cy + size * (rng.random(joints) - .5),
                          rng.integers(0, 3, joints).astype(np.float64)], axis=1)
            if rng.random() < .08 and not any((p[0][:, 2] == 0).all() for p in people):
                k[:, 2] = 0.0   # (one such person per image at most: a detection inside two doubled boxes has OKS 1.0 twice, a tie)
            area = size * size * rng.uniform(.4, .9)
            people.append((k, size))
            gts.append((int(image), k, area, int(rng.random() < .08), (cx - size / 2, cy - size / 2, size, size)))
        for _ in range(rng.integers(0, max_dt + 1) if counts is None else counts[at][0]):
            if people and rng.random() < .75:
                k, size = people[rng.integers(len(people))]
                d = np.array(k)
                d[:, :2] += rng.normal(0, size * rng.choice([.01, .03, .1, .3]), (joints, 2))
                d[:, 2] = rng.random(joints)
            else:
                size = float(np.exp(rng.uniform(np.log(10.0), np.log(300.0))))
                d = np.stack([rng.uniform(0, 640) + size * (rng.random(joints) - .5), rng.uniform(0, 480) + size * (rng.random(joints) - .5),
                              rng.random(joints)], axis=1)
            score = rng.random()
            dts.append((int(image), round(score, 1) if rng.random() < .3 else score, d))
    sigmas = None if joints == 17 else np.linspace(.025, .107, joints)
    order = rng.permutation(len(dts))
    return make_set([dts[i] for i in order], gts, sigmas, joints)


def margins_ok(oks_per_image, thresholds, near=1e-9, tie=1e-12):
    """may the host form and the numpy restatement be compared on this set?  Their exps differ by an ulp, so a set is left out when
    some OKS lies within `near` of a threshold, or when two OKS of one slot lie within `tie` of each other -- among the values
    that can decide a match: those not below the lowest threshold (anything lower is skipped by every matching whatever it is)"""
    lowest = min(thresholds) - near
    for oks in oks_per_image:
        if oks.size == 0:
            continue
        if (np.abs(oks[:, :, None] - np.asarray(thresholds)[None, None, :]) <= near).any():
            return False
        for row in oks:
            live = np.sort(row[row >= lowest])
            if (np.diff(live) <= tie).any():
                return False
    return True
