"""Boxes from joints, restated in numpy float64 (include/hrnet_mi355.h: hrn_pose_boxes) -- the definition the host entry and the
kernel are held to, bit for bit -- and the poses the host and GPU tests share.

Joint j of a person is live iff ``confidence > threshold`` in float32 and y and x are finite.  Fewer than ``min_joints`` live
joints: five zeros.  Otherwise, in double, one operation at a time: the extent of the live joints (each coordinate as
``float64(v) + 0.0``), ``c = (lo + hi) * 0.5``, ``side = max((hi - lo) * scale, min_side)``, ``first = max(0, c - side * 0.5)``,
``last = min(limit, c + side * 0.5)`` per axis, ``score = (sum of the live confidences in joint order) / nlive``; each of the
five numbers rounded once to float32."""
import numpy as np


def pose_boxes_ref(pts, frame_hw, threshold=0.5, min_joints=3, scale=1.25, min_side=0.0):
    pts = np.asarray(pts, np.float32)
    n = len(pts)
    hw = np.broadcast_to(np.asarray(frame_hw, np.int64).reshape(-1, 2), (n, 2))
    out = np.zeros((n, 5), np.float32)
    scale, min_side = np.float64(scale), np.float64(min_side)
    for i in range(n):
        y, x, c = pts[i, :, 0], pts[i, :, 1], pts[i, :, 2]
        live = (c > np.float32(threshold)) & np.isfinite(y) & np.isfinite(x)
        nlive = int(live.sum())
        if nlive < min_joints:
            continue
        total = np.float64(0.0)
        for v in c[live]:            # in joint order (np.sum adds pairwise)
            total = total + np.float64(v)
        row = []
        for v, limit in ((x, hw[i, 1]), (y, hw[i, 0])):
            v = v[live].astype(np.float64) + 0.0
            lo, hi = v.min(), v.max()
            centre = (lo + hi) * 0.5
            grown = (hi - lo) * scale
            side = grown if grown > min_side else min_side
            half = side * 0.5
            a, b = centre - half, centre + half
            row.append((a if a > 0.0 else np.float64(0.0), b if b < np.float64(limit) else np.float64(limit)))
        with np.errstate(over="ignore"):
            out[i] = [np.float32(row[0][0]), np.float32(row[1][0]), np.float32(row[0][1]), np.float32(row[1][1]),
                      np.float32(total / np.float64(nlive))]
    return out


# ---- the poses of tests/test_track_host.py and tests/test_track_gpu.py ---------------------------------------------------------
FRAME = (120, 160)   # (height, width) of the constructed rows


def random_poses(n, J, seed, frame_hw=FRAME):
    """people scattered over (and a little beyond) the frame, confidences around the default threshold, some joints broken"""
    rng = np.random.default_rng(seed)
    h, w = frame_hw
    centre = rng.uniform([-0.1 * h, -0.1 * w], [1.1 * h, 1.1 * w], (n, 1, 2))
    spread = rng.uniform(1.0, 0.4 * max(h, w), (n, 1, 1))
    pts = np.empty((n, J, 3), np.float32)
    pts[..., :2] = centre + rng.normal(0.0, 1.0, (n, J, 2)) * spread
    pts[..., 2] = rng.uniform(0.0, 1.0, (n, J))
    pts[..., :2] = np.where(rng.random((n, J, 1)) < 0.3, np.floor(pts[..., :2]), pts[..., :2])   # integer coordinates, as the decode's
    broken = rng.random((n, J))
    pts[..., 2][broken < 0.02] = np.nan
    pts[..., 0][(broken > 0.02) & (broken < 0.03)] = np.inf
    pts[..., 1][(broken > 0.03) & (broken < 0.04)] = np.nan
    pts[rng.random(n) < 0.1, :, 2] *= 0.4          # people with few live joints
    return pts


def person(J, joints, conf=0.9, rest=0.1):
    """(J, 3): the given (y, x[, confidence]) joints first, the others dead (confidence `rest`) at (50, 50)"""
    p = np.empty((J, 3), np.float32)
    p[:] = (50.0, 50.0, rest)
    for j, jt in enumerate(joints):
        p[j] = tuple(jt) + ((conf,) if len(jt) == 2 else ())
    return p


def constructed_cases(J):
    """[(name, pts (n, J, 3), frame_hw, keyword arguments)]: the rows the issue names, each against the default frame"""
    nan, inf = float("nan"), float("inf")
    tri = [(10.0, 20.0), (40.0, 30.0), (25.5, 70.25)]
    cases = [
        ("exactly min_joints live, and one fewer", np.stack([person(J, tri), person(J, tri[:2])]), FRAME, {}),
        ("four live of min_joints 4, and three", np.stack([person(J, tri + [(60.0, 61.0)]), person(J, tri)]), FRAME, {"min_joints": 4}),
        ("a confidence equal to the threshold is not live",
         np.stack([person(J, tri + [(100.0, 150.0, 0.5)]), person(J, tri[:2] + [(100.0, 150.0, 0.5)])]), FRAME, {}),
        ("a NaN confidence is not live", np.stack([person(J, tri + [(100.0, 150.0, nan)])]), FRAME, {}),
        ("NaN or inf coordinates on otherwise live joints",
         np.stack([person(J, tri + [(nan, 150.0), (100.0, inf), (-inf, 3.0), (inf, nan)]), person(J, tri[:2] + [(nan, 1.0)])]), FRAME, {}),
        ("all joints at one point, min_side 0", np.stack([person(J, [(33.0, 44.0)] * 3)]), FRAME, {}),
        ("all joints at one point, min_side 24.5", np.stack([person(J, [(33.0, 44.0)] * 3), person(J, [(2.0, 158.0)] * 3)]), FRAME,
         {"min_side": 24.5}),
        ("joints left of, above and beyond the frame",
         np.stack([person(J, [(10.0, -30.0), (20.0, -5.0), (30.0, -12.0)]), person(J, [(-40.0, 10.0), (-7.0, 80.0), (-9.0, 50.0)]),
                   person(J, [(130.0, 190.0), (150.0, 220.0), (125.0, 200.0)]), person(J, [(60.0, 150.0), (70.0, 190.0), (119.0, 10.0)])]),
         FRAME, {}),
        ("negative coordinates and zeros of both signs",
         np.stack([person(J, [(-3.5, -2.25), (7.0, 9.0), (-0.0, 0.0)]), person(J, [(-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0)]),
                   person(J, [(-5.0, -5.0), (-0.0, -0.0), (-2.0, -1.0)])]), FRAME, {"min_side": 0.0}),
        ("scale 1.0", np.stack([person(J, tri), person(J, [(0.0, 0.0), (119.0, 159.0), (60.0, 80.0)])]), FRAME, {"scale": 1.0}),
        ("a negative threshold takes every finite joint", np.stack([person(J, tri, rest=-1e30)]), FRAME, {"threshold": -3e38}),
        ("a frame size per person", np.stack([person(J, [(10.0, 20.0), (90.0, 120.0), (30.0, 5.0)])] * 3),
         np.asarray([[120, 160], [50, 60], [97, 131]], np.int32), {}),
    ]
    return cases
