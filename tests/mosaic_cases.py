"""Designed inputs of the mosaic tests (tests/test_mosaic_host.py, tests/test_mosaic_gpu.py, tests/mosaic_walk.cpp): people as
(n, 17, 3) float32 (y, x, confidence) built joint by joint, and boxes.  Coordinates are given for a canvas of about 37 x 53 /
38 x 54 (the host tests) and hold on any larger one."""
import numpy as np

F32 = np.float32
J = 17
HEAD = (0, 1, 2, 3, 4)
CELLS = (2, 4, 8, 16, 32)
NAN, INF = float("nan"), float("inf")


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def person(joints, rest=None):
    """(17, 3): joints = {j: (x, y) or (x, y, confidence)}, confidence 0.9 by default; the other joints are dead at (0, 0) unless
    `rest` = (x, y) puts them there alive"""
    p = np.zeros((J, 3), F32)
    if rest is not None:
        p[:] = (rest[1], rest[0], 0.9)
    for j, v in joints.items():
        p[j] = (v[1], v[0], v[2] if len(v) > 2 else 0.9)
    return p


def people():
    """[(name, (17, 3))]: every rule of the region once"""
    face = {0: (20, 12), 1: (22, 10), 2: (18, 10), 3: (25, 11), 4: (15, 11)}
    return [
        ("a frontal face, the body below", person({**face, 15: (16, 36), 16: (24, 36)})),
        ("inside one cell", person({0: (5.9, 4.2), 1: (6.1, 3.0), 2: (4.0, 3.9)})),
        ("over the right and bottom edge cells", person({0: (50, 34), 1: (52, 33), 2: (48, 33)})),
        ("partly outside, top left", person({0: (-3, -2), 1: (1, -4), 2: (-6, 0.5)})),
        ("wholly outside", person({0: (200, 300), 1: (204, 298), 2: (196, 298)})),
        ("wholly outside, negative", person({0: (-200, -300), 1: (-204, -298)})),
        ("nobody live", person({j: (10 + j, 10, 0.2) for j in range(J)})),
        ("the list is dead, the body lives", person({0: (20, 12, 0.1), 1: (22, 10, 0.5), 11: (20, 30), 12: (24, 30)})),
        ("NaN and infinities among the listed joints", person({0: (NAN, 12), 1: (22, INF), 2: (-INF, 10), 3: (30, 14), 4: (26, 11, NAN)})),
        ("only NaN", person({0: (NAN, NAN), 1: (NAN, 3)})),
        ("the ends of the range: the region covers everything", person({0: (-8192, -8192), 1: (16383, 16383)})),
        ("the ends of the range, fractions included", person({0: (-8192.9, 5), 1: (16383.9, 9)})),
        ("one step beyond the range: not live", person({0: (-8193, 5), 1: (16384, 9), 2: (5, 16384)})),
        ("beyond the range, one joint left", person({0: (-8193, 5), 1: (16384, 9), 2: (33, 20)})),
        ("profile: the listed joints on one pixel, rmin decides", person({0: (30, 8), 1: (30.4, 8.7), 3: (30.9, 8.1), 15: (28, 37), 16: (33, 36)})),
        ("profile, nobody else: a single pixel", person({0: (30, 8), 1: (30.4, 8.7)})),
        ("truncation towards zero", person({0: (-0.7, -0.2), 1: (0.9, 0.99)})),
        ("equality with the threshold is not live", person({0: (20, 12, 0.5), 1: (22, 10, 0.5), 2: (40, 30, np.nextafter(F32(0.5), F32(1)))})),
        ("an odd centre", person({0: (20, 12), 1: (23, 15)})),
        ("a negative odd centre", person({0: (-6, -3), 1: (-1, 2)})),
        ("everybody alive at one point", person({}, rest=(26, 18))),
    ]


def all_people():
    return np.stack([p for _, p in people()])


SETTINGS = [  # (joints, threshold, scale, min_half)
    (HEAD, 0.5, (1, 1), None), (HEAD, 0.5, (3, 2), None), (HEAD, 0.5, (64, 1), None), (HEAD, 0.5, (1, 64), 1), (HEAD, 0.5, (1, 1), 4096),
    (None, 0.5, (1, 1), None), ((2, 2, 0), 0.05, (5, 3), 3), (HEAD, -1.0, (1, 1), None), ((16,), 0.5, (2, 1), None),
]

BOXES = np.asarray([[3, 4, 9, 7], [0, 0, 0, 0], [10, 10, 10, 20], [12, 9, 5, 20], [-5, -6, 4, 3], [48, 30, 90, 80], [60, 5, 70, 9],
                    [-20, -20, -1, -1], [31, 15, 33, 17], [-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1], [7, 7, 8, 8], [0, 36, 53, 37]], np.int32)


def scattered(n, h, w, seed, spread=None):
    """n people with a small face somewhere on (or just off) an h x w canvas; spread = (rows, cols): inside that corner only"""
    rng = np.random.default_rng(seed)
    rows, cols = spread or (h + 10, w + 10)
    pts = np.zeros((n, J, 3), F32)
    cx, cy = rng.integers(-5 if spread is None else 3, cols - 3, n), rng.integers(-5 if spread is None else 3, rows - 3, n)
    for j in range(J):
        pts[:, j, 1] = cx + rng.uniform(-3, 3, n) * (1 if j < 5 else 4)
        pts[:, j, 0] = cy + rng.uniform(-3, 3, n) + (0 if j < 5 else 3 * j)
        pts[:, j, 2] = rng.uniform(0.3, 1.0, n)
    return pts
