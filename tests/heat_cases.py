"""The designed inputs the host and the GPU tests of the heat-map overlay share (tests/test_heatmaps_host.py,
tests/test_heatmaps_gpu.py): the quantiser's edge vector and the canvas / map / box matrix.  Data only; the expected bytes come
from tests/heat_ref.py."""
import numpy as np

F32 = np.float32
SIZES = [(46, 70), (70, 100)]            # tile borders on both axes, a partial last tile, even sides
MAP_SHAPES = [(5, 4), (16, 12), (1, 1)]  # (hq, wq)
J = 3
RANGES = [(0.0, 1.0), (-0.3, 0.9), (0.1, 0.7)]      # (lo, hi): the last two are no powers of two, nor is their difference
HALF_STEPS = [0.0, 0.5, 1.0, 1.5, 127.5, 253.5, 254.5, 255.0]      # t where Q changes, or where it saturates


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def quantise_vector(lo, hi):
    """float32 values whose t = (v - lo) * k lies at, and one ulp of v either side of, every half-step; then the specials"""
    lo, hi = F32(lo), F32(hi)
    k = F32(F32(255.0) / F32(hi - lo))
    out = []
    for t in HALF_STEPS:
        v = F32(lo + F32(F32(t) / k))
        out += [np.nextafter(np.nextafter(v, F32(-np.inf)), F32(-np.inf)), np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf)),
                np.nextafter(np.nextafter(v, F32(np.inf)), F32(np.inf))]
    out += [F32(np.inf), F32(-np.inf), F32(np.nan), F32(-0.0), F32(0.0), lo, hi, F32(1e-30), F32(-1e-30), F32(3e38), F32(-3e38),
            np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf)), F32((lo + hi) / 2)]
    return np.asarray(out, F32)


def quantise_maps(lo, hi):
    """(2, 3, 1, L) maps: person 0 carries the vector in joint 0 beside an all-NaN joint and a -inf joint; person 1 carries it in
    joint 2 beside NaN in joint 0 (a NaN FIRST must not stick) and the vector reversed in joint 1; the last cell of both is all NaN"""
    v = quantise_vector(lo, hi)
    v = np.concatenate([v, [F32(np.nan)]])
    L = len(v)
    maps = np.empty((2, 3, 1, L), F32)
    maps[0, 0, 0], maps[0, 1, 0], maps[0, 2, 0] = v, np.nan, -np.inf
    maps[1, 0, 0], maps[1, 1, 0], maps[1, 2, 0] = np.nan, v[::-1], v
    maps[:, :, 0, L - 1] = np.nan
    return maps


def random_maps(n, hq, wq, seed, joints=J):
    """values over [-0.2, 1.2] (both clips engage for vmin, vmax = 0, 1), a few NaN and infinities"""
    rng = np.random.default_rng(seed)
    maps = rng.uniform(-0.2, 1.2, (n, joints, hq, wq)).astype(F32)
    special = rng.uniform(0, 1, maps.shape)
    maps[special < 0.03] = np.nan
    maps[(special >= 0.03) & (special < 0.04)] = np.inf
    maps[(special >= 0.04) & (special < 0.05)] = -np.inf
    return maps


def drawn_boxes(h, w, hq, wq):
    """boxes of which something shows, or could: wider and narrower than the map, one pixel wide, across the tile borders, over
    every canvas edge, fully outside"""
    return np.asarray([
        [3, 5, 3 + 3 * wq + 1, 5 + 2 * hq + 1],              # wider than the map
        [40, 8, 40 + max(1, wq // 2), 8 + max(1, hq // 2)],  # narrower (bw < wq where wq > 1)
        [20, 3, 21, 40], [2, 40, 38, 41],                    # bw = 1, bh = 1
        [28, 27, 37, 36],                                    # across x = 31 | 32 and y = 31 | 32
        [-7, -9, 12, 15], [w - 9, h - 11, w + 13, h + 6], [-5, h - 8, w + 5, h + 20], [w - 3, -4, w + 9, h + 4],      # over every edge
        [w + 3, 2, w + 30, 20], [-40, -40, -2, -3], [5, h, 30, h + 9], [w, 5, w + 9, 30],                          # fully outside
    ], np.int32)


SKIPPED_BOXES = np.asarray([[5, 5, 5, 20], [5, 5, 20, 5], [20, 5, 10, 20], [5, 20, 20, 10], [0, 0, 0, 0], [-8193, 0, 40, 40],
                            [0, -8193, 40, 40], [0, 0, 16384, 40], [0, 0, 40, 16384], [-2147483648, 0, 2147483647, 40]], np.int32)
OVERLAPPING = np.asarray([[6, 4, 52, 39], [25, 18, 66, 44]], np.int32)
EVERYTHING = np.asarray([[-8192, -8192, 16383, 16383]], np.int32)


def settings(k):
    """the blend settings the matrix alternates: (alpha, mode 0 CONST | 1 VALUE, cutoff)"""
    return [(153, 1, 26), (200, 0, 1), (255, 1, 128), (77, 0, 40)][k % 4]


def matrix():
    """[(name, h, w, maps (n, J, hq, wq), boxes (n, 4), mask or None, (alpha, mode, cutoff), unchanged)]: `unchanged` cases must
    leave the canvas as it was"""
    out = []
    k = 0
    for h, w in SIZES:
        for hq, wq in MAP_SHAPES:
            boxes = drawn_boxes(h, w, hq, wq)
            tag = "%dx%d maps %dx%d" % (h, w, hq, wq)
            out.append((tag + " drawn", h, w, random_maps(len(boxes), hq, wq, 10 + k), boxes, None, settings(k), False))
            out.append((tag + " single joint", h, w, random_maps(len(boxes), hq, wq, 20 + k), boxes, [0, 1, 0], settings(k + 1), False))
            out.append((tag + " skipped", h, w, random_maps(len(SKIPPED_BOXES), hq, wq, 30 + k), SKIPPED_BOXES, None, settings(k + 1), True))
            out.append((tag + " everything", h, w, random_maps(2, hq, wq, 40 + k), np.concatenate([EVERYTHING, boxes[:1]]), [1, 0, 1],
                        settings(k + 2), False))
            k += 1
    return out
