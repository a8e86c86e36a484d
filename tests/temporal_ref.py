"""Joints over time restated in numpy float64 from the definition in include/hrnet_mi355.h (hrn_filter_poses), not from the C
text: the One-Euro filter per joint and axis and the prediction raw + filtered velocity * lookahead, whole frames at a time.
Every operation below is one correctly rounded IEEE operation, as in csrc/temporal_math.h, so the results are compared bit for bit.

Also the inputs tests/test_temporal_host.py and tests/test_temporal_gpu.py share: random sequences with partial matches, dropped
joints and poisoned values, the parameter sets, and the driver that feeds a sequence through any of the three forms."""
import numpy as np

from assoc_cases import sequence

TWO_PI = 6.283185307179586
MAX_AGE = 2 ** 30
DEFAULTS = dict(min_cutoff=1.0, beta=0.007, d_cutoff=1.0, threshold=0.5)
PARAM_SETS = [DEFAULTS, dict(DEFAULTS, beta=0.0), dict(DEFAULTS, min_cutoff=1e6, d_cutoff=1e6), dict(DEFAULTS, min_cutoff=1e-3, d_cutoff=1e-3)]
DTS = (1 / 30, 1 / 25, 0.04171)


def alpha(fc, dt):
    return 1.0 / (1.0 + (1.0 / (TWO_PI * fc)) / dt)


def segments(counts, total):
    c = np.asarray([total] if counts is None else counts, dtype=np.int64).reshape(-1)
    assert c.sum() == total
    return np.concatenate([[0], np.cumsum(c)])


def previous_index(match, counts, prev_counts, n, m):
    """per current person: the index of its previous person in the previous arrays, or -1"""
    before = np.full(n, -1, np.int64)
    if match is None:
        return before
    cur = segments(counts, n)
    prev = np.zeros(len(cur), np.int64) if prev_counts is None and m == 0 else segments(prev_counts, m)
    for p in range(len(cur) - 1):
        for i in range(cur[p], cur[p + 1]):
            if 0 <= match[i] < prev[p + 1] - prev[p]:
                before[i] = prev[p] + int(match[i])
    return before


def filter_poses(pts, state=None, match=None, counts=None, prev_counts=None, dt=1 / 30, min_cutoff=1.0, beta=0.007, d_cutoff=1.0,
                 threshold=0.5, lookahead=None):
    """postproc.filter_poses' arguments and results"""
    pts = np.asarray(pts, np.float32)
    n, J = pts.shape[:2]
    lookahead = dt if lookahead is None else lookahead
    m = 0 if state is None else len(state[0])
    before = previous_index(match, counts, prev_counts, n, m)
    v, conf = pts[:, :, :2], pts[:, :, 2]
    live = (conf > np.float32(threshold)) & np.isfinite(v).all(-1)
    prev_values, prev_age = np.zeros((n, J, 6), np.float32), np.zeros((n, J), np.int32)
    known = before >= 0
    if known.any():
        prev_values[known], prev_age[known] = state[0][before[known]], state[1][before[known]]
    prior = live & (prev_age > 0)
    with np.errstate(all="ignore"):
        x = v.astype(np.float64)
        r, p, d = (prev_values[:, :, k:k + 2].astype(np.float64) for k in (0, 2, 4))
        raw_d = (x - r) / dt
        dh = d + alpha(d_cutoff, dt) * (raw_d - d)
        fc = min_cutoff + beta * np.abs(dh)
        xh = p + alpha(fc, dt) * (x - p)
        hat32, dh32 = xh.astype(np.float32), dh.astype(np.float32)
        pred32 = (x + dh32.astype(np.float64) * lookahead).astype(np.float32)
    pred32 = np.where(np.isfinite(pred32), pred32, v)
    filtered = prior & np.isfinite(hat32).all(-1) & np.isfinite(dh32).all(-1)
    fresh = live & ~filtered
    out, pred = pts.copy(), pts.copy()
    out[:, :, :2][filtered], pred[:, :, :2][filtered] = hat32[filtered], pred32[filtered]
    values, age = np.zeros((n, J, 6), np.float32), np.zeros((n, J), np.int32)
    values[fresh] = np.concatenate([v, v, np.zeros_like(v)], -1)[fresh]
    values[filtered] = np.concatenate([v, hat32, dh32], -1)[filtered]
    age[fresh] = 1
    age[filtered] = np.minimum(prev_age.astype(np.int64) + 1, MAX_AGE)[filtered]
    return out, pred, (values, age)


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
def poison(rng, pts, threshold=0.5):
    """a frame with the values the definition singles out: a confidence exactly at the threshold, NaN / +-inf / -0.0 coordinates
    under a high confidence, and +-3e38 jumps (with a prior: (float)dh overflows and the joint is initialised anew)"""
    n, J = pts.shape[:2]
    if n == 0:
        return pts
    for value in (np.nan, np.inf, -np.inf, -0.0, 3e38, -3e38, 3e38, -3e38):
        i, j, axis = rng.integers(n), rng.integers(J), rng.integers(2)
        pts[i, j, axis], pts[i, j, 2] = value, 0.9
    pts[rng.integers(n), rng.integers(J), 2] = np.float32(threshold)
    pts[rng.integers(n), rng.integers(J), 2] = np.nan
    return pts


def random_match(rng, n, m):
    """a random partial permutation of the m previous people for n current ones, with -1 and values out of range in it"""
    match = np.full(n, -1, np.int32)
    take = rng.permutation(m)[:n]
    match[rng.permutation(n)[:len(take)]] = take
    for i in range(n):
        roll = rng.random()
        if roll < 0.1:
            match[i] = -1
        elif roll < 0.2:
            match[i] = rng.choice([m, m + 5, -2, -7, 2 ** 31 - 1, -2 ** 31])
    return match


def random_sequence(seed, J, streams=1, frames=12, most=9, poisoned=True):
    """`frames` frames of (pts, match, counts, dt): 0..most people per frame over `streams` streams (the middle one of three is
    empty in every other frame), people carried over with a little motion where matched, a fifth of the joints dropped"""
    rng = np.random.default_rng(seed)
    out, prev_pts, prev_counts = [], np.zeros((0, J, 3), np.float32), np.zeros(streams, np.int64)
    for k in range(frames):
        counts = rng.multinomial(int(most * rng.random() ** 0.5 + 0.5), np.ones(streams) / streams)   # 0..most, more often many
        if streams > 1 and k % 2 == 0:
            counts[streams // 2] = 0
        n = int(counts.sum())
        pts = np.empty((n, J, 3), np.float32)
        pts[:, :, :2] = rng.uniform(0, 1000, (n, J, 2))
        pts[:, :, 2] = np.where(rng.random((n, J)) < 0.2, rng.uniform(0, 0.5, (n, J)), rng.uniform(0.5, 1.0, (n, J)))
        match = np.concatenate([random_match(rng, int(c), int(pc)) for c, pc in zip(counts, prev_counts)] + [np.zeros(0, np.int32)])
        before = previous_index(match, counts, prev_counts, n, len(prev_pts))
        for i in np.flatnonzero(before >= 0):            # the same person, moved a little; some joints exactly where they were
            moved = prev_pts[before[i], :, :2] + rng.normal(0, 3, (J, 2)).astype(np.float32) * (rng.random((J, 1)) < 0.8)
            pts[i, :, :2] = np.where(np.isfinite(moved) & (np.abs(moved) < 1e6), moved, pts[i, :, :2])
        if poisoned:
            pts = poison(rng, pts)
        out.append((pts, match.astype(np.int32), counts, DTS[rng.integers(len(DTS))]))
        prev_pts, prev_counts = pts, counts
    return out


def run_sequence(entry, sequence, params, first_match=False, **extra):
    """feeds a sequence through `entry` (filter_poses here, postproc's or the engine's) with the state passed back in; per frame
    (pts_out, pred, values, age) as the entry returned them.  The first frame has no state; its match is withheld unless asked for"""
    state, prev_counts, results = None, None, []
    for k, (pts, match, counts, dt) in enumerate(sequence):
        out, pred, state = entry(pts, state, match if k or first_match else None, counts=counts, prev_counts=prev_counts, dt=dt, **params,
                                 **extra)
        results.append((out, pred, state[0], state[1]))
        prev_counts = counts
    return results


ONE_EURO = dict(min_cutoff=1.5, beta=0.01, d_cutoff=1.0, threshold=0.3, rate=25.0)


def tracker_frames(streams):
    """assoc_cases.sequence for one stream; for three, two more sequences beside it (one of them backwards): (boxes, pts, counts)"""
    runs = [sequence()] if streams == 1 else [sequence(), sequence(seed=9)[::-1], sequence(seed=3)[2:] + sequence(seed=3)[:2]]
    for step in zip(*runs):
        yield (np.concatenate([b for b, _ in step]), np.concatenate([p for _, p in step]),
               None if streams == 1 else [len(b) for b, _ in step])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
