"""TEST INFRASTRUCTURE ONLY -- the track table's update (include/hrnet_mi355.h: hrn_track_people, steps 1-8) restated in numpy
from the header text, not from the C.  The cost and similarity matrices come from ``hrn_associate_similarity`` and the matching
from ``hrn_assignment``, both pinned by their own tests (tests/test_assoc_host.py, tests/test_postproc.py): what is restated here
is the table logic -- presence, column order, compared state, velocity, ageing, free slots, numbering."""
import numpy as np

from conftest import load_pkg

FIELDS = ("slot_id", "slot_lost", "slot_hits", "slot_row", "slot_boxes", "slot_pts", "slot_vel", "next_id")
I32_MIN, I32_MAX = -2147483648, 2147483647


def copy_table(table):
    return {k: np.array(v, copy=True) for k, v in table.items()}


def table_bits(table):
    return {k: (np.ascontiguousarray(v).view(np.uint32) if v.dtype == np.float32 else v) for k, v in table.items()}


def assert_tables_equal(got, want, what=""):
    g, w = table_bits(got), table_bits(want)
    assert set(g) == set(w) == set(FIELDS), (what, sorted(g))
    for k in FIELDS:
        assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, (what, k)
        assert np.array_equal(g[k], w[k]), (what, k, np.argwhere(g[k] != w[k])[:4].tolist())


def similarity(boxes, pts, d_boxes, d_pts, pose_alpha):
    lib = load_pkg("_lib").load()
    n, m, J = len(boxes), len(d_boxes), pts.shape[1]
    cost, sim = np.zeros((n, m), np.float64), np.zeros((n, m), np.float32)
    if n and m:
        args = [np.ascontiguousarray(a) for a in (boxes, pts, d_boxes, d_pts)]
        rc = lib.hrn_associate_similarity(args[0].ctypes.data, args[1].ctypes.data, n, args[2].ctypes.data, args[3].ctypes.data, m, J,
                                          float(pose_alpha), cost.ctypes.data, sim.ctypes.data)
        assert rc == 0
    return cost, sim


def assignment(cost):
    lib = load_pkg("_lib").load()
    n, m = cost.shape
    col = np.full(n, -1, np.int32)
    if n and m:
        cost = np.ascontiguousarray(cost)
        assert lib.hrn_assignment(cost.ctypes.data, n, m, col.ctypes.data) == 0
    return col


def compared_box(b, v, k):
    """step 3: one box component `k` updates ahead along v"""
    if k == 0.0:
        return int(b)
    with np.errstate(all="ignore"):
        t = np.float64(b) + np.float64(v) * np.float64(k)
    if np.isnan(t):
        return int(b)
    return int(np.trunc(min(max(t, float(I32_MIN)), float(I32_MAX))))


def compared_state(box, joints, vel, k):
    """(box (4,) int32, joints (J, 3) float32) of one slot; vel = (dy, dx)"""
    if k == 0.0:
        return box.copy(), joints.copy()
    cbox = np.array([compared_box(box[c], vel[0] if c & 1 else vel[1], k) for c in range(4)], np.int32)
    cj = joints.copy()
    with np.errstate(all="ignore"):
        cj[:, 0] = (joints[:, 0].astype(np.float64) + np.float64(vel[0]) * k).astype(np.float32)
        cj[:, 1] = (joints[:, 1].astype(np.float64) + np.float64(vel[1]) * k).astype(np.float32)
    return cbox, cj


def velocity(vel, c_now, c_stored, old_lost, old_hits, va):
    with np.errstate(all="ignore"):
        d = (np.float64(c_now) - np.float64(c_stored)) / (np.float64(old_lost) + 1.0)
        v = np.float32(d) if old_hits == 1 else np.float32(np.float64(vel) + np.float64(va) * (d - np.float64(vel)))
    return v if np.isfinite(v) else np.float32(0.0)


def centre(lo, hi):
    return (np.float64(lo) + np.float64(hi)) / 2


def update(boxes, pts, table, pose_alpha, threshold, smoothing_alpha, max_lost, coast, velocity_alpha, counts=None):
    """one update of every stream; `table` (a dict of numpy arrays) is updated in place, boxes / pts are copied.  Returns
    (boxes, pts, ids, match_row, slot, status)."""
    boxes, pts = np.array(boxes, np.int32).reshape(-1, 4), np.array(pts, np.float32)
    P, C = table["slot_id"].shape
    counts = [len(boxes)] if counts is None else list(counts)
    assert len(counts) == P
    start = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    ids, match_row, slot = (np.full(len(boxes), -1, np.int32) for _ in range(3))
    status = np.zeros(P, np.int32)
    a = float(smoothing_alpha)
    f_now, f_before, f_thr = np.float32(1.0 - a), np.float32(a), np.float32(threshold)
    for p in range(P):
        t = {k: table[k][p] for k in FIELDS if k != "next_id"}
        b, q = boxes[start[p]:start[p + 1]], pts[start[p]:start[p + 1]]
        # 1. present rows
        rows = [i for i in range(len(b)) if b[i, 2] > b[i, 0] and b[i, 3] > b[i, 1]]
        # 2. columns
        live = [s for s in range(C) if t["slot_id"][s] >= 0]
        seen = sorted((s for s in live if t["slot_lost"][s] == 0), key=lambda s: (int(t["slot_row"][s]), s))
        cols = seen + [s for s in live if t["slot_lost"][s] != 0]
        # 3. compared state
        ks = {s: (float(t["slot_lost"][s]) + 1.0 if coast else 0.0) for s in cols}
        comp = {s: compared_state(t["slot_boxes"][s], t["slot_pts"][s], t["slot_vel"][s], ks[s]) for s in cols}
        # 4. association
        J = pts.shape[1]
        d_boxes = np.array([comp[s][0] for s in cols], np.int32).reshape(-1, 4)
        d_pts = np.array([comp[s][1] for s in cols], np.float32).reshape(-1, J, 3)
        cost, sim = similarity(b[rows], q[rows], d_boxes, d_pts, pose_alpha)
        if np.isnan(sim).any():
            status[p] |= 1
        col = assignment(cost)
        # 5. accepted pairs
        taken, row_ids = set(), {}
        for r, i in enumerate(rows):
            c = col[r]
            if c < 0 or not sim[r, c] > f_thr:
                continue
            s = cols[c]
            taken.add(s)
            old_lost, old_hits = int(t["slot_lost"][s]), int(t["slot_hits"][s])
            row_ids[i] = int(t["slot_id"][s])
            ids[start[p] + i], slot[start[p] + i] = t["slot_id"][s], s
            match_row[start[p] + i] = t["slot_row"][s] if old_lost == 0 else -1
            stored = t["slot_boxes"][s]
            vy = velocity(t["slot_vel"][s][0], centre(b[i, 1], b[i, 3]), centre(stored[1], stored[3]), old_lost, old_hits, velocity_alpha)
            vx = velocity(t["slot_vel"][s][1], centre(b[i, 0], b[i, 2]), centre(stored[0], stored[2]), old_lost, old_hits, velocity_alpha)
            t["slot_vel"][s] = (vy, vx)
            if a != 0.0:
                cbox, cj = comp[s]
                with np.errstate(all="ignore"):
                    b[i] = [int(np.trunc((1.0 - a) * float(b[i, c4]) + a * float(cbox[c4]))) for c4 in range(4)]
                    q[i] = f_now * q[i] + f_before * cj
            t["slot_boxes"][s], t["slot_pts"][s] = b[i], q[i]
            t["slot_lost"][s], t["slot_hits"][s], t["slot_row"][s] = 0, min(old_hits + 1, 1 << 30), i
        # 6. unaccepted live slots
        for s in cols:
            if s in taken:
                continue
            if int(t["slot_lost"][s]) + 1 > max_lost:
                t["slot_id"][s], t["slot_lost"][s], t["slot_hits"][s], t["slot_row"][s] = -1, 0, 0, -1
                t["slot_boxes"][s], t["slot_pts"][s], t["slot_vel"][s] = 0, 0, 0
            else:
                t["slot_lost"][s] += 1
                t["slot_row"][s] = -1
        # 7. new people
        free = [s for s in range(C) if t["slot_id"][s] < 0]
        nxt = int(table["next_id"][p])
        fresh = [i for i in rows if i not in row_ids]
        for rank, i in enumerate(fresh):
            new_id = np.array(nxt, np.int64).astype(np.uint32) + np.uint32(rank)
            new_id = int(np.array(new_id, np.uint32).view(np.int32))
            row_ids[i] = new_id
            ids[start[p] + i] = new_id
            if rank < len(free):
                s = free[rank]
                slot[start[p] + i] = s
                t["slot_id"][s], t["slot_lost"][s], t["slot_hits"][s], t["slot_row"][s] = new_id, 0, 1, i
                t["slot_boxes"][s], t["slot_pts"][s], t["slot_vel"][s] = b[i], q[i], 0
            else:
                status[p] |= 4
        # 8. next_id
        if rows:
            table["next_id"][p] = max(nxt, min(max(row_ids.values()) + 1, I32_MAX))
    return boxes, pts, ids, match_row, slot, status


# ---- inputs shared by tests/test_tracks_host.py and tests/test_tracks_gpu.py ---------------------------------------------------
def boxes_of(pts):
    """int32 boxes (x1, y1, x2, y2) around (n, J, 3) skeletons, as assoc_cases.people makes them"""
    if len(pts) == 0:
        return np.zeros((0, 4), np.int32)
    b = np.stack([pts[:, :, 1].min(1) - 5, pts[:, :, 0].min(1) - 5, pts[:, :, 1].max(1) + 5, pts[:, :, 0].max(1) + 5], 1)
    return np.round(b).astype(np.int32)


def sequence_frames(seed, P, J, updates=12, special=True):
    """`updates` frames of P streams: per stream 0-9 people moving at constant velocity with jitter, each now and then missing for
    1-4 updates; a person duplicated exactly (ties); a row zeroed (the library's nobody); NaN / inf / -0.0 in joints.  Per frame
    (boxes, pts, counts)."""
    from assoc_cases import people

    rng = np.random.default_rng(seed)
    base, vel, gone = [], [], []
    for p in range(P):
        n = int(rng.integers(0, 10))
        base.append(people(rng, n, J)[0])
        vel.append(rng.uniform(-6, 6, (n, 1, 2)).astype(np.float32))
        gone.append(np.zeros(n, int))
    frames = []
    for u in range(updates):
        all_b, all_p, counts = [], [], []
        for p in range(P):
            rows = []
            for k in range(len(base[p])):
                if gone[p][k] > 0:
                    gone[p][k] -= 1
                    continue
                if u and rng.random() < 0.15:
                    gone[p][k] = int(rng.integers(1, 5)) - 1
                    continue
                person = base[p][k].copy()
                person[:, :2] += vel[p][k] * u + rng.normal(0, 1.0, (J, 2)).astype(np.float32)
                rows.append(person)
            if rows and rng.random() < 0.3:
                rows.append(rows[int(rng.integers(len(rows)))].copy())
            order = rng.permutation(len(rows))
            pts = np.ascontiguousarray(np.stack([rows[k] for k in order])) if rows else np.zeros((0, J, 3), np.float32)
            boxes = boxes_of(pts)
            if len(pts) and rng.random() < 0.3:
                k = int(rng.integers(len(pts)))
                boxes[k], pts[k] = 0, 0
            if special and len(pts) and rng.random() < 0.4:
                k, j = int(rng.integers(len(pts))), int(rng.integers(J))
                pts[k, j, int(rng.integers(2))] = [np.nan, np.inf, -np.inf, -0.0][int(rng.integers(4))]
            all_b.append(boxes), all_p.append(pts), counts.append(len(pts))
        frames.append((np.ascontiguousarray(np.concatenate(all_b)), np.ascontiguousarray(np.concatenate(all_p)), counts))
    return frames


def layout_case(seed, n, live, C, J, lost_every=0, absent_every=0, packed=False, ties=False):
    """one stream's table with `live` live slots of C (spread over the table unless `packed`; every `lost_every`-th lost for 1-3
    updates, the seen ones with a shuffled slot_row) and n current rows: jittered copies of the tracks where they are expected,
    then strangers; every `absent_every`-th row zeroed; `ties`: no jitter and every third row a copy of the row before.  Returns
    (boxes, pts, table) with P = 1."""
    from assoc_cases import people

    pp = load_pkg("postproc")
    rng = np.random.default_rng(seed)
    table = pp.new_track_table(1, C, J)
    slots = np.arange(live) if packed else np.sort(rng.permutation(C)[:live])
    t_pts, t_boxes = people(rng, live, J)
    seen_rows = rng.permutation(live)
    for k, s in enumerate(slots):
        lost = int(rng.integers(1, 4)) if lost_every and k % lost_every == 0 else 0
        table["slot_id"][0, s], table["slot_lost"][0, s], table["slot_hits"][0, s] = 3 * k + 1, lost, int(rng.integers(1, 6))
        table["slot_row"][0, s] = -1 if lost else seen_rows[k]
        table["slot_boxes"][0, s], table["slot_pts"][0, s] = t_boxes[k], t_pts[k]
        table["slot_vel"][0, s] = rng.uniform(-4, 4, 2)
    table["next_id"][0] = 3 * live + 5
    common = min(n, live)
    who = rng.permutation(live)[:common]
    cur = t_pts[who].copy()
    if common:
        steps = table["slot_vel"][0, slots[who]] * (table["slot_lost"][0, slots[who]] + 1)[:, None]
        jitter = np.zeros((common, J, 2)) if ties else rng.normal(0, 2.0, (common, J, 2))
        cur[:, :, :2] += (steps[:, None, :] + jitter).astype(np.float32)
    if n > common:
        cur = np.concatenate([cur, people(rng, n - common, J)[0]])
    cur = np.ascontiguousarray(cur[rng.permutation(n)], dtype=np.float32)
    if ties:
        cur[2::3] = cur[1::3][:len(cur[2::3])]
    boxes = boxes_of(cur)
    if absent_every:
        boxes[::absent_every], cur[::absent_every] = 0, 0
    return boxes, cur, table
