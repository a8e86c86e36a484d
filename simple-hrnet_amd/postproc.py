"""The reference's host-side pose post-processing on the native library: OKS NMS (``misc/nms/nms.py:97-180``) and the
tracker's association step (``misc/utils.py:372-429``) -- same names, arguments and results.

The arithmetic (OKS, box IoU, the similarity matrices, the optimal assignment) is in ``csrc/postproc.cpp`` behind the C
ABI; what the reference does with numpy around it -- the score sort, the float32 blend of the two similarity matrices,
thresholding, temporal smoothing (with numpy's casting into the caller's arrays) and the numbering of new people -- is
done with the same numpy expressions here, so dtypes and tie-breaks are numpy's.  No pure-Python twin: without the
library these functions raise like the rest of the package."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np

from . import _lib


def _nan_if_none(v) -> float:
    return float("nan") if v is None else float(v)


def _db_arrays(kpts_db: Sequence[dict]):
    entries = list(kpts_db)
    scores = np.array([e["score"] for e in entries])
    kpts = np.ascontiguousarray(np.stack([np.asarray(e["keypoints"]).reshape(-1) for e in entries]), np.float64)
    areas = np.ascontiguousarray(np.array([e["area"] for e in entries]), np.float64)
    if kpts.ndim != 2 or kpts.shape[1] % 3:
        raise ValueError("keypoints must be (J, 3) per entry")
    return scores, kpts, areas


def _sigmas(sigmas, joints):
    if isinstance(sigmas, np.ndarray):
        s = np.ascontiguousarray(sigmas, np.float64)
        if s.shape != (joints,):
            raise ValueError("sigmas must have one value per joint")
        return s
    if joints != 17:
        raise ValueError("the default sigmas are COCO's 17; pass sigmas for %d joints" % joints)
    return None


def oks_nms(kpts_db: Sequence[dict], thresh: float, sigmas=None, in_vis_thre=None) -> List[int]:
    """``misc/nms/nms.py:97-122``: greedy NMS with OKS as the overlap; returns the indices to keep, best first."""
    if len(kpts_db) == 0:
        return []
    scores, kpts, areas = _db_arrays(kpts_db)
    n, joints = kpts.shape[0], kpts.shape[1] // 3
    sg = _sigmas(sigmas, joints)
    order = np.ascontiguousarray(scores.argsort()[::-1], np.int32)
    keep = np.zeros(n, np.int32)
    num = ctypes.c_int32(0)
    rc = _lib.load().hrn_oks_nms(keep.ctypes.data, ctypes.byref(num), kpts.ctypes.data, areas.ctypes.data, order.ctypes.data, n, joints,
                                 float(thresh), None if sg is None else sg.ctypes.data, _nan_if_none(in_vis_thre))
    if rc:
        raise ValueError("hrn_oks_nms: bad arguments")
    return [int(i) for i in keep[:num.value]]


def soft_oks_nms(kpts_db: Sequence[dict], thresh: float, sigmas=None, in_vis_thre=None):
    """``misc/nms/nms.py:138-180``: gaussian rescoring instead of removal, at most 20 kept; returns an index array."""
    if len(kpts_db) == 0:
        return []
    scores, kpts, areas = _db_arrays(kpts_db)
    n, joints = kpts.shape[0], kpts.shape[1] // 3
    sg = _sigmas(sigmas, joints)
    order64 = scores.argsort()[::-1]
    sorted_scores = np.ascontiguousarray(scores[order64], np.float64)
    order = np.ascontiguousarray(order64, np.int32)
    keep = np.zeros(max(n, 20), np.int32)
    num = ctypes.c_int32(0)
    rc = _lib.load().hrn_soft_oks_nms(keep.ctypes.data, ctypes.byref(num), kpts.ctypes.data, areas.ctypes.data, sorted_scores.ctypes.data,
                                      order.ctypes.data, n, joints, float(thresh), None if sg is None else sg.ctypes.data,
                                      _nan_if_none(in_vis_thre))
    if rc:
        raise ValueError("hrn_soft_oks_nms: bad arguments")
    return keep[:num.value].astype(np.intp)


def compute_similarity_matrices(bboxes_a, bboxes_b, poses_a, poses_b):
    """``misc/utils.py:372-384``: ``(box IoU, OKS)`` of every skeleton of a against every skeleton of b, float32."""
    assert len(bboxes_a) == len(poses_a) and len(bboxes_b) == len(poses_b)
    na, nb = len(poses_a), len(poses_b)
    pa = np.ascontiguousarray(poses_a, np.float32).reshape(na, -1, 3) if na else np.zeros((0, 1, 3), np.float32)
    pb = np.ascontiguousarray(poses_b, np.float32).reshape(nb, -1, 3) if nb else np.zeros((0, 1, 3), np.float32)
    joints = pa.shape[1] if na else pb.shape[1]
    if na and nb and pa.shape[1] != pb.shape[1]:
        raise ValueError("the two sets of skeletons have different joint counts")
    ba = np.ascontiguousarray(np.asarray(bboxes_a, np.float64).reshape(na, 4))
    bb = np.ascontiguousarray(np.asarray(bboxes_b, np.float64).reshape(nb, 4))
    result_bbox = np.zeros((na, nb), dtype=np.float32)
    result_pose = np.zeros((na, nb), dtype=np.float32)
    if na and nb:
        rc = _lib.load().hrn_pose_similarity(ba.ctypes.data, pa.ctypes.data, na, bb.ctypes.data, pb.ctypes.data, nb, joints,
                                             result_bbox.ctypes.data, result_pose.ctypes.data)
        if rc:
            raise ValueError("hrn_pose_similarity: bad arguments")
    return result_bbox, result_pose


def assignment(cost) -> List[tuple]:
    """What ``munkres.Munkres().compute(cost)`` returns (``misc/utils.py:406-407``): the pairs of a minimum-cost matching."""
    c = np.ascontiguousarray(cost, np.float64)
    if c.ndim != 2 or c.size == 0:
        return []
    row_to_col = np.full(c.shape[0], -1, np.int32)
    rc = _lib.load().hrn_assignment(c.ctypes.data, c.shape[0], c.shape[1], row_to_col.ctypes.data)
    if rc:
        raise ValueError("hrn_assignment: costs must be finite")
    return [(r, int(col)) for r, col in enumerate(row_to_col) if col >= 0]


def find_person_id_associations(boxes, pts, prev_boxes, prev_pts, prev_person_ids, next_person_id=0, pose_alpha=0.5,
                                similarity_threshold=0.5, smoothing_alpha=0.):
    """``misc/utils.py:387-429``: match the current skeletons to the previous frame's, carry the ids over, smooth matched
    boxes / joints in place, number the new people from ``next_person_id``.  Returns ``(boxes, pts, person_ids)``."""
    sim_box, sim_pose = compute_similarity_matrices(boxes, prev_boxes, pts, prev_pts)
    # the blend keeps the reference's operand order (float32 matrix * python float, pose term first): its rounding decides
    # which pairs clear the threshold
    similarity_matrix = sim_pose * pose_alpha + sim_box * (1 - pose_alpha)
    pairs = assignment((1 - similarity_matrix).tolist())
    person_ids = np.full(len(pts), -1, dtype=np.int32)

    def blend(now, before):   # linear temporal filter; assigning the result casts it to the caller's dtype (int32 boxes truncate)
        return (1 - smoothing_alpha) * now + smoothing_alpha * before

    for cur, prev in pairs:
        if not similarity_matrix[cur, prev] > similarity_threshold:
            continue
        person_ids[cur] = prev_person_ids[prev]
        if smoothing_alpha:
            boxes[cur], pts[cur] = blend(boxes[cur], prev_boxes[prev]), blend(pts[cur], prev_pts[prev])
    fresh = person_ids == -1
    person_ids[fresh] = np.arange(next_person_id, next_person_id + np.sum(fresh))
    return boxes, pts, person_ids


def _segments(counts, total: int, what: str) -> np.ndarray:
    """``counts`` of ``associate_people`` as the int32 segment table (P + 1 starts); None: one problem with everybody"""
    c = np.asarray([total] if counts is None else counts, dtype=np.int64).reshape(-1)
    if (c < 0).any() or int(c.sum()) != total:
        raise ValueError("%s must be non-negative and sum to %d people, got %s" % (what, total, c.tolist()))
    return np.ascontiguousarray(np.concatenate([[0], np.cumsum(c)]), dtype=np.int32)


def _next_ids(next_id, problems: int) -> np.ndarray:
    """``next_id`` of ``associate_people`` as P int32 values of its own (one int serves every problem)"""
    v = np.array(next_id, dtype=np.int32).reshape(-1)
    if len(v) == 1 and problems != 1:
        v = np.repeat(v, problems)
    if len(v) != problems:
        raise ValueError("next_id must hold one value per problem: %d for %d" % (len(v), problems))
    return np.ascontiguousarray(v)


def associate_people(boxes, pts, prev_boxes, prev_pts, prev_ids, next_id, pose_alpha=0.5, similarity_threshold=0.5,
                     smoothing_alpha=0., counts=None, prev_counts=None):
    """``find_person_id_associations`` plus the demo's ``next_id = max(next_id, max(ids) + 1)`` for P independent problems in one
    native call (``hrn_associate_people``, no GPU): the host form of ``NativeHRNet.associate_people``, equal to it bit for bit.

    ``boxes`` (n, 4) int32, ``pts`` (n, J, 3) float32 ``(y, x, confidence)``, ``prev_*`` likewise with ``prev_ids`` (m,) int32;
    ``counts`` / ``prev_counts``: people per problem on either side (the streams of a camera wall; None: one problem);
    ``next_id``: one int, or one per problem.  C-contiguous int32 ``boxes`` / float32 ``pts`` are smoothed IN PLACE, as
    ``find_person_id_associations`` does; anything else is converted first and the converted arrays are returned.
    Returns ``(boxes, pts, ids (n,) int32, match (n,) int32, next_id (P,) int32, status (P,) int32)``: ``match`` is the accepted
    previous person counted inside its problem, or -1; ``status`` bit 0: a non-finite similarity (two zero boxes) was counted as 0
    and not accepted -- where ``find_person_id_associations`` raises.  At most 256 people per problem and side."""
    boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    prev_boxes = np.ascontiguousarray(prev_boxes, dtype=np.int32).reshape(-1, 4)
    pts, prev_pts = np.ascontiguousarray(pts, dtype=np.float32), np.ascontiguousarray(prev_pts, dtype=np.float32)
    prev_ids = np.ascontiguousarray(prev_ids, dtype=np.int32).reshape(-1)
    if pts.size == 0 and pts.ndim != 3:           # (an empty list of skeletons)
        pts = pts.reshape(0, prev_pts.shape[1] if prev_pts.ndim == 3 else 1, 3)
    if prev_pts.size == 0 and prev_pts.ndim != 3:
        prev_pts = prev_pts.reshape(0, pts.shape[1], 3)
    n, m = len(boxes), len(prev_boxes)
    if pts.ndim != 3 or prev_pts.ndim != 3 or pts.shape[2] != 3 or prev_pts.shape[2] != 3 or len(pts) != n or len(prev_pts) != m \
            or len(prev_ids) != m:
        raise ValueError("pts must be (n, J, 3) beside (n, 4) boxes, and prev_ids one per previous person: got %s, %s, %s, %s, %s"
                         % (boxes.shape, pts.shape, prev_boxes.shape, prev_pts.shape, prev_ids.shape))
    if n and m and pts.shape[1] != prev_pts.shape[1]:
        raise ValueError("the two sets of skeletons have different joint counts")
    joints = int(pts.shape[1] if n else prev_pts.shape[1]) or 1
    cur, prev = _segments(counts, n, "counts"), _segments(prev_counts, m, "prev_counts")
    if len(cur) != len(prev):
        raise ValueError("counts and prev_counts name %d and %d problems" % (len(cur) - 1, len(prev) - 1))
    problems = len(cur) - 1
    nxt = _next_ids(next_id, problems)
    ids, match, status = np.empty(n, np.int32), np.empty(n, np.int32), np.zeros(problems, np.int32)
    lib = _lib.load()
    rc = lib.hrn_associate_people(problems, cur.ctypes.data, prev.ctypes.data, joints, boxes.ctypes.data, pts.ctypes.data,
                                  prev_boxes.ctypes.data, prev_pts.ctypes.data, prev_ids.ctypes.data, nxt.ctypes.data,
                                  float(pose_alpha), float(similarity_threshold), float(smoothing_alpha), ids.ctypes.data,
                                  match.ctypes.data, status.ctypes.data)
    if rc:
        raise ValueError("hrn_associate_people: " + lib.hrn_associate_people_last_error().decode())
    return boxes, pts, ids, match, nxt, status


HRN_MAX_TRACKED = 256
# the arrays of a track table in the entries' order: name, shape behind (P, C), dtype, value of a fresh table
TRACK_FIELDS = (("slot_id", (), np.int32, -1), ("slot_lost", (), np.int32, 0), ("slot_hits", (), np.int32, 0), ("slot_row", (), np.int32, -1),
                ("slot_boxes", (4,), np.int32, 0), ("slot_pts", None, np.float32, 0), ("slot_vel", (2,), np.float32, 0))


def new_track_table(streams: int = 1, capacity: int = HRN_MAX_TRACKED, joints: int = 17) -> dict:
    """a fresh track table for ``track_people``: a dict of numpy arrays, ``slot_id`` / ``slot_lost`` / ``slot_hits`` / ``slot_row``
    (P, C) int32, ``slot_boxes`` (P, C, 4) int32, ``slot_pts`` (P, C, J, 3) float32, ``slot_vel`` (P, C, 2) float32 and ``next_id``
    (P,) int32 -- ids and rows -1, everything else 0"""
    if streams < 0 or not 1 <= capacity <= HRN_MAX_TRACKED or joints < 1:
        raise ValueError("a track table needs streams >= 0, 1 <= capacity <= %d and joints >= 1, got %d, %d, %d"
                         % (HRN_MAX_TRACKED, streams, capacity, joints))
    table = {name: np.full((streams, capacity) + ((joints, 3) if tail is None else tail), fill, dtype)
             for name, tail, dtype, fill in TRACK_FIELDS}
    table["next_id"] = np.zeros(streams, np.int32)
    return table


def track_table_shape(table, shape_of) -> tuple:
    """(P, C, J) of a track table whose arrays answer ``shape_of(array)``; raises on a table that is not one"""
    try:
        shapes = {name: tuple(shape_of(table[name])) for name, *_ in TRACK_FIELDS}
        shapes["next_id"] = tuple(shape_of(table["next_id"]))
    except (KeyError, TypeError) as exc:
        raise ValueError("a track table is the dict new_track_table returns: %s" % (exc,))
    pts = shapes["slot_pts"]
    if len(pts) != 4 or pts[3] != 3:
        raise ValueError("slot_pts must be (P, C, J, 3), got %s" % (pts,))
    P, C, J = pts[:3]
    want = {name: (P, C) + ((J, 3) if tail is None else tail) for name, tail, _, _ in TRACK_FIELDS}
    want["next_id"] = (P,)
    if shapes != want:
        raise ValueError("the arrays of the track table do not fit together: %s" % (shapes,))
    return int(P), int(C), int(J)


def track_people(boxes, pts, table, pose_alpha=0.5, similarity_threshold=0.5, smoothing_alpha=0., max_lost=0, coast=False,
                 velocity_alpha=0.5, counts=None):
    """one update of a track table (``hrn_track_people``, no GPU): the host form of ``NativeHRNet.track_people``, equal to it bit
    for bit.  ``include/hrnet_mi355.h`` states the update; in short: rows with an empty box are nobody (ids -1); the others are
    matched against the live tracks -- lost ones for up to ``max_lost`` updates, with ``coast`` where their velocity expects them
    -- exactly as ``associate_people`` matches two frames; new people take free slots and fresh ids.

    ``boxes`` (n, 4) int32, ``pts`` (n, J, 3) float32 ``(y, x, confidence)``; ``table``: what ``new_track_table`` returned,
    C-contiguous arrays of its dtypes, updated IN PLACE (``next_id`` included); ``counts``: rows per stream (None: one stream).
    C-contiguous int32 ``boxes`` / float32 ``pts`` are smoothed in place, anything else is converted first.  Returns
    ``(boxes, pts, ids, match_row, slot, status)``: ``match_row`` the row the person had in the previous update (what
    ``filter_poses`` takes as ``match``) or -1, ``slot`` the person's slot or -1, ``status`` per stream (bits 0, 1 as
    ``associate_people``; bit 2: the table was full and somebody new got no slot)."""
    streams, capacity, joints = track_table_shape(table, lambda a: a.shape)
    for name, _, dtype, _ in TRACK_FIELDS + (("next_id", (), np.int32, 0),):
        a = table[name]
        if not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError("%s of the track table must be a writable C-contiguous %s array" % (name, np.dtype(dtype).name))
    boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    if pts.size == 0 and pts.ndim != 3:
        pts = pts.reshape(0, joints, 3)
    n = len(boxes)
    if pts.ndim != 3 or pts.shape[2] != 3 or len(pts) != n or (n and pts.shape[1] != joints):
        raise ValueError("pts must be (n, %d, 3) beside (n, 4) boxes: got %s, %s" % (joints, boxes.shape, pts.shape))
    cur = _segments(counts, n, "counts")
    if len(cur) - 1 != streams:
        raise ValueError("counts names %d streams, the table holds %d" % (len(cur) - 1, streams))
    ids, match_row, slot = (np.empty(n, np.int32) for _ in range(3))
    status = np.zeros(streams, np.int32)
    lib = _lib.load()
    rc = lib.hrn_track_people(streams, cur.ctypes.data, capacity, joints, boxes.ctypes.data, pts.ctypes.data,
                              *[table[name].ctypes.data for name, *_ in TRACK_FIELDS], table["next_id"].ctypes.data, float(pose_alpha),
                              float(similarity_threshold), float(smoothing_alpha), int(max_lost), int(coast), float(velocity_alpha),
                              ids.ctypes.data, match_row.ctypes.data, slot.ctypes.data, status.ctypes.data)
    if rc:
        raise ValueError("hrn_track_people: " + lib.hrn_track_people_last_error().decode())
    return boxes, pts, ids, match_row, slot, status


def filter_arguments(pts_shape,state_shapes, match_len, counts, prev_counts, dt, min_cutoff, beta, d_cutoff, threshold, lookahead):
    """what ``filter_poses`` and ``NativeHRNet.filter_poses`` share, from shapes alone: ``(n, m, joints, cur, prev, numbers)`` --
    people on either side, J, the two int32 segment tables and the six numbers in the entries' order (``lookahead=None``: ``dt``)"""
    if len(pts_shape) != 3 or pts_shape[2] != 3:
        raise ValueError("pts must be (n, J, 3), got %s" % (tuple(pts_shape),))
    n, m = int(pts_shape[0]), 0
    if n and pts_shape[1] < 1:
        raise ValueError("pts holds people without joints: %s" % (tuple(pts_shape),))
    if state_shapes is not None:
        values, age = (tuple(s) for s in state_shapes)
        if len(values) != 3 or values[2] != 6 or age != values[:2]:
            raise ValueError("state must be ((m, J, 6) values, (m, J) ages), got %s and %s" % (values, age))
        m = int(values[0])
        if n and m and values[1] != pts_shape[1]:
            raise ValueError("the state holds %d joints per person, pts %d" % (values[1], pts_shape[1]))
    joints = int(pts_shape[1] if n or not m else state_shapes[0][1]) or 1
    if match_len is not None and match_len != n:
        raise ValueError("match must hold one value per person: %d for %d" % (match_len, n))
    cur = _segments(counts, n, "counts")
    prev = np.zeros(len(cur), np.int32) if prev_counts is None and m == 0 else _segments(prev_counts, m, "prev_counts")
    if len(cur) != len(prev):
        raise ValueError("counts and prev_counts name %d and %d streams" % (len(cur) - 1, len(prev) - 1))
    dt = float(dt)
    return n, m, joints, cur, prev, (dt, float(min_cutoff), float(beta), float(d_cutoff), float(threshold), dt if lookahead is None else float(lookahead))


def filter_poses(pts, state=None, match=None, counts=None, prev_counts=None, dt=1 / 30, min_cutoff=1.0, beta=0.007, d_cutoff=1.0,
                 threshold=0.5, lookahead=None):
    """Joints over time in one native call (``hrn_filter_poses``, no GPU): the One-Euro filter (Casiez, Roussel, Vogel, CHI 2012)
    of every joint and the prediction of the next frame's joints -- the host form of ``NativeHRNet.filter_poses``, equal to it bit
    for bit (``include/hrnet_mi355.h`` states the arithmetic in full).

    ``pts`` (n, J, 3) float32 ``(y, x, confidence)`` of this frame; ``state``: what the previous call returned, or None on the
    first frame; ``match`` (n,) int32: who of the previous frame each person is, counted inside its stream, or -1
    (``associate_people``'s ``match``; None: nobody is known); ``counts`` / ``prev_counts``: people per stream on either side
    (None: one stream); ``dt``: seconds since the previous frame; ``min_cutoff`` (Hz: less jitter at rest when lower), ``beta``
    (less lag in motion when higher), ``d_cutoff``: the filter's parameters; joints with ``confidence > threshold`` and finite
    coordinates are filtered, the others pass through and lose their state; ``lookahead``: seconds ahead of this frame that the
    prediction looks (None: ``dt``, the next frame).

    Returns ``(pts_out, pred, state)``: the filtered joints, the predicted joints ``raw position + filtered velocity * lookahead``
    (what ``track_frame`` wants as ``prev_pts``) and the ``(values (n, J, 6) float32, age (n, J) int32)`` pair to pass back in.
    The prediction starts from the RAW position on purpose: the filtered position lags on steady motion -- the filter's known
    trade, tuned by ``beta`` -- while raw + velocity converges to zero error.  ``pts`` is left as it is."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    if pts.size == 0 and pts.ndim != 3:           # (an empty list of skeletons)
        pts = pts.reshape(0, state[0].shape[1] if state is not None and np.ndim(state[0]) == 3 else 1, 3)
    if state is not None:
        state = np.ascontiguousarray(state[0], dtype=np.float32), np.ascontiguousarray(state[1], dtype=np.int32)
    if match is not None:
        match = np.ascontiguousarray(match, dtype=np.int32).reshape(-1)
    n, m, joints, cur, prev, numbers = filter_arguments(pts.shape, None if state is None else (state[0].shape, state[1].shape),
                                                        None if match is None else len(match), counts, prev_counts, dt, min_cutoff, beta,
                                                        d_cutoff, threshold, lookahead)
    pts_out, pred = np.empty_like(pts), np.empty_like(pts)
    values, age = np.empty((n, joints, 6), np.float32), np.empty((n, joints), np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    lib = _lib.load()
    rc = lib.hrn_filter_poses(len(cur) - 1, cur.ctypes.data, prev.ctypes.data, joints, ptr(pts), ptr(match), ptr(state and state[0]),
                              ptr(state and state[1]), *numbers, ptr(pts_out), ptr(pred), ptr(values), ptr(age))
    if rc:
        raise ValueError("hrn_filter_poses: " + lib.hrn_filter_poses_last_error().decode())
    return pts_out, pred, (values, age)


POSE_NMS_SOFT, POSE_NMS_SUPPRESS, POSE_NMS_ENGINE = 1, 2, 4      # HRN_POSE_NMS_* of include/hrnet_mi355.h


def pose_nms_flags(engine: bool, soft: bool, suppress: bool) -> int:
    return (POSE_NMS_ENGINE if engine else 0) | (POSE_NMS_SOFT if soft else 0) | (POSE_NMS_SUPPRESS if suppress else 0)


def pose_nms(pts=None, boxes=None, det_scores=None, counts=None, thresh=0.9, in_vis_thre=None, rescore_thre=None, soft=False,
             sigmas=None, suppress=False, kpts=None, areas=None, scores=None):
    """Rescoring and OKS NMS, hard or soft, of P independent problems in one native call (``hrn_pose_nms``, no GPU): the host form
    of ``NativeHRNet.pose_nms``, equal to it bit for bit.  The people come in one of two layouts:

    * engine layout: ``pts`` (n, J, 3) float32 ``(y, x, confidence)`` and ``boxes`` (n, 4) int32 as ``predict_frame`` /
      ``track_frame`` return them, ``det_scores`` (n,) float32 or None (1.0);
    * COCO layout (``misc/nms/nms.py``'s): ``kpts`` (n, J, 3) float64 ``(x, y, score)``, ``areas`` (n,), ``scores`` (n,) float64.

    ``counts``: people per problem (the images of an evaluation, the streams of a camera wall; None: one problem).
    ``in_vis_thre``: only the candidate's joints above it enter an OKS (None: all).  ``rescore_thre``: every score first becomes
    the mean confidence of the person's joints above it times the score (``datasets/COCO.py:360-372``; None: off).  ``sigmas``: J
    values, or None for COCO's 17.  ``soft``: gaussian rescoring instead of removal, at most 20 kept.  The order is descending
    score and stable (equal scores keep index order; NaN last).  ``suppress`` (engine layout): everybody who is not kept gets zero
    confidences and a zero box IN PLACE when ``pts`` / ``boxes`` are C-contiguous float32 / int32 arrays, else in the converted
    arrays that are returned.

    Returns a dict: ``keep`` (n,) int32 -- per problem the kept people in selection order, counted from the problem's first
    person, then -1; ``num`` (P,); ``scores`` (n,) float64 after rescoring; ``suppressor`` (n,) -- -1 kept, else who removed it
    (soft: -2 for the people left over at the cap); ``status`` (P,) -- bit 0: a NaN score was ordered last, bit 1: a non-finite OKS
    counted as 0; in the engine layout also ``pts`` and ``boxes``."""
    engine = kpts is None
    if engine:
        if pts is None or boxes is None or areas is not None or scores is not None:
            raise ValueError("give pts and boxes (engine layout) or kpts, areas and scores (COCO layout)")
        k = np.ascontiguousarray(pts, dtype=np.float32)
        a = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
        sc = None if det_scores is None else np.ascontiguousarray(det_scores, dtype=np.float32).reshape(-1)
    else:
        if pts is not None or boxes is not None or det_scores is not None or areas is None or scores is None:
            raise ValueError("give pts and boxes (engine layout) or kpts, areas and scores (COCO layout)")
        k = np.ascontiguousarray(kpts, dtype=np.float64)
        a = np.ascontiguousarray(areas, dtype=np.float64).reshape(-1)
        sc = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
    n = len(a)
    if k.size == 0 and k.ndim != 3:
        k = k.reshape(0, 17 if sigmas is None else len(sigmas), 3)
    if k.ndim != 3 or k.shape[2] != 3 or len(k) != n or (sc is not None and len(sc) != n):
        raise ValueError("keypoints must be (n, J, 3) beside n areas / boxes and n scores, got %s, %s, %s"
                         % (k.shape, a.shape, None if sc is None else sc.shape))
    joints = int(k.shape[1])
    sg = None if sigmas is None else np.ascontiguousarray(sigmas, dtype=np.float64).reshape(-1)
    if sg is not None and len(sg) != joints:
        raise ValueError("sigmas must have one value per joint")
    seg = _segments(counts, n, "counts")
    problems = len(seg) - 1
    keep, num = np.full(n, -1, np.int32), np.zeros(problems, np.int32)
    scores_out, suppressor, status = np.zeros(n, np.float64), np.full(n, -1, np.int32), np.zeros(problems, np.int32)
    lib = _lib.load()
    rc = lib.hrn_pose_nms(problems, seg.ctypes.data, joints, pose_nms_flags(engine, soft, suppress), k.ctypes.data, a.ctypes.data,
                          None if sc is None else sc.ctypes.data, float(thresh), _nan_if_none(in_vis_thre), _nan_if_none(rescore_thre),
                          None if sg is None else sg.ctypes.data, keep.ctypes.data, num.ctypes.data, scores_out.ctypes.data,
                          suppressor.ctypes.data, status.ctypes.data)
    if rc:
        raise ValueError("hrn_pose_nms: " + lib.hrn_pose_nms_last_error().decode())
    out = dict(keep=keep, num=num, scores=scores_out, suppressor=suppressor, status=status)
    if engine:
        out["pts"], out["boxes"] = k, a
    return out


def pose_nms_oks_row(kpts, areas, g: int, in_vis_thre=None, sigmas=None) -> np.ndarray:
    """The OKS of every person of one problem (COCO layout) against its person ``g`` as ``pose_nms`` computes it -- what
    ``oks_iou(kpts[g], kpts, areas[g], areas, sigmas, in_vis_thre)`` of ``misc/nms/nms.py`` returns, in pose_nms_math.h's
    arithmetic (``hrn_pose_nms_oks_row``, no GPU)."""
    k = np.ascontiguousarray(kpts, dtype=np.float64)
    a = np.ascontiguousarray(areas, dtype=np.float64).reshape(-1)
    if k.ndim != 3 or k.shape[2] != 3 or len(k) != len(a):
        raise ValueError("kpts must be (n, J, 3) beside n areas, got %s, %s" % (k.shape, a.shape))
    sg = None if sigmas is None else np.ascontiguousarray(sigmas, dtype=np.float64).reshape(-1)
    if sg is not None and len(sg) != k.shape[1]:
        raise ValueError("sigmas must have one value per joint")
    out = np.zeros(len(a), np.float64)
    rc = _lib.load().hrn_pose_nms_oks_row(len(a), int(k.shape[1]), 0, k.ctypes.data, a.ctypes.data, int(g), _nan_if_none(in_vis_thre),
                                          None if sg is None else sg.ctypes.data, out.ctypes.data)
    if rc:
        raise ValueError("hrn_pose_nms_oks_row: bad arguments")
    return out


def _host(x, dtype) -> np.ndarray:
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=dtype)


def nms_eval(preds, maxvals, areas, box_scores, image_index, oks_thre=0.9, in_vis_thre=0.2, soft=False, sigmas=None, solve=None):
    """The rescoring and OKS NMS of ``evaluate_overall_accuracy`` (``datasets/COCO.py:353-382``) for a whole evaluation set, one
    problem per image: the host form of ``NativeHRNet.nms_eval`` (same arguments and result; it passes its device call as
    ``solve``, which takes ``pose_nms``'s COCO-layout arguments in order and returns its dict)."""
    if solve is None:
        def solve(kpts, areas, scores, counts, thresh, vis, rescore, soft, sigmas):
            return pose_nms(kpts=kpts, areas=areas, scores=scores, counts=counts, thresh=thresh, in_vis_thre=vis, rescore_thre=rescore,
                            soft=soft, sigmas=sigmas)
    preds, maxvals = _host(preds, np.float64), _host(maxvals, np.float64)
    total = len(preds)
    if preds.ndim != 3 or preds.shape[2] != 2 or maxvals.size != total * preds.shape[1]:
        raise ValueError("preds must be (N, J, 2) and maxvals (N, J) or (N, J, 1), got %s, %s" % (preds.shape, maxvals.shape))
    image_index = np.asarray(image_index).reshape(-1)
    areas = np.asarray(areas, dtype=np.float64).reshape(-1)
    box_scores = np.asarray(box_scores, dtype=np.float64).reshape(-1)
    if not (len(image_index) == len(areas) == len(box_scores) == total):
        raise ValueError("areas, box_scores and image_index must hold one value per person")
    order = np.argsort(image_index, kind="stable")
    images, counts = np.unique(image_index, return_counts=True)
    kpts = np.ascontiguousarray(np.concatenate([preds, maxvals.reshape(total, -1, 1)], axis=2)[order])
    res = solve(kpts, np.ascontiguousarray(areas[order]), np.ascontiguousarray(box_scores[order]), counts, oks_thre, None, in_vis_thre,
                soft, sigmas)
    scores = np.empty(total, np.float64)
    scores[order] = res["scores"]
    by_image, first = {}, 0
    for image, count, num in zip(images.tolist(), counts.tolist(), res["num"].tolist()):
        members = order[first:first + count]
        by_image[image] = members[res["keep"][first:first + num]] if num else members
        first += count
    seen = dict.fromkeys(image_index.tolist())
    return scores, {image: by_image[image] for image in seen}


# -- COCO keypoint AP / AR (csrc/keypoint_eval_math.h) ---------------------------------------------------------------------------------
EVAL_MAX_DET, EVAL_AREAS, EVAL_THRS, EVAL_RECS = 20, 3, 10, 101
# the ten statistics as datasets/COCO.py:582 spells them
EVAL_STAT_NAMES = ("AP", "Ap .5", "AP .75", "AP (M)", "AP (L)", "AR", "AR .5", "AR .75", "AR (M)", "AR (L)")


def keypoint_eval_constants():
    """``(iouThrs (10,), recThrs (101,), area ranges (3, 2))`` as the library holds them (``hrn_keypoint_eval_constants``)"""
    iou, rec, areas = np.zeros(EVAL_THRS), np.zeros(EVAL_RECS), np.zeros((EVAL_AREAS, 2))
    if _lib.load().hrn_keypoint_eval_constants(iou.ctypes.data, rec.ctypes.data, areas.ctypes.data):
        raise ValueError("hrn_keypoint_eval_constants: bad arguments")
    return iou, rec, areas


def keypoint_eval_groups(dt_image, gt_image):
    """Both sides of an evaluation grouped by image id on the host: ``(images, dt_order, gt_order, dt_start, gt_start, slots)``.
    ``images``: the union of the ids of both sides, ascending; ``*_order``: a stable sort of each side by id (None where the side
    already is in that order); ``*_start`` (P + 1,) int32: where each image's members start in the sorted side; ``slots``: the sum
    over the images of min(detections, 20)."""
    dt_image, gt_image = np.asarray(dt_image, dtype=np.int64).reshape(-1), np.asarray(gt_image, dtype=np.int64).reshape(-1)
    images = np.union1d(dt_image, gt_image)
    sides = []
    for ids in (dt_image, gt_image):
        order = np.argsort(ids, kind="stable")
        start = np.append(np.searchsorted(ids[order], images, side="left"), len(ids)).astype(np.int32)
        sides.append((None if np.array_equal(order, np.arange(len(ids))) else order.astype(np.int32), start))
    slots = int(np.minimum(np.diff(sides[0][1]), EVAL_MAX_DET).sum())
    return images, sides[0][0], sides[1][0], sides[0][1], sides[1][1], slots


def keypoint_eval_joints(dt_shape, gt_shape, sigmas) -> int:
    """J of an evaluation call from the (n, J, 3) shapes of its keypoints (an empty side has no say), else from ``sigmas``, else 17"""
    for shape in (tuple(dt_shape), tuple(gt_shape)):
        if len(shape) == 3 and shape[0] > 0:
            if shape[2] != 3:
                raise ValueError("keypoints must be (n, J, 3), got %s" % (shape,))
            return int(shape[1])
    return 17 if sigmas is None else len(sigmas)


def keypoint_eval(dt_kpts, dt_scores, dt_image, gt_kpts, gt_area, gt_bbox, gt_iscrowd, gt_image, sigmas=None):
    """COCO keypoint AP / AR of an evaluation set in one native call (``hrn_keypoint_eval``, no GPU): the host form of
    ``NativeHRNet.keypoint_eval``, equal to it bit for bit.  What pycocotools' ``COCOeval(gt, dt, 'keypoints')`` computes for one
    category with ``maxDets = 20``, as DEFINED in ``csrc/keypoint_eval_math.h`` (parity with pycocotools is not pinned).

    ``dt_kpts`` (N, J, 3) ``(x, y, score)``, ``dt_scores`` (N,), ``dt_image`` (N,) integer image ids; ``gt_kpts`` (M, J, 3)
    ``(x, y, v)``, ``gt_area`` (M,), ``gt_bbox`` (M, 4) ``(x, y, w, h)``, ``gt_iscrowd`` (M,), ``gt_image`` (M,).  Any order: both
    sides are grouped by image id (a stable sort; the images are the union of both sides' ids, ascending).  ``sigmas``: J values,
    or None for COCO's 17.  At most 256 detections and 256 people per image.

    Returns a dict: ``stats`` (10,) in ``EVAL_STAT_NAMES``' order; ``precision`` (3, 10, 101) and ``recall`` (3, 10) over (area
    range all / medium / large, OKS threshold, recall threshold), -1 where a range has no counted ground truth; per slot (each
    image's up to 20 best detections, images in order) ``slot_person`` (S,) int32 -- the index into the caller's detections --
    ``slot_score`` (S,), ``dt_match`` (3, 10, S) int32 -- the index into the caller's ground truth or -1 -- and ``dt_ignore``
    (3, 10, S) uint8; ``npig`` (P, 3) int32; ``status`` (P,) int32 -- bit 0: a NaN score was ordered last, bit 1: a non-finite OKS
    counted as 0; ``images`` (P,) int64."""
    images, dt_order, gt_order, dt_start, gt_start, slots = keypoint_eval_groups(dt_image, gt_image)
    total, people, problems = int(dt_start[-1]), int(gt_start[-1]), len(images)
    joints = keypoint_eval_joints(np.shape(dt_kpts), np.shape(gt_kpts), sigmas)
    sg = None if sigmas is None else np.ascontiguousarray(sigmas, dtype=np.float64).reshape(-1)
    if sg is not None and len(sg) != joints:
        raise ValueError("sigmas must have one value per joint")

    def side(x, dtype, shape, order):
        x = np.asarray(x, dtype=dtype).reshape(shape)
        return np.ascontiguousarray(x if order is None else x[order])

    dk, ds = side(dt_kpts, np.float64, (total, joints, 3), dt_order), side(dt_scores, np.float64, (total,), dt_order)
    gk, ga = side(gt_kpts, np.float64, (people, joints, 3), gt_order), side(gt_area, np.float64, (people,), gt_order)
    gb, gc = side(gt_bbox, np.float64, (people, 4), gt_order), side(gt_iscrowd, np.int32, (people,), gt_order)
    out = dict(stats=np.zeros(10), precision=np.zeros((EVAL_AREAS, EVAL_THRS, EVAL_RECS)), recall=np.zeros((EVAL_AREAS, EVAL_THRS)),
               slot_person=np.zeros(slots, np.int32), slot_score=np.zeros(slots), dt_match=np.zeros((EVAL_AREAS, EVAL_THRS, slots), np.int32),
               dt_ignore=np.zeros((EVAL_AREAS, EVAL_THRS, slots), np.uint8), npig=np.zeros((problems, EVAL_AREAS), np.int32),
               status=np.zeros(problems, np.int32))
    lib = _lib.load()
    rc = lib.hrn_keypoint_eval(problems, dt_start.ctypes.data, gt_start.ctypes.data, joints, dk.ctypes.data, ds.ctypes.data, gk.ctypes.data,
                               ga.ctypes.data, gb.ctypes.data, gc.ctypes.data, None if sg is None else sg.ctypes.data,
                               *[out[k].ctypes.data for k in ("stats", "precision", "recall", "slot_person", "slot_score", "dt_match",
                                                              "dt_ignore", "npig", "status")])
    if rc:
        raise ValueError("hrn_keypoint_eval: " + lib.hrn_keypoint_eval_last_error().decode())
    if dt_order is not None:
        out["slot_person"] = dt_order[out["slot_person"]]
    if gt_order is not None:
        out["dt_match"] = np.where(out["dt_match"] >= 0, gt_order[np.maximum(out["dt_match"], 0)], -1).astype(np.int32)
    out["images"] = images
    return out


def keypoint_eval_oks(dt_kpts, gt_kpts, gt_area, gt_bbox, sigmas=None) -> np.ndarray:
    """The OKS of every (detection, person) pair of one image, (n_d, n_g), as ``keypoint_eval`` computes it
    (``hrn_keypoint_eval_oks``, no GPU): what COCOeval's ``computeOks`` returns, in keypoint_eval_math.h's arithmetic."""
    dk, gk = np.ascontiguousarray(dt_kpts, dtype=np.float64), np.ascontiguousarray(gt_kpts, dtype=np.float64)
    ga, gb = np.ascontiguousarray(gt_area, dtype=np.float64).reshape(-1), np.ascontiguousarray(gt_bbox, dtype=np.float64).reshape(-1, 4)
    if dk.ndim != 3 or gk.ndim != 3 or dk.shape[1:] != gk.shape[1:] or dk.shape[2] != 3 or len(ga) != len(gk) or len(gb) != len(gk):
        raise ValueError("keypoints must be (n_d, J, 3) and (n_g, J, 3) beside n_g areas and boxes")
    sg = None if sigmas is None else np.ascontiguousarray(sigmas, dtype=np.float64).reshape(-1)
    if sg is not None and len(sg) != dk.shape[1]:
        raise ValueError("sigmas must have one value per joint")
    out = np.zeros((len(dk), len(gk)), np.float64)
    if _lib.load().hrn_keypoint_eval_oks(len(dk), len(gk), int(dk.shape[1]), dk.ctypes.data, gk.ctypes.data, ga.ctypes.data, gb.ctypes.data,
                                         None if sg is None else sg.ctypes.data, out.ctypes.data):
        raise ValueError("hrn_keypoint_eval_oks: bad arguments")
    return out


def eval_detections(preds, maxvals, scores, kept):
    """What ``_coco_keypoint_results_one_category_kernel`` writes to the result file (``datasets/COCO.py:551-564``) for the people
    ``nms_eval`` kept: ``(dt_kpts (n, J, 3), dt_scores (n,), dt_image (n,))``, keypoints and scores rounded through float32, the
    people of each image best first."""
    preds, maxvals = _host(preds, np.float64), _host(maxvals, np.float64)
    index = np.concatenate([np.asarray(v, dtype=np.int64) for v in kept.values()]) if kept else np.zeros(0, np.int64)
    image = np.concatenate([np.full(len(v), k, np.int64) for k, v in kept.items()]) if kept else np.zeros(0, np.int64)
    kpts = np.concatenate([preds, maxvals.reshape(len(preds), -1, 1)], axis=2)[index]
    return kpts.astype(np.float32).astype(np.float64), np.asarray(scores)[index].astype(np.float32).astype(np.float64), image


def evaluate_overall_accuracy(preds, maxvals, areas, box_scores, image_index, gt_kpts, gt_area, gt_bbox, gt_iscrowd, gt_image,
                              oks_thre=0.9, in_vis_thre=0.2, soft=False, sigmas=None, nms=None, evaluate=None):
    """``evaluate_overall_accuracy`` of the reference's COCO dataset (``datasets/COCO.py:353-388``) from arrays: rescoring and OKS
    NMS (``nms_eval``), the float32 rounding of the result file (``eval_detections``), then the keypoint evaluation
    (``keypoint_eval``).  Returns ``(OrderedDict of the ten statistics by EVAL_STAT_NAMES, AP)``.  The host form of
    ``NativeHRNet.evaluate_overall_accuracy``, which passes its device calls as ``nms`` / ``evaluate``."""
    from collections import OrderedDict

    scores, kept = (nms or nms_eval)(preds, maxvals, areas, box_scores, image_index, oks_thre, in_vis_thre, soft, sigmas)
    dt_kpts, dt_scores, dt_image = eval_detections(preds, maxvals, scores, kept)
    out = (evaluate or keypoint_eval)(dt_kpts, dt_scores, dt_image, gt_kpts, gt_area, gt_bbox, gt_iscrowd, gt_image, sigmas)
    stats = _host(out["stats"], np.float64)
    name_value = OrderedDict((name, float(v)) for name, v in zip(EVAL_STAT_NAMES, stats))
    return name_value, name_value["AP"]


def inverse_affine(center, scale, pixel_std, output_size) -> np.ndarray:
    """The 2x3 matrix ``get_affine_transform(center, scale, pixel_std, 0, output_size, inv=1)`` returns
    (``misc/utils.py:44-76``): heat-map coordinates back to image coordinates for an unrotated crop.  The reference builds
    three float32 point pairs and lets ``cv2.getAffineTransform`` solve for the matrix in float64; the same pairs are built
    here with the same float32 roundings and the 6x6 system is solved by LU in float64 (``numpy.linalg.solve``)."""
    scale = np.asarray(scale)
    if scale.ndim == 0:
        scale = np.array([scale, scale])
    scale_tmp = scale * 1.0 * pixel_std
    src_w, dst_w, dst_h = scale_tmp[0], output_size[0], output_size[1]
    shift = np.array([0, 0], dtype=np.float32)
    src, dst = np.zeros((3, 2), dtype=np.float32), np.zeros((3, 2), dtype=np.float32)
    src[0, :] = center + scale_tmp * shift
    src[1, :] = center + [0 * 1.0 - (src_w * -0.5) * 0.0, 0 * 0.0 + (src_w * -0.5) * 1.0] + scale_tmp * shift   # get_dir, rot = 0
    dst[0, :] = [dst_w * 0.5, dst_h * 0.5]
    dst[1, :] = np.array([dst_w * 0.5, dst_h * 0.5]) + np.array([0, dst_w * -0.5], np.float32)
    for pts in (src, dst):                                   # get_3rd_point: b + (-(a - b).y, (a - b).x)
        direct = pts[0, :] - pts[1, :]
        pts[2, :] = pts[1, :] + np.array([-direct[1], direct[0]], dtype=np.float32)
    a = np.zeros((6, 6), np.float64)
    b = np.zeros(6, np.float64)
    for k in range(3):                                       # dst -> src (inv = 1)
        a[2 * k, 0:3] = (dst[k, 0], dst[k, 1], 1.0)
        a[2 * k + 1, 3:6] = (dst[k, 0], dst[k, 1], 1.0)
        b[2 * k], b[2 * k + 1] = src[k, 0], src[k, 1]
    return np.linalg.solve(a, b).reshape(2, 3)


def _solve_affine(frm: np.ndarray, to: np.ndarray) -> np.ndarray:
    """what ``cv2.getAffineTransform(frm, to)`` solves, three float32 point pairs -> the 2x3 float64 matrix: the same 6x6
    system, the same LU solve as ``inverse_affine``"""
    a = np.zeros((6, 6), np.float64)
    b = np.zeros(6, np.float64)
    for k in range(3):
        a[2 * k, 0:3] = (frm[k, 0], frm[k, 1], 1.0)
        a[2 * k + 1, 3:6] = (frm[k, 0], frm[k, 1], 1.0)
        b[2 * k], b[2 * k + 1] = to[k, 0], to[k, 1]
    return np.linalg.solve(a, b).reshape(2, 3)


def affine_matrix(center, scale, pixel_std, rot, output_size, inv=0) -> np.ndarray:
    """``get_affine_transform(center, scale, pixel_std, rot, output_size, inv=inv)`` in full (``misc/utils.py:46-96``): the
    2x3 float64 matrix that takes image coordinates to crop coordinates (``inv=0``: what ``cv2.warpAffine`` /
    ``NativeHRNet.warp_crops`` are given) or back (``inv=1``).  ``rot`` in degrees; ``output_size`` = (width, height).
    The three point pairs are built as the reference builds them -- ``get_dir`` in float64 ``sin`` / ``cos``, then the float32
    point arrays -- and ``cv2.getAffineTransform`` is replaced by the float64 solve ``inverse_affine`` uses: for ``rot = 0``,
    ``inv = 1`` the two functions return the same bits."""
    scale = np.asarray(scale)
    if scale.ndim == 0:
        scale = np.array([scale, scale])
    scale_tmp = scale * 1.0 * pixel_std
    src_w, dst_w, dst_h = scale_tmp[0], output_size[0], output_size[1]
    shift = np.array([0, 0], dtype=np.float32)
    rot_rad = np.pi * rot / 180
    sn, cs = np.sin(rot_rad), np.cos(rot_rad)                # get_dir([0, src_w * -0.5], rot_rad)
    src_point = [0, src_w * -0.5]
    src_dir = [src_point[0] * cs - src_point[1] * sn, src_point[0] * sn + src_point[1] * cs]
    dst_dir = np.array([0, dst_w * -0.5], np.float32)
    src, dst = np.zeros((3, 2), dtype=np.float32), np.zeros((3, 2), dtype=np.float32)
    src[0, :] = center + scale_tmp * shift
    src[1, :] = center + src_dir + scale_tmp * shift
    dst[0, :] = [dst_w * 0.5, dst_h * 0.5]
    dst[1, :] = np.array([dst_w * 0.5, dst_h * 0.5]) + dst_dir
    for pts in (src, dst):                                   # get_3rd_point: b + (-(a - b).y, (a - b).x)
        direct = pts[0, :] - pts[1, :]
        pts[2, :] = pts[1, :] + np.array([-direct[1], direct[0]], dtype=np.float32)
    return _solve_affine(dst, src) if inv else _solve_affine(src, dst)


def box_to_center_scale(box_xywh, aspect_ratio, pixel_std=200):
    """``_box2cs`` / ``_xywh2cs`` (``datasets/COCO.py:394-413``): an ``(x, y, w, h)`` box -> ``(center (2,), scale (2,))``
    float32, the box grown to ``aspect_ratio`` = crop width / crop height about its centre, in units of ``pixel_std`` pixels,
    with the reference's 1.25 margin (applied unless ``center[0] == -1``)."""
    x, y, w, h = box_xywh[:4]
    center = np.zeros((2,), dtype=np.float32)
    center[0] = x + w * 0.5
    center[1] = y + h * 0.5
    if w > aspect_ratio * h:
        h = w * 1.0 / aspect_ratio
    elif w < aspect_ratio * h:
        w = h * aspect_ratio
    scale = np.array([w * 1.0 / pixel_std, h * 1.0 / pixel_std], dtype=np.float32)
    if center[0] != -1:
        scale = scale * 1.25
    return center, scale


def transform_preds(coords, center, scale, pixel_std, output_size) -> np.ndarray:
    """``misc/utils.py:116-123``: (J, 2) heat-map coordinates of one crop -> image coordinates, float32.  With the
    ``preds`` of ``NativeHRNet.predict_flip_tta`` this completes ``get_final_preds`` (``misc/utils.py:154-180``)."""
    coords = np.asarray(coords.detach().cpu().numpy() if hasattr(coords, "detach") else coords)
    target = np.zeros(coords.shape, dtype=np.float32)
    trans = inverse_affine(center, scale, pixel_std, output_size)
    for p in range(coords.shape[0]):
        target[p, 0:2] = np.dot(trans, np.array([coords[p, 0], coords[p, 1], 1.]).T)[:2]
    return target


def final_preds(preds, center, scale, pixel_std, heatmap_size) -> np.ndarray:
    """the "Transform back" loop of ``get_final_preds`` (``misc/utils.py:176-178``) over a batch: preds (n, J, 2) in heat-map
    pixels (x, y), center / scale (n, 2) as the dataset provides them, heatmap_size = (width, height)."""
    preds = np.asarray(preds.detach().cpu().numpy() if hasattr(preds, "detach") else preds)
    out = np.empty(preds.shape, np.float32)
    for i in range(preds.shape[0]):
        out[i] = transform_preds(preds[i], center[i], scale[i], pixel_std, heatmap_size)
    return out


def joints_to_crop(joints_image, visibility, matrices) -> np.ndarray:
    """``affine_transform`` (``misc/utils.py:78-81``) of every visible ground-truth joint by its person's forward matrix
    (``affine_matrix(..., inv=0)``, image -> crop), as ``datasets/COCO.py:298-300`` does before ``_generate_target``:
    ``joints_image`` (n, J, 2) in image pixels, ``visibility`` (n, J) or (n, J, k) (column 0 is read), ``matrices`` (n, 2, 3).
    Returns (n, J, 2) float64; a joint whose visibility is not > 0 is left as it is."""
    jt = np.array(joints_image, dtype=np.float64)
    vis = np.asarray(visibility)
    if vis.ndim == 3:
        vis = vis[:, :, 0]
    m = np.asarray(matrices, dtype=np.float64)
    if jt.ndim != 3 or jt.shape[2] < 2 or vis.shape != jt.shape[:2] or m.shape != (jt.shape[0], 2, 3):
        raise ValueError("joints_image must be (n, J, 2), visibility (n, J) or (n, J, k), matrices (n, 2, 3): got %s, %s, %s"
                         % (jt.shape, vis.shape, m.shape))
    jt = np.ascontiguousarray(jt[:, :, :2])
    for i in range(jt.shape[0]):
        for j in range(jt.shape[1]):
            if vis[i, j] > 0.:
                jt[i, j] = np.dot(m[i], np.array([jt[i, j, 0], jt[i, j, 1], 1.]).T)[:2]
    return jt


def target_centers(joints, visibility, resolution, sigma=2, joints_weight=None):
    """The host half of ``_generate_target`` (``datasets/COCO.py:466-488, 512-513``; ``hrn_target_centers``, no GPU): ``joints``
    (n, J, 2) in crop pixels, ``visibility`` (n, J), ``resolution`` = (height, width) of the crop.  Returns ``(mu (n, J, 2) int32
    = (x, y) in heat-map cells, weight (n, J) float32 before joints_weight, target_weight (n, J) float32)``."""
    import ctypes

    from . import _lib

    jt = np.ascontiguousarray(np.asarray(joints, dtype=np.float64))
    vis = np.ascontiguousarray(np.asarray(visibility, dtype=np.float32))
    if jt.ndim != 3 or jt.shape[2] != 2 or vis.shape != jt.shape[:2]:
        raise ValueError("joints must be (n, J, 2) and visibility (n, J), got %s and %s" % (jt.shape, vis.shape))
    n, J = vis.shape
    jw = None if joints_weight is None else np.ascontiguousarray(np.asarray(joints_weight, dtype=np.float32).reshape(-1))
    if jw is not None and jw.shape != (J,):
        raise ValueError("joints_weight must hold %d values" % J)
    mu, draw, tw = np.empty((n, J, 2), np.int32), np.empty((n, J), np.float32), np.empty((n, J), np.float32)
    lib = _lib.load()
    rc = lib.hrn_target_centers(jt.ctypes.data, vis.ctypes.data, None if jw is None else jw.ctypes.data, n, J, int(resolution[0]),
                                int(resolution[1]), ctypes.c_double(float(sigma)), mu.ctypes.data, draw.ctypes.data, tw.ctypes.data)
    if rc != 0:
        raise ValueError(lib.hrn_last_error(None).decode())
    return mu, draw, tw


def _frame_sizes(frame_hw, n: int):
    """``frame_hw`` of ``pose_boxes`` / ``NativeHRNet.boxes_from_poses`` as a contiguous int32 array and its per-person flag: one
    (height, width) for everybody, or (n, 2)"""
    hw = np.ascontiguousarray(np.asarray(frame_hw, dtype=np.int32))
    if hw.shape == (2,):
        hw = hw.reshape(1, 2)
    if hw.ndim != 2 or hw.shape[1] != 2 or len(hw) not in (1, n):
        raise ValueError("frame_hw must be (height, width) or (n, 2), got %s for %d people" % (hw.shape, n))
    return hw, int(len(hw) == n and n > 1)


def pose_boxes(pts, frame_hw, threshold: float = 0.5, min_joints: int = 3, scale: float = 1.25, min_side: float = 0.0) -> np.ndarray:
    """A detection-shaped box around each person's joints, on the host (``hrn_pose_boxes``, no GPU): what a tracker cuts the next
    frame's crop from between two detector runs.  ``pts`` (n, J, 3) float32 ``(y, x, confidence)``; ``frame_hw`` = (height, width)
    for everybody or (n, 2).  Returns (n, 5) float32 rows ``(x1, y1, x2, y2, score)``: the extent of the joints with
    ``confidence > threshold`` grown by ``scale`` about its centre, at least ``min_side`` long, cut to the frame; ``score`` is their
    mean confidence; five zeros where fewer than ``min_joints`` are live (include/hrnet_mi355.h has the definition, to the bit;
    ``NativeHRNet.boxes_from_poses`` is the same on the GPU)."""
    import ctypes

    from . import _lib

    p = np.ascontiguousarray(np.asarray(pts, dtype=np.float32))
    if p.ndim != 3 or p.shape[2] != 3:
        raise ValueError("pts must be (n, J, 3), got %s" % (p.shape,))
    n, J = p.shape[:2]
    hw, per_person = _frame_sizes(frame_hw, n)
    out = np.empty((n, 5), np.float32)
    lib = _lib.load()
    rc = lib.hrn_pose_boxes(p.ctypes.data, n, J, hw.ctypes.data, per_person, ctypes.c_float(threshold), int(min_joints),
                            ctypes.c_double(scale), ctypes.c_double(min_side), out.ctypes.data)
    if rc != 0:
        raise ValueError("hrn_pose_boxes: " + lib.hrn_pose_boxes_last_error().decode())
    return out


# -- person labels on the host: the record of one person and what it puts on a pixel ------------------------------------------------
def label_layout(box, person_id=None, score=None, scale: int = 1, thickness: int = 2):
    """The label of one person as ``NativeHRNet.draw_labels`` builds it on the device (``hrn_label_layout``, no GPU): a
    ``_lib.LabelRecordC`` with the outline rectangle, the plate rectangle and the cells (``ncells``; cell k = four bits at 4 k of
    ``cells_hi : cells_lo``, 0..9 a digit, 15 a blank).  ``box`` = (x1, y1, x2, y2) integers; ``person_id`` / ``score``: None = not
    given; ``scale`` in [1, 16], ``thickness`` in [0, 16].  include/hrnet_mi355.h has the definition."""
    import ctypes

    from . import _lib

    b = np.ascontiguousarray(np.asarray(box, dtype=np.int32).reshape(-1))
    if b.shape != (4,):
        raise ValueError("box must be (x1, y1, x2, y2)")
    lib = _lib.load()
    rec = _lib.LabelRecordC()
    rc = lib.hrn_label_layout(b.ctypes.data, int(person_id is not None), 0 if person_id is None else int(person_id),
                              int(score is not None), ctypes.c_float(0.0 if score is None else score), int(scale), int(thickness),
                              ctypes.byref(rec))
    if rc != 0:
        raise ValueError("hrn_label_layout: " + lib.hrn_label_last_error().decode())
    return rec


def label_covers(record, px: int, py: int) -> int:
    """What the label ``record`` (of ``label_layout``) puts on pixel (px, py): 0 nothing, 1 the person's colour (plate or outline),
    2 the person's text colour (ink) -- ``hrn_label_covers``, the function the rasteriser compiles."""
    import ctypes

    from . import _lib

    lib = _lib.load()
    rc = lib.hrn_label_covers(ctypes.byref(record), int(px), int(py))
    if rc not in (0, 1, 2):
        raise ValueError("hrn_label_covers: " + lib.hrn_label_last_error().decode())
    return rc


# -- heat-map overlays on the host: the quantised maps, and the whole definition on the CPU ---------------------------------------
def heatmap_quantise(heatmaps, joints=None, vmin: float = 0.0, vmax: float = 1.0) -> np.ndarray:
    """Step 1 of ``NativeHRNet.draw_heatmaps`` on the host (``hrn_heatmap_quantise``, no GPU): the maximum of every person's
    (n, J, h, w) float32 maps over ``joints`` (indices; default all), quantised to (n, h, w) uint8 -- ``vmin`` -> 0, ``vmax`` ->
    255, NaN -> 0.  include/hrnet_mi355.h has the definition."""
    import ctypes

    from . import _lib
    from .native import heat_arguments

    maps = np.ascontiguousarray(np.asarray(heatmaps, dtype=np.float32))
    if maps.ndim == 3:
        maps = maps[None]
    if maps.ndim != 4:
        raise ValueError("heatmaps must be (J, h, w) or (n, J, h, w)")
    n, J, hq, wq = maps.shape
    mask = heat_arguments(J, joints, "gray", 0, "const", vmin, vmax, 1)[0] if joints is not None else None
    out = np.empty((n, hq, wq), np.uint8)
    lib = _lib.load()
    rc = lib.hrn_heatmap_quantise(maps.ctypes.data, n, J, hq, wq, None if mask is None else mask.ctypes.data, ctypes.c_float(vmin),
                                  ctypes.c_float(vmax), out.ctypes.data)
    if rc != 0:
        raise ValueError("hrn_heatmap_quantise: " + lib.hrn_heatmap_last_error().decode())
    return out


def draw_heatmaps(frames, heatmaps, boxes, frame_index=None, joints=None, colormap="jet", alpha=0.6, alpha_mode: str = "value",
                  vmin: float = 0.0, vmax: float = 1.0, cutoff=0.1, matrix=None, range=None):  # noqa: A002
    """``NativeHRNet.draw_heatmaps`` on the host (``hrn_draw_heatmaps_host``, no GPU): the same arguments, the same bytes.
    ``frames``: (H, W, 3) uint8 BGR arrays (rows may be strided) or host ``YuvFrame``s, one or a list (None: nobody is on it);
    they are drawn IN PLACE and returned.  ``heatmaps`` (n, J, h, w) float32 and ``boxes`` (n, 4) integers are host arrays."""
    import ctypes

    import torch

    from . import _lib
    from .frames import Frames
    from .native import heat_arguments
    from .palettes import bgr_to_yuv_colors

    single = not isinstance(frames, (list, tuple))
    items = [frames] if single else list(frames)
    if not items:
        raise ValueError("draw_heatmaps needs at least one frame")
    canvases = Frames.canvases(items, torch.device("cpu"))
    table = canvases.table(kind=_lib.CanvasC)
    maps = np.ascontiguousarray(np.asarray(heatmaps, dtype=np.float32))
    if maps.ndim == 3:
        maps = maps[None]
    if maps.ndim != 4 or min(maps.shape[1:]) < 1:
        raise ValueError("heatmaps must be (J, h, w) or (n, J, h, w)")
    n, J, hq, wq = maps.shape
    b = np.asarray(boxes)
    if b.dtype.kind not in "iu":
        raise ValueError("boxes must be integers (the int32 boxes predict_frame / PersonTracker.update return)")
    b = np.ascontiguousarray(b.reshape(-1, 4), dtype=np.int32)
    if len(b) != n:
        raise ValueError("boxes must be (n, 4) (x1, y1, x2, y2), one row per person: %d for %d people" % (len(b), n))
    fi = None
    if frame_index is not None:
        fi = np.ascontiguousarray(np.asarray(frame_index, dtype=np.int32).reshape(-1))
        if len(fi) != n:
            raise ValueError("frame_index must have one entry per person: %d for %d people" % (len(fi), n))
    elif len(items) != 1:
        raise ValueError("several frames need frame_index: which frame each person is drawn on")
    mask, lut, a, mode, lo, hi, cut = heat_arguments(J, joints, colormap, alpha, alpha_mode, vmin, vmax, cutoff)
    if canvases.yuv:
        spaces = {(matrix or f.matrix, range or f.range) for f in canvases if f is not None}
        if len(spaces) != 1:
            raise ValueError("the YuvFrames of one draw_heatmaps call share one matrix and range (the table is converted once)")
        (matrix_, range_), = spaces
        lut = bgr_to_yuv_colors(lut, matrix_, range_)
    lib = _lib.load()
    rc = lib.hrn_draw_heatmaps_host(table, len(items), maps.ctypes.data if n else None, b.ctypes.data if n else None, n, J, hq, wq,
                                    None if fi is None else fi.ctypes.data, None if mask is None else mask.ctypes.data,
                                    ctypes.c_float(lo), ctypes.c_float(hi), lut.ctypes.data, a, mode, cut)
    if rc != 0:
        raise ValueError("hrn_draw_heatmaps_host: " + lib.hrn_heatmap_last_error().decode())
    return items[0] if single else items


# -- the face mosaic on the host: everybody's region, and the whole definition on the CPU -------------------------------------------
def _mosaic_people(pts, boxes):
    """(pts (n, J, 3) float32 or None, boxes (n, 4) int32 or None, n, J or None) of exactly one source, host arrays"""
    if (pts is None) == (boxes is None):
        raise ValueError("mosaic takes pts or boxes: exactly one of them")
    if pts is not None:
        p = np.ascontiguousarray(np.asarray(pts, dtype=np.float32))
        if p.ndim == 2:
            p = p[None]
        if p.ndim != 3 or p.shape[2] != 3 or p.shape[1] < 1:
            raise ValueError("pts must be (J, 3) or (n, J, 3) (y, x, confidence)")
        return p, None, p.shape[0], p.shape[1]
    b = np.asarray(boxes)
    if b.dtype.kind not in "iu":
        raise ValueError("boxes must be integers (the int32 boxes predict_frame / PersonTracker.update return)")
    b = np.ascontiguousarray(b.reshape(-1, 4), dtype=np.int32)
    return None, b, len(b), None


def mosaic_regions(canvas_hw, pts=None, boxes=None, joints=None, confidence_threshold: float = 0.5, scale=(1, 1), min_half=None):
    """The rectangle ``NativeHRNet.mosaic`` hides of every person, on the host (``hrn_mosaic_regions``, no GPU): ``canvas_hw`` =
    (height, width) for everybody or (n, 2); the other arguments are ``mosaic``'s.  Returns ((n, 4) int32 ``(x1, y1, x2, y2)``
    clipped to the canvas, (n,) int32 status: 0 a region, 1 none -- no chosen joint counts, or a degenerate box --, 2 it lies
    outside the canvas); without status 0 the rectangle is four zeros.  include/hrnet_mi355.h has the definition."""
    import ctypes

    from . import _lib
    from .native import mosaic_arguments

    p, b, n, J = _mosaic_people(pts, boxes)
    hw = np.asarray(canvas_hw, dtype=np.int32).reshape(-1, 2)
    if len(hw) not in (1, n):
        raise ValueError("canvas_hw must be (height, width) or (n, 2), got %s for %d people" % (hw.shape, n))
    hw = np.ascontiguousarray(np.broadcast_to(hw, (n, 2)))
    idx, num, den, half, _ = mosaic_arguments(J, joints, scale, min_half, None)
    regions, status = np.zeros((n, 4), np.int32), np.zeros((n,), np.int32)
    lib = _lib.load()
    rc = lib.hrn_mosaic_regions(p.ctypes.data if p is not None and n else None, n, J or 0, None if idx is None else idx.ctypes.data,
                                0 if idx is None else len(idx), b.ctypes.data if b is not None and n else None, hw.ctypes.data,
                                ctypes.c_float(confidence_threshold), num, den, half, regions.ctypes.data, status.ctypes.data)
    if rc != 0:
        raise ValueError("hrn_mosaic_regions: " + lib.hrn_mosaic_last_error().decode())
    return regions, status


def mosaic(frames, pts=None, boxes=None, joints=None, frame_index=None, confidence_threshold: float = 0.5, scale=(1, 1), min_half=None,
           cell=None, return_status: bool = False):
    """``NativeHRNet.mosaic`` on the host (``hrn_mosaic_host``, no GPU): the same arguments, the same bytes.  ``frames``:
    (H, W, 3) uint8 BGR arrays (rows may be strided) or host ``YuvFrame``s, one or a list (None: nobody is on it); they are
    changed IN PLACE and returned.  ``pts`` (n, J, 3) float32 or ``boxes`` (n, 4) integers are host arrays.  ``return_status``: also
    the (n,) int32 status as a numpy array."""
    import ctypes

    import torch

    from . import _lib
    from .frames import Frames
    from .native import mosaic_arguments

    single = not isinstance(frames, (list, tuple))
    items = [frames] if single else list(frames)
    if not items:
        raise ValueError("mosaic needs at least one frame")
    p, b, n, J = _mosaic_people(pts, boxes)
    canvases = Frames.canvases(items, torch.device("cpu"))
    table = canvases.table(kind=_lib.CanvasC)
    fi = None
    if frame_index is not None:
        fi = np.ascontiguousarray(np.asarray(frame_index, dtype=np.int32).reshape(-1))
        if len(fi) != n:
            raise ValueError("frame_index must have one entry per person: %d for %d people" % (len(fi), n))
    elif len(items) != 1:
        raise ValueError("several frames need frame_index: which frame each person is on")
    idx, num, den, half, size = mosaic_arguments(J, joints, scale, min_half, cell)
    status = np.zeros((n,), np.int32)
    lib = _lib.load()
    rc = lib.hrn_mosaic_host(table, len(items), p.ctypes.data if p is not None and n else None, n, J or 0,
                             None if idx is None else idx.ctypes.data, 0 if idx is None else len(idx),
                             b.ctypes.data if b is not None and n else None, None if fi is None else fi.ctypes.data,
                             ctypes.c_float(confidence_threshold), num, den, half, size, status.ctypes.data if n else None)
    if rc != 0:
        raise ValueError("hrn_mosaic_host: " + lib.hrn_mosaic_last_error().decode())
    out = items[0] if single else items
    return (out, status) if return_status else out


# -- the detector link on the host: letterbox geometry and the detector's boxes back in frame coordinates -------------------------
LETTERBOX_RULES = {"yolov3": 0, "yolov5": 1}     # include/hrnet_mi355.h: HRN_LETTERBOX_MAX_SIDE / _MIN_RATIO
LETTERBOX_PAD = {"yolov3": 128, "yolov5": 114}   # the wrappers' border: 127.5 is 128 under cv2's round-half-even saturation
DET_STATUS = {0: "kept", 1: "below the threshold", 2: "other class", 5: "not finite"}


class LetterboxGeometry:
    """What ``letterbox_geometry`` / ``NativeHRNet.detector_input`` return and ``detections_to_frame`` takes: the geometry of
    ``n`` frames letterboxed to one output size.  ``style``, ``size`` = (out_h, out_w), ``frame_hw`` (n, 2) int32, and per frame the
    arrays ``new_w``, ``new_h``, ``left``, ``top`` (int32), ``right``, ``bottom`` (derived) and ``ratio``, ``dw``, ``dh`` (float64, the
    wrappers' values BEFORE rounding: YOLOv5's inverse uses those)."""

    def __init__(self, style: str, size, frame_hw: np.ndarray, table):
        self.style, self.rule, self.size = style, LETTERBOX_RULES[style], (int(size[0]), int(size[1]))
        self.frame_hw, self.table = frame_hw, table
        rows = [table[k] for k in range(len(frame_hw))]
        self.new_w, self.new_h = (np.asarray([getattr(r, f) for r in rows], np.int32) for f in ("new_w", "new_h"))
        self.left, self.top = (np.asarray([getattr(r, f) for r in rows], np.int32) for f in ("left", "top"))
        self.ratio, self.dw, self.dh = (np.asarray([getattr(r, f) for r in rows], np.float64) for f in ("ratio_w", "dw", "dh"))
        self.right, self.bottom = self.size[1] - self.left - self.new_w, self.size[0] - self.top - self.new_h

    def __len__(self):
        return len(self.frame_hw)


def _letterbox_size(size, style: str):
    if style not in LETTERBOX_RULES:
        raise ValueError("style must be 'yolov3' or 'yolov5', got %r" % (style,))
    out = (int(size), int(size)) if np.ndim(size) == 0 else (int(size[0]), int(size[1]))
    if style == "yolov3" and out[0] != out[1]:
        raise ValueError("the yolov3 letterbox is square, got %r" % (size,))
    return out


def letterbox_geometry(frame_hw, size, style: str = "yolov3") -> LetterboxGeometry:
    """The letterbox of frames of ``frame_hw`` = (height, width) or (n, 2) to ``size`` (an int, or (out_h, out_w) for ``"yolov5"``),
    on the host (``hrn_letterbox_geometry``, no GPU): ``style="yolov3"`` is ``letterbox(mode='square')`` of the reference's YOLOv3
    wrapper, ``"yolov5"`` its YOLOv5 wrapper's ``letterbox(auto=False, scaleFill=False)``.  ValueError where the resized frame would
    be empty (cv2.resize raises there)."""
    out = _letterbox_size(size, style)
    hw = np.ascontiguousarray(np.asarray(frame_hw, dtype=np.int32).reshape(-1, 2))
    table = (_lib.Letterbox * max(len(hw), 1))()
    lib = _lib.load()
    rc = lib.hrn_letterbox_geometry(LETTERBOX_RULES[style], hw.ctypes.data, len(hw), out[0], out[1], ctypes.addressof(table))
    if rc != 0:
        raise ValueError("hrn_letterbox_geometry: " + lib.hrn_letterbox_last_error().decode())
    return LetterboxGeometry(style, out, hw, table)


def detection_arguments(dets_shape, geometry: LetterboxGeometry, counts, conf_thres, classes, class_col, compact):
    """the host arguments ``detections_to_frame`` and ``NativeHRNet.detections_to_frame`` share: (start int32 (P + 1), threshold,
    class column, class ids int32, flags)"""
    if len(dets_shape) != 2 or dets_shape[1] < 5:
        raise ValueError("dets must be (n, >=5), got %s" % (tuple(dets_shape),))
    n, P = int(dets_shape[0]), len(geometry)
    if counts is None:
        if P != 1:
            raise ValueError("%d frames need counts (rows per frame)" % P)
        counts = [n]
    start = _segments(counts, n, "rows")
    if len(start) != P + 1:
        raise ValueError("counts has %d entries for %d frames" % (len(start) - 1, P))
    ids = np.ascontiguousarray(np.asarray([] if classes is None else classes, dtype=np.int32).reshape(-1))
    if len(ids) > 16:
        raise ValueError("at most 16 classes")
    col = int(dets_shape[1]) if classes is None else int(class_col)
    thres = float("-inf") if conf_thres is None else float(conf_thres)
    return start, thres, col, ids, 1 if compact else 0


def detections_to_frame(dets, geometry: LetterboxGeometry, counts=None, conf_thres=None, classes=None, compact=True, conf_col: int = 4,
                        class_col: int = -1):
    """A detector's rows from letterbox coordinates back to the frame, on the host (``hrn_detections_to_frame``, no GPU):
    ``filter_classes`` + ``scale_coords`` of the reference's YOLOv3 wrapper, or the confidence / class filter and
    ``(x - dw) / ratio`` of its YOLOv5 wrapper, selected by ``geometry.style``.

    ``dets`` (n, >=5) float32 rows ``x1, y1, x2, y2, confidence, ...`` after the detector's NMS; ``geometry`` from
    ``letterbox_geometry`` / ``detector_input``; ``counts``: rows per frame (one frame: may be None); ``conf_thres``: keep rows with
    ``row[conf_col] >= conf_thres`` in float32 (None: everybody); ``classes``: up to 16 accepted ids of column ``class_col``
    (negative: from the end; None: no class filter).  Returns ``(rows (n, stride) float32, counts (P,) int32, status (n,) int32)``:
    kept rows mapped (columns beyond the fourth unchanged), every other row zeros; ``compact`` moves the kept rows of each frame to
    the front of its segment in their order; ``status`` per input row: 0 kept, 1 below the threshold, 2 other class, 5 not finite."""
    d = np.ascontiguousarray(np.asarray(dets, dtype=np.float32))
    start, thres, col, ids, flags = detection_arguments(d.shape, geometry, counts, conf_thres, classes, class_col, compact)
    out, status = np.empty_like(d), np.empty((len(d),), np.int32)
    kept = np.empty((len(geometry),), np.int32)
    lib = _lib.load()
    rc = lib.hrn_detections_to_frame(geometry.rule, d.ctypes.data, int(d.shape[1]), start.ctypes.data, len(geometry),
                                     ctypes.addressof(geometry.table), geometry.frame_hw.ctypes.data, geometry.size[0], geometry.size[1],
                                     int(conf_col), ctypes.c_float(thres), col, ids.ctypes.data, len(ids), flags, out.ctypes.data,
                                     kept.ctypes.data, status.ctypes.data)
    if rc != 0:
        raise ValueError("hrn_detections_to_frame: " + lib.hrn_letterbox_last_error().decode())
    return out, kept, status


# -- detector NMS: the raw output of a YOLO head to kept rows, on the host ---------------------------------------------------------
DETECTOR_NMS_RULES = {"yolov3": 0, "yolov5": 1}   # include/hrnet_mi355.h: HRN_DNMS_YOLOV3 / _YOLOV5
DETECTOR_NMS_AGNOSTIC = 1                          # HRN_DNMS_AGNOSTIC
DETECTOR_NMS_DTYPES = {"float32": 0, "float16": 2}   # HRN_F32 / HRN_F16
DETECTOR_NMS_STATUS = {1: "more rows qualified than max_candidates", 2: "max_det reached with candidates left", 4: "a NaN key was dropped"}


def detector_nms_arguments(pred_shape, dtype_name: str, rule, max_det, max_candidates, agnostic):
    """the host arguments ``detector_nms`` and ``NativeHRNet.detector_nms`` share: (B, N, C, dtype code, rule code, flags, floats
    per output row).  The library judges the numbers; this judges the shapes and names."""
    if len(pred_shape) != 3 or pred_shape[2] < 6:
        raise ValueError("pred must be (B, N, 5 + C) with C >= 1, got %s" % (tuple(pred_shape),))
    if dtype_name not in DETECTOR_NMS_DTYPES:
        raise ValueError("pred must be float32 or float16, got %s" % dtype_name)
    if rule not in DETECTOR_NMS_RULES:
        raise ValueError("rule must be 'yolov3' or 'yolov5', got %r" % (rule,))
    code = DETECTOR_NMS_RULES[rule]
    return (int(pred_shape[0]), int(pred_shape[1]), int(pred_shape[2]) - 5, DETECTOR_NMS_DTYPES[dtype_name], code,
            DETECTOR_NMS_AGNOSTIC if agnostic else 0, 7 if code == 0 else 6)


def detector_nms(pred, rule, conf_thres, iou_thres, max_det: int = 300, max_candidates: int = 4096, agnostic: bool = False):
    """The detector's own non-maximum suppression on the host (``hrn_detector_nms``, no GPU): the raw ``(B, N, 5 + C)`` output of
    a YOLO head (rows ``cx, cy, w, h, obj, cls...``, float32 or float16) to kept rows -- the host form of
    ``NativeHRNet.detector_nms``, equal to it bit for bit.  ``rule``: ``"yolov5"`` (ultralytics' ``non_max_suppression`` with
    ``multi_label=False``: rows ``x1, y1, x2, y2, conf, class``) or ``"yolov3"`` (the YOLOv3 wrapper's, with its weighted merge:
    rows ``x1, y1, x2, y2, obj, class confidence, class``); include/hrnet_mi355.h states both in full.  ``agnostic``: boxes of
    different classes suppress one another.  At most ``max_candidates`` (<= 4096) rows per image take part, at most ``max_det``
    are kept.

    Returns ``(rows (B, max_det, 6 | 7) float32, counts (B,) int32, index (B, max_det) int32, status (B,) int32)``: the rows beyond
    an image's count are zeros, ``index`` is the row of ``pred`` a kept row came from (-1 beyond the count), ``status`` bit 0: more
    rows qualified than ``max_candidates``, bit 1: ``max_det`` was reached with candidates left, bit 2: a candidate with a NaN key
    was dropped."""
    p = np.asarray(pred)
    if p.dtype != np.float16:
        p = p.astype(np.float32, copy=False)
    p = np.ascontiguousarray(p)
    B, N, C, dtype, code, flags, F = detector_nms_arguments(p.shape, p.dtype.name, rule, max_det, max_candidates, agnostic)
    max_det, max_candidates = int(max_det), int(max_candidates)
    shape = (B, max(max_det, 0))
    rows, index = np.empty(shape + (F,), np.float32), np.empty(shape, np.int32)
    counts, status = np.empty((B,), np.int32), np.empty((B,), np.int32)
    lib = _lib.load()
    rc = lib.hrn_detector_nms(p.ctypes.data, dtype, B, N, C, code, flags, float(conf_thres), float(iou_thres), max_candidates, max_det,
                              rows.ctypes.data, index.ctypes.data, counts.ctypes.data, status.ctypes.data)
    if rc != 0:
        raise ValueError("hrn_detector_nms: " + lib.hrn_detector_nms_last_error().decode())
    return rows, counts, index, status


# -- people between a frame and its rotation, on the host ------------------------------------------------------------------------
def rotate_people_arguments(pts_shape, boxes_shape, frame_hw, rotation_code):
    """the host arguments ``rotate_people`` and ``NativeHRNet.rotate_people`` share: (n, J, frame sizes int32, their per-person flag,
    codes int32, their per-person flag)"""
    from .frames import rotation_codes

    if pts_shape is None and boxes_shape is None:
        raise ValueError("rotate_people needs pts, boxes or both")
    if pts_shape is not None and boxes_shape is not None and pts_shape[0] != boxes_shape[0]:
        raise ValueError("pts and boxes must describe the same people: %d and %d" % (pts_shape[0], boxes_shape[0]))
    n = int((pts_shape or boxes_shape)[0])
    J = int(pts_shape[1]) if pts_shape is not None else 1
    if frame_hw is None or rotation_code is None:
        raise ValueError("rotate_people needs frame_hw (the SOURCE frame's height and width) and rotation_code")
    hw, per_hw = _frame_sizes(frame_hw, n)
    one = np.ndim(rotation_code) == 0
    return n, J, hw, per_hw, rotation_codes(rotation_code, 1 if one else n), int(not one and n > 1)


def rotate_people(pts=None, boxes=None, frame_hw=None, rotation_code=None):
    """Joints and boxes of people between a frame and its ``cv2.rotate``-d form, on the host (``hrn_rotate_people``, no GPU).
    ``pts`` (n, J, 3) float32 ``(y, x, confidence)`` and / or ``boxes`` (n, 4) int32 half-open ``(x1, y1, x2, y2)``; ``frame_hw``:
    (height, width) of the SOURCE frame for everybody, or (n, 2); ``rotation_code``: 0 (90 degrees clockwise), 1 (180), 2 (90
    counter-clockwise), one or n.  A coordinate is one float32 subtraction or a copy; NaN and inf pass through; the all-zero box of
    a lost person stays all-zero (include/hrnet_mi355.h has the table).  Returns the rotated array -- ``(pts, boxes)`` when both
    were given.  There is no inverse flag: the way back is code ``2 - c`` with the ROTATED frame's (height, width)."""
    p = None if pts is None else np.ascontiguousarray(np.asarray(pts, dtype=np.float32))
    b = None if boxes is None else np.ascontiguousarray(np.asarray(boxes, dtype=np.int32))
    if p is not None and (p.ndim != 3 or p.shape[2] != 3):
        raise ValueError("pts must be (n, J, 3), got %s" % (p.shape,))
    if b is not None and (b.ndim != 2 or b.shape[1] != 4):
        raise ValueError("boxes must be (n, 4), got %s" % (b.shape,))
    n, J, hw, per_hw, codes, per_code = rotate_people_arguments(None if p is None else p.shape, None if b is None else b.shape, frame_hw,
                                                                 rotation_code)
    p_out, b_out = None if p is None else np.empty_like(p), None if b is None else np.empty_like(b)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    lib = _lib.load()
    rc = lib.hrn_rotate_people(n, J, hw.ctypes.data, per_hw, codes.ctypes.data, per_code, ptr(p), ptr(b), ptr(p_out), ptr(b_out))
    if rc != 0:
        raise ValueError("hrn_rotate_people: " + lib.hrn_rotate_people_last_error().decode())
    return p_out if b is None else b_out if p is None else (p_out, b_out)
