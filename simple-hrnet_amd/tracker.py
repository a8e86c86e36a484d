"""Person ids over a video: the state of the reference's demo loop (``scripts/live-demo.py:114-130``) kept where the joints are.

``PersonTracker`` holds the previous frame's boxes, joints and ids and ``next_id``; every ``update`` is one
``associate_people`` -- ``NativeHRNet.associate_people`` on the engine's GPU (one launch, no host read: the ids feed
``draw_poses`` from the device), or ``postproc.associate_people`` on the host when there is no engine.  With ``one_euro`` it
also holds the joints' filter state and follows every association with one ``filter_poses``: smoothed joints for the overlay,
predicted joints for the next frame's crops."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import postproc


class PersonTracker:
    """``net``: a ``NativeHRNet`` -- state and results are tensors on its GPU -- or None: numpy arrays on the host, the same numbers.
    ``pose_alpha``, ``similarity_threshold``, ``smoothing_alpha``: as ``find_person_id_associations``; the defaults are the demo's.

    ``update(boxes, pts, counts=None) -> (boxes, pts, ids)``: ``boxes`` (n, 4) int32 and ``pts`` (n, J, 3) float32 of this frame
    (``predict_frame`` / ``track_frame``); ``counts``: people per stream when several streams are tracked at once (the same
    number of streams in every update).  The arguments are left as they are; the returned ``boxes`` and ``pts`` (smoothed where
    matched) are the tracker's state until the next update -- read them, do not write to them.  The FIRST update follows the
    demo: ids ``arange(n)`` and ``next_id = n + 1`` per stream that has somebody (no kernel; a first frame without people leaves
    ``next_id`` at 0, as the demo does).  An update with nobody keeps ``next_id`` and stores empty arrays.  ``status`` holds the
    last association's status per stream (None before), ``next_id`` the counters; ``reset()`` forgets everything.
    Behind an update, on the frame: ``net.draw_poses(frame, pts, skeleton, person_ids=ids)``; ``net.draw_labels(frame, boxes, ids)``.

    ``one_euro``: None, or ``dict(min_cutoff, beta, d_cutoff, threshold, rate=30.0)`` (any subset; the rest are
    ``filter_poses``' defaults): every update is then followed by ONE ``filter_poses`` call whose state follows the people
    through that update's ``match`` (no ``match`` on the first update; with nobody present the state is emptied).  ``update``
    then returns the FILTERED joints, and ``predicted`` holds the joints expected ``lookahead`` seconds later -- for
    ``track_frame(frame, tracker.predicted)``.  ``dt``: seconds since the previous update (None: ``1 / rate``); ``lookahead``
    None: ``dt``.  What the tracker keeps for the next association stays the association's own output.  The prediction starts
    from the raw position; the filtered joints lag on steady motion, the filter's known trade (``beta``).  With ``one_euro=None``
    no filter call is made and every result is what it is without the option.

    ``max_lost``: None -- everything above, nothing else -- or a number: the tracker then owns a TRACK TABLE (``capacity`` slots per
    stream, at most 256) and every ``update``, the first included, is one ``track_people`` on it (``include/hrnet_mi355.h``
    states the update).  A person missing for up to ``max_lost`` updates returns with their id; with ``coast`` a lost person is
    compared where a constant-velocity model of the box centre (``velocity_alpha``: its exponential smoothing) expects them; a row
    with an empty box -- ``track_frame``'s lost person, ``pose_nms``' suppressed one -- is nobody: id -1, no new id spent.  The
    demo's ``next_id = n + 1`` after the first frame is kept (one in-place add on the streams that had somebody), so
    ``max_lost=0`` on frames without empty boxes gives what ``max_lost=None`` gives.  ``slot`` then holds every row's slot (-1:
    nobody, or the table was full -- ``status`` bit 2); with ``one_euro`` a person returning from a gap starts a fresh filter
    state.  ``lost()`` names the tracks that are currently lost."""

    def __init__(self, net=None, pose_alpha: float = 0.2, similarity_threshold: float = 0.4, smoothing_alpha: float = 0.1,
                 one_euro: Optional[dict] = None, max_lost: Optional[int] = None, coast: bool = False, velocity_alpha: float = 0.5,
                 capacity: int = postproc.HRN_MAX_TRACKED):
        self.net = net
        self.max_lost, self.coast, self.velocity_alpha, self.capacity = max_lost, bool(coast), float(velocity_alpha), int(capacity)
        self.pose_alpha, self.similarity_threshold, self.smoothing_alpha = float(pose_alpha), float(similarity_threshold), float(smoothing_alpha)
        self.one_euro = None
        if one_euro is not None:
            self.one_euro = dict(one_euro)
            self.rate = float(self.one_euro.pop("rate", 30.0))
            unknown = set(self.one_euro) - {"min_cutoff", "beta", "d_cutoff", "threshold"}
            if unknown or not self.rate > 0.0:
                raise ValueError("one_euro takes min_cutoff, beta, d_cutoff, threshold and a positive rate, got %r" % (one_euro,))
        self.reset()

    def reset(self):
        self.prev_boxes = self.prev_pts = self.prev_ids = self.prev_counts = self.next_id = self.status = None
        self.filter_state = self.predicted = None
        self.table = self.slot = None

    def _own(self, boxes, pts):
        """copies of this frame's boxes and joints where the tracker works: (n, 4) int32 and (n, J, 3) float32"""
        if self.net is None:
            b = np.array(boxes.cpu() if hasattr(boxes, "cpu") else boxes, dtype=np.int32).reshape(-1, 4)
            p = np.array(pts.cpu() if hasattr(pts, "cpu") else pts, dtype=np.float32)
            return b, p.reshape(len(b), -1 if p.size else 1, 3) if p.ndim != 3 else p
        import torch

        from .frames import device_tensor

        def own(v, dtype):
            moved = device_tensor(v, self.net.torch_device, dtype)
            return moved.clone() if moved is v else moved   # the caller's own tensor, used where it lies: never aliased

        b = own(boxes, torch.int32).reshape(-1, 4).contiguous()
        p = own(pts, torch.float32)
        return b, (p.reshape(int(b.shape[0]), -1 if p.numel() else 1, 3) if p.dim() != 3 else p).contiguous()

    def _upload(self, v: np.ndarray):
        if self.net is None:
            return v
        import torch

        return torch.from_numpy(v).to(self.net.torch_device, non_blocking=True)

    def update(self, boxes, pts, counts: Optional[object] = None, dt: Optional[float] = None, lookahead: Optional[float] = None):
        boxes, pts = self._own(boxes, pts)
        match = None
        n = int(boxes.shape[0])
        if int(pts.shape[0]) != n:
            raise ValueError("%d boxes for %d skeletons" % (n, int(pts.shape[0])))
        counts = np.asarray([n] if counts is None else counts, dtype=np.int64).reshape(-1)
        if (counts < 0).any() or int(counts.sum()) != n:
            raise ValueError("counts must be non-negative and sum to %d people, got %s" % (n, counts.tolist()))
        if self.prev_counts is not None and len(counts) != len(self.prev_counts):
            raise ValueError("%d streams after %d: reset() the tracker first" % (len(counts), len(self.prev_counts)))
        if self.max_lost is not None and self.table is None and n == 0:   # nobody yet: the table waits for somebody (and their J)
            ids, self.next_id = self._upload(np.zeros(0, np.int32)), self._upload(np.zeros(len(counts), np.int32))
        elif self.max_lost is not None:
            if self.table is None:
                fresh = postproc.new_track_table if self.net is None else self.net.new_track_table
                self.table = fresh(len(counts), self.capacity, int(pts.shape[1]))
            entry = postproc.track_people if self.net is None else self.net.track_people
            boxes, pts, ids, match, self.slot, self.status = entry(boxes, pts, self.table, self.pose_alpha, self.similarity_threshold,
                                                                   self.smoothing_alpha, self.max_lost, self.coast, self.velocity_alpha,
                                                                   counts=counts)
            self.next_id = self.table["next_id"]
            if self.prev_counts is None:  # live-demo.py:118: next_id = n + 1 after the first frame, on the streams that had somebody
                self.next_id += self.next_id > 0
            if self.prev_counts is None or n == 0:   # (no filter state to follow yet / nobody to follow it)
                match = None
        elif self.prev_counts is None:    # live-demo.py:116-118, per stream
            ids = np.concatenate([np.arange(c, dtype=np.int32) for c in counts]) if n else np.zeros(0, np.int32)
            ids, self.next_id = self._upload(ids), self._upload(np.where(counts > 0, counts + 1, 0).astype(np.int32))
        elif n == 0:                      # live-demo.py:125-126: nobody, next_id stays
            ids = self._upload(np.zeros(0, np.int32))
        else:
            entry = postproc.associate_people if self.net is None else self.net.associate_people
            boxes, pts, ids, match, self.next_id, self.status = entry(boxes, pts, self.prev_boxes, self.prev_pts, self.prev_ids, self.next_id,
                                                                      self.pose_alpha, self.similarity_threshold, self.smoothing_alpha,
                                                                      counts=counts, prev_counts=self.prev_counts)
        filtered = pts
        if self.one_euro is not None:     # the state follows the people through this update's match; prev_pts stays the association's
            entry = postproc.filter_poses if self.net is None else self.net.filter_poses
            filtered, self.predicted, self.filter_state = entry(pts, self.filter_state, match, counts=counts,
                                                                prev_counts=None if self.filter_state is None else self.prev_counts,
                                                                dt=1.0 / self.rate if dt is None else dt, lookahead=lookahead, **self.one_euro)
        self.prev_boxes, self.prev_pts, self.prev_ids, self.prev_counts = boxes, pts, ids, counts
        return boxes, filtered, ids

    def lost(self):
        """``(ids, boxes, pts, lost)`` of the tracks that are currently lost (``max_lost`` given): their ids (k,) int32, the boxes
        (k, 4) int32 and joints (k, J, 3) float32 they are compared at in the next update (with ``coast``: where the velocity
        expects them; otherwise as last seen) and the updates they have been missing (k,) int32 -- stream after stream, slots in
        order; tensors on the engine's GPU or numpy arrays.  For drawing ghosts or seeding crops.  The masking reads a count back."""
        if self.table is None:
            raise ValueError("lost() needs a tracker with max_lost and at least one update")
        t = self.table
        mask = (t["slot_id"] >= 0) & (t["slot_lost"] > 0)
        lost, vel = t["slot_lost"][mask], t["slot_vel"][mask]
        boxes, pts = t["slot_boxes"][mask], t["slot_pts"][mask]
        if self.coast and len(lost):
            f64, f32, i32 = (np.float64, np.float32, np.int32) if self.net is None else (_torch().float64, _torch().float32, _torch().int32)
            cast = (lambda a, d: a.astype(d)) if self.net is None else (lambda a, d: a.to(d))
            k = cast(lost, f64) + 1.0
            step = cast(vel, f64) * k[:, None]                                  # (k, 2): dy, dx
            moved = cast(boxes, f64) + step[:, [1, 0, 1, 0]]
            boxes = cast((np.clip if self.net is None else _torch().clamp)(moved, -2147483648.0, 2147483647.0), i32)
            pts = pts.copy() if self.net is None else pts.clone()
            pts[:, :, :2] = cast(cast(pts[:, :, :2], f64) + step[:, None, :], f32)
        return t["slot_id"][mask], boxes, pts, lost


def _torch():
    import torch

    return torch
