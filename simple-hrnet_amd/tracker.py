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

    ``one_euro``: None, or ``dict(min_cutoff, beta, d_cutoff, threshold, rate=30.0)`` (any subset; the rest are
    ``filter_poses``' defaults): every update is then followed by ONE ``filter_poses`` call whose state follows the people
    through that update's ``match`` (no ``match`` on the first update; with nobody present the state is emptied).  ``update``
    then returns the FILTERED joints, and ``predicted`` holds the joints expected ``lookahead`` seconds later -- for
    ``track_frame(frame, tracker.predicted)``.  ``dt``: seconds since the previous update (None: ``1 / rate``); ``lookahead``
    None: ``dt``.  What the tracker keeps for the next association stays the association's own output.  The prediction starts
    from the raw position; the filtered joints lag on steady motion, the filter's known trade (``beta``).  With ``one_euro=None``
    no filter call is made and every result is what it is without the option."""

    def __init__(self, net=None, pose_alpha: float = 0.2, similarity_threshold: float = 0.4, smoothing_alpha: float = 0.1,
                 one_euro: Optional[dict] = None):
        self.net = net
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
        if self.prev_counts is None:      # live-demo.py:116-118, per stream
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
