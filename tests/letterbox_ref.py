"""TEST INFRASTRUCTURE ONLY -- restatements of the detector link (``include/hrnet_mi355.h``: ``hrn_letterbox_geometry``,
``hrn_letterbox_frames``, ``hrn_detections_to_frame``) that the tests compare the library with.

* the two letterbox functions of the reference's detector wrappers (``models_/detectors/YOLOv3.py:23-45`` with ``mode='square'``,
  ``YOLOv5.py:9-39`` with ``auto=False, scaleFill=False``), in numpy, with ``cv2.resize(INTER_LINEAR)`` taken from
  ``oracle.cv2_resize_oracle.resize_u8`` plus the one rule that oracle does not have: a frame exactly twice the resized size in both
  axes goes through cv2's INTER_AREA fast path, ``(a + b + c + d + 2) >> 2`` over each 2 x 2 block.  PARITY WITH cv2 IS UNPINNED
  (cv2 is not installed here; ``tests/golden/make_letterbox_golden.py`` makes the pin where it is);
* ``ToTensor`` (``float32(v) / 255``) and the 16-bit roundings;
* the two inverses -- ``scale_coords`` (``YOLOv3.py:49-56``) and ``(x - dw) / ratio`` (``YOLOv5.py:95-98``) -- in torch CPU float32
  operations, with the filters in front of them.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.cv2_resize_oracle import INTER_LINEAR, resize_u8  # noqa: E402

PAD = {"yolov3": 128, "yolov5": 114}   # 127.5 saturates to 128 (round half to even); YOLOv5's 114


def geometry_ref(h, w, size, style):
    """(new_w, new_h, top, bottom, left, right, ratio, dw, dh) for arrays (or scalars) of frame sizes; np.rint = Python's round"""
    h, w = np.asarray(h, np.int64), np.asarray(w, np.int64)
    if style == "yolov3":
        out_h = out_w = int(size)
        ratio = float(size) / np.maximum(h, w)
    else:
        out_h, out_w = (size, size) if np.ndim(size) == 0 else size
        ratio = np.minimum(out_h / h, out_w / w)
    new_w, new_h = np.rint(w * ratio).astype(np.int64), np.rint(h * ratio).astype(np.int64)
    dw, dh = (out_w - new_w) / 2, (out_h - new_h) / 2
    top, bottom = np.rint(dh - 0.1).astype(np.int64), np.rint(dh + 0.1).astype(np.int64)
    left, right = np.rint(dw - 0.1).astype(np.int64), np.rint(dw + 0.1).astype(np.int64)
    return new_w, new_h, top, bottom, left, right, ratio, dw, dh


def geometry_scalar(h, w, size, style):
    """the wrappers' statements, one frame, in plain Python (what geometry_ref vectorises)"""
    if style == "yolov3":
        out_h = out_w = size
        ratio = float(size) / max(h, w)
    else:
        out_h, out_w = (size, size) if isinstance(size, int) else size
        ratio = min(out_h / h, out_w / w)
    new_w, new_h = int(round(w * ratio)), int(round(h * ratio))
    dw, dh = (out_w - new_w) / 2, (out_h - new_h) / 2
    return (new_w, new_h, int(round(dh - 0.1)), int(round(dh + 0.1)), int(round(dw - 0.1)), int(round(dw + 0.1)), ratio, dw, dh)


def resize_linear(img, new_hw):
    """cv2.resize(img, (new_w, new_h), interpolation=cv2.INTER_LINEAR) for (h, w, 3) uint8, the 2:1 rule included"""
    h, w = img.shape[:2]
    nh, nw = new_hw
    if h == 2 * nh and w == 2 * nw:
        s = img.astype(np.int64)
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    return resize_u8(img, (nh, nw), INTER_LINEAR)


def letterbox_u8(frame_bgr, size, style, order="rgb", pad=None):
    """the (out_h, out_w, 3) uint8 image the detector wrapper hands to ToTensor, channels in `order`"""
    h, w = frame_bgr.shape[:2]
    new_w, new_h, top, bottom, left, right, _, _, _ = geometry_scalar(h, w, size, style)
    fill = np.broadcast_to(np.asarray(PAD[style] if pad is None else pad, np.uint8).reshape(-1), (3,))
    body = resize_linear(frame_bgr, (new_h, new_w))
    if order == "rgb":
        body = body[..., ::-1]
    out = np.empty((top + new_h + bottom, left + new_w + right, 3), np.uint8)
    out[...] = fill
    out[top:top + new_h, left:left + new_w] = body
    return out


def to_tensor(u8_hwc, dtype):
    """ToTensor in float32, then the 16-bit rounding torch's .to() performs; uint8: the image itself"""
    if dtype == torch.uint8:
        return torch.from_numpy(np.ascontiguousarray(u8_hwc))
    x = torch.from_numpy(np.ascontiguousarray(u8_hwc.transpose(2, 0, 1))).to(torch.float32)
    x = x / torch.full((1, 1, 1), 255.0, dtype=torch.float32)
    return x.to(dtype)


def scale_coords(coords, from_shape, to_shape):
    """YOLOv3.py:49-56 on a float32 CPU tensor (a copy is returned)"""
    coords = coords.clone()
    gain = max(from_shape) / max(to_shape)
    coords[:, [0, 2]] -= (from_shape[1] - to_shape[1] * gain) / 2
    coords[:, [1, 3]] -= (from_shape[0] - to_shape[0] * gain) / 2
    coords[:, :4] /= gain
    coords[:, :4] = coords[:, :4].clamp(min=0)
    return coords


def yolov5_inverse(dets, dw, dh, ratio):
    """YOLOv5.py:95-98 on a float32 CPU tensor (a copy is returned)"""
    dets = dets.clone()
    dets[:, [0, 2]] = (dets[:, [0, 2]] - dw) / ratio
    dets[:, [1, 3]] = (dets[:, [1, 3]] - dh) / ratio
    return dets


def detections_ref(dets, frame_hw, size, style, counts, conf_thres=None, classes=None, class_col=-1, compact=True, conf_col=4):
    """the whole link after the network: (rows, counts, status) as hrn_detections_to_frame defines them"""
    dets = np.asarray(dets, np.float32)
    out, status, kept_counts = np.zeros_like(dets), np.zeros(len(dets), np.int32), []
    out_hw = (size, size) if np.ndim(size) == 0 else tuple(size)
    first = 0
    for (h, w), n in zip(frame_hw, counts):
        rows = dets[first:first + n]
        finite = np.isfinite(rows[:, :4]).all(axis=1) & np.isfinite(rows[:, conf_col])
        st = np.where(finite, 0, 5).astype(np.int32)
        if conf_thres is not None:
            st[(st == 0) & ~(rows[:, conf_col] >= np.float32(conf_thres))] = 1
        if classes is not None:
            st[(st == 0) & ~np.isin(rows[:, class_col], np.asarray(classes, np.float32))] = 2
        keep = st == 0
        t = torch.from_numpy(rows[keep].copy())
        if style == "yolov3":
            mapped = scale_coords(t, out_hw, (h, w))
        else:
            g = geometry_scalar(int(h), int(w), size if np.ndim(size) == 0 else tuple(size), style)
            mapped = yolov5_inverse(t, g[7], g[8], g[6])
        mapped = mapped.numpy()
        if compact:
            out[first:first + len(mapped)] = mapped
        else:
            out[first:first + n][keep] = mapped
        status[first:first + n] = st
        kept_counts.append(int(keep.sum()))
        first += n
    return out, np.asarray(kept_counts, np.int32), status


def random_rows(n, stride, size, seed, nclasses=3):
    """n detector rows in letterbox coordinates: boxes around and beyond the square, confidences in [0, 1], integer classes"""
    rng = np.random.default_rng(seed)
    side = float(size if np.ndim(size) == 0 else max(size))
    d = np.empty((n, stride), np.float32)
    a, b = rng.uniform(-0.2 * side, 1.2 * side, (2, n, 2)).astype(np.float32)
    d[:, 0:2], d[:, 2:4] = np.minimum(a, b), np.maximum(a, b)
    d[:, 4:] = rng.uniform(0, 1, (n, stride - 4)).astype(np.float32)
    d[:, -1] = rng.integers(0, nclasses, n).astype(np.float32)
    return d
