"""numpy restatement of the face mosaic of include/hrnet_mi355.h (hrn_mosaic_dev, hrn_mosaic_host, hrn_mosaic_regions), written
from the header's text and sharing no code with csrc/mosaic_math.h: a person's region from joints or from a box, the marked
cells of a canvas, the mean of a marked cell.  Test infrastructure, beside draw_ref.py and heat_ref.py: the host forms and
the kernels are held to this file byte for byte and status for status."""
import numpy as np

import yuv_ref

F32 = np.float32
LO, HI = -8192, 16383


def live_joints(person, threshold):
    """[(j, X, Y)] of the live joints of one person's (J, 3) float32 (y, x, confidence)"""
    out = []
    for j, (y, x, c) in enumerate(np.asarray(person, F32)):
        if not c > F32(threshold):                      # float32 compare: equality and NaN are not live
            continue
        if not (np.isfinite(x) and np.isfinite(y)):
            continue
        X, Y = int(np.trunc(np.float64(x))), int(np.trunc(np.float64(y)))
        if LO <= X <= HI and LO <= Y <= HI:
            out.append((j, X, Y))
    return out


def clip(x_lo, y_lo, x_hi, y_hi, H, W):
    x1, y1, x2, y2 = max(x_lo, 0), max(y_lo, 0), min(x_hi, W), min(y_hi, H)
    if x2 <= x1 or y2 <= y1:
        return (0, 0, 0, 0), 2
    return (x1, y1, x2, y2), 0


def region_from_joints(person, joints, threshold, H, W, scale=(1, 1), min_half=0):
    live = live_joints(person, threshold)
    listed = [(X, Y) for j, X, Y in live if j in set(joints)]
    if not listed:
        return (0, 0, 0, 0), 1
    extent = lambda pts: max(max(p[0] for p in pts) - min(p[0] for p in pts), max(p[1] for p in pts) - min(p[1] for p in pts))   # noqa: E731
    E, P = extent(listed), extent([(X, Y) for _, X, Y in live])
    rmin = min_half if min_half else (P + 15) // 16
    R = max(rmin, (E * scale[0] + scale[1] - 1) // scale[1])
    cx2 = min(p[0] for p in listed) + max(p[0] for p in listed)
    cy2 = min(p[1] for p in listed) + max(p[1] for p in listed)
    return clip((cx2 >> 1) - R, (cy2 >> 1) - R, ((cx2 + 1) >> 1) + R + 1, ((cy2 + 1) >> 1) + R + 1, H, W)      # Python's >> floors


def region_from_box(box, H, W):
    x1, y1, x2, y2 = (int(v) for v in box)
    if x2 <= x1 or y2 <= y1:
        return (0, 0, 0, 0), 1
    return clip(x1, y1, x2, y2, H, W)


def regions(canvas_hw, pts=None, boxes=None, joints=None, threshold=0.5, scale=(1, 1), min_half=0):
    """((n, 4) int32, (n,) int32 status); canvas_hw: (height, width) or one pair per person"""
    n = len(pts) if pts is not None else len(boxes)
    hw = np.broadcast_to(np.asarray(canvas_hw).reshape(-1, 2), (n, 2))
    out, status = np.zeros((n, 4), np.int32), np.zeros((n,), np.int32)
    for i in range(n):
        H, W = int(hw[i, 0]), int(hw[i, 1])
        if pts is not None:
            J = np.asarray(pts).shape[1]
            out[i], status[i] = region_from_joints(pts[i], range(J) if joints is None else joints, threshold, H, W, scale, min_half)
        else:
            out[i], status[i] = region_from_box(boxes[i], H, W)
    return out, status


def cell_size(cell, H, W):
    if cell:
        return cell
    m = min(max(min(H, W) // 64, 8), 32)
    return 1 << (m.bit_length() - 1)


def marks(H, W, s, rects):
    """bool (ceil(H / s), ceil(W / s)): the cells that intersect a non-empty rectangle"""
    m = np.zeros((-(-H // s), -(-W // s)), bool)
    for x1, y1, x2, y2 in rects:
        if x2 > x1 and y2 > y1:
            m[y1 // s:(y2 - 1) // s + 1, x1 // s:(x2 - 1) // s + 1] = True
    return m


def flatten(plane, m, s):
    """every marked cell of a (rows, cols[, channels]) uint8 view takes its rounded mean, per channel, in place"""
    for cy, cx in zip(*np.nonzero(m)):
        part = plane[cy * s:(cy + 1) * s, cx * s:(cx + 1) * s]                # numpy cuts the slice at the edge: the partial cell
        c = part.shape[0] * part.shape[1]
        if c == 0:
            continue
        total = part.reshape(c, -1).astype(np.int64).sum(0)
        part[...] = ((total + (c >> 1)) // c).astype(np.uint8)
    return plane


def mosaic_bgr(frame, rects, cell=0):
    """frame: (H, W, 3) uint8 view (any strides), changed in place"""
    H, W = frame.shape[:2]
    s = cell_size(cell, H, W)
    return flatten(frame, marks(H, W, s, rects), s)


def mosaic_yuv(data, H, W, fmt, rects, cell=0, pitch=None):
    """data: a rawvideo NV12 / I420 buffer (yuv_ref.planes' layout), changed in place"""
    Y, U, V = yuv_ref.planes(data, H, W, fmt, pitch)
    s = cell_size(cell, H, W)
    m = marks(H, W, s, rects)
    flatten(Y, m, s), flatten(U, m, s // 2), flatten(V, m, s // 2)             # even sides: a cell's chroma is (s / 2) x (s / 2)
    return data


def mosaic_clip(frames, rects, frame_index, cell=0):
    """several BGR frames (None: nobody is on it): the people of frame f are those with frame_index == f"""
    idx = np.asarray(frame_index)
    for f, frame in enumerate(frames):
        if frame is not None and (idx == f).any():
            mosaic_bgr(frame, np.asarray(rects)[idx == f], cell)
    return frames
