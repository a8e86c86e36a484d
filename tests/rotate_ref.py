"""The numpy restatement of frame rotation (include/hrnet_mi355.h: hrn_rotate_frames, hrn_rotate_people): ``cv2.rotate`` is a pure
permutation of pixels and ``np.rot90`` its exact restatement, plane by plane; the people table in ``np.float32`` / ``np.int32``."""
import numpy as np

ROT90_K = {0: -1, 1: 2, 2: 1}   # cv2.ROTATE_90_CLOCKWISE / _180 / _90_COUNTERCLOCKWISE as np.rot90's k


def rotate_plane(a, code):
    """an (H, W) or (H, W, C) array rotated as cv2.rotate does"""
    return np.ascontiguousarray(np.rot90(a, ROT90_K[int(code)], axes=(0, 1)))


def rotated_hw(h, w, code):
    return (h, w) if int(code) == 1 else (w, h)


def yuv_planes(data, h, w, fmt, pitch=None):
    """the planes of a rawvideo NV12 / I420 buffer of row pitch ``pitch`` as arrays of ELEMENTS: Y (h, w), then NV12's
    (h/2, w/2, 2) pair plane, or I420's U and V (h/2, w/2)"""
    pitch = w if pitch is None else pitch
    data = np.asarray(data, np.uint8).reshape(-1)
    y = data[:pitch * h].reshape(h, pitch)[:, :w]
    if fmt == "nv12":
        uv = data[pitch * h:pitch * h * 3 // 2].reshape(h // 2, pitch)[:, :w].reshape(h // 2, w // 2, 2)
        return [y, uv]
    half = pitch // 2
    u = data[pitch * h:pitch * h + half * (h // 2)].reshape(h // 2, half)[:, :w // 2]
    v = data[pitch * h + half * (h // 2):pitch * h + 2 * half * (h // 2)].reshape(h // 2, half)[:, :w // 2]
    return [y, u, v]


def rotate_yuv(data, h, w, fmt, code, pitch=None, out_pitch=None, fill=None):
    """the rotated frame as a rawvideo buffer of row pitch ``out_pitch`` (default: its width); bytes of a row beyond its elements
    keep ``fill`` (a buffer of the output's size, default zeros)"""
    rh, rw = rotated_hw(h, w, code)
    out_pitch = rw if out_pitch is None else out_pitch
    out = np.zeros(out_pitch * rh * 3 // 2, np.uint8) if fill is None else np.array(fill, np.uint8).reshape(-1)
    assert out.size == out_pitch * rh * 3 // 2
    for src, dst in zip(yuv_planes(data, h, w, fmt, pitch), yuv_planes(out, rh, rw, fmt, out_pitch)):
        dst[...] = rotate_plane(src, code)
    return out


def rotate_joints(pts, frame_hw, codes):
    """(n, J, 3) float32 (y, x, c) -> the rotated frame's coordinates: one float32 subtraction or a copy per coordinate"""
    pts = np.asarray(pts, np.float32)
    n = len(pts)
    hw = np.broadcast_to(np.asarray(frame_hw, np.int32).reshape(-1, 2), (n, 2))
    codes = np.broadcast_to(np.asarray(codes, np.int32).reshape(-1), (n,))
    out = pts.copy()
    with np.errstate(invalid="ignore"):
        for i in range(n):
            hs1, ws1 = np.float32(hw[i, 0] - 1), np.float32(hw[i, 1] - 1)
            y, x = pts[i, :, 0], pts[i, :, 1]
            if codes[i] == 0:
                out[i, :, 0], out[i, :, 1] = x, hs1 - y
            elif codes[i] == 1:
                out[i, :, 0], out[i, :, 1] = hs1 - y, ws1 - x
            else:
                out[i, :, 0], out[i, :, 1] = ws1 - x, y
    return out


def rotate_boxes(boxes, frame_hw, codes):
    """(n, 4) int32 half-open (x1, y1, x2, y2) -> the range the rotated slice occupies; all-zero rows stay all-zero"""
    boxes = np.asarray(boxes, np.int32)
    n = len(boxes)
    hw = np.broadcast_to(np.asarray(frame_hw, np.int32).reshape(-1, 2), (n, 2))
    codes = np.broadcast_to(np.asarray(codes, np.int32).reshape(-1), (n,))
    out = np.zeros_like(boxes)
    for i in range(n):
        x1, y1, x2, y2 = (np.int32(v) for v in boxes[i])
        hs, ws = hw[i]
        if not boxes[i].any():
            continue
        if codes[i] == 0:
            out[i] = (hs - y2, x1, hs - y1, x2)
        elif codes[i] == 1:
            out[i] = (ws - x2, hs - y2, ws - x1, hs - y1)
        else:
            out[i] = (y1, ws - x2, y2, ws - x1)
    return out
