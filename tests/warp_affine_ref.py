"""``cv2.warpAffine(frame, M, (W, H), flags=cv2.INTER_LINEAR)`` for 8-bit 3-channel frames with the default border
(``BORDER_CONSTANT``, value 0), restated in numpy int64 / float64 -- what ``hrn_warp_crops`` is pinned to (include/hrnet_mi355.h)
-- and the evaluation transform built on it (``datasets/COCO.py:290-304``: warpAffine, BGR -> RGB as the dataset reads its
images, ToTensor, Normalize).

OpenCV's classic 8-bit path is integer arithmetic throughout: the forward matrix is inverted in float64, source coordinates
are formed in 1/1024 pixel per row and per column, added, and rounded to 1/32 pixel; the four taps are blended with weights
``(32 - fx) * (32 - fy)`` ... out of 1024 (its 15-bit table for 5-bit fractions holds exact multiples of 32).  A helper module
like ``subpixel_ref.py``; parity with a cv2 build is pinned by ``tests/golden/make_warp_golden.py`` where opencv-python exists."""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


def invert(M):
    """the inversion ``cv::warpAffine`` applies to a forward matrix, statement for statement (float64 scalars: numpy rounds
    after every operation)"""
    m = [np.float64(v) for v in np.asarray(M, np.float64).reshape(6)]
    D = m[0] * m[4] - m[1] * m[3]
    D = np.float64(1.0) / D if D != 0 else np.float64(0.0)
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] = m[1] * -D
    m[3] = m[3] * -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return np.array(m, np.float64).reshape(2, 3)


def source_coords(Minv, H, W):
    """``(X, Y)`` int64 arrays (H, W): the source coordinate of every output pixel in 1/32 pixel"""
    Minv = np.asarray(Minv, np.float64).reshape(2, 3)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    rint = lambda a: np.rint(a).astype(np.int64)   # noqa: E731 -- round half to even
    X = (rint((Minv[0, 1] * y + Minv[0, 2]) * 1024) + 16 + rint(Minv[0, 0] * x * 1024)) >> 5
    Y = (rint((Minv[1, 1] * y + Minv[1, 2]) * 1024) + 16 + rint(Minv[1, 0] * x * 1024)) >> 5
    return X, Y


def _tap(frame, sy, sx):
    """frame[sy, sx] as int64 (H, W, C), 0 outside the frame"""
    h, w = frame.shape[:2]
    inside = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
    v = frame[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)].astype(np.int64)
    return v * inside[..., None]


def warp_u8(frame, M, out_hw):
    """``cv2.warpAffine(frame, M, (W, H), flags=cv2.INTER_LINEAR)``: (Hf, Wf, C) uint8 -> (H, W, C) uint8"""
    H, W = out_hw
    X, Y = source_coords(invert(M), H, W)
    sx, sy, fx, fy = X >> 5, Y >> 5, (X & 31)[..., None], (Y & 31)[..., None]
    v = (_tap(frame, sy, sx) * (32 - fx) * (32 - fy) + _tap(frame, sy, sx + 1) * fx * (32 - fy) +
         _tap(frame, sy + 1, sx) * (32 - fx) * fy + _tap(frame, sy + 1, sx + 1) * fx * fy + 512) >> 10
    return v.astype(np.uint8)


def eval_transform(frames, matrices, frame_index, out_hw):
    """the (n, 3, H, W) float32 batch of the evaluation path: crop i = warp of ``frames[frame_index[i]]`` (BGR) by
    ``matrices[i]``, as RGB planes, ``(v / 255 - mean) / std`` in float32"""
    frames = np.asarray(frames)
    if frames.ndim == 3:
        frames = frames[None]
    matrices = np.asarray(matrices, np.float64).reshape(-1, 2, 3)
    n = len(matrices)
    if frame_index is None:
        frame_index = np.zeros(n, int) if len(frames) == 1 else np.arange(n)
    out = np.empty((n, 3) + tuple(out_hw), np.float32)
    for i in range(n):
        rgb = warp_u8(frames[frame_index[i]], matrices[i], out_hw)[..., ::-1]
        x = rgb.astype(np.float32) / np.float32(255)
        out[i] = ((x - MEAN) / STD).transpose(2, 0, 1)
    return out
