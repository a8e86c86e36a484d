"""numpy restatement of the heat-map overlay definition of include/hrnet_mi355.h (hrn_draw_heatmaps_dev), written from the header's
text: int64 throughout, np.float32 scalars for the quantiser, one full-frame V per canvas and a plain loop over people -- no
tiles, no culling, no 2 x 2 threads.  Test infrastructure, beside draw_ref.py and label_ref.py: the host tests hold
hrn_heatmap_quantise / hrn_draw_heatmaps_host to this file byte for byte, the GPU tests the kernels."""
import numpy as np

import yuv_ref
from draw_ref import grid

LO, HI = -8192, 16383
CONST, VALUE = 0, 1
F32 = np.float32


def jet():
    """(256, 3) uint8 (B, G, R): the issue's integer formula, k = 3, 2, 1 for R, G, B"""
    out = np.zeros((256, 3), np.uint8)
    for i in range(256):
        for col, k in ((2, 3), (1, 2), (0, 1)):
            out[i, col] = (min(max(765 - abs(8 * i - 510 * k), 0), 510) + 1) >> 1
    return out


def gray():
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)


def reduce_max(maps, mask=None):
    """(n, hq, wq) float32: the maximum over the masked joints; a NaN never wins, all-NaN gives NaN"""
    maps = np.asarray(maps, F32)
    n, J = maps.shape[:2]
    sel = np.ones(J, bool) if mask is None else np.asarray(mask).astype(bool)
    assert sel.any()
    part = maps[:, sel]
    nan = np.isnan(part)
    best = np.where(nan, F32(-np.inf), part).max(1)
    return np.where(nan.all(1), F32(np.nan), best).astype(F32)


def quantise(maps, mask, lo, hi):
    """Q (n, hq, wq) uint8"""
    lo, hi = F32(lo), F32(hi)
    with np.errstate(all="ignore"):
        k = F32(F32(255.0) / F32(hi - lo))
        v = reduce_max(maps, mask)
        t = ((v - lo).astype(F32) * k).astype(F32)           # each operation rounded to float32 on its own
        lifted = (t + F32(0.5)).astype(F32)
        q = np.where(t > 0, np.where(t >= 255, 255, np.where((t > 0) & (t < 255), lifted, 0).astype(np.int64)), 0)
    return q.astype(np.uint8)


def is_drawn(box):
    x1, y1, x2, y2 = (int(v) for v in box)
    return all(LO <= v <= HI for v in (x1, y1, x2, y2)) and x2 > x1 and y2 > y1


def sample_plane(q, box, height, width):
    """(S (H, W) int64, inside (H, W) bool) of one person's Q (hq, wq) under its box"""
    hq, wq = q.shape
    x1, y1, x2, y2 = (np.int64(v) for v in box)
    px, py = grid(height, width)
    inside = (x1 <= px) & (px < x2) & (y1 <= py) & (py < y2)
    bw, bh = x2 - x1, y2 - y1
    ux = np.minimum(((np.clip(px - x1, 0, None)) * wq * 256) // bw, (wq - 1) * 256)
    uy = np.minimum(((np.clip(py - y1, 0, None)) * hq * 256) // bh, (hq - 1) * 256)
    c0, fx, r0, fy = ux >> 8, ux & 255, uy >> 8, uy & 255
    c1, r1 = np.minimum(c0 + 1, wq - 1), np.minimum(r0 + 1, hq - 1)
    c0, c1, r0, r1 = (np.clip(v, 0, m) for v, m in ((c0, wq - 1), (c1, wq - 1), (r0, hq - 1), (r1, hq - 1)))   # (outside: unused)
    q = q.astype(np.int64)
    top = q[r0, c0] * (256 - fx) + q[r0, c1] * fx
    bot = q[r1, c0] * (256 - fx) + q[r1, c1] * fx
    return (top * (256 - fy) + bot * fy + 32768) >> 16, inside


def value_plane(height, width, Q, boxes):
    """V (H, W) int64: the maximum of S over the people whose box holds the pixel, 0 where nobody's does"""
    V = np.zeros((height, width), np.int64)
    for q, box in zip(Q, np.asarray(boxes, np.int64).reshape(-1, 4)):
        if not is_drawn(box):
            continue
        S, inside = sample_plane(q, box, height, width)
        V = np.where(inside, np.maximum(V, S), V)
    return V


def alpha_of(V, alpha, mode):
    return np.full(V.shape, alpha, np.int64) if mode == CONST else (alpha * V + 127) // 255


def blend(src, colour, a):
    return (src.astype(np.int64) * (255 - a) + colour.astype(np.int64) * a + 127) // 255


def draw_bgr(frame, maps, boxes, lut, mask=None, lo=0.0, hi=1.0, alpha=153, mode=VALUE, cutoff=26, Q=None):
    """draws into `frame` ((H, W, 3) uint8, any row stride) in place; only written pixels are stored"""
    lut = np.asarray(lut, np.uint8)
    Q = quantise(maps, mask, lo, hi) if Q is None else Q
    V = value_plane(frame.shape[0], frame.shape[1], Q, boxes)
    a = alpha_of(V, alpha, mode)
    written = (V >= cutoff) & (a > 0)
    out = blend(frame, lut[V], a[..., None]).astype(np.uint8)
    frame[written] = out[written]
    return frame


def draw_yuv(data, height, width, fmt, maps, boxes, lut, pitch=None, mask=None, lo=0.0, hi=1.0, alpha=153, mode=VALUE, cutoff=26, Q=None):
    """draws into the rawvideo buffer `data` (yuv_ref.planes' layout) in place; `lut` rows are (Y, U, V)"""
    lut = np.asarray(lut, np.uint8)
    Q = quantise(maps, mask, lo, hi) if Q is None else Q
    V = value_plane(height, width, Q, boxes)
    a = alpha_of(V, alpha, mode)
    written = (V >= cutoff) & (a > 0)
    Y, U, Vp = yuv_ref.planes(data, height, width, fmt, pitch)
    assert np.shares_memory(Y, data) and np.shares_memory(U, data) and np.shares_memory(Vp, data)
    Y[written] = blend(Y, lut[V][..., 0], a).astype(np.uint8)[written]
    blocks = V.reshape(height // 2, 2, width // 2, 2)
    Vc = (blocks.sum((1, 3)) + 2) >> 2
    ac = alpha_of(Vc, alpha, mode)
    chroma = written.reshape(height // 2, 2, width // 2, 2).any((1, 3)) & (ac > 0)
    U[chroma] = blend(U, lut[Vc][..., 1], ac).astype(np.uint8)[chroma]
    Vp[chroma] = blend(Vp, lut[Vc][..., 2], ac).astype(np.uint8)[chroma]
    return data


def draw_clip(frames, maps, boxes, frame_index, lut, **kw):
    """BGR frames of a clip: person i on frames[frame_index[i]]"""
    maps, boxes = np.asarray(maps), np.asarray(boxes)
    for f, frame in enumerate(frames):
        who = [i for i in range(len(boxes)) if frame_index[i] == f]
        if who:
            draw_bgr(frame, maps[who], boxes[who], lut, **kw)
    return frames
