"""numpy restatement of the overlay definition of include/hrnet_mi355.h (hrn_draw_poses): int64 throughout, one full-frame mask per
primitive and a plain painter's loop in primitive order -- no tiles, no lists, no culling, and the disc by its own formula (the
kernel treats it as a zero-length capsule).  Test infrastructure, beside yuv_ref.py: the GPU tests hold the kernels to this file
byte for byte."""
import numpy as np

import yuv_ref

LO, HI = -8192, 16383


def default_radius(height, width):
    return max(1, min(height, width) // 160)


def live_joints(person, threshold):
    """[(X, Y) or None] of one person's (J, 3) float32 (y, x, confidence)"""
    out = []
    thr = np.float32(threshold)
    for y, x, c in np.asarray(person, np.float32):
        ok = bool(c > thr) and bool(np.isfinite(y)) and bool(np.isfinite(x))
        if ok:
            X, Y = int(x), int(y)                     # Python's int(): towards zero
            ok = LO <= X <= HI and LO <= Y <= HI
        out.append((X, Y) if ok else None)
    return out


def grid(height, width):
    py, px = np.meshgrid(np.arange(height, dtype=np.int64), np.arange(width, dtype=np.int64), indexing="ij")
    return px, py


def disc_mask(px, py, X, Y, r):
    return (px - X) ** 2 + (py - Y) ** 2 <= r * r + r


def bone_mask(px, py, p0, p1, T):
    x0, y0, x1, y1 = (np.int64(v) for v in (*p0, *p1))
    dx, dy = x1 - x0, y1 - y0
    L2 = dx * dx + dy * dy
    wx, wy = px - x0, py - y0
    t = wx * dx + wy * dy
    T2 = np.int64(T * T)
    head = (t <= 0) & (4 * (wx * wx + wy * wy) <= T2)
    tail = (t >= L2) & (4 * ((px - x1) ** 2 + (py - y1) ** 2) <= T2)
    cross = wx * dy - wy * dx
    body = (t > 0) & (t < L2) & (4 * cross * cross <= T2 * L2)
    return head | tail | body


def primitives(pts, skeleton, point_colors, bone_colors, person_index, radius, thickness, threshold, px, py):
    """yields (mask, colour) in primitive order: person-major; bones k = 0..K-1, then joints j = 0..J-1"""
    point_colors, bone_colors = np.asarray(point_colors, np.uint8), np.asarray(bone_colors, np.uint8)
    for i, person in enumerate(pts):
        joints = live_joints(person, threshold)
        pid = i if person_index is None else int(person_index[i])
        for a, b in skeleton:
            if joints[a] is not None and joints[b] is not None:
                yield bone_mask(px, py, joints[a], joints[b], thickness), bone_colors[pid % len(bone_colors)]
        for j, p in enumerate(joints):
            if p is not None:
                yield disc_mask(px, py, p[0], p[1], radius), point_colors[j % len(point_colors)]


def paint(height, width, pts, skeleton, point_colors, bone_colors, person_index=None, radius=None, thickness=2, threshold=0.5):
    """(number (H, W) int64: the highest-numbered primitive on each pixel or -1, colour (H, W, 3) uint8 of that primitive)"""
    pts = np.asarray(pts, np.float32).reshape(-1, np.shape(pts)[-2], 3)
    radius = default_radius(height, width) if not radius else radius
    px, py = grid(height, width)
    number = np.full((height, width), -1, np.int64)
    colour = np.zeros((height, width, 3), np.uint8)
    for k, (mask, c) in enumerate(primitives(pts, skeleton, point_colors, bone_colors, person_index, radius, thickness, threshold, px, py)):
        number[mask] = k
        colour[mask] = c
    return number, colour


def draw_bgr(frame, pts, skeleton, point_colors, bone_colors, **kw):
    """draws into `frame` ((H, W, 3) uint8, any row stride) in place; only covered pixels are written"""
    number, colour = paint(frame.shape[0], frame.shape[1], pts, skeleton, point_colors, bone_colors, **kw)
    frame[number >= 0] = colour[number >= 0]
    return frame


def draw_yuv(data, height, width, fmt, pts, skeleton, point_colors, bone_colors, pitch=None, **kw):
    """draws into the rawvideo buffer `data` (yuv_ref.planes' layout) in place; colours are (Y, U, V)"""
    number, colour = paint(height, width, pts, skeleton, point_colors, bone_colors, **kw)
    Y, U, V = yuv_ref.planes(data, height, width, fmt, pitch)
    assert np.shares_memory(Y, data) and np.shares_memory(U, data) and np.shares_memory(V, data)
    Y[number >= 0] = colour[..., 0][number >= 0]
    for by in range(height // 2):
        for bx in range(width // 2):
            block = number[2 * by:2 * by + 2, 2 * bx:2 * bx + 2]
            if block.max() >= 0:
                dy, dx = np.unravel_index(int(block.argmax()), (2, 2))
                U[by, bx], V[by, bx] = colour[2 * by + dy, 2 * bx + dx, 1], colour[2 * by + dy, 2 * bx + dx, 2]
    return data


def draw_clip(frames, pts, frame_index, skeleton, point_colors, bone_colors, person_index=None, radius=None, **kw):
    """BGR frames of a clip: person i on frames[frame_index[i]], numbered in call order (person_index defaults to i)"""
    ids = np.arange(len(pts)) if person_index is None else np.asarray(person_index)
    for f, frame in enumerate(frames):
        who = [i for i in range(len(pts)) if frame_index[i] == f]
        if who:
            draw_bgr(frame, np.asarray(pts)[who], skeleton, point_colors, bone_colors, person_index=ids[who], radius=radius, **kw)
    return frames
