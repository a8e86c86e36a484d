"""numpy restatement of the label definition of include/hrnet_mi355.h (hrn_draw_labels_dev), written from the header's text: int64
throughout, one full-frame mask per primitive (outline, plate, ink) and a plain painter's loop in primitive order -- no tiles, no
records, no culling.  Test infrastructure, beside draw_ref.py: the host tests hold hrn_label_layout / hrn_label_covers to this
file pixel for pixel, the GPU tests the kernels byte for byte."""
import numpy as np

import yuv_ref
from draw_ref import grid

LO, HI = -8192, 16383
GLYPHS = {d: [int(b, 16) for b in row.split()] for d, row in enumerate([
    "0E 11 13 15 19 11 0E", "04 0C 04 04 04 04 0E", "0E 11 01 02 04 08 1F", "1F 02 04 02 01 11 0E", "02 06 0A 12 1F 02 02",
    "1F 10 1E 01 01 11 0E", "06 08 10 1E 11 11 0E", "1F 01 02 04 08 08 08", "0E 11 11 0E 11 11 0E", "0E 11 11 0F 01 02 0C"])}
BLANK = None


def default_scale(height, width):
    return min(16, max(1, min(height, width) // 360))


def percent(score):
    """p of a score, or None for NaN: two float32 operations, each rounded once"""
    v = np.float32(score)
    if np.isnan(v):
        return None
    v = np.float32(0) if v < 0 else (np.float32(1) if v > 1 else v)
    return int(np.float32(np.float32(v * np.float32(100.0)) + np.float32(0.5)))


def cells(person_id=None, score=None):
    """the row of cells: digits (ints) and BLANK"""
    out = []
    if person_id is not None and int(person_id) >= 0:
        out += [int(ch) for ch in str(int(person_id))]
    p = None if score is None else percent(score)
    if p is not None:
        out += ([BLANK] if out else []) + [int(ch) for ch in str(p)]
    assert len(out) <= 14
    return out


def is_drawn(box):
    x1, y1, x2, y2 = (int(v) for v in box)
    return all(LO <= v <= HI for v in (x1, y1, x2, y2)) and x2 > x1 and y2 > y1


def plate_rect(box, ncells, s):
    """(left, top, width, height) of the plate of a drawn box with ncells > 0 cells"""
    x1, y1 = int(box[0]), int(box[1])
    return x1, (y1 - 9 * s if y1 - 9 * s >= 0 else y1), s * (6 * ncells + 1), 9 * s


def outline_mask(px, py, box, T):
    x1, y1, x2, y2 = (np.int64(v) for v in box)
    if T == 0:
        return np.zeros(px.shape, bool)
    outer = (x1 <= px) & (px <= x2) & (y1 <= py) & (py <= y2)
    inner = (x1 + T <= px) & (px <= x2 - T) & (y1 + T <= py) & (py <= y2 - T)
    return outer & ~inner


def plate_mask(px, py, rect):
    left, top, width, height = rect
    return (left <= px) & (px < left + width) & (top <= py) & (py < top + height)


def ink_mask(px, py, rect, row, s):
    left, top = rect[:2]
    mask = np.zeros(px.shape, bool)
    for k, d in enumerate(row):
        if d is BLANK:
            continue
        u, v = px - left - s * (1 + 6 * k), py - top - s
        inside = (0 <= u) & (u < 5 * s) & (0 <= v) & (v < 7 * s)
        glyph = np.asarray(GLYPHS[d], np.int64)
        bits = (glyph[np.clip(v // s, 0, 6)] >> (4 - np.clip(u // s, 0, 4))) & 1
        mask |= inside & (bits == 1)
    return mask


def person_primitives(px, py, box, person_id, score, s, T):
    """[(mask, kind)] of one person in primitive order: kind 1 = the person's colour, 2 = the text colour"""
    if not is_drawn(box):
        return []
    out = [(outline_mask(px, py, box, T), 1)]
    row = cells(person_id, score)
    if row:
        rect = plate_rect(box, len(row), s)
        out += [(plate_mask(px, py, rect), 1), (ink_mask(px, py, rect, row, s), 2)]
    return out


def paint(height, width, boxes, colors, text_colors, person_ids=None, scores=None, scale=None, thickness=2, colour_index=None):
    """(number (H, W) int64: the highest-numbered primitive on each pixel or -1, colour (H, W, 3) uint8 of that primitive);
    colour_index: the i of each person in its call, when `boxes` is a part of one (only read without ids)"""
    boxes = np.asarray(boxes, np.int64).reshape(-1, 4)
    colors, text_colors = np.asarray(colors, np.uint8), np.asarray(text_colors, np.uint8)
    assert len(colors) == len(text_colors)
    s = default_scale(height, width) if not scale else scale
    px, py = grid(height, width)
    number = np.full((height, width), -1, np.int64)
    colour = np.zeros((height, width, 3), np.uint8)
    for i, box in enumerate(boxes):
        c = ((i if colour_index is None else int(colour_index[i])) if person_ids is None else int(person_ids[i])) % len(colors)   # Python's modulo
        prims = person_primitives(px, py, box, None if person_ids is None else person_ids[i], None if scores is None else scores[i],
                                  s, thickness)
        for k, (mask, kind) in enumerate(prims):
            number[mask] = 3 * i + k
            colour[mask] = colors[c] if kind == 1 else text_colors[c]
    return number, colour


def draw_bgr(frame, boxes, colors, text_colors, **kw):
    """draws into `frame` ((H, W, 3) uint8, any row stride) in place; only covered pixels are written"""
    number, colour = paint(frame.shape[0], frame.shape[1], boxes, colors, text_colors, **kw)
    frame[number >= 0] = colour[number >= 0]
    return frame


def draw_yuv(data, height, width, fmt, boxes, colors, text_colors, pitch=None, **kw):
    """draws into the rawvideo buffer `data` (yuv_ref.planes' layout) in place; colours are (Y, U, V)"""
    number, colour = paint(height, width, boxes, colors, text_colors, **kw)
    Y, U, V = yuv_ref.planes(data, height, width, fmt, pitch)
    assert np.shares_memory(Y, data) and np.shares_memory(U, data) and np.shares_memory(V, data)
    Y[number >= 0] = colour[..., 0][number >= 0]
    blocks = number.reshape(height // 2, 2, width // 2, 2).transpose(0, 2, 1, 3).reshape(height // 2, width // 2, 4)
    for by, bx in zip(*np.nonzero(blocks.max(-1) >= 0)):
        dy, dx = divmod(int(blocks[by, bx].argmax()), 2)
        U[by, bx], V[by, bx] = colour[2 * by + dy, 2 * bx + dx, 1], colour[2 * by + dy, 2 * bx + dx, 2]
    return data


def draw_clip(frames, boxes, frame_index, colors, text_colors, person_ids=None, scores=None, **kw):
    """BGR frames of a clip: person i on frames[frame_index[i]], numbered in call order (without ids the colour index is i)"""
    boxes = np.asarray(boxes)
    for f, frame in enumerate(frames):
        who = [i for i in range(len(boxes)) if frame_index[i] == f]
        if who:
            draw_bgr(frame, boxes[who], colors, text_colors, person_ids=None if person_ids is None else np.asarray(person_ids)[who],
                     scores=None if scores is None else np.asarray(scores)[who], colour_index=who, **kw)
    return frames
