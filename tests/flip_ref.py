"""Flip test-time augmentation restated in plain numpy: what the tests hold ``predict_flip_tta`` to (test infrastructure only).

Written from the reference's own loops (``misc/utils.py:19-29`` flip_back, ``:125-151`` get_max_preds, ``:160-175`` the
post-processing of get_final_preds, ``testing/Test.py:132-140`` the average), not from the engine: the in-place swaps are
performed one pair after the other, there is no composed ``pair[]`` table here.

Everything is float32: the combine is one fp32 addition and one multiplication by 0.5 (exact), so a kernel that computes the same
two passes has to give the same bits."""
import math

import numpy as np

COCO_PAIRS = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]
SHARED_PAIRS = [(1, 2), (2, 3), (5, 6), (5, 6), (0, 16)]     # (1,2),(2,3) is a 3-cycle; (5,6) twice is the identity


def flip_back(b, pairs):
    """``flip_back(output_flipped, matched_parts)``: mirror the last axis, then swap maps p0 <-> p1 in place, pair after pair."""
    out = np.array(np.asarray(b)[..., ::-1], copy=True)
    assert out.ndim == 4
    for p0, p1 in np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist():
        tmp = out[:, p0].copy()
        out[:, p0] = out[:, p1]
        out[:, p1] = tmp
    return out


def flip_tta_expected(a, b, pairs):
    """``(model(x) + flip_back(model(flip(x)), pairs)) * 0.5`` from the two plain passes ``a`` and ``b``, float32 throughout."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    with np.errstate(invalid="ignore"):                      # (inf + -inf, NaN maps: the adversarial cases)
        out = (a + flip_back(b, pairs)) * np.float32(0.5)
    assert out.dtype == np.float32
    return out


def max_preds(hm, post_processing=True):
    """``get_max_preds`` (first maximum of the flattened map, a NaN is a maximum; coordinates zeroed unless maxval > 0) and, with
    ``post_processing``, get_final_preds's quarter cell towards the higher neighbour: preds (n,J,2) = (x, y), maxvals (n,J,1).

    Out of scope: a map that holds +inf next to its maximum makes ``sign(inf - inf)`` NaN in numpy / torch, while the kernel
    steps by 0 there; no test constructs such a map."""
    hm = np.asarray(hm)
    n, nj, h, w = hm.shape
    preds = np.zeros((n, nj, 2), np.float32)
    maxvals = np.zeros((n, nj, 1), np.float32)
    for i in range(n):
        for j in range(nj):
            m = hm[i, j]
            idx = int(np.argmax(m))                          # np.argmax: first maximum, first NaN if there is one
            v = m.reshape(-1)[idx]
            maxvals[i, j, 0] = v
            if v > 0.0:
                preds[i, j] = (idx % w, idx // w)
            if post_processing:
                px, py = int(math.floor(preds[i, j, 0] + 0.5)), int(math.floor(preds[i, j, 1] + 0.5))
                if 1 < px < w - 1 and 1 < py < h - 1:
                    preds[i, j, 0] += np.sign(m[py, px + 1] - m[py, px - 1]) * np.float32(0.25)
                    preds[i, j, 1] += np.sign(m[py + 1, px] - m[py - 1, px]) * np.float32(0.25)
    return preds, maxvals


def symmetric_crops(x):
    """left half of each crop followed by its own mirror image: the crop equals its mirror image exactly"""
    x = np.asarray(x)
    half = x[..., : x.shape[-1] // 2]
    return np.ascontiguousarray(np.concatenate([half, half[..., ::-1]], axis=-1))
