"""What a palette is: the colours ``draw_poses`` draws with, as (C, 3) uint8 arrays of (B, G, R) rows -- by matplotlib name, from
the stored tables of the demo programs, or converted to (Y, U, V) for ``YuvFrame``s.  ``native.palette`` caches ``find_palette``."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib
from .frames import YUV_MATRICES, YUV_RANGES

# The palettes of the reference's demo programs (scripts/live-demo.py, misc/visualization.py defaults) as (B, G, R) rows, kept
# here so that drawing works where matplotlib is not installed; tests/golden/palettes.json holds the reference's colours they
# (and palette()) are pinned to.  Listed palettes (tab20, Set2) ignore the sample count; sampled ones are keyed by it.
EMBEDDED_PALETTES = {
    ("tab20", None): [[180, 119, 31], [232, 199, 174], [14, 127, 255], [120, 187, 255], [44, 160, 44], [138, 223, 152], [40, 39, 214],
                      [150, 152, 255], [189, 103, 148], [213, 176, 197], [75, 86, 140], [148, 156, 196], [194, 119, 227], [210, 182, 247],
                      [127, 127, 127], [199, 199, 199], [34, 189, 188], [141, 219, 219], [207, 190, 23], [229, 218, 158]],
    ("Set2", None): [[165, 194, 102], [98, 141, 252], [203, 160, 141], [195, 138, 231], [84, 216, 166], [47, 217, 255], [148, 196, 229],
                     [179, 179, 179]],
    ("gist_rainbow", 10): [[41, 0, 255], [0, 110, 255], [0, 255, 249], [0, 255, 92], [59, 255, 0], [215, 255, 0], [255, 143, 0],
                           [255, 0, 14], [255, 0, 167], [191, 0, 255]],
    ("jet", 8): [[128, 0, 0], [255, 16, 0], [255, 164, 0], [183, 255, 64], [64, 255, 183], [0, 185, 255], [0, 48, 255], [0, 0, 128]],
}


def embedded_palette(name: str, samples: int) -> Optional[np.ndarray]:
    """the stored (C, 3) uint8 BGR table of a demo palette, or None"""
    rows = EMBEDDED_PALETTES.get((name, None)) or EMBEDDED_PALETTES.get((name, int(samples)))
    return None if rows is None else np.asarray(rows, np.uint8)


def find_palette(name: str, samples: int) -> np.ndarray:
    """the colours of ``native.palette(name, samples)``, looked up afresh: with matplotlib where it can be imported, else from the
    stored tables (ValueError for a name that is not stored)"""
    key = (str(name), int(samples))
    try:
        import matplotlib
    except ImportError:
        matplotlib = None
    if matplotlib is None:
        out = embedded_palette(*key)
        if out is None:
            raise ValueError("palette %r with %d samples is not stored and matplotlib is not installed" % key)
    else:
        registry = getattr(matplotlib, "colormaps", None)       # matplotlib >= 3.5; before that the lookup lived in matplotlib.cm
        if registry is None:
            from matplotlib import cm
            cmap = cm.get_cmap(key[0])
        elif key[0] in registry:
            cmap = registry[key[0]]
        else:
            raise ValueError("matplotlib has no palette %r" % key[0])
        listed = getattr(cmap, "colors", None)                   # a listed palette's own colours; a continuous one is sampled
        rgb = np.asarray(listed, np.float64) if listed is not None else np.asarray(cmap(np.linspace(0.0, 1.0, key[1])), np.float64)
        out = np.rint(rgb[:, :3] * 255.0).astype(np.uint8)[:, ::-1]   # 8 bits per channel, rounded half to even; R, G, B -> B, G, R
    return np.ascontiguousarray(out)


HEAT_COLORMAPS = ("jet", "hot", "gray")


def heat_colormap(name: str = "jet") -> np.ndarray:
    """The (256, 3) uint8 table of (B, G, R) rows ``draw_heatmaps`` colours a value 0..255 with, defined in integers (no matplotlib):

    ``"jet"``: for ``i`` in 0..255 and ``k`` = 3, 2, 1 for R, G, B: ``(clamp(765 - |8 i - 510 k|, 0, 510) + 1) >> 1`` -- dark blue,
    blue, cyan, yellow, red, dark red; ``"hot"``: for ``k`` = 0, 1, 2 for R, G, B: ``clamp(3 i - 255 k, 0, 255)`` -- black, red,
    yellow, white, each channel ramping over a third of the range after the one before is full; ``"gray"``: ``i`` in all three.
    For a ``YuvFrame`` the table goes through ``bgr_to_yuv_colors``.  Any other name raises ValueError."""
    i = np.arange(256, dtype=np.int64)
    if name == "jet":
        rgb = [(np.clip(765 - np.abs(8 * i - 510 * k), 0, 510) + 1) >> 1 for k in (3, 2, 1)]
    elif name == "hot":
        rgb = [np.clip(3 * i - 255 * k, 0, 255) for k in (0, 1, 2)]
    elif name == "gray":
        rgb = [i, i, i]
    else:
        raise ValueError("colormap must be one of %s or a (256, 3) uint8 array, got %r" % (", ".join(repr(n) for n in HEAT_COLORMAPS), name))
    return np.ascontiguousarray(np.stack(rgb[::-1], 1).astype(np.uint8))   # R, G, B -> B, G, R


def bgr_to_yuv_colors(colors, matrix: str = "bt601", range: str = "limited") -> np.ndarray:  # noqa: A002
    """(C, 3) uint8 (B, G, R) colours as (Y, U, V) of a matrix and range (``hrn_yuv_from_bgr``: the float64 forward formula of the
    conversion ``YuvFrame``s are read with, rounded once): what ``draw_poses`` draws with on a ``YuvFrame``."""
    if matrix not in YUV_MATRICES or range not in YUV_RANGES:
        raise ValueError("matrix must be 'bt601' or 'bt709' and range 'limited' or 'full', got %r, %r" % (matrix, range))
    c = np.ascontiguousarray(np.asarray(colors, dtype=np.uint8).reshape(-1, 3))
    out = np.empty_like(c)
    rc = _lib.load().hrn_yuv_from_bgr(YUV_MATRICES[matrix], YUV_RANGES[range], c.ctypes.data, len(c), out.ctypes.data)
    if rc != 0:
        raise RuntimeError("hrn_yuv_from_bgr failed (%d)" % rc)
    return out
