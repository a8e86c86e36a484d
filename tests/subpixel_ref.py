"""numpy restatement of the sub-pixel joint decoding contract (include/hrnet_mi355.h: HRN_REFINE_*), in float64.

Imported by tests/test_refine_host.py (the restatement itself, on CPU) and tests/test_refine_gpu.py (the engine against it)."""
import numpy as np

MODES = {"quarter": 1, "dark": 2}
# the 11-tap sigma-2 Gaussian, g[k] = exp(-k^2/8) / sum, k = -5..5 (cv2.getGaussianKernel(11, 0))
G = np.exp(-np.arange(-5, 6, dtype=np.float64) ** 2 / 8.0)
G /= G.sum()
# the 13 offsets (x, y) at which DARK needs the blurred map
POINTS = [(cx, cy) for cy in range(-2, 3) for cx in range(-2, 3) if abs(cx) + abs(cy) <= 2]


def argmax_xy(hm):
    """first maximum of one (h, w) map (np.argmax order) -> (px, py, value)"""
    i = int(np.argmax(hm))
    return i % hm.shape[1], i // hm.shape[1], hm.flat[i]


def quarter_offset(hm, px, py):
    h, w = hm.shape
    if 1 < px < w - 1 and 1 < py < h - 1:
        return (0.25 * float(np.sign(hm[py, px + 1] - hm[py, px - 1])),   # fp32 differences, as the map is stored
                0.25 * float(np.sign(hm[py + 1, px] - hm[py - 1, px])))
    return 0.0, 0.0


def dark_terms(hm, px, py):
    """the derivatives of L = ln(max(B, 1e-10)) at (px, py) and the unclamped Newton step, or None outside the interior"""
    h, w = hm.shape
    if not (2 <= px <= w - 3 and 2 <= py <= h - 3):
        return None
    pad = np.zeros((h + 14, w + 14))
    pad[7:-7, 7:-7] = hm                 # H counts as zero outside the map
    L = {}
    for cx, cy in POINTS:
        patch = pad[py + 7 + cy - 5:py + 7 + cy + 6, px + 7 + cx - 5:px + 7 + cx + 6]
        L[cx, cy] = np.log(np.maximum(G @ patch @ G, 1e-10))
    t = {"dx": (L[1, 0] - L[-1, 0]) / 2, "dy": (L[0, 1] - L[0, -1]) / 2,
         "dxx": (L[2, 0] - 2 * L[0, 0] + L[-2, 0]) / 4, "dyy": (L[0, 2] - 2 * L[0, 0] + L[0, -2]) / 4,
         "dxy": (L[1, 1] - L[1, -1] - L[-1, 1] + L[-1, -1]) / 4}
    t["det"] = t["dxx"] * t["dyy"] - t["dxy"] * t["dxy"]
    with np.errstate(divide="ignore", invalid="ignore"):
        t["sx"] = -(t["dyy"] * t["dx"] - t["dxy"] * t["dy"]) / t["det"]
        t["sy"] = -(t["dxx"] * t["dy"] - t["dxy"] * t["dx"]) / t["det"]
    return t


def dark_offset(hm, px, py):
    t = dark_terms(hm, px, py)
    if t is None or not (t["dxx"] < 0 and t["det"] > 0):
        return 0.0, 0.0
    return float(np.clip(t["sx"], -1.0, 1.0)), float(np.clip(t["sy"], -1.0, 1.0))


def offset(hm, px, py, mode):
    return {"quarter": quarter_offset, "dark": dark_offset}[mode](hm, px, py)


def borderline(hm, px, py, rel=1e-5):
    """a DARK joint whose result another evaluation order may legitimately change: an ill-conditioned Hessian (condition
    number > 1e3), or a definiteness / clamp decision within `rel` (relative) of its threshold"""
    t = dark_terms(hm, px, py)
    if t is None:
        return False
    dxx, dyy, dxy, det = t["dxx"], t["dyy"], t["dxy"], t["det"]
    scale = max(abs(dxx), abs(dyy), abs(dxy))
    if not np.isfinite(scale) or scale == 0:
        return False                     # a flat window: no offset however it is evaluated
    if abs(dxx) <= rel * scale or abs(det) <= rel * (abs(dxx * dyy) + dxy * dxy):
        return True
    if np.linalg.cond(np.array([[dxx, dxy], [dxy, dyy]])) > 1e3:
        return True
    if dxx < 0 and det > 0:
        return any(abs(abs(s) - 1.0) <= rel for s in (t["sx"], t["sy"]))
    return False


def decode(heatmaps, boxes, mode):
    """(n,J,h,w) float32 maps + (n,4) int32 / float32 boxes -> pts (n,J,3) float32 (y, x, confidence) as the engine's
    refined decode computes them: y = (py + oy) * 1. / h * (y2 - y1) + y1 in float64, the box difference in its own dtype"""
    n, nj, h, w = heatmaps.shape
    pts = np.empty((n, nj, 3), np.float32)
    for i in range(n):
        b = boxes[i]
        x1, y1, dxb, dyb = float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])
        for j in range(nj):
            px, py, v = argmax_xy(heatmaps[i, j])
            ox, oy = offset(heatmaps[i, j], px, py, mode) if mode else (0.0, 0.0)
            pts[i, j] = ((py + oy) * 1. / h * dyb + y1, (px + ox) * 1. / w * dxb + x1, v)
    return pts


def refine_coords(heatmaps, coords, mode):
    """hrn_refine_coords: integer-valued (x, y) in cells, refined; entries off the map are left as they are"""
    n, nj, h, w = heatmaps.shape
    out = np.array(coords, np.float32, copy=True)
    for i in range(n):
        for j in range(nj):
            x, y = out[i, j]
            if 0 <= x <= w - 1 and 0 <= y <= h - 1:
                ox, oy = offset(heatmaps[i, j], int(x), int(y), mode)
                out[i, j] = (np.float64(x) + ox, np.float64(y) + oy)
    return out


def gaussian_maps(n, h, w, rng, sigma=2.0, margin=8):
    """(n, h, w) float32 maps of one Gaussian each, centred at a fractional position >= margin cells from the border"""
    cx = rng.uniform(margin, w - 1 - margin, n)
    cy = rng.uniform(margin, h - 1 - margin, n)
    xs, ys = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    maps = np.exp(-((xs[None, None, :] - cx[:, None, None]) ** 2 + (ys[None, :, None] - cy[:, None, None]) ** 2) / (2 * sigma ** 2))
    return maps.astype(np.float32), cx, cy
