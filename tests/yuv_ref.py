"""numpy restatement of the YUV -> BGR conversion of include/hrnet_mi355.h (hrn_yuv_coefficients, hrn_yuv_to_bgr and the YUV
crop pre-path): cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420)'s form -- the chroma sample of a 2x2 block shared by its pixels, 20-bit
fixed point in int32, arithmetic shift.

    yy = max(0, Y - y0) * CY;  u = U - 128;  v = V - 128;  h = 1 << 19
    B = clip8((yy + h + CUB*u) >> 20);  G = clip8((yy + h + CVG*v + CUG*u) >> 20);  R = clip8((yy + h + CVR*v) >> 20)

Test infrastructure, beside warp_affine_ref.py: the GPU tests hold the kernels to this file bit for bit."""
import numpy as np

SHIFT = 20

# (y0, CY, CUB, CUG, CVG, CVR).  BT.601 limited: OpenCV's published constants, verbatim; the others floor(x * 2^20 + 0.5)
TABLES = {
    ("bt601", "limited"): (16, 1220542, 2116026, -409993, -852492, 1673527),
    ("bt601", "full"): (0, 1048576, 1858077, -360853, -748826, 1470104),
    ("bt709", "limited"): (16, 1220945, 2215014, -223607, -558796, 1879825),
    ("bt709", "full"): (0, 1048576, 1945738, -196424, -490864, 1651297),
}
MATRICES = {"bt601": 0, "bt709": 1}
RANGES = {"limited": 0, "full": 1}


def exact_coefficients(matrix, range_):
    """(y0, luma scale, B per u, G per u, G per v, R per v) as real numbers: what the tables quantise"""
    kr, kb = (0.299, 0.114) if matrix == "bt601" else (0.2126, 0.0722)
    kg = 1.0 - kr - kb
    sy, sc = (255.0 / 219.0, 255.0 / 224.0) if range_ == "limited" else (1.0, 1.0)
    return (16 if range_ == "limited" else 0, sy, 2 * (1 - kb) * sc, -2 * (1 - kb) * kb / kg * sc, -2 * (1 - kr) * kr / kg * sc,
            2 * (1 - kr) * sc)


def derived_table(matrix, range_):
    y0, *x = exact_coefficients(matrix, range_)
    return (y0,) + tuple(int(np.floor(v * (1 << SHIFT) + 0.5)) for v in x)


def convert(Y, U, V, table):
    """uint8 arrays of one shape -> (B, G, R) uint8 arrays; every intermediate is int32, as on the device"""
    y0, cy, cub, cug, cvg, cvr = (np.int32(c) for c in table)
    yy = np.maximum(Y.astype(np.int32) - y0, 0) * cy + np.int32(1 << (SHIFT - 1))
    u, v = U.astype(np.int32) - 128, V.astype(np.int32) - 128
    b = (yy + cub * u) >> SHIFT
    g = (yy + cvg * v + cug * u) >> SHIFT
    r = (yy + cvr * v) >> SHIFT
    assert b.dtype == g.dtype == r.dtype == np.int32
    return tuple(np.clip(c, 0, 255).astype(np.uint8) for c in (b, g, r))


def convert_float(Y, U, V, matrix, range_):
    """clip(rint(float64 formula)) with max(0, Y - y0): what the fixed-point form approximates"""
    y0, sy, cub, cug, cvg, cvr = exact_coefficients(matrix, range_)
    yy = np.maximum(Y.astype(np.float64) - y0, 0.0) * sy
    u, v = U.astype(np.float64) - 128.0, V.astype(np.float64) - 128.0
    return tuple(np.clip(np.rint(c), 0, 255).astype(np.uint8) for c in (yy + cub * u, yy + cug * u + cvg * v, yy + cvr * v))


def planes(data, height, width, fmt, pitch=None):
    """(Y (h, w), U (h/2, w/2), V (h/2, w/2)) views of a rawvideo buffer: `height` rows of `pitch` bytes of Y, then
    nv12: height/2 rows of `pitch` bytes of interleaved U, V; i420: height/2 rows of pitch/2 bytes of U, then of V"""
    pitch = width if pitch is None else pitch
    data = np.asarray(data, np.uint8).reshape(-1)
    h2, w2 = height // 2, width // 2
    Y = data[:pitch * height].reshape(height, pitch)[:, :width]
    c = data[pitch * height:pitch * height * 3 // 2]
    if fmt == "nv12":
        uv = c.reshape(h2, pitch)[:, :width].reshape(h2, w2, 2)
        return Y, uv[:, :, 0], uv[:, :, 1]
    pc = pitch // 2
    return Y, c[:pc * h2].reshape(h2, pc)[:, :w2], c[pc * h2:].reshape(h2, pc)[:, :w2]


def yuv_to_bgr(data, height, width, fmt="nv12", matrix="bt601", range_="limited", pitch=None):
    """(height, width, 3) uint8 BGR of a rawvideo NV12 / I420 buffer"""
    Y, U, V = planes(data, height, width, fmt, pitch)
    U, V = (np.repeat(np.repeat(c, 2, 0), 2, 1) for c in (U, V))   # nearest: a 2x2 block shares its chroma sample
    return np.ascontiguousarray(np.stack(convert(Y, U, V, TABLES[(matrix, range_)]), -1))


def nbytes(height, width, pitch=None):
    return (width if pitch is None else pitch) * height * 3 // 2
