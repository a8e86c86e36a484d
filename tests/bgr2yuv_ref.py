"""numpy restatement of the BGR -> 4:2:0 YCbCr conversion of include/hrnet_mi355.h (hrn_yuv_forward_coefficients,
hrn_bgr_to_yuv_blocks, hrn_bgr_to_yuv_frames), written from the definition, not from csrc/yuv_fwd.h:

    table   y0, (CYR CYG CYB), (CUR CUG CUB), (CVR CVG CVB) at scale 2^20, q(x) = floor(x 2^20 + 0.5) of the exact forward
            coefficients; CUB = -(CUR + CUG), CVR = -(CVG + CVB): a chroma row sums to zero
    8 bit   Y = clip8 ((CY . (R, G, B)    + (y0 << 20)  + (1 << 19)) >> 20)   per pixel
            U = clip8 ((CU . (Rs, Gs, Bs) + (128 << 22) + (1 << 21)) >> 22)   per 2x2 block, from the SUMS of its four pixels
    10 bit  Y = clip10((CY . (R, G, B)    + (y0 << 20)  + (1 << 17)) >> 18)
            U = clip10((CU . (Rs, Gs, Bs) + (128 << 22) + (1 << 19)) >> 20)   V likewise
    P010 stores s << 6, I010 stores s; NV21 is NV12 with the pair written (V, U)

Everything is int64 here and every sum is CHECKED to fit int32, which is what the library computes in.
Test infrastructure, beside yuv_ref.py: the tests hold the host form and the kernel to this file bit for bit."""
import numpy as np

SCALE = 1 << 20
PRIMARIES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
MATRICES = {"bt601": 0, "bt709": 1}
RANGES = {"limited": 0, "full": 1}
LAYOUTS = {"nv12": 1, "i420": 2, "nv21": 4, "p010": 5, "i010": 6}   # HRN_PIX_*
TEN_BIT = ("p010", "i010")
PLANAR = ("i420", "i010")
INT32_MAX = (1 << 31) - 1


def q(x):
    return int(np.floor(x * SCALE + 0.5))


def table(matrix, range_):
    """(y0, CYR, CYG, CYB, CUR, CUG, CUB, CVR, CVG, CVB) as Python ints"""
    kr, kb = PRIMARIES[matrix]
    kg = 1.0 - kr - kb
    sy, sc, y0 = (219.0 / 255.0, 224.0 / 255.0, 16) if range_ == "limited" else (1.0, 1.0, 0)
    cur, cug = q(-sc * kr / (2.0 * (1.0 - kb))), q(-sc * kg / (2.0 * (1.0 - kb)))
    cvg, cvb = q(-sc * kg / (2.0 * (1.0 - kr))), q(-sc * kb / (2.0 * (1.0 - kr)))
    return (y0, q(sy * kr), q(sy * kg), q(sy * kb), cur, cug, -(cur + cug), -(cvg + cvb), cvg, cvb)


def _fits(s):
    assert int(np.min(s, initial=0)) >= -INT32_MAX - 1 and int(np.max(s, initial=0)) <= INT32_MAX, "a sum leaves int32"
    return s


def luma_raw(t, depth, r, g, b):
    """the luma of pixels BEFORE the clip (int64): what shows whether a clip engages"""
    r, g, b = (np.asarray(c).astype(np.int64) for c in (r, g, b))
    s = _fits(_fits(t[1] * r + t[2] * g + t[3] * b + (t[0] << 20)) + (1 << (19 if depth == 8 else 17)))
    return s >> (20 if depth == 8 else 18)


def chroma_raw(row, depth, rs, gs, bs):
    """a chroma sample from the SUMS over a 2x2 block, before the clip; row = (CUR, CUG, CUB) or (CVR, CVG, CVB)"""
    rs, gs, bs = (np.asarray(c).astype(np.int64) for c in (rs, gs, bs))
    s = _fits(_fits(row[0] * rs + row[1] * gs + row[2] * bs + (128 << 22)) + (1 << (21 if depth == 8 else 19)))
    return s >> (22 if depth == 8 else 20)


def clip(v, depth):
    return np.clip(v, 0, 255 if depth == 8 else 1023).astype(np.uint16)


def blocks(bgr, t, depth):
    """(n, 4, 3) uint8 -- the (B, G, R) of a 2x2 block's pixels, row-major -- to (n, 6) uint16 Y00 Y01 Y10 Y11 U V sample values"""
    bgr = np.asarray(bgr, np.uint8).reshape(-1, 4, 3).astype(np.int64)
    b, g, r = bgr[:, :, 0], bgr[:, :, 1], bgr[:, :, 2]
    out = np.empty((len(bgr), 6), np.uint16)
    out[:, :4] = clip(luma_raw(t, depth, r, g, b), depth)
    rs, gs, bs = r.sum(1), g.sum(1), b.sum(1)
    out[:, 4] = clip(chroma_raw(t[4:7], depth, rs, gs, bs), depth)
    out[:, 5] = clip(chroma_raw(t[7:10], depth, rs, gs, bs), depth)
    return out


def samples(bgr, matrix, range_, depth):
    """an (H, W, 3) uint8 BGR frame of even sides to sample planes Y (H, W), U and V (H/2, W/2), uint16"""
    bgr = np.asarray(bgr, np.uint8)
    h, w = bgr.shape[:2]
    assert h % 2 == 0 and w % 2 == 0 and bgr.shape[2] == 3
    t = table(matrix, range_)
    b, g, r = (bgr[:, :, k].astype(np.int64) for k in range(3))
    Y = clip(luma_raw(t, depth, r, g, b), depth)
    rs, gs, bs = (c.reshape(h // 2, 2, w // 2, 2).sum((1, 3)) for c in (r, g, b))
    return Y, clip(chroma_raw(t[4:7], depth, rs, gs, bs), depth), clip(chroma_raw(t[7:10], depth, rs, gs, bs), depth)


def write_frame(buf, bgr, fmt, matrix, range_, y_off, pitch_y, u_off, pitch_c, v_off=None):
    """the sample bytes of `bgr` in layout `fmt` into the flat uint8 array `buf`, whose other bytes stay: Y rows pitch_y bytes
    apart from y_off; chroma rows pitch_c apart from u_off (nv12 / nv21 / p010: interleaved pairs) and v_off (i420 / i010)"""
    ten = fmt in TEN_BIT
    Y, U, V = samples(bgr, matrix, range_, 10 if ten else 8)
    if fmt == "p010":
        Y, U, V = Y << 6, U << 6, V << 6

    def put(off, pitch, plane):
        rows = (plane.astype("<u2") if ten else plane.astype(np.uint8)).reshape(plane.shape[0], -1).view(np.uint8)
        for i, row in enumerate(rows):
            buf[off + i * pitch:off + i * pitch + len(row)] = row

    put(y_off, pitch_y, Y)
    if fmt in PLANAR:
        put(u_off, pitch_c, U)
        put(v_off, pitch_c, V)
    else:
        put(u_off, pitch_c, np.stack((V, U) if fmt == "nv21" else (U, V), -1).reshape(U.shape[0], -1))
    return buf


def packed(bgr, fmt, matrix="bt601", range_="limited"):
    """the rawvideo bytes of `bgr` in layout `fmt`, no pitch padding: Y, then the chroma plane(s)"""
    h, w = np.asarray(bgr).shape[:2]
    pitch = w * (2 if fmt in TEN_BIT else 1)
    pitch_c = pitch // 2 if fmt in PLANAR else pitch
    buf = np.zeros(pitch * h * 3 // 2, np.uint8)
    return write_frame(buf, bgr, fmt, matrix, range_, 0, pitch, pitch * h, pitch_c, pitch * h + pitch_c * (h // 2))


def float_formula(matrix, range_, r, g, b):
    """hrn_yuv_from_bgr's float64 forward formula, each clip8(rint(.)): (Y, U, V) uint8"""
    kr, kb = PRIMARIES[matrix]
    kg = 1.0 - kr - kb
    y0, sy, sc = (16.0, 219.0 / 255.0, 224.0 / 255.0) if range_ == "limited" else (0.0, 1.0, 1.0)
    r, g, b = (np.asarray(c, np.float64) for c in (r, g, b))
    lum = kr * r + kg * g + kb * b
    c8 = lambda v: np.clip(np.rint(v), 0, 255).astype(np.uint8)   # noqa: E731
    return c8(y0 + sy * lum), c8(128.0 + sc * (b - lum) / (2.0 * (1.0 - kb))), c8(128.0 + sc * (r - lum) / (2.0 * (1.0 - kr)))
