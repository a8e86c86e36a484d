"""numpy restatement of the three layouts beside NV12 / I420 (include/hrnet_mi355.h: HRN_PIX_NV21, HRN_PIX_P010, HRN_PIX_I010):
sample extraction, the 10-bit conversion in exact integers, plane views and packers.  The 8-bit arithmetic is yuv_ref.py's.

    P010: s = word >> 6 (the low six bits are ignored)        I010: s = word & 1023 (the high six bits are ignored)
    yy = max(0, Y - 4*y0) * CY;  u = U - 512;  v = V - 512;  h = 1 << 21
    B = clip8((yy + h + CUB*u) >> 22);  G = clip8((yy + h + CVG*v + CUG*u) >> 22);  R = clip8((yy + h + CVR*v) >> 22)

The sums do not fit int32 (BT.709 limited: yy + h + CUB*u reaches 2 304 855 561): everything here is int64.
Test infrastructure, beside yuv_ref.py: the GPU tests hold the kernels to this file bit for bit."""
import numpy as np

import yuv_ref
from yuv_ref import MATRICES, RANGES, TABLES  # noqa: F401

SHIFT = 22
FORMATS = {"nv21": 4, "p010": 5, "i010": 6}
TEN_BIT = ("p010", "i010")


def frame(pkg, data, height, width, fmt, matrix="bt601", range_="limited", pitch=None):
    """the package's ``YuvFrame`` of a buffer of layout `fmt`, this file's names: NV21 is its "nv12" with chroma_order="vu\""""
    if fmt == "nv21":
        return pkg.YuvFrame(data, height, width, "nv12", matrix, range_, pitch, chroma_order="vu")
    return pkg.YuvFrame(data, height, width, fmt, matrix, range_, pitch)


def clone(pkg, f, data):
    """frame `f` over other bytes (a pinned or device-resident copy of its own)"""
    return pkg.YuvFrame(data, f.height, f.width, f.format, f.matrix, f.range, f.pitch, chroma_order=f.chroma_order)


def layout(f):
    """this file's name of the layout of a ``YuvFrame``"""
    return "nv21" if f.chroma_order == "vu" else f.format


def sample_bytes(fmt):
    return 2 if fmt in TEN_BIT else 1


def samples(words, fmt):
    """the 10-bit samples of uint16 words of a `fmt` plane"""
    words = np.asarray(words, np.uint16)
    return words >> 6 if fmt == "p010" else words & 1023


def convert10(Y, U, V, table):
    """arrays of one shape of 10-bit samples -> (B, G, R) uint8 arrays; every intermediate is int64"""
    y0, cy, cub, cug, cvg, cvr = (np.int64(c) for c in table)
    yy = np.maximum(Y.astype(np.int64) - 4 * y0, 0) * cy + np.int64(1 << (SHIFT - 1))
    u, v = U.astype(np.int64) - 512, V.astype(np.int64) - 512
    b = (yy + cub * u) >> SHIFT
    g = (yy + cvg * v + cug * u) >> SHIFT
    r = (yy + cvr * v) >> SHIFT
    assert b.dtype == g.dtype == r.dtype == np.int64
    return tuple(np.clip(c, 0, 255).astype(np.uint8) for c in (b, g, r))


def convert10_float(Y, U, V, matrix, range_):
    """clip(rint(float64 formula)) of 10-bit samples, 8-bit result: yuv_ref.convert_float's formula on s / 4"""
    y0, sy, cub, cug, cvg, cvr = yuv_ref.exact_coefficients(matrix, range_)
    yy = np.maximum(Y.astype(np.float64) / 4.0 - y0, 0.0) * sy
    u, v = (U.astype(np.float64) - 512.0) / 4.0, (V.astype(np.float64) - 512.0) / 4.0
    return tuple(np.clip(np.rint(c), 0, 255).astype(np.uint8) for c in (yy + cub * u, yy + cug * u + cvg * v, yy + cvr * v))


def row_bytes(width, fmt):
    return width * sample_bytes(fmt)


def nbytes(height, width, fmt, pitch=None):
    return (row_bytes(width, fmt) if pitch is None else pitch) * height * 3 // 2


def planes(data, height, width, fmt, pitch=None):
    """(Y (h, w), U (h/2, w/2), V (h/2, w/2)) views of a rawvideo buffer of bytes -- uint8 samples for nv21, uint16 WORDS (not yet
    samples) for p010 / i010: `height` rows of `pitch` bytes of Y, then nv21 / p010: height/2 rows of `pitch` bytes of interleaved
    (V, U) bytes / (U, V) words; i010: height/2 rows of pitch/2 bytes of U words, then of V"""
    pitch = row_bytes(width, fmt) if pitch is None else pitch
    data = np.asarray(data, np.uint8).reshape(-1)
    h2, w2 = height // 2, width // 2
    luma, c = data[:pitch * height].reshape(height, pitch), data[pitch * height:pitch * height * 3 // 2]
    if fmt == "nv21":
        vu = c.reshape(h2, pitch)[:, :width].reshape(h2, w2, 2)
        return luma[:, :width], vu[:, :, 1], vu[:, :, 0]
    assert pitch % 2 == 0
    Y = luma.view("<u2")[:, :width]
    if fmt == "p010":
        uv = c.reshape(h2, pitch).view("<u2")[:, :width].reshape(h2, w2, 2)
        return Y, uv[:, :, 0], uv[:, :, 1]
    assert fmt == "i010" and pitch % 4 == 0
    pc = pitch // 2
    return Y, c[:pc * h2].reshape(h2, pc).view("<u2")[:, :w2], c[pc * h2:].reshape(h2, pc).view("<u2")[:, :w2]


def yuv_to_bgr(data, height, width, fmt, matrix="bt601", range_="limited", pitch=None):
    """(height, width, 3) uint8 BGR of a rawvideo NV21 / P010 / I010 buffer"""
    Y, U, V = planes(data, height, width, fmt, pitch)
    U, V = (np.repeat(np.repeat(c, 2, 0), 2, 1) for c in (U, V))   # nearest: a 2x2 block shares its chroma sample
    table = TABLES[(matrix, range_)]
    if fmt == "nv21":
        out = yuv_ref.convert(Y, U, V, table)
    else:
        out = convert10(samples(Y, fmt), samples(U, fmt), samples(V, fmt), table)
    return np.ascontiguousarray(np.stack(out, -1))


def pack(Y, U, V, fmt, pitch=None, junk=None, fill=0xA5):
    """rawvideo bytes of `fmt` from sample arrays Y (h, w), U and V (h/2, w/2): uint8 for nv12 / nv21 / i420, 10-bit values for
    p010 / i010.  `junk`: a numpy Generator that sets the six ignored bits of every word at random (default: zero).  `pitch`:
    bytes between rows (default: packed); pitch bytes hold `fill`."""
    def words(s):
        s = np.asarray(s).astype(np.uint16)
        assert int(s.max(initial=0)) < 1024
        extra = junk.integers(0, 64, s.shape, dtype=np.uint16) if junk is not None else np.zeros(s.shape, np.uint16)
        return ((s << 6) | extra) if fmt == "p010" else (s | (extra << 10))

    if fmt in TEN_BIT:
        Y, U, V = words(Y), words(U), words(V)
    return pack_elements(Y, U, V, fmt, pitch, fill)


def pack_elements(Y, U, V, fmt, pitch=None, fill=0xA5):
    """rawvideo bytes of `fmt` from its planes as they are stored: uint8 samples, or whole uint16 WORDS for p010 / i010"""
    h, w = Y.shape
    h2, w2 = h // 2, w // 2
    assert U.shape == V.shape == (h2, w2)
    bps = sample_bytes(fmt)
    pitch = w * bps if pitch is None else pitch
    out = np.full(pitch * h * 3 // 2, fill, np.uint8)
    luma, c = out[:pitch * h].reshape(h, pitch), out[pitch * h:]
    words = lambda s: np.asarray(s, np.uint16)   # noqa: E731

    if bps == 1:
        luma[:, :w] = Y
        if fmt in ("nv12", "nv21"):
            pair = (U, V) if fmt == "nv12" else (V, U)
            c.reshape(h2, pitch)[:, :w] = np.stack(pair, -1).reshape(h2, w)
        else:
            pc = pitch // 2
            c[:pc * h2].reshape(h2, pc)[:, :w2], c[pc * h2:].reshape(h2, pc)[:, :w2] = U, V
        return out
    luma.view("<u2")[:, :w] = words(Y)
    if fmt == "p010":
        c.reshape(h2, pitch).view("<u2")[:, :w] = np.stack([words(U), words(V)], -1).reshape(h2, w)
    else:
        pc = pitch // 2
        c[:pc * h2].reshape(h2, pc).view("<u2")[:, :w2] = words(U)
        c[pc * h2:].reshape(h2, pc).view("<u2")[:, :w2] = words(V)
    return out


def random_samples(rng, height, width, fmt):
    """random sample planes of a `fmt` frame: every value of the format's range"""
    top = 1024 if fmt in TEN_BIT else 256
    dt = np.uint16 if fmt in TEN_BIT else np.uint8
    return (rng.integers(0, top, (height, width)).astype(dt), rng.integers(0, top, (height // 2, width // 2)).astype(dt),
            rng.integers(0, top, (height // 2, width // 2)).astype(dt))


def any_yuv_to_bgr(data, height, width, fmt, matrix="bt601", range_="limited", pitch=None):
    """yuv_to_bgr for all five layouts"""
    if fmt in ("nv12", "i420"):
        return yuv_ref.yuv_to_bgr(data, height, width, fmt, matrix, range_, pitch)
    return yuv_to_bgr(data, height, width, fmt, matrix, range_, pitch)
