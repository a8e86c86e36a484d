"""NV21 and 10-bit (P010 / I010) input without a GPU: the two properties of the 10-bit conversion (tests/yuv10_ref.py) -- it
contains the 8-bit conversion bit for bit, and it is within one grey level of the rounded float64 formula -- for all four tables;
``YuvFrame``'s layouts and refusals for the three formats; every new refusal of the C ABI on a plan-only handle."""
import ctypes
import os
import re

import numpy as np
import pytest

import yuv10_ref
import yuv_ref
from conftest import load_pkg

TABLE_KEYS = [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")]
IDS = ["%s-%s" % k for k in TABLE_KEYS]


# ---------------------------------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize("key", TABLE_KEYS, ids=IDS)
def test_the_10bit_conversion_contains_the_8bit_conversion(key):
    """samples that are multiples of 4 convert to the bits of the 8-bit conversion of s / 4: all 2^24 byte triples"""
    table = yuv_ref.TABLES[key]
    uv = np.arange(65536, dtype=np.int64)
    u8, v8 = (uv >> 8).astype(np.uint8), (uv & 255).astype(np.uint8)
    for lo in range(0, 256, 32):     # in slabs of 2^21 triples
        y8 = np.repeat(np.arange(lo, lo + 32, dtype=np.uint8)[:, None], 65536, 1)
        u, v = np.broadcast_to(u8, y8.shape), np.broadcast_to(v8, y8.shape)
        want = yuv_ref.convert(y8, u, v, table)
        got = yuv10_ref.convert10(y8.astype(np.uint16) << 2, u.astype(np.uint16) << 2, v.astype(np.uint16) << 2, table)
        for g, w, name in zip(got, want, "BGR"):
            assert np.array_equal(g, w), (key, name, lo)


@pytest.mark.parametrize("key", TABLE_KEYS, ids=IDS)
def test_the_10bit_conversion_is_within_one_grey_level_of_the_float_formula(key):
    """B and R over all 2^20 (Y, chroma) pairs, G on 2^24 seeded random triples; and the sums really leave int32"""
    table = yuv_ref.TABLES[key]
    y, c = (a.reshape(-1) for a in np.meshgrid(np.arange(1024, dtype=np.uint16), np.arange(1024, dtype=np.uint16), indexing="ij"))
    other = np.full(y.shape, 512, np.uint16)
    worst = {}
    b = yuv10_ref.convert10(y, c, other, table)[0], yuv10_ref.convert10_float(y, c, other, *key)[0]
    r = yuv10_ref.convert10(y, other, c, table)[2], yuv10_ref.convert10_float(y, other, c, *key)[2]
    worst["B"] = int(np.abs(b[0].astype(np.int16) - b[1].astype(np.int16)).max())
    worst["R"] = int(np.abs(r[0].astype(np.int16) - r[1].astype(np.int16)).max())
    rng = np.random.default_rng(1010)
    worst["G"] = 0
    for _ in range(8):               # 8 x 2^21 triples
        yy, uu, vv = (rng.integers(0, 1024, 1 << 21).astype(np.uint16) for _ in range(3))
        got, want = yuv10_ref.convert10(yy, uu, vv, table)[1], yuv10_ref.convert10_float(yy, uu, vv, *key)[1]
        worst["G"] = max(worst["G"], int(np.abs(got.astype(np.int16) - want.astype(np.int16)).max()))
    print("max |fixed - float|, 10-bit, %s %s: %s" % (key + (worst,)))
    assert max(worst.values()) <= 1, worst
    # the extremes in exact integers: every PRODUCT fits int32 (the device multiplies in 32 bits), the sums need more
    y0, cy, cub, cug, cvg, cvr = table
    top = (1023 - 4 * y0) * cy + (1 << 21)
    assert top < 2 ** 31 and abs(cub) * 512 < 2 ** 31 and abs(cvr) * 512 < 2 ** 31 and (abs(cug) + abs(cvg)) * 512 < 2 ** 31
    if key[1] == "limited":
        assert top + cub * 511 >= 2 ** 31
    if key == ("bt709", "limited"):
        assert top + cub * 511 == 2304855561
    if key == ("bt601", "limited"):
        assert top + cub * 511 == 2253886216


def test_sample_extraction_and_packers():
    """P010 keeps the top ten bits, I010 the low ten; the packers put the samples where `planes` finds them, junk and pitch or not;
    NV21 is NV12 with the pair swapped"""
    words = np.asarray([0, 63, 64, 0xFFC0, 0xFFFF, 0x03FF, 0x0400, 0xFC00], np.uint16)
    assert yuv10_ref.samples(words, "p010").tolist() == [0, 0, 1, 1023, 1023, 15, 16, 1008]
    assert yuv10_ref.samples(words, "i010").tolist() == [0, 63, 64, 960, 1023, 1023, 0, 0]
    rng = np.random.default_rng(5)
    h, w = 6, 10
    for fmt in ("p010", "i010"):
        Y, U, V = yuv10_ref.random_samples(rng, h, w, fmt)
        plain = yuv10_ref.pack(Y, U, V, fmt)
        assert plain.size == yuv10_ref.nbytes(h, w, fmt) == h * w * 3
        want = yuv10_ref.yuv_to_bgr(plain, h, w, fmt)
        for pitch in (None, 2 * w + 12):
            junky = yuv10_ref.pack(Y, U, V, fmt, pitch, junk=rng)
            assert junky.size == yuv10_ref.nbytes(h, w, fmt, pitch)
            for got, s in zip(yuv10_ref.planes(junky, h, w, fmt, pitch), (Y, U, V)):
                assert np.array_equal(yuv10_ref.samples(got, fmt), s)
            assert np.array_equal(yuv10_ref.yuv_to_bgr(junky, h, w, fmt, pitch=pitch), want)
        assert not np.array_equal(yuv10_ref.pack(Y, U, V, fmt, junk=rng), plain)          # (the junk is there)
        # by hand: the pixel in the middle of a 2x2 block pair
        bgr = yuv10_ref.convert10(Y[3:4, 5:6], U[1:2, 2:3], V[1:2, 2:3], yuv_ref.TABLES[("bt601", "limited")])
        assert tuple(int(c[0, 0]) for c in bgr) == tuple(int(c) for c in want[3, 5])
    Y, U, V = yuv10_ref.random_samples(rng, h, w, "nv21")
    nv12, nv21 = yuv10_ref.pack(Y, U, V, "nv12"), yuv10_ref.pack(Y, U, V, "nv21", 14)
    assert np.array_equal(nv21.reshape(-1, 14)[h:, 0:w:2], V) and np.array_equal(nv21.reshape(-1, 14)[h:, 1:w:2], U)
    assert np.array_equal(yuv10_ref.yuv_to_bgr(nv21, h, w, "nv21", pitch=14), yuv_ref.yuv_to_bgr(nv12, h, w, "nv12"))
    i420 = yuv10_ref.pack(Y, U, V, "i420")
    assert np.array_equal(yuv_ref.yuv_to_bgr(i420, h, w, "i420"), yuv_ref.yuv_to_bgr(nv12, h, w, "nv12"))


# ----------------------------------------------------------------------------------------------------------- YuvFrame
def test_yuv_frame_layouts_of_the_new_formats():
    pkg, lib = load_pkg(), load_pkg("_lib")
    F = pkg.YuvFrame
    frames = load_pkg("frames")
    # the format strings: the 8-bit table is what it was, the 10-bit formats have their own, NV21 is "nv12" with chroma_order="vu"
    assert frames.PIX_FORMATS == {"nv12": 1, "i420": 2} and frames.PIX_FORMATS_10BIT == {"p010": 5, "i010": 6} and frames.PIX_NV21 == 4
    assert dict(frames.PIX_FORMATS_10BIT, nv21=frames.PIX_NV21) == yuv10_ref.FORMATS

    def NV21(data, height, width, **k):
        return F(data, height, width, "nv12", chroma_order="vu", **k)
    h, w = 34, 50
    e = lib.YuvFrameC()
    # default pitch and nbytes
    for fmt, pitch, nbytes in (("nv21", 50, 34 * 50 * 3 // 2), ("p010", 100, 34 * 100 * 3 // 2), ("i010", 100, 34 * 100 * 3 // 2)):
        f = yuv10_ref.frame(pkg, np.zeros(nbytes, np.uint8), h, w, fmt)
        assert yuv10_ref.layout(f) == fmt and f.chroma_order == ("vu" if fmt == "nv21" else "uv")
        assert (f.pitch, f.nbytes, f.data.numel()) == (pitch, nbytes, nbytes) and f.sample_bytes == (1 if fmt == "nv21" else 2)
        with pytest.raises(ValueError, match="the buffer has"):
            yuv10_ref.frame(pkg, np.zeros(nbytes - 1, np.uint8), h, w, fmt)
    # the table entries: plane addresses and pitches, in bytes
    NV21(np.zeros(34 * 64 * 3 // 2, np.uint8), h, w, pitch=64)._fill(e, 4096)
    assert (e.y, e.u, e.v, e.pitch_y, e.pitch_c, e.format) == (4096, 4096 + 34 * 64, None, 64, 64, 4)
    F(np.zeros(34 * 128 * 3 // 2, np.uint8), h, w, "p010", "bt709", "full", pitch=128)._fill(e, 4096)
    assert (e.y, e.u, e.v, e.pitch_y, e.pitch_c, e.format) == (4096, 4096 + 34 * 128, None, 128, 128, 5)
    assert (e.height, e.width, e.matrix, e.range) == (34, 50, 1, 1)
    F(np.zeros(34 * 128 * 3 // 2, np.uint8), h, w, "i010", pitch=128)._fill(e, 4096)
    assert (e.y, e.u, e.v, e.pitch_y, e.pitch_c, e.format) == (4096, 4096 + 34 * 128, 4096 + 34 * 128 + 17 * 64, 128, 64, 6)
    F(np.zeros(34 * 100 * 3 // 2, np.uint8), h, w, "i010")._fill(e, 8192)
    assert (e.y, e.u, e.v, e.pitch_y, e.pitch_c) == (8192, 8192 + 3400, 8192 + 3400 + 17 * 50, 100, 50)
    # 16-bit words are taken as their bytes
    words = (np.arange(34 * 50 * 3 // 2, dtype=np.uint16) * 37).reshape(-1, 50)
    f = F(words, h, w, "p010")
    assert f.data.dtype.is_floating_point is False and f.data.numel() == 34 * 100 * 3 // 2
    assert np.array_equal(f.data.numpy(), words.reshape(-1).view(np.uint8))
    import torch
    g = F(torch.from_numpy(words.view(np.int16).copy()), h, w, "i010")
    assert g.data.dtype == torch.uint8 and np.array_equal(g.data.numpy(), f.data.numpy())
    with pytest.raises(ValueError, match="uint8"):
        NV21(words, h, w)                                     # an 8-bit format takes bytes only
    with pytest.raises(ValueError, match="uint8"):
        F(np.zeros(34 * 100 * 3 // 2, np.int8), h, w, "p010")
    # every new refusal
    buf = np.zeros(34 * 256 * 3 // 2, np.uint8)
    with pytest.raises(ValueError, match="below the width"):
        NV21(buf, h, w, pitch=48)
    for fmt, order in (("nv12", "VU"), ("nv12", "yx"), ("nv12", None), ("i420", "vu"), ("p010", "vu"), ("i010", "vu")):
        with pytest.raises(ValueError, match="chroma_order"):
            F(buf, h, w, fmt, chroma_order=order)
    assert F(buf, h, w, "i420", chroma_order="uv").chroma_order == "uv" and F(buf, h, w).chroma_order == "uv"
    moved = NV21(buf, h, w, pitch=64)
    assert moved.to("cpu") is moved
    for fmt in ("p010", "i010"):
        with pytest.raises(ValueError, match="below twice the width"):
            F(buf, h, w, fmt, pitch=98)
        with pytest.raises(ValueError, match="multiple of"):
            F(buf, h, w, fmt, pitch=101)
        with pytest.raises(ValueError, match="even, positive"):
            F(buf, 33, w, fmt)
    F(buf, h, w, "p010", pitch=102)                           # even is enough for p010 ...
    with pytest.raises(ValueError, match="multiple of 4"):
        F(buf, h, w, "i010", pitch=102)                       # ... i010's chroma rows are pitch / 2 bytes of words
    F(buf, h, w, "i010", pitch=104)
    for bad in ("nv16", "p016", "yuv420p10le", "P010", 5, "nv21"):      # ("nv21": the string stays refused, NV21 is chroma_order="vu")
        with pytest.raises(ValueError, match="format"):
            F(buf, h, w, bad)
    # a rotated destination is sized at 2 bytes per sample
    src = frames.Frames([F(buf, h, w, "p010", pitch=128), NV21(buf, h, w, pitch=64), None], True)
    out = src.rotated([0, 1, 2], "cpu")
    assert (out[0].height, out[0].width, out[0].pitch, out[0].nbytes, out[0].format) == (50, 34, 68, 50 * 68 * 3 // 2, "p010")
    assert (out[1].height, out[1].width, out[1].pitch, out[1].nbytes, yuv10_ref.layout(out[1])) == (34, 50, 50, 34 * 50 * 3 // 2, "nv21") and out[2] is None
    out[1]._fill(e, 4096)
    assert e.format == 4
    t = F._trusted(out[0].data, 50, 34, src[0])
    assert (t.pitch, t.nbytes) == (68, out[0].nbytes)
    t = F._trusted(out[1].data, 34, 50, src[1])
    t._fill(e, 4096)
    assert (t.pitch, t.chroma_order, e.format) == (50, "vu", 4)


def test_header_values():
    lib = load_pkg("_lib")
    text = open(os.path.join(lib.INCLUDE, "hrnet_mi355.h")).read()
    for name, value in (("HRN_PIX_NV12", 1), ("HRN_PIX_I420", 2), ("HRN_PIX_NV21", 4), ("HRN_PIX_P010", 5), ("HRN_PIX_I010", 6), ("HRN_PIX_BGR", 0)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
    assert not re.search(r"\bHRN_PIX_\w+ = 3\b", text)


# ------------------------------------------------------------------------------------------- the C ABI, plan-only handle
def test_new_format_refusals_need_no_gpu():
    """a plan-only handle (device = -1): each new refusal by its text, a good call of each format as 'plan-only', format 3 still
    unknown, the overlays still refuse formats 4 - 6"""
    pkg, lib = load_pkg(), load_pkg("_lib")
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h
    W = 160

    def good(fmt, kind=lib.YuvFrameC, **change):
        e = kind()
        e.y, e.u, e.v = 4096, 65536, (131072 if fmt in (2, 6) else None)         # never read: nothing is launched on this handle
        e.height, e.width, e.pitch_y, e.pitch_c, e.format = 120, W, 384 if fmt in (5, 6) else 192, {2: 96, 5: 384}.get(fmt, 192), fmt
        for k, v in change.items():
            setattr(e, k, v)
        return e

    def table_of(*entries):
        t = (type(entries[0]) * len(entries))()
        for k, e in enumerate(entries):
            ctypes.memmove(ctypes.addressof(t[k]), ctypes.addressof(e), ctypes.sizeof(e))
        return t

    dets = np.asarray([[10, 8, 90, 100], [20, 20, 60, 90]], np.float32)
    out, pad = 4096, np.asarray([114, 114, 114], np.uint8)
    status = 8192

    def entries(e):
        """the four entries that read a YUV frame, each over `e`: (name, rc, text)"""
        res = []
        rc = L.hrn_yuv_to_bgr(h, ctypes.byref(e), out, None)
        res.append(("hrn_yuv_to_bgr", rc, L.hrn_last_error(h).decode()))
        idx = np.asarray([0, 1], np.int32)
        rc = L.hrn_preprocess_frames_yuv(h, table_of(good(1), e), 2, dets.ctypes.data, 4, idx.ctypes.data, 2, 0, out, None, None, None)
        res.append(("hrn_preprocess_frames_yuv", rc, L.hrn_last_error(h).decode()))
        rc = L.hrn_preprocess_frames_yuv_dev(h, table_of(good(1), e), 2, out, 4, idx.ctypes.data, 2, 0, out, out, status, None)
        res.append(("hrn_preprocess_frames_yuv_dev", rc, L.hrn_last_error(h).decode()))
        rc = L.hrn_letterbox_frames_yuv(h, table_of(good(2), e), 2, 1, 64, 96, pad.ctypes.data, 0, 0, out, None, None)
        res.append(("hrn_letterbox_frames_yuv", rc, L.hrn_last_error(h).decode()))
        return res

    def rotate(src, dst, code=1):
        codes = np.asarray([code], np.int32)
        rc = L.hrn_rotate_frames(h, table_of(src), table_of(dst), 1, codes.ctypes.data, None)
        return rc, L.hrn_last_error(h).decode()

    far = 1 << 24
    for fmt in (4, 5, 6):                                                        # good calls reach the handle
        for name, rc, err in entries(good(fmt)):
            assert rc == 7 and "plan-only" in err, (fmt, name, err)
        shift = dict(y=far, u=far + 65536, v=(far + 131072 if fmt == 6 else None))
        rc, err = rotate(good(fmt, lib.CanvasC), good(fmt, lib.CanvasC, **shift))
        assert rc == 7 and "plan-only" in err, (fmt, err)
        turned = dict(shift, height=W, width=120, pitch_y=120 * (1 if fmt == 4 else 2), pitch_c={4: 120, 5: 240, 6: 120}[fmt])
        rc, err = rotate(good(fmt, lib.CanvasC), good(fmt, lib.CanvasC, **turned), code=0)
        assert rc == 7 and "plan-only" in err, (fmt, err)
    # exactly the smallest pitches
    for fmt, change in ((4, dict(pitch_y=W, pitch_c=W)), (5, dict(pitch_y=2 * W, pitch_c=2 * W)), (6, dict(pitch_y=2 * W, pitch_c=W))):
        for name, rc, err in entries(good(fmt, **change)):
            assert rc == 7 and "plan-only" in err, (fmt, name, err)
    odd = "odd plane address or pitch on a 10-bit frame"
    faults = [
        (good(3), "unknown format"), (good(1, format=7), "unknown format"), (good(1, format=0), "unknown format"),
        (good(4, pitch_y=W - 2), "pitch_y below its width"), (good(4, pitch_c=W - 2), "pitch_c below its width"),
        (good(4, u=None), "null plane"),
        (good(5, pitch_y=2 * W - 2), "pitch_y below twice its width"), (good(5, pitch_c=2 * W - 2), "pitch_c below twice its width"),
        (good(6, pitch_y=2 * W - 2), "pitch_y below twice its width"), (good(6, pitch_c=W - 2), "pitch_c below its width"),
        (good(5, y=None), "null plane"), (good(5, u=None), "null plane"), (good(6, v=None), "null plane"),
        (good(5, y=4097), odd), (good(5, u=65537), odd), (good(5, pitch_y=385), odd), (good(5, pitch_c=385), odd),
        (good(6, y=4097), odd), (good(6, u=65537), odd), (good(6, v=131073), odd), (good(6, pitch_y=385), odd), (good(6, pitch_c=193), odd),
        (good(5, width=W - 1), "odd or non-positive width or height"), (good(6, matrix=2), "unknown matrix"),
    ]
    for e, text in faults:
        for name, rc, err in entries(e):
            assert rc == 7 and name in err and text in err and "plan-only" not in err, (name, text, err)
    for e in (good(3), good(1, format=7)):                                       # the unknown-format text lists the names
        err = entries(e)[0][2]
        for name in ("HRN_PIX_NV12", "HRN_PIX_I420", "HRN_PIX_NV21", "HRN_PIX_P010", "HRN_PIX_I010"):
            assert name in err, err
    e = good(4, y=4097, u=65537, pitch_y=193, pitch_c=193)                       # 8-bit frames go anywhere
    for name, rc, err in entries(e):
        assert rc == 7 and "plan-only" in err, (name, err)
    # rotation: both sides are judged
    C = lambda fmt, **k: good(fmt, lib.CanvasC, **k)   # noqa: E731
    away = dict(y=far, u=far + 65536)
    rot_faults = [
        ((C(3), C(3, **away)), "the source has an unknown format"),
        ((C(5, y=4097), C(5, **away)), "the source has an " + odd), ((C(5), C(5, **dict(away, u=far + 65537))), "the destination has an " + odd),
        ((C(5, pitch_c=386 + 1), C(5, **away)), "the source has an " + odd), ((C(6), C(6, v=far + 131073, **away)), "the destination has an " + odd),
        ((C(6, pitch_y=385), C(6, v=far + 131072, **away)), "the source has an " + odd),
        ((C(5, pitch_y=2 * W - 2), C(5, **away)), "the source has pitch_y below its row's bytes"),
        ((C(5), C(5, pitch_c=2 * W - 2, **away)), "the destination has pitch_c below its chroma row's bytes"),
        ((C(6, pitch_c=W - 2), C(6, v=far + 131072, **away)), "the source has pitch_c below its chroma row's bytes"),
        ((C(4, pitch_c=W - 2), C(4, **away)), "the source has pitch_c below"),
        ((C(6), C(6, v=None, **away)), "the destination has a null plane"),
        ((C(5), C(1, **away)), "source and destination differ in format"),
    ]
    for (src, dst), text in rot_faults:
        rc, err = rotate(src, dst)
        assert rc == 7 and err.startswith("hrn_rotate_frames: ") and text in err and "plan-only" not in err, (text, err)
    err = rotate(C(3), C(3, **away))[1]
    for name in ("HRN_PIX_BGR", "HRN_PIX_NV12", "HRN_PIX_I420", "HRN_PIX_NV21", "HRN_PIX_P010", "HRN_PIX_I010"):
        assert name in err, err
    # the overlays keep refusing the new layouts
    skel = np.asarray([[0, 1]], np.int32)
    colours = np.arange(12, dtype=np.uint8).reshape(4, 3)
    for fmt in (4, 5, 6):
        rc = L.hrn_draw_poses(h, table_of(C(fmt)), 1, 4096, 1, 17, None, skel.ctypes.data, 1, colours.ctypes.data, 4, colours.ctypes.data, 4,
                              None, 2, 2, 0.5, None)
        err = L.hrn_last_error(h).decode()
        assert rc == 7 and "hrn_draw_poses" in err and "unknown format" in err, (fmt, err)
    rc = L.hrn_draw_poses(h, table_of(C(1)), 1, 4096, 1, 17, None, skel.ctypes.data, 1, colours.ctypes.data, 4, colours.ctypes.data, 4,
                          None, 2, 2, 0.5, None)
    assert rc == 7 and "plan-only" in L.hrn_last_error(h).decode()
    net.close()
