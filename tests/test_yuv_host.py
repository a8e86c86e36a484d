"""YUV (NV12 / I420) input without a GPU: the coefficient tables of ``hrn_yuv_coefficients``, the numpy restatement of the
conversion (tests/yuv_ref.py) against the float64 formula over every byte triple, ``YuvFrame``'s validation, every refusal of
``hrn_preprocess_frames_yuv`` / ``hrn_yuv_to_bgr`` on a plan-only handle, the declarations, and the cv2 pin (skipped, loudly,
until tests/golden/make_yuv_golden.py has been run where opencv-python is installed)."""
import ctypes
import importlib.util
import os
import re
import zlib

import numpy as np
import pytest

import yuv_ref
from conftest import GOLDEN, load_pkg

TABLE_KEYS = [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")]


def coefficients(L, matrix, range_):
    out = (ctypes.c_int32 * 6)(*([-7] * 6))
    rc = L.hrn_yuv_coefficients(matrix, range_, out)
    return rc, tuple(out)


def test_coefficient_tables():
    L = load_pkg("_lib").load()
    want = {("bt601", "limited"): (16, 1220542, 2116026, -409993, -852492, 1673527),
            ("bt601", "full"): (0, 1048576, 1858077, -360853, -748826, 1470104),
            ("bt709", "limited"): (16, 1220945, 2215014, -223607, -558796, 1879825),
            ("bt709", "full"): (0, 1048576, 1945738, -196424, -490864, 1651297)}
    for key in TABLE_KEYS:
        rc, got = coefficients(L, yuv_ref.MATRICES[key[0]], yuv_ref.RANGES[key[1]])
        assert rc == 0 and got == want[key] == yuv_ref.TABLES[key], (key, got)
        if key != ("bt601", "limited"):     # the three derived tables: floor(x * 2^20 + 0.5) of the exact coefficients
            assert yuv_ref.derived_table(*key) == want[key]
    for matrix, range_ in ((2, 0), (-1, 0), (0, 2), (0, -1), (7, 7)):
        rc, got = coefficients(L, matrix, range_)
        assert rc == 7 and got == (-7,) * 6
    assert L.hrn_yuv_coefficients(0, 0, None) == 7


@pytest.fixture(scope="module")
def all_triples():
    """every (Y, U, V): 2^24 triples as three (256, 65536) uint8 arrays (Y along the rows)"""
    y = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 65536, 1)
    uv = np.arange(65536, dtype=np.int64)
    u, v = (uv >> 8).astype(np.uint8), (uv & 255).astype(np.uint8)
    return y, np.broadcast_to(u, y.shape), np.broadcast_to(v, y.shape)


@pytest.mark.parametrize("key", TABLE_KEYS, ids=["%s-%s" % k for k in TABLE_KEYS])
def test_restatement_within_one_grey_level_of_the_float_formula(all_triples, key):
    y, u, v = all_triples
    table = yuv_ref.TABLES[key]
    worst = 0
    for lo in range(0, 256, 32):     # in slabs: 2^24 triples x int32 x a few temporaries
        sl = slice(lo, lo + 32)
        got = yuv_ref.convert(y[sl], u[sl], v[sl], table)
        want = yuv_ref.convert_float(y[sl], u[sl], v[sl], *key)
        for g, w in zip(got, want):
            worst = max(worst, int(np.abs(g.astype(np.int16) - w.astype(np.int16)).max()))
    print("max |fixed - float| over 2^24 triples, %s %s: %d" % (key + (worst,)))
    assert worst <= 1
    # no sum leaves int32: the extremes of every term, in exact integers
    y0, cy, cub, cug, cvg, cvr = table
    top = (255 - y0) * cy + (1 << 19)
    for terms in ((cub,), (cvg, cug), (cvr,)):
        assert top + sum(abs(c) * 128 for c in terms) < 2 ** 31 and (1 << 19) - sum(abs(c) * 128 for c in terms) > -2 ** 31
    if key[1] == "full":             # grey stays grey, exactly
        grey = np.arange(256, dtype=np.uint8)
        mid = np.full(256, 128, np.uint8)
        for c in yuv_ref.convert(grey, mid, mid, table):
            np.testing.assert_array_equal(c, grey)


def test_ref_layouts_agree():
    """the restatement's plane views: an I420 frame and the NV12 frame of the same planes convert alike; pitch bytes are not read"""
    rng = np.random.default_rng(3)
    h, w, pitch = 6, 10, 16
    Y, U, V = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8), \
        rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    i420 = np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)])
    nv12 = np.concatenate([Y.reshape(-1), np.stack([U, V], -1).reshape(-1)])
    a, b = yuv_ref.yuv_to_bgr(i420, h, w, "i420"), yuv_ref.yuv_to_bgr(nv12, h, w, "nv12")
    np.testing.assert_array_equal(a, b)
    pitched = rng.integers(0, 256, yuv_ref.nbytes(h, w, pitch), dtype=np.uint8)
    py, pu, pv = yuv_ref.planes(pitched, h, w, "nv12", pitch)
    pitched.reshape(-1, pitch)[:h, :w], pitched.reshape(-1, pitch)[h:, :w] = Y, np.stack([U, V], -1).reshape(h // 2, w)
    np.testing.assert_array_equal(yuv_ref.yuv_to_bgr(pitched, h, w, "nv12", pitch=pitch), a)
    assert a.shape == (h, w, 3) and a.dtype == np.uint8
    # the pixel in the middle of a 2x2 block pair: by hand
    bgr = yuv_ref.convert(Y[3:4, 5:6], U[1:2, 2:3], V[1:2, 2:3], yuv_ref.TABLES[("bt601", "limited")])
    assert tuple(int(c[0, 0]) for c in bgr) == tuple(int(c) for c in a[3, 5])


def test_yuv_frame_validation():
    pkg = load_pkg()
    F = pkg.YuvFrame
    buf = np.zeros(34 * 64 * 3 // 2, np.uint8)
    f = F(buf, 34, 50, "nv12", pitch=64)
    assert f.nbytes == 34 * 64 * 3 // 2 and f.data.numel() == f.nbytes and f.device.type == "cpu"
    assert f.to("cpu") is f
    assert F(np.zeros((3, 2), np.uint8), 2, 2).nbytes == 6                      # any shape, pitch defaults to the width
    assert F(np.zeros(100, np.uint8), 2, 2, "i420", "bt709", "full").data.numel() == 6   # a longer buffer: its head
    for h, w in ((33, 50), (34, 49), (0, 50), (34, -2)):
        with pytest.raises(ValueError, match="even, positive"):
            F(buf, h, w)
    with pytest.raises(ValueError, match="the buffer has"):
        F(buf[:-1], 34, 50, pitch=64)
    with pytest.raises(ValueError, match="the buffer has"):
        F(np.zeros(5, np.uint8), 2, 2, "i420")
    with pytest.raises(ValueError, match="below the width"):
        F(buf, 34, 50, pitch=48)
    with pytest.raises(ValueError, match="even pitch"):
        F(buf, 34, 50, "i420", pitch=51)
    with pytest.raises(ValueError, match="format"):
        F(buf, 34, 50, "nv21")
    with pytest.raises(ValueError, match="matrix"):
        F(buf, 34, 50, matrix="bt2020")
    with pytest.raises(ValueError, match="range"):
        F(buf, 34, 50, range="tv")
    with pytest.raises(ValueError, match="uint8"):
        F(np.zeros(34 * 64 * 3 // 2, np.int8), 34, 50, pitch=64)
    # the table entry: plane addresses and pitches of both layouts
    lib = load_pkg("_lib")
    e = lib.YuvFrameC()
    f._fill(e, 4096)
    assert (e.y, e.u, e.v, e.pitch_y, e.pitch_c, e.format) == (4096, 4096 + 34 * 64, None, 64, 64, 1)
    g = F(buf, 34, 50, "i420", "bt709", "full", pitch=64)
    g._fill(e, 4096)
    assert (e.y, e.u, e.v, e.pitch_y, e.pitch_c) == (4096, 4096 + 34 * 64, 4096 + 34 * 64 + 17 * 32, 64, 32)
    assert (e.height, e.width, e.format, e.matrix, e.range) == (34, 50, 2, 1, 1)


def test_symbols_are_declared_and_exported():
    lib = load_pkg("_lib")
    names = {"hrn_yuv_coefficients", "hrn_yuv_to_bgr", "hrn_preprocess_frames_yuv"}
    assert names <= set(lib.header_symbols()) and names <= set(lib.SYMBOLS)
    L = lib.load()
    for name in names:
        assert hasattr(L, name)
    assert L.hrn_preprocess_frames_yuv(None, None, 0, None, 4, None, 0, 0, None, None, None, None) == 1     # no handle
    assert L.hrn_yuv_to_bgr(None, None, None, None) == 1
    text = open(os.path.join(lib.INCLUDE, "hrnet_mi355.h")).read()
    fields = re.search(r"typedef struct \{([^}]*)\} hrn_yuv_frame;", re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [f[0] for f in lib.YuvFrameC._fields_]
    assert ctypes.sizeof(lib.YuvFrameC) == 56 and lib.YuvFrameC.height.offset == 24 and lib.YuvFrameC.range.offset == 48
    for name, value in (("HRN_PIX_NV12", 1), ("HRN_PIX_I420", 2), ("HRN_YUV_BT601", 0), ("HRN_YUV_BT709", 1), ("HRN_YUV_LIMITED", 0),
                        ("HRN_YUV_FULL", 1)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
    native = load_pkg("native")
    assert (native.PIX_FORMATS, native.YUV_MATRICES, native.YUV_RANGES) == ({"nv12": 1, "i420": 2}, yuv_ref.MATRICES, yuv_ref.RANGES)


def test_yuv_refusals_need_no_gpu():
    """a plan-only handle (device = -1): every argument error is reported as such, and a good call as 'plan-only'"""
    pkg = load_pkg()
    lib = load_pkg("_lib")
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h

    def good(fmt=1):
        e = lib.YuvFrameC()
        e.y, e.u, e.v = 4096, 8192, (12288 if fmt == 2 else None)             # never read: nothing is launched on this handle
        e.height, e.width, e.pitch_y, e.pitch_c, e.format, e.matrix, e.range = 120, 160, 192, 192 if fmt == 1 else 96, fmt, 0, 0
        return e

    def table_of(*entries):
        t = (lib.YuvFrameC * len(entries))()
        for k, e in enumerate(entries):
            ctypes.memmove(ctypes.addressof(t[k]), ctypes.addressof(e), ctypes.sizeof(e))
        return t

    dets = np.asarray([[10, 8, 90, 100], [20, 20, 60, 90]], np.float32)
    idx = np.zeros(2, np.int32)
    out = 4096                                                                  # "device" outputs, never written

    def call(table, nframes, idx, n=2, variant=0, stride=4, d=dets):
        rc = L.hrn_preprocess_frames_yuv(h, table, nframes, None if d is None else d.ctypes.data, stride,
                                         None if idx is None else idx.ctypes.data, n, variant, out, None, None, None)
        return rc, L.hrn_last_error(h).decode()

    def bgr(entry, dst=out):
        rc = L.hrn_yuv_to_bgr(h, None if entry is None else ctypes.byref(entry), dst, None)
        return rc, L.hrn_last_error(h).decode()

    empty = lib.YuvFrameC()                                                     # all zero: a frame nobody is cut from
    for fmt in (1, 2):
        table = table_of(good(fmt), empty)
        for args in ((table, 2, idx), (table, 1, None), (table, 2, idx, 0)):    # good calls (the handle is judged before n == 0)
            rc, err = call(*args)
            assert rc == 7 and "plan-only" in err, err
        rc, err = bgr(good(fmt))
        assert rc == 7 and "plan-only" in err, err
    table = table_of(good(), empty)
    # hrn_preprocess_frames' own refusals, with its texts
    for bad, f, person in (([0, 2], 2, 1), ([-1, 0], -1, 0), ([0, 1 << 30], 1 << 30, 1)):
        rc, err = call(table, 2, np.asarray(bad, np.int32))
        assert rc == 7 and "frame_index %d of person %d is outside [0, 2)" % (f, person) in err, err
    for args in ((None, 2, idx), (table, 0, idx), (table, 2, idx, -1), (table, 2, idx, 2, 0, 3)):
        rc, err = call(*args)
        assert rc == 7 and "bad frames / detections / n" in err, err
    rc, err = call(table, 2, idx, d=None)
    assert rc == 7 and "bad frames / detections / n" in err
    rc, err = call(table, 2, None)
    assert rc == 7 and "without frame_index there must be one frame" in err
    rc, err = call(table, 2, idx, variant=2)
    assert rc == 7 and "variant must be HRN_CROP_PAD or HRN_CROP_CLAMP" in err
    # the frames' own: each names its cause, for the table entry a person refers to and for hrn_yuv_to_bgr's frame
    faults = [
        (dict(format=0), "unknown format"), (dict(format=3), "unknown format"),
        (dict(matrix=2), "unknown matrix"), (dict(matrix=-1), "unknown matrix"),
        (dict(range=2), "unknown range"), (dict(range=-1), "unknown range"),
        (dict(width=159), "odd or non-positive width or height"), (dict(height=121), "odd or non-positive width or height"),
        (dict(width=0), "odd or non-positive width or height"), (dict(height=-2), "odd or non-positive width or height"),
        (dict(pitch_y=158), "pitch_y below its width"),
        (dict(pitch_c=158), "pitch_c below its width"),
        (dict(format=2, v=12288, pitch_c=79), "pitch_c below half its width"),
        (dict(y=None), "null plane"), (dict(u=None), "null plane"), (dict(format=2, pitch_c=80, v=None), "null plane"),
    ]
    for change, text in faults:
        e = good()
        for name, value in change.items():
            setattr(e, name, value)
        rc, err = call(table_of(good(), e), 2, np.asarray([0, 1], np.int32))
        assert rc == 7 and "frame 1, which person 1 is cut from, " in err and text in err, (change, err)
        rc, err = call(table_of(good(), e), 2, np.asarray([0, 0], np.int32))    # ... while nobody referring to it is fine
        assert rc == 7 and "plan-only" in err, (change, err)
        rc, err = bgr(e)
        assert rc == 7 and "hrn_yuv_to_bgr" in err and text in err, (change, err)
    e = good()
    e.format, e.pitch_c, e.v = 2, 80, 12288                                     # I420 at exactly half the width: fine
    rc, err = bgr(e)
    assert rc == 7 and "plan-only" in err
    rc, err = bgr(None)
    assert rc == 7 and "null frame or output" in err
    rc, err = bgr(good(), None)
    assert rc == 7 and "null frame or output" in err
    # a detection that fails the box arithmetic would be judged after the handle, as in hrn_preprocess_frames
    net.close()


def test_python_entries_refuse_a_mixture():
    """BGR and YUV frames in one call: ValueError before anything reaches the library"""
    native = load_pkg("native")
    y = native.YuvFrame(np.zeros(6, np.uint8), 2, 2)
    b = np.zeros((2, 2, 3), np.uint8)
    with pytest.raises(ValueError, match="mixture"):
        native._frame_kind([y, None, b])
    assert native._frame_kind([y, None, y]) is True and native._frame_kind([b, None]) is False and native._frame_kind([]) is False


def test_restatement_against_cv2_golden():
    """tests/yuv_ref.py (and with it the kernels, which the GPU tests hold to it bit for bit) against a real cv2 build: BT.601
    limited range, both layouts.  The fixture is made by tests/golden/make_yuv_golden.py wherever opencv-python is installed."""
    path = os.path.join(GOLDEN, "cv2_yuv_cases.npz")
    if not os.path.exists(path):
        pytest.skip("UNPINNED: tests/golden/cv2_yuv_cases.npz is absent -- run tests/golden/make_yuv_golden.py where opencv-python "
                    "is installed and commit its output; until then equality of the BT.601 table with cv2 is not checked")
    spec = importlib.util.spec_from_file_location("make_yuv_golden", os.path.join(GOLDEN, "make_yuv_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = dict(np.load(path))
    assert int(g["ncases"]) >= 8
    for k in range(int(g["ncases"])):
        hh, ww, fmt, seed, crc = (int(v) for v in g["case%d_meta" % k])
        f = gen.frame(hh, ww, seed)
        assert zlib.crc32(f.tobytes()) == crc, "this numpy draws other frames than the one the fixture was made with"
        np.testing.assert_array_equal(yuv_ref.yuv_to_bgr(f, hh, ww, "nv12" if fmt == 0 else "i420"), g["case%d_out" % k],
                                      err_msg="cv2 %s, case %d" % (g["cv2_version"], k))
