"""Heat-map overlays without a GPU: ``hrn_heatmap_quantise`` / ``hrn_draw_heatmaps_host`` -- the text the kernels compile,
csrc/heat_math.h -- against the numpy restatement of the definition (tests/heat_ref.py), whole buffers byte for byte on noise
canvases with guard bytes in the pitch; the colour tables against their formulas; the declarations; every refusal with its
message; and the same cases walked by a stand-alone C++ program under AddressSanitizer and UBSan (a child process of its own;
nothing is preloaded into Python)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import heat_cases
import heat_ref
import yuv_ref
from conftest import load_pkg
from heat_cases import F32, noise
from test_labels_host import sanitizer_compiler

FORMATS = [("bgr", None), ("nv12", ("bt601", "limited")), ("i420", ("bt709", "full"))]
GUARD = 26      # bytes of pitch beyond a row


def table_for(fmt_key):
    """the jet table in the canvas's colour space, from the restatement's own formula"""
    pkg = load_pkg()
    fmt, key = fmt_key
    return heat_ref.jet() if key is None else pkg.bgr_to_yuv_colors(heat_ref.jet(), *key)


class Canvas:
    """a noise canvas of one format with guard bytes behind every row: `frame` is what the library draws into, `buffer` every
    byte of it, `expected(draw)` the restatement's drawing on a copy"""

    def __init__(self, fmt_key, h, w, seed):
        pkg = load_pkg()
        self.fmt, self.key = fmt_key
        self.h, self.w = h, w
        if self.fmt == "bgr":
            self.buffer = noise((h, w + 9, 3), seed)
            self.frame = self.buffer[:, :w]
        else:
            self.pitch = w + GUARD
            self.buffer = noise(yuv_ref.nbytes(h, w, self.pitch), seed)
            self.frame = pkg.YuvFrame(self.buffer, h, w, self.fmt, self.key[0], self.key[1], self.pitch)
            assert np.shares_memory(self.frame.data.numpy(), self.buffer)
        self.before = self.buffer.copy()

    def expected(self, maps, boxes, lut, **kw):
        want = self.before.copy()
        if self.fmt == "bgr":
            heat_ref.draw_bgr(want[:, :self.w], maps, boxes, lut, **kw)
        else:
            heat_ref.draw_yuv(want, self.h, self.w, self.fmt, maps, boxes, lut, pitch=self.pitch, **kw)
        return want


def draw_and_compare(post, fmt_key, h, w, maps, boxes, mask, setting, seed, lo=0.0, hi=1.0, colormap=None):
    """draws with the library's host form and with the restatement; returns (before, after), the two having been held equal"""
    alpha, mode, cutoff = setting
    c = Canvas(fmt_key, h, w, seed)
    bgr_table = heat_ref.jet() if colormap is None else colormap
    lut = bgr_table if fmt_key[1] is None else load_pkg().bgr_to_yuv_colors(bgr_table, *fmt_key[1])
    joints = None if mask is None else [j for j, m in enumerate(mask) if m]
    out = post.draw_heatmaps(c.frame, maps, boxes, joints=joints, colormap=bgr_table, alpha=alpha, alpha_mode=("const", "value")[mode],
                             vmin=lo, vmax=hi, cutoff=cutoff)
    assert out is c.frame
    want = c.expected(maps, boxes, lut, mask=mask, lo=lo, hi=hi, alpha=alpha, mode=mode, cutoff=cutoff)
    np.testing.assert_array_equal(c.buffer, want, err_msg=str((fmt_key, h, w, setting)))
    return c.before, c.buffer


def test_symbols_are_declared_and_exported_and_the_header_is_one_text():
    lib = load_pkg("_lib")
    names = {"hrn_draw_heatmaps_dev", "hrn_heatmap_quantise", "hrn_draw_heatmaps_host", "hrn_heatmap_last_error"}
    assert names <= set(lib.header_symbols()) and names <= set(lib.SYMBOLS)
    assert set(lib.header_symbols()) == set(lib.SYMBOLS)
    assert "heat.hip" in lib.SOURCES
    math_h = os.path.join(lib.CSRC, "heat_math.h")
    assert math_h in lib._deps("heat.hip") and math_h in lib._deps("hrnet_mi355.cpp")
    heat, host = open(os.path.join(lib.CSRC, "heat.hip")).read(), open(os.path.join(lib.CSRC, "hrnet_mi355.cpp")).read()
    assert '#include "heat_math.h"' in heat and '#include "heat_math.h"' in host
    for fn in ("heat_quantise(", "heat_coord(", "heat_sample(", "heat_written(", "heat_blend(", "heat_block_value(", "heat_max("):
        assert fn in heat and fn in host, fn                    # both sides call the one text; neither restates it
    code = "\n".join(line.split("//")[0] for line in heat.splitlines())
    assert "heat_reduce_kernel" in code and "heat_raster_kernel" in code and "atomic" not in code.lower()
    assert "fp contract(off)" in open(math_h).read()
    L = lib.load()
    for name in names:
        assert hasattr(L, name)
    text = open(os.path.join(lib.INCLUDE, "hrnet_mi355.h")).read()
    assert "HRN_HEAT_ALPHA_CONST = 0, HRN_HEAT_ALPHA_VALUE = 1" in text and "(top (256 - fy) + bot fy + 32768) >> 16" in text
    assert L.hrn_draw_heatmaps_dev(None, None, 0, None, None, 0, 1, 1, 1, None, None, 0.0, 1.0, None, 0, 0, 1, None) == 1   # no handle
    pkg = load_pkg()
    assert "heat_colormap" in pkg.__all__ and pkg.heat_colormap is load_pkg("native").heat_colormap


@pytest.mark.parametrize("lo,hi", heat_cases.RANGES)
def test_quantise_on_the_designed_vector(lo, hi):
    post = load_pkg("postproc")
    maps = heat_cases.quantise_maps(lo, hi)
    L = maps.shape[-1]
    for joints, mask in ((None, None), ([0], [1, 0, 0]), ([0, 2], [1, 0, 1]), ([1], [0, 1, 0]), ([2, 1], [0, 1, 1])):
        got = post.heatmap_quantise(maps, joints=joints, vmin=lo, vmax=hi)
        want = heat_ref.quantise(maps, mask, lo, hi)
        assert got.shape == (2, 1, L) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, want, err_msg=str((lo, hi, joints)))
    q = post.heatmap_quantise(maps, joints=[0], vmin=lo, vmax=hi)[0, 0]
    v = heat_cases.quantise_vector(lo, hi)
    k = F32(F32(255.0) / F32(F32(hi) - F32(lo)))
    for value, got in zip(v, q):                       # the rule once more, in scalars: two float32 operations, then one
        with np.errstate(all="ignore"):
            t = F32(F32(value - F32(lo)) * k)
        assert got == (0 if not t > 0 else 255 if t >= 255 else int(F32(t + F32(0.5)))), (float(value), float(t))
    assert set(range(0, 3)) <= set(q.tolist()) and {127, 128, 253, 254, 255} <= set(q.tolist())      # both sides of every half-step
    special = dict(zip([np.inf, -np.inf, np.nan, -0.0], q[5 * len(heat_cases.HALF_STEPS):]))
    assert special[np.inf] == 255 and special[-np.inf] == 0 and q[-1] == 0                            # +inf, -inf, all-NaN
    assert post.heatmap_quantise(maps, joints=[1], vmin=lo, vmax=hi)[0].max() == 0                     # an all-NaN joint
    assert post.heatmap_quantise(maps, joints=[2], vmin=lo, vmax=hi)[0].max() == 0                     # -inf everywhere
    np.testing.assert_array_equal(post.heatmap_quantise(maps, vmin=lo, vmax=hi)[1, 0, :-1], np.maximum(q, q[::-1])[:-1])     # NaN first: it does not stick
    rnd = heat_cases.random_maps(4, 7, 5, 3)
    np.testing.assert_array_equal(post.heatmap_quantise(rnd, vmin=lo, vmax=hi), heat_ref.quantise(rnd, None, lo, hi))


@pytest.mark.parametrize("fmt_key", FORMATS, ids=[f[0] for f in FORMATS])
def test_the_matrix_equals_the_restatement(fmt_key):
    post = load_pkg("postproc")
    changed = 0
    for k, (name, h, w, maps, boxes, mask, setting, unchanged) in enumerate(heat_cases.matrix()):
        before, after = draw_and_compare(post, fmt_key, h, w, maps, boxes, mask, setting, seed=k)
        if unchanged:
            np.testing.assert_array_equal(before, after, err_msg=name)
        else:
            changed += int((before != after).any())
    assert changed >= len(heat_cases.matrix()) // 2


@pytest.mark.parametrize("fmt_key", FORMATS, ids=[f[0] for f in FORMATS])
def test_overlapping_people_in_both_orders_and_the_alpha_rules(fmt_key):
    post = load_pkg("postproc")
    h, w = 46, 70
    maps, boxes = heat_cases.random_maps(2, 16, 12, 5), heat_cases.OVERLAPPING
    _, one = draw_and_compare(post, fmt_key, h, w, maps, boxes, None, (153, 1, 26), seed=1)
    _, other = draw_and_compare(post, fmt_key, h, w, maps[::-1], boxes[::-1], None, (153, 1, 26), seed=1)
    np.testing.assert_array_equal(one, other)
    for mode in (0, 1):                                 # alpha 0: nothing is written
        before, after = draw_and_compare(post, fmt_key, h, w, maps, boxes, None, (0, mode, 1), seed=2)
        np.testing.assert_array_equal(before, after)
    # alpha 255, cutoff 1, CONST: a written pixel equals the table
    ones = np.full((1, 3, 5, 4), 0.5, F32)
    box = np.asarray([[10, 8, 40, 30]], np.int32)
    before, after = draw_and_compare(post, fmt_key, h, w, ones, box, None, (255, 0, 1), seed=3)
    lut = table_for(fmt_key)
    if fmt_key[0] == "bgr":
        assert (after[8:30, 10:40] == lut[128]).all() and (after[:8] == before[:8]).all() and (after[:, 40:] == before[:, 40:]).all()
    else:
        Y, U, V = yuv_ref.planes(after, h, w, fmt_key[0], w + GUARD)
        assert (Y[8:30, 10:40] == lut[128][0]).all() and (U[4:15, 5:20] == lut[128][1]).all() and (V[4:15, 5:20] == lut[128][2]).all()
    for mode in (0, 1):                                 # cutoff 255: only saturated pixels
        draw_and_compare(post, fmt_key, h, w, maps, boxes, None, (200, mode, 255), seed=4)
    before, after = draw_and_compare(post, fmt_key, h, w, np.full((1, 3, 5, 4), 0.99, F32), box, None, (200, 1, 255), seed=4)
    np.testing.assert_array_equal(before, after)        # Q = 252 everywhere: below the cutoff
    draw_and_compare(post, fmt_key, h, w, maps, boxes, None, (1, 1, 1), seed=5)        # VALUE mode where a rounds to 0 for small V
    draw_and_compare(post, fmt_key, h, w, maps, boxes, None, (153, 1, 26), seed=6, lo=-0.3, hi=0.9)
    draw_and_compare(post, fmt_key, h, w, maps, boxes, None, (153, 1, 26), seed=7, colormap=load_pkg().heat_colormap("hot"))


def test_two_canvases_of_different_sizes():
    pkg, post = load_pkg(), load_pkg("postproc")
    rng = np.random.default_rng(8)
    sizes = [(46, 70), None, (70, 100)]
    frame_index = np.asarray([0, 2, 2, 0, 2, 0, 0], np.int32)
    n = len(frame_index)
    boxes = np.empty((n, 4), np.int32)
    for i, f in enumerate(frame_index):
        hh, ww = sizes[f]
        boxes[i, :2] = rng.integers(-10, ww - 20), rng.integers(-10, hh - 20)
        boxes[i, 2:] = boxes[i, :2] + rng.integers(5, 60, 2)
    maps = heat_cases.random_maps(n, 16, 12, 9)
    before = [None if s is None else noise(s + (3,), 20 + k) for k, s in enumerate(sizes)]
    frames = [None if b is None else b.copy() for b in before]
    out = post.draw_heatmaps(frames, maps, boxes, frame_index=frame_index, colormap="jet", alpha=200, alpha_mode="const", cutoff=20)
    assert out[1] is None and out[0] is frames[0]
    want = heat_ref.draw_clip([None if b is None else b.copy() for b in before], maps, boxes, frame_index, heat_ref.jet(), alpha=200,
                              mode=0, cutoff=20)
    for f in (0, 2):
        np.testing.assert_array_equal(frames[f], want[f], err_msg="frame %d" % f)
        assert (frames[f] != before[f]).any()
    # the same on two NV12 frames
    key = ("bt601", "limited")
    lut = pkg.bgr_to_yuv_colors(heat_ref.jet(), *key)
    data = [None if s is None else noise(yuv_ref.nbytes(s[0], s[1], s[1] + GUARD), 30 + k) for k, s in enumerate(sizes)]
    yuv = [None if s is None else pkg.YuvFrame(d, s[0], s[1], "nv12", key[0], key[1], s[1] + GUARD) for s, d in zip(sizes, data)]
    want = [None if d is None else d.copy() for d in data]
    post.draw_heatmaps(yuv, maps, boxes, frame_index=frame_index)
    for f in (0, 2):
        who = np.nonzero(frame_index == f)[0]
        heat_ref.draw_yuv(want[f], sizes[f][0], sizes[f][1], "nv12", maps[who], boxes[who], lut, pitch=sizes[f][1] + GUARD)
        np.testing.assert_array_equal(data[f], want[f], err_msg="NV12 frame %d" % f)
    with pytest.raises(ValueError, match="frame_index"):
        post.draw_heatmaps(frames, maps, boxes)
    with pytest.raises(ValueError, match="is null"):
        post.draw_heatmaps(frames, maps[:1], boxes[:1], frame_index=[1])


def test_colour_tables():
    pkg = load_pkg()
    jet = pkg.heat_colormap("jet")
    assert jet.shape == (256, 3) and jet.dtype == np.uint8
    for i in range(256):
        for col, k in ((2, 3), (1, 2), (0, 1)):        # the table is (B, G, R); k = 3, 2, 1 for R, G, B
            assert jet[i, col] == (min(max(765 - abs(8 * i - 510 * k), 0), 510) + 1) >> 1, (i, col)
    np.testing.assert_array_equal(jet, heat_ref.jet())
    assert jet[0].tolist() == [128, 0, 0] and jet[255].tolist() == [0, 0, 128]                  # dark blue to dark red
    assert jet[:, 0].max() == 255 and jet[:, 1].max() == 255 and jet[:, 2].max() == 255
    for col in range(3):                                # every channel: up, flat at the top, down -- once
        d = np.sign(np.diff(jet[:, col].astype(int)))
        d = d[d != 0]
        assert (np.diff(d) != 0).sum() <= 1 and (d[0] > 0 or col == 0) and (d[-1] < 0 or col == 2), col
    b, g, r = (int(np.argmax(jet[:, c])) for c in range(3))
    assert b < g < r                                    # blue peaks first, red last
    np.testing.assert_array_equal(pkg.heat_colormap("gray"), heat_ref.gray())
    hot = pkg.heat_colormap("hot").astype(int)
    i = np.arange(256)
    for col, k in ((2, 0), (1, 1), (0, 2)):
        np.testing.assert_array_equal(hot[:, col], np.clip(3 * i - 255 * k, 0, 255))
    assert hot[0].tolist() == [0, 0, 0] and hot[255].tolist() == [255, 255, 255] and (np.diff(hot, axis=0) >= 0).all()
    for name in ("jet", "hot", "gray"):
        for key in (("bt601", "limited"), ("bt709", "full")):
            np.testing.assert_array_equal(pkg.bgr_to_yuv_colors(pkg.heat_colormap(name), *key),
                                          np.stack([pkg.bgr_to_yuv_colors(row[None], *key)[0] for row in pkg.heat_colormap(name)]))
    with pytest.raises(ValueError, match="colormap must be one of"):
        pkg.heat_colormap("viridis")
    # a YUV canvas drawn with a name is drawn with bgr_to_yuv_colors of the BGR table (draw_and_compare passes the BGR table)
    post = load_pkg("postproc")
    key = ("bt709", "limited")
    data = noise(yuv_ref.nbytes(46, 70), 1)
    want = data.copy()
    maps, boxes = heat_cases.random_maps(2, 5, 4, 2), heat_cases.OVERLAPPING
    post.draw_heatmaps(pkg.YuvFrame(data, 46, 70, "i420", *key), maps, boxes, colormap="hot")
    heat_ref.draw_yuv(want, 46, 70, "i420", maps, boxes, pkg.bgr_to_yuv_colors(pkg.heat_colormap("hot"), *key))
    np.testing.assert_array_equal(data, want)


def canvas_entries(lib):
    def bgr(**change):
        e = lib.CanvasC()
        e.y, e.height, e.width, e.pitch_y, e.format = 4096, 120, 160, 480, 0      # never touched: every call below is refused
        for k, v in change.items():
            setattr(e, k, v)
        return e

    def yuv(fmt=1, **change):
        e = lib.CanvasC()
        e.y, e.u, e.v = 4096, 8192, (12288 if fmt == 2 else None)
        e.height, e.width, e.pitch_y, e.pitch_c, e.format = 120, 160, 192, 192 if fmt == 1 else 96, fmt
        for k, v in change.items():
            setattr(e, k, v)
        return e

    def table_of(*entries):
        t = (lib.CanvasC * len(entries))()
        for k, e in enumerate(entries):
            ctypes.memmove(ctypes.addressof(t[k]), ctypes.addressof(e), ctypes.sizeof(e))
        return t

    return bgr, yuv, table_of


REFUSED = [
    (dict(n=-1), "n is negative"), (dict(J=0), "J must be in [1, 256]"), (dict(J=257), "J must be in [1, 256]"),
    (dict(hq=0), "hq and wq must be in [1, 1024]"), (dict(wq=0), "hq and wq must be in [1, 1024]"), (dict(hq=1025), "hq and wq must be in [1, 1024]"),
    (dict(lo=np.nan), "lo and hi must be finite"), (dict(lo=-np.inf), "lo and hi must be finite"), (dict(hi=np.inf), "lo and hi must be finite"),
    (dict(lo=1.0, hi=1.0), "hi must be above lo"), (dict(lo=0.5, hi=0.25), "hi must be above lo"),
    (dict(mask=np.zeros(3, np.uint8)), "the joint mask selects no joint"),
    (dict(alpha=-1), "alpha must be in [0, 255]"), (dict(alpha=256), "alpha must be in [0, 255]"),
    (dict(mode=2), "alpha_mode must be HRN_HEAT_ALPHA_CONST or HRN_HEAT_ALPHA_VALUE"),
    (dict(cutoff=0), "cutoff must be in [1, 255]"), (dict(cutoff=256), "cutoff must be in [1, 255]"),
    (dict(table=None), "null canvases / heat-maps / boxes / colour table"), (dict(maps=None), "null canvases"), (dict(boxes=None), "null canvases"),
    (dict(lut=None), "null canvases"), (dict(nframes=0), "null canvases"),
    (dict(idx=None), "without frame_index there must be one frame"),
    (dict(idx=np.asarray([0, 2], np.int32)), "frame_index 2 of person 1 is outside [0, 2)"),
    (dict(idx=np.asarray([-1, 0], np.int32)), "frame_index -1 of person 0 is outside [0, 2)"),
    (dict(idx=np.asarray([0, 1], np.int32)), "canvas 1, which person 1 is drawn on, is null"),
]


def refusal_calls(lib, call, prefix, accepted):
    """every refusal against `call(**change) -> (rc, error text)`; `accepted(rc, err)`: what a good call answers"""
    bgr, yuv, table_of = canvas_entries(lib)
    for change in (dict(), dict(mask=None), dict(mask=np.asarray([0, 0, 1], np.uint8)), dict(nframes=1, idx=None), dict(n=0),
                   dict(n=0, maps=None, boxes=None), dict(alpha=0), dict(alpha=255, mode=0, cutoff=255), dict(hq=1024, wq=1),
                   dict(table=table_of(yuv(1), lib.CanvasC())), dict(table=table_of(yuv(2), yuv(1, y=16384)), idx=np.asarray([0, 1], np.int32))):
        rc, err = call(**change)
        assert accepted(rc, err), (list(change), rc, err)
    for change, text in REFUSED:
        rc, err = call(**change)
        assert rc == 7 and err.startswith(prefix) and text in err, (list(change), err)
    faults = [
        (bgr(y=None), "is null"), (bgr(height=0), "non-positive width or height"), (bgr(height=8193), "side above 8192"),
        (bgr(pitch_y=479), "pitch below three times its width"), (bgr(format=3), "unknown format"), (bgr(format=4), "unknown format"),
        (yuv(1, format=5), "unknown format"), (yuv(2, format=6), "unknown format"),
        (yuv(1, height=121), "odd width or height"), (yuv(1, pitch_y=158), "pitch_y below its width"), (yuv(1, pitch_c=158), "pitch_c below its width"),
        (yuv(2, pitch_c=79), "pitch_c below half its width"), (yuv(2, v=None), "null plane"),
    ]
    for entry, text in faults:
        first = yuv(1) if entry.format in (1, 2, 5, 6) else bgr()
        rc, err = call(table=table_of(first, entry), idx=np.asarray([0, 1], np.int32))
        assert rc == 7 and "canvas 1, which person 1 is drawn on, " in err and text in err, (text, err)
        rc, err = call(table=table_of(first, entry))                      # ... while nobody referring to it is fine
        assert accepted(rc, err), (text, err)
    rc, err = call(table=table_of(bgr(), bgr(height=60)), idx=np.asarray([0, 1], np.int32))
    assert rc == 7 and "canvases 0 and 1 name the same buffer" in err and "must not overlap" in err, err
    rc, err = call(table=table_of(bgr(), yuv(1)), idx=np.asarray([0, 1], np.int32))
    assert rc == 7 and "mixes formats" in err and "all BGR or all YUV" in err, err


def test_device_entry_refusals_need_no_gpu():
    """a plan-only handle (device = -1): every argument error is reported as such, and a good call as 'plan-only'"""
    pkg, lib = load_pkg(), load_pkg("_lib")
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h
    bgr, yuv, table_of = canvas_entries(lib)
    lut = heat_ref.jet()
    good = dict(table=table_of(bgr(), lib.CanvasC()), nframes=2, maps=4096, boxes=8192, n=2, J=3, hq=5, wq=4, idx=np.zeros(2, np.int32),
                mask=np.asarray([1, 0, 1], np.uint8), lo=0.0, hi=1.0, lut=lut, alpha=153, mode=1, cutoff=26)

    def call(**change):
        a = dict(good, **change)
        p = lambda v: None if v is None else (v.ctypes.data if isinstance(v, np.ndarray) else v)   # noqa: E731
        rc = L.hrn_draw_heatmaps_dev(h, a["table"], a["nframes"], a["maps"], a["boxes"], a["n"], a["J"], a["hq"], a["wq"], p(a["idx"]),
                                     p(a["mask"]), a["lo"], a["hi"], p(a["lut"]), a["alpha"], a["mode"], a["cutoff"], None)
        return rc, L.hrn_last_error(h).decode()

    refusal_calls(lib, call, "hrn_draw_heatmaps_dev: ", lambda rc, err: rc == 7 and "plan-only" in err)
    net.close()


def test_host_entry_refusals():
    lib = load_pkg("_lib")
    post, L = load_pkg("postproc"), lib.load()
    bgr, yuv, table_of = canvas_entries(lib)
    # real memory behind the good call: the canvases refused below are never touched, the accepted ones are drawn into
    pixels = np.zeros(4096 + 192 * 120 * 3, np.uint8)
    base = pixels.ctypes.data

    def real(e):
        for name in ("y", "u", "v"):
            if getattr(e, name):
                setattr(e, name, base + getattr(e, name) - 4096)
        return e

    maps, boxes = heat_cases.random_maps(2, 5, 4, 1), np.asarray([[3, 4, 40, 50], [20, 10, 90, 70]], np.int32)
    good = dict(table=table_of(real(bgr()), lib.CanvasC()), nframes=2, maps=maps, boxes=boxes, n=2, J=3, hq=5, wq=4, idx=np.zeros(2, np.int32),
                mask=np.asarray([1, 0, 1], np.uint8), lo=0.0, hi=1.0, lut=heat_ref.jet(), alpha=153, mode=1, cutoff=26)

    def call(**change):
        a = dict(good, **change)
        if "table" in change and change["table"] is not None:
            for e in a["table"]:
                real(e)
        p = lambda v: None if v is None else (v.ctypes.data if isinstance(v, np.ndarray) else v)   # noqa: E731
        rc = L.hrn_draw_heatmaps_host(a["table"], a["nframes"], p(a["maps"]), p(a["boxes"]), a["n"], a["J"], a["hq"], a["wq"], p(a["idx"]),
                                      p(a["mask"]), a["lo"], a["hi"], p(a["lut"]), a["alpha"], a["mode"], a["cutoff"])
        return rc, "hrn_draw_heatmaps_host: " + L.hrn_heatmap_last_error().decode()

    # (hq = 1024, wq = 1 would read maps beyond the two small ones: the accepted calls here keep the good shapes)
    accepted = lambda rc, err: rc == 0 and err == "hrn_draw_heatmaps_host: "      # noqa: E731
    big = np.zeros((2, 3, 1024, 1), F32)
    rc, err = call(hq=1024, wq=1, maps=big)
    assert accepted(rc, err)

    def call_small(**change):
        if change.get("hq") == 1024:
            change = dict(change, maps=big)
        return call(**change)

    refusal_calls(lib, call_small, "hrn_draw_heatmaps_host: ", accepted)
    out = np.empty((2, 5, 4), np.uint8)
    q = lambda *a: (L.hrn_heatmap_quantise(*a), L.hrn_heatmap_last_error().decode())      # noqa: E731
    zero = np.zeros(3, np.uint8)
    assert q(maps.ctypes.data, 2, 3, 5, 4, None, 0.0, 1.0, out.ctypes.data) == (0, "")
    assert q(maps.ctypes.data, 2, 3, 5, 4, zero.ctypes.data, 0.0, 1.0, out.ctypes.data) == (7, "the joint mask selects no joint")
    assert q(maps.ctypes.data, 2, 3, 5, 4, None, 1.0, 1.0, out.ctypes.data) == (7, "hi must be above lo")
    assert q(maps.ctypes.data, 2, 3, 5, 4, None, np.nan, 1.0, out.ctypes.data) == (7, "lo and hi must be finite")
    assert q(maps.ctypes.data, 2, 3, 0, 4, None, 0.0, 1.0, out.ctypes.data) == (7, "hq and wq must be in [1, 1024]")
    assert q(None, 2, 3, 5, 4, None, 0.0, 1.0, out.ctypes.data) == (7, "null heat-maps")
    assert q(maps.ctypes.data, 2, 3, 5, 4, None, 0.0, 1.0, None) == (7, "null output")
    assert q(None, 0, 3, 5, 4, None, 0.0, 1.0, None) == (0, "")
    frame = np.zeros((20, 30, 3), np.uint8)
    for kw, text in ((dict(joints=[]), "non-empty list of indices"), (dict(joints=[3]), r"indices in \[0, 3\)"), (dict(joints=["nose"]), "no joint names"),
                     (dict(colormap="viridis"), "colormap must be one of"), (dict(colormap=np.zeros((255, 3), np.uint8)), r"\(256, 3\) uint8"),
                     (dict(alpha_mode="linear"), "alpha_mode must be"), (dict(alpha=1.5), "alpha must be in"), (dict(cutoff=0.0), "cutoff must be in"),
                     (dict(vmin=1.0, vmax=0.5), "hi must be above lo"), (dict(vmin=float("nan")), "lo and hi must be finite")):
        with pytest.raises(ValueError, match=text):
            post.draw_heatmaps(frame, maps, boxes, **kw)
    with pytest.raises(ValueError, match="integers"):
        post.draw_heatmaps(frame, maps, boxes.astype(np.float32))
    with pytest.raises(ValueError, match="one row per person"):
        post.draw_heatmaps(frame, maps, boxes[:1])
    assert not frame.any()
    assert load_pkg("native").heat_arguments(3, None, "gray", 0.6, "value", 0, 1, 0.1)[2::4] == (153, 26)      # round(255 x)


def fnv(data):
    h = 1469598103934665603
    for v in np.asarray(data, np.uint8).reshape(-1).tolist():
        h = ((h ^ v) * 1099511628211) & (2 ** 64 - 1)
    return h


def walk_cases():
    """(fmt code, h, w, maps, boxes, mask, lo, hi, (alpha, mode, cutoff)): the matrix on BGR and I420, the quantiser's vector, the
    overlap in both orders"""
    out = []
    for k, (name, h, w, maps, boxes, mask, setting, unchanged) in enumerate(heat_cases.matrix()):
        out.append((0 if k % 2 else 2, h, w, maps, boxes, mask, 0.0, 1.0, setting))
    for lo, hi in heat_cases.RANGES:
        maps = heat_cases.quantise_maps(lo, hi)
        boxes = np.asarray([[-3, 2, 60, 30], [10, 20, 70, 46]], np.int32)
        out += [(0, 46, 70, maps, boxes, None, lo, hi, (255, 0, 1)), (2, 46, 70, maps, boxes, [1, 0, 1], lo, hi, (200, 1, 3))]
    maps = heat_cases.random_maps(2, 16, 12, 5)
    out += [(2, 46, 70, maps, heat_cases.OVERLAPPING, None, -0.3, 0.9, (153, 1, 26)),
            (2, 46, 70, maps[::-1], heat_cases.OVERLAPPING[::-1], None, -0.3, 0.9, (153, 1, 26))]
    return out


def test_the_walk_under_sanitizers(tmp_path):
    """tests/heat_walk.cpp: the header alone, compiled for the host with AddressSanitizer and UBSan, over the cases above"""
    lib = load_pkg("_lib")
    cc, why = sanitizer_compiler(tmp_path)
    assert cc, "no host compiler links -fsanitize=address,undefined here: " + str(why)
    exe = tmp_path / "heat_walk"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "heat_walk.cpp")
    subprocess.run(cc + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fno-sanitize-recover=all",
                         "-I", lib.CSRC, "-o", str(exe), src], check=True)
    cases = walk_cases()
    lut = heat_ref.jet()
    with open(tmp_path / "cases.txt", "w") as f:
        for fmt, h, w, maps, boxes, mask, lo, hi, (alpha, mode, cutoff) in cases:
            n, J, hq, wq = maps.shape
            head = [fmt, h, w, hq, wq, n, J, alpha, mode, cutoff, int(F32(lo).view(np.uint32)), int(F32(hi).view(np.uint32))]
            body = list(mask if mask is not None else [1] * J) + np.asarray(boxes).reshape(-1).tolist() + \
                np.ascontiguousarray(maps, F32).view(np.uint32).reshape(-1).tolist() + lut.reshape(-1).tolist()
            f.write(" ".join(str(int(v)) for v in head + body) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    for (fmt, h, w, maps, boxes, mask, lo, hi, (alpha, mode, cutoff)), line in zip(cases, out):
        Q = heat_ref.quantise(maps, mask, lo, hi)
        V = heat_ref.value_plane(h, w, Q, boxes)
        a = heat_ref.alpha_of(V, alpha, mode)
        nbytes = h * w * 3 if fmt == 0 else h * w * 3 // 2
        canvas = ((131 * np.arange(nbytes, dtype=np.int64) + 17) & 255).astype(np.uint8)
        if fmt == 0:
            heat_ref.draw_bgr(canvas.reshape(h, w, 3), maps, boxes, lut, Q=Q, alpha=alpha, mode=mode, cutoff=cutoff)
        else:
            heat_ref.draw_yuv(canvas, h, w, "i420", maps, boxes, lut, Q=Q, alpha=alpha, mode=mode, cutoff=cutoff)
        want = (fnv(Q), fnv(V), int(((V >= cutoff) & (a > 0)).sum()), fnv(canvas))
        assert tuple(int(v) for v in line.split()) == want, (fmt, h, w, maps.shape, line)
    assert out[-1].split()[1:] == out[-2].split()[1:]   # the overlap in both orders: Q is per person, V and the canvas are not
