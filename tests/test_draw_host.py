"""Pose overlays without a GPU: the numpy restatement of the drawing definition (tests/draw_ref.py) against the literal shapes of
include/hrnet_mi355.h and against big-integer evaluation at the extreme legal coordinates, the declarations, every refusal of
``hrn_draw_poses`` on a plan-only handle, the palettes against the reference's recorded colours (tests/golden/palettes.json), and ``hrn_yuv_from_bgr`` over all 2^24
colours through the conversion the kernels are pinned to (tests/yuv_ref.py)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import draw_ref
import yuv_ref
from conftest import GOLDEN, load_pkg

TABLE_KEYS = [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")]


def rows(text):
    return np.asarray([[ch == "#" for ch in line] for line in text.split()], bool)


def test_discs_are_the_literal_masks():
    px, py = draw_ref.grid(9, 9)
    want = {1: rows(".........  .........  .........  ...###...  ...###...  ...###...  .........  .........  ........."),
            2: rows(".........  .........  ...###...  ..#####..  ..#####..  ..#####..  ...###...  .........  ........."),
            3: rows(".........  ...###...  ..#####..  .#######.  .#######.  .#######.  ..#####..  ...###...  .........")}
    for r, mask in want.items():
        np.testing.assert_array_equal(draw_ref.disc_mask(px, py, 4, 4, r), mask, err_msg="r = %d" % r)
    # r = 3: row half-widths 3, 3, 2, 1 at |dy| = 0 .. 3
    m = draw_ref.disc_mask(px, py, 4, 4, 3)
    assert [int(m[4 + d].sum()) for d in range(5)] == [7, 7, 5, 3, 0]


def test_bones_are_the_literal_masks():
    px, py = draw_ref.grid(7, 9)
    horizontal = rows(".........  .........  ..#####..  .#######.  ..#####..  .........  .........")   # 3 rows thick, one-pixel tips
    np.testing.assert_array_equal(draw_ref.bone_mask(px, py, (2, 3), (6, 3), 2), horizontal)
    np.testing.assert_array_equal(draw_ref.bone_mask(px, py, (6, 3), (2, 3), 2), horizontal)
    plus = rows(".........  .........  ....#....  ...###...  ....#....  .........  .........")           # P0 == P1
    np.testing.assert_array_equal(draw_ref.bone_mask(px, py, (4, 3), (4, 3), 2), plus)
    px, py = draw_ref.grid(7, 7)
    # 45 degrees, (1, 1) -> (4, 4): the diagonal, its two neighbours (4 * 1 <= 4 * 18 / 18 ... cross = +-1: 4 <= 4 * 18), tips by the caps
    diagonal = rows(".#.....  ###....  .###...  ..###..  ...###.  ....#..  .......")
    np.testing.assert_array_equal(draw_ref.bone_mask(px, py, (1, 1), (4, 4), 2), diagonal)
    np.testing.assert_array_equal(draw_ref.bone_mask(px, py, (4, 4), (1, 1), 2), diagonal)


def bone_covers_bigint(p, p0, p1, T):
    (x, y), (x0, y0), (x1, y1) = p, p0, p1      # Python integers: no width at all
    dx, dy, wx, wy = x1 - x0, y1 - y0, x - x0, y - y0
    L2, t = dx * dx + dy * dy, wx * dx + wy * dy
    if t <= 0:
        return 4 * (wx * wx + wy * wy) <= T * T
    if t >= L2:
        return 4 * ((x - x1) ** 2 + (y - y1) ** 2) <= T * T
    return 4 * (wx * dy - wy * dx) ** 2 <= T * T * L2


def test_restatement_at_the_extreme_coordinates():
    """int64 holds every expression for frame sides up to 8192 and live coordinates in [-8192, 16383]: the restatement against
    exact integers along bones between the corners of that range, on the pixels around where they cross the last row / column"""
    lo, hi = draw_ref.LO, draw_ref.HI
    ends = [((lo, lo), (hi, hi)), ((hi, lo), (lo, hi)), ((lo, hi), (hi, 8191)), ((hi, hi), (lo, lo)), ((lo, 8191), (hi, 8190)),
            ((8191, lo), (8190, hi)), ((hi, hi), (hi, hi)), ((lo, lo), (lo, lo)), ((8191, 8191), (hi, hi))]
    ys = np.asarray([0, 1, 4095, 8189, 8190, 8191], np.int64)
    py, px = np.meshgrid(ys, ys, indexing="ij")
    for T in (1, 2, 16):
        for p0, p1 in ends:
            got = draw_ref.bone_mask(px, py, p0, p1, T)
            want = np.asarray([[bone_covers_bigint((int(x), int(y)), p0, p1, T) for x in ys] for y in ys])
            np.testing.assert_array_equal(got, want, err_msg=str((T, p0, p1)))
    # the largest magnitudes, by hand: 4 cross^2 < 2^62 and T^2 L2 far below
    cross = 2 * 16383 * 24575
    assert 4 * cross * cross < 2 ** 62 and 4 * (64 * 64 + 64) * 2 * 24575 ** 2 < 2 ** 62
    # a disc far outside and one on the last pixel
    px, py = draw_ref.grid(4, 4)
    assert not draw_ref.disc_mask(px, py, hi, hi, 64).any() and not draw_ref.disc_mask(px, py, lo, lo, 64).any()
    assert draw_ref.disc_mask(px + 8188, py + 8188, 8191, 8191, 1).sum() == 4


def test_liveness_of_the_restatement():
    j = draw_ref.live_joints(np.asarray([[3.9, -0.7, 0.9], [1, 1, 0.5], [1, 1, np.nan], [np.nan, 1, 1], [1, np.inf, 1], [20000, 1, 1],
                                         [1, -20000, 1], [-8192.9, 16383.9, 1], [-8193, 0, 1], [0, 16384, 1]], np.float32), 0.5)
    assert j == [(0, 3), None, None, None, None, None, None, (16383, -8192), None, None]


def test_symbols_are_declared_and_exported():
    lib = load_pkg("_lib")
    names = {"hrn_draw_poses", "hrn_yuv_from_bgr"}
    assert names <= set(lib.header_symbols()) and names <= set(lib.SYMBOLS)
    assert "draw.hip" in lib.SOURCES and os.path.exists(os.path.join(lib.CSRC, "draw.hip"))
    L = lib.load()
    for name in names:
        assert hasattr(L, name)
    assert L.hrn_draw_poses(None, None, 0, None, 0, 17, None, None, 0, None, 1, None, 1, None, 0, 2, 0.5, None) == 1   # no handle
    text = open(os.path.join(lib.INCLUDE, "hrnet_mi355.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fields = re.search(r"typedef struct \{([^}]*)\} hrn_canvas;", bare).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [f[0] for f in lib.CanvasC._fields_]
    assert ctypes.sizeof(lib.CanvasC) == 56
    assert re.search(r"\bHRN_PIX_BGR = 0\b", text)
    assert "fits signed 64" in text and "2^62" in text        # the integer ranges are stated where the contract is
    native = load_pkg("native")
    kernels = open(os.path.join(lib.CSRC, "kernels.h")).read()
    assert re.search(r"kDrawTile = %d;" % native.DRAW_TILE, kernels)


def test_draw_refusals_need_no_gpu():
    """a plan-only handle (device = -1): every argument error is reported as such, and a good call as 'plan-only'"""
    pkg = load_pkg()
    lib = load_pkg("_lib")
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h

    def bgr(**change):
        e = lib.CanvasC()
        e.y, e.height, e.width, e.pitch_y, e.format = 4096, 120, 160, 480, 0      # never touched: nothing is launched
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

    skel = np.asarray([[0, 1], [1, 16]], np.int32)
    colours = np.arange(12, dtype=np.uint8).reshape(4, 3)
    good = dict(table=table_of(bgr(), lib.CanvasC()), nframes=2, pts=4096, n=2, J=17, idx=np.zeros(2, np.int32), skel=skel, K=2, pc=colours,
                Cp=4, bc=colours, Cb=4, ids=None, radius=0, T=2)

    def call(**change):
        a = dict(good, **change)
        p = lambda v: None if v is None else (v.ctypes.data if isinstance(v, np.ndarray) else v)   # noqa: E731
        rc = L.hrn_draw_poses(h, a["table"], a["nframes"], a["pts"], a["n"], a["J"], p(a["idx"]), p(a["skel"]), a["K"], p(a["pc"]),
                              a["Cp"], p(a["bc"]), a["Cb"], p(a["ids"]), a["radius"], a["T"], 0.5, None)
        return rc, L.hrn_last_error(h).decode()

    # good calls: BGR, both YUV layouts, one frame without an index, ids given, n == 0 (the handle is judged first), K == 0
    for change in (dict(), dict(table=table_of(yuv(1), lib.CanvasC())), dict(table=table_of(yuv(2), yuv(1, y=16384)), idx=np.asarray([0, 1], np.int32)),
                   dict(nframes=1, idx=None), dict(ids=np.asarray([-3, 9], np.int32)), dict(n=0), dict(n=0, pts=None),
                   dict(K=0, skel=None), dict(radius=64, T=16), dict(T=1, J=256), dict(table=table_of(bgr(height=8192, width=8192, pitch_y=24576)), nframes=1)):
        rc, err = call(**change)
        assert rc == 7 and "plan-only" in err, (change.keys(), err)
    refused = [
        (dict(table=None), "null canvases / joints / skeleton / colours"), (dict(pts=None), "null canvases"),
        (dict(skel=None), "null canvases"), (dict(pc=None), "null canvases"), (dict(bc=None), "null canvases"),
        (dict(nframes=0), "null canvases"),
        (dict(n=-1), "n is negative"),
        (dict(J=0), "J must be in [1, 256]"), (dict(J=257), "J must be in [1, 256]"),
        (dict(K=-1), "K must be in"),
        (dict(Cp=0), "Cp and Cb must be at least 1"), (dict(Cb=0), "Cp and Cb must be at least 1"), (dict(Cb=-2), "Cp and Cb"),
        (dict(T=0), "thickness must be in [1, 16]"), (dict(T=17), "thickness must be in [1, 16]"),
        (dict(radius=-1), "radius must be in [0, 64]"), (dict(radius=65), "radius must be in [0, 64]"),
        (dict(idx=None), "without frame_index there must be one frame"),
        (dict(skel=np.asarray([[0, 1], [1, 17]], np.int32)), "skeleton index 17 of bone 1 is outside [0, 17)"),
        (dict(skel=np.asarray([[-1, 1], [1, 2]], np.int32)), "skeleton index -1 of bone 0 is outside [0, 17)"),
        (dict(idx=np.asarray([0, 2], np.int32)), "frame_index 2 of person 1 is outside [0, 2)"),
        (dict(idx=np.asarray([-1, 0], np.int32)), "frame_index -1 of person 0 is outside [0, 2)"),
        (dict(idx=np.asarray([0, 1], np.int32)), "canvas 1, which person 1 is drawn on, is null"),
    ]
    for change, text in refused:
        rc, err = call(**change)
        assert rc == 7 and "hrn_draw_poses" in err and text in err, (list(change), err)
    faults = [
        (bgr(y=None), "is null"), (bgr(height=0), "non-positive width or height"), (bgr(width=-4), "non-positive width or height"),
        (bgr(height=8193, pitch_y=480), "side above 8192"), (bgr(width=8193, pitch_y=3 * 8193), "side above 8192"),
        (bgr(pitch_y=479), "pitch below three times its width"), (bgr(format=3), "unknown format"), (bgr(format=-1), "unknown format"),
        (yuv(1, height=121), "odd width or height"), (yuv(2, width=159), "odd width or height"), (yuv(1, width=8194, pitch_y=8194), "side above 8192"),
        (yuv(1, pitch_y=158), "pitch_y below its width"), (yuv(1, pitch_c=158), "pitch_c below its width"),
        (yuv(2, pitch_c=79), "pitch_c below half its width"), (yuv(1, u=None), "null plane"), (yuv(2, v=None), "null plane"),
        (yuv(1, y=None), "null plane"),
    ]
    for entry, text in faults:
        first = yuv(1) if entry.format in (1, 2) else bgr()
        rc, err = call(table=table_of(first, entry), idx=np.asarray([0, 1], np.int32))
        assert rc == 7 and "canvas 1, which person 1 is drawn on, " in err and text in err, (text, err)
        rc, err = call(table=table_of(first, entry))                      # ... while nobody referring to it is fine
        assert rc == 7 and "plan-only" in err, (text, err)
    # two canvases people are drawn on that name the same buffer (one writer per byte needs disjoint canvases); unreferenced: fine
    rc, err = call(table=table_of(bgr(), bgr(height=60)), idx=np.asarray([0, 1], np.int32))
    assert rc == 7 and "canvases 0 and 1 name the same buffer" in err and "must not overlap" in err, err
    rc, err = call(table=table_of(bgr(), bgr(height=60)))
    assert rc == 7 and "plan-only" in err, err
    rc, err = call(table=table_of(bgr(), bgr(y=8192)), idx=np.asarray([0, 1], np.int32))
    assert rc == 7 and "plan-only" in err, err
    for pair in ((bgr(), yuv(1)), (yuv(2), bgr())):
        rc, err = call(table=table_of(*pair), idx=np.asarray([0, 1], np.int32))
        assert rc == 7 and "mixes formats" in err and "all BGR or all YUV" in err, err
    net.close()


DEMO_PALETTES = [("tab20", 16), ("Set2", 8), ("gist_rainbow", 10), ("jet", 8)]


def recorded_palettes():
    """tests/golden/palettes.json: the colours the reference's draw_points / draw_skeleton derive from a palette name and a sample
    count, recorded by running its expression -- {(name, samples): [[B, G, R], ...]}"""
    cases = json.load(open(os.path.join(GOLDEN, "palettes.json")))["cases"]
    return {(c["name"], c["samples"]): c["bgr"] for c in cases}


def test_embedded_palettes_equal_the_recorded_colours():
    native = load_pkg("native")
    recorded = recorded_palettes()
    assert set(DEMO_PALETTES) <= set(recorded) and len(recorded) > len(DEMO_PALETTES)
    for name, samples in DEMO_PALETTES:
        got = native.embedded_palette(name, samples)
        assert got.dtype == np.uint8 and got.tolist() == recorded[(name, samples)], name
    assert native.embedded_palette("jet", 9) is None and native.embedded_palette("viridis", 5) is None
    assert native.embedded_palette("tab20", 3).tolist() == recorded[("tab20", 16)]      # a listed palette ignores the count


def test_palette_equals_the_recorded_colours():
    """with matplotlib: every recorded case, listed and sampled; without it: the demo palettes, from the stored tables"""
    native = load_pkg("native")
    try:
        import matplotlib  # noqa: F401
        cases = recorded_palettes()
    except ImportError:
        cases = {k: v for k, v in recorded_palettes().items() if k in DEMO_PALETTES}
    for (name, samples), want in cases.items():
        got = native.palette(name, samples)
        assert got.dtype == np.uint8 and got.ndim == 2 and got.shape[1] == 3 and got.flags.c_contiguous
        assert got.tolist() == want, (name, samples)
    with pytest.raises(ValueError):
        native.palette("no such palette", 4)


def test_embedded_palettes_serve_without_matplotlib(monkeypatch):
    import builtins
    native = load_pkg("native")
    real = builtins.__import__

    def no_matplotlib(name, *a, **k):
        if name.startswith("matplotlib"):
            raise ImportError(name)
        return real(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_matplotlib)
    monkeypatch.setattr(native, "_PALETTE_CACHE", {})
    assert native.palette("tab20", 16).shape == (20, 3) and native.palette("Set2", 8).shape == (8, 3)
    assert native.palette("gist_rainbow", 10).tolist()[0] == [41, 0, 255] and native.palette("jet", 8).tolist()[-1] == [0, 0, 128]
    with pytest.raises(ValueError, match="not stored"):
        native.palette("jet", 9)
    with pytest.raises(ValueError, match="not stored"):
        native.palette("viridis", 8)


def test_coco_skeleton_fixture():
    sk = json.load(open(os.path.join(GOLDEN, "coco_skeleton.json")))["coco_skeleton"]
    assert len(sk) == 19 and all(len(p) == 2 and 0 <= min(p) and max(p) < 17 for p in sk)


@pytest.mark.parametrize("key", TABLE_KEYS, ids=["%s-%s" % k for k in TABLE_KEYS])
def test_yuv_from_bgr_round_trip_over_every_colour(key):
    """every (B, G, R) through hrn_yuv_from_bgr and back through the restatement the kernels are pinned to: at most 2 grey levels
    for the limited-range tables, at most 1 for the full-range ones"""
    native = load_pkg("native")
    table = yuv_ref.TABLES[key]
    gr = np.arange(65536, dtype=np.int64)
    worst, at_worst, total = 0, 0, 0
    for b0 in range(0, 256, 32):
        b = np.repeat(np.arange(b0, b0 + 32, dtype=np.uint8), 65536)
        g, r = np.tile((gr >> 8).astype(np.uint8), 32), np.tile((gr & 255).astype(np.uint8), 32)
        bgr = np.stack([b, g, r], -1)
        yuv = native.bgr_to_yuv_colors(bgr, *key)
        back = np.stack(yuv_ref.convert(yuv[:, 0], yuv[:, 1], yuv[:, 2], table), -1)
        err = np.abs(back.astype(np.int16) - bgr.astype(np.int16)).max(1)
        if int(err.max()) > worst:
            worst, at_worst = int(err.max()), 0
        at_worst += int((err == worst).sum())
        total += len(err)
    print("hrn_yuv_from_bgr round trip, %s %s: max error %d (%.2f %% of colours there)" % (key + (worst, 100.0 * at_worst / total)))
    assert worst <= (2 if key[1] == "limited" else 1)
    # by hand: white, black and the primaries of BT.601 limited
    if key == ("bt601", "limited"):
        got = native.bgr_to_yuv_colors(np.asarray([[255, 255, 255], [0, 0, 0], [0, 0, 255], [255, 0, 0]], np.uint8), *key).tolist()
        assert got == [[235, 128, 128], [16, 128, 128], [81, 90, 240], [41, 240, 110]]
    L = load_pkg("_lib").load()
    out = np.zeros(3, np.uint8)
    assert L.hrn_yuv_from_bgr(2, 0, out.ctypes.data, 1, out.ctypes.data) == 7 and L.hrn_yuv_from_bgr(0, 2, out.ctypes.data, 1, out.ctypes.data) == 7
    assert L.hrn_yuv_from_bgr(0, 0, None, 1, out.ctypes.data) == 7 and L.hrn_yuv_from_bgr(0, 0, None, 0, None) == 0
