"""The face mosaic without a GPU: ``hrn_mosaic_regions`` / ``hrn_mosaic_host`` -- the text the kernels compile,
csrc/mosaic_math.h -- against the numpy restatement of the definition (tests/mosaic_ref.py), whole buffers byte for byte on
noise canvases with sentinel bytes in the pitch, status for status; the properties the header states; the declarations; every
refusal with its message; and the same cases walked by a stand-alone C++ program under AddressSanitizer and UBSan (a child
process of its own; nothing is preloaded into Python)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mosaic_cases
import mosaic_ref
import yuv_ref
from conftest import load_pkg
from mosaic_cases import BOXES, CELLS, F32, HEAD, SETTINGS, noise
from test_heatmaps_host import canvas_entries
from test_labels_host import sanitizer_compiler

FORMATS = ["bgr", "nv12", "i420"]
SIZES = {"bgr": (37, 53), "nv12": (38, 54), "i420": (38, 54)}
GUARD = 26      # bytes of pitch beyond a row of a YUV canvas (BGR: 5, odd on purpose)


class Canvas:
    """a noise canvas of one format with sentinel bytes behind every row: `frame` is what the library changes, `buffer` every
    byte of it, `expected(rects, cell)` the restatement's result on a copy"""

    def __init__(self, fmt, seed, size=None):
        pkg = load_pkg()
        self.fmt = fmt
        self.h, self.w = h, w = size or SIZES[fmt]
        if fmt == "bgr":
            self.pitch = 3 * w + 5
            self.buffer = noise(h * self.pitch, seed)
            self.frame = np.lib.stride_tricks.as_strided(self.buffer, (h, w, 3), (self.pitch, 3, 1))
        else:
            self.pitch = w + GUARD
            self.buffer = noise(yuv_ref.nbytes(h, w, self.pitch), seed)
            self.frame = pkg.YuvFrame(self.buffer, h, w, fmt, "bt601", "limited", self.pitch)
            assert np.shares_memory(self.frame.data.numpy(), self.buffer)
        self.before = self.buffer.copy()

    def view(self, buffer):
        return np.lib.stride_tricks.as_strided(buffer, (self.h, self.w, 3), (self.pitch, 3, 1))

    def expected(self, rects, cell):
        want = self.before.copy()
        if self.fmt == "bgr":
            mosaic_ref.mosaic_bgr(self.view(want), rects, cell)
        else:
            mosaic_ref.mosaic_yuv(want, self.h, self.w, self.fmt, rects, cell, self.pitch)
        return want


def run_and_compare(fmt, seed, cell, pts=None, boxes=None, joints=None, threshold=0.5, scale=(1, 1), min_half=None, size=None):
    """the library's host form and the restatement on the same canvas; returns (before, after, status), the two having been held
    equal in every byte and status"""
    post = load_pkg("postproc")
    c = Canvas(fmt, seed, size)
    rects, status = mosaic_ref.regions((c.h, c.w), pts, boxes, joints, threshold, scale, min_half or 0)
    out, got_status = post.mosaic(c.frame, pts=pts, boxes=boxes, joints=joints, confidence_threshold=threshold, scale=scale,
                                  min_half=min_half, cell=cell, return_status=True)
    assert out is c.frame
    np.testing.assert_array_equal(got_status, status, err_msg=str((fmt, cell, joints, scale, min_half)))
    np.testing.assert_array_equal(c.buffer, c.expected(rects, cell or 0), err_msg=str((fmt, cell, joints, scale, min_half)))
    return c.before, c.buffer, got_status


def test_symbols_are_declared_and_exported_and_the_header_is_one_text():
    lib = load_pkg("_lib")
    names = {"hrn_mosaic_dev", "hrn_mosaic_regions", "hrn_mosaic_host", "hrn_mosaic_last_error"}
    assert names <= set(lib.header_symbols()) and names <= set(lib.SYMBOLS)
    assert set(lib.header_symbols()) == set(lib.SYMBOLS)
    assert "mosaic.hip" in lib.SOURCES
    math_h = os.path.join(lib.CSRC, "mosaic_math.h")
    assert math_h in lib._deps("mosaic.hip") and math_h in lib._deps("hrnet_mi355.cpp")
    kernel, host = open(os.path.join(lib.CSRC, "mosaic.hip")).read(), open(os.path.join(lib.CSRC, "hrnet_mi355.cpp")).read()
    assert '#include "mosaic_math.h"' in kernel and '#include "mosaic_math.h"' in host
    for fn in ("mosaic_region(", "mosaic_region_of_box(", "mosaic_cell_count(", "mosaic_mean(", "mosaic_joint_live(", "mosaic_meets("):
        assert fn in kernel and (fn in host or fn in open(math_h).read()), fn       # both sides call the one text; neither restates it
    code = "\n".join(line.split("//")[0] for line in kernel.splitlines())
    assert "mosaic_build_kernel" in code and "mosaic_raster_kernel" in code and "atomic" not in code.lower()
    assert "block_compact(" in code and "frame_of_tile(" in code and "__shfl_xor(" in code
    L = lib.load()
    for name in names:
        assert hasattr(L, name)
    text = open(os.path.join(lib.INCLUDE, "hrnet_mi355.h")).read()
    for phrase in ("R = max(rmin, (E scale_num + scale_den - 1) / scale_den)", "rmin = (P + 15) / 16", "(sum + (c >> 1)) / c",
                   "E * 64 < 2^21", "is not irreversible anonymisation", "BEFORE hrn_draw_heatmaps_dev / hrn_draw_poses / hrn_draw_labels_dev"):
        assert phrase in text, phrase
    assert L.hrn_mosaic_dev(None, None, 0, None, 0, 1, None, 1, None, None, 0.5, 1, 1, 0, 0, None, None) == 1      # no handle
    pkg = load_pkg()
    assert "COCO_HEAD_JOINTS" in pkg.__all__ and pkg.COCO_HEAD_JOINTS == (0, 1, 2, 3, 4)
    assert callable(pkg.NativeHRNet.mosaic) and callable(pkg.postproc.mosaic) and callable(pkg.postproc.mosaic_regions)


def test_regions_equal_the_restatement_and_the_rules_by_hand():
    post = load_pkg("postproc")
    pts = mosaic_cases.all_people()
    n = len(pts)
    sizes = np.stack([np.arange(n) % 3 * 500 + 37, np.arange(n) % 4 * 300 + 53], 1).astype(np.int32)
    seen = set()
    for joints, threshold, scale, min_half in SETTINGS:
        for hw in ((37, 53), sizes):
            got, status = post.mosaic_regions(hw, pts=pts, joints=joints, confidence_threshold=threshold, scale=scale, min_half=min_half)
            want, want_status = mosaic_ref.regions(hw, pts, None, joints, threshold, scale, min_half or 0)
            assert got.dtype == np.int32 and got.shape == (n, 4) and status.dtype == np.int32
            np.testing.assert_array_equal(status, want_status, err_msg=str((joints, scale, min_half)))
            np.testing.assert_array_equal(got, want, err_msg=str((joints, scale, min_half)))
            seen |= set(status.tolist())
    assert seen == {0, 1, 2}
    by_name = {name: i for i, (name, _) in enumerate(mosaic_cases.people())}
    region = lambda name, **kw: tuple(r[by_name[name]].tolist() for r in post.mosaic_regions((1000, 1000), pts=pts, joints=HEAD, **kw))   # noqa: E731
    # the frontal face: X 15..25, Y 10..12, E = 10; the body reaches Y = 36: P = 26, rmin = 2; R = 10; cx2 = 40, cy2 = 22
    assert region("a frontal face, the body below") == ([10, 1, 31, 22], 0)
    assert region("a frontal face, the body below", scale=(3, 2)) == ([5, 0, 36, 27], 0)            # R = 15, clipped at the top
    assert region("a frontal face, the body below", min_half=12) == ([8, 0, 33, 24], 0)
    # the profile: one pixel (30, 8), E = 0; P = max(33 - 28, 37 - 8) = 29, rmin = (29 + 15) / 16 = 2: a 5 x 5 square
    assert region("profile: the listed joints on one pixel, rmin decides") == ([28, 6, 33, 11], 0)
    assert region("profile: the listed joints on one pixel, rmin decides", scale=(64, 1)) == ([28, 6, 33, 11], 0)   # E = 0: the scale has nothing to grow
    assert region("profile, nobody else: a single pixel") == ([30, 8, 31, 9], 0)
    assert region("an odd centre") == ([18, 10, 26, 18], 0)                 # cx2 = 43: 21 - 3 .. 22 + 3 + 1; cy2 = 27: 13 - 3 .. 14 + 3 + 1
    assert region("a negative odd centre") == ([0, 0, 3, 6], 0)             # cx2 = -7: floor -> -4 - 5 .. -3 + 5 + 1; cy2 = -1: -1 - 5 .. 0 + 5 + 1
    assert region("truncation towards zero") == ([0, 0, 1, 1], 0)
    assert region("equality with the threshold is not live") == ([40, 30, 41, 31], 0)
    assert region("the ends of the range: the region covers everything") == ([0, 0, 1000, 1000], 0)
    assert region("the ends of the range: the region covers everything", scale=(64, 1)) == ([0, 0, 1000, 1000], 0)
    assert region("one step beyond the range: not live") == ([0, 0, 0, 0], 1)
    assert region("beyond the range, one joint left") == ([33, 20, 34, 21], 0)
    assert region("nobody live") == ([0, 0, 0, 0], 1) and region("only NaN") == ([0, 0, 0, 0], 1)
    assert region("the list is dead, the body lives") == ([0, 0, 0, 0], 1)
    assert region("wholly outside", confidence_threshold=0.5)[1] == 0 and post.mosaic_regions((37, 53), pts=pts, joints=HEAD)[1][by_name["wholly outside"]] == 2
    # boxes: the box itself, clipped; all-zero and degenerate boxes have no region
    got, status = post.mosaic_regions((37, 53), boxes=BOXES)
    want, want_status = mosaic_ref.regions((37, 53), None, BOXES)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(status, want_status)
    assert status.tolist() == [0, 1, 1, 1, 0, 0, 2, 2, 0, 0, 0, 0] and got[9].tolist() == [0, 0, 53, 37] and got[4].tolist() == [0, 0, 4, 3]
    empty = post.mosaic_regions((37, 53), pts=np.zeros((0, 17, 3), F32))
    assert empty[0].shape == (0, 4) and empty[1].shape == (0,)


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_host_form_equals_the_restatement(fmt):
    pts = mosaic_cases.all_people()
    changed = 0
    for k, cell in enumerate(CELLS):
        for m, (joints, threshold, scale, min_half) in enumerate(SETTINGS):
            before, after, _ = run_and_compare(fmt, 10 * k + m, cell, pts=pts, joints=joints, threshold=threshold, scale=scale, min_half=min_half)
            changed += int((before != after).any())
        run_and_compare(fmt, 100 + k, cell, boxes=BOXES)
    assert changed == len(CELLS) * len(SETTINGS)
    # every designed person alone, at a small and at the largest cell: a region inside one cell, over partial edge cells, outside
    for i, (name, p) in enumerate(mosaic_cases.people()):
        for cell in (8, 32):
            before, after, status = run_and_compare(fmt, 200 + i, cell, pts=p[None], joints=HEAD)
            assert (status[0] == 0) == bool((before != after).any()), name      # (noise: a flattened cell changes)
    h, w = SIZES[fmt]
    before, after, _ = run_and_compare(fmt, 300, 32, pts=mosaic_cases.people()[1][1][None], joints=HEAD)       # inside one cell: that cell, whole
    if fmt == "bgr":
        c = Canvas(fmt, 300)
        img, was = c.view(after), c.view(before)
        assert (img[:32, :32] == img[0, 0]).all() and (img[32:] == was[32:]).all() and (img[:, 32:] == was[:, 32:]).all()
        assert img[0, 0].tolist() == [(int(was[:32, :32, ch].astype(np.int64).sum()) + 512) // 1024 for ch in range(3)]
    # the region (46, 29, 53, 37) lies in the two right-hand cells: 21 x 32 pixels, and the corner cell of 21 x 5
    before, after, _ = run_and_compare(fmt, 301, 32, pts=mosaic_cases.people()[2][1][None], joints=HEAD)
    if fmt == "bgr":
        c = Canvas(fmt, 301)
        img, was = c.view(after), c.view(before)
        assert (img[32:, 32:] == img[36, 52]).all() and (img[:32, 32:] == img[0, 52]).all() and (img[:, :32] == was[:, :32]).all()
        assert img[36, 52].tolist() == [(int(was[32:, 32:, ch].astype(np.int64).sum()) + 52) // 105 for ch in range(3)]
        assert img[0, 52].tolist() == [(int(was[:32, 32:, ch].astype(np.int64).sum()) + 336) // 672 for ch in range(3)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_properties_the_header_states(fmt):
    post = load_pkg("postproc")
    designed = [p for name, p in mosaic_cases.people() if "the ends of the range" not in name]      # (those cover the whole canvas)
    pts = np.concatenate([np.stack(designed), mosaic_cases.scattered(40, *SIZES[fmt], seed=5, spread=(20, 30))])
    for cell in (4, 16):
        _, one, status = run_and_compare(fmt, 7, cell, pts=pts, joints=HEAD)
        order = np.random.default_rng(cell).permutation(len(pts))
        _, other, permuted = run_and_compare(fmt, 7, cell, pts=pts[order], joints=HEAD)
        np.testing.assert_array_equal(one, other)                           # the order of the people does not matter
        np.testing.assert_array_equal(status[order], permuted)
        c = Canvas(fmt, 7)
        post.mosaic(c.frame, pts=pts, joints=HEAD, cell=cell)
        np.testing.assert_array_equal(c.buffer, one)
        post.mosaic(c.frame, pts=pts, joints=HEAD, cell=cell)               # a second identical call changes no byte
        np.testing.assert_array_equal(c.buffer, one)
        # overlaps do not matter: the people one at a time, each on the result of the one before, mark the same set of cells -- but
        # a cell flattened twice keeps its first mean, so the bytes are the same as well
        c = Canvas(fmt, 7)
        for p in pts:
            post.mosaic(c.frame, pts=p[None], joints=HEAD, cell=cell)
        np.testing.assert_array_equal(c.buffer, one)
        # sentinels: the pitch padding, and every cell no region touches
        rects, _ = mosaic_ref.regions(SIZES[fmt], pts, None, HEAD)
        m = mosaic_ref.marks(*SIZES[fmt], cell, rects)
        assert m.any() and not m.all()
        h, w = SIZES[fmt]
        if fmt == "bgr":
            rows_before, rows_after = c.before.reshape(h, c.pitch), one.reshape(h, c.pitch)
            np.testing.assert_array_equal(rows_after[:, 3 * w:], rows_before[:, 3 * w:])
            untouched = ~np.repeat(np.repeat(m, cell, 0), cell, 1)[:h, :w]
            np.testing.assert_array_equal(c.view(one)[untouched], c.view(c.before.copy())[untouched])
        else:
            rows_before, rows_after = c.before.reshape(-1, c.pitch), one.reshape(-1, c.pitch)
            np.testing.assert_array_equal(rows_after[:h, w:], rows_before[:h, w:])
            if fmt == "nv12":
                np.testing.assert_array_equal(rows_after[h:, w:], rows_before[h:, w:])
            untouched = ~np.repeat(np.repeat(m, cell, 0), cell, 1)[:h, :w]
            np.testing.assert_array_equal(rows_after[:h, :w][untouched], rows_before[:h, :w][untouched])


def test_the_cell_rule_and_two_canvases():
    pkg, post = load_pkg(), load_pkg("postproc")
    for size, s in (((40, 50), 8), ((1023, 1100), 8), ((1024, 1030), 16), ((1100, 2047), 16), ((2048, 2050), 32), ((720, 1280), 8),
                    ((1080, 1920), 16), ((2160, 3840), 32), ((8192, 8192), 32)):
        assert mosaic_ref.cell_size(0, *size) == s, size
    faces = np.concatenate([mosaic_cases.scattered(4, 40, 50, seed=3), mosaic_cases.scattered(6, 1024, 1030, seed=3)])
    for fmt, size in (("bgr", (40, 50)), ("bgr", (1024, 1030)), ("bgr", (2048, 2050)), ("nv12", (1024, 1030)), ("i420", (2048, 2050))):
        before, after, status = run_and_compare(fmt, 11, None, pts=faces, joints=HEAD, size=size)
        _, same, _ = run_and_compare(fmt, 11, mosaic_ref.cell_size(0, *size), pts=faces, joints=HEAD, size=size)
        np.testing.assert_array_equal(after, same)
        assert (status == 0).any() and (before != after).any()
    # two canvases of different sizes and one nobody refers to; cell 0 gives each canvas its own size
    sizes = [(46, 70), None, (1030, 1100)]
    frame_index = np.asarray([0, 2, 2, 0, 2, 0, 0], np.int32)
    pts = mosaic_cases.scattered(len(frame_index), 46, 70, seed=9)
    before = [None if s is None else noise(s + (3,), 20 + k) for k, s in enumerate(sizes)]
    frames = [None if b is None else b.copy() for b in before]
    out, status = post.mosaic(frames, pts=pts, joints=HEAD, frame_index=frame_index, return_status=True)
    assert out[1] is None and out[0] is frames[0]
    hw = np.asarray([sizes[f] for f in frame_index])
    rects, want_status = mosaic_ref.regions(hw, pts, None, HEAD)
    np.testing.assert_array_equal(status, want_status)
    want = mosaic_ref.mosaic_clip([None if b is None else b.copy() for b in before], rects, frame_index, 0)
    for f in (0, 2):
        np.testing.assert_array_equal(frames[f], want[f], err_msg="frame %d" % f)
        assert (frames[f] != before[f]).any()
    key = ("bt601", "limited")
    sizes = [(46, 70), None, (70, 100)]
    data = [None if s is None else noise(yuv_ref.nbytes(s[0], s[1], s[1] + GUARD), 30 + k) for k, s in enumerate(sizes)]
    yuv = [None if s is None else pkg.YuvFrame(d, s[0], s[1], "nv12", key[0], key[1], s[1] + GUARD) for s, d in zip(sizes, data)]
    want = [None if d is None else d.copy() for d in data]
    post.mosaic(yuv, pts=pts, joints=HEAD, frame_index=frame_index, cell=4)
    for f in (0, 2):
        who = frame_index == f
        rects, _ = mosaic_ref.regions(sizes[f], pts[who], None, HEAD)
        mosaic_ref.mosaic_yuv(want[f], sizes[f][0], sizes[f][1], "nv12", rects, 4, sizes[f][1] + GUARD)
        np.testing.assert_array_equal(data[f], want[f], err_msg="NV12 frame %d" % f)
    with pytest.raises(ValueError, match="frame_index"):
        post.mosaic(frames, pts=pts, joints=HEAD)
    with pytest.raises(ValueError, match="is null"):
        post.mosaic(frames, pts=pts[:1], joints=HEAD, frame_index=[1])


LIST = np.asarray([0, 1, 2, 3, 4], np.int32)
REFUSED = [
    (dict(n=-1), "n is negative"),
    (dict(boxes=8192), "people come from pts or from boxes, not from both"), (dict(pts=None), "null pts and boxes: people come from one of them"),
    (dict(J=0), "J must be in [1, 256]"), (dict(J=257), "J must be in [1, 256]"),
    (dict(K=0), "K must be in [1, 256]"), (dict(K=257), "K must be in [1, 256]"), (dict(joints=None), "null joint list"),
    (dict(joints=np.asarray([0, 1, 17, 3, 4], np.int32)), "joint index 17 at position 2 of the list is outside [0, 17)"),
    (dict(joints=np.asarray([0, -1, 2, 3, 4], np.int32)), "joint index -1 at position 1 of the list is outside [0, 17)"),
    (dict(scale_num=0), "scale_num and scale_den must be in [1, 64]"), (dict(scale_num=65), "scale_num and scale_den must be in [1, 64]"),
    (dict(scale_den=0), "scale_num and scale_den must be in [1, 64]"), (dict(scale_den=65), "scale_num and scale_den must be in [1, 64]"),
    (dict(min_half=-1), "min_half must be in [0, 4096]"), (dict(min_half=4097), "min_half must be in [0, 4096]"),
    (dict(cell=1), "cell must be 0, 2, 4, 8, 16 or 32"), (dict(cell=3), "cell must be 0, 2, 4, 8, 16 or 32"), (dict(cell=64), "cell must be 0, 2, 4, 8, 16 or 32"),
    (dict(cell=-2), "cell must be 0, 2, 4, 8, 16 or 32"), (dict(cell=12), "cell must be 0, 2, 4, 8, 16 or 32"),
    (dict(table=None), "null canvases"), (dict(nframes=0), "null canvases"),
    (dict(idx=None), "without frame_index there must be one frame"),
    (dict(idx=np.asarray([0, 2], np.int32)), "frame_index 2 of person 1 is outside [0, 2)"),
    (dict(idx=np.asarray([-1, 0], np.int32)), "frame_index -1 of person 0 is outside [0, 2)"),
    (dict(idx=np.asarray([0, 1], np.int32)), "canvas 1, which person 1 is drawn on, is null"),
]


def refusal_calls(lib, call, prefix, accepted, boxes):
    """every refusal against `call(**change) -> (rc, error text)`; `accepted(rc, err)`: what a good call answers"""
    bgr, yuv, table_of = canvas_entries(lib)
    for change in (dict(), dict(nframes=1, idx=None), dict(n=0), dict(n=0, pts=None), dict(n=0, pts=None, joints=None, J=0, K=0),
                   dict(pts=None, boxes=boxes), dict(pts=None, boxes=boxes, joints=None, J=0, K=0), dict(K=1), dict(scale_num=64, scale_den=64),
                   dict(min_half=4096), dict(cell=0), dict(cell=2), dict(cell=32), dict(joints=np.zeros(256, np.int32), K=256),
                   dict(table=table_of(yuv(1), lib.CanvasC())), dict(table=table_of(yuv(2), yuv(1, y=16384)), idx=np.asarray([0, 1], np.int32))):
        rc, err = call(**change)
        assert accepted(rc, err), (list(change), rc, err)
    for change, text in REFUSED:
        rc, err = call(**change)
        assert rc == 7 and err.startswith(prefix) and text in err, (list(change), err)
    faults = [
        (bgr(y=None), "is null"), (bgr(height=0), "non-positive width or height"), (bgr(height=8193), "side above 8192"),
        (bgr(pitch_y=479), "pitch below three times its width"), (bgr(format=3), "unknown format"), (bgr(format=4), "unknown format"),
        (yuv(1, format=5), "unknown format"), (yuv(2, format=6), "unknown format"), (yuv(1, format=7), "unknown format"),
        (yuv(1, height=121), "odd width or height"), (yuv(1, pitch_y=158), "pitch_y below its width"), (yuv(1, pitch_c=158), "pitch_c below its width"),
        (yuv(2, pitch_c=79), "pitch_c below half its width"), (yuv(2, v=None), "null plane"),
    ]
    for entry, text in faults:
        first = yuv(1) if entry.format in (1, 2, 5, 6, 7) else bgr()
        rc, err = call(table=table_of(first, entry), idx=np.asarray([0, 1], np.int32))
        assert rc == 7 and "canvas 1, which person 1 is drawn on, " in err and text in err, (text, err)
        rc, err = call(table=table_of(first, entry))                      # ... while nobody referring to it is fine
        assert accepted(rc, err), (text, err)
    rc, err = call(table=table_of(bgr(), bgr(height=60)), idx=np.asarray([0, 1], np.int32))
    assert rc == 7 and "canvases 0 and 1 name the same buffer" in err and "must not overlap" in err, err
    rc, err = call(table=table_of(bgr(), yuv(1)), idx=np.asarray([0, 1], np.int32))
    assert rc == 7 and "mixes formats" in err and "all BGR or all YUV" in err, err


def pointer(v):
    return None if v is None else (v.ctypes.data if isinstance(v, np.ndarray) else v)


def test_device_entry_refusals_need_no_gpu():
    """a plan-only handle (device = -1): every argument error is reported as such, and a good call as 'plan-only'"""
    pkg, lib = load_pkg(), load_pkg("_lib")
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h
    bgr, yuv, table_of = canvas_entries(lib)
    good = dict(table=table_of(bgr(), lib.CanvasC()), nframes=2, pts=4096, n=2, J=17, joints=LIST, K=5, boxes=None, idx=np.zeros(2, np.int32),
                threshold=0.5, scale_num=1, scale_den=1, min_half=0, cell=8, status=None)

    def call(**change):
        a = dict(good, **change)
        rc = L.hrn_mosaic_dev(h, a["table"], a["nframes"], pointer(a["pts"]), a["n"], a["J"], pointer(a["joints"]), a["K"], pointer(a["boxes"]),
                              pointer(a["idx"]), a["threshold"], a["scale_num"], a["scale_den"], a["min_half"], a["cell"], pointer(a["status"]), None)
        return rc, L.hrn_last_error(h).decode()

    refusal_calls(lib, call, "hrn_mosaic_dev: ", lambda rc, err: rc == 7 and "plan-only" in err, 8192)
    with pytest.raises(ValueError, match="exactly one of them"):
        net.mosaic(np.zeros((20, 30, 3), np.uint8))
    net.close()


def test_host_entry_refusals():
    lib = load_pkg("_lib")
    post, L = load_pkg("postproc"), lib.load()
    bgr, yuv, table_of = canvas_entries(lib)
    # real memory behind the good call: the canvases refused below are never touched, the accepted ones are changed
    pixels = np.zeros(4096 + 192 * 120 * 3, np.uint8)
    base = pixels.ctypes.data

    def real(e):
        for name in ("y", "u", "v"):
            if getattr(e, name):
                setattr(e, name, base + getattr(e, name) - 4096)
        return e

    pts = mosaic_cases.all_people()[:2].copy()
    boxes = np.ascontiguousarray(BOXES[:2])
    status = np.zeros(2, np.int32)
    good = dict(table=table_of(real(bgr()), lib.CanvasC()), nframes=2, pts=pts, n=2, J=17, joints=LIST, K=5, boxes=None, idx=np.zeros(2, np.int32),
                threshold=0.5, scale_num=1, scale_den=1, min_half=0, cell=8, status=status)

    def call(**change):
        a = dict(good, **change)
        if isinstance(change.get("boxes"), int):           # (the refusal table's stand-in for "a pointer": the host entry gets real memory)
            a["boxes"] = boxes
        if "table" in change and change["table"] is not None:
            for e in a["table"]:
                real(e)
        rc = L.hrn_mosaic_host(a["table"], a["nframes"], pointer(a["pts"]), a["n"], a["J"], pointer(a["joints"]), a["K"], pointer(a["boxes"]),
                               pointer(a["idx"]), a["threshold"], a["scale_num"], a["scale_den"], a["min_half"], a["cell"], pointer(a["status"]))
        return rc, "hrn_mosaic_host: " + L.hrn_mosaic_last_error().decode()

    refusal_calls(lib, call, "hrn_mosaic_host: ", lambda rc, err: rc == 0 and err == "hrn_mosaic_host: ", boxes)
    assert call(status=None) == (0, "hrn_mosaic_host: ")
    # hrn_mosaic_regions: the shared checks, and its own
    hw = np.asarray([[37, 53], [37, 53]], np.int32)
    out, st = np.zeros((2, 4), np.int32), np.zeros(2, np.int32)
    r = lambda *a: (L.hrn_mosaic_regions(*[pointer(v) for v in a]), L.hrn_mosaic_last_error().decode())      # noqa: E731
    assert r(pts, 2, 17, LIST, 5, None, hw, 0.5, 1, 1, 0, out, st) == (0, "")
    assert r(None, 2, 17, LIST, 5, boxes, hw, 0.5, 1, 1, 0, out, st) == (0, "")
    assert r(pts, 2, 17, LIST, 5, boxes, hw, 0.5, 1, 1, 0, out, st) == (7, "people come from pts or from boxes, not from both")
    assert r(None, 2, 17, LIST, 5, None, hw, 0.5, 1, 1, 0, out, st) == (7, "null pts and boxes: people come from one of them")
    assert r(pts, 2, 17, LIST, 0, None, hw, 0.5, 1, 1, 0, out, st) == (7, "K must be in [1, 256]")
    assert r(pts, 2, 17, LIST, 5, None, hw, 0.5, 0, 1, 0, out, st) == (7, "scale_num and scale_den must be in [1, 64]")
    assert r(pts, 2, 17, LIST, 5, None, hw, 0.5, 1, 1, 4097, out, st) == (7, "min_half must be in [0, 4096]")
    assert r(pts, 2, 17, LIST, 5, None, None, 0.5, 1, 1, 0, out, st) == (7, "null canvas sizes / outputs")
    assert r(pts, 2, 17, LIST, 5, None, hw, 0.5, 1, 1, 0, None, st) == (7, "null canvas sizes / outputs")
    assert r(pts, 2, 17, LIST, 5, None, np.asarray([[37, 53], [0, 53]], np.int32), 0.5, 1, 1, 0, out, st) == (7, "the canvas size of person 1 is outside [1, 8192]")
    assert r(pts, 2, 17, LIST, 5, None, np.asarray([[37, 8193], [37, 53]], np.int32), 0.5, 1, 1, 0, out, st) == (7, "the canvas size of person 0 is outside [1, 8192]")
    assert r(None, 0, 0, None, 0, None, None, 0.5, 1, 1, 0, None, None) == (0, "")
    frame = np.zeros((20, 30, 3), np.uint8)
    for kw, text in ((dict(joints=[]), "1 to 256 indices"), (dict(joints=[17]), r"indices in \[0, 17\)"), (dict(joints=["nose"]), "no joint names"),
                     (dict(joints=list(range(17)) * 16), "1 to 256 indices"), (dict(scale=1.5), "pair of integers"), (dict(scale=(1.5, 1)), "pair of integers"),
                     (dict(scale=(0, 1)), "scale_num and scale_den must be in"), (dict(min_half=5000), "min_half must be in"), (dict(cell=3), "cell must be 0, 2, 4, 8, 16 or 32")):
        with pytest.raises(ValueError, match=text):
            post.mosaic(frame, pts=pts, **kw)
    with pytest.raises(ValueError, match="integers"):
        post.mosaic(frame, boxes=boxes.astype(np.float32))
    with pytest.raises(ValueError, match="with boxes there are none"):
        post.mosaic(frame, boxes=boxes, joints=HEAD)
    for kw in (dict(), dict(pts=pts, boxes=boxes)):
        with pytest.raises(ValueError, match="exactly one of them"):
            post.mosaic(frame, **kw)
    assert not frame.any()


def fnv(data):
    h = 1469598103934665603
    for v in np.asarray(data, np.uint8).reshape(-1).tolist():
        h = ((h ^ v) * 1099511628211) & (2 ** 64 - 1)
    return h


def walk_cases():
    """(fmt code, h, w, cell, pts or None, boxes or None, joints, threshold, scale, min_half): the designed people under every
    setting and cell on BGR, NV12 and I420, the boxes, the cell rule"""
    out = []
    pts = mosaic_cases.all_people()
    for k, (joints, threshold, scale, min_half) in enumerate(SETTINGS):
        for m, cell in enumerate(CELLS):
            fmt = (0, 1, 2)[(k + m) % 3]
            out.append((fmt,) + ((37, 53) if fmt == 0 else (38, 54)) + (cell, pts, None, joints, threshold, scale, min_half or 0))
    for fmt in (0, 1, 2):
        out.append((fmt,) + ((37, 53) if fmt == 0 else (38, 54)) + (8, None, BOXES, None, 0.5, (1, 1), 0))
    out.append((0, 1024, 1030, 0, pts, None, HEAD, 0.5, (1, 1), 0))
    out.append((2, 2048, 2050, 0, pts, None, HEAD, 0.5, (1, 1), 0))
    return out


def test_the_walk_under_sanitizers(tmp_path):
    """tests/mosaic_walk.cpp: the header alone, compiled for the host with AddressSanitizer and UBSan, over the cases above"""
    lib = load_pkg("_lib")
    cc, why = sanitizer_compiler(tmp_path)
    assert cc, "no host compiler links -fsanitize=address,undefined here: " + str(why)
    exe = tmp_path / "mosaic_walk"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mosaic_walk.cpp")
    subprocess.run(cc + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-sanitize-recover=all",
                         "-I", lib.CSRC, "-o", str(exe), src], check=True)
    cases = walk_cases()
    with open(tmp_path / "cases.txt", "w") as f:
        for fmt, h, w, cell, pts, boxes, joints, threshold, scale, min_half in cases:
            n = len(pts) if pts is not None else len(boxes)
            listed = list(range(mosaic_cases.J)) if joints is None else list(joints)
            head = [fmt, h, w, cell, n, 0 if pts is None else mosaic_cases.J, 0 if pts is None else len(listed), int(F32(threshold).view(np.uint32)),
                    scale[0], scale[1], min_half]
            body = (listed + np.ascontiguousarray(pts, F32).view(np.uint32).reshape(-1).tolist()) if pts is not None else \
                np.asarray(boxes).reshape(-1).tolist()
            f.write(" ".join(str(int(v)) for v in head + body) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    for (fmt, h, w, cell, pts, boxes, joints, threshold, scale, min_half), line in zip(cases, out):
        rects, status = mosaic_ref.regions((h, w), pts, boxes, joints, threshold, scale, min_half)
        s = mosaic_ref.cell_size(cell, h, w)
        m = mosaic_ref.marks(h, w, s, rects)
        nbytes = h * w * 3 if fmt == 0 else h * w * 3 // 2
        canvas = ((131 * np.arange(nbytes, dtype=np.int64) + 17) & 255).astype(np.uint8)
        if fmt == 0:
            mosaic_ref.mosaic_bgr(canvas.reshape(h, w, 3), rects, cell)
        else:
            mosaic_ref.mosaic_yuv(canvas, h, w, ("nv12", "i420")[fmt - 1], rects, cell)
        weights = (np.arange(nbytes, dtype=np.uint64) % np.uint64(65521)) + np.uint64(1)
        checksum = int((canvas.astype(np.uint64) * weights).sum(dtype=np.uint64))                  # (modulo 2^64, as the program's)
        want = (fnv(rects.astype("<i4").view(np.uint8)), fnv(status.astype("<i4").view(np.uint8)), s, int(m.sum()), checksum)
        assert tuple(int(v) for v in line.split()) == want, (fmt, h, w, cell, joints, scale, min_half, line)
