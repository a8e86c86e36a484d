"""The detector link without a GPU: ``hrn_letterbox_geometry`` against the restated wrappers on every frame size below 300,
``hrn_detections_to_frame`` against the torch CPU restatement of the two inverses bit for bit, the refusals, the declarations."""
import os

import numpy as np
import pytest
import torch

from conftest import load_pkg
from letterbox_ref import detections_ref, geometry_ref, geometry_scalar, random_rows

NEW = {"hrn_letterbox_geometry", "hrn_letterbox_last_error", "hrn_letterbox_frames", "hrn_letterbox_frames_yuv",
       "hrn_detections_to_frame", "hrn_detections_to_frame_dev"}


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).any(axis=1))
    assert len(bad) == 0, "%s: rows %s differ, first %s != %s" % (what, bad[:5], got[bad[0]], want[bad[0]])


def test_symbols_and_sources():
    lib = load_pkg("_lib")
    assert NEW <= set(lib.header_symbols()) and NEW <= set(lib.SYMBOLS)
    assert set(lib.header_symbols()) == set(lib.SYMBOLS)
    assert "letterbox.hip" in lib.SOURCES
    for f in ("letterbox.hip", "letterbox_math.h", "resize_taps.h", "yuv_px.h"):
        assert os.path.exists(os.path.join(lib.CSRC, f)), f
    # one text: both resizing kernels compile resize_taps.h, and the tap arithmetic is typed nowhere else
    for f in ("prepath.hip", "letterbox.hip"):
        text = open(os.path.join(lib.CSRC, f)).read()
        assert '#include "resize_taps.h"' in text and "interpolateCubic" not in text.split("namespace hrn", 1)[1], f
    for f in ("letterbox.hip", "postproc.cpp", "hrnet_mi355.cpp"):
        assert '#include "letterbox_math.h"' in open(os.path.join(lib.CSRC, f)).read(), f


@pytest.mark.parametrize("size,style", [(64, "yolov3"), ((64, 96), "yolov5"), (64, "yolov5"), (416, "yolov3"), (640, "yolov5")])
def test_geometry_equals_the_restatement_on_every_frame_size_below_300(size, style):
    P = load_pkg("postproc")
    h, w = (a.reshape(-1) for a in np.meshgrid(np.arange(1, 300), np.arange(1, 300), indexing="ij"))
    new_w, new_h, top, bottom, left, right, ratio, dw, dh = geometry_ref(h, w, size, style)
    ok = (new_w >= 1) & (new_h >= 1)
    assert ok.sum() > 80000 or np.ndim(size) == 0 and size == 64
    out_h, out_w = (size, size) if np.ndim(size) == 0 else size
    assert ((top + new_h + bottom == out_h) & (left + new_w + right == out_w))[ok].all()     # the issue's observation
    g = P.letterbox_geometry(np.stack([h[ok], w[ok]], 1), size, style)
    for name, want in (("new_w", new_w), ("new_h", new_h), ("top", top), ("left", left), ("bottom", bottom), ("right", right)):
        np.testing.assert_array_equal(getattr(g, name), want[ok], name)
    for name, want in (("ratio", ratio), ("dw", dw), ("dh", dh)):
        np.testing.assert_array_equal(getattr(g, name).view(np.uint64), want[ok].view(np.uint64), name)
    # frames that resize to nothing are refused one by one (a sample of them: each is a call)
    for i in np.flatnonzero(~ok)[:40]:
        with pytest.raises(ValueError, match="resized to nothing"):
            P.letterbox_geometry((h[i], w[i]), size, style)
    # the vectorised restatement is the wrappers' plain Python on a sample
    for i in np.random.default_rng(0).integers(0, len(h), 300):
        want = geometry_scalar(int(h[i]), int(w[i]), size, style)
        got = (new_w[i], new_h[i], top[i], bottom[i], left[i], right[i], ratio[i], dw[i], dh[i])
        assert tuple(float(x) for x in got) == tuple(float(x) for x in want)


@pytest.mark.parametrize("hw,size,style,new_wh,pads,dw", [
    ((48, 64), 64, "yolov3", (64, 48), (8, 8, 0, 0), None),
    ((37, 53), 64, "yolov3", (64, 45), (9, 10, 0, 0), None),
    ((1080, 1920), 416, "yolov3", (416, 234), (91, 91, 0, 0), None),
    ((48, 64), (64, 96), "yolov5", (85, 64), (0, 0, 5, 6), 5.5),
])
def test_geometry_rows_written_down(hw, size, style, new_wh, pads, dw):
    g = load_pkg("postproc").letterbox_geometry(hw, size, style)
    assert (int(g.new_w[0]), int(g.new_h[0])) == new_wh
    assert (int(g.top[0]), int(g.bottom[0]), int(g.left[0]), int(g.right[0])) == pads
    if dw is not None:
        assert g.dw[0] == dw


def test_geometry_errors():
    P, lib = load_pkg("postproc"), load_pkg("_lib").load()
    with pytest.raises(ValueError, match="resized to nothing"):
        P.letterbox_geometry((1, 200), 64, "yolov3")
    hw = np.asarray([[1, 200]], np.int32)
    out = (load_pkg("_lib").Letterbox * 1)()
    import ctypes
    assert lib.hrn_letterbox_geometry(0, hw.ctypes.data, 1, 64, 64, ctypes.addressof(out)) == 7
    assert b"frame 0 (1 x 200)" in lib.hrn_letterbox_last_error()
    assert lib.hrn_letterbox_geometry(0, hw.ctypes.data, 1, 64, 96, ctypes.addressof(out)) == 7      # MAX_SIDE is square
    assert lib.hrn_letterbox_geometry(2, hw.ctypes.data, 1, 64, 64, ctypes.addressof(out)) == 7      # unknown rule
    assert lib.hrn_letterbox_geometry(0, None, 1, 64, 64, ctypes.addressof(out)) == 7
    hw[0] = (0, 5)
    assert lib.hrn_letterbox_geometry(1, hw.ctypes.data, 1, 64, 64, ctypes.addressof(out)) == 7
    with pytest.raises(ValueError):
        P.letterbox_geometry((48, 64), (64, 96), "yolov3")
    with pytest.raises(ValueError):
        P.letterbox_geometry((48, 64), 64, "yolov4")


FRAMES = [(480, 640), (37, 53), (1080, 1920), (720, 1280), (300, 200)]


@pytest.mark.parametrize("style,size", [("yolov3", 416), ("yolov5", 640), ("yolov5", (384, 640))])
def test_inverse_equals_the_torch_restatement_on_random_rows(style, size):
    P = load_pkg("postproc")
    counts = [700, 0, 600, 300, 400]
    d = random_rows(sum(counts), 7, size, seed=11)
    g = P.letterbox_geometry(FRAMES, size, style)
    thres = float(d[5, 4])                                       # a confidence EXACTLY at the threshold: kept (>=)
    for kw in ({}, {"conf_thres": thres}, {"conf_thres": thres, "classes": [0, 2]}, {"classes": [1], "class_col": 6},
               {"conf_thres": 0.3, "classes": [2], "class_col": -1, "compact": False}):
        got = P.detections_to_frame(d, g, counts=counts, **kw)
        want = detections_ref(d, FRAMES, size, style, counts, **kw)
        same_bits(got[0], want[0], str(kw))
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])
        if "conf_thres" in kw and kw["conf_thres"] == thres:
            assert got[2][5] in (0, 2) and (d[:, 4] < np.float32(thres)).sum() == (got[2] == 1).sum()
    assert got[1][1] == 0 and sum(counts) == 2000


def test_inverse_statuses_order_and_carried_columns():
    P = load_pkg("postproc")
    g = P.letterbox_geometry([(480, 640)], 416, "yolov3")
    d = random_rows(12, 8, 416, seed=3)
    d[:, 4] = 0.9
    d[:, -1] = 0
    d[1, 0], d[2, 3], d[3, 4] = np.nan, np.inf, np.nan            # 5: a coordinate or the confidence is not finite
    d[4, 4] = 0.1                                                 # 1
    d[5, -1] = 7                                                  # 2
    d[6, 4], d[6, -1] = 0.1, 7                                    # below the threshold comes before the class
    d[7, 1], d[7, -1] = -np.inf, 7                                # not finite comes before both
    rows, counts, status = P.detections_to_frame(d, g, conf_thres=0.5, classes=[0])
    np.testing.assert_array_equal(status, [0, 5, 5, 5, 1, 2, 1, 5, 0, 0, 0, 0])
    assert counts.tolist() == [5]
    kept = [0, 8, 9, 10, 11]
    np.testing.assert_array_equal(rows[:5, 4:], d[kept][:, 4:])   # in their order, other columns untouched
    assert not rows[5:].any()
    loose = P.detections_to_frame(d, g, conf_thres=0.5, classes=[0], compact=False)
    np.testing.assert_array_equal(loose[0][kept], rows[:5])
    assert not np.delete(loose[0], kept, axis=0).any() and loose[1].tolist() == [5]
    # no filter at all: only the rows that are not finite go
    assert P.detections_to_frame(d, g)[1].tolist() == [8]
    # nobody, and no frames
    empty = P.detections_to_frame(np.zeros((0, 6), np.float32), g)
    assert empty[0].shape == (0, 6) and empty[1].tolist() == [0]


def test_inverse_errors():
    P = load_pkg("postproc")
    g = P.letterbox_geometry([(480, 640), (48, 64)], 416, "yolov3")
    d = random_rows(10, 6, 416, seed=1)
    for kw, text in (({"counts": None}, "need counts"), ({"counts": [4, 5]}, "sum to"), ({"counts": [10]}, "entries for"),
                     ({"counts": [4, 6], "conf_col": 6}, "conf_col"), ({"counts": [4, 6], "conf_col": 3}, "conf_col"),
                     ({"counts": [4, 6], "classes": [0], "class_col": -7}, "class_col"),
                     ({"counts": [4, 6], "classes": list(range(17))}, "16"), ({"counts": [4, 6], "conf_thres": float("nan")}, "NaN")):
        with pytest.raises(ValueError, match=text):
            P.detections_to_frame(d, g, **kw)
    with pytest.raises(ValueError, match=">=5"):
        P.detections_to_frame(d[:, :4], g, counts=[4, 6])
    # aliasing the input is an argument error
    import ctypes
    lib = load_pkg("_lib").load()
    start, st, cnt = np.asarray([0, 4, 10], np.int32), np.zeros(10, np.int32), np.zeros(2, np.int32)
    args = lambda out: (0, d.ctypes.data, 6, start.ctypes.data, 2, ctypes.addressof(g.table), g.frame_hw.ctypes.data, 416, 416, 4,  # noqa: E731
                        ctypes.c_float(0.5), 6, None, 0, 1, out, cnt.ctypes.data, st.ctypes.data)
    assert lib.hrn_detections_to_frame(*args(d.ctypes.data)) == 7 and b"overlaps" in lib.hrn_letterbox_last_error()
    assert lib.hrn_detections_to_frame(*args(d.ctypes.data + 24)) == 7
    assert lib.hrn_detections_to_frame(*args(np.empty_like(d).ctypes.data)) == 0


@pytest.mark.parametrize("style,size", [("yolov3", 416), ("yolov5", (384, 640))])
def test_round_trip_within_a_pixel(style, size):
    """a box in frame coordinates, forward by the geometry the tensor was made with, back by the inverse: within 1 pixel"""
    P = load_pkg("postproc")
    rng = np.random.default_rng(5)
    frames = [(480, 640), (37, 53), (1080, 1920), (333, 111)]
    g = P.letterbox_geometry(frames, size, style)
    counts, rows, boxes = [], [], []
    for k, (h, w) in enumerate(frames):
        a, b = rng.uniform(0, 1, (2, 50, 2)) * (w, h)
        box = np.concatenate([np.minimum(a, b), np.maximum(a, b)], 1)
        # where the resize puts frame pixel x: x * new_w / w + left (pixel centres: (x + 0.5) * s - 0.5, within the pixel asked for)
        sx, sy = g.new_w[k] / w, g.new_h[k] / h
        fwd = box * (sx, sy, sx, sy) + (g.left[k], g.top[k], g.left[k], g.top[k])
        rows.append(np.concatenate([fwd, np.ones((50, 1))], 1).astype(np.float32))
        boxes.append(box)
        counts.append(50)
    back, kept, status = P.detections_to_frame(np.concatenate(rows), g, counts=counts)
    assert kept.tolist() == counts and not status.any()
    err = np.abs(back[:, :4] - np.concatenate(boxes))
    assert err.max() <= 1.0, err.max()
