"""The tracking link without a GPU: ``hrn_pose_boxes`` (boxes from joints, the host form) against its numpy float64 restatement,
bit for bit; every refusal of the new entries on a plan-only handle; the declarations; and that the crop geometry the record
kernel compiles is the text ``hrn_crop_geometry`` runs (tests/test_frames_host.py pins its bits)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import load_pkg
from pose_boxes_ref import FRAME, constructed_cases, pose_boxes_ref, random_poses

NEW = {"hrn_pose_boxes", "hrn_pose_boxes_last_error", "hrn_boxes_from_poses", "hrn_preprocess_frames_dev",
       "hrn_preprocess_frames_yuv_dev"}


def same_bits(got, want, what=""):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, "%s: rows %s differ, first %s != %s" % (what, bad[:5], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("J", [17, 133])
def test_pose_boxes_equals_the_restatement_on_random_poses(J):
    P = load_pkg("postproc")
    total = 0
    for seed, kw in enumerate([{}, {"threshold": 0.3, "min_joints": 5, "scale": 1.0, "min_side": 12.0},
                               {"threshold": -3e38, "min_joints": 1, "scale": 1.7, "min_side": 0.5}]):
        pts = random_poses(1200, J, 10 * J + seed)
        got = P.pose_boxes(pts, FRAME, **kw)
        same_bits(got, pose_boxes_ref(pts, FRAME, **kw), "seed %d" % seed)
        dead = ~got.any(axis=1)
        if not kw:
            assert 0 < dead.sum() < len(pts)                                  # both kinds of rows occur
        total += len(pts)
    assert total >= 3000
    # a frame size per person, people in one call
    rng = np.random.default_rng(J)
    hw = rng.integers(40, 400, (500, 2)).astype(np.int32)
    pts = random_poses(500, J, 99)
    same_bits(P.pose_boxes(pts, hw), pose_boxes_ref(pts, hw), "per-person frames")


@pytest.mark.parametrize("J", [17, 133])
def test_pose_boxes_on_the_constructed_rows(J):
    P = load_pkg("postproc")
    for name, pts, hw, kw in constructed_cases(J):
        same_bits(P.pose_boxes(pts, hw, **kw), pose_boxes_ref(pts, hw, **kw), name)


def test_the_constructed_rows_are_what_their_names_say():
    """the restatement's answers on the rows whose answer can be written down"""
    got = {name: pose_boxes_ref(pts, hw, **kw) for name, pts, hw, kw in constructed_cases(17)}
    rows = got["exactly min_joints live, and one fewer"]
    # x in [20, 70.25], y in [10, 40]: centre (45.125, 25), sides 62.8125 and 37.5
    np.testing.assert_array_equal(rows[0], np.asarray([13.71875, 6.25, 76.53125, 43.75, 0.9], np.float32))
    assert not rows[1].any()
    rows = got["four live of min_joints 4, and three"]
    assert rows[0].any() and not rows[1].any()
    rows = got["a confidence equal to the threshold is not live"]
    np.testing.assert_array_equal(rows[0], got["exactly min_joints live, and one fewer"][0])     # the fourth joint does not count
    assert not rows[1].any()
    np.testing.assert_array_equal(got["a NaN confidence is not live"][0], rows[0])
    rows = got["NaN or inf coordinates on otherwise live joints"]
    np.testing.assert_array_equal(rows[0], got["exactly min_joints live, and one fewer"][0])
    assert not rows[1].any()
    np.testing.assert_array_equal(got["all joints at one point, min_side 0"][0], np.asarray([44, 33, 44, 33, 0.9], np.float32))
    rows = got["all joints at one point, min_side 24.5"]
    np.testing.assert_array_equal(rows[0], np.asarray([31.75, 20.75, 56.25, 45.25, 0.9], np.float32))
    np.testing.assert_array_equal(rows[1], np.asarray([145.75, 0, 160, 14.25, 0.9], np.float32))   # cut to the frame
    rows = got["joints left of, above and beyond the frame"]
    assert rows[0][2] < rows[0][0] == 0 and rows[1][3] < rows[1][1] == 0           # x2 < x1 = 0, y2 < y1 = 0: degenerate downstream
    assert rows[2][0] > rows[2][2] == 160 and rows[2][1] > rows[2][3] == 120       # beyond: x1 > x2 = frame_w
    assert rows[3][2] == 160 and rows[3][3] == 120 and rows[3][0] < 160            # straddling the edge: cut
    rows = got["negative coordinates and zeros of both signs"]
    assert (rows.view(np.uint32)[1, :4] == 0).all()                                  # zeros of either sign give +0
    assert not np.signbit(rows[:, :4]).any()
    np.testing.assert_array_equal(got["scale 1.0"][1], np.asarray([0, 0, 159, 119, 0.9], np.float32))
    row = got["a negative threshold takes every finite joint"][0]
    assert row[0] == 13.71875 and row[4] < -1e29              # the dead joints at (50, 50) count too: same extent, their confidences
    rows = got["a frame size per person"]
    assert rows[0][2] == 134.375 and rows[1][2] == 60 and rows[2][2] == 131 and rows[1][3] == 50


def test_pose_boxes_argument_errors():
    lib = load_pkg("_lib")
    L = lib.load()
    pts = np.zeros((2, 17, 3), np.float32)
    hw = np.asarray([[120, 160]], np.int32)
    out = np.zeros((2, 5), np.float32)
    F, D = ctypes.c_float, ctypes.c_double

    def call(p=pts.ctypes.data, n=2, J=17, f=hw.ctypes.data, per=0, mj=3, scale=1.25, side=0.0, o=out.ctypes.data):
        rc = L.hrn_pose_boxes(p, n, J, f, per, F(0.5), mj, D(scale), D(side), o)
        return rc, L.hrn_pose_boxes_last_error().decode()

    assert call() == (0, "")
    assert call(n=-1) == (7, "n is negative")
    for J in (0, 257, -3):
        assert call(J=J) == (7, "J must be in [1, 256]")
    assert call(J=256, n=0) == (0, "")
    assert call(mj=0) == (7, "min_joints must be at least 1")
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert call(scale=scale) == (7, "scale must be finite and positive")
    for side in (-0.5, float("nan"), float("inf")):
        assert call(side=side) == (7, "min_side must be finite and not negative")
    for kw in ({"p": None}, {"f": None}, {"o": None}):
        assert call(**kw) == (7, "null joints / frame sizes / output")
    assert call(p=None, f=None, o=None, n=0) == (0, "")                      # nobody: nothing is read
    bad = np.asarray([[120, 160], [0, 160]], np.int32)
    assert call(f=bad.ctypes.data) == (0, "")                                # one size for everybody: row 0 only
    assert call(f=bad.ctypes.data, per=1) == (7, "the frame of person 1 has a non-positive side")
    bad[0, 1] = -4
    assert call(f=bad.ctypes.data) == (7, "the frame of person 0 has a non-positive side")
    P = load_pkg("postproc")
    with pytest.raises(ValueError, match="scale must be finite and positive"):
        P.pose_boxes(pts, (120, 160), scale=0)
    with pytest.raises(ValueError, match="frame_hw"):
        P.pose_boxes(pts, [[1, 2], [3, 4], [5, 6]])
    with pytest.raises(ValueError, match="pts must be"):
        P.pose_boxes(np.zeros((2, 17, 2), np.float32), (120, 160))
    assert P.pose_boxes(np.zeros((0, 17, 3), np.float32), (120, 160)).shape == (0, 5)


def test_symbols_are_declared_and_exported():
    lib = load_pkg("_lib")
    assert NEW <= set(lib.header_symbols()) and NEW <= set(lib.SYMBOLS)
    L = lib.load()
    for name in NEW:
        assert hasattr(L, name)
    assert "track.hip" in lib.SOURCES
    text = open(os.path.join(lib.INCLUDE, "hrnet_mi355.h")).read()
    assert re.search(r"int hrn_preprocess_frames_dev\(hrn_handle h, const hrn_frame \*frames_host, int nframes, const float \*dets_dev,", text)
    assert re.search(r"int hrn_boxes_from_poses\(hrn_handle h, const float \*pts_dev, int n, int J, const int32_t \*frame_hw_host", text)
    # no handle
    assert L.hrn_boxes_from_poses(None, None, 0, 17, None, 0, ctypes.c_float(0), 3, ctypes.c_double(1), ctypes.c_double(0), None, None) == 1
    assert L.hrn_preprocess_frames_dev(None, None, 0, None, 4, None, 0, 0, None, None, None, None) == 1
    assert L.hrn_preprocess_frames_yuv_dev(None, None, 0, None, 4, None, 0, 0, None, None, None, None) == 1
    pkg = load_pkg()
    for name in ("boxes_from_poses", "preprocess_frames_dev", "track_frame"):
        assert callable(getattr(pkg.NativeHRNet, name))
    assert callable(pkg.postproc.pose_boxes)


def test_boxes_from_poses_refusals_need_no_gpu():
    pkg = load_pkg()
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h
    hw = np.asarray([[120, 160], [97, 131]], np.int32)
    F, D = ctypes.c_float, ctypes.c_double
    dev = 4096   # "device" pointers, never read: nothing is launched on this handle

    def call(p=dev, n=2, J=17, f=hw.ctypes.data, per=1, mj=3, scale=1.25, side=0.0, o=dev):
        rc = L.hrn_boxes_from_poses(h, p, n, J, f, per, F(0.5), mj, D(scale), D(side), o, None)
        return rc, L.hrn_last_error(h).decode()

    for kw in ({}, {"per": 0}, {"n": 0}, {"J": 133}, {"J": 256}, {"n": 0, "p": None, "f": None, "o": None}):
        rc, err = call(**kw)
        assert rc == 7 and "plan-only" in err, (kw, err)
    for kw, text in (({"n": -1}, "n is negative"), ({"J": 0}, "J must be in [1, 256]"), ({"J": 257}, "J must be in [1, 256]"),
                     ({"mj": 0}, "min_joints must be at least 1"), ({"scale": 0.0}, "scale must be finite and positive"),
                     ({"scale": float("nan")}, "scale must be finite and positive"),
                     ({"scale": float("inf")}, "scale must be finite and positive"),
                     ({"side": -1.0}, "min_side must be finite and not negative"),
                     ({"side": float("inf")}, "min_side must be finite and not negative"),
                     ({"p": None}, "null joints / frame sizes / output"), ({"f": None}, "null joints / frame sizes / output"),
                     ({"o": None}, "null joints / frame sizes / output")):
        rc, err = call(**kw)
        assert rc == 7 and err == "hrn_boxes_from_poses: " + text, (kw, err)
    bad = np.asarray([[120, 160], [97, 0]], np.int32)
    rc, err = call(f=bad.ctypes.data)
    assert rc == 7 and err == "hrn_boxes_from_poses: the frame of person 1 has a non-positive side"
    rc, err = call(f=bad.ctypes.data, per=0)                                  # only row 0 counts
    assert rc == 7 and "plan-only" in err
    net.close()


@pytest.mark.parametrize("yuv", [False, True])
def test_preprocess_frames_dev_refusals_need_no_gpu(yuv):
    """a plan-only handle: every argument error of the host-detection entries (minus the per-detection ones) with its text, and
    a good call as 'plan-only'"""
    pkg = load_pkg()
    lib = load_pkg("_lib")
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h
    name = "hrn_preprocess_frames_yuv_dev" if yuv else "hrn_preprocess_frames_dev"
    entry = getattr(L, name)
    if yuv:
        table = (lib.YuvFrameC * 2)()
        table[0].y, table[0].u, table[0].height, table[0].width, table[0].pitch_y, table[0].pitch_c = 4096, 8192, 120, 160, 160, 160
        table[0].format = 1
    else:
        table = (lib.Frame * 2)()
        table[0].data, table[0].height, table[0].width = 4096, 120, 160
    idx = np.zeros(2, np.int32)
    dev = 4096

    def call(table=table, nframes=2, idx=idx, n=2, variant=0, stride=5, d=dev, images=dev, boxes=dev, status=dev):
        rc = entry(h, table, nframes, d, stride, None if idx is None else idx.ctypes.data, n, variant, images, boxes, status, None)
        return rc, L.hrn_last_error(h).decode()

    for kw in ({}, {"nframes": 1, "idx": None}, {"n": 0}, {"stride": 4}, {"variant": 1}):
        rc, err = call(**kw)
        assert rc == 7 and "plan-only" in err, (kw, err)
    for bad, f, person in (([0, 2], 2, 1), ([-1, 0], -1, 0), ([0, 1 << 30], 1 << 30, 1)):
        rc, err = call(idx=np.asarray(bad, np.int32))
        assert rc == 7 and "%s: frame_index %d of person %d is outside [0, 2)" % (name, f, person) in err, err
    rc, err = call(idx=np.asarray([0, 1], np.int32))                          # frame 1 is null and person 1 refers to it
    assert rc == 7 and "%s: frame 1, which person 1 is cut from, " % name in err
    assert ("has an unknown format" if yuv else "is null or has no size") in err
    if yuv:
        table[1].y, table[1].u, table[1].height, table[1].width, table[1].pitch_y, table[1].pitch_c = 4096, 8192, 121, 160, 160, 160
        table[1].format = 1
        rc, err = call(idx=np.asarray([1, 0], np.int32))
        assert rc == 7 and "frame 1, which person 0 is cut from, has an odd or non-positive width or height" in err
    else:
        table[1].data, table[1].height, table[1].width = 4096, 0, 160
        rc, err = call(idx=np.asarray([1, 0], np.int32))
        assert rc == 7 and "frame 1, which person 0 is cut from, is null or has no size" in err
    rc, err = call(nframes=2, idx=None)
    assert rc == 7 and "%s: without frame_index there must be one frame" % name in err
    for kw in ({"table": None}, {"nframes": 0}, {"d": None}, {"n": -1}, {"stride": 3}, {"images": None}, {"boxes": None},
               {"status": None}):
        rc, err = call(**kw)
        assert rc == 7 and err == "bad frames / detections / n", (kw, err)
    for variant in (2, -1):
        rc, err = call(variant=variant)
        assert rc == 7 and err == "variant must be HRN_CROP_PAD or HRN_CROP_CLAMP"
    net.close()


def test_simple_hrnet_redetect_every_is_checked_without_a_gpu():
    S = load_pkg().SimpleHRNet
    for bad in (0, -2, 2.5):
        with pytest.raises(ValueError, match="redetect_every"):
            S(32, 17, {}, detector=object(), redetect_every=bad)


def test_the_record_kernel_compiles_the_text_hrn_crop_geometry_runs():
    """one function text for the host and the device: the host runtime has no copy of the box arithmetic of its own"""
    lib = load_pkg("_lib")
    shared = open(os.path.join(lib.CSRC, "track_geometry.h")).read()
    host = open(os.path.join(lib.CSRC, "hrnet_mi355.cpp")).read()
    kernels = open(os.path.join(lib.CSRC, "track.hip")).read()
    assert len(re.findall(r"__host__ __device__ inline int crop_geometry_one\(", shared)) == 1
    assert "fp contract(off)" in shared and "rint(" in shared
    for text in (host, kernels):
        assert '#include "track_geometry.h"' in text
        assert "nearbyint((double)d[" not in text and "center - length / 2" not in text      # the arithmetic lives in the header only
    assert "hrn::crop_geometry_one(d, frame_h, frame_w, H, W, variant, cp, box, pad_hw)" in host
    assert "crop_geometry_one(d, f.height, f.width, a.H, a.W, a.variant, cp, box, pad_hw)" in kernels
    assert "pose_box_finish(" in kernels and "pose_box_finish(" in shared and "pose_box_one(" in host
    assert os.path.join(lib.CSRC, "track_geometry.h") in lib._deps("track.hip")


class _FakeTracker:
    """stands in for NativeHRNet on a box without a GPU: joints carry (person id, call number), and track_frame reports the people
    whose id is in `lose` as not followed (status 2) -- what is tested is the schedule and the assembly of SimpleHRNet.predict"""
    lose = ()

    def __init__(self, c, nof_joints, resolution, dtype, max_batch, device, model_name):
        self.j, self.res, self.calls, self.tracked = nof_joints, resolution, 0, []

    def load_state_dict(self, sd):
        return self

    def _pts(self, ids):
        import torch
        pts = torch.zeros((len(ids), self.j, 3))
        pts[:, :, 0] = torch.as_tensor(ids, dtype=torch.float32)[:, None]
        pts[:, :, 1] = float(self.calls)
        return pts

    def predict_frame(self, frame, dets, return_heatmaps=False, variant="pad"):
        import torch
        self.calls += 1
        boxes = np.rint(np.asarray(dets, np.float32)[:, :4]).astype(np.int32)
        pts = self._pts(list(range(len(dets))))
        hm = torch.zeros((len(dets), self.j, self.res[0] // 4, self.res[1] // 4))
        return (boxes, pts, hm) if return_heatmaps else (boxes, pts)

    def track_frame(self, frame, prev_pts, return_heatmaps=False, **box_args):
        import torch
        self.calls += 1
        self.tracked.append(dict(box_args))
        ids = prev_pts[:, 0, 0].to(torch.int64).tolist()
        status = torch.tensor([2 if i in self.lose else 0 for i in ids], dtype=torch.int32)
        boxes = torch.tensor([[i, i, i + 10, i + 20] for i in ids], dtype=torch.int32).reshape(-1, 4)
        boxes[status != 0] = 0
        hm = torch.zeros((len(ids), self.j, self.res[0] // 4, self.res[1] // 4))
        out = (boxes, self._pts(ids), status)
        return out + (hm,) if return_heatmaps else out


def test_simple_hrnet_redetect_schedule_without_a_gpu(monkeypatch):
    """redetect_every = 3 on a fake engine: the detector on calls 0, 3, 6 and after a call that returned nobody; people who are
    not followed are dropped; redetect_every = 1 never reaches the tracking code"""
    from importlib import import_module
    from test_simple_hrnet import TableDetector
    mod = import_module("simple-hrnet_amd.simple_hrnet")
    monkeypatch.setattr(mod, "NativeHRNet", _FakeTracker)
    asked, now = [], [0]

    class Detector(TableDetector):
        def predict_single(self, image, color_mode="BGR"):
            asked.append(now[0])                                 # the number of the predict() call that asks
            return super().predict_single(image, color_mode)

    frame = np.zeros((60, 80, 3), np.uint8)
    dets = np.asarray([[1, 2, 30, 50], [5, 5, 20, 40], [7, 9, 60, 55]], np.float32)
    m = mod.SimpleHRNet(32, 17, {}, resolution=(64, 48), multiperson=True, return_heatmaps=True, return_bounding_boxes=True,
                        detector=Detector({0: dets}), redetect_every=3, track_args={"threshold": 0.2})

    def predict(call):
        now[0] = call
        return m.predict(frame)

    seen = []
    for call in range(7):
        if call == 4:
            m.model.lose = (1,)                                  # person 1 cannot be followed from here on
        hm, boxes, pts = predict(call)
        assert boxes.dtype == np.int32 and pts.dtype == np.float32 and len(hm) == len(boxes) == len(pts)
        seen.append(pts[:, 0, 0].tolist())
    assert asked == [0, 3, 6]
    assert seen == [[0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 2], [0, 2], [0, 1, 2]]
    assert m.model.tracked == [{"threshold": 0.2}] * 4
    np.testing.assert_array_equal(predict(7)[1], [[0, 0, 10, 20], [2, 2, 12, 22]])     # tracked, person 1 dropped again
    # nobody left: the nobody result of the reference, and the detector on the next call whatever its number
    m.model.lose = (0, 1, 2)
    hm, boxes, pts = predict(8)
    assert pts.shape == (0, 0, 3) and boxes.shape == (0, 4) and hm.shape == (0, 17, 16, 12) and asked == [0, 3, 6]
    m.model.lose = ()
    assert len(predict(9)[2]) == 3 and asked == [0, 3, 6, 9]     # (a detector call anyway)
    m.model.lose = (0, 1, 2)
    assert predict(10)[2].shape == (0, 0, 3) and asked == [0, 3, 6, 9]
    m.model.lose = ()
    assert len(predict(11)[2]) == 3 and asked == [0, 3, 6, 9, 11]          # not a multiple of 3: asked because nobody was left
    m.detector = Detector({0: None})
    for call in (12, 13, 14):                                    # the detector finds nobody: it is asked again on every call
        assert predict(call)[2].shape == (0, 0, 3)
    assert asked == [0, 3, 6, 9, 11, 12, 13, 14]
    # the default: every call asks the detector, track_frame is never reached
    plain = mod.SimpleHRNet(32, 17, {}, resolution=(64, 48), multiperson=True, detector=TableDetector({0: dets}))
    for _ in range(4):
        assert plain.predict(frame).shape == (3, 17, 3)
    assert plain.model.tracked == [] and plain.model.calls == 4 and plain.redetect_every == 1
