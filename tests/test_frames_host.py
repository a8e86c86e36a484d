"""Clip mode without a GPU: the host half of ``hrn_preprocess_frames`` (SimpleHRNet.py:236-278 and :383-412 over many frames).

``hrn_crop_geometry`` -- the box arithmetic both pre-path entries share -- against ``oracle.prepath_oracle`` (boxes AND the
slice / pad numbers, the latter derived from the oracle's own numpy slicing); every refusal with its code and text; the
declarations; the frame-grouping rule of ``predict_frames`` / ``predict_clip``."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import load_pkg
from oracle import prepath_oracle as P

FRAME_SIZES = [(333, 517), (480, 640), (720, 1280), (1080, 1920)]
RESOLUTIONS = [(384, 288), (256, 192), (64, 96)]
PER_CASE = 400   # x 4 frame sizes x 3 resolutions = 4800 random boxes per variant, plus the edge and tie cases


def make_boxes(rng, hf, wf, count):
    """boxes that are valid in both variants -- the generator of test_prepath.test_gpu_prepath_random_boxes_vs_oracle (any
    aspect, tiny to huge, fractional corners) plus boxes on each frame edge and half-integer corners (round-half-even)"""
    dets = []
    for _ in range(count):
        bw, bh = rng.integers(6, wf), rng.integers(6, hf)
        x1, y1 = rng.uniform(0, wf - bw), rng.uniform(0, hf - bh)
        dets.append([x1, y1, x1 + bw + rng.uniform(-0.49, 0.49), y1 + bh + rng.uniform(-0.49, 0.49)])
    for _ in range(count // 8):   # half-integer corners: ties go to the even neighbour
        bw, bh = int(rng.integers(6, wf - 2)), int(rng.integers(6, hf - 2))
        x1, y1 = int(rng.integers(0, wf - bw - 1)), int(rng.integers(0, hf - bh - 1))
        dets.append([x1 + 0.5, y1 + 0.5, x1 + bw + 0.5, y1 + bh + 0.5])
        dets.append([x1 + 0.5, y1, x1 + bw, y1 + bh + 0.5])
    bw, bh = wf // 3, hf // 3
    dets += [[0, 0, wf, hf], [0.5, 1.5, 2.5, 3.5],                                   # whole frame; ties in the rounding
             [0, hf // 4, bw, hf // 4 + bh], [wf - bw, hf // 4, wf, hf // 4 + bh],   # left edge, right edge
             [wf // 4, 0, wf // 4 + bw, bh], [wf // 4, hf - bh, wf // 4 + bw, hf],   # top edge, bottom edge
             [0, 0, 7, hf], [0, 0, wf, 7], [wf - 7, 0, wf, hf], [0, hf - 7, wf, hf],  # slivers along each edge: the other side grows
             [wf - 8.5, hf - 8.5, wf - 0.5, hf - 0.5]]
    dets = np.asarray(dets, np.float32)
    dets[:, 2] = np.minimum(dets[:, 2], wf)
    dets[:, 3] = np.minimum(dets[:, 3], hf)
    return np.ascontiguousarray(dets)


def oracle_geometry(dets, hf, wf, H, W, variant):
    """(boxes (n,4), slices (n,8)) from the oracle; the slice numbers are the shapes numpy's own slicing of a frame gives"""
    frame = np.zeros((hf, wf), np.uint8)
    boxes, slices = [], []
    for det in dets:
        if variant == "pad":
            (x1, y1, x2, y2), new, (pt, pb, pl, pr) = P.crop_box(det, H, W)
        else:
            x1, y1, x2, y2 = new = P.crop_box_clamped(det, H, W, hf, wf)
            pt = pb = pl = pr = 0
        assert 0 <= x1 and 0 <= y1, "the generator made a box numpy would wrap around"
        hc, wc = frame[y1:y2, x1:x2].shape
        boxes.append(new)
        slices.append((x1, y1, wc, hc, pt, pl, hc + pt + pb, wc + pl + pr))
    return np.asarray(boxes, np.int32), np.asarray(slices, np.int32)


def crop_geometry(L, dets, frame_hw, per_person, H, W, variant):
    dets = np.ascontiguousarray(dets, np.float32)
    hw = np.ascontiguousarray(frame_hw, np.int32)
    n = len(dets)
    boxes, slices = np.full((n, 4), -7, np.int32), np.full((n, 8), -7, np.int32)
    rc = L.hrn_crop_geometry(dets.ctypes.data, dets.shape[1], n, hw.ctypes.data, per_person, H, W, variant, boxes.ctypes.data,
                             slices.ctypes.data)
    return rc, boxes, slices, L.hrn_crop_geometry_last_error().decode()


@pytest.mark.parametrize("variant", ["pad", "clamp"])
def test_crop_geometry_equals_the_oracle(variant):
    L = load_pkg("_lib").load()
    total = 0
    for si, (hf, wf) in enumerate(FRAME_SIZES):
        for ri, (H, W) in enumerate(RESOLUTIONS):
            dets = make_boxes(np.random.default_rng(100 * si + ri), hf, wf, PER_CASE)
            want_boxes, want_slices = oracle_geometry(dets, hf, wf, H, W, variant)
            rc, boxes, slices, err = crop_geometry(L, dets, [[hf, wf]], 0, H, W, 0 if variant == "pad" else 1)
            assert rc == 0, err
            np.testing.assert_array_equal(boxes, want_boxes)
            np.testing.assert_array_equal(slices, want_slices)
            total += len(dets)
    assert total >= 4800


@pytest.mark.parametrize("variant", ["pad", "clamp"])
def test_crop_geometry_with_a_frame_size_per_person(variant):
    """people of frames of differing sizes in one call, a detector's 7 columns per row"""
    L = load_pkg("_lib").load()
    H, W = 256, 192
    rng = np.random.default_rng(5)
    parts = [(make_boxes(rng, hf, wf, 40), hf, wf) for hf, wf in FRAME_SIZES]
    dets = np.concatenate([np.concatenate([d, np.full((len(d), 3), 0.9, np.float32)], 1) for d, _, _ in parts])
    hw = np.concatenate([np.repeat([[hf, wf]], len(d), 0) for d, hf, wf in parts])
    order = rng.permutation(len(dets))           # people in any order
    want = [oracle_geometry(d, hf, wf, H, W, variant) for d, hf, wf in parts]
    rc, boxes, slices, err = crop_geometry(L, dets[order], hw[order], 1, H, W, 0 if variant == "pad" else 1)
    assert rc == 0, err
    np.testing.assert_array_equal(boxes, np.concatenate([w[0] for w in want])[order])
    np.testing.assert_array_equal(slices, np.concatenate([w[1] for w in want])[order])


def test_crop_geometry_errors():
    L = load_pkg("_lib").load()
    ok = [40.0, 30.0, 200.0, 330.0]
    cases = [
        (0, [[10, 10, 10, 100]], "detection 0 is degenerate"),
        (1, [[10, 10, 50, 10]], "detection 0 is degenerate"),
        (0, [ok, [-5, 10, 50, 100]], "detection 1 starts outside the frame"),
        (0, [[500, 10, 600, 100]], "detection 0 starts outside the frame"),
        (0, [[10, 400, 60, 500]], "detection 0 starts outside the frame"),
        (1, [ok, ok, [-3, 10, 200, 60]], "detection 2 starts outside the frame"),    # wide box: clamp re-derives y, x stays as given
        (1, [[-100, 10, -90, 200]], "detection 0 is degenerate after clamping"),      # tall box left of the frame: x clamps to nothing
        (1, [[10, -400, 300, -390]], "detection 0 is degenerate after clamping"),     # wide box above the frame
    ]
    for variant, dets, text in cases:
        rc, _, _, err = crop_geometry(L, np.asarray(dets, np.float32), [[360, 480]], 0, 384, 288, variant)
        assert rc == 7 and err == text, (variant, dets, rc, err)
    for variant in (2, -1):
        rc, _, _, err = crop_geometry(L, np.asarray([ok], np.float32), [[360, 480]], 0, 384, 288, variant)
        assert rc == 7 and err == "variant must be HRN_CROP_PAD or HRN_CROP_CLAMP"
    d = np.asarray([ok], np.float32)
    hw = np.asarray([[360, 480]], np.int32)
    assert L.hrn_crop_geometry(d.ctypes.data, 3, 1, hw.ctypes.data, 0, 384, 288, 0, None, None) == 7      # det_stride < 4
    assert L.hrn_crop_geometry_last_error() == b"bad frame / detections / n"
    assert L.hrn_crop_geometry(None, 4, 1, hw.ctypes.data, 0, 384, 288, 0, None, None) == 7
    assert L.hrn_crop_geometry(d.ctypes.data, 4, 1, None, 0, 384, 288, 0, None, None) == 7
    assert L.hrn_crop_geometry(d.ctypes.data, 4, -1, hw.ctypes.data, 0, 384, 288, 0, None, None) == 7
    assert L.hrn_crop_geometry(d.ctypes.data, 4, 1, hw.ctypes.data, 0, 0, 288, 0, None, None) == 7
    bad_hw = np.asarray([[0, 480]], np.int32)
    assert L.hrn_crop_geometry(d.ctypes.data, 4, 1, bad_hw.ctypes.data, 0, 384, 288, 0, None, None) == 7
    # a success clears the text; nobody and no outputs are fine
    assert L.hrn_crop_geometry(d.ctypes.data, 4, 1, hw.ctypes.data, 0, 384, 288, 0, None, None) == 0
    assert L.hrn_crop_geometry_last_error() == b""
    assert L.hrn_crop_geometry(None, 4, 0, None, 0, 384, 288, 1, None, None) == 0


def test_symbols_are_declared_and_exported():
    lib = load_pkg("_lib")
    names = {"hrn_preprocess_frames", "hrn_crop_geometry", "hrn_crop_geometry_last_error"}
    assert names <= set(lib.header_symbols()) and names <= set(lib.SYMBOLS)
    L = lib.load()
    for name in names:
        assert hasattr(L, name)
    assert L.hrn_preprocess_frames(None, None, 0, None, 4, None, 0, 0, None, None, None, None) == 1     # no handle
    text = open(os.path.join(lib.INCLUDE, "hrnet_mi355.h")).read()
    fields = re.search(r"typedef struct \{([^}]*)\} hrn_frame;", text).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [f[0] for f in lib.Frame._fields_] == ["data", "height", "width"]
    assert ctypes.sizeof(lib.Frame) == 16 and lib.Frame.height.offset == 8 and lib.Frame.width.offset == 12
    assert re.search(r"int hrn_preprocess_frames\(hrn_handle h, const hrn_frame \*frames_host, int nframes,", text)


def test_preprocess_frames_refusals_need_no_gpu():
    """a plan-only handle (device = -1): every argument error is reported as such, and a good call as 'plan-only'"""
    pkg = load_pkg()
    lib = load_pkg("_lib")
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h
    table = (lib.Frame * 2)()
    table[0].data, table[0].height, table[0].width = 4096, 120, 160     # never read: nothing is launched on this handle
    dets = np.asarray([[10, 8, 90, 100], [20, 20, 60, 90]], np.float32)
    idx = np.zeros(2, np.int32)
    out = 4096                                                           # "device" outputs, never written

    def call(table, nframes, idx, n=2, variant=0, stride=4, d=dets):
        rc = L.hrn_preprocess_frames(h, table, nframes, None if d is None else d.ctypes.data, stride,
                                     None if idx is None else idx.ctypes.data, n, variant, out, None, None, None)
        return rc, L.hrn_last_error(h).decode()

    rc, err = call(table, 2, idx)
    assert rc == 7 and "plan-only" in err
    rc, err = call(table, 1, None)                                       # NULL index: one frame
    assert rc == 7 and "plan-only" in err
    rc, err = call(table, 2, idx, n=0)                                   # (as hrn_preprocess_frame: the handle is judged before n == 0)
    assert rc == 7 and "plan-only" in err
    for bad, f, person in (([0, 2], 2, 1), ([-1, 0], -1, 0), ([0, 1 << 30], 1 << 30, 1)):
        rc, err = call(table, 2, np.asarray(bad, np.int32))
        assert rc == 7 and "frame_index %d of person %d is outside [0, 2)" % (f, person) in err, err
    rc, err = call(table, 2, np.asarray([0, 1], np.int32))               # frame 1 is null and person 1 refers to it
    assert rc == 7 and "frame 1, which person 1 is cut from, is null or has no size" in err
    rc, err = call(table, 2, np.asarray([0, 0], np.int32))               # ... while nobody referring to it is fine
    assert rc == 7 and "plan-only" in err
    table[1].data, table[1].height, table[1].width = 4096, 0, 160        # a non-positive side
    rc, err = call(table, 2, np.asarray([1, 0], np.int32))
    assert rc == 7 and "frame 1, which person 0 is cut from" in err
    rc, err = call(None, 2, idx)                                         # a null table
    assert rc == 7 and "bad frames / detections / n" in err
    rc, err = call(table, 2, None)                                       # NULL index with more than one frame
    assert rc == 7 and "without frame_index there must be one frame" in err
    rc, err = call(table, 0, idx)
    assert rc == 7 and "bad frames / detections / n" in err
    rc, err = call(table, 2, idx, d=None)
    assert rc == 7 and "bad frames / detections / n" in err
    rc, err = call(table, 2, idx, n=-1)
    assert rc == 7 and "bad frames / detections / n" in err
    rc, err = call(table, 2, idx, stride=3)
    assert rc == 7 and "bad frames / detections / n" in err
    rc, err = call(table, 2, idx, variant=2)
    assert rc == 7 and "variant must be HRN_CROP_PAD or HRN_CROP_CLAMP" in err
    # the single-frame entry on the same handle: its own checks, its own texts
    rc = L.hrn_preprocess_frame(h, 4096, 120, 160, dets.ctypes.data, 4, 2, 0, out, None, None, None)
    assert rc == 7 and b"plan-only" in L.hrn_last_error(h)
    net.close()


def test_group_frames():
    native = load_pkg("native")
    G = lambda counts, limit, per_pass=None: list(native.group_frames(counts, limit, per_pass))   # noqa: E731
    # greedy packing by people: a frame is never split to fill a group
    assert G([3, 3, 3, 3], 8) == [[(0, 0, 3), (1, 0, 3)], [(2, 0, 3), (3, 0, 3)]]
    assert G([8, 8], 8) == [[(0, 0, 8)], [(1, 0, 8)]]
    assert G([1, 2, 5, 1, 7, 1], 8) == [[(0, 0, 1), (1, 0, 2), (2, 0, 5)], [(3, 0, 1), (4, 0, 7)], [(5, 0, 1)]]
    # people_per_pass below max_batch
    assert G([2, 2, 2, 2, 2], 32, 4) == [[(0, 0, 2), (1, 0, 2)], [(2, 0, 2), (3, 0, 2)], [(4, 0, 2)]]
    # an empty frame inside a group, at the start and at the end: it joins the group being formed
    assert G([0, 3, 0, 4, 0], 8) == [[(0, 0, 0), (1, 0, 3), (2, 0, 0), (3, 0, 4), (4, 0, 0)]]
    assert G([4, 0, 4, 1], 8) == [[(0, 0, 4), (1, 0, 0), (2, 0, 4)], [(3, 0, 1)]]
    assert G([0, 0], 8) == [[(0, 0, 0), (1, 0, 0)]] and G([], 8) == []
    # a frame above max_batch: alone, in as many groups as it needs; its neighbours do not share them
    assert G([9], 4) == [[(0, 0, 4)], [(0, 4, 8)], [(0, 8, 9)]]
    assert G([2, 9, 1, 1], 4) == [[(0, 0, 2)], [(1, 0, 4)], [(1, 4, 8)], [(1, 8, 9)], [(2, 0, 1), (3, 0, 1)]]
    assert G([5], 8, 2) == [[(0, 0, 2)], [(0, 2, 4)], [(0, 4, 5)]]
    # every person exactly once, in order, whatever the counts
    rng = np.random.default_rng(0)
    for _ in range(200):
        counts = rng.integers(0, 12, rng.integers(0, 20)).tolist()
        limit = int(rng.integers(1, 10))
        groups = G(counts, limit)
        assert all(sum(hi - lo for _, lo, hi in g) <= limit for g in groups)
        flat = [(f, i) for g in groups for f, lo, hi in g for i in range(lo, hi)]
        assert flat == [(f, i) for f, c in enumerate(counts) for i in range(c)]
        assert sorted({f for g in groups for f, _, _ in g}) == list(range(len(counts)))
        assert [f for g in groups for f, _, _ in g] == sorted(f for g in groups for f, _, _ in g)
    # it reads lazily: one frame beyond the group it yields
    seen = []

    def counts():
        for k, c in enumerate([3, 3, 3, 3, 3]):
            seen.append(k)
            yield c

    it = native.group_frames(counts(), 8)
    assert next(it) == [(0, 0, 3), (1, 0, 3)] and seen == [0, 1, 2]
    # refusals
    with pytest.raises(ValueError, match="people_per_pass=16 exceeds max_batch=8"):
        G([1], 8, 16)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="people_per_pass"):
            G([1], 8, bad)
    with pytest.raises(ValueError, match="negative"):
        G([1, -1], 8)
