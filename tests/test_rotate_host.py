"""Frame rotation without a GPU: ``hrn_rotate_people`` against the numpy restatement (tests/rotate_ref.py) bit for bit, boxes
against pixels, the way back, every refusal of ``hrn_rotate_frames`` / ``hrn_rotate_people(_dev)`` on a plan-only handle, the
declarations, ``rotation_code_from_degrees``."""
import os

import numpy as np
import pytest

from conftest import load_pkg
from rotate_ref import rotate_boxes, rotate_joints, rotate_plane, rotated_hw

NEW = {"hrn_rotate_frames", "hrn_rotate_people", "hrn_rotate_people_last_error", "hrn_rotate_people_dev"}


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    assert len(bad) == 0, "%s: %d words differ, first at %d: %r != %r" % (what, len(bad), bad[0], got.reshape(-1)[bad[0]],
                                                                          want.reshape(-1)[bad[0]])


def random_people(n, J, seed, hw=(480, 640)):
    """joints in and around the frame with NaN, inf and -0.0 among them; boxes inside the frame with all-zero rows among them"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-20, max(hw) + 20, (n, J, 3)).astype(np.float32)
    pts[..., 2] = rng.uniform(0, 1, (n, J)).astype(np.float32)
    flat = pts.reshape(-1, 3)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0, 1e30, 16777217.0)):
        if len(flat) > 2 * k + 1:
            flat[2 * k, 0] = v
            flat[2 * k + 1, 1] = v
    if len(flat) > 20:
        flat[20, 2] = np.nan
    a = np.stack([rng.integers(0, hw[1], (n, 2)), rng.integers(0, hw[0], (n, 2))], 2)   # (n, 2 picks, (x, y))
    boxes = np.concatenate([a.min(1), a.max(1) + 1], 1).astype(np.int32)
    boxes[::5] = 0
    return pts, boxes


def test_symbols_and_sources():
    lib = load_pkg("_lib")
    assert NEW <= set(lib.header_symbols()) and NEW <= set(lib.SYMBOLS)
    assert set(lib.header_symbols()) == set(lib.SYMBOLS)
    assert "rotate.hip" in lib.SOURCES
    for f in ("rotate.hip", "rotate_math.h"):
        assert os.path.exists(os.path.join(lib.CSRC, f)), f
    for f in ("rotate.hip", "postproc.cpp", "hrnet_mi355.cpp"):   # one text for the host and the device
        assert '#include "rotate_math.h"' in open(os.path.join(lib.CSRC, f)).read(), f
    header = open(os.path.join(lib.INCLUDE, "hrnet_mi355.h")).read()
    assert "HRN_ROTATE_90_CW = 0, HRN_ROTATE_180 = 1, HRN_ROTATE_90_CCW = 2" in header
    pkg = load_pkg()
    for name in ("rotate_people", "rotation_code_from_degrees"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert hasattr(pkg.NativeHRNet, "rotate_frames") and hasattr(pkg.NativeHRNet, "rotate_people")


@pytest.mark.parametrize("J", [17, 133])
def test_people_equal_the_restatement_bit_for_bit(J):
    P = load_pkg("postproc")
    n = 60
    pts, boxes = random_people(n, J, seed=J)
    rng = np.random.default_rng(1)
    sizes = np.stack([rng.integers(1, 2000, n), rng.integers(1, 2000, n)], 1).astype(np.int32)
    codes = rng.integers(0, 3, n).astype(np.int32)
    for hw, code in (((480, 640), 0), ((480, 640), 1), ((480, 640), 2), ((1, 1), 0), (sizes, 2), ((1080, 1920), codes), (sizes, codes)):
        got_p, got_b = P.rotate_people(pts, boxes, hw, code)
        same_bits(got_p, rotate_joints(pts, hw, code), "joints")
        np.testing.assert_array_equal(got_b, rotate_boxes(boxes, hw, code))
        assert not got_b[::5].any()                                   # the lost person's box stays all-zero
        same_bits(P.rotate_people(pts=pts, frame_hw=hw, rotation_code=code), got_p, "joints alone")
        np.testing.assert_array_equal(P.rotate_people(boxes=boxes, frame_hw=hw, rotation_code=code), got_b)
        same_bits(got_p[..., 2], pts[..., 2], "confidences are copied")
    assert np.isnan(P.rotate_people(pts, None, (480, 640), 1)[0, 0, 0]) and P.rotate_people(pts, None, (480, 640), 0)[0, 2, 1] == -np.inf
    empty = P.rotate_people(np.zeros((0, J, 3), np.float32), np.zeros((0, 4), np.int32), (4, 4), 1)
    assert empty[0].shape == (0, J, 3) and empty[1].shape == (0, 4)


@pytest.mark.parametrize("hw", [(37, 53), (64, 48), (1, 9)])
def test_boxes_and_pixels_agree(hw):
    """on a frame of unique values, rot90 of the slice a box cuts is the rotated frame sliced by the rotated box"""
    P = load_pkg("postproc")
    h, w = hw
    frame = np.arange(h * w, dtype=np.int64).reshape(h, w)
    rng = np.random.default_rng(h)
    xs, ys = np.sort(rng.integers(0, w + 1, (40, 2)), 1), np.sort(rng.integers(0, h + 1, (40, 2)), 1)
    keep = (xs[:, 0] < xs[:, 1]) & (ys[:, 0] < ys[:, 1])
    boxes = np.stack([xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1]], 1)[keep].astype(np.int32)
    boxes = np.concatenate([boxes, [[0, 0, w, h], [w - 1, h - 1, w, h], [0, 0, 1, 1]]]).astype(np.int32)
    for code in (0, 1, 2):
        turned = rotate_plane(frame, code)
        assert turned.shape == rotated_hw(h, w, code)
        for (x1, y1, x2, y2), (rx1, ry1, rx2, ry2) in zip(boxes, P.rotate_people(boxes=boxes, frame_hw=hw, rotation_code=code)):
            assert 0 <= rx1 < rx2 <= turned.shape[1] and 0 <= ry1 < ry2 <= turned.shape[0]
            np.testing.assert_array_equal(rotate_plane(frame[y1:y2, x1:x2], code), turned[ry1:ry2, rx1:rx2])
        # and joints: the pixel under an integer-valued joint is the pixel under the rotated joint
        yy, xx = rng.integers(0, h, 50), rng.integers(0, w, 50)
        pts = np.stack([yy, xx, np.ones(50)], 1).astype(np.float32)[None]
        out = P.rotate_people(pts=pts, frame_hw=hw, rotation_code=code)[0]
        np.testing.assert_array_equal(turned[out[:, 0].astype(int), out[:, 1].astype(int)], frame[yy, xx])


def test_the_way_back_is_code_two_minus_c():
    P = load_pkg("postproc")
    rng = np.random.default_rng(4)
    n = 50
    sizes = np.stack([rng.integers(1, 3000, n), rng.integers(1, 3000, n)], 1).astype(np.int32)
    pts = rng.integers(-4000, 4000, (n, 17, 3)).astype(np.float32)
    _, boxes = random_people(n, 17, seed=9)
    codes = rng.integers(0, 3, n).astype(np.int32)
    for hw, code in (((480, 640), 0), ((480, 640), 1), ((481, 641), 2), (sizes, codes)):
        hw_arr = np.broadcast_to(np.asarray(hw, np.int32).reshape(-1, 2), (n, 2))
        c_arr = np.broadcast_to(np.asarray(code, np.int32).reshape(-1), (n,))
        turned_hw = np.where((c_arr == 1)[:, None], hw_arr, hw_arr[:, ::-1]).astype(np.int32)
        there = P.rotate_people(pts, boxes, hw_arr, c_arr)
        back = P.rotate_people(there[0], there[1], turned_hw, 2 - c_arr)
        same_bits(back[0], pts, "joints there and back")
        np.testing.assert_array_equal(back[1], boxes)


def canvas(lib, fmt=0, h=120, w=160, y=4096, pitch=None, **change):
    e = lib.CanvasC()
    e.format, e.height, e.width = fmt, h, w
    if fmt == 0:
        e.y, e.pitch_y = y, 3 * w if pitch is None else pitch
    else:
        pitch = w if pitch is None else pitch
        e.y, e.u, e.pitch_y = y, y + pitch * h, pitch
        e.pitch_c = pitch if fmt == 1 else pitch // 2
        if fmt == 2:
            e.v = e.u + (pitch // 2) * (h // 2)
    for k, v in change.items():
        setattr(e, k, v)
    return e


def table_of(lib, *entries):
    t = (lib.CanvasC * len(entries))()
    for k, e in enumerate(entries):
        t[k] = e
    return t


def test_rotate_frames_refusals_need_no_gpu():
    """a plan-only handle (device = -1): every argument error is reported as such, before 'plan-only'; a good call as 'plan-only'"""
    pkg, lib = load_pkg(), load_pkg("_lib")
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h

    def call(src, dst, codes, n=None):
        codes = None if codes is None else np.asarray(codes, np.int32)
        rc = L.hrn_rotate_frames(h, None if src is None else table_of(lib, *src), None if dst is None else table_of(lib, *dst),
                                 len(src) if n is None else n, None if codes is None else codes.ctypes.data, None)
        return rc, L.hrn_last_error(h).decode()

    C = lambda *a, **k: canvas(lib, *a, **k)   # noqa: E731
    far = 1 << 24
    good = [
        ([C()], [C(h=160, w=120, y=far)], [0]), ([C()], [C(y=far)], [1]), ([C()], [C(h=160, w=120, y=far, pitch=487)], [2]),
        ([C(1)], [C(1, 160, 120, far)], [0]), ([C(2)], [C(2, 160, 120, far, pitch=126)], [2]), ([C(2, pitch=166)], [C(2, y=far)], [1]),
        ([C(), C(1, y=8192)], [C(y=far), C(1, 160, 120, 2 * far)], [1, 2]),                  # formats and codes may differ by frame
        ([C(h=1, w=1)], [C(h=1, w=1, y=far)], [0]),
        ([C(h=715827882, w=1, pitch=3)], [C(h=1, w=715827882, y=far)], [0]),                 # pitch * rows = 2^31 - 2
    ]
    for src, dst, codes in good:
        rc, err = call(src, dst, codes)
        assert rc == 7 and "plan-only" in err, err
    rc, err = call([], [], [], n=0)
    assert rc == 7 and "plan-only" in err, err
    assert L.hrn_rotate_frames(h, None, None, 0, None, None) == 7 and "plan-only" in L.hrn_last_error(h).decode()
    refused = [
        (([C()], [C(y=far)], [1], -1), "nframes is negative"),
        ((None, [C(y=far)], [1], 1), "null frame tables / codes"), (([C()], None, [1], 1), "null frame tables"), (([C()], [C(y=far)], None), "null frame tables"),
        (([C()], [C(y=far)], [3]), "frame 0: code 3 is outside {0, 1, 2}"), (([C()], [C(y=far)], [-1]), "code -1 is outside"),
        (([C()], [C(1, y=far)], [1]), "frame 0: source and destination differ in format"),
        (([C(3)], [C(3, y=far)], [1]), "the source has an unknown format"), (([C(-1)], [C(-1, y=far)], [1]), "unknown format"),
        (([C(y=None)], [C(y=far)], [1]), "the source has a null plane"), (([C()], [C(y=None)], [1]), "the destination has a null plane"),
        (([C(1, u=None)], [C(1, y=far)], [1]), "the source has a null plane"), (([C(2)], [C(2, y=far, v=None)], [1]), "the destination has a null plane"),
        (([C(h=0)], [C(h=0, y=far)], [1]), "the source has a non-positive width or height"), (([C(w=-4)], [C(w=-4, y=far)], [1]), "non-positive"),
        (([C(1, h=121)], [C(1, h=121, y=far)], [1]), "the source has an odd width or height"), (([C(2, w=161)], [C(2, w=161, y=far)], [1]), "odd width"),
        (([C()], [C(y=far)], [0]), "frame 0: the destination is 120 x 160, the rotated size is 160 x 120"),
        (([C()], [C(h=160, w=120, y=far)], [1]), "the destination is 160 x 120, the rotated size is 120 x 160"),
        (([C()], [C(h=160, w=121, y=far)], [2]), "the rotated size is 160 x 120"),
        (([C(pitch=479)], [C(y=far)], [1]), "the source has pitch_y below its row's bytes"), (([C()], [C(y=far, pitch=479)], [1]), "the destination has pitch_y below"),
        (([C(1, pitch=158)], [C(1, y=far)], [1]), "pitch_y below"), (([C(1, pitch_c=158)], [C(1, y=far)], [1]), "the source has pitch_c below"),
        (([C(2)], [C(2, y=far, pitch_c=79)], [1]), "the destination has pitch_c below"),
        (([C(h=715827883, w=1, pitch=3)], [C(h=1, w=715827883, y=far)], [0]), "the source has a plane with pitch * rows >= 2^31"),
        (([C(h=2, w=2)], [C(h=2, w=2, y=far, pitch=1 << 30)], [1]), "the destination has a plane with pitch * rows >= 2^31"),
        (([C()], [C()], [1]), "the source of frame 0 is the destination of frame 0: in-place rotation is not offered"),
        (([C(), C(y=far)], [C(y=far), C(y=2 * far)], [1, 1]), "the source of frame 1 is the destination of frame 0"),
        (([C(), C(y=8192)], [C(y=far), C(y=far)], [1, 1]), "frames 0 and 1 name the same destination"),
        (([C(), C()], [C(y=far), C(y=2 * far)], [1, 3]), "frame 1: code 3"),
    ]
    for args, text in refused:
        rc, err = call(*args)
        assert rc == 7 and err.startswith("hrn_rotate_frames: ") and text in err and "plan-only" not in err, (text, err)
    net.close()


def test_rotate_people_refusals_need_no_gpu():
    pkg = load_pkg()
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h
    pts, boxes = np.zeros((3, 17, 3), np.float32), np.zeros((3, 4), np.int32)
    hw1, hw3 = np.asarray([[480, 640]], np.int32), np.asarray([[480, 640], [4, 4], [9, 1]], np.int32)

    def both(n=3, J=17, hw=hw1, per_hw=0, codes=(1,), per_code=0, p=pts, b=boxes, po=pts, bo=boxes):
        codes = None if codes is None else np.asarray(codes, np.int32)
        a = (n, J, None if hw is None else hw.ctypes.data, per_hw, None if codes is None else codes.ctypes.data, per_code)
        d = tuple(None if x is None else x.ctypes.data for x in (p, b, po, bo))   # never touched by the device form: nothing is launched
        host = L.hrn_rotate_people(*a, *(d if n <= 3 else (None, None, None, None)))
        dev = L.hrn_rotate_people_dev(h, *a, *d, None)
        return host, L.hrn_rotate_people_last_error().decode(), dev, L.hrn_last_error(h).decode()

    for kw in (dict(), dict(hw=hw3, per_hw=1), dict(codes=(0, 1, 2), per_code=1), dict(p=None, po=None), dict(b=None, bo=None), dict(n=0),
               dict(n=0, hw=None, codes=None), dict(J=256, b=None, bo=None, n=0), dict(J=1, n=1)):
        host, _, dev, err = both(**kw)
        assert host == 0 and dev == 7 and "plan-only" in err, (kw, err)
    for kw, text in ((dict(n=-1), "n is negative"), (dict(J=0), "J must be in [1, HRN_MAX_JOINTS]"), (dict(J=257), "HRN_MAX_JOINTS"),
                     (dict(p=None, b=None), "pts and boxes are both null"), (dict(po=None), "an input without its output"),
                     (dict(bo=None), "an input without its output"), (dict(hw=None), "null frame sizes / codes"), (dict(codes=None), "null frame sizes"),
                     (dict(codes=(3,)), "a rotation code is outside {0, 1, 2}"), (dict(codes=(0, 1, -1), per_code=1), "a rotation code"),
                     (dict(hw=np.asarray([[0, 5]], np.int32)), "a frame has a non-positive side"),
                     (dict(hw=np.asarray([[4, 4], [4, 4], [4, -1]], np.int32), per_hw=1), "non-positive side")):
        host, herr, dev, err = both(**kw)
        assert host == 7 and text in herr, (kw, herr)
        assert dev == 7 and err.startswith("hrn_rotate_people_dev: ") and text in err and "plan-only" not in err, (kw, err)
    # what only everybody's entry of a per-person array would refuse is not looked at
    assert both(codes=(1, 7, 7))[0] == 0 and both(hw=np.asarray([[4, 4], [0, 0], [0, 0]], np.int32))[0] == 0
    net.close()
    # the Python forms refuse what they can tell themselves
    P = load_pkg("postproc")
    for kw in (dict(), dict(pts=pts), dict(pts=pts, frame_hw=(4, 4)), dict(pts=pts, frame_hw=(4, 4), rotation_code=3),
               dict(pts=pts, frame_hw=(4, 4), rotation_code=[0, 1]), dict(pts=pts, boxes=boxes[:2], frame_hw=(4, 4), rotation_code=0),
               dict(pts=pts[0], frame_hw=(4, 4), rotation_code=0), dict(boxes=boxes[:, :3], frame_hw=(4, 4), rotation_code=0),
               dict(pts=pts, frame_hw=(4, 4, 4), rotation_code=0), dict(pts=pts, frame_hw=(4, 0), rotation_code=0),
               dict(pts=pts, frame_hw=(4, 4), rotation_code=1.5)):
        with pytest.raises(ValueError):
            P.rotate_people(**kw)


def test_rotation_code_from_degrees():
    pkg = load_pkg()
    f = pkg.rotation_code_from_degrees
    assert (f(90), f(180), f(270)) == (0, 1, 2) and f(None) is None and f(0) is None
    assert f(90.0) == 0 and f(np.int64(270)) == 2
    for bad in (45, -90, 360, 91, 90.5, "90", True):
        with pytest.raises(ValueError):
            f(bad)
