"""The tracking link on the GPU: boxes from joints, the crop pre-path from detections on the device, and the chain
pts(k) -> boxes -> crops(k+1) -> pass -> pts(k+1) against the host composition it replaces.  Every comparison is bit equality.

W32, 17 joints, crops (64, 64) and (64, 96); frames of (120, 160), (97, 131) and (150, 90) noise.  A 4:2:0 frame has even sides, so
the YUV cases take (98, 132) for the second frame."""
import numpy as np
import pytest
import torch

import yuv_ref
from conftest import load_pkg, state_dict_np
from pose_boxes_ref import FRAME, constructed_cases, pose_boxes_ref, random_poses
from test_frames_host import make_boxes
from test_simple_hrnet import TableDetector

pytestmark = pytest.mark.gpu

RESOLUTIONS = [(64, 64), (64, 96)]
SIZES = [(120, 160), (97, 131), (150, 90)]
YUV_SIZES = [(120, 160), (98, 132), (150, 90)]
_NETS = {}


def engine(res=(64, 96), dtype="fp32"):
    """one engine per (resolution, dtype) for the whole module, weights loaded"""
    key = (tuple(res), dtype)
    if key not in _NETS:
        _NETS[key] = load_pkg().NativeHRNet(32, 17, key[0], dtype, max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    return _NETS[key]


def noise_frame(hf, wf, seed):
    return np.random.default_rng(seed).integers(0, 256, (hf, wf, 3), dtype=np.uint8)


def black_crop(H, W):
    """Normalize(0) in float32: what the all-padding crop of a refused person holds"""
    mean, std = np.asarray([0.485, 0.456, 0.406], np.float32), np.asarray([0.229, 0.224, 0.225], np.float32)
    value = (np.float32(0.0) / np.float32(255.0) - mean) / std
    return np.broadcast_to(value.astype(np.float32)[:, None, None], (3, H, W))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ boxes from joints
@pytest.mark.parametrize("J", [17, 133])
def test_boxes_from_poses_equals_the_host_form(J):
    pkg = load_pkg()
    net = engine()
    for name, pts, hw, kw in constructed_cases(J):
        got = net.boxes_from_poses(torch.from_numpy(pts).cuda(), hw, **kw)
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(pts), 5) and got.is_cuda
        want = pkg.postproc.pose_boxes(pts, hw, **kw)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), name
        assert np.array_equal(bits(want), bits(pose_boxes_ref(pts, hw, **kw))), name
    rng = np.random.default_rng(J)
    for n in (1, 5, 70):
        pts = random_poses(n, J, 7 * J + n)
        for kw in ({}, {"threshold": 0.3, "min_joints": 5, "scale": 1.0, "min_side": 12.0}, {"threshold": -3e38, "min_joints": 1}):
            for hw in (FRAME, rng.integers(40, 400, (n, 2)).astype(np.int32)):
                got = net.boxes_from_poses(pts, hw, **kw).cpu().numpy()      # (a host array is uploaded)
                assert np.array_equal(bits(got), bits(pkg.postproc.pose_boxes(pts, hw, **kw))), (n, kw)
    assert tuple(net.boxes_from_poses(np.zeros((0, J, 3), np.float32), FRAME).shape) == (0, 5)
    with pytest.raises(RuntimeError, match="min_joints must be at least 1"):
        net.boxes_from_poses(pts, FRAME, min_joints=0)


# ----------------------------------------------------------------------------------------- the pre-path from device detections
def make_frames(pkg, kind, pitched_first=False):
    """three frames of three sizes: (what the engine takes, ...)"""
    if kind == "bgr":
        return [noise_frame(hf, wf, 10 + k) for k, (hf, wf) in enumerate(SIZES)], SIZES
    out = []
    for k, (hf, wf) in enumerate(YUV_SIZES):
        pitch = wf + 32 if (k == 0 and pitched_first) else None
        fmt = kind if k != 1 else ("i420" if kind == "nv12" else "nv12")     # the formats mixed in one call
        data = np.random.default_rng(30 + k).integers(0, 256, yuv_ref.nbytes(hf, wf, pitch), dtype=np.uint8)
        out.append(pkg.YuvFrame(data, hf, wf, fmt, "bt601", "limited", pitch))
    return out, YUV_SIZES


def people_of(sizes, seed):
    """make_boxes' mix for every frame, the people of all frames in shuffled order: (dets (n, 4), frame_index (n,))"""
    rng = np.random.default_rng(seed)
    dets = [make_boxes(rng, hf, wf, 8) for hf, wf in sizes]
    index = np.repeat(np.arange(len(sizes), dtype=np.int32), [len(d) for d in dets])
    order = rng.permutation(len(index))
    return np.ascontiguousarray(np.concatenate(dets)[order]), np.ascontiguousarray(index[order])


def host_path(net, frames, dets, index, variant):
    """hrn_preprocess_frames(_yuv) with the same detections on the host: (images, boxes on the device)"""
    dev = net._device_frames(frames)
    images, _, boxes_dev = net._preprocess_table(net._frame_table(dev), len(dev), dets, index, variant)
    return images, boxes_dev


@pytest.mark.parametrize("kind", ["bgr", "nv12", "i420"])
@pytest.mark.parametrize("variant", ["pad", "clamp"])
def test_preprocess_frames_dev_equals_the_host_detection_path(variant, kind):
    pkg = load_pkg()
    frames, sizes = make_frames(pkg, kind, pitched_first=(kind == "nv12"))
    for res in RESOLUTIONS:
        net = engine(res)
        # one frame (the pitched one, for NV12), no frame_index
        dets = make_boxes(np.random.default_rng(3), sizes[0][0], sizes[0][1], 8)
        want_images, _, want_boxes = net.preprocess_frame(frames[0], dets, variant)
        images, boxes, status = net.preprocess_frames_dev(frames[0], torch.from_numpy(dets).cuda(), variant=variant)
        assert status.dtype == torch.int32 and boxes.dtype == torch.int32 and not status.any()
        assert torch.equal(boxes, want_boxes) and torch.equal(images, want_images)
        # three frames of three sizes, people in shuffled order, a detector's 5 columns per row
        dets, index = people_of(sizes, 4)
        want_images, want_boxes = host_path(net, frames, dets, index, variant)
        rows = np.concatenate([dets, np.full((len(dets), 1), 0.9, np.float32)], 1)
        images, boxes, status = net.preprocess_frames_dev(frames, torch.from_numpy(rows).cuda(), index, variant)
        assert len(dets) > 60 and not status.any()
        assert torch.equal(boxes, want_boxes) and torch.equal(images, want_images)


# the refused kinds, and what each variant makes of them (frames are at least 97 x 90):
#   [10, 10, 10, 50]     x2 == x1                                                      degenerate in both
#   [-3, 10, 140, 40]    a wide box (cf > 1): x is sliced as given and starts left of the frame in both
#   [-100, 10, -90, 80]  a tall box left of the frame: PAD slices x as given (outside); CLAMP re-derives x and clamps it to nothing
#   [10, 10, 1e6, 60]    PAD pads the height to H / W times a million columns: taller than any scratch (4); CLAMP clamps the height
#                        to the frame and slices to its right edge: a valid crop, as in the host path
#   NaN, inf, 2e9        not a coordinate (5), judged before anything else
REFUSED = [([10, 10, 10, 50], 1, 1), ([-3, 10, 140, 40], 2, 2), ([-100, 10, -90, 80], 2, 3), ([10, 10, 1e6, 60], 4, 0),
           ([float("nan"), 10, 50, 60], 5, 5), ([10, 10, float("inf"), 60], 5, 5), ([10, -2e9, 50, 60], 5, 5)]


@pytest.mark.parametrize("kind", ["bgr", "nv12"])
@pytest.mark.parametrize("variant", ["pad", "clamp"])
def test_refused_people_get_a_status_and_a_black_crop_and_leave_their_neighbours_alone(variant, kind):
    pkg = load_pkg()
    frames, sizes = make_frames(pkg, kind)
    for res in RESOLUTIONS:
        net = engine(res)
        dets, index = people_of(sizes, 5)
        clean_images, clean_boxes, clean_status = net.preprocess_frames_dev(frames, torch.from_numpy(dets).cuda(), index, variant)
        assert not clean_status.any()
        # one row of each kind spliced in, on every frame in turn
        at = [3 + 5 * k for k in range(len(REFUSED))]
        all_dets, all_index, want_status, origin = list(dets), list(index), [0] * len(dets), list(range(len(dets)))
        for k, (pos, (row, st_pad, st_clamp)) in enumerate(zip(at, REFUSED)):
            all_dets.insert(pos, np.asarray(row, np.float32))
            all_index.insert(pos, k % 3)
            want_status.insert(pos, st_pad if variant == "pad" else st_clamp)
            origin.insert(pos, -1)
        all_dets, all_index = np.asarray(all_dets, np.float32), np.asarray(all_index, np.int32)
        want_status, origin = np.asarray(want_status, np.int32), np.asarray(origin)
        images, boxes, status = net.preprocess_frames_dev(frames, torch.from_numpy(all_dets).cuda(), all_index, variant)
        images, boxes = images.cpu().numpy(), boxes.cpu().numpy()
        np.testing.assert_array_equal(status.cpu().numpy(), want_status)
        dead = want_status != 0
        assert dead.sum() == (7 if variant == "pad" else 6)
        assert not boxes[dead].any()
        black = black_crop(*res)
        for i in np.flatnonzero(dead):
            assert np.array_equal(bits(images[i]), bits(black)), i
        kept = origin >= 0
        assert np.array_equal(bits(images[kept]), bits(clean_images.cpu().numpy()[origin[kept]]))
        np.testing.assert_array_equal(boxes[kept], clean_boxes.cpu().numpy()[origin[kept]])
        if variant == "clamp":        # the spliced row CLAMP accepts: the host path's crop of it
            i = int(np.flatnonzero((origin < 0) & ~dead)[0])
            want_images, want_boxes = host_path(net, frames, all_dets[i:i + 1], all_index[i:i + 1], variant)
            assert np.array_equal(bits(images[i]), bits(want_images.cpu().numpy()[0]))
            np.testing.assert_array_equal(boxes[i], want_boxes.cpu().numpy()[0])
        # a five-zero row of boxes_from_poses is a degenerate detection
        _, zb, zs = net.preprocess_frames_dev(frames[0], torch.zeros((2, 5), device="cuda"), variant=variant)
        assert zs.tolist() == [1, 1] and not zb.any()


# ------------------------------------------------------------------------------------------------------------------ the chain
def host_accepts(L, dets, hw, res, variant=0):
    """per detection: 0 where hrn_crop_geometry accepts it, else the status of its refusal"""
    texts = {"is degenerate": 1, "starts outside the frame": 2, "is degenerate after clamping": 3}
    out = []
    hw = np.asarray([hw], np.int32)
    for d in np.ascontiguousarray(dets[:, :4], np.float32):
        rc = L.hrn_crop_geometry(d.ctypes.data, 4, 1, hw.ctypes.data, 0, res[0], res[1], variant, None, None)
        out.append(0 if rc == 0 else texts[L.hrn_crop_geometry_last_error().decode().split(" ", 2)[2]])
    return np.asarray(out, np.int32)


# Seed of the frames and the first detections.  The test needs at least 2 of the 3 people alive (status 0) in every frame and asserts
# it; whether seed 0 gives that has NOT been confirmed on a GPU yet -- if the assertion fires, choose another seed here.
CHAIN_SEED = 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_the_chain_equals_the_host_composition_it_replaces(dtype):
    res = (64, 96)
    net = engine(res, dtype)
    L = net._lib
    hf, wf = SIZES[0]
    frames = [torch.from_numpy(noise_frame(hf, wf, 100 * CHAIN_SEED + k)).cuda() for k in range(4)]
    rng = np.random.default_rng(CHAIN_SEED)
    dets0 = make_boxes(rng, hf, wf, 8)[[0, 3, 5]]
    box_args = {"threshold": -3e38}
    _, prev = net.predict_frame(frames[0], dets0)
    black = black_crop(*res)
    for k in (1, 2, 3):
        boxes, pts, status = net.track_frame(frames[k], prev, **box_args)
        assert boxes.is_cuda and pts.is_cuda and status.is_cuda and tuple(pts.shape) == (3, 17, 3)
        # the composition it replaces: download, boxes on the host, predict_frame for the people the host geometry accepts
        host_dets = pose_boxes_ref(prev.cpu().numpy(), (hf, wf), **box_args)
        want_status = host_accepts(L, host_dets, (hf, wf), res)
        np.testing.assert_array_equal(status.cpu().numpy(), want_status)
        ok = want_status == 0
        print("frame %d: status %s" % (k, want_status.tolist()))
        assert ok.sum() >= 2, "a chain of dead people tests nothing: choose another CHAIN_SEED"
        want_boxes, want_pts = net.predict_frame(frames[k], host_dets[ok])
        np.testing.assert_array_equal(boxes.cpu().numpy()[ok], want_boxes)
        assert np.array_equal(bits(pts.cpu().numpy()[ok]), bits(want_pts.cpu().numpy()))
        # the others: the black crop, a zero box
        dets_dev = net.boxes_from_poses(prev, (hf, wf), **box_args)
        assert np.array_equal(bits(dets_dev.cpu().numpy()), bits(host_dets))
        images, boxes2, status2 = net.preprocess_frames_dev(frames[k], dets_dev)
        assert torch.equal(status2, status) and torch.equal(boxes2, boxes)
        for i in np.flatnonzero(~ok):
            assert np.array_equal(bits(images[i].cpu().numpy()), bits(black)) and not boxes[i].any()
        prev = pts
    # with heat-maps and a refined decode: the same boxes, the composition's joints
    out = net.track_frame(frames[3], prev, return_heatmaps=True, refine="quarter", **box_args)
    assert len(out) == 4 and tuple(out[3].shape) == (3, 17, 16, 24)
    host_dets = pose_boxes_ref(prev.cpu().numpy(), (hf, wf), **box_args)
    ok = host_accepts(L, host_dets, (hf, wf), res) == 0
    want = net.predict_frame(frames[3], host_dets[ok], return_heatmaps=True, refine="quarter")
    assert np.array_equal(bits(out[1].cpu().numpy()[ok]), bits(want[1].cpu().numpy()))
    assert np.array_equal(bits(out[3].cpu().numpy()[ok]), bits(want[2].cpu().numpy()))
    assert net.pad_violations() == 0


@pytest.mark.parametrize("kind", ["bgr", "nv12"])
def test_the_clip_form_equals_single_calls(kind):
    """the people of 3 frames (three sizes) in one track_frame call, interleaved, against one call per frame"""
    pkg = load_pkg()
    net = engine((64, 64))
    frames, sizes = make_frames(pkg, kind)
    frames = net._device_frames(frames)
    rng = np.random.default_rng(8)
    prev = [net.predict_frame(f, make_boxes(rng, hf, wf, 8)[[1, 4, 6]])[1] for f, (hf, wf) in zip(frames, sizes)]
    box_args = {"threshold": -3e38, "min_side": 4.0}
    single = [net.track_frame(f, p, **box_args) for f, p in zip(frames, prev)]
    index = np.asarray([0, 1, 2, 2, 1, 0, 1, 0, 2], np.int32)
    slot = np.asarray([0, 0, 0, 1, 1, 1, 2, 2, 2])             # person i of the call is person slot[i] of its frame
    all_prev = torch.stack([prev[f][s] for f, s in zip(index, slot)])
    boxes, pts, status = net.track_frame(frames, all_prev, frame_index=index, **box_args)
    for i, (f, s) in enumerate(zip(index, slot)):
        assert torch.equal(boxes[i], single[f][0][s]) and torch.equal(status[i], single[f][2][s])
        assert np.array_equal(bits(pts[i].cpu().numpy()), bits(single[f][1][s].cpu().numpy()))
    assert int((status == 0).sum()) >= 6
    with pytest.raises(ValueError, match="frame_index"):
        net.track_frame(frames, all_prev, **box_args)
    assert net.pad_violations() == 0


# --------------------------------------------------------------------------------------------------------------- SimpleHRNet
class CountingDetector(TableDetector):
    def __init__(self, table):
        super().__init__(table)
        self.calls = []

    def predict_single(self, image, color_mode="BGR"):
        self.calls.append(self.frame_number)
        return super().predict_single(image, color_mode)


def test_simple_hrnet_redetects_every_third_call():
    pkg = load_pkg()
    hf, wf = SIZES[0]
    frames = [noise_frame(hf, wf, 200 + k) for k in range(7)]
    dets = make_boxes(np.random.default_rng(9), hf, wf, 8)[[0, 2, 5, 7]]
    track_args = {"threshold": -3e38}
    detector = CountingDetector({0: dets})
    model = pkg.SimpleHRNet(32, 17, state_dict_np(32, 0), resolution=(64, 96), multiperson=True, return_heatmaps=True,
                            return_bounding_boxes=True, device="cuda:0", detector=detector, redetect_every=3, track_args=track_args)
    plain = pkg.SimpleHRNet(32, 17, state_dict_np(32, 0), resolution=(64, 96), multiperson=True, return_heatmaps=True,
                            return_bounding_boxes=True, device="cuda:0", detector=TableDetector({0: dets}))
    net = model.model
    prev = None
    for k, frame in enumerate(frames):
        detector.frame_number = k
        hm, boxes, pts = model.predict(frame)
        assert hm.dtype == np.float32 and boxes.dtype == np.int32 and pts.dtype == np.float32
        if k % 3 == 0:
            # a detector call: what redetect_every = 1 (the default: the parent's code path) returns for this frame, which is
            # predict_frame with the detector's rows
            want_hm, want_boxes, want_pts = plain.predict(frame)
            ref = net.predict_frame(frame, dets, return_heatmaps=True)
            np.testing.assert_array_equal(want_boxes, ref[0])
            assert np.array_equal(bits(want_pts), bits(ref[1].cpu().numpy())) and np.array_equal(bits(want_hm), bits(ref[2].cpu().numpy()))
        else:
            # a tracked call: track_frame from the previous call's joints, dead people removed
            tb, tp, ts, th = net.track_frame(frame, torch.from_numpy(prev).cuda(), return_heatmaps=True, **track_args)
            alive = (ts == 0).cpu().numpy()
            assert alive.sum() >= 2
            want_boxes, want_pts, want_hm = tb.cpu().numpy()[alive], tp.cpu().numpy()[alive], th.cpu().numpy()[alive]
        np.testing.assert_array_equal(boxes, want_boxes)
        assert np.array_equal(bits(pts), bits(want_pts)) and np.array_equal(bits(hm), bits(want_hm))
        prev = pts
    assert detector.calls == [0, 3, 6]
    # after a call that returned nobody the detector runs again, whatever the call number
    for k in (7, 8):
        detector.frame_number = k
        model.predict(frames[k - 7])
    assert detector.calls == [0, 3, 6]
    model.detector = empty = CountingDetector({0: None})
    empty.frame_number = 9
    assert model.predict(frames[2])[2].shape == (0, 0, 3) and empty.calls == [9]
    model.detector = again = CountingDetector({0: dets})
    again.frame_number = 10
    assert len(model.predict(frames[3])[2]) == 4 and again.calls == [10]
    again.frame_number = 11
    assert len(model.predict(frames[4])[2]) >= 2 and again.calls == [10]       # tracked
    assert net.pad_violations() == 0 and plain.model.pad_violations() == 0


def test_no_pad_violations_after_the_new_paths():
    engine()
    for key, net in _NETS.items():
        assert net.pad_violations() == 0, key
