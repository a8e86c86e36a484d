"""YUV (NV12 / I420) input on the GPU: ``yuv_to_bgr`` against the numpy restatement (tests/yuv_ref.py), and every entry that
accepts a ``YuvFrame`` against the same entry on the restatement's BGR frame -- images, boxes, joints and heat-maps, bit for
bit, no tolerance.  Frames are random bytes in all planes, so both clips and max(0, Y - y0) are exercised."""
import numpy as np
import pytest
import torch

import yuv_ref
from conftest import load_pkg, state_dict_np
from test_frames_host import make_boxes

pytestmark = pytest.mark.gpu

TABLE_KEYS = [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")]
H, W = 64, 96


def raw(height, width, seed, pitch=None):
    """rawvideo bytes of a frame, the pitch bytes included: all random"""
    return np.random.default_rng(seed).integers(0, 256, yuv_ref.nbytes(height, width, pitch), dtype=np.uint8)


def make(pkg, height, width, fmt, key, seed, pitch=None):
    """(YuvFrame on the host, the restatement's BGR frame of it)"""
    data = raw(height, width, seed, pitch)
    frame = pkg.YuvFrame(data, height, width, fmt, key[0], key[1], pitch)
    return frame, yuv_ref.yuv_to_bgr(data, height, width, fmt, key[0], key[1], pitch)


def people(hf, wf, count, seed):
    rng = np.random.default_rng(seed)
    boxes = make_boxes(rng, hf, wf, 16)
    return np.ascontiguousarray(boxes[rng.permutation(len(boxes))[:count]])


@pytest.fixture(scope="module")
def net32():
    net = load_pkg().NativeHRNet(32, 17, (H, W), "fp32", max_batch=4, device=0)
    yield net
    net.close()


# ----------------------------------------------------------------------------------------------------- whole frames
# (height, width, pitch): the smallest frame; a pitched one whose width is 2 mod 4 (a last run of 2 pixels, odd rows that start
# off a dword); an unpitched one of that kind; widths that are multiples of the run of 4, in one block and in several
BGR_CASES = [(2, 2, None), (34, 50, 64), (8, 22, None), (12, 40, None), (48, 88, None), (6, 4, 6)]


@pytest.mark.parametrize("key", TABLE_KEYS, ids=["%s-%s" % k for k in TABLE_KEYS])
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_yuv_to_bgr_equals_the_restatement(net32, fmt, key):
    pkg = load_pkg()
    for k, (h, w, pitch) in enumerate(BGR_CASES):
        frame, want = make(pkg, h, w, fmt, key, 100 + k, pitch)
        got = net32.yuv_to_bgr(frame)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3) and got.is_cuda and got.is_contiguous()
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=str((fmt, key, h, w, pitch)))
        # a device-resident frame, at an address that is off a dword: nothing leaks from the bytes around it either
        buf = torch.full((frame.nbytes + 3,), 255, dtype=torch.uint8, device="cuda")
        buf[1:1 + frame.nbytes] = frame.data.cuda()
        resident = pkg.YuvFrame(buf[1:1 + frame.nbytes], h, w, fmt, key[0], key[1], pitch)
        np.testing.assert_array_equal(net32.yuv_to_bgr(resident).cpu().numpy(), want)
    with pytest.raises(TypeError):
        net32.yuv_to_bgr(np.zeros((2, 2, 3), np.uint8))


# ------------------------------------------------------------------------------------------------------ one frame
# boxes of a 120 x 160 frame for a (64, 96) network, valid in both variants
FRAME_BOXES = np.asarray([
    [31, 17, 90, 80],        # odd x1 and odd y1: a chroma sample is shared across the crop's left and top edge
    [33, 21, 96, 63],        # ... and an odd x2 / y2 as well
    [100, 60, 160, 120],     # touches the right and the bottom edge
    [10, 50, 150, 70],       # wide: "pad" adds zero rows above and below
    [70, 5, 90, 115],        # tall: "pad" adds zero columns left and right
    [0, 0, 160, 120],        # the whole frame: downscaled
    [40, 40, 64, 56],        # 24 x 16: upscaled
    [20, 30, 116, 94],       # 96 x 64: no pass at all
    [20, 0, 116, 40],        # padded width == W with another height ("clamp": the top edge cuts the enlarged box)
    [0, 20, 30, 84],         # padded height == H with another width ("clamp": the left edge cuts it)
    [12.5, 7.5, 77.5, 101.5],  # ties in the rounding
], np.float32)


def test_the_boxes_are_what_their_comments_say():
    """the geometry of FRAME_BOXES through hrn_crop_geometry: every branch the cases are there for is taken"""
    L = load_pkg("_lib").load()
    hw = np.asarray([[120, 160]], np.int32)
    sl = {}
    for variant in (0, 1):
        out = np.zeros((len(FRAME_BOXES), 8), np.int32)
        assert L.hrn_crop_geometry(FRAME_BOXES.ctypes.data, 4, len(FRAME_BOXES), hw.ctypes.data, 0, H, W, variant, None, out.ctypes.data) == 0
        sl[variant] = out     # x1, y1, w_crop, h_crop, pad_top, pad_left, h_pad, w_pad
    pad, clamp = sl[0], sl[1]
    assert (pad[:2, :2] % 2 == 1).all()
    assert pad[2, 0] + pad[2, 2] == 160 and pad[2, 1] + pad[2, 3] == 120
    assert pad[3, 4] > 0 and pad[3, 6] - pad[3, 3] - pad[3, 4] > 0          # zero rows above and below
    assert pad[4, 5] > 0 and pad[4, 7] - pad[4, 2] - pad[4, 5] > 0          # zero columns left and right
    assert pad[5, 7] > W and pad[5, 6] > H and pad[6, 7] < W and pad[6, 6] < H
    assert tuple(pad[7, 6:]) == (H, W) == tuple(clamp[7, 6:])
    assert clamp[8, 7] == W and clamp[8, 6] != H and clamp[9, 6] == H and clamp[9, 7] != W
    assert (clamp[:, 4:6] == 0).all()


@pytest.mark.parametrize("variant", ["pad", "clamp"])
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_preprocess_frame_equals_the_bgr_path(net32, fmt, variant):
    pkg = load_pkg()
    for k, key in enumerate(TABLE_KEYS):
        pitch = (None, 192)[k % 2]
        frame, bgr = make(pkg, 120, 160, fmt, key, 200 + k, pitch)
        want = net32.preprocess_frame(bgr, FRAME_BOXES, variant)
        got = net32.preprocess_frame(frame, FRAME_BOXES, variant)
        assert tuple(got[0].shape) == (len(FRAME_BOXES), 3, H, W) and got[0].dtype == torch.float32
        assert torch.equal(got[0], want[0]), (fmt, key, variant)
        assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1])
        assert got[2].dtype == torch.int32 and torch.equal(got[2], want[2])
        # the device's own conversion of the frame gives the same crops once more
        again = net32.preprocess_frame(net32.yuv_to_bgr(frame), FRAME_BOXES, variant)
        assert torch.equal(again[0], want[0])
    images, boxes, boxes_dev = net32.preprocess_frame(frame, np.zeros((0, 4), np.float32), variant)
    assert tuple(images.shape) == (0, 3, H, W) and boxes.shape == (0, 4) and tuple(boxes_dev.shape) == (0, 4)


# ----------------------------------------------------------------------------------------------------- many frames
def five_frames(pkg):
    """one NV12, one I420, one pitched, two of another size with nobody (None / an empty array); all four tables"""
    spec = [(120, 160, "nv12", TABLE_KEYS[0], None, 5), (120, 160, "i420", TABLE_KEYS[2], None, 4), (120, 160, "i420", TABLE_KEYS[3], 192, 3),
            (96, 132, "nv12", TABLE_KEYS[1], None, None), (96, 132, "nv12", TABLE_KEYS[1], 136, 0)]
    frames, bgrs, dets = [], [], []
    for k, (h, w, fmt, key, pitch, count) in enumerate(spec):
        f, b = make(pkg, h, w, fmt, key, 300 + k, pitch)
        frames.append(f), bgrs.append(b)
        dets.append(None if count is None else people(h, w, count, 310 + k) if count else np.zeros((0, 7), np.float32))
    return frames, bgrs, dets


@pytest.mark.parametrize("variant", ["pad", "clamp"])
def test_preprocess_frames_equals_per_frame_calls(net32, variant):
    pkg = load_pkg()
    frames, bgrs, dets = five_frames(pkg)
    assert {(f.matrix, f.range) for f in frames} == set(TABLE_KEYS)
    singles = [net32.preprocess_frame(f, d, variant) for f, d in zip(frames, dets) if d is not None and len(d)]
    want = (torch.cat([s[0] for s in singles]), np.concatenate([s[1] for s in singles]), torch.cat([s[2] for s in singles]))
    bgr_want = net32.preprocess_frames(bgrs, dets, variant)
    for given in (frames,
                  [frames[0], frames[1].to("cuda"), frames[2], None, frames[4]],      # one device-resident, one absent
                  tuple(f.to(net32.torch_device) for f in frames)):
        got = net32.preprocess_frames(given, dets, variant)
        assert got[3] == [5, 4, 3, 0, 0]
        for g, w, b in zip(got[:3], want, bgr_want[:3]):
            assert (torch.equal(g, w) and torch.equal(g, b)) if isinstance(g, torch.Tensor) else (np.array_equal(g, w) and np.array_equal(g, b))
    with pytest.raises(ValueError, match="mixture"):
        net32.preprocess_frames([frames[0], bgrs[1], frames[2], None, None], dets, variant)
    with pytest.raises(ValueError, match="mixture"):
        net32.predict_frames([bgrs[0], frames[1], frames[2], None, None], dets, variant=variant)
    with pytest.raises(ValueError, match="is None but has"):
        net32.preprocess_frames([None] + frames[1:], dets, variant)


CLIP_COUNTS = [3, 0, 4, 2, 9, 1, 3, 2]      # max_batch 8: one frame above a pass; four people per pass: nine groups


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_predict_frames_and_predict_clip_equal_the_bgr_path(dtype):
    pkg, native = load_pkg(), load_pkg("native")
    net = pkg.NativeHRNet(32, 17, (H, W), dtype, max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    sizes = [(120, 160), (96, 132), (120, 160), (150, 90), (120, 160), (96, 132), (150, 90), (120, 160)]
    frames, bgrs, dets = [], [], []
    for k, ((h, w), count) in enumerate(zip(sizes, CLIP_COUNTS)):
        f, b = make(pkg, h, w, ("nv12", "i420")[k % 2], TABLE_KEYS[k % 4], 400 + k, (None, None, w + 14)[k % 3])
        frames.append(f), bgrs.append(b)
        dets.append(people(h, w, count, 410 + k) if count else None)
    assert len(list(native.group_frames(CLIP_COUNTS, 8, 4))) >= 4 and max(CLIP_COUNTS) > 8
    for variant in ("pad", "clamp"):
        want = net.predict_frames(bgrs, dets, return_heatmaps=True, variant=variant)
        got = net.predict_frames(frames, dets, return_heatmaps=True, variant=variant)
        pinned = [(pkg.YuvFrame(f.data.pin_memory(), f.height, f.width, f.format, f.matrix, f.range, f.pitch), d) for f, d in zip(frames, dets)]
        clip = list(net.predict_clip(iter(pinned), people_per_pass=4, return_heatmaps=True, variant=variant))
        torch.cuda.synchronize()
        assert len(got) == len(clip) == len(want) == len(frames)
        for k, w in enumerate(want):
            for res in (got[k], clip[k]):
                assert res[0].dtype == np.int32 and np.array_equal(res[0], w[0]), (dtype, variant, k)
                assert torch.equal(res[1], w[1]) and torch.equal(res[2], w[2]), (dtype, variant, k)
            assert len(w[0]) == CLIP_COUNTS[k]
    # one frame, the live loop's call
    boxes, pts, hm = net.predict_frame(frames[2], dets[2], return_heatmaps=True)
    wb, wp, wh = net.predict_frame(bgrs[2], dets[2], return_heatmaps=True)
    assert np.array_equal(boxes, wb) and torch.equal(pts, wp) and torch.equal(hm, wh) and len(boxes) == 4
    # refusals of the clip loop: a device-resident frame, a mixture
    with pytest.raises(TypeError, match="predict_frames"):
        list(net.predict_clip([(frames[0].to("cuda"), dets[0])]))
    with pytest.raises(ValueError, match="mixture"):
        list(net.predict_clip([(frames[0], dets[0]), (bgrs[2], dets[2])]))
    net.close()


def test_predict_frame_smoke(net32):
    """predict_frame(YuvFrame) == predict_frame(its BGR frame): boxes, joints, heat-maps (weights as the engine is created)"""
    pkg = load_pkg()
    net = pkg.NativeHRNet(32, 17, (H, W), "bf16", max_batch=4, device=0).load_state_dict(state_dict_np(32, 0))
    frame, bgr = make(pkg, 120, 160, "nv12", TABLE_KEYS[0], 500)
    d = people(120, 160, 3, 501)
    got, want = net.predict_frame(frame, d, return_heatmaps=True), net.predict_frame(bgr, d, return_heatmaps=True)
    assert np.array_equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert tuple(got[1].shape) == (3, 17, 3)
    net.close()
