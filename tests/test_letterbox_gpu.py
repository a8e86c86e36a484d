"""The detector link on the GPU: ``detector_input`` against the restated letterbox byte for byte / bit for bit, the clip and YUV
forms, ``detections_to_frame`` against its host form, the chain into ``preprocess_frames_dev``, and
``SimpleHRNet(device_detector=...)`` against ``SimpleHRNet(detector=...)`` with the host-mapped rows.  Every comparison is equality.

W32, 17 joints, crops (64, 96); detector tensors of 64 x 64 and (64, 96); frames of a few dozen pixels a side."""
import numpy as np
import pytest
import torch

import yuv_ref
from conftest import load_pkg, state_dict_np
from letterbox_ref import PAD, letterbox_u8, random_rows, to_tensor

pytestmark = pytest.mark.gpu

# (frame h, w), size, what the case is
CASES = [((48, 64), 64, "copy"), ((37, 53), 64, "upscale, odd pad"), ((90, 160), 64, "downscale"), ((72, 128), 64, "2:1 wide"),
         ((128, 72), 64, "2:1 tall"), ((73, 128), 64, "ratio 0.5 but not 2:1"), ((3, 200), 64, "one resized row"),
         ((50, 100), (64, 96), "rectangular")]
DTYPES = [torch.uint8, torch.float32, torch.float16, torch.bfloat16]
_NETS = {}


def engine(dtype="fp32"):
    if dtype not in _NETS:
        _NETS[dtype] = load_pkg().NativeHRNet(32, 17, (64, 96), dtype, max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    return _NETS[dtype]


def noise_frame(hf, wf, seed):
    return np.random.default_rng(seed).integers(0, 256, (hf, wf, 3), dtype=np.uint8)


def same(got: torch.Tensor, want: torch.Tensor, what=""):
    """equal bits (the 16-bit and float forms compared as integers of their width)"""
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, got.shape, want.shape)
    view = {torch.uint8: torch.uint8, torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}[got.dtype]
    a, b = got.cpu().contiguous().view(view), want.contiguous().view(view)
    assert torch.equal(a, b), "%s: %d of %d elements differ" % (what, int((a != b).sum()), a.numel())


def styles_of(size):
    return ("yolov5",) if np.ndim(size) else ("yolov3", "yolov5")


@pytest.mark.parametrize("hw,size,what", CASES, ids=[c[2] for c in CASES])
def test_detector_input_equals_the_restatement(hw, size, what):
    net = engine()
    frame = noise_frame(hw[0], hw[1], hw[0] * 1000 + hw[1])
    on_device = torch.from_numpy(frame).cuda()
    for style in styles_of(size):
        for order in ("rgb", "bgr"):
            want_u8 = letterbox_u8(frame, size, style, order)
            for dtype in DTYPES:
                got, geometry = net.detector_input(on_device, size, style, dtype=dtype, order=order)
                same(got[0], to_tensor(want_u8, dtype), "%s %s %s %s" % (what, style, order, dtype))
                assert got.is_cuda and len(geometry) == 1 and tuple(geometry.frame_hw[0]) == hw
    # the cases are what their names say: which of cv2.resize's three paths the frame takes
    g = geometry
    copy, area = (g.new_h[0], g.new_w[0]) == hw, (2 * g.new_h[0], 2 * g.new_w[0]) == hw
    assert copy == (what == "copy") and area == what.startswith("2:1")
    # a pad of the caller's, per channel in OUTPUT order; the default is the style's
    got, _ = net.detector_input(frame, size, styles_of(size)[0], dtype=torch.uint8, order="bgr", pad=(1, 2, 3))
    same(got[0], to_tensor(letterbox_u8(frame, size, styles_of(size)[0], "bgr", (1, 2, 3)), torch.uint8), "pad")
    if what != "rectangular" and (g.top[0] or g.left[0]):
        assert int(got[0, 0, 0, 2]) == 3 and PAD["yolov3"] == 128 and PAD["yolov5"] == 114


def test_detector_input_clip_form_equals_single_calls():
    net = engine()
    frames = [noise_frame(90, 160, 1), noise_frame(37, 53, 2), noise_frame(128, 72, 3)]
    for style, size in (("yolov3", 64), ("yolov5", (64, 96))):
        for dtype in DTYPES:
            got, geometry = net.detector_input(frames, size, style, dtype=dtype)
            assert len(geometry) == 3 and got.shape[0] == 3
            for k, f in enumerate(frames):
                one, g1 = net.detector_input(f, size, style, dtype=dtype)
                same(got[k], one[0].cpu(), "%s %s frame %d" % (style, dtype, k))
                same(one[0], to_tensor(letterbox_u8(f, size, style), dtype), "single")
                assert (g1.new_w[0], g1.top[0], g1.dw[0]) == (geometry.new_w[k], geometry.top[k], geometry.dw[k])
    # a stack is the same call
    stack = np.stack([noise_frame(48, 64, 5), noise_frame(48, 64, 6)])
    got, _ = net.detector_input(stack, 64, dtype=torch.uint8)
    for k in range(2):
        same(got[k], to_tensor(letterbox_u8(stack[k], 64, "yolov3"), torch.uint8), "stack")


@pytest.mark.parametrize("fmt,matrix,range_", [("nv12", "bt601", "limited"), ("i420", "bt709", "full"), ("nv12", "bt709", "full"),
                                               ("i420", "bt601", "limited")])
def test_detector_input_from_yuv_equals_the_bgr_entry_on_the_converted_frame(fmt, matrix, range_):
    pkg, net = load_pkg(), engine()
    frames, converted = [], []
    for k, (hf, wf) in enumerate([(72, 128), (38, 54), (90, 160), (48, 64)]):     # 2:1, upscale, downscale, copy
        pitch = wf + 32 if k % 2 == 0 else None
        data = np.random.default_rng(70 + k).integers(0, 256, yuv_ref.nbytes(hf, wf, pitch), dtype=np.uint8)
        frames.append(pkg.YuvFrame(data, hf, wf, fmt, matrix, range_, pitch))
        converted.append(yuv_ref.yuv_to_bgr(data, hf, wf, fmt, matrix, range_, pitch))
    for dtype in (torch.uint8, torch.float16):
        got, _ = net.detector_input(frames, 64, "yolov3", dtype=dtype)
        want, _ = net.detector_input(converted, 64, "yolov3", dtype=dtype)
        same(got, want.cpu(), "%s %s" % (fmt, dtype))
        for k in range(len(frames)):
            same(got[k], to_tensor(letterbox_u8(converted[k], 64, "yolov3"), dtype), "restatement, frame %d" % k)
    one, _ = net.detector_input(frames[0], (64, 96), "yolov5", dtype=torch.float32, order="bgr")
    same(one[0], to_tensor(letterbox_u8(converted[0], (64, 96), "yolov5", "bgr"), torch.float32), "one YUV frame")


def test_detector_input_refusals():
    net = engine()
    frame = noise_frame(48, 64, 0)
    with pytest.raises(RuntimeError, match="resized to nothing"):
        net.detector_input(noise_frame(1, 200, 0), 64)
    for kw in ({"style": "yolov4"}, {"dtype": torch.float64}, {"order": "gbr"}, {"pad": 300}, {"pad": (1, 2)}):
        with pytest.raises(ValueError):
            net.detector_input(frame, 64, **kw)
    with pytest.raises(ValueError):
        net.detector_input(frame, (64, 96), "yolov3")


# ------------------------------------------------------------------------------------------------------------ boxes back
FRAMES4 = [(480, 640), (37, 53), (1080, 1920), (300, 200)]


@pytest.mark.parametrize("style,size", [("yolov3", 416), ("yolov5", (384, 640))])
@pytest.mark.parametrize("compact", [True, False])
def test_detections_to_frame_equals_the_host_form(compact, style, size):
    P, net = load_pkg("postproc"), engine()
    g1 = P.letterbox_geometry(FRAMES4[:1], size, style)
    kw = {"conf_thres": 0.4, "classes": [0, 2], "compact": compact}
    for n in (0, 1, 255, 256, 257, 700):                                     # across the chunks of 256 rows
        d = random_rows(n, 7, size, seed=n)
        if n >= 255:
            d[3, 0], d[200, 4], d[254, 2] = np.nan, np.inf, -np.inf          # every status value occurs
        got = net.detections_to_frame(torch.from_numpy(d).cuda(), g1, **kw)
        want = P.detections_to_frame(d, g1, **kw)
        for a, b in zip(got, want):
            assert a.is_cuda and np.array_equal(a.cpu().numpy().view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), n
        if n >= 255:
            assert set(np.unique(want[2]).tolist()) == {0, 1, 2, 5}
    # four frames in one launch, one of them empty, one longer than two chunks
    g4 = P.letterbox_geometry(FRAMES4, size, style)
    counts = [300, 0, 700, 5]
    d = random_rows(sum(counts), 6, size, seed=9)
    d[301, 1] = np.nan
    for more in ({}, {"conf_thres": None, "classes": None}, {"class_col": 5}):
        args = dict(kw, **more)
        got = net.detections_to_frame(d, g4, counts=counts, **args)          # (a host array is uploaded)
        want = P.detections_to_frame(d, g4, counts=counts, **args)
        for a, b in zip(got, want):
            assert np.array_equal(a.cpu().numpy().view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), more
    assert want[1][1] == 0 and 0 < want[1][2] < 700
    with pytest.raises(RuntimeError, match="conf_col"):
        net.detections_to_frame(d, g4, counts=counts, conf_col=9)


def people_rows(geometry, sizes, per_frame, seed):
    """detector rows in LETTERBOX coordinates whose boxes lie inside their frames: frame boxes mapped forward"""
    rng = np.random.default_rng(seed)
    rows = []
    for k, (hf, wf) in enumerate(sizes):
        a, b = rng.uniform(0.05, 0.95, (2, per_frame, 2)) * (wf, hf)
        lo, hi = np.minimum(a, b), np.maximum(a, b) + 6
        box = np.concatenate([lo, hi], 1)
        sx, sy = geometry.new_w[k] / wf, geometry.new_h[k] / hf
        fwd = box * (sx, sy, sx, sy) + (geometry.left[k], geometry.top[k], geometry.left[k], geometry.top[k])
        conf = rng.uniform(0.2, 1.0, (per_frame, 1))
        cls = rng.integers(0, 2, (per_frame, 1))
        rows.append(np.concatenate([fwd, conf, conf, cls], 1).astype(np.float32))
    return rows


@pytest.mark.parametrize("variant", ["pad", "clamp"])
def test_chained_with_preprocess_frames_dev(variant):
    P, net = load_pkg("postproc"), engine()
    sizes = [(120, 160), (97, 131), (150, 90)]
    frames = [noise_frame(hf, wf, 10 + k) for k, (hf, wf) in enumerate(sizes)]
    _, geometry = net.detector_input(frames, 64, "yolov3")
    rows = people_rows(geometry, sizes, 6, seed=2)
    counts = [len(r) for r in rows]
    d = np.concatenate(rows)
    kw = {"conf_thres": 0.5, "classes": [0], "compact": False}
    index = np.repeat(np.arange(3, dtype=np.int32), counts)
    on_dev, kept_dev, status_dev = net.detections_to_frame(torch.from_numpy(d).cuda(), geometry, counts=counts, **kw)
    images, boxes, status = net.preprocess_frames_dev(frames, on_dev, index, variant)
    host_rows, kept, host_status = P.detections_to_frame(d, geometry, counts=counts, **kw)
    assert 0 < kept.sum() < len(d)
    alive = host_status == 0
    # dropped rows are the five-zero row: status 1 there, an all-padding crop and a zero box
    np.testing.assert_array_equal(status.cpu().numpy(), np.where(alive, 0, 1))
    assert not boxes.cpu().numpy()[~alive].any()
    dev_frames = net._device_frames(frames)
    want_images, want_boxes, _ = net._preprocess_table(net._frame_table(dev_frames), 3, np.ascontiguousarray(host_rows[alive][:, :4]),
                                                       np.ascontiguousarray(index[alive]), variant)
    keep = torch.from_numpy(np.flatnonzero(alive)).cuda()
    assert torch.equal(images[keep], want_images) and np.array_equal(boxes.cpu().numpy()[alive], want_boxes)
    # compacted: the kept rows alone, by the counts
    packed, kept2, _ = net.detections_to_frame(d, geometry, counts=counts, **dict(kw, compact=True))
    assert kept2.cpu().numpy().tolist() == kept.tolist() == kept_dev.cpu().numpy().tolist()
    starts = np.concatenate([[0], np.cumsum(counts)])
    gather = np.concatenate([np.arange(s, s + k) for s, k in zip(starts, kept)])
    images2, boxes2, status2 = net.preprocess_frames_dev(frames, packed[torch.from_numpy(gather).cuda()], index[alive], variant)
    assert not status2.any() and torch.equal(images2, want_images) and np.array_equal(boxes2.cpu().numpy(), want_boxes)


# ------------------------------------------------------------------------------------------ SimpleHRNet(device_detector=...)
class FakeDeviceDetector:
    """fixed rows in letterbox coordinates, returned as device tensors; what it was given is kept for the test to look at"""
    size, style, conf_thres, classes = 64, "yolov3", 0.5, [0]

    def __init__(self, table):
        self.table, self.seen, self.frame_number = table, [], 0

    def predict_tensor(self, x):
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape[1:]) == (3, 64, 64)
        self.seen.append(x)
        first = self.frame_number
        return [None if self.table.get(first + k) is None else torch.from_numpy(self.table[first + k]).cuda() for k in range(x.shape[0])]


class FakeHostDetector:
    """the same rows mapped on the host: what the reference's wrapper hands to predict()"""

    def __init__(self, table, geometries, P):
        self.frame_number, self.P, self.table, self.geometries = 0, P, table, geometries

    def rows(self, k):
        if self.table.get(k) is None:
            return None
        out, kept, _ = self.P.detections_to_frame(self.table[k], self.geometries[k], conf_thres=0.5, classes=[0])
        return out[:kept[0]]

    def predict_single(self, image, color_mode="BGR"):
        return self.rows(self.frame_number)

    def predict(self, images, color_mode="BGR"):
        return [self.rows(self.frame_number + k) for k in range(len(images))]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_simple_hrnet_device_detector_equals_the_host_detector(dtype):
    pkg, P = load_pkg(), load_pkg("postproc")
    hf, wf = 120, 160
    frames = [noise_frame(hf, wf, 40 + k) for k in range(4)]
    g = P.letterbox_geometry((hf, wf), 64, "yolov3")
    table = {k: people_rows(g, [(hf, wf)], 7, seed=20 + k)[0] for k in range(4)}
    table[3] = None                                                               # the detector finds nobody on the last frame
    kw = dict(resolution=(64, 96), multiperson=True, return_heatmaps=True, return_bounding_boxes=True, device="cuda:0", dtype=dtype)
    sd = state_dict_np(32, 0)
    fake = FakeDeviceDetector(table)
    dev = pkg.SimpleHRNet(32, 17, sd, device_detector=fake, **kw)
    host_detector = FakeHostDetector(table, {k: g for k in range(4)}, P)
    host = pkg.SimpleHRNet(32, 17, sd, detector=host_detector, **kw)

    def equal(got, want):
        for a, b in zip(got, want):
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))

    for k in range(4):                                                            # single images
        fake.frame_number = host_detector.frame_number = k
        got, want = dev.predict(frames[k]), host.predict(frames[k])
        equal(got, want)
        assert len(want[2]) == (0 if k == 3 else len(want[1])) and (k == 3 or 0 < len(want[2]) < 7)
    # what the detector was given is the letterboxed frame
    assert torch.equal(fake.seen[0].cpu()[0], to_tensor(letterbox_u8(frames[0], 64, "yolov3"), torch.float32))
    fake.frame_number = host_detector.frame_number = 0                            # a stack of two, and one with the empty frame
    for lo, hi in ((0, 2), (2, 4)):
        fake.frame_number = host_detector.frame_number = lo
        got, want = dev.predict(np.stack(frames[lo:hi])), host.predict(np.stack(frames[lo:hi]))
        for a, b in zip(got, want):
            assert len(a) == len(b) == 2
            equal(a, b)
    # redetect_every = 3: the detector on calls 0 and 3, tracking in between, with either kind of detector
    dev3 = pkg.SimpleHRNet(32, 17, sd, device_detector=fake, redetect_every=3, **kw)
    host3 = pkg.SimpleHRNet(32, 17, sd, detector=host_detector, redetect_every=3, **kw)
    seen = len(fake.seen)
    for k in (0, 1, 2, 1):
        fake.frame_number = host_detector.frame_number = k
        equal(dev3.predict(frames[k]), host3.predict(frames[k]))
    assert len(fake.seen) == seen + 2
    with pytest.raises(ValueError, match="not both"):
        pkg.SimpleHRNet(32, 17, sd, detector=host_detector, device_detector=fake, **kw)
