"""Detector NMS on the GPU: ``hrn_detector_nms_dev`` against the host form BIT FOR BIT on all four outputs (both compile
csrc/detector_nms_math.h), over whole output buffers pre-filled with a sentinel; float16 input; a side stream; scratch reuse;
refusals; and ``SimpleHRNet(device_detector=<predict_raw>)`` against the same detector with its NMS on the host.

Shapes are the smallest that reach each branch of csrc/detector_nms.hip: N around one wave (63 / 64 / 65), one block (255 / 256 /
257) and several blocks (1023 / 1025) of the scoring launch; C = 1, 2, 3, 80 (20-, 28-, 32- and 340-byte rows, a lane per class
with and without a second trip); candidate counts around a wave and a block of the per-image launch; max_candidates below the
number that qualifies (the radix select and the ordered compaction) with equal keys across the cut; 4096 candidates of 5000 (the
largest LDS layout); and the two head sizes of the reference's detectors, (2, 10 647, 85) and (1, 25 200, 85)."""
import numpy as np
import pytest
import torch

from conftest import load_pkg, state_dict_np
from detector_nms_ref import RULES, designed_cases, random_pred

pytestmark = pytest.mark.gpu

_NETS = {}
OUTPUTS = ("rows", "counts", "index", "status")
SENTINEL_F, SENTINEL_I = -7.5, -77


def engine():
    if "net" not in _NETS:
        _NETS["net"] = load_pkg().NativeHRNet(32, 17, (64, 64), "fp32", max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    return _NETS["net"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def device_call(pred, rule, conf, iou, max_det=300, max_candidates=4096, agnostic=False, net=None):
    """the raw entry on a tensor that lies on the GPU, with outputs pre-filled with a sentinel: (rows, counts, index, status) as
    device tensors.  A refusal raises RuntimeError and leaves the tensors in `device_call.last`."""
    P = load_pkg("postproc")
    net = net or engine()
    B, N, C, dtype, code, flags, F = P.detector_nms_arguments(tuple(pred.shape), str(pred.dtype).replace("torch.", ""), rule, max_det,
                                                              max_candidates, agnostic)
    rows = torch.full((B, max(max_det, 1), F), SENTINEL_F, dtype=torch.float32, device="cuda")
    index = torch.full((B, max(max_det, 1)), SENTINEL_I, dtype=torch.int32, device="cuda")
    counts = torch.full((max(B, 1),), SENTINEL_I, dtype=torch.int32, device="cuda")
    status = torch.full((max(B, 1),), SENTINEL_I, dtype=torch.int32, device="cuda")
    device_call.last = (rows, counts, index, status)
    net._launch("hrn_detector_nms_dev", pred.data_ptr() if pred.numel() else None, dtype, B, N, C, code, flags, float(conf), float(iou),
                int(max_candidates), int(max_det), rows.data_ptr(), index.data_ptr(), counts.data_ptr(), status.data_ptr())
    return rows[:, :max_det], counts[:B], index[:, :max_det], status[:B]


def check(pred, rule, conf=0.25, iou=0.45, what="", **kw):
    """device == host on one case; returns the host results"""
    P = load_pkg("postproc")
    want = P.detector_nms(pred, rule, conf, iou, **kw)
    got = device_call(torch.from_numpy(np.ascontiguousarray(pred)).cuda(), rule, conf, iou, **kw)
    for name, g, w in zip(OUTPUTS, got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, name, int((bits(g) != bits(w)).sum()))
    return want


def with_candidates(rng, B, N, C, count, empty_image=None):
    """clustered rows of which exactly `count` per image pass the thresholds (image `empty_image`: none)"""
    pred = random_pred(rng, B, N, C, passing=1.0)
    for b in range(B):
        n = 0 if b == empty_image else count
        lose = rng.permutation(N)[n:]
        pred[b, lose, 4] = rng.uniform(0.0, 0.2, len(lose)).astype(np.float32)
    return pred


@pytest.mark.parametrize("C", [1, 2, 3, 80])
@pytest.mark.parametrize("rule", RULES)
def test_row_counts_around_a_wave_and_a_block(rule, C):
    rng = np.random.default_rng(100 + C)
    for N in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025):
        for B, empty in ((1, None), (4, 2)):
            pred = with_candidates(rng, B, N, C, (N + 1) // 2, empty)
            want = check(pred, rule, what=(N, B), agnostic=bool(N & 1))
            assert empty is None or want[1][empty] == 0
            # few take part: the selection path, and max_det below what survives
            want = check(pred, rule, what=(N, B, "select"), max_candidates=7, max_det=5)
            assert N < 16 or (want[3][0] & 1)


@pytest.mark.parametrize("rule", RULES)
def test_candidate_counts(rule):
    rng = np.random.default_rng(7)
    for N, C, count in ((1025, 3, 0), (1025, 3, 1), (1025, 80, 64), (1025, 2, 65), (1025, 3, 1024), (1025, 1, 1025), (257, 80, 257),
                        (64, 2, 64), (1, 1, 1)):
        want = check(with_candidates(rng, 2, N, C, count), rule, what=(N, C, count), max_det=300 if count >= 300 else max(count, 1))
        assert count == 0 or want[1][0] > 0


@pytest.mark.parametrize("rule", RULES)
def test_equal_keys_across_the_cut(rule):
    """200 rows qualify, 64 take part, and the keys come from eight values: the cut falls inside a run of equal keys, of which the
    lowest rows take part"""
    rng = np.random.default_rng(11)
    pred = with_candidates(rng, 2, 300, 2, 200, None)
    pred[..., 4] = np.where(pred[..., 4] > 0.25, np.round(pred[..., 4] * 8) / 8, pred[..., 4]).astype(np.float32)
    pred[..., 5:] = np.where(pred[..., 5:] > 0.5, 1.0, pred[..., 5:]).astype(np.float32)
    want = check(pred, rule, what="cut", max_candidates=64, max_det=64)
    assert (want[3] & 1).all()
    keys = pred[0, :, 4][pred[0, :, 4] > 0.25]
    assert np.sort(keys)[::-1][63] == np.sort(keys)[::-1][64]           # the cut does fall between equal keys
    check(pred, rule, what="cut, agnostic", max_candidates=64, max_det=10, agnostic=True)


@pytest.mark.parametrize("rule", RULES)
def test_all_of_5000_rows_qualify_and_4096_take_part(rule):
    pred = with_candidates(np.random.default_rng(13), 1, 5000, 2, 5000)
    want = check(pred, rule, what="5000", max_candidates=4096, max_det=300)
    assert want[3][0] & 1 and want[1][0] > 100


@pytest.mark.parametrize("shape", [(2, 10647, 85), (1, 25200, 85)])
@pytest.mark.parametrize("rule", RULES)
def test_head_sizes_of_the_reference_detectors(rule, shape):
    B, N, width = shape
    pred = with_candidates(np.random.default_rng(N), B, N, width - 5, 200)
    want = check(pred, rule, what=shape)
    assert (want[1] > 20).all() and (want[1] < 200).all() and not want[3].any()


@pytest.mark.parametrize("name", sorted(designed_cases()))
def test_designed_cases(name):
    pred, rule, conf, iou, max_det, max_candidates, agnostic = designed_cases()[name]
    check(pred, rule, conf, iou, what=name, max_det=max_det, max_candidates=max_candidates, agnostic=agnostic)


@pytest.mark.parametrize("rule", RULES)
def test_float16_input_equals_float32_input_of_the_converted_values(rule):
    rng = np.random.default_rng(5)
    pred = with_candidates(rng, 2, 700, 3, 150).astype(np.float16)
    pred[0, 0] = np.array([0x0001, 0x03FF, 0x0400, 0x7BFF, 0x3C00, 0xFC00, 0x7E00, 0x8000], np.uint16).view(np.float16)
    pred[1, 5, :4] = np.array([0x8001, 0x7C00, 0x7E00, 0x0002], np.uint16).view(np.float16)
    want = check(pred, rule, what="float16")
    got = device_call(torch.from_numpy(pred.astype(np.float32)).cuda(), rule, 0.25, 0.45)
    for name, g, w in zip(OUTPUTS, got, want):
        assert np.array_equal(bits(g.cpu().numpy()), bits(w)), name


def test_the_python_entry_a_side_stream_and_the_scratch():
    P = load_pkg("postproc")
    net = engine()
    rng = np.random.default_rng(17)
    small, large = with_candidates(rng, 1, 300, 3, 60), with_candidates(rng, 3, 2000, 80, 150)
    # NativeHRNet.detector_nms: a host array is uploaded, a device tensor used where it lies; everything comes back on the GPU
    for pred in (small, torch.from_numpy(large).cuda()):
        got = net.detector_nms(pred, "yolov5", 0.25, 0.45, max_det=100)
        want = P.detector_nms(pred.cpu().numpy() if isinstance(pred, torch.Tensor) else pred, "yolov5", 0.25, 0.45, max_det=100)
        assert all(t.is_cuda for t in got)
        for name, g, w in zip(OUTPUTS, got, want):
            assert np.array_equal(bits(g.cpu().numpy()), bits(w)), name
    # two calls on one handle reuse the scratch: large (it grows), small, large again -- and a call on a side stream in between
    check(large, "yolov3", what="large")
    check(small, "yolov3", what="small after large")
    side = torch.cuda.Stream()
    dev = torch.from_numpy(large).cuda()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = device_call(dev, "yolov3", 0.25, 0.45)
    again = device_call(dev, "yolov3", 0.25, 0.45)          # the default stream: waits for the side stream's call on the scratch
    side.synchronize()
    want = P.detector_nms(large, "yolov3", 0.25, 0.45)
    for name, g, a, w in zip(OUTPUTS, got, again, want):
        assert np.array_equal(bits(g.cpu().numpy()), bits(w)) and np.array_equal(bits(a.cpu().numpy()), bits(w)), name


def test_refusals_leave_the_sentinel_intact():
    rng = np.random.default_rng(19)
    pred = torch.from_numpy(with_candidates(rng, 2, 100, 3, 30)).cuda()
    for kw, text in ((dict(max_det=0), "max_det must be in"), (dict(max_det=65, max_candidates=64), "max_det must be in"),
                     (dict(max_candidates=4097), "max_candidates must be in"), (dict(conf=float("nan")), "must be finite"),
                     (dict(iou=float("inf")), "must be finite")):
        args = dict(conf=0.25, iou=0.45)
        args.update(kw)
        with pytest.raises(RuntimeError, match=text):
            device_call(pred, "yolov5", args.pop("conf"), args.pop("iou"), **args)
        torch.cuda.synchronize()
        rows, counts, index, status = device_call.last
        assert (rows == SENTINEL_F).all() and all((t == SENTINEL_I).all() for t in (counts, index, status)), kw
    with pytest.raises(ValueError, match="rule must be"):
        engine().detector_nms(pred, "yolov4", 0.25, 0.45)
    with pytest.raises(ValueError, match="float32 or float16"):
        device_call(pred.to(torch.bfloat16), "yolov5", 0.25, 0.45)


# ------------------------------------------------------------------------------------- SimpleHRNet(device_detector=<predict_raw>)
def raw_head(seed, people, N=160, C=3):
    """the raw output of a fake head for one 64 x 64 letterboxed frame: `people` clusters of candidates whose boxes lie inside the
    picture area of a 120 x 160 frame (rows 8 .. 56), most of class 0; every other row has a low obj"""
    rng = np.random.default_rng(seed)
    out = np.zeros((N, 5 + C), np.float32)
    out[:, 0:2] = rng.uniform(10, 54, (N, 2))
    out[:, 2:4] = rng.uniform(4, 12, (N, 2))
    out[:, 4] = rng.uniform(0.0, 0.2, N)
    out[:, 5:] = rng.uniform(0.0, 0.3, (N, C))
    rows = rng.permutation(N)[:people * 5].reshape(people, 5) if people else np.zeros((0, 5), int)
    for k, members in enumerate(rows):
        centre, size = rng.uniform((16, 22), (48, 42)), rng.uniform(8, 18, 2)
        out[members, 0:2] = centre + rng.normal(0, 0.4, (5, 2))
        out[members, 2:4] = size * rng.uniform(0.95, 1.05, (5, 2))
        out[members, 4] = rng.uniform(0.6, 1.0, 5)
        out[members, 5 + (k % 4 == 3)] = rng.uniform(0.8, 1.0, 5)        # every fourth cluster is of class 1: filtered afterwards
    return out.astype(np.float32)


class Head:
    """a fake detector network: the raw (n, N, 5 + C) tensor of the frames it is asked about, on the device"""
    size, conf_thres, classes, nms_thres, max_det = 64, 0.25, [0], 0.45, 20

    def __init__(self, style, table):
        self.style, self.table, self.frame_number, self.calls = style, table, 0, 0

    def raw(self, x):
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape[1:]) == (3, 64, 64)
        self.calls += 1
        return torch.from_numpy(np.stack([self.table[self.frame_number + k] for k in range(x.shape[0])])).cuda()


class RawDetector(Head):
    """a detector that stops at its head: the NMS is left to the GPU"""

    def predict_raw(self, x):
        return self.raw(x)


class HostNmsDetector(Head):
    """the same head with its NMS on the host: downloads the raw tensor, runs postproc.detector_nms, uploads per-image rows"""

    def predict_tensor(self, x):
        P = load_pkg("postproc")
        rows, counts, _, _ = P.detector_nms(self.raw(x).cpu().numpy(), self.style, self.conf_thres, self.nms_thres, max_det=self.max_det)
        return [torch.from_numpy(rows[k, :counts[k]].copy()).cuda() for k in range(len(rows))]


@pytest.mark.parametrize("style", RULES)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_simple_hrnet_raw_detector_equals_the_host_nms(dtype, style):
    pkg = load_pkg()
    hf, wf = 120, 160
    frames = [np.random.default_rng(40 + k).integers(0, 256, (hf, wf, 3), dtype=np.uint8) for k in range(4)]
    table = {k: raw_head(60 + k, (5, 3, 4, 0)[k]) for k in range(4)}             # the head finds nobody on the last frame
    kw = dict(resolution=(64, 96), multiperson=True, return_heatmaps=True, return_bounding_boxes=True, device="cuda:0", dtype=dtype)
    sd = state_dict_np(32, 0)
    raw, ref = RawDetector(style, table), HostNmsDetector(style, table)
    assert not hasattr(raw, "predict_tensor") and not hasattr(ref, "predict_raw")
    dev, host = pkg.SimpleHRNet(32, 17, sd, device_detector=raw, **kw), pkg.SimpleHRNet(32, 17, sd, device_detector=ref, **kw)

    def equal(got, want):                      # heat-maps, boxes, joints
        assert len(got) == len(want)
        for a, b in zip(got, want):
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))

    for k in range(4):                                                            # single images
        raw.frame_number = ref.frame_number = k
        got, want = dev.predict(frames[k]), host.predict(frames[k])
        equal(got, want)
        assert len(want[2]) == (0 if k == 3 else len(want[1])) and (k == 3 or 0 < len(want[2]) <= (5, 3, 4)[k])
    for lo, hi in ((0, 2), (2, 4)):                                               # a stack of two, and one with the empty frame
        raw.frame_number = ref.frame_number = lo
        got, want = dev.predict(np.stack(frames[lo:hi])), host.predict(np.stack(frames[lo:hi]))
        for a, b in zip(got, want):
            assert len(a) == len(b) == 2
            equal(a, b)
    # redetect_every = 3: the detector on calls 0 and 3, tracking in between
    dev3 = pkg.SimpleHRNet(32, 17, sd, device_detector=raw, redetect_every=3, **kw)
    host3 = pkg.SimpleHRNet(32, 17, sd, device_detector=ref, redetect_every=3, **kw)
    seen = raw.calls
    for k in (0, 1, 2, 1):
        raw.frame_number = ref.frame_number = k
        equal(dev3.predict(frames[k]), host3.predict(frames[k]))
    assert raw.calls == seen + 2
