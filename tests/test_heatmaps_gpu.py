"""Heat-map overlays on the GPU: ``NativeHRNet.draw_heatmaps`` against the numpy restatement of the definition
(tests/heat_ref.py) -- whole buffers, byte for byte, on frames of random bytes with guard bytes in the pitch, so that a stray
write shows."""
import json
import os

import numpy as np
import pytest
import torch

import draw_ref
import heat_cases
import heat_ref
import yuv_ref
from conftest import GOLDEN, load_pkg, state_dict_np
from heat_cases import F32, noise

pytestmark = pytest.mark.gpu

COCO = json.load(open(os.path.join(GOLDEN, "coco_skeleton.json")))["coco_skeleton"]
FORMATS = [("bgr", None), ("nv12", ("bt601", "limited")), ("i420", ("bt709", "full"))]
GUARD = 26      # bytes of pitch beyond a row
MODES = ("const", "value")


@pytest.fixture(scope="module")
def net():
    n = load_pkg().NativeHRNet(32, 17, (64, 96), "fp32", max_batch=4, device=0)
    yield n
    n.close()


class Canvas:
    """a noise canvas of one format on the device, guard bytes behind every row: `frame` is what the engine draws into,
    `download()` every byte of the buffer, `expected(...)` the restatement's drawing on a host copy"""

    def __init__(self, fmt_key, h, w, seed):
        pkg = load_pkg()
        self.fmt, self.key = fmt_key
        self.h, self.w = h, w
        if self.fmt == "bgr":
            self.before = noise((h, w + 9, 3), seed)
            self.dev = torch.from_numpy(self.before.copy()).cuda()
            self.frame = self.dev[:, :w]                        # a column-sliced view: the rows are pitched
        else:
            self.pitch = w + GUARD
            self.before = noise(yuv_ref.nbytes(h, w, self.pitch), seed)
            self.dev = torch.from_numpy(self.before.copy()).cuda()
            self.frame = pkg.YuvFrame(self.dev, h, w, self.fmt, self.key[0], self.key[1], self.pitch)

    def table(self, bgr_table):
        return bgr_table if self.key is None else load_pkg().bgr_to_yuv_colors(bgr_table, *self.key)

    def download(self):
        return self.dev.cpu().numpy()

    def expected(self, maps, boxes, bgr_table, **kw):
        want = self.before.copy()
        if self.fmt == "bgr":
            heat_ref.draw_bgr(want[:, :self.w], maps, boxes, self.table(bgr_table), **kw)
        else:
            heat_ref.draw_yuv(want, self.h, self.w, self.fmt, maps, boxes, self.table(bgr_table), pitch=self.pitch, **kw)
        return want


def check(net, fmt_key, h, w, maps, boxes, mask=None, setting=(153, 1, 26), seed=0, lo=0.0, hi=1.0, table=None, device_boxes=True):
    """draws on the GPU and in numpy; returns (buffer before, buffer after), the two having been held equal"""
    alpha, mode, cutoff = setting
    c = Canvas(fmt_key, h, w, seed)
    table = heat_ref.jet() if table is None else table
    joints = None if mask is None else [j for j, m in enumerate(mask) if m]
    given = torch.from_numpy(np.ascontiguousarray(boxes, np.int32)).cuda() if device_boxes else np.asarray(boxes, np.int32)
    out = net.draw_heatmaps(c.frame, torch.from_numpy(np.ascontiguousarray(maps, F32)).cuda(), given, joints=joints, colormap=table, alpha=alpha,
                            alpha_mode=MODES[mode], vmin=lo, vmax=hi, cutoff=cutoff)
    assert out is c.frame or (c.fmt == "bgr" and out.data_ptr() == c.frame.data_ptr())
    want = c.expected(maps, boxes, table, mask=mask, lo=lo, hi=hi, alpha=alpha, mode=mode, cutoff=cutoff)
    got = c.download()
    np.testing.assert_array_equal(got, want, err_msg=str((fmt_key, h, w, setting)))
    return c.before, got


@pytest.mark.parametrize("fmt_key", FORMATS, ids=[f[0] for f in FORMATS])
def test_the_matrix_equals_the_restatement(net, fmt_key):
    changed = 0
    for k, (name, h, w, maps, boxes, mask, setting, unchanged) in enumerate(heat_cases.matrix()):
        before, after = check(net, fmt_key, h, w, maps, boxes, mask, setting, seed=k)
        if unchanged:
            np.testing.assert_array_equal(before, after, err_msg=name)
        else:
            changed += int((before != after).any())
    assert changed >= len(heat_cases.matrix()) // 2
    # two people overlapping: both call orders give equal bytes
    maps, boxes = heat_cases.random_maps(2, 16, 12, 5), heat_cases.OVERLAPPING
    _, one = check(net, fmt_key, 46, 70, maps, boxes, seed=1)
    _, other = check(net, fmt_key, 46, 70, maps[::-1], boxes[::-1], seed=1)
    np.testing.assert_array_equal(one, other)
    for setting in ((0, 0, 1), (0, 1, 1)):              # alpha 0: nothing is written
        before, after = check(net, fmt_key, 46, 70, maps, boxes, setting=setting, seed=2)
        np.testing.assert_array_equal(before, after)
    check(net, fmt_key, 46, 70, maps, boxes, setting=(200, 0, 255), seed=3)
    check(net, fmt_key, 46, 70, maps, boxes, setting=(1, 1, 1), seed=4, lo=-0.3, hi=0.9, table=load_pkg().heat_colormap("hot"))


@pytest.mark.parametrize("lo,hi", heat_cases.RANGES)
def test_the_quantiser_at_its_edges_equals_the_host(net, lo, hi):
    """CONST mode, alpha 255, a gray table, a box of exactly one pixel per cell: a written pixel IS the device's Q"""
    post = load_pkg("postproc")
    vector = heat_cases.quantise_maps(lo, hi)              # (2, 3, 1, L)
    L = vector.shape[-1]
    wq = 8
    hq = -(-L // wq)
    maps = np.full((2, 3, hq * wq), np.nan, F32)
    maps[:, :, :L] = vector[:, :, 0]
    maps = maps.reshape(2, 3, hq, wq)
    Q = post.heatmap_quantise(maps, vmin=lo, vmax=hi)
    np.testing.assert_array_equal(Q, heat_ref.quantise(maps, None, lo, hi))
    boxes = np.asarray([[3, 2, 3 + wq, 2 + hq], [29, 27, 29 + wq, 27 + hq]], np.int32)      # the second across the tile borders
    for mask in (None, [1, 0, 0], [1, 0, 1]):
        Qm = post.heatmap_quantise(maps, joints=None if mask is None else [j for j, m in enumerate(mask) if m], vmin=lo, vmax=hi)
        before, after = check(net, ("bgr", None), 46, 70, maps, boxes, mask, (255, 0, 1), seed=5, lo=lo, hi=hi, table=heat_ref.gray())
        for (x1, y1, _, _), q in zip(boxes, Qm):
            seen = after[y1:y1 + hq, x1:x1 + wq]
            want = np.where((q >= 1)[..., None], q[..., None], before[y1:y1 + hq, x1:x1 + wq])
            np.testing.assert_array_equal(seen, want)
    assert {0, 1, 2, 127, 128, 253, 254, 255} <= set(Q[0].reshape(-1).tolist())


def test_more_people_than_one_cull_chunk(net):
    """300 people with 6 x 6 boxes and one box over everything: scattered over the canvas, then all on one tile, where the 301
    survivors make two chunks; the large box first and last"""
    rng = np.random.default_rng(3)
    n = 300
    maps = heat_cases.random_maps(n + 1, 5, 4, 6)
    for spread, fmt_key in (((46 - 6, 70 - 6), FORMATS[0]), ((26, 26), FORMATS[0]), ((26, 26), FORMATS[1])):
        x1, y1 = rng.integers(0, spread[1], n), rng.integers(0, spread[0], n)
        small = np.stack([x1, y1, x1 + 6, y1 + 6], 1).astype(np.int32)
        if spread == (26, 26):
            assert (small[:, 2] <= 32).all() and (small[:, 3] <= 32).all()          # everybody is on tile (0, 0)
        everything = np.asarray([[-30, -20, 90, 60]], np.int32)
        check(net, fmt_key, 46, 70, maps, np.concatenate([small, everything]), setting=(200, 0, 1), seed=7)
        check(net, fmt_key, 46, 70, maps, np.concatenate([everything, small]), setting=(153, 1, 26), seed=8)
    # only people of the second chunk show: the first 256 have nothing to say
    quiet = maps.copy()
    quiet[:256] = -1.0
    before, after = check(net, FORMATS[0], 46, 70, quiet[:n], small, setting=(255, 0, 1), seed=9)
    assert (before != after).any()


def test_boxes_from_device_memory_and_from_numpy(net):
    maps, boxes = heat_cases.random_maps(13, 16, 12, 11), heat_cases.drawn_boxes(46, 70, 16, 12)
    for fmt_key in FORMATS:
        _, a = check(net, fmt_key, 46, 70, maps, boxes, seed=10, device_boxes=True)
        _, b = check(net, fmt_key, 46, 70, maps, boxes, seed=10, device_boxes=False)
        np.testing.assert_array_equal(a, b)


def test_pitched_views_keep_their_guard_bytes(net):
    big = noise((50, 100, 3), 7)
    dev = torch.from_numpy(big.copy()).cuda()
    maps, boxes = heat_cases.random_maps(2, 16, 12, 12), np.asarray([[-3, 12, 40, 38], [30, 3, 75, 45]], np.int32)
    out = net.draw_heatmaps(dev[5:45, 10:80], maps, boxes, alpha=200, alpha_mode="const", cutoff=1)
    assert out.data_ptr() == dev[5:45, 10:80].data_ptr()
    want = big.copy()
    heat_ref.draw_bgr(want[5:45, 10:80], maps, boxes, heat_ref.jet(), alpha=200, mode=0, cutoff=1)
    np.testing.assert_array_equal(dev.cpu().numpy(), want)
    assert (want != big).any() and (want[:5] == big[:5]).all() and (want[:, :10] == big[:, :10]).all() and (want[:, 80:] == big[:, 80:]).all()
    host = net.draw_heatmaps(big[5:45, 10:80], maps, boxes, alpha=200, alpha_mode="const", cutoff=1)       # a host frame is uploaded
    np.testing.assert_array_equal(host.cpu().numpy(), want[5:45, 10:80])
    # a padded Y / UV pitch: Canvas has GUARD bytes behind every row of every plane (the matrix runs on it; once more, by plane)
    for fmt_key in FORMATS[1:]:
        before, after = check(net, fmt_key, 46, 70, maps, boxes, setting=(200, 0, 1), seed=13)
        pitch = 70 + GUARD
        rows = after[:pitch * 46].reshape(46, pitch)
        np.testing.assert_array_equal(rows[:, 70:], before[:pitch * 46].reshape(46, pitch)[:, 70:])
        assert (rows[:, :70] != before[:pitch * 46].reshape(46, pitch)[:, :70]).any()


def test_nobody_and_a_canvas_nobody_refers_to(net):
    before = noise((46, 70, 3), 2)
    dev = torch.from_numpy(before.copy()).cuda()
    assert net.draw_heatmaps(dev, np.zeros((0, 3, 5, 4), F32), np.zeros((0, 4), np.int32)) is dev             # n == 0
    other = torch.from_numpy(before.copy()).cuda()
    maps, boxes = heat_cases.random_maps(2, 5, 4, 14), heat_cases.OVERLAPPING
    out = net.draw_heatmaps([dev, None, other], maps, boxes, frame_index=[2, 2])
    assert out[0] is dev and out[1] is None and out[2] is other
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.cpu().numpy(), before)
    np.testing.assert_array_equal(other.cpu().numpy(), heat_ref.draw_bgr(before.copy(), maps, boxes, heat_ref.jet()))
    # two canvases of different sizes
    sizes = [(46, 70), (70, 100)]
    frames = [noise(s + (3,), 30 + k) for k, s in enumerate(sizes)]
    devs = [torch.from_numpy(f.copy()).cuda() for f in frames]
    maps, index = heat_cases.random_maps(5, 16, 12, 15), np.asarray([1, 0, 1, 1, 0], np.int32)
    boxes = np.asarray([[5, 5, 60, 60], [-4, 3, 30, 44], [50, 20, 120, 80], [40, 30, 70, 50], [33, 10, 69, 40]], np.int32)
    net.draw_heatmaps(devs, maps, boxes, frame_index=index, colormap="hot", alpha=1.0, alpha_mode="value", cutoff=1)
    want = heat_ref.draw_clip([f.copy() for f in frames], maps, boxes, index, load_pkg().heat_colormap("hot"), alpha=255, mode=1, cutoff=1)
    for d, w in zip(devs, want):
        np.testing.assert_array_equal(d.cpu().numpy(), w)
    for kw, text in ((dict(cutoff=0), "cutoff must be in"), (dict(vmin=1.0, vmax=1.0), "hi must be above lo")):
        with pytest.raises((ValueError, RuntimeError), match=text):
            net.draw_heatmaps(dev, maps[:2], boxes[:2], **kw)
    with pytest.raises(RuntimeError, match="is null"):
        net.draw_heatmaps([dev, None], maps[:1], boxes[:1], frame_index=[1])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.cpu().numpy(), before)


def test_a_joint_subset_equals_the_maps_reduced_by_hand(net):
    maps = heat_cases.random_maps(3, 16, 12, 16, joints=17)
    boxes = np.asarray([[2, 3, 50, 40], [30, 10, 69, 45], [-5, 20, 20, 60]], np.int32)
    subset = [0, 5, 9, 16]
    mask = [int(j in subset) for j in range(17)]
    part = maps[:, subset]
    by_hand = np.where(np.isnan(part).all(1), np.nan, np.nanmax(np.where(np.isnan(part), -np.inf, part), 1)).astype(F32)[:, None]
    _, a = check(net, FORMATS[0], 46, 70, maps, boxes, mask, seed=17)
    _, b = check(net, FORMATS[0], 46, 70, by_hand, boxes, None, seed=17)
    np.testing.assert_array_equal(a, b)
    _, c = check(net, FORMATS[0], 46, 70, maps, boxes, None, seed=17)
    assert (a != c).any()                               # the other joints do have something to say


def test_predict_frame_to_heatmaps_to_poses(net):
    """the documented chain on a synthetic checkpoint: the bytes outside every box are unchanged, and the result equals the
    restatements fed the same maps, boxes and joints"""
    pkg = load_pkg()
    net.load_state_dict(state_dict_np(32, 0))
    before = noise((120, 160, 3), 18)
    dets = np.asarray([[10.2, 8.7, 90.4, 100.1], [60.5, 20.5, 150.0, 70.0]], np.float32)
    frame = torch.from_numpy(before.copy()).cuda()
    boxes, pts, maps = net.predict_frame(frame, dets, return_heatmaps=True)
    assert maps.is_cuda and tuple(maps.shape) == (2, 17, 16, 24) and np.array_equal(frame.cpu().numpy(), before)
    h_maps = maps.cpu().numpy()
    lo, hi = float(h_maps.min()), float(h_maps.max())      # synthetic weights: the maps are no probabilities
    assert np.isfinite([lo, hi]).all() and hi > lo
    net.draw_heatmaps(frame, maps, boxes, vmin=lo, vmax=hi, alpha=0.8, cutoff=0.3)
    heat = frame.cpu().numpy()
    want = heat_ref.draw_bgr(before.copy(), h_maps, boxes, heat_ref.jet(), lo=lo, hi=hi, alpha=204, mode=1, cutoff=76)
    np.testing.assert_array_equal(heat, want)
    outside = np.ones((120, 160), bool)
    for x1, y1, x2, y2 in boxes:
        outside[max(y1, 0):max(y2, 0), max(x1, 0):max(x2, 0)] = False
    assert outside.any() and (heat[outside] == before[outside]).all() and (heat != before).any()
    net.draw_poses(frame, pts, COCO, confidence_threshold=-1.0)
    want = draw_ref.draw_bgr(want, pts.cpu().numpy(), COCO, pkg.palette("tab20", 16), pkg.palette("Set2", 8), threshold=-1.0)
    np.testing.assert_array_equal(frame.cpu().numpy(), want)


def test_two_streams_from_one_handle_equal_serial_calls(net):
    """the call scratch (table and Q) is the handle's: a call on another stream waits for the one before"""
    cases = []
    for k in range(2):
        maps, boxes = heat_cases.random_maps(13, 16, 12, 20 + k), heat_cases.drawn_boxes(70, 100, 16, 12)
        before = noise((70, 100, 3), 22 + k)
        cases.append((torch.from_numpy(maps).cuda(), torch.from_numpy(boxes).cuda(), before,
                      heat_ref.draw_bgr(before.copy(), maps, boxes, heat_ref.jet(), alpha=200, mode=k, cutoff=10)))
    serial = [torch.from_numpy(c[2].copy()).cuda() for c in cases]
    for k, (maps, boxes, _, _) in enumerate(cases):
        net.draw_heatmaps(serial[k], maps, boxes, alpha=200, alpha_mode=MODES[k], cutoff=10)
    torch.cuda.synchronize()
    frames = [torch.from_numpy(c[2].copy()).cuda() for c in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for rounds in range(3):
        for k, (maps, boxes, before, _) in enumerate(cases):
            streams[k].wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(streams[k]):
                if rounds:
                    frames[k].copy_(torch.from_numpy(before), non_blocking=False)
                net.draw_heatmaps(frames[k], maps, boxes, alpha=200, alpha_mode=MODES[k], cutoff=10)
    for s in streams:
        s.synchronize()
    for k, (_, _, _, want) in enumerate(cases):
        np.testing.assert_array_equal(frames[k].cpu().numpy(), want, err_msg="stream %d" % k)
        np.testing.assert_array_equal(serial[k].cpu().numpy(), want, err_msg="serial %d" % k)
