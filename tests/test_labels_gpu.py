"""Person labels on the GPU: ``NativeHRNet.draw_labels`` against the numpy restatement of the definition (tests/label_ref.py) --
whole buffers, byte for byte, on frames of random bytes so that a stray write shows."""
import json
import os

import numpy as np
import pytest
import torch

import draw_ref
import label_ref
import yuv_ref
from conftest import GOLDEN, load_pkg

pytestmark = pytest.mark.gpu

COCO = json.load(open(os.path.join(GOLDEN, "coco_skeleton.json")))["coco_skeleton"]
# colours of the tests' own: three, so that the modulo is exercised; every text colour differs from every plate colour
CO = np.asarray([[250, 10, 20], [30, 240, 40], [50, 60, 230]], np.uint8)
TX = np.asarray([[0, 0, 0], [255, 255, 255], [7, 200, 90]], np.uint8)


@pytest.fixture(scope="module")
def net():
    n = load_pkg().NativeHRNet(32, 17, (64, 96), "fp32", max_batch=4, device=0)
    yield n
    n.close()


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def check_bgr(net, h, w, boxes, seed=0, **kw):
    """draws on the GPU and in numpy; returns (frame before, frame after), the two having been held equal"""
    before = noise((h, w, 3), seed)
    boxes = np.asarray(boxes, np.int32).reshape(-1, 4)
    dev = torch.from_numpy(before.copy()).cuda()
    out = net.draw_labels(dev, boxes, palette=CO, text_colors=TX, **kw)
    assert out is dev
    want = label_ref.draw_bgr(before.copy(), boxes, CO, TX, person_ids=kw.get("person_ids"), scores=kw.get("scores"),
                              scale=kw.get("scale"), thickness=kw.get("thickness", 2))
    got = dev.cpu().numpy()
    np.testing.assert_array_equal(got, want, err_msg=str((h, w, kw)))
    return before, got


@pytest.mark.parametrize("h,w", [(45, 70), (70, 100)])
def test_single_labels_across_the_tile_borders(net, h, w):
    native = load_pkg("native")
    t = native.DRAW_TILE
    assert t < h and 2 * t < w and w % t and h % t                  # tile borders on both axes, the last tile partial
    for k, (s, T) in enumerate([(1, 2), (2, 1), (1, 0), (3, 3)]):
        # the plate (19 s wide for three cells, 9 s high) and its digits across x = 31 | 32 and y = 31 | 32
        x1, y1 = t - 8 * s, t + 4 * s
        before, after = check_bgr(net, h, w, [x1, y1, x1 + 30, y1 + 9], seed=k, person_ids=[407], scale=s, thickness=T)
        assert (after[y1 - 9 * s, x1] == CO[407 % 3]).all() and (before != after).any()
        assert ((after[y1 - 9 * s:y1, x1:x1 + 19 * s] == TX[407 % 3]).all(-1)).sum() >= 20 * s * s      # the ink is there, on both sides
        assert ((after[y1 - 9 * s:y1, x1:t] == TX[407 % 3]).all(-1)).any() and ((after[y1 - 9 * s:y1, t:] == TX[407 % 3]).all(-1)).any()
        check_bgr(net, h, w, [x1, y1, w + 40, h + 40], seed=k, person_ids=[5], scores=[0.87], scale=s, thickness=T)
    check_bgr(net, h, w, [0, 0, w - 1, h - 1], person_ids=[12], scores=[0.5])           # the frame's own rectangle: the plate inside
    check_bgr(net, h, w, [-20, -30, w + 20, h + 30], person_ids=[12], thickness=16)     # larger than the frame
    before, after = check_bgr(net, h, w, [-20, -30, w + 20, h + 30], thickness=3)       # ... its outline and (no text) nothing else: unchanged
    np.testing.assert_array_equal(before, after)
    for box in ([-60, 5, -30, 30], [w + 2, 5, w + 40, 30], [5, h + 12, 30, h + 50], [0, 0, 0, 0], [30, 10, 30, 40], [40, 10, 30, 40],
                [-8193, 0, 40, 40], [0, 0, 16384, 40]):
        before, after = check_bgr(net, h, w, box, person_ids=[3], scores=[0.4])         # fully outside, empty, degenerate, out of range
        np.testing.assert_array_equal(before, after, err_msg=str(box))
    check_bgr(net, h, w, [-8192, -8192, 16383, 16383], person_ids=[1], thickness=16)
    check_bgr(net, h, w, [w - 5, h - 4, 16383, 16383], person_ids=[2147483647], scores=[1.0], scale=1)
    check_bgr(net, h, w, [-8192, 12, 9, 40], person_ids=[88], scores=[np.nan])


def test_ids_scores_and_fields(net):
    h, w = 45, 70
    ids = [0, 7, 10, 99, 100, 2147483647, -1]
    scores = np.asarray([np.nan, -0.5, 0.0, np.nextafter(np.float32(0.005), np.float32(-1)), 0.005, 0.995, 7.0], np.float32)
    boxes = [[2, 10 + 5 * k, 60, 44] for k in range(len(ids))]
    check_bgr(net, 70, 100, boxes, person_ids=ids, scores=scores, thickness=1)
    check_bgr(net, 70, 100, boxes, person_ids=ids, thickness=1)
    check_bgr(net, 70, 100, boxes, scores=scores, thickness=1)
    check_bgr(net, 70, 100, boxes, thickness=1)
    for k in range(len(ids)):
        check_bgr(net, h, w, boxes[k], seed=k, person_ids=ids[k:k + 1], scores=scores[k:k + 1])
    # a box narrower than 2 T is filled
    before, after = check_bgr(net, h, w, [30, 12, 33, 40], thickness=2)
    assert (after[12:41, 30:34] == CO[0]).all()


def test_later_people_lie_over_earlier_ones(net):
    # three people whose plates, ink and outlines overlap; the colours tell who lies on top
    boxes = [[10, 20, 50, 40], [14, 24, 60, 44], [30, 21, 45, 30]]
    before, after = check_bgr(net, 45, 70, boxes, person_ids=[8, 18, 88], thickness=2)
    number, _ = label_ref.paint(45, 70, boxes, CO, TX, person_ids=[8, 18, 88])
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8} == set(np.unique(number[number >= 0]).tolist())      # every primitive of every person shows somewhere
    assert number[16, 14] == 4 and number[20, 20] == 4 and number[25, 30] == 6              # plate 1 over ink 0 and outline 0; outline 2 over outline 1
    assert (after[12, 30] == CO[88 % 3]).all() and (after[11, 10] == CO[8 % 3]).all()
    check_bgr(net, 45, 70, boxes[::-1], person_ids=[88, 18, 8], scores=[0.1, 0.2, 0.3], thickness=3, scale=2)


def test_300_people_on_one_tile(net):
    """more than one cull chunk of 256: the people of the second chunk (the early ones) show wherever the later ones left pixels
    free, and nobody is lost"""
    native = load_pkg("native")
    t = native.DRAW_TILE
    rng = np.random.default_rng(3)
    n = 300
    x1, y1 = rng.integers(t - 20, 2 * t - 2, n), rng.integers(t - 6, 2 * t - 2, n)
    boxes = np.stack([x1, y1, x1 + rng.integers(21, 50, n), y1 + rng.integers(7, 30, n)], 1).astype(np.int32)
    assert ((boxes[:, 0] < 2 * t) & (boxes[:, 2] >= t) & (boxes[:, 1] < 2 * t) & (boxes[:, 3] >= t)).all()     # everybody meets tile (1, 1)
    ids = rng.integers(-5, 1000, n).astype(np.int32)
    before, after = check_bgr(net, 97, 131, boxes, seed=1, person_ids=ids, thickness=1)
    early, _ = label_ref.paint(97, 131, boxes[:n - 256], CO, TX, person_ids=ids[:n - 256], thickness=1)
    late, _ = label_ref.paint(97, 131, boxes[n - 256:], CO, TX, person_ids=ids[n - 256:], thickness=1)
    assert ((early >= 0) & (late < 0)).sum() > 20
    check_bgr(net, 97, 131, boxes, seed=2, scores=rng.uniform(0, 1, n).astype(np.float32), thickness=0)
    only_early = boxes.copy()
    only_early[40:] = 0                                                       # only people of the second chunk are drawn
    check_bgr(net, 97, 131, only_early, seed=3, person_ids=ids)


def test_pitched_view(net):
    big = noise((50, 100, 3), 7)
    dev = torch.from_numpy(big.copy()).cuda()
    boxes = np.asarray([[-3, 12, 40, 38], [30, 3, 75, 45]], np.int32)
    out = net.draw_labels(dev[5:45, 10:80], boxes, person_ids=[4, 21], scores=[0.33, 0.9], palette=CO, text_colors=TX, thickness=3)
    assert out.data_ptr() == dev[5:45, 10:80].data_ptr()
    want = big.copy()
    label_ref.draw_bgr(want[5:45, 10:80], boxes, CO, TX, person_ids=[4, 21], scores=[0.33, 0.9], thickness=3)
    np.testing.assert_array_equal(dev.cpu().numpy(), want)
    assert (want != big).any() and (want[:5] == big[:5]).all() and (want[:, :10] == big[:, :10]).all() and (want[:, 80:] == big[:, 80:]).all()
    host = net.draw_labels(big[5:45, 10:80], boxes, person_ids=[4, 21], scores=[0.33, 0.9], palette=CO, text_colors=TX, thickness=3)
    np.testing.assert_array_equal(host.cpu().numpy(), want[5:45, 10:80])


@pytest.mark.parametrize("fmt,key", [("nv12", ("bt601", "limited")), ("i420", ("bt709", "full"))])
def test_yuv_canvases(net, fmt, key):
    pkg = load_pkg()
    h, w, pitch = 46, 70, 96
    co, tx = pkg.bgr_to_yuv_colors(CO, *key), pkg.bgr_to_yuv_colors(TX, *key)
    # odd corners, so that outlines, plates and ink share 2 x 2 blocks with each other and with untouched pixels
    boxes = np.asarray([[7, 13, 41, 35], [33, 11, 69, 45], [-5, 31, 20, 60]], np.int32)
    ids, scores = [3, 14, 159], np.asarray([0.26, 0.5, 0.99], np.float32)
    for T, s in ((1, 1), (2, 1), (3, 2)):
        data = noise(yuv_ref.nbytes(h, w, pitch), 40 + T)
        frame = pkg.YuvFrame(torch.from_numpy(data.copy()).cuda(), h, w, fmt, key[0], key[1], pitch)
        out = net.draw_labels(frame, boxes, person_ids=ids, scores=scores, palette=CO, text_colors=TX, scale=s, thickness=T)
        assert out is frame
        want = label_ref.draw_yuv(data.copy(), h, w, fmt, boxes, co, tx, pitch=pitch, person_ids=ids, scores=scores, scale=s, thickness=T)
        got = frame.data.cpu().numpy()
        for name, a, b in zip("YUV", yuv_ref.planes(got, h, w, fmt, pitch), yuv_ref.planes(want, h, w, fmt, pitch)):
            np.testing.assert_array_equal(a, b, err_msg="%s plane %s" % (name, (fmt, T, s)))
        np.testing.assert_array_equal(got, want, err_msg="pitch bytes %s" % ((fmt, T, s),))
        assert (got != data).any()
        number, _ = label_ref.paint(h, w, boxes, CO, TX, person_ids=ids, scores=scores, scale=s, thickness=T)
        blocks = number.reshape(h // 2, 2, w // 2, 2)
        drawn = np.where(blocks >= 0, blocks, blocks.max() + 1)
        assert (drawn.min((1, 3)) < blocks.max((1, 3))).any()          # two primitives among one block's covered pixels
        assert ((blocks.max((1, 3)) >= 0) & (blocks.min((1, 3)) < 0)).any()      # ... and a block only partly covered


def test_clip_mode_and_the_scale_rule(net):
    sizes = [(720, 724), (161, 200), None, (720, 96)]
    assert [label_ref.default_scale(*s) for s in sizes if s] == [2, 1, 1] and label_ref.default_scale(8192, 8192) == 16
    rng = np.random.default_rng(11)
    frame_index = rng.permutation(np.repeat([0, 1, 3], [5, 3, 4])).astype(np.int32)
    n = len(frame_index)
    boxes = np.empty((n, 4), np.int32)
    for i, f in enumerate(frame_index):
        hh, ww = sizes[f]
        boxes[i, :2] = rng.integers(-10, ww - 20), rng.integers(-10, hh - 20)
        boxes[i, 2:] = boxes[i, :2] + rng.integers(5, 150, 2)
    ids, scores = rng.integers(0, 3000, n).astype(np.int32), rng.uniform(0, 1, n).astype(np.float32)
    before = [None if s is None else noise(s + (3,), 20 + k) for k, s in enumerate(sizes)]
    for kw in (dict(person_ids=ids, scores=scores), dict(scores=scores), dict(person_ids=ids, scale=3)):
        dev = [None if b is None else torch.from_numpy(b.copy()).cuda() for b in before]
        given = {k: torch.from_numpy(v).cuda() if k != "scale" else v for k, v in kw.items()}
        out = net.draw_labels(dev, torch.from_numpy(boxes).cuda(), frame_index=frame_index, palette=CO, text_colors=TX, **given)
        assert out[2] is None and all(o is d for o, d in zip(out, dev))
        want = label_ref.draw_clip([None if b is None else b.copy() for b in before], boxes, frame_index, CO, TX, **kw)
        for f, s in enumerate(sizes):
            if s is not None:
                np.testing.assert_array_equal(dev[f].cpu().numpy(), want[f], err_msg="frame %d %s" % (f, list(kw)))
    with pytest.raises(ValueError, match="frame_index"):
        net.draw_labels(dev, boxes)
    with pytest.raises(RuntimeError, match="is null"):
        net.draw_labels(dev, boxes[:1], frame_index=[2])


def test_tracker_state_is_labelled_where_it_lies(net):
    """two designed frames through PersonTracker.update on the device; its boxes and ids, never downloaded, go to draw_poses and
    draw_labels; the result is draw_ref followed by label_ref on the downloaded state"""
    pkg = load_pkg()
    rng = np.random.default_rng(4)

    def people(boxes):
        pts = np.empty((len(boxes), 17, 3), np.float32)
        for i, (x1, y1, x2, y2) in enumerate(boxes):
            shape = np.random.default_rng(50).uniform(0.1, 0.9, (17, 2))          # everybody strikes the same pose in their box
            pts[i, :, 0], pts[i, :, 1], pts[i, :, 2] = y1 + shape[:, 0] * (y2 - y1), x1 + shape[:, 1] * (x2 - x1), 0.9
        return pts

    first = np.asarray([[10, 30, 60, 110], [90, 20, 150, 100]], np.int32)
    second = np.asarray([[92, 22, 151, 101], [12, 31, 61, 112], [60, 50, 100, 118]], np.int32)      # the two swapped, and a newcomer
    tracker = pkg.PersonTracker(net)
    tracker.update(torch.from_numpy(first).cuda(), torch.from_numpy(people(first)).cuda())
    boxes, pts, ids = tracker.update(torch.from_numpy(second).cuda(), torch.from_numpy(people(second)).cuda())
    assert boxes.is_cuda and ids.is_cuda and ids.dtype == torch.int32
    before = noise((120, 160, 3), int(rng.integers(100)))
    dev = torch.from_numpy(before.copy()).cuda()
    net.draw_poses(dev, pts, COCO, person_ids=ids)
    net.draw_labels(dev, boxes, ids)
    h_boxes, h_pts, h_ids = boxes.cpu().numpy(), pts.cpu().numpy(), ids.cpu().numpy()
    assert h_ids[:2].tolist() == [1, 0] and h_ids[2] >= 2                      # the ids held through the swap
    set2 = pkg.palette("Set2", 8)
    wide = set2.astype(np.int64)
    luma = (114 * wide[:, 0] + 587 * wide[:, 1] + 299 * wide[:, 2]) // 1000
    text = np.where(luma[:, None] >= 128, 0, 255).astype(np.uint8).repeat(3, 1)
    assert (luma >= 128).all()                                                 # Set2 is light: black digits
    want = draw_ref.draw_bgr(before.copy(), h_pts, COCO, pkg.palette("tab20", 16), set2, person_index=h_ids)
    want = label_ref.draw_bgr(want, h_boxes, set2, text, person_ids=h_ids)
    np.testing.assert_array_equal(dev.cpu().numpy(), want)
    # host ids / boxes give the same bytes as the ones on the device
    again = net.draw_labels(net.draw_poses(before.copy(), h_pts, COCO, person_ids=h_ids), h_boxes, h_ids)
    np.testing.assert_array_equal(again.cpu().numpy(), want)
    # a dark palette takes white digits
    dark = np.asarray([[20, 30, 40], [200, 220, 240]], np.uint8)
    dev2 = torch.from_numpy(before.copy()).cuda()
    net.draw_labels(dev2, boxes, ids, palette=dark)
    want2 = label_ref.draw_bgr(before.copy(), h_boxes, dark, np.asarray([[255] * 3, [0] * 3], np.uint8), person_ids=h_ids)
    np.testing.assert_array_equal(dev2.cpu().numpy(), want2)


def test_scores_are_read_from_the_detections_where_they_lie(net):
    rng = np.random.default_rng(6)
    dets = np.zeros((5, 5), np.float32)
    dets[:, :2] = rng.uniform(0, 40, (5, 2))
    dets[:, 2:4] = dets[:, :2] + rng.uniform(10, 50, (5, 2))
    dets[:, 4] = [0.912, 0.5, 0.049, 1.0, np.nan]
    d_dets = torch.from_numpy(dets).cuda()
    boxes = np.rint(dets[:, :4]).astype(np.int32)
    before = noise((70, 100, 3), 9)
    dev = torch.from_numpy(before.copy()).cuda()
    view = d_dets[:, 4]
    assert view.stride(0) == 5 and not view.is_contiguous()
    net.draw_labels(dev, boxes, scores=view, palette=CO, text_colors=TX)
    want = label_ref.draw_bgr(before.copy(), boxes, CO, TX, scores=dets[:, 4])
    np.testing.assert_array_equal(dev.cpu().numpy(), want)
    np.testing.assert_array_equal(d_dets.cpu().numpy(), dets)                  # the detections are only read
    host = net.draw_labels(before.copy(), boxes, scores=dets[:, 4], palette=CO, text_colors=TX)      # a strided host view is uploaded
    np.testing.assert_array_equal(host.cpu().numpy(), want)


def test_nobody_and_refusals_leave_the_frame_untouched(net):
    before = noise((45, 70, 3), 2)
    dev = torch.from_numpy(before.copy()).cuda()
    assert net.draw_labels(dev, np.zeros((0, 4), np.int32)) is dev                               # n == 0
    assert net.draw_labels(dev, np.zeros((0, 4), np.int32), person_ids=np.zeros(0, np.int32), scores=np.zeros(0, np.float32)) is dev
    box = np.asarray([[5, 15, 40, 40]], np.int32)
    for kw, text in ((dict(scale=17), r"scale must be in \[0, 16\]"), (dict(scale=-1), "scale must be in"), (dict(thickness=17), "thickness must be in"),
                     (dict(thickness=-1), r"thickness must be in \[0, 16\]")):
        with pytest.raises(RuntimeError, match=text):
            net.draw_labels(dev, box, person_ids=[3], **kw)
    for kw, text in ((dict(person_ids=[1, 2]), "one entry per person"), (dict(scores=[0.1, 0.2]), "one entry per person"),
                     (dict(frame_index=[0, 0]), "one entry per person"), (dict(text_colors=TX[:2], palette=CO), "one colour per palette entry")):
        with pytest.raises(ValueError, match=text):
            net.draw_labels(dev, box, **kw)
    with pytest.raises(ValueError, match="integers"):
        net.draw_labels(dev, box.astype(np.float32))
    with pytest.raises(ValueError, match="in place"):
        net.draw_labels(dev[:, :, [2, 1, 0]].permute(1, 0, 2), box)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.cpu().numpy(), before)
