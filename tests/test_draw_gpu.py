"""Pose overlays on the GPU: ``NativeHRNet.draw_poses`` against the numpy restatement of the drawing definition
(tests/draw_ref.py) -- whole buffers, byte for byte, on frames of random bytes so that a stray write shows."""
import json
import os

import numpy as np
import pytest
import torch

import draw_ref
import yuv_ref
from conftest import GOLDEN, load_pkg, state_dict_np

pytestmark = pytest.mark.gpu

COCO = json.load(open(os.path.join(GOLDEN, "coco_skeleton.json")))["coco_skeleton"]
# colours of the tests' own: five for the joints and three for the bones, so that both modulos are exercised
PC = np.asarray([[250, 10, 20], [30, 240, 40], [50, 60, 230], [200, 210, 0], [0, 220, 215]], np.uint8)
BC = np.asarray([[255, 255, 255], [1, 2, 3], [90, 160, 70]], np.uint8)


@pytest.fixture(scope="module")
def net():
    n = load_pkg().NativeHRNet(32, 17, (64, 96), "fp32", max_batch=4, device=0)
    yield n
    n.close()


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def person(*joints, conf=0.9):
    """(J, 3) (y, x, confidence) from (x, y) or (x, y, confidence) tuples"""
    return np.asarray([[j[1], j[0], j[2] if len(j) > 2 else conf] for j in joints], np.float32)


def check_bgr(net, h, w, pts, skeleton, seed=0, **kw):
    """draws on the GPU and in numpy; returns (frame before, frame after), the two having been held equal"""
    before = noise((h, w, 3), seed)
    pts = np.asarray(pts, np.float32)
    pts = pts[None] if pts.ndim == 2 else pts
    dev = torch.from_numpy(before.copy()).cuda()
    out = net.draw_poses(dev, pts, skeleton, points_palette=PC, skeleton_palette=BC, **kw)
    assert out is dev
    ref_kw = dict(radius=kw.get("radius"), thickness=kw.get("thickness", 2), threshold=kw.get("confidence_threshold", 0.5),
                  person_index=kw.get("person_ids"))
    want = draw_ref.draw_bgr(before.copy(), pts, skeleton, PC, BC, **ref_kw)
    got = dev.cpu().numpy()
    np.testing.assert_array_equal(got, want, err_msg=str((h, w, kw)))
    return before, got


@pytest.mark.parametrize("r", [1, 2, 3, 6, 13])
def test_single_discs(net, r):
    native = load_pkg("native")
    h, w, t = 45, 70, native.DRAW_TILE
    assert t < h and 2 * t < w                              # the frame has tile borders on both axes
    places = [(35, 22), (0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    places += [(x, y) for x in (t - 1, t, 2 * t - 1, 2 * t) for y in (20, t - 1, t)]     # across every tile border
    for k, (x, y) in enumerate(places):
        before, after = check_bgr(net, h, w, person((x, y)), [], seed=k, radius=r)
        changed = (before != after).any(-1)
        assert changed.sum() <= (2 * r + 1) ** 2 and after[y, x].tolist() == PC[0].tolist()
    before, after = check_bgr(net, h, w, person((-r - 1, 20)), [], radius=r)              # one column too far left
    np.testing.assert_array_equal(before, after)
    before, after = check_bgr(net, h, w, person((-r, 20)), [], radius=r)                  # ... and touching column 0
    assert (after[20, 0] == PC[0]).all() and (before != after).any(-1).sum() <= 2 * int(r ** 0.5) + 1     # rows with dy * dy <= r
    if r == 1:                                                                            # the 3 x 3 square, literally
        before, after = check_bgr(net, h, w, person((35, 22)), [], seed=99, radius=1)
        ys, xs = np.nonzero((after == PC[0]).all(-1) & ~(before == PC[0]).all(-1))
        assert set(zip(xs.tolist(), ys.tolist())) <= {(35 + a, 22 + b) for a in (-1, 0, 1) for b in (-1, 0, 1)}
        assert (after[21:24, 34:37] == PC[0]).all()


BONES = {
    "horizontal": ((10, 20), (50, 20)), "vertical": ((40, 5), (40, 40)), "diagonal": ((5, 5), (40, 40)),
    "slope 11:4": ((10, 10), (54, 26)), "slope 4:11": ((20, 3), (32, 36)), "zero length": ((30, 30), (30, 30)),
    "one end outside": ((-5, 20), (40, 30)), "crossing": ((-10, -10), (80, 60)), "outside": ((-30, 10), (-10, 40)),
}


@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_single_bones(net, T):
    one = PC[:1]                                            # both joints in one colour: reversed endpoints give the same pixels
    for k, (name, (p0, p1)) in enumerate(BONES.items()):
        frames = []
        for a, b in ((p0, p1), (p1, p0)):
            before = noise((45, 70, 3), k)
            dev = torch.from_numpy(before.copy()).cuda()
            pts = person(a, b)[None]
            net.draw_poses(dev, pts, [[0, 1]], points_palette=one, skeleton_palette=BC, radius=1, thickness=T)
            want = draw_ref.draw_bgr(before.copy(), pts, [[0, 1]], one, BC, radius=1, thickness=T)
            np.testing.assert_array_equal(dev.cpu().numpy(), want, err_msg="%s T=%d" % (name, T))
            frames.append(want)
        np.testing.assert_array_equal(frames[0], frames[1], err_msg=name)
        if name == "outside":
            np.testing.assert_array_equal(frames[0], noise((45, 70, 3), k))
        elif name != "zero length":
            assert ((frames[0] == BC[0]).all(-1)).sum() > 5, name          # the bone is there, in the bone colour


def test_liveness(net):
    sk = [[0, 1], [1, 2], [2, 3]]
    base = [(10, 10), (30, 12), (50, 30), (20, 40)]
    dead = [(30, 12, 0.5), (30, 12, np.nan), (np.nan, 12), (30, np.nan), (np.inf, 12), (30, -np.inf), (20000, 12), (30, -20000),
            (-20000, 12), (30, 20000)]
    for k, joint in enumerate(dead):
        pts = person(base[0], joint, base[2], base[3])
        before, after = check_bgr(net, 45, 70, pts, sk, seed=k)
        alone = draw_ref.draw_bgr(before.copy(), person(base[2], base[3])[None], [[0, 1]], PC[2:4], BC)   # joints 2, 3 and their bone
        alone = draw_ref.draw_bgr(alone, person(base[0])[None], [], PC, BC)
        np.testing.assert_array_equal(after, alone, err_msg=str(joint))
    # just above the threshold is live; x = -0.7 truncates to column 0; the largest legal coordinates are live (and off the frame)
    before, after = check_bgr(net, 45, 70, person((30, 12, np.nextafter(np.float32(0.5), np.float32(1)))), [])
    assert (after[12, 30] == PC[0]).all()
    before, after = check_bgr(net, 45, 70, person((-0.7, 20.9)), [], radius=1)
    assert (after[19:22, 0:2] == PC[0]).all() and (before != after).any(-1).sum() <= 6
    check_bgr(net, 45, 70, person((16383.9, -8192.9), (35, 22)), [[0, 1]])
    check_bgr(net, 45, 70, person((-8192, 16383), (16383, -8192)), [[0, 1]], thickness=16)
    check_bgr(net, 45, 70, person((35, 22, 0.2)), [], confidence_threshold=0.1)


def test_order(net):
    # coincident joints of two people, under different joint numbers so that the colours tell who lies on top
    a = person((30, 20), (50, 25), (12, 30))
    b = person((50, 25), (30, 20), (40, 40))
    before, after = check_bgr(net, 45, 70, [a, b], [[0, 1], [1, 2]], radius=3)
    assert (after[20, 30] == PC[1]).all() and (after[25, 50] == PC[0]).all()     # person 1's joints lie on top
    # a bone of person 1 over a joint of person 0; a joint over its own bones
    a = person((35, 22), (35, 22), (35, 22))
    b = person((10, 22), (60, 22), (60, 40))
    before, after = check_bgr(net, 45, 70, [a, b], [[0, 1], [1, 2]], radius=6, thickness=3)
    assert (after[22, 35] == BC[1]).all() and (after[27, 35] == PC[2]).all() and (after[22, 60] == PC[1]).all()
    # person_ids beyond the palette, and negative (Python's modulo)
    people = [person((10 + 12 * i, 8), (14 + 12 * i, 38)) for i in range(5)]
    before, after = check_bgr(net, 45, 70, people, [[0, 1]], person_ids=[7, 3, -1, 300, 2], thickness=3, radius=1)
    for i, pid in enumerate([7, 3, -1, 300, 2]):
        assert (after[23, 12 + 12 * i] == BC[pid % 3]).all(), (i, after[23, 12 + 12 * i])


def test_crowd_overflows_every_list(net):
    """48 people x (19 bones + 17 joints) inside one tile: 1728 primitives, more than the tile's list holds at once"""
    native = load_pkg("native")
    t = native.DRAW_TILE
    rng = np.random.default_rng(5)
    pts = np.empty((48, 17, 3), np.float32)
    pts[..., 0] = rng.uniform(t + 2, t + 26, (48, 17))
    pts[..., 1] = rng.uniform(t + 2, t + 26, (48, 17))
    pts[..., 2] = 0.9
    assert 48 * (len(COCO) + 17) == 1728 and t + 26 < 2 * t
    check_bgr(net, 97, 131, pts, COCO, seed=1, radius=1, thickness=1)      # thin shapes: deep into the list before a pixel is settled
    check_bgr(net, 97, 131, pts, COCO, seed=2)
    pts[::2, :, 2] = 0.3
    check_bgr(net, 97, 131, pts, COCO, seed=3, radius=2, thickness=3)


def test_more_people_than_one_chunk(net):
    """300 people on one frame: the rasteriser takes a frame's people 256 at a time from the end of the call order, so a tile
    sees two person chunks; the early people (the second chunk) show wherever the later ones left pixels free"""
    rng = np.random.default_rng(8)
    h, w, n = 97, 131, 300
    pts = np.empty((n, 3, 3), np.float32)
    pts[..., 0] = rng.uniform(-6, h + 6, (n, 3))
    pts[..., 1] = rng.uniform(-6, w + 6, (n, 3))
    pts[..., 2] = rng.uniform(0.3, 1.0, (n, 3))
    sk = [[0, 1], [1, 2]]
    before, after = check_bgr(net, h, w, pts, sk, seed=4, thickness=1)
    number, _ = draw_ref.paint(h, w, pts[:300 - 256], sk, PC, BC, thickness=1)        # what the first 44 people alone cover ...
    late, _ = draw_ref.paint(h, w, pts[300 - 256:], sk, PC, BC, thickness=1)
    assert ((number >= 0) & (late < 0)).sum() > 20                                    # ... and the others leave visible
    check_bgr(net, h, w, pts, sk, seed=5, person_ids=rng.integers(-50, 50, n).tolist())
    pts[40:, :, 2] = 0.1                                                              # only people of the second chunk are live
    check_bgr(net, h, w, pts, sk, seed=6)


def test_many_joints(net):
    """J = 133 (whole-body) and J = 256: the build launch takes the joints 64 at a time and the live mask has eight words"""
    rng = np.random.default_rng(9)
    h, w = 97, 131
    for J in (133, 256):
        pts = np.empty((3, J, 3), np.float32)
        pts[..., 0] = rng.uniform(-6, h + 6, (3, J))
        pts[..., 1] = rng.uniform(-6, w + 6, (3, J))
        pts[..., 2] = rng.uniform(0.2, 1.0, (3, J))
        sk = [[int(a), int(b)] for a, b in rng.integers(0, J, (90, 2))] + [[J - 1, 0], [64, 63], [J - 1, J - 2]]
        check_bgr(net, h, w, pts, sk, seed=J, thickness=1)
        dead = pts.copy()
        dead[:, :64, 2] = 0.0                                                         # the first pass of the build loop: nobody live
        before, after = check_bgr(net, h, w, dead, sk, seed=J + 1)
        assert (before != after).any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_people(net, seed):
    rng = np.random.default_rng(100 + seed)
    h, w, n = 131, 97, 7
    pts = np.empty((n, 17, 3), np.float32)
    pts[..., 0] = rng.uniform(-12, h + 12, (n, 17))
    pts[..., 1] = rng.uniform(-12, w + 12, (n, 17))
    pts[..., 2] = rng.uniform(0.2, 1.0, (n, 17))
    check_bgr(net, h, w, pts, COCO, seed=seed, radius=int(rng.integers(1, 5)), thickness=int(rng.integers(1, 6)))
    check_bgr(net, h, w, pts, COCO, seed=seed)


def test_clip_mode(net):
    sizes = [(320, 400), (161, 200), None, (480, 96)]
    assert [draw_ref.default_radius(*s) for s in sizes if s] == [2, 1, 1]
    rng = np.random.default_rng(11)
    frame_index = rng.permutation(np.repeat([0, 1, 3], [5, 3, 4])).astype(np.int32)
    pts = np.empty((len(frame_index), 17, 3), np.float32)
    for i, f in enumerate(frame_index):
        pts[i, :, 0] = rng.uniform(-5, sizes[f][0] + 5, 17)
        pts[i, :, 1] = rng.uniform(-5, sizes[f][1] + 5, 17)
    pts[..., 2] = rng.uniform(0.3, 1.0, pts.shape[:2])
    before = [None if s is None else noise(s + (3,), 20 + k) for k, s in enumerate(sizes)]
    dev = [None if b is None else torch.from_numpy(b.copy()).cuda() for b in before]
    out = net.draw_poses(dev, torch.from_numpy(pts).cuda(), COCO, frame_index=frame_index, points_palette=PC, skeleton_palette=BC)
    assert out[2] is None and all(o is d for o, d in zip(out, dev))
    want = draw_ref.draw_clip([None if b is None else b.copy() for b in before], pts, frame_index, COCO, PC, BC)
    for f, s in enumerate(sizes):
        if s is None:
            continue
        np.testing.assert_array_equal(dev[f].cpu().numpy(), want[f], err_msg="frame %d" % f)
        who = np.nonzero(frame_index == f)[0]                      # ... and the same as a call of that frame's own
        alone = net.draw_poses(before[f], pts[who], COCO, person_ids=who, points_palette=PC, skeleton_palette=BC)
        assert alone.is_cuda
        np.testing.assert_array_equal(alone.cpu().numpy(), want[f], err_msg="frame %d alone" % f)
    with pytest.raises(ValueError, match="frame_index"):
        net.draw_poses(dev, pts, COCO)
    with pytest.raises(RuntimeError, match="is null"):
        net.draw_poses(dev, pts[:1], COCO, frame_index=[2])


def test_pitched_view(net):
    big = noise((50, 100, 3), 7)
    dev = torch.from_numpy(big.copy()).cuda()
    pts = np.stack([person((-3, 5), (75, 38), (30, 20)), person((69, 0), (0, 39), (35, 45))])
    out = net.draw_poses(dev[5:45, 10:80], pts, [[0, 1], [1, 2]], points_palette=PC, skeleton_palette=BC, radius=4, thickness=5)
    assert out.data_ptr() == dev[5:45, 10:80].data_ptr()
    want = big.copy()
    draw_ref.draw_bgr(want[5:45, 10:80], pts, [[0, 1], [1, 2]], PC, BC, radius=4, thickness=5)
    np.testing.assert_array_equal(dev.cpu().numpy(), want)
    assert (want != big).any() and (want[:5] == big[:5]).all() and (want[:, :10] == big[:, :10]).all()
    with pytest.raises(ValueError, match="in place"):
        net.draw_poses(dev[:, :, [2, 1, 0]].permute(1, 0, 2), pts, [])
    # a host array with the same strides is uploaded, drawn and returned
    host = net.draw_poses(big[5:45, 10:80], pts, [[0, 1], [1, 2]], points_palette=PC, skeleton_palette=BC, radius=4, thickness=5)
    np.testing.assert_array_equal(host.cpu().numpy(), want[5:45, 10:80])


YUV_SIZES = [(2, 2, None), (34, 50, 64), (48, 88, None)]


@pytest.mark.parametrize("fmt,key", [("nv12", ("bt601", "limited")), ("i420", ("bt709", "full")), ("nv12", ("bt709", "limited")),
                                     ("i420", ("bt601", "full"))])
def test_yuv_canvases(net, fmt, key):
    pkg = load_pkg()
    bound = 2 if key[1] == "limited" else 1
    pc, bc = pkg.bgr_to_yuv_colors(PC, *key), pkg.bgr_to_yuv_colors(BC, *key)
    sk = [[0, 1], [1, 2]]
    for k, (h, w, pitch) in enumerate(YUV_SIZES):
        # person 0: a vertical bone on the odd column 7, rows 3 .. h - 5; person 1: a horizontal one on the odd row 11 that
        # crosses it (two colours meet in 2 x 2 blocks), then down to a corner; person 2: a fat disc that fills whole blocks
        people = np.stack([person((7, 3), (7, h - 5), (7, h - 5)), person((4, 11), (w - 6, 11), (w - 1, h - 1)),
                           person((w // 2, h // 2), (w // 2, h // 2, 0.1), (0, 0))])
        for T, r in ((1, 1), (2, 5)):
            data = noise(yuv_ref.nbytes(h, w, pitch), 40 + k)
            frame = pkg.YuvFrame(torch.from_numpy(data.copy()).cuda(), h, w, fmt, key[0], key[1], pitch)
            out = net.draw_poses(frame, people, sk, points_palette=PC, skeleton_palette=BC, radius=r, thickness=T)
            assert out is frame
            want = draw_ref.draw_yuv(data.copy(), h, w, fmt, people, sk, pc, bc, pitch=pitch, radius=r, thickness=T)
            got = frame.data.cpu().numpy()
            for name, a, b in zip("YUV", yuv_ref.planes(got, h, w, fmt, pitch), yuv_ref.planes(want, h, w, fmt, pitch)):
                np.testing.assert_array_equal(a, b, err_msg="%s plane %s" % (name, (fmt, h, w, pitch, T, r)))
            np.testing.assert_array_equal(got, want, err_msg="pitch bytes %s" % ((fmt, h, w, pitch, T, r),))
            if (h, w) != (2, 2):
                assert (got != data).any()
            # where ONE primitive covers a whole 2 x 2 block the frame reads back as that primitive's colour, within the
            # bound of hrn_yuv_from_bgr's round trip
            number, colour = draw_ref.paint(h, w, people, sk, PC, BC, radius=r, thickness=T)
            blocks = number.reshape(h // 2, 2, w // 2, 2)
            if (h, w) != (2, 2):
                # the cases this test is about are really there: a 2 x 2 block shared by two primitives (two colours meet in one
                # chroma sample), and at T = 1 the vertical bone as a run of single pixels on the odd column 7
                drawn = np.where(blocks >= 0, blocks, blocks.max() + 1)
                assert (drawn.min((1, 3)) < blocks.max((1, 3))).any()      # two different primitives among a block's covered pixels
                if T == 1:
                    bone0 = number[5:h - 7, 6:9] == 0                  # primitive 0 = person 0's bone (0, 1), away from its discs
                    assert bone0[:, 1].any() and not bone0[:, 0].any() and not bone0[:, 2].any()
            whole = (blocks.min((1, 3)) == blocks.max((1, 3))) & (blocks.min((1, 3)) >= 0)
            whole = np.repeat(np.repeat(whole, 2, 0), 2, 1)
            back = net.yuv_to_bgr(frame).cpu().numpy()
            err = np.abs(back.astype(np.int16) - colour.astype(np.int16))[whole]
            assert r == 1 or whole.any()
            assert err.size == 0 or err.max() <= bound, (fmt, key, h, w, int(err.max()))


def test_predict_then_draw(net):
    frame = noise((120, 160, 3), 3)
    net.load_state_dict(state_dict_np(32))
    dets = np.asarray([[10.2, 8.7, 90.4, 100.1], [60.5, 20.5, 150.0, 70.0], [5, 40, 70, 118]], np.float32)
    dev = torch.from_numpy(frame.copy()).cuda()
    _, pts = net.predict_frame(dev, dets)
    thr = float(np.median(pts[..., 2].cpu().numpy()))          # about half of the joints are live
    net.draw_poses(dev, pts, COCO, confidence_threshold=thr, points_palette=PC, skeleton_palette=BC)
    once = dev.cpu().numpy()
    want = draw_ref.draw_bgr(frame.copy(), pts.cpu().numpy(), COCO, PC, BC, threshold=thr)
    np.testing.assert_array_equal(once, want)
    assert (once != frame).any()
    net.draw_poses(dev, pts, COCO, confidence_threshold=thr, points_palette=PC, skeleton_palette=BC)
    np.testing.assert_array_equal(dev.cpu().numpy(), once)      # drawing twice is drawing once
    # the palettes by name, as the demo calls it
    pkg = load_pkg()
    dev2 = torch.from_numpy(frame.copy()).cuda()
    net.draw_poses(dev2, pts, COCO, confidence_threshold=thr)
    want = draw_ref.draw_bgr(frame.copy(), pts.cpu().numpy(), COCO, pkg.palette("tab20", 16), pkg.palette("Set2", 8), threshold=thr)
    np.testing.assert_array_equal(dev2.cpu().numpy(), want)
