"""Frame rotation on the GPU: ``NativeHRNet.rotate_frames`` against the numpy restatement (tests/rotate_ref.py), byte for byte over
WHOLE destination buffers pre-filled with a sentinel (a write into pitch padding or past a row shows), the chain into
``predict_frame`` / ``detector_input`` / ``draw_poses``, ``rotate_people`` against its host form.  Every comparison is equality.

The sides sit on, below and above the edge of any 16-, 32- or 64-element tile, with a remainder after two tiles (131)."""
import json
import os

import numpy as np
import pytest
import torch

import yuv_ref
from conftest import GOLDEN, load_pkg, state_dict_np
from rotate_ref import rotate_plane, rotate_yuv, rotated_hw

pytestmark = pytest.mark.gpu

SIDES = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 131]
YUV_SIDES = sorted({s for s in SIDES if s % 2 == 0} | {2, 30, 34, 62, 66, 130})
SENTINEL = 0xA5
COCO = json.load(open(os.path.join(GOLDEN, "coco_skeleton.json")))["coco_skeleton"]
_NETS = {}


def engine(dtype="fp32"):
    if dtype not in _NETS:
        _NETS[dtype] = load_pkg().NativeHRNet(32, 17, (64, 64), dtype, max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    return _NETS[dtype]


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def pitched_bgr(buf, offset, h, w, pitch):
    """an (h, w, 3) view of rows `pitch` bytes apart at byte `offset` of the flat tensor or array `buf`"""
    if isinstance(buf, torch.Tensor):
        return buf[offset:offset + h * pitch].as_strided((h, w, 3), (pitch, 3, 1))
    return np.lib.stride_tricks.as_strided(buf[offset:offset + h * pitch], (h, w, 3), (pitch, 3, 1))


# ------------------------------------------------------------------------------------------------------------------- BGR
@pytest.mark.parametrize("pitched", [False, True], ids=["packed", "pitched"])
@pytest.mark.parametrize("code", [0, 1, 2])
def test_bgr_every_size_in_one_call(code, pitched):
    """144 frames of differing sizes in ONE call, all sources in one buffer and all destinations in another; pitched: source
    rows 3 W + 5 and destination rows 3 W' + 7 bytes apart and the frames back to back, so that bases and rows are misaligned"""
    net = engine()
    sizes = [(h, w) for h in SIDES for w in SIDES]
    spitch = [3 * w + (5 if pitched else 0) for h, w in sizes]
    dsize = [rotated_hw(h, w, code) for h, w in sizes]
    dpitch = [3 * w + (7 if pitched else 0) for h, w in dsize]
    room = (lambda b: b) if pitched else (lambda b: (b + 15) // 16 * 16)   # packed frames start on 16 bytes: the dword paths run
    soff = np.concatenate([[0], np.cumsum([room(h * p) for (h, w), p in zip(sizes, spitch)])])
    doff = np.concatenate([[0], np.cumsum([room(h * p) for (h, w), p in zip(dsize, dpitch)])])
    src_host = noise(int(soff[-1]), 100 + code)
    want = np.full(int(doff[-1]), SENTINEL, np.uint8)
    for k, ((h, w), (rh, rw)) in enumerate(zip(sizes, dsize)):
        pitched_bgr(want, int(doff[k]), rh, rw, dpitch[k])[...] = rotate_plane(pitched_bgr(src_host, int(soff[k]), h, w, spitch[k]), code)
    src_dev = torch.from_numpy(src_host).cuda()
    dst_dev = torch.full((int(doff[-1]),), SENTINEL, dtype=torch.uint8, device="cuda")
    frames = [pitched_bgr(src_dev, int(soff[k]), h, w, spitch[k]) for k, (h, w) in enumerate(sizes)]
    out = [pitched_bgr(dst_dev, int(doff[k]), rh, rw, dpitch[k]) for k, (rh, rw) in enumerate(dsize)]
    back = net.rotate_frames(frames, code, out=out)
    assert all(a is b for a, b in zip(back, out))
    got = dst_dev.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%d bytes differ, first at %d (frame %d)" % (len(bad), bad[0], np.searchsorted(doff, bad[0], "right") - 1)
    np.testing.assert_array_equal(src_dev.cpu().numpy(), src_host)          # the sources are only read
    if not pitched:   # without out=: fresh frames of the rotated sizes, the same bytes
        fresh = net.rotate_frames([f.contiguous() for f in frames], code)
        for k in (0, 13, 77, 143):
            np.testing.assert_array_equal(fresh[k].cpu().numpy(), pitched_bgr(want, int(doff[k]), *dsize[k], dpitch[k]))


# ------------------------------------------------------------------------------------------------------------------- YUV
def yuv_case(fmt, code, pitched, seed):
    pkg = load_pkg()
    frames, outs, wants, raws = [], [], [], []
    for k, (h, w) in enumerate((h, w) for h in YUV_SIDES for w in YUV_SIDES):
        rh, rw = rotated_hw(h, w, code)
        pitch, out_pitch = (w + 6, rw + 6) if pitched else (w, rw)
        data = noise(yuv_ref.nbytes(h, w, pitch), seed + k)
        raws.append((data, h, w, pitch))
        frames.append(pkg.YuvFrame(torch.from_numpy(data).cuda(), h, w, fmt, "bt601", "limited", pitch))
        fill = np.full(yuv_ref.nbytes(rh, rw, out_pitch), SENTINEL, np.uint8)
        outs.append(pkg.YuvFrame(torch.from_numpy(fill).cuda(), rh, rw, fmt, "bt601", "limited", out_pitch))
        wants.append(rotate_yuv(data, h, w, fmt, code, pitch, out_pitch, fill))
    return frames, outs, wants, raws


@pytest.mark.parametrize("pitched", [False, True], ids=["packed", "pitched"])
@pytest.mark.parametrize("code", [0, 1, 2])
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_yuv_every_size_in_one_call(fmt, code, pitched):
    net = engine()
    frames, outs, wants, raws = yuv_case(fmt, code, pitched, 1000 * code + 7)
    back = net.rotate_frames(frames, code, out=outs)
    assert all(a is b for a, b in zip(back, outs))
    for k, (o, want) in enumerate(zip(outs, wants)):
        np.testing.assert_array_equal(o.data.cpu().numpy(), want, err_msg="frame %d (%d x %d)" % (k, raws[k][1], raws[k][2]))
    if pitched:
        return
    # fresh YuvFrames: swapped sides, the frame's own format, matrix and range, pitch == width; and the conversion commutes with
    # the rotation, bit for bit: 2 x 2 chroma blocks map onto 2 x 2 blocks
    fresh = net.rotate_frames(frames, code)
    for k, (f, r, want) in enumerate(zip(frames, fresh, wants)):
        assert (r.height, r.width) == rotated_hw(f.height, f.width, code) and r.pitch == r.width
        assert (r.format, r.matrix, r.range) == (f.format, f.matrix, f.range) and r.data.is_cuda
        np.testing.assert_array_equal(r.data.cpu().numpy(), want)
        np.testing.assert_array_equal(net.yuv_to_bgr(r).cpu().numpy(), rotate_plane(net.yuv_to_bgr(f).cpu().numpy(), code), err_msg=str(k))


# ------------------------------------------------------------------------------------------- the forms of a call, 1080p
def test_mixed_codes_stack_sequence_and_out():
    net = engine()
    frames = [noise((48, 80, 3), 1), noise((33, 17, 3), 2), None, noise((64, 64, 3), 3), noise((5, 131, 3), 4)]
    codes = [2, 0, 1, 1, 0]
    mixed = net.rotate_frames(frames, codes)
    assert mixed[2] is None and len(mixed) == 5
    for k, (f, c) in enumerate(zip(frames, codes)):
        if f is None:
            continue
        alone = net.rotate_frames(f, c)                                   # one frame: its planes travel in the kernel arguments
        assert alone.is_cuda and torch.equal(alone, mixed[k])
        assert torch.equal(net.rotate_frames(torch.from_numpy(f).cuda(), c), alone)     # a resident frame: the lean path of the call
        np.testing.assert_array_equal(alone.cpu().numpy(), rotate_plane(f, c))
    stack = noise((4, 40, 56, 3), 5)
    for c in (0, 1, 2):
        turned = net.rotate_frames(stack, c)                              # a stack comes back as a stack
        assert turned.shape == (4,) + rotated_hw(40, 56, c) + (3,) and turned.is_cuda
        sequence = net.rotate_frames(list(stack), c)
        for k in range(4):
            assert torch.equal(turned[k], sequence[k])
            np.testing.assert_array_equal(turned[k].cpu().numpy(), rotate_plane(stack[k], c))
        out = torch.full_like(turned, SENTINEL)
        assert net.rotate_frames(torch.from_numpy(stack).cuda(), c, out=out) is out and torch.equal(out, turned)
    per_frame = net.rotate_frames(stack, [0, 2, 2, 0])
    np.testing.assert_array_equal(per_frame[1].cpu().numpy(), rotate_plane(stack[1], 2))
    with pytest.raises(ValueError, match="stack"):
        net.rotate_frames(stack, [0, 1, 0, 0])
    # no code: the resident frames, unrotated
    same = net.rotate_frames(stack, None)
    assert same.is_cuda and np.array_equal(same.cpu().numpy(), stack)
    assert net.rotate_frames(frames, None)[2] is None and net.rotate_frames(frames[0], None).shape == (48, 80, 3)
    assert net.rotate_frames([], 1) == []


@pytest.mark.parametrize("code", [0, 1, 2])
@pytest.mark.parametrize("fmt", ["bgr", "nv12", "i420"])
def test_full_hd_frame(fmt, code):
    pkg, net = load_pkg(), engine()
    if fmt == "bgr":
        frame = noise((1080, 1920, 3), code)
        got = net.rotate_frames(frame, code)
        np.testing.assert_array_equal(got.cpu().numpy(), rotate_plane(frame, code))
    else:
        data = noise(yuv_ref.nbytes(1080, 1920), 10 + code)
        got = net.rotate_frames(pkg.YuvFrame(data, 1080, 1920, fmt, "bt709", "limited"), code)
        assert (got.height, got.width, got.matrix) == rotated_hw(1080, 1920, code) + ("bt709",)
        np.testing.assert_array_equal(got.data.cpu().numpy(), rotate_yuv(data, 1080, 1920, fmt, code))


# ------------------------------------------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_predict_frame_on_the_rotated_frame(fmt, dtype):
    """a frame rotated on the device and a frame rotated on the host give the same boxes, joints and confidences, bit for bit"""
    pkg, net = load_pkg(), engine(dtype)
    h, w = 96, 128
    for code in (0, 1, 2):
        rh, rw = rotated_hw(h, w, code)
        dets = np.asarray([[5, 7, rw - 9, rh - 11, 0.9], [rw // 3, rh // 4, rw // 3 + 30, rh // 4 + 44, 0.8], [0, 0, 21, 40, 0.7]], np.float32)
        if fmt == "bgr":
            frame = noise((h, w, 3), 40 + code)
            on_device, on_host = net.rotate_frames(frame, code), rotate_plane(frame, code)
        else:
            data = noise(yuv_ref.nbytes(h, w), 50 + code)
            on_device = net.rotate_frames(pkg.YuvFrame(data, h, w, "nv12", "bt601", "full"), code)
            on_host = pkg.YuvFrame(rotate_yuv(data, h, w, "nv12", code), rh, rw, "nv12", "bt601", "full")
        boxes_a, pts_a = net.predict_frame(on_device, dets)
        boxes_b, pts_b = net.predict_frame(on_host, dets)
        np.testing.assert_array_equal(boxes_a, boxes_b)
        assert pts_a.shape == (3, 17, 3) and torch.equal(pts_a.view(torch.int32), pts_b.view(torch.int32))
        size = 64
        got, _ = net.detector_input(on_device, size, dtype=torch.uint8)
        want, _ = net.detector_input(on_host, size, dtype=torch.uint8)
        assert torch.equal(got, want)


@pytest.mark.parametrize("J", [17, 133])
def test_rotate_people_equals_the_host_form(J):
    P, net = load_pkg("postproc"), engine()
    rng = np.random.default_rng(J)
    for n in (0, 1, 2, 63, 64, 65, 300):
        pts = rng.uniform(-50, 2000, (n, J, 3)).astype(np.float32)
        if n:
            pts[0, 0, 0], pts[0, 1, 1], pts[-1, -1, 0], pts[-1, 0, 2] = np.nan, np.inf, -np.inf, np.nan
        boxes = rng.integers(0, 1900, (n, 4)).astype(np.int32)
        boxes[::3] = 0
        sizes = np.stack([rng.integers(1, 2000, n), rng.integers(1, 2000, n)], 1).astype(np.int32)
        codes = rng.integers(0, 3, n).astype(np.int32)
        for hw, code in (((1080, 1920), 0), ((1080, 1920), 1), ((7, 3), 2), (sizes, 1), ((1080, 1920), codes), (sizes, codes)):
            want_p, want_b = P.rotate_people(pts, boxes, hw, code)
            got_p, got_b = net.rotate_people(torch.from_numpy(pts).cuda(), torch.from_numpy(boxes).cuda(), hw, code)
            assert got_p.is_cuda and got_b.is_cuda
            np.testing.assert_array_equal(got_p.cpu().numpy().view(np.uint32), want_p.view(np.uint32))
            np.testing.assert_array_equal(got_b.cpu().numpy(), want_b)
        alone = net.rotate_people(pts=pts, frame_hw=(1080, 1920), rotation_code=2)
        np.testing.assert_array_equal(alone.cpu().numpy().view(np.uint32), P.rotate_people(pts, None, (1080, 1920), 2).view(np.uint32))
        alone = net.rotate_people(boxes=boxes, frame_hw=(1080, 1920), rotation_code=0)
        np.testing.assert_array_equal(alone.cpu().numpy(), P.rotate_people(None, boxes, (1080, 1920), 0))


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_drawing_and_rotating_commute(fmt):
    """integer-valued joints: rotate(draw(f, pts)) == draw(rotate(f), rotate_people(pts)) -- discs and capsules are symmetric, and
    'the highest primitive wins' does not depend on the orientation"""
    pkg, net = load_pkg(), engine()
    h, w = 120, 168
    rng = np.random.default_rng(3)
    pts = np.stack([rng.integers(-6, h + 6, (6, 17)), rng.integers(-6, w + 6, (6, 17)), rng.uniform(0.3, 1.0, (6, 17))], 2).astype(np.float32)
    data = noise((h, w, 3), 8) if fmt == "bgr" else noise(yuv_ref.nbytes(h, w), 9)

    def fresh():
        return torch.from_numpy(data.copy()).cuda() if fmt == "bgr" else pkg.YuvFrame(torch.from_numpy(data.copy()).cuda(), h, w, "nv12")

    raw = lambda f: (f if fmt == "bgr" else f.data).cpu().numpy()   # noqa: E731
    drawn = net.draw_poses(fresh(), pts, COCO, radius=3, thickness=3)
    assert not np.array_equal(raw(drawn), data)
    for code in (0, 1, 2):
        a = net.rotate_frames(drawn, code)
        turned_pts = net.rotate_people(pts=pts, frame_hw=(h, w), rotation_code=code)
        b = net.draw_poses(net.rotate_frames(fresh(), code), turned_pts, COCO, radius=3, thickness=3)
        np.testing.assert_array_equal(raw(a), raw(b), err_msg="code %d" % code)


def test_refusals_leave_the_destination_alone():
    net = engine()
    f = torch.from_numpy(noise((40, 56, 3), 1)).cuda()
    g = torch.from_numpy(noise((40, 56, 3), 2)).cuda()
    before = f.clone()
    with pytest.raises(RuntimeError, match="in-place rotation is not offered"):
        net.rotate_frames(f, 1, out=f)
    assert torch.equal(f, before)
    d = torch.full((40, 56, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="name the same destination"):
        net.rotate_frames([f, g], 1, out=[d, d])
    with pytest.raises(RuntimeError, match="the rotated size is 56 x 40"):
        net.rotate_frames(f, 0, out=d)
    for bad in (3, -1, [0, 1], 1.0):
        with pytest.raises(ValueError):
            net.rotate_frames(f, bad, out=d)
    with pytest.raises(ValueError, match="engine's device"):
        net.rotate_frames(f, 1, out=np.zeros((40, 56, 3), np.uint8))
    with pytest.raises(ValueError):
        net.rotate_frames([f, g], 1, out=[d])
    torch.cuda.synchronize()
    assert bool((d == SENTINEL).all()) and torch.equal(f, before)
