"""NV21 and 10-bit (P010 / I010) input on the GPU: ``yuv_to_bgr`` against the numpy restatement (tests/yuv10_ref.py), the 10-bit
path against the shipped 8-bit kernels on frames both can express, and every entry that accepts a ``YuvFrame`` against the same
entry on the restatement's BGR frame -- bit for bit, no tolerance anywhere.  Frames are random in every sample and in the six
ignored bits of every 10-bit word."""
import numpy as np
import pytest
import torch

import yuv10_ref
import yuv_ref
from conftest import load_pkg, state_dict_np
from test_yuv_gpu import FRAME_BOXES, people

pytestmark = pytest.mark.gpu

TABLE_KEYS = [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")]
NEW = ["nv21", "p010", "i010"]
H, W = 64, 96
POISON = 0x5A


def padded_pitch(fmt, width, extra=12):
    """a pitch with padding: a multiple of 4 for the 10-bit layouts (i010 needs it)"""
    return (yuv10_ref.row_bytes(width, fmt) + extra + 3) // 4 * 4


def make(pkg, height, width, fmt, key, seed, pitch=None):
    """(YuvFrame on the host, the restatement's BGR frame of it): random samples, random junk in the ignored bits"""
    rng = np.random.default_rng(seed)
    if fmt in ("nv12", "i420"):
        data = rng.integers(0, 256, yuv_ref.nbytes(height, width, pitch), dtype=np.uint8)
    else:
        data = yuv10_ref.pack(*yuv10_ref.random_samples(rng, height, width, fmt), fmt, pitch, junk=rng, fill=int(rng.integers(0, 256)))
    frame = yuv10_ref.frame(pkg, data, height, width, fmt, key[0], key[1], pitch)
    return frame, yuv10_ref.any_yuv_to_bgr(data, height, width, fmt, key[0], key[1], pitch)


def resident(pkg, frame, offset):
    """`frame` on the device, its bytes `offset` bytes behind a 256-byte boundary, poison around them"""
    buf = torch.full((frame.nbytes + 64,), POISON, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[offset:offset + frame.nbytes] = frame.data.cuda()
    return yuv10_ref.clone(pkg, frame, buf[offset:offset + frame.nbytes])


@pytest.fixture(scope="module")
def net32():
    net = load_pkg().NativeHRNet(32, 17, (H, W), "fp32", max_batch=4, device=0)
    yield net
    net.close()


# ------------------------------------------------------------------------------------------------------ 1. whole frames
@pytest.mark.parametrize("key", TABLE_KEYS, ids=["%s-%s" % k for k in TABLE_KEYS])
@pytest.mark.parametrize("fmt", NEW)
def test_yuv_to_bgr_equals_the_restatement(net32, fmt, key):
    """34 x 46: full runs of four pixels plus the run of two; a padded pitch; junk in the ignored bits; the buffer on a dword (the
    dword loads -- for i010 at pitch 100 every other chroma row is off a dword) and 2 bytes behind one (the 16-bit loads)"""
    pkg = load_pkg()
    h, w = 34, 46
    pitch = {"nv21": 64, "p010": 104, "i010": 100}[fmt]
    frame, want = make(pkg, h, w, fmt, key, 1000 + TABLE_KEYS.index(key), pitch)
    for offset in (0, 2):
        got = net32.yuv_to_bgr(resident(pkg, frame, offset))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3) and got.is_cuda and got.is_contiguous()
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=str((fmt, key, offset)))
    np.testing.assert_array_equal(net32.yuv_to_bgr(frame).cpu().numpy(), want)          # a host frame is uploaded
    packed, want = make(pkg, 2, 2, fmt, key, 1100)                                       # the smallest frame, no pitch
    np.testing.assert_array_equal(net32.yuv_to_bgr(packed).cpu().numpy(), want)


# ------------------------------------------------------------------------------- 2. the 10-bit path contains the 8-bit path
@pytest.mark.parametrize("pair", [("nv12", "p010", 8), ("i420", "i010", 2)], ids=["nv12-p010", "i420-i010"])
def test_the_10bit_kernels_contain_the_8bit_kernels(net32, pair):
    """an 8-bit frame and its 10-bit twin (every byte shifted into a word: samples x 4): the shipped 8-bit kernels and the 10-bit
    ones give the same BGR frame and the same crops"""
    pkg = load_pkg()
    fmt8, fmt10, shift = pair
    h, w = 120, 160
    for k, key in enumerate(TABLE_KEYS):
        data = np.random.default_rng(2000 + k).integers(0, 256, yuv_ref.nbytes(h, w), dtype=np.uint8)
        twin = data.astype(np.uint16) << shift
        f8, f10 = pkg.YuvFrame(data, h, w, fmt8, *key), pkg.YuvFrame(twin, h, w, fmt10, *key)
        assert f10.nbytes == 2 * f8.nbytes
        want = net32.yuv_to_bgr(f8)
        assert torch.equal(net32.yuv_to_bgr(f10), want), (pair, key)
        np.testing.assert_array_equal(want.cpu().numpy(), yuv_ref.yuv_to_bgr(data, h, w, fmt8, *key))
        variant = ("pad", "clamp")[k % 2]
        a, b = net32.preprocess_frame(f8, FRAME_BOXES, variant), net32.preprocess_frame(f10, FRAME_BOXES, variant)
        assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and torch.equal(a[2], b[2]), (pair, key, variant)


# ------------------------------------------------------------------------------------------------------------ 3. crops
@pytest.mark.parametrize("variant", ["pad", "clamp"])
@pytest.mark.parametrize("fmt", NEW)
def test_preprocess_frame_equals_the_bgr_path(net32, fmt, variant):
    """FRAME_BOXES holds the w_pad == W shortcut and real horizontal passes (test_yuv_gpu checks that); people() adds boxes on
    every frame edge, whose padded crops run past it"""
    pkg = load_pkg()
    for k, key in enumerate(TABLE_KEYS):
        pitch = (None, padded_pitch(fmt, 160, 32))[k % 2]
        frame, bgr = make(pkg, 120, 160, fmt, key, 3000 + k, pitch)
        for dets in (FRAME_BOXES, people(120, 160, 14, 3100 + k)):
            want = net32.preprocess_frame(bgr, dets, variant)
            got = net32.preprocess_frame(frame, dets, variant)
            assert tuple(got[0].shape) == (len(dets), 3, H, W) and got[0].dtype == torch.float32
            assert torch.equal(got[0], want[0]), (fmt, key, variant)
            assert np.array_equal(got[1], want[1]) and torch.equal(got[2], want[2])
        again = net32.preprocess_frame(net32.yuv_to_bgr(frame), FRAME_BOXES, variant)   # the device's own conversion, once more
        assert torch.equal(again[0], net32.preprocess_frame(bgr, FRAME_BOXES, variant)[0])


# -------------------------------------------------------------------------------------------------------- 4. clip mode
def five_frames(pkg):
    """five sizes, five formats, all four tables.  The first is NV12 with pitch 47 and height 34: 2397 bytes, an odd count -- the
    P010 frame behind it must still start on an even address in predict_clip's upload arena."""
    spec = [(34, 46, "nv12", TABLE_KEYS[0], 47, 3), (120, 160, "p010", TABLE_KEYS[2], None, 4), (96, 132, "nv21", TABLE_KEYS[1], 140, 2),
            (150, 90, "i010", TABLE_KEYS[3], 192, 3), (64, 100, "i420", TABLE_KEYS[0], None, 2)]
    frames, bgrs, dets = [], [], []
    for k, (h, w, fmt, key, pitch, count) in enumerate(spec):
        f, b = make(pkg, h, w, fmt, key, 4000 + k, pitch)
        frames.append(f), bgrs.append(b), dets.append(people(h, w, count, 4100 + k))
    assert frames[0].nbytes % 2 == 1 and [yuv10_ref.layout(f) for f in frames] == ["nv12", "p010", "nv21", "i010", "i420"]
    return frames, bgrs, dets


@pytest.mark.parametrize("variant", ["pad", "clamp"])
def test_preprocess_frames_mixes_the_five_formats(net32, variant):
    pkg = load_pkg()
    frames, bgrs, dets = five_frames(pkg)
    singles = [net32.preprocess_frame(f, d, variant) for f, d in zip(frames, dets)]
    want = (torch.cat([s[0] for s in singles]), np.concatenate([s[1] for s in singles]), torch.cat([s[2] for s in singles]))
    bgr_want = net32.preprocess_frames(bgrs, dets, variant)
    for given in (frames, [f.to("cuda") for f in frames]):
        got = net32.preprocess_frames(given, dets, variant)
        assert got[3] == [3, 4, 2, 3, 2]
        for g, w, b in zip(got[:3], want, bgr_want[:3]):
            assert (torch.equal(g, w) and torch.equal(g, b)) if isinstance(g, torch.Tensor) else (np.array_equal(g, w) and np.array_equal(g, b))


def test_predict_clip_from_host_frames_equals_predict_frames():
    pkg = load_pkg()
    net = pkg.NativeHRNet(32, 17, (H, W), "bf16", max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    frames, bgrs, dets = five_frames(pkg)
    want = net.predict_frames(bgrs, dets, return_heatmaps=True)
    got = net.predict_frames([f.to("cuda") for f in frames], dets, return_heatmaps=True)
    pinned = [(yuv10_ref.clone(pkg, f, f.data.pin_memory()), d) for f, d in zip(frames, dets)]
    clip = list(net.predict_clip(iter(pinned), people_per_pass=8, return_heatmaps=True))
    torch.cuda.synchronize()
    assert len(got) == len(clip) == len(want) == 5
    for k, w in enumerate(want):
        for res in (got[k], clip[k]):
            assert res[0].dtype == np.int32 and np.array_equal(res[0], w[0]), k
            assert torch.equal(res[1], w[1]) and torch.equal(res[2], w[2]), k
    net.close()


# ----------------------------------------------------------------------------------------------------- 5. tracking link
@pytest.mark.parametrize("variant", ["pad", "clamp"])
def test_preprocess_frames_dev_on_a_p010_frame(net32, variant):
    pkg = load_pkg()
    frame, _ = make(pkg, 120, 160, "p010", TABLE_KEYS[2], 5000, 352)
    other, _ = make(pkg, 96, 132, "i010", TABLE_KEYS[1], 5001)
    dets = people(120, 160, 9, 5002)
    want_images, _, want_boxes = net32.preprocess_frame(frame, dets, variant)
    images, boxes, status = net32.preprocess_frames_dev(frame, torch.from_numpy(dets).cuda(), variant=variant)
    assert not status.any() and torch.equal(boxes, want_boxes) and torch.equal(images, want_images)
    # two frames, two 10-bit layouts, people in shuffled order
    d2 = people(96, 132, 5, 5003)
    rows, index = np.concatenate([dets[:5], d2]), np.asarray([0] * 5 + [1] * 5, np.int32)
    order = np.random.default_rng(5004).permutation(10)
    rows, index = np.ascontiguousarray(rows[order]), np.ascontiguousarray(index[order])
    host = net32.preprocess_frames([frame, other], [rows[index == 0], rows[index == 1]], variant)
    images, boxes, status = net32.preprocess_frames_dev([frame, other], torch.from_numpy(rows).cuda(), index, variant)
    back = np.concatenate([np.flatnonzero(index == 0), np.flatnonzero(index == 1)])   # preprocess_frames groups by frame
    assert not status.any() and torch.equal(images[back], host[0]) and torch.equal(boxes[back], host[2])


# --------------------------------------------------------------------------------------------------------- 6. letterbox
@pytest.mark.parametrize("style,size", [("yolov3", 64), ("yolov5", (64, 96))], ids=["yolov3", "yolov5"])
def test_detector_input_equals_the_bgr_path(net32, style, size):
    """per format one frame that is enlarged and one that is halved exactly (the 2 x 2 mean), in one call with the other formats"""
    pkg, P = load_pkg(), load_pkg("postproc")
    big = (128, 96) if style == "yolov3" else (128, 192)
    frames, bgrs = [], []
    for k, fmt in enumerate(NEW):
        for j, (h, w) in enumerate(((40, 52), big)):
            f, b = make(pkg, h, w, fmt, TABLE_KEYS[(k + j) % 4], 6000 + 10 * k + j, (None, padded_pitch(fmt, w))[j])
            frames.append(f), bgrs.append(b)
    g = P.letterbox_geometry(np.asarray([(f.height, f.width) for f in frames]), size, style)
    halved = (2 * g.new_h == [f.height for f in frames]) & (2 * g.new_w == [f.width for f in frames])
    assert halved.tolist() == [False, True] * 3 and (g.new_h[~halved] > 40).all()
    for dtype in (torch.uint8, torch.float32):
        got, _ = net32.detector_input(frames, size, style, dtype=dtype)
        want, _ = net32.detector_input(bgrs, size, style, dtype=dtype)
        assert got.dtype == dtype and torch.equal(got.view(torch.uint8), want.view(torch.uint8)), (style, dtype)
    one, _ = net32.detector_input(frames[3], size, style, dtype=torch.uint8, order="bgr")
    want, _ = net32.detector_input(bgrs[3], size, style, dtype=torch.uint8, order="bgr")
    assert torch.equal(one, want)


# ---------------------------------------------------------------------------------------------------------- 7. rotation
def rot(plane, code):
    return np.rot90(plane, {0: 3, 1: 2, 2: 1}[code])   # cv2.ROTATE_90_CLOCKWISE, _180, _90_COUNTERCLOCKWISE


@pytest.mark.parametrize("code", [0, 1, 2])
@pytest.mark.parametrize("fmt", NEW)
def test_rotation_is_a_permutation_of_elements(net32, fmt, code):
    """70 x 134: two tiles with a partial one on both axes of the Y plane.  Case A: buffers on a dword, padded pitches that are
    multiples of 4 (the dword path).  Case B: base and pitch 2 mod 4 (nv21: odd), where no dword may be used.  The destination is
    poisoned: its pitch padding must come back intact, its planes word for word np.rot90 of the source's -- ignored bits included."""
    pkg = load_pkg()
    h, w = 70, 134
    rh, rw = (h, w) if code == 1 else (w, h)
    row, rrow = yuv10_ref.row_bytes(w, fmt), yuv10_ref.row_bytes(rw, fmt)
    rng = np.random.default_rng(7000 + code)
    for case, offset in enumerate((0, 2)):
        spitch, dpitch = (row + 20 + 3) // 4 * 4, (rrow + 24 + 3) // 4 * 4
        if case == 1:    # off the dword: pitch 2 mod 4 where the layout allows it (i010's pitch is a multiple of 4: its base moves)
            spitch, dpitch = (spitch + 2, dpitch + 2) if fmt == "p010" else (spitch + 1, dpitch + 1) if fmt == "nv21" else (spitch, dpitch)
        for p, r in ((spitch, row), (dpitch, rrow)):
            assert p >= r and (fmt == "nv21" or p % (4 if fmt == "i010" else 2) == 0)
        src_bytes = yuv10_ref.pack(*yuv10_ref.random_samples(rng, h, w, fmt), fmt, spitch, junk=rng, fill=0xC3)
        Y, U, V = yuv10_ref.planes(src_bytes, h, w, fmt, spitch)
        want = yuv10_ref.pack_elements(rot(Y, code), rot(U, code), rot(V, code), fmt, dpitch, fill=POISON)
        src = resident(pkg, yuv10_ref.frame(pkg, src_bytes, h, w, fmt, "bt709", "limited", spitch), offset)
        dst = resident(pkg, yuv10_ref.frame(pkg, np.full(len(want), POISON, np.uint8), rh, rw, fmt, "bt709", "limited", dpitch), offset)
        assert src.data.data_ptr() % 4 == offset and dst.data.data_ptr() % 4 == offset
        back = net32.rotate_frames(src, code, out=dst)
        assert back is dst
        got = dst.data.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, "%s code %d case %d: %d bytes differ, first at %d" % (fmt, code, case, len(bad), bad[0])
        np.testing.assert_array_equal(src.data.cpu().numpy(), src_bytes)                     # the source is only read
        # a fresh destination: no padding, the same elements; and the conversion commutes with the rotation
        fresh = net32.rotate_frames(src, code)
        assert (fresh.height, fresh.width, fresh.pitch, yuv10_ref.layout(fresh)) == (rh, rw, rrow, fmt)
        np.testing.assert_array_equal(fresh.data.cpu().numpy(), yuv10_ref.pack_elements(rot(Y, code), rot(U, code), rot(V, code), fmt))
        np.testing.assert_array_equal(net32.yuv_to_bgr(fresh).cpu().numpy(), rot(net32.yuv_to_bgr(src).cpu().numpy(), code))
        np.testing.assert_array_equal(net32.yuv_to_bgr(dst).cpu().numpy(), rot(yuv10_ref.yuv_to_bgr(src_bytes, h, w, fmt, "bt709", "limited", spitch), code))
