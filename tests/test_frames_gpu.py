"""Clip mode on the GPU: ``hrn_preprocess_frames`` / ``preprocess_frames`` / ``predict_frames`` / ``predict_clip`` and the stack
path of ``SimpleHRNet`` built on them.

Anchor: the Pillow restatement of ``oracle.prepath_oracle`` applied frame by frame (bit-exact).  Everything else is equality
with the calls clip mode replaces -- per-frame ``preprocess_frame`` + ``torch.cat`` + ``predict_crops`` -- with no tolerance
and no case left out."""
import numpy as np
import pytest
import torch

from conftest import golden, load_pkg, state_dict_np
from oracle import prepath_oracle as P
from test_frames_host import FRAME_SIZES, RESOLUTIONS, make_boxes
from test_prepath import DETS_BATCH
from test_simple_hrnet import TableDetector, _frames

pytestmark = pytest.mark.gpu


def noise_frame(hf, wf, seed):
    return np.random.default_rng(seed).integers(0, 256, (hf, wf, 3), dtype=np.uint8)


def people(hf, wf, count, seed):
    """`count` boxes of make_boxes' mix (random, half-integer, edge-touching), valid in both variants"""
    rng = np.random.default_rng(seed)
    boxes = make_boxes(rng, hf, wf, 16)
    return np.ascontiguousarray(boxes[rng.permutation(len(boxes))[:count]])


def per_frame_reference(net, frames, dets, variant):
    """the composition preprocess_frames replaces: one preprocess_frame per frame with people, concatenated"""
    outs = [net.preprocess_frame(f, d, variant) for f, d in zip(frames, dets) if d is not None and len(d)]
    if not outs:
        h, w = net.resolution
        return torch.zeros((0, 3, h, w), device=net.torch_device), np.zeros((0, 4), np.int32), torch.zeros((0, 4), dtype=torch.int32,
                                                                                                          device=net.torch_device)
    return torch.cat([o[0] for o in outs]), np.concatenate([o[1] for o in outs]), torch.cat([o[2] for o in outs])


def assert_same_prepath(got, want, counts=None, want_counts=None):
    assert torch.equal(got[0], want[0])
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1])
    assert got[2].dtype == torch.int32 and torch.equal(got[2], want[2])
    if want_counts is not None:
        assert list(counts) == list(want_counts)


# ------------------------------------------------------------------------------------------------------- the anchor
@pytest.mark.parametrize("variant", ["pad", "clamp"])
def test_three_frames_of_three_sizes_equal_the_oracle(variant):
    pkg = load_pkg()
    H, W = 64, 96
    sizes = [(120, 160), (97, 131), (150, 90)]
    frames = [noise_frame(hf, wf, 10 + k) for k, (hf, wf) in enumerate(sizes)]
    dets = [people(hf, wf, 4 + k, 20 + k) for k, (hf, wf) in enumerate(sizes)]
    ref = P.prepath if variant == "pad" else P.prepath_clamped
    want = [ref(f, d, H, W) for f, d in zip(frames, dets)]
    net = pkg.NativeHRNet(32, 17, (H, W), "fp32", max_batch=4, device=0)
    images, boxes, boxes_dev, counts = net.preprocess_frames(frames, dets, variant)
    assert counts == [4, 5, 6] and images.dtype == torch.float32 and tuple(images.shape) == (15, 3, H, W)
    np.testing.assert_array_equal(boxes, np.concatenate([w[1] for w in want]))
    np.testing.assert_array_equal(boxes_dev.cpu().numpy(), boxes)
    np.testing.assert_array_equal(images.cpu().numpy(), np.concatenate([w[0] for w in want]))
    net.close()


# ------------------------------------------------------------------------------------- equality with per-frame calls
@pytest.mark.parametrize("variant", ["pad", "clamp"])
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_preprocess_frames_equals_per_frame_calls(res, variant):
    pkg = load_pkg()
    net = pkg.NativeHRNet(32, 17, res, "bf16", max_batch=4, device=0)
    seed = 1000 * res[0] + (variant == "clamp")
    # F = 1, a host array and a device tensor
    hf, wf = FRAME_SIZES[2]
    frame, d = noise_frame(hf, wf, seed), people(hf, wf, 5, seed)
    want = per_frame_reference(net, [frame], [d], variant)
    assert_same_prepath(net.preprocess_frames([frame], [d], variant), want)
    got = net.preprocess_frames(torch.from_numpy(frame).cuda()[None], [d], variant)
    assert_same_prepath(got, want, got[3], [5])
    # F = 7 with mixed sizes; nobody in the first, a middle and the last frame (empty array and None)
    sizes = [FRAME_SIZES[k % 4] for k in range(7)] if res != (384, 288) else [FRAME_SIZES[k % 3] for k in range(7)]
    frames = [noise_frame(hf, wf, seed + 1 + k) for k, (hf, wf) in enumerate(sizes)]
    counts = [0, 3, 2, 0, 4, 1, 0]
    dets = [people(hf, wf, c, seed + 50 + k) if c else (None if k == 3 else np.zeros((0, 7), np.float32))
            for k, ((hf, wf), c) in enumerate(zip(sizes, counts))]
    want = per_frame_reference(net, frames, dets, variant)
    got = net.preprocess_frames(frames, dets, variant)
    assert_same_prepath(got, want, got[3], counts)
    # again on device-resident frames, the unused ones absent (None): scratch and staging are reused
    resident = [torch.from_numpy(f).cuda() if c else None for f, c in zip(frames, counts)]
    assert_same_prepath(net.preprocess_frames(resident, dets, variant), want)
    # a 4-D stack of equal frames, everybody present
    stack = np.stack([noise_frame(*FRAME_SIZES[0], seed + 80 + k) for k in range(3)])
    sdets = [people(*FRAME_SIZES[0], 2 + k, seed + 90 + k) for k in range(3)]
    want = per_frame_reference(net, list(stack), sdets, variant)
    assert_same_prepath(net.preprocess_frames(stack, sdets, variant), want)
    assert_same_prepath(net.preprocess_frames(torch.from_numpy(stack), sdets, variant), want)
    # nobody at all
    images, boxes, boxes_dev, c0 = net.preprocess_frames(frames[:2], [None, np.zeros((0, 4), np.float32)], variant)
    assert tuple(images.shape) == (0, 3) + res and boxes.shape == (0, 4) and tuple(boxes_dev.shape) == (0, 4) and c0 == [0, 0]
    net.close()


@pytest.mark.parametrize("variant", ["pad", "clamp"])
def test_people_in_interleaved_frame_order_through_the_c_entry(variant):
    pkg, lib = load_pkg(), load_pkg("_lib")
    H, W = 64, 96
    net = pkg.NativeHRNet(32, 17, (H, W), "fp32", max_batch=4, device=0)
    sizes = [(120, 160), (97, 131), (150, 90), (64, 64)]
    frames = [torch.from_numpy(noise_frame(hf, wf, 30 + k)).cuda() for k, (hf, wf) in enumerate(sizes)]
    dets = [people(hf, wf, 3, 40 + k) for k, (hf, wf) in enumerate(sizes[:3])]
    singles = [net.preprocess_frame(f, d, variant) for f, d in zip(frames, dets)]
    order = [(2, 1), (0, 0), (1, 2), (0, 2), (2, 0), (1, 0), (0, 1), (2, 2), (1, 1)]     # (frame, person of that frame)
    table = (lib.Frame * 4)()
    for k, f in enumerate(frames[:3]):                                                    # frame 3 stays null: nobody refers to it
        table[k].data, table[k].height, table[k].width = f.data_ptr(), f.shape[0], f.shape[1]
    all_dets = np.ascontiguousarray(np.stack([np.concatenate([dets[f][p], [0.9, 0.9, 0.0]]) for f, p in order]).astype(np.float32))
    fidx = np.asarray([f for f, _ in order], np.int32)
    n = len(order)
    images = torch.full((n, 3, H, W), float("nan"), device="cuda")
    boxes, boxes_dev = np.zeros((n, 4), np.int32), torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    rc = net._lib.hrn_preprocess_frames(net._h, table, 4, all_dets.ctypes.data, 7, fidx.ctypes.data, n, 0 if variant == "pad" else 1,
                                        images.data_ptr(), boxes.ctypes.data, boxes_dev.data_ptr(), net._stream())
    assert rc == 0, net._lib.hrn_last_error(net._h)
    torch.cuda.synchronize()
    for i, (f, p) in enumerate(order):
        assert torch.equal(images[i], singles[f][0][p]), (i, f, p)
        assert np.array_equal(boxes[i], singles[f][1][p]) and torch.equal(boxes_dev[i], singles[f][2][p])
    # NULL frame index: one frame, everybody is cut from it (and boxes_host / boxes_dev are optional)
    images1 = torch.empty((3, 3, H, W), device="cuda")
    rc = net._lib.hrn_preprocess_frames(net._h, table, 1, dets[0].ctypes.data, 4, None, 3, 0 if variant == "pad" else 1,
                                        images1.data_ptr(), None, None, net._stream())
    assert rc == 0 and torch.equal(images1, singles[0][0])
    # refused with nothing launched: an index outside the table, a person of the null frame, a box outside ITS frame
    images.fill_(7.0)
    for bad_idx in ([0, 4], [3, 0]):
        rc = net._lib.hrn_preprocess_frames(net._h, table, 4, all_dets.ctypes.data, 7, np.asarray(bad_idx, np.int32).ctypes.data, 2, 0,
                                            images.data_ptr(), None, None, net._stream())
        assert rc == 7
    wide = np.asarray([[100, 10, 150, 80]], np.float32)      # inside the 120x160 frame, starts outside the 150x90 one
    assert net._lib.hrn_preprocess_frames(net._h, table, 4, wide.ctypes.data, 4, np.asarray([0], np.int32).ctypes.data, 1, 0,
                                          images1.data_ptr(), None, None, net._stream()) == 0
    rc = net._lib.hrn_preprocess_frames(net._h, table, 4, wide.ctypes.data, 4, np.asarray([2], np.int32).ctypes.data, 1, 0,
                                        images.data_ptr(), None, None, net._stream())
    assert rc == 7 and b"detection 0 starts outside the frame" in net._lib.hrn_last_error(net._h)
    torch.cuda.synchronize()
    assert bool((images == 7.0).all())
    net.close()


# --------------------------------------------------------------------------------------------------- predict_frames
CLIP_SIZES = [(240, 320), (200, 150), (333, 517), (240, 320), (180, 400), (240, 320), (120, 160), (300, 300), (240, 320)]
CLIP_COUNTS = [3, 0, 4, 2, 5, 1, 0, 3, 2]


def make_items(sizes, counts, seed):
    frames = [noise_frame(hf, wf, seed + k) for k, (hf, wf) in enumerate(sizes)]
    dets = [people(hf, wf, c, seed + 100 + k) if c else (None if k % 2 else np.zeros((0, 4), np.float32))
            for k, ((hf, wf), c) in enumerate(zip(sizes, counts))]
    return frames, dets


def composed(net, native, frames, dets, variant, limit, **kw):
    """what predict_frames replaces, with its batch composition: per group of group_frames, preprocess_frame per frame + cat +
    predict_crops.  Returns per frame lists of (boxes, pts, hm or None) pieces."""
    counts = [0 if d is None else len(d) for d in dets]
    pieces = [[] for _ in frames]
    for group in native.group_frames(counts, limit):
        parts = [(f, net.preprocess_frame(frames[f], dets[f][lo:hi], variant)) for f, lo, hi in group if hi > lo]
        if not parts:
            continue
        out = net.predict_crops(torch.cat([p[1][0] for p in parts]), torch.cat([p[1][2] for p in parts]), **kw)
        hm, pts = out if kw.get("return_heatmaps") else (None, out)
        at = 0
        for f, (im, bx, _) in parts:
            pieces[f].append((bx, pts[at:at + len(bx)], None if hm is None else hm[at:at + len(bx)]))
            at += len(bx)
    return pieces


def assert_frame_results(net, results, pieces, return_heatmaps):
    J, (h, w) = net.nof_joints, net.resolution
    assert len(results) == len(pieces)
    for res, p in zip(results, pieces):
        assert len(res) == (3 if return_heatmaps else 2)
        boxes, pts = res[0], res[1]
        assert isinstance(boxes, np.ndarray) and boxes.dtype == np.int32 and pts.is_cuda and pts.dtype == torch.float32
        if not p:
            assert boxes.shape == (0, 4) and tuple(pts.shape) == (0, J, 3)
            if return_heatmaps:
                assert tuple(res[2].shape) == (0, J, h // 4, w // 4)
            continue
        assert np.array_equal(boxes, np.concatenate([x[0] for x in p]))
        assert torch.equal(pts, torch.cat([x[1] for x in p]))
        if return_heatmaps:
            assert torch.equal(res[2], torch.cat([x[2] for x in p]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_predict_frames_equals_the_composition_it_replaces(dtype):
    pkg, native = load_pkg(), load_pkg("native")
    net = pkg.NativeHRNet(32, 17, (128, 96), dtype, max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    frames, dets = make_items(CLIP_SIZES, CLIP_COUNTS, 7)
    assert len(list(native.group_frames(CLIP_COUNTS, 8))) == 3
    for variant in ("pad", "clamp"):
        for kw in (dict(), dict(return_heatmaps=True), dict(refine="dark"), dict(return_heatmaps=True, refine="dark")):
            want = composed(net, native, frames, dets, variant, 8, **kw)
            got = net.predict_frames(frames, dets, variant=variant, **kw)
            assert_frame_results(net, got, want, bool(kw.get("return_heatmaps")))
    # single-frame predict_frame calls: a crop's bits do not depend on what shares its pass
    for kw in (dict(return_heatmaps=True), dict(return_heatmaps=True, refine="dark")):
        got = net.predict_frames(frames, dets, **kw)
        for f, (frame, d) in enumerate(zip(frames, dets)):
            bx, pts, hm = net.predict_frame(frame, d if d is not None else np.zeros((0, 4), np.float32), **kw)
            assert np.array_equal(got[f][0], bx) and torch.equal(got[f][1], pts) and torch.equal(got[f][2], hm), (dtype, f, kw)
    net.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_frame_with_more_people_than_max_batch(dtype):
    pkg, native = load_pkg(), load_pkg("native")
    net = pkg.NativeHRNet(32, 17, (128, 96), dtype, max_batch=4, device=0).load_state_dict(state_dict_np(32, 0))
    sizes, counts = [(240, 320), (333, 517), (200, 150)], [2, 9, 3]
    frames, dets = make_items(sizes, counts, 11)
    assert [len(g) for g in native.group_frames(counts, 4)] == [1, 1, 1, 1, 1]       # 2 | 4 4 1 | 3: the big frame in three passes
    want = composed(net, native, frames, dets, "pad", 4, return_heatmaps=True)
    assert [len(p) for p in want] == [1, 3, 1]
    got = net.predict_frames(frames, dets, return_heatmaps=True)
    assert_frame_results(net, got, want, True)
    assert [len(r[1]) for r in got] == counts
    for f, (frame, d) in enumerate(zip(frames, dets)):
        bx, pts, hm = net.predict_frame(frame, d, return_heatmaps=True)
        assert np.array_equal(got[f][0], bx) and torch.equal(got[f][1], pts) and torch.equal(got[f][2], hm), (dtype, f)
    # the same through predict_clip: the big frame spans three groups and still comes out once, in its place
    items = [(torch.from_numpy(f).pin_memory(), d) for f, d in zip(frames, dets)]
    clip = list(net.predict_clip(items, return_heatmaps=True))
    torch.cuda.synchronize()
    assert_frame_results(net, clip, want, True)
    net.close()


# ----------------------------------------------------------------------------------------------------- predict_clip
def assert_clip_equals_frames(net, frames, dets, per_pass, **kw):
    resident = [torch.from_numpy(f).cuda() for f in frames]
    want = net.predict_frames(resident, dets, **kw)
    items = [(torch.from_numpy(f).pin_memory(), d) for f, d in zip(frames, dets)]
    got = []
    for k, res in enumerate(net.predict_clip(iter(items), people_per_pass=per_pass, **kw)):
        counts = 0 if dets[k] is None else len(dets[k])
        assert len(res[1]) == counts, "results arrive in frame order"
        got.append(res)
    torch.cuda.synchronize()
    assert len(got) == len(frames)
    for g, w in zip(got, want):
        assert len(g) == len(w) and np.array_equal(g[0], w[0])
        assert all(torch.equal(a, b) for a, b in zip(g[1:], w[1:]))
    return got


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_predict_clip_equals_predict_frames(dtype):
    pkg, native = load_pkg(), load_pkg("native")
    net = pkg.NativeHRNet(32, 17, (128, 96), dtype, max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    frames, dets = make_items(CLIP_SIZES, CLIP_COUNTS, 21)
    assert len(list(native.group_frames(CLIP_COUNTS, 8, 6))) >= 4                     # uneven groups: 3+0 | 4+2 | 5+1+0 | 3+2
    assert_clip_equals_frames(net, frames, dets, 6, return_heatmaps=True)
    # a second time on the same engine (the pre-path scratch and staging are reused), other options
    assert_clip_equals_frames(net, frames, dets, 6, variant="clamp", refine="dark")
    assert_clip_equals_frames(net, frames, dets, None)                                 # default: max_batch people per pass
    # larger frames: the arenas of a call grow with its groups (later groups hold bigger frames than the first)
    big_sizes = [(120, 160), (240, 320), (480, 640), (720, 1280), (333, 517), (1080, 1920), (240, 320)]
    big_counts = [2, 3, 3, 4, 1, 5, 2]
    big_frames, big_dets = make_items(big_sizes, big_counts, 33)
    assert_clip_equals_frames(net, big_frames, big_dets, 6, return_heatmaps=True)
    # numpy frames are taken as they are; an iterator that ends in the middle of a group; nobody anywhere; nothing at all
    got = list(net.predict_clip(((f, d) for f, d in zip(frames[:5], dets[:5])), people_per_pass=6))
    want = net.predict_frames(frames[:5], dets[:5])
    torch.cuda.synchronize()
    assert len(got) == 5 and all(np.array_equal(g[0], w[0]) and torch.equal(g[1], w[1]) for g, w in zip(got, want))
    got = list(net.predict_clip([(frames[0], None), (None, None), (frames[1], np.zeros((0, 7), np.float32))], return_heatmaps=True))
    assert len(got) == 3 and all(r[0].shape == (0, 4) and tuple(r[1].shape) == (0, 17, 3) and tuple(r[2].shape) == (0, 17, 32, 24)
                                 for r in got)
    assert list(net.predict_clip([])) == []
    # refusals: a device frame, more people per pass than the engine holds, a person of no frame
    with pytest.raises(TypeError, match="predict_frames"):
        list(net.predict_clip([(torch.from_numpy(frames[0]).cuda(), dets[0])]))
    with pytest.raises(ValueError, match="exceeds max_batch"):
        list(net.predict_clip(zip(frames, dets), people_per_pass=9))
    with pytest.raises(ValueError, match="is None but has"):
        list(net.predict_clip([(None, dets[0])]))
    net.close()


# ------------------------------------------------------------------------------------------------------ stack path
def test_stack_path_runs_on_preprocess_frames_and_equals_the_reference():
    """SimpleHRNet on a 4-D stack with an injected table detector against the arrays the unmodified reference's predict()
    returned (tests/golden/make_golden.py predict_cases), read again here"""
    pkg = load_pkg()
    frames = _frames()
    g = golden("w32_128x96_predict_batch_multi")
    model = pkg.SimpleHRNet(32, 17, state_dict_np(32, 0), resolution=(128, 96), multiperson=True, return_heatmaps=True,
                            return_bounding_boxes=True, device="cuda:0",
                            detector=TableDetector({0: DETS_BATCH[0], 1: None, 2: DETS_BATCH[2]}))
    calls = []
    engine_entry = model.model.preprocess_frames

    def spy(stack, dets, variant="pad"):
        out = engine_entry(stack, dets, variant)
        calls.append((len(stack), variant, out[0].clone(), out[3]))
        return out

    model.model.preprocess_frames = spy
    model.model.preprocess_frame = None          # the per-image entry is not what the stack path calls any more
    hm, boxes, pts = model.predict(frames[3])
    assert len(calls) == 1 and calls[0][:2] == (3, "clamp") and calls[0][3] == [2, 0, 1]
    np.testing.assert_array_equal(calls[0][2].cpu().numpy(), g["crops"])                 # the crops the reference fed its model
    assert [len(p) for p in pts] == list(g["counts"]) == [2, 0, 1]
    assert pts[1].shape == (0, 17, 3) and hm[1].shape == (0, 17, 32, 24) and boxes[1].shape == (0, 4)
    np.testing.assert_array_equal(np.concatenate(boxes, 0), g["boxes"])
    np.testing.assert_allclose(np.concatenate(hm, 0), g["heatmaps"], rtol=0, atol=2e-4)
    np.testing.assert_array_equal(np.concatenate(pts, 0)[..., :2], g["pts"][..., :2])
    np.testing.assert_allclose(np.concatenate(pts, 0)[..., 2], g["pts"][..., 2], rtol=0, atol=2e-4)
    # nobody in any image (:477-484): no engine call at all
    model.detector = TableDetector({})
    hm, boxes, pts = model.predict(frames[3])
    assert len(calls) == 1 and len(pts) == 3 and all(p.shape == (0, 17, 3) for p in pts) and boxes.shape == (0,)
    # the single-person stack of the second fixture does not pass through the crop pre-path and is unchanged
    g = golden("w48_128x96_predict_batch5")
    model = pkg.SimpleHRNet(48, 17, state_dict_np(48, 0), resolution=(128, 96), multiperson=False, return_heatmaps=True,
                            return_bounding_boxes=True, max_batch_size=2, device="cuda:0")
    hm, boxes, pts = model.predict(frames[2])
    assert pts.shape == g["pts"].shape == (5, 1, 17, 3)
    np.testing.assert_array_equal(boxes, g["boxes"])
    np.testing.assert_allclose(hm, g["heatmaps"], rtol=0, atol=2e-4)
    np.testing.assert_array_equal(pts[..., :2], g["pts"][..., :2])
