"""COCO keypoint AP / AR on the GPU: NativeHRNet.keypoint_eval / hrn_keypoint_eval_dev against the host form, BIT FOR BIT for every
output (both compile csrc/keypoint_eval_math.h), with nothing left out.

Sizes are the smallest that reach each loop of csrc/keypoint_eval.hip: no image; one image with nothing, one pair, 20 x 256,
256 x 1 and 256 x 256 (detections x people: all four waves rank, the whole OKS matrix, the longest matchings); images with only
one side; slot totals 255 / 256 / 257 around the rank tile and the curve chunk; 300 images (about 5 000 slots: several tiles and
chunks); J = 1 / 17 / 133 / 256 (numpy's pairwise recursion above 8 and above 128 terms); 2 000 slots of one score (the tie order
across tiles)."""
import numpy as np
import pytest
import torch

import keypoint_eval_cases as C
from conftest import load_pkg, state_dict_np

pytestmark = pytest.mark.gpu

_NETS = {}
OUTPUTS = ("stats", "precision", "recall", "slot_person", "slot_score", "dt_match", "dt_ignore", "npig", "status")
INPUTS = ("dt_kpts", "dt_scores", "gt_kpts", "gt_area", "gt_bbox", "gt_iscrowd")


def engine():
    if "net" not in _NETS:
        _NETS["net"] = load_pkg().NativeHRNet(32, 17, (64, 64), "fp32", max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    return _NETS["net"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same(got, want, what):
    for name in OUTPUTS + ("images",):
        g = got[name].cpu().numpy() if isinstance(got[name], torch.Tensor) else got[name]
        w = want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, name)


def on_device(case):
    dtypes = dict(gt_iscrowd=torch.int32)
    return {k: torch.as_tensor(v, dtype=dtypes.get(k, torch.float64)).cuda() if k in INPUTS else v for k, v in case.items()}


def both(case, what):
    """the device call on tensors that already lie on the GPU against the host form"""
    want = load_pkg("postproc").keypoint_eval(**case)
    got = engine().keypoint_eval(**on_device(case))
    assert all(got[k].is_cuda for k in OUTPUTS)
    assert_same(got, want, what)
    return want


def test_no_image():
    want = both(C.make_set([], []), "P = 0")
    assert (want["stats"] == -1).all() and want["precision"].shape == (3, 10, 101) and (want["precision"] == -1).all()


@pytest.mark.parametrize("name", sorted(C.designed()))
def test_designed_sets(name):
    both(C.designed()[name], name)


@pytest.mark.parametrize("dt, gt", [(1, 1), (20, 256), (256, 1), (256, 256), (0, 5), (5, 0)])
def test_one_image(dt, gt):
    want = both(C.random_set(10 + dt + gt, counts=[(dt, gt)]), (dt, gt))
    assert want["slot_person"].shape == (min(dt, 20),)


def test_images_with_one_side_only_between_full_ones():
    want = both(C.random_set(3, counts=[(4, 3), (6, 0), (0, 5), (25, 2), (0, 1), (3, 0)]), "one-sided images")
    assert want["npig"].shape == (6, 3) and want["slot_person"].shape == (4 + 6 + 20 + 3,)


@pytest.mark.parametrize("slots", [255, 256, 257])
def test_slot_totals_around_the_tile_and_chunk_edge(slots):
    counts = [(25, 3)] * 12 + [(slots - 240, 2)]          # 12 images of 20 slots, one of 15 / 16 / 17
    want = both(C.random_set(slots, counts=counts), slots)
    assert want["slot_person"].shape == (slots,)


def test_three_hundred_images():
    rng = np.random.default_rng(0)
    dets = np.concatenate([rng.integers(0, 26, 60), rng.integers(12, 26, 240)])      # up to 25 per image, about 5 000 slots
    counts = list(zip(dets.tolist(), rng.integers(0, 8, 300).tolist()))
    want = both(C.random_set(300, counts=counts), "300 images")
    assert 4500 < len(want["slot_person"]) < 5500 and 0 < want["stats"][0] < 1


@pytest.mark.parametrize("joints", [1, 17, 133, 256])
def test_joint_counts_and_custom_sigmas(joints):
    case = C.random_set(joints, joints, max_images=6)
    case["sigmas"] = np.linspace(.03, .2, joints)
    both(case, joints)


def test_two_thousand_slots_of_one_score():
    case = C.random_set(77, counts=[(20, 3)] * 100)
    case["dt_scores"][:] = 0.5
    want = both(case, "ties")
    # equal scores: image order, then the caller's order inside an image
    ids = case["dt_image"][want["slot_person"]]
    assert (np.diff(ids) >= 0).all() and all((np.diff(want["slot_person"][ids == i]) > 0).all() for i in np.unique(ids))


def test_nan_and_inf_inputs():
    case = C.random_set(41, counts=[(12, 4), (25, 6), (3, 3)])
    case["dt_scores"][[0, 7, 20]] = np.nan
    case["dt_scores"][[3, 9]] = np.inf, -np.inf
    case["dt_kpts"][2, 3, 0], case["dt_kpts"][11, 0, 1], case["dt_kpts"][15, 5, 0] = np.nan, np.inf, -np.inf
    case["gt_kpts"][1, 2, 1], case["gt_area"][2], case["gt_area"][5], case["gt_bbox"][7, 2] = np.nan, 0.0, -1.0, np.inf
    want = both(case, "nan / inf")
    assert (want["status"] & 1).any() and (want["status"] & 2).any() and np.isfinite(want["stats"]).all()


def test_side_stream_and_host_inputs():
    case = C.random_set(9, counts=[(25, 5)] * 14)
    want = load_pkg("postproc").keypoint_eval(**case)
    net = engine()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        first = net.keypoint_eval(**on_device(case))
        again = net.keypoint_eval(**on_device(case))      # the handle's scratch is reused behind the first call
    side.synchronize()
    assert_same(first, want, "side stream")
    assert_same(again, want, "side stream, again")
    assert_same(net.keypoint_eval(**case), want, "host inputs")   # arrays on the host are uploaded


def test_device_inputs_in_image_order_are_used_where_they_lie(monkeypatch):
    case = C.random_set(12, counts=[(5, 2), (7, 3), (2, 2)])
    for side in ("dt", "gt"):
        order = np.argsort(case[side + "_image"], kind="stable")
        for k in [k for k in case if k.startswith(side)]:
            case[k] = np.ascontiguousarray(case[k][order])
    dev = on_device(case)
    net, seen = engine(), []
    launch = net._launch
    monkeypatch.setattr(net, "_launch", lambda name, *a: (seen.append((name, a)), launch(name, *a))[1])
    got = net.keypoint_eval(**dev)
    assert_same(got, load_pkg("postproc").keypoint_eval(**case), "resident")
    assert seen[0][0] == "hrn_keypoint_eval_dev" and list(seen[0][1][4:10]) == [dev[k].data_ptr() for k in INPUTS]   # no copy was made


# ---- refusals: code 7, the message on the handle, sentinel-filled outputs intact ------------------------------------------------------
def raw_call(P=1, dt_start=(0, 1), gt_start=(0, 1), J=17, null=(), sigmas=False):
    net = engine()
    n = 300
    dt_start, gt_start = np.array(dt_start, np.int32), np.array(gt_start, np.int32)
    arrays = dict(dt_kpts=torch.zeros((n, 256, 3), dtype=torch.float64), dt_scores=torch.zeros(n, dtype=torch.float64),
                  gt_kpts=torch.ones((n, 256, 3), dtype=torch.float64), gt_area=torch.ones(n, dtype=torch.float64),
                  gt_bbox=torch.ones((n, 4), dtype=torch.float64), gt_iscrowd=torch.zeros(n, dtype=torch.int32))
    arrays = {k: v.cuda() for k, v in arrays.items()}
    sg = torch.full((256,), .5, dtype=torch.float64).cuda()
    fill = lambda count, dtype: torch.full((count,), 7, dtype=dtype).cuda()   # noqa: E731
    outs = dict(stats=fill(10, torch.float64), precision=fill(3030, torch.float64), recall=fill(30, torch.float64),
                slot_person=fill(n, torch.int32), slot_score=fill(n, torch.float64), dt_match=fill(30 * n, torch.int32),
                dt_ignore=fill(30 * n, torch.uint8), npig=fill(24, torch.int32), status=fill(8, torch.int32))
    ptr = lambda name, v: None if name in null else v.data_ptr()   # noqa: E731
    rc = net._lib.hrn_keypoint_eval_dev(net._h, P, None if "dt_start" in null else dt_start.ctypes.data,
                                        None if "gt_start" in null else gt_start.ctypes.data, J, *[ptr(k, v) for k, v in arrays.items()],
                                        sg.data_ptr() if sigmas else None, *[ptr(k, v) for k, v in outs.items()],
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if rc == 0 and not null:   # an accepted call equals the host form on the same arguments
        host = {k: v.cpu().numpy() for k, v in outs.items()}
        S = int(np.minimum(np.diff(dt_start), 20).sum())
        inputs, sg_host = [v.cpu().numpy() for v in arrays.values()], sg.cpu().numpy()
        assert load_pkg("_lib").load().hrn_keypoint_eval(P, dt_start.ctypes.data, gt_start.ctypes.data, J, *[v.ctypes.data for v in inputs],
                                                         sg_host.ctypes.data if sigmas else None, *[v.ctypes.data for v in host.values()]) == 0
        for k, v in outs.items():
            count = {"slot_person": S, "slot_score": S, "npig": 3 * P, "status": P}.get(k, len(host[k]))
            if k in ("dt_match", "dt_ignore"):   # (3, 10, S) packed at the front of the buffer
                count = 30 * S
            assert np.array_equal(bits(v.cpu().numpy()[:count]), bits(host[k][:count])), k
    return rc, net._lib.hrn_last_error(net._h).decode(), all(bool((v == 7).all()) for v in outs.values())


@pytest.mark.parametrize("kwargs, message", [
    (dict(J=0, sigmas=True), "J must be in [1, HRN_MAX_JOINTS]"),
    (dict(J=257, sigmas=True), "J must be in [1, HRN_MAX_JOINTS]"),
    (dict(J=16), "the default sigmas are COCO's 17: pass sigmas for another J"),
    (dict(P=2, dt_start=(0, 2, 1), gt_start=(0, 1, 2)), "a segment table decreases"),
    (dict(dt_start=(0, 257)), "more than HRN_MAX_TRACKED detections in one image"),
    (dict(gt_start=(0, 257)), "more than HRN_MAX_TRACKED ground-truth people in one image"),
    (dict(null=("gt_start",)), "null segment tables / npig / status"),
    (dict(null=("recall",)), "null stats / precision / recall"),
    (dict(null=("dt_scores",)), "null detections / slot outputs"),
    (dict(null=("gt_iscrowd",)), "null ground truth"),
])
def test_refusals_leave_the_outputs_intact(kwargs, message):
    rc, text, untouched = raw_call(**kwargs)
    assert rc == 7 and text == "hrn_keypoint_eval_dev: " + message and untouched


def test_one_image_with_nothing_and_the_limits():
    rc, _, untouched = raw_call(dt_start=(0, 0), gt_start=(0, 0))          # P = 1, 0 x 0: launches, writes -1 everywhere
    assert rc == 0 and not untouched
    rc, _, untouched = raw_call(dt_start=(0, 256), gt_start=(0, 256), J=256, sigmas=True)
    assert rc == 0 and not untouched


# ---- the chain: predict_eval -> evaluate_overall_accuracy ------------------------------------------------------------------------------
def test_predict_eval_to_average_precision_equals_the_host_chain():
    net, P = engine(), load_pkg("postproc")
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, (3, 96, 128, 3), dtype=np.uint8)
    image_index = np.array([0, 1, 1, 2, 2, 2])
    centers = rng.uniform([30, 30], [98, 66], (6, 2)).astype(np.float32)
    scales = rng.uniform(.2, .4, (6, 2)).astype(np.float32)
    pairs = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
    preds, maxvals, _ = net.predict_eval(frames, centers, scales, pairs, frame_index=image_index)
    areas, box_scores = (scales[:, 0] * 200 * scales[:, 1] * 200).astype(np.float64), rng.uniform(.5, 1, 6)
    # ground truth: four of the predicted people, nudged; one of them a crowd
    who = [0, 1, 3, 5]
    gt_kpts = np.concatenate([preds[who].astype(np.float64) + rng.normal(0, 1.5, (4, 17, 2)), rng.integers(0, 3, (4, 17, 1))], axis=2)
    gt = dict(gt_kpts=gt_kpts, gt_area=areas[who] * .6, gt_bbox=np.concatenate([centers[who] - 30, np.full((4, 2), 60.0)], axis=1),
              gt_iscrowd=np.array([0, 0, 1, 0], np.int32), gt_image=image_index[who])
    got = net.evaluate_overall_accuracy(preds, maxvals, areas, box_scores, image_index, **gt)
    want = P.evaluate_overall_accuracy(preds, maxvals.cpu().numpy(), areas, box_scores, image_index, **gt)
    assert list(got[0]) == list(P.EVAL_STAT_NAMES) and got[1] == got[0]["AP"]
    assert [np.float64(v).tobytes() for v in got[0].values()] == [np.float64(v).tobytes() for v in want[0].values()]
    assert got[0]["AP"] > 0
