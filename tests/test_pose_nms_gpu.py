"""Pose NMS on the GPU: NativeHRNet.pose_nms (engine layout) and the COCO-layout path of nms_eval against the host form, BIT FOR BIT
(both compile csrc/pose_nms_math.h): keep, num, the rescored scores, suppressor, status, and pts / boxes after `suppress`; the
reference's own fixtures through the device; and a three-frame track_frame -> pose_nms(suppress) -> draw_poses loop against the
same loop with the joints downloaded.

Shapes are the smallest that reach each branch of csrc/pose_nms.hip: nobody, one person, two identical people; 25 people under
soft NMS (the cap of 20); the cap on people (256: all four waves, long suppression chains beside many survivors); J = 17 / 16 /
133 (COCO's sigmas, given sigmas, numpy's pairwise recursion above 128 terms); four problems in one launch (the table upload)."""
import numpy as np
import pytest
import torch

import pose_nms_ref as R
from conftest import golden, load_pkg, state_dict_np

pytestmark = pytest.mark.gpu

_NETS = {}
NAMES = ("keep", "num", "scores", "suppressor", "status")
SKELETON = [[15, 13], [13, 11], [16, 14], [14, 12], [11, 12], [5, 11], [6, 12], [5, 6], [5, 7], [6, 8], [7, 9], [8, 10], [1, 2], [0, 1],
            [0, 2], [1, 3], [2, 4], [3, 5], [4, 6]]


def engine():
    if "net" not in _NETS:
        _NETS["net"] = load_pkg().NativeHRNet(32, 17, (64, 64), "fp32", max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    return _NETS["net"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same(got, want, what, names=NAMES):
    for name in names:
        g, w = got[name].cpu().numpy() if isinstance(got[name], torch.Tensor) else got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, name)


def both(pts, boxes, det=None, **kw):
    """(device results, host results) of one engine-layout call; the device gets tensors that already lie on the GPU"""
    want = load_pkg("postproc").pose_nms(pts.copy(), boxes.copy(), det, **kw)
    got = engine().pose_nms(torch.from_numpy(pts.copy()).cuda(), torch.from_numpy(boxes.copy()).cuda(),
                            None if det is None else torch.from_numpy(det).cuda(), **kw)
    assert all(t.is_cuda for t in got.values())
    return got, want


@pytest.mark.parametrize("soft", [False, True])
def test_nobody_one_person_and_twins(soft):
    one = R.clustered(1, 1, 17)
    for n, (pts, boxes, det) in ((0, R.clustered(0, 0, 17)), (1, one), (2, tuple(np.concatenate([v, v]) for v in one))):
        got, want = both(pts, boxes, det, thresh=0.9, soft=soft)
        assert_same(got, want, (n, soft), NAMES + ("pts", "boxes"))
        assert want["num"].tolist() == [min(n, 2 if soft else 1)]
    assert soft or want["suppressor"].tolist() == [-1, 0]                   # equal scores: the lower index is kept


def test_reference_fixtures_on_the_device():
    G = golden("tracking_cases")
    net = engine()
    for k in (int(v) for v in G["oks_cases"]):
        kpts, scores, areas = (np.ascontiguousarray(G["oks%d_%s" % (k, n)]) for n in ("kpts", "scores", "areas"))
        thresh, vis = float(G["oks%d_thresh" % k]), float(G["oks%d_vis" % k])
        vis = None if np.isnan(vis) else vis
        for soft, name in ((False, "keep"), (True, "soft_keep")):
            got = net._pose_nms_coco(kpts, areas, scores, None, thresh, vis, None, soft, None)
            want = load_pkg("postproc").pose_nms(kpts=kpts, areas=areas, scores=scores, thresh=thresh, in_vis_thre=vis, soft=soft)
            assert_same(got, want, (k, soft))
            assert got["keep"][:int(got["num"][0])].tolist() == G["oks%d_%s" % (k, name)].tolist(), (k, soft)


def test_soft_nms_reaches_the_cap_of_twenty():
    pts, boxes, det = R.clustered(25, 25, 17)
    got, want = both(pts, boxes, det, thresh=0.7, soft=True, in_vis_thre=0.2)
    assert_same(got, want, 25)
    assert want["num"].tolist() == [20] and (want["suppressor"] == -2).sum() == 5


@pytest.mark.parametrize("soft", [False, True])
def test_the_cap_on_people(soft):
    pts, boxes, det = R.clustered(256, 256, 17, groups=40)                  # 40 bodies, six or seven skeletons on each
    got, want = both(pts, boxes, det, thresh=0.5, soft=soft, rescore_thre=0.2)
    assert_same(got, want, (256, soft))
    if not soft:
        removed = np.bincount(want["suppressor"][want["suppressor"] >= 0], minlength=256)
        print("kept %d of 256; the longest chain removes %d" % (int(want["num"][0]), int(removed.max())))
        assert 30 <= int(want["num"][0]) <= 200 and removed.max() >= 4      # many survivors beside long suppression chains


@pytest.mark.parametrize("n,J", [(40, 133), (12, 16), (9, 129), (6, 255)])
def test_given_sigmas_and_the_pairwise_recursion(n, J):
    pts, boxes, det = R.clustered(n + J, n, J)
    sigmas = R.random_sigmas(J, J)
    for soft in (False, True):
        got, want = both(pts, boxes, det, thresh=0.5, soft=soft, sigmas=sigmas)
        assert_same(got, want, (n, J, soft))
        assert int(want["num"][0]) == min(n, 20) if soft else 1 <= int(want["num"][0]) < n
    with pytest.raises(RuntimeError, match="sigmas"):
        engine().pose_nms(pts, boxes, det)


@pytest.mark.parametrize("soft", [False, True])
def test_four_problems_in_one_launch_equal_four_calls(soft):
    shapes = [0, 1, 25, 256]
    parts = [R.clustered(300 + k, n, 17, groups=30 if n > 100 else None) for k, n in enumerate(shapes)]
    cat = [np.concatenate([p[k] for p in parts]) for k in range(3)]
    got, want = both(*cat, counts=shapes, thresh=0.6, soft=soft, suppress=True)
    assert_same(got, want, ("segments", soft), NAMES + ("pts", "boxes"))
    single = [both(*p, thresh=0.6, soft=soft, suppress=True)[0] for p in parts]
    for name in NAMES + ("pts", "boxes"):
        assert torch.equal(got[name], torch.cat([s[name] for s in single])), name


@pytest.mark.parametrize("soft", [False, True])
def test_rescoring_with_and_without_detection_scores(soft):
    pts, boxes, det = R.clustered(44, 30, 17)
    pts[3, :, 2] = 0.1                                                      # nobody above the threshold: score 0
    for d in (det, None):
        got, want = both(pts, boxes, d, thresh=0.6, in_vis_thre=0.3, rescore_thre=0.2, soft=soft)
        assert_same(got, want, (soft, d is None))
        assert want["scores"][3] == 0.0 and not np.array_equal(want["scores"], np.ones(30) if d is None else det.astype(np.float64))
    # host arrays are uploaded
    up = engine().pose_nms(pts, boxes, det, thresh=0.6, rescore_thre=0.2, soft=soft)
    assert_same(up, load_pkg("postproc").pose_nms(pts.copy(), boxes.copy(), det, thresh=0.6, rescore_thre=0.2, soft=soft), "uploaded")


@pytest.mark.parametrize("soft", [False, True])
def test_ties_and_a_nan_score(soft):
    pts, boxes, det = R.tie_case()
    got, want = both(pts, boxes, det, thresh=0.5, in_vis_thre=0.1, soft=soft)
    assert_same(got, want, soft)
    assert want["status"].tolist() == [1]
    # a non-finite OKS: COCO layout with areas that make the denominator zero
    kpts, areas, scores = R.engine_to_coco(*R.clustered(3, 4, 17))
    areas[:] = -np.spacing(1)
    kpts[1] = kpts[0]
    got = engine()._pose_nms_coco(kpts, areas, scores, None, 0.5, None, None, soft, None)
    want = load_pkg("postproc").pose_nms(kpts=kpts, areas=areas, scores=scores, thresh=0.5, soft=soft)
    assert_same(got, want, "non-finite")
    assert int(want["status"][0]) & 2


@pytest.mark.parametrize("soft,n", [(False, 12), (True, 25)])
def test_suppress_is_byte_equal_outside_the_suppressed_people(soft, n):
    pts, boxes, det = R.clustered(8 + n, n, 17)
    given = torch.from_numpy(pts.copy()).cuda(), torch.from_numpy(boxes.copy()).cuda()
    got = engine().pose_nms(given[0], given[1], torch.from_numpy(det).cuda(), thresh=0.5, soft=soft, suppress=True)
    want = load_pkg("postproc").pose_nms(pts.copy(), boxes.copy(), det, thresh=0.5, soft=soft, suppress=True)
    assert got["pts"].data_ptr() == given[0].data_ptr() and got["boxes"].data_ptr() == given[1].data_ptr()      # in place
    assert_same(got, want, (soft, n), NAMES + ("pts", "boxes"))
    gone = want["suppressor"] != -1
    assert gone.any() and (~gone).any()
    p2, b2 = given[0].cpu().numpy(), given[1].cpu().numpy()
    assert np.array_equal(bits(p2[~gone]), bits(pts[~gone])) and np.array_equal(b2[~gone], boxes[~gone])
    assert np.array_equal(bits(p2[gone][:, :, :2]), bits(pts[gone][:, :, :2]))
    assert (p2[gone][:, :, 2] == 0).all() and (b2[gone] == 0).all()


def test_side_streams_and_the_call_guard():
    shapes = [3, 0, 25, 9]
    parts = [R.clustered(500 + k, n, 17) for k, n in enumerate(shapes)]
    cat = [np.concatenate([p[k] for p in parts]) for k in range(3)]
    pp = load_pkg("postproc")
    for k, soft in enumerate((False, True, False)):                         # a side stream, a second one, and the first again
        stream = _NETS.setdefault("streams", [torch.cuda.Stream(), torch.cuda.Stream()])[k % 2]
        with torch.cuda.stream(stream):
            got, _ = both(*cat, counts=shapes, thresh=0.6, soft=soft)       # four problems: the table on the handle
            one, _ = both(*parts[2], thresh=0.6, soft=soft)                 # one problem: nothing on the handle
            got = {name: v.cpu() for name, v in got.items()}
            one = {name: v.cpu() for name, v in one.items()}
        assert_same(got, pp.pose_nms(cat[0].copy(), cat[1].copy(), cat[2], counts=shapes, thresh=0.6, soft=soft), ("stream", k))
        assert_same(one, pp.pose_nms(parts[2][0].copy(), parts[2][1].copy(), parts[2][2], thresh=0.6, soft=soft), ("stream", k, "one"))


def test_refusals_name_their_cause():
    net = engine()
    pts, boxes, det = R.clustered(6, 257, 17)
    with pytest.raises(RuntimeError, match="HRN_MAX_TRACKED"):
        net.pose_nms(pts, boxes, det)
    with pytest.raises(RuntimeError, match="thresh > 0"):
        net.pose_nms(pts[:5], boxes[:5], det[:5], thresh=0.0, soft=True)
    with pytest.raises(RuntimeError, match="finite"):
        net.pose_nms(pts[:5], boxes[:5], det[:5], thresh=float("nan"))


def test_nms_eval_on_the_device_equals_the_host_form(monkeypatch):
    pkg = load_pkg()
    net = engine()
    counts = [3, 1, 25, 8]
    parts = [R.clustered(200 + k, n, 17) for k, n in enumerate(counts)]
    kpts, areas, box_scores = R.engine_to_coco(*(np.concatenate([p[k] for p in parts]) for k in range(3)))
    image_index = np.repeat(np.asarray([900, 17, 5, 333]), counts)
    shuffle = np.random.default_rng(1).permutation(len(areas))
    args = (kpts[shuffle][:, :, :2], kpts[shuffle][:, :, 2:], areas[shuffle], box_scores[shuffle], image_index[shuffle])
    scores, kept = net.nms_eval(*args, oks_thre=0.7)

    def host_form(self, k, a, s, cnt, thresh, vis, rescore_thre, soft, sigmas):
        return load_pkg("postproc").pose_nms(kpts=k, areas=a, scores=s, counts=cnt, thresh=thresh, in_vis_thre=vis, rescore_thre=rescore_thre,
                                             soft=soft, sigmas=sigmas)

    monkeypatch.setattr(pkg.NativeHRNet, "_pose_nms_coco", host_form)
    want_scores, want = net.nms_eval(*args, oks_thre=0.7)
    assert np.array_equal(bits(scores), bits(want_scores)) and list(kept) == list(want)
    assert all(np.array_equal(kept[image], want[image]) for image in want)
    assert sum(len(v) for v in kept.values()) < len(areas)


def test_device_loop_equals_the_loop_through_the_host():
    """predict_frame on frame 0 from two copies of one detection plus another, then three frames of track_frame ->
    pose_nms(suppress=True) -> draw_poses on the device, against the same loop with the joints and boxes downloaded,
    postproc.pose_nms on the host and the result uploaded for the overlay.  A lost person stays lost: both loops zero the
    confidences of whoever track_frame reports with a status (its joints mean nothing)."""
    pp = load_pkg("postproc")
    net = engine()
    rng = np.random.default_rng(8)
    frames = [rng.integers(0, 256, (120, 160, 3), dtype=np.uint8) for _ in range(4)]
    dets = np.asarray([[10.2, 8.7, 90.4, 100.1], [10.2, 8.7, 90.4, 100.1], [60.5, 20.5, 150.0, 70.0]], np.float32)
    box_args = dict(threshold=0.0, min_joints=1)                            # a joint with confidence 0 is not live

    _, pts0 = net.predict_frame(torch.from_numpy(frames[0]).cuda(), dets)
    assert torch.equal(pts0[0], pts0[1])
    d_pts, h_pts = pts0, pts0.cpu().numpy()
    for k in (1, 2, 3):
        frame = torch.from_numpy(frames[k]).cuda()
        t_boxes, t_pts, t_status = net.track_frame(frame, d_pts, **box_args)
        t_pts[:, :, 2] *= (t_status == 0).to(t_pts.dtype)[:, None]
        out = net.pose_nms(t_pts, t_boxes, thresh=0.9, suppress=True)
        d_pts, d_boxes = out["pts"], out["boxes"]
        canvas = net.draw_poses(frame.clone(), d_pts, SKELETON, confidence_threshold=0.0)
        assert all(t.is_cuda for t in (d_pts, d_boxes, canvas, *(out[name] for name in NAMES)))
        # the same step through the host
        u_boxes, u_pts, u_status = (t.cpu().numpy() for t in net.track_frame(frame, torch.from_numpy(h_pts).cuda(), **box_args))
        u_pts[:, :, 2] *= (u_status == 0).astype(np.float32)[:, None]
        host = pp.pose_nms(u_pts, u_boxes, thresh=0.9, suppress=True)
        h_pts, h_boxes = host["pts"], host["boxes"]
        want = net.draw_poses(frame.clone(), h_pts, SKELETON, confidence_threshold=0.0)
        status = t_status.cpu().numpy()
        print("frame %d: status %s, suppressor %s" % (k, status.tolist(), host["suppressor"].tolist()))
        assert_same(out, host, k, NAMES + ("pts", "boxes"))
        assert np.array_equal(status, u_status) and torch.equal(canvas, want), k
        if k == 1:
            assert status.tolist()[:2] == [0, 0] and host["suppressor"].tolist()[:2] == [-1, 0]     # the copy falls to its twin
            assert not torch.equal(canvas, frame)                           # something was drawn
        else:
            assert status[1] != 0 and status[0] == 0                        # the duplicate stays lost, its twin lives on
        assert (h_pts[1, :, 2] == 0).all() and (h_boxes[1] == 0).all()
