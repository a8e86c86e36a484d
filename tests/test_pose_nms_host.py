"""Pose NMS, host form (postproc.pose_nms / hrn_pose_nms, no GPU): against the reference's own outputs (tracking_cases.npz), against
the existing host functions hrn_oks_nms / hrn_soft_oks_nms fed the same stable order, and against the numpy restatement
(tests/pose_nms_ref.py) for what the existing functions do not have: rescoring, the engine layout, the order's definition, the
status bits, `suppress`, segments and the refusals.  NativeHRNet.nms_eval's grouping runs here too, with the device call replaced
by the host form."""
import ctypes

import numpy as np
import pytest

import pose_nms_ref as R
from conftest import golden, load_pkg


def pp():
    return load_pkg("postproc")


def lib_mod():
    return load_pkg("_lib")


def kept(out, first=0, p=0):
    return out["keep"][first:first + int(out["num"][p])].tolist()


def assert_equals_ref(out, want, what):
    assert kept(out) == want["keep"][:want["num"]].tolist(), what
    assert int(out["num"][0]) == want["num"] and int(out["status"][0]) == want["status"], what
    assert np.array_equal(out["keep"], want["keep"]) and np.array_equal(out["suppressor"], want["suppressor"]), what
    assert np.array_equal(out["scores"].view(np.uint64), want["scores"].view(np.uint64)), what


def test_symbols_and_sources():
    lib = lib_mod()
    names = ["hrn_pose_nms", "hrn_pose_nms_dev", "hrn_pose_nms_last_error", "hrn_pose_nms_oks_row"]
    assert all(n in lib.header_symbols() and n in lib.SYMBOLS for n in names)
    assert set(lib.header_symbols()) == set(lib.SYMBOLS)
    assert "pose_nms.hip" in lib.SOURCES
    assert all(hasattr(lib.load(), n) for n in names)


def test_reference_fixtures():
    G = golden("tracking_cases")
    worst = 0.0
    for k in (int(v) for v in G["oks_cases"]):
        kpts, scores, areas = (G["oks%d_%s" % (k, n)] for n in ("kpts", "scores", "areas"))
        thresh, vis = float(G["oks%d_thresh" % k]), float(G["oks%d_vis" % k])
        vis = None if np.isnan(vis) else vis
        hard = pp().pose_nms(kpts=kpts, areas=areas, scores=scores, thresh=thresh, in_vis_thre=vis)
        soft = pp().pose_nms(kpts=kpts, areas=areas, scores=scores, thresh=thresh, in_vis_thre=vis, soft=True)
        assert kept(hard) == G["oks%d_keep" % k].tolist(), k
        assert kept(soft) == G["oks%d_soft_keep" % k].tolist(), k
        assert hard["status"].tolist() == [0] and soft["status"].tolist() == [0]
        assert np.array_equal(hard["scores"], scores)                       # rescoring off: the scores as given
        row, want = pp().pose_nms_oks_row(kpts, areas, 0, in_vis_thre=vis), G["oks%d_oks_row0" % k]
        rel = float(np.max(np.abs(row - want) / np.abs(want)))
        worst = max(worst, rel)
        assert rel <= 1e-14, (k, rel)
    print("largest relative distance of an OKS of row 0 from the reference's: %.3g" % worst)


def _existing(kpts, areas, scores, thresh, vis, sigmas, soft):
    """hrn_oks_nms / hrn_soft_oks_nms with the STABLE order (postproc.oks_nms would take numpy's argsort()[::-1])"""
    lib = lib_mod().load()
    n, J = len(areas), kpts.shape[1]
    order = np.asarray(R.stable_order(scores), np.int32)
    keep, num = np.zeros(max(n, 20), np.int32), ctypes.c_int32(0)
    sg = None if sigmas is None else np.ascontiguousarray(sigmas, np.float64)
    nan = float("nan") if vis is None else float(vis)
    if soft:
        sorted_scores = np.ascontiguousarray(scores[order], np.float64)
        rc = lib.hrn_soft_oks_nms(keep.ctypes.data, ctypes.byref(num), kpts.ctypes.data, areas.ctypes.data, sorted_scores.ctypes.data,
                                  order.ctypes.data, n, J, float(thresh), None if sg is None else sg.ctypes.data, nan)
    else:
        rc = lib.hrn_oks_nms(keep.ctypes.data, ctypes.byref(num), kpts.ctypes.data, areas.ctypes.data, order.ctypes.data, n, J,
                             float(thresh), None if sg is None else sg.ctypes.data, nan)
    assert rc == 0
    return keep[:num.value].tolist()


def test_random_cases_equal_the_existing_host_functions():
    rng = np.random.default_rng(2024)
    left_out = compared = 0
    for case in range(300):
        n = int(rng.integers(0, 41))
        J = (17, 16, 133)[case % 3]
        sigmas = None if J == 17 else R.random_sigmas(case, J)
        thresh = float(rng.uniform(0.3, 0.9))
        vis = None if case % 2 else float(rng.uniform(0.1, 0.5))
        pts, boxes, det = R.clustered(1000 + case, n, J)
        kpts, areas, scores = R.engine_to_coco(pts, boxes, det)
        edge = False
        for soft in (False, True):
            ref = R.pose_nms(kpts, areas, scores, thresh, vis, None, soft, sigmas)
            if ref["gap"] < (1e-12 if soft else 1e-9):
                edge = True
                continue
            out = pp().pose_nms(kpts=kpts, areas=areas, scores=scores, thresh=thresh, in_vis_thre=vis, soft=soft, sigmas=sigmas)
            assert kept(out) == _existing(kpts, areas, scores, thresh, vis, sigmas, soft), (case, n, J, soft)
            assert kept(out) == ref["keep"][:ref["num"]].tolist() and np.array_equal(out["suppressor"], ref["suppressor"]), (case, soft)
            compared += 1
        left_out += edge
    print("knife-edge cases left out: %d of 300; comparisons made: %d" % (left_out, compared))
    assert left_out <= 6                                                    # 2 % of 300; continuous random data: expected 0


def test_rescoring_is_bit_equal_to_the_restatement():
    pts, boxes, det = R.clustered(5, 12, 17)
    pts[3, :, 2] = 0.1                                                      # nobody above the threshold: score 0 * det
    pts[4, :5, 2] = 0.2                                                     # equality is not above
    kpts, areas, scores = R.engine_to_coco(pts, boxes, det)
    for d in (det, None):
        want = R.rescore(kpts, scores if d is not None else np.ones(12), 0.2)
        out = pp().pose_nms(pts.copy(), boxes.copy(), d, thresh=0.9, rescore_thre=0.2)
        assert np.array_equal(out["scores"].view(np.uint64), want.view(np.uint64))
        assert out["scores"][3] == 0.0
        coco = pp().pose_nms(kpts=kpts, areas=areas, scores=scores if d is not None else np.ones(12), thresh=0.9, rescore_thre=0.2)
        assert np.array_equal(coco["scores"].view(np.uint64), want.view(np.uint64))
    off = pp().pose_nms(pts.copy(), boxes.copy(), det, thresh=0.9)
    assert np.array_equal(off["scores"], det.astype(np.float64))


@pytest.mark.parametrize("J", [17, 16, 133, 255])
@pytest.mark.parametrize("soft", [False, True])
def test_engine_layout_equals_the_coco_layout_on_widened_arrays(J, soft):
    sigmas = None if J == 17 else R.random_sigmas(J, J)
    for n, vis, rescore in ((1, None, None), (9, 0.3, None), (30, None, 0.2), (40, 0.2, 0.2)):
        pts, boxes, det = R.clustered(70 + n + J, n, J)
        kpts, areas, scores = R.engine_to_coco(pts, boxes, det)
        a = pp().pose_nms(pts.copy(), boxes.copy(), det, thresh=0.6, in_vis_thre=vis, rescore_thre=rescore, soft=soft, sigmas=sigmas)
        b = pp().pose_nms(kpts=kpts, areas=areas, scores=scores, thresh=0.6, in_vis_thre=vis, rescore_thre=rescore, soft=soft, sigmas=sigmas)
        for name in ("keep", "num", "suppressor", "status"):
            assert np.array_equal(a[name], b[name]), (n, name)
        assert np.array_equal(a["scores"].view(np.uint64), b["scores"].view(np.uint64))
        ref = R.pose_nms(kpts, areas, scores, 0.6, vis, rescore, soft, sigmas)
        if ref["gap"] > 1e-9:
            assert_equals_ref(b, ref, (n, J, soft))
        assert 1 <= int(a["num"][0]) <= (20 if soft else n)
        assert np.array_equal(a["pts"], pts) and np.array_equal(a["boxes"], boxes)      # without suppress nothing is written


@pytest.mark.parametrize("soft", [False, True])
def test_ties_nan_masked_and_zero_area(soft):
    pts, boxes, det = R.tie_case()
    kpts, areas, scores = R.engine_to_coco(pts, boxes, det)
    out = pp().pose_nms(pts.copy(), boxes.copy(), det, thresh=0.5, in_vis_thre=0.1, soft=soft)
    ref = R.pose_nms(kpts, areas, scores, 0.5, 0.1, None, soft)
    assert_equals_ref(out, ref, soft)
    assert int(out["status"][0]) == 1                                       # the NaN score, ordered last
    row = pp().pose_nms_oks_row(kpts, areas, 8, in_vis_thre=0.1)
    assert row[2] == 0.0                                                    # all joints masked: no term
    zero = pp().pose_nms_oks_row(kpts, areas, 4, in_vis_thre=None)
    assert zero[10] == 1.0 and zero[4] == 1.0                               # zero areas, zero distance: exp(0) per joint
    if not soft:
        k = kept(out)
        assert 2 in k and 8 in k                                            # masked candidates are never removed: OKS 0.0
        for i in (i for i in k if i < 6 and i != 2):                        # of two equal people the lower index is kept; the NaN
            assert out["suppressor"][i + 6] == i                            # copy and the zero-area copy fall to their twins too
        assert any(i < 6 and i != 2 for i in k)


def test_non_finite_oks_sets_status_bit_1():
    pts, boxes, det = R.clustered(3, 4, 17)
    kpts, areas, scores = R.engine_to_coco(pts, boxes, det)
    areas[:] = -np.spacing(1)                                               # denominator 0, distances > 0: e = inf or NaN
    kpts[1] = kpts[0]                                                       # 0 / 0
    out = pp().pose_nms(kpts=kpts, areas=areas, scores=scores, thresh=0.5)
    assert int(out["status"][0]) & 2
    assert int(out["num"][0]) >= 1


def test_suppress_changes_only_people_who_were_not_kept():
    for soft, n in ((False, 12), (True, 25)):
        pts, boxes, det = R.clustered(8 + n, n, 17)
        plain = pp().pose_nms(pts.copy(), boxes.copy(), det, thresh=0.5, soft=soft)
        p2, b2 = pts.copy(), boxes.copy()
        out = pp().pose_nms(p2, b2, det, thresh=0.5, soft=soft, suppress=True)
        assert np.shares_memory(out["pts"], p2) and np.shares_memory(out["boxes"], b2)      # in place
        for name in ("keep", "num", "suppressor", "status", "scores"):
            assert np.array_equal(out[name], plain[name])
        gone = out["suppressor"] != -1
        assert gone.any() and (~gone).any() and (~gone).sum() == int(out["num"][0])
        assert np.array_equal(p2[~gone], pts[~gone]) and np.array_equal(b2[~gone], boxes[~gone])
        assert np.array_equal(p2[gone][:, :, :2], pts[gone][:, :, :2])      # the coordinates stay
        assert (p2[gone][:, :, 2] == 0).all() and (b2[gone] == 0).all()
    assert (out["suppressor"] == -2).sum() == 5 and int(out["num"][0]) == 20


def test_segments_and_empty_cases():
    shapes = [0, 1, 25, 7]
    parts = [R.clustered(90 + k, n, 17) for k, n in enumerate(shapes)]
    cat = [np.concatenate([p[k] for p in parts]) for k in range(3)]
    for soft in (False, True):
        whole = pp().pose_nms(cat[0].copy(), cat[1].copy(), cat[2], counts=shapes, thresh=0.6, rescore_thre=0.2, soft=soft)
        single = [pp().pose_nms(p[0].copy(), p[1].copy(), p[2], thresh=0.6, rescore_thre=0.2, soft=soft) for p in parts]
        for name in ("keep", "num", "suppressor", "status", "scores"):
            assert np.array_equal(whole[name], np.concatenate([s[name] for s in single])), name
        assert whole["num"][0] == 0 and whole["num"][1] == 1
    empty = pp().pose_nms(np.zeros((0, 17, 3), np.float32), np.zeros((0, 4), np.int32))
    assert empty["num"].tolist() == [0] and empty["status"].tolist() == [0] and len(empty["keep"]) == 0
    nothing = pp().pose_nms(np.zeros((0, 17, 3), np.float32), np.zeros((0, 4), np.int32), counts=[])
    assert len(nothing["num"]) == 0


def test_refusals_leave_the_outputs_untouched():
    lib = lib_mod().load()
    pts, boxes, det = R.clustered(4, 5, 17)
    kpts, areas, scores = R.engine_to_coco(pts, boxes, det)
    p16 = np.ascontiguousarray(pts[:, :16])
    big = R.clustered(6, 257, 17)
    sig = R.random_sigmas(1, 17)
    nan = float("nan")
    E, S, U = 4, 1, 2

    def call(P, start, J, flags, k, a, s, thresh, sigmas=None, null=()):
        start = None if start is None else np.asarray(start, np.int32)
        n = 300
        outs = dict(keep=np.full(n, 77, np.int32), num=np.full(8, 77, np.int32), scores_out=np.full(n, 77.0), suppressor=np.full(n, 77, np.int32),
                    status=np.full(8, 77, np.int32))
        k0, a0 = k.copy(), a.copy()
        ptr = {name: (None if name in null else v.ctypes.data) for name, v in outs.items()}
        rc = lib.hrn_pose_nms(P, None if start is None else start.ctypes.data, J, flags, None if "kpts" in null else k.ctypes.data,
                              a.ctypes.data, None if s is None else s.ctypes.data, thresh, nan, nan,
                              None if sigmas is None else sigmas.ctypes.data, ptr["keep"], ptr["num"], ptr["scores_out"],
                              ptr["suppressor"], ptr["status"])
        assert all((v == 77).all() for v in outs.values()) and np.array_equal(k, k0) and np.array_equal(a, a0)
        return rc, lib.hrn_pose_nms_last_error().decode()

    cases = [
        (call(1, None, 17, E, pts, boxes, det, 0.5), "null segment table"),
        (call(1, [0, 5], 17, E, pts, boxes, det, 0.5, null=("num",)), "null segment table"),
        (call(1, [0, 5], 17, E, pts, boxes, det, 0.5, null=("keep",)), "null keypoints"),
        (call(1, [0, 5], 17, E, pts, boxes, det, 0.5, null=("kpts",)), "null keypoints"),
        (call(1, [0, 5], 17, 0, kpts, areas, None, 0.5), "null scores"),
        (call(2, [0, 3, 2], 17, E, pts, boxes, det, 0.5), "decreases"),
        (call(1, [-1, 4], 17, E, pts, boxes, det, 0.5), "below zero"),
        (call(1, [0, 257], 17, E, big[0], big[1], big[2], 0.5), "HRN_MAX_TRACKED"),
        (call(1, [0, 5], 0, E, pts, boxes, det, 0.5), "HRN_MAX_JOINTS"),
        (call(1, [0, 5], 257, E, pts, boxes, det, 0.5, sigmas=sig), "HRN_MAX_JOINTS"),
        (call(1, [0, 5], 17, E, pts, boxes, det, nan), "finite"),
        (call(1, [0, 5], 17, E, pts, boxes, det, float("inf")), "finite"),
        (call(1, [0, 5], 17, E | S, pts, boxes, det, 0.0), "thresh > 0"),
        (call(1, [0, 5], 17, E | S, pts, boxes, det, -0.5), "thresh > 0"),
        (call(1, [0, 5], 16, E, p16, boxes, det, 0.5), "sigmas"),
        (call(1, [0, 5], 17, U, kpts, areas, scores, 0.5), "engine layout"),
        (call(1, [0, 5], 17, 8, kpts, areas, scores, 0.5), "flag"),
        (call(-1, [0, 5], 17, E, pts, boxes, det, 0.5), "negative"),
    ]
    for (rc, text), word in cases:
        assert rc == 7 and word in text, (rc, text, word)
    # the accepted neighbours of two refusals: thresh <= 0 is fine for hard NMS, and sigmas make J = 16 legal
    assert pp().pose_nms(pts.copy(), boxes.copy(), det, thresh=0.0)["num"][0] >= 1
    assert pp().pose_nms(p16, boxes.copy(), det, thresh=0.5, sigmas=sig[:16])["num"][0] >= 1
    with pytest.raises(ValueError, match="engine layout"):
        pp().pose_nms(kpts=kpts, areas=areas, scores=scores, suppress=True)


def _coco_loop(preds, maxvals, areas, box_scores, image_index, oks_thre, in_vis_thre, soft):
    """datasets/COCO.py:349-382 over postproc.oks_nms / soft_oks_nms: (rescored scores, image -> kept indices)"""
    from collections import defaultdict

    people = [{"keypoints": np.concatenate([preds[i], maxvals[i].reshape(-1, 1)], 1), "area": areas[i], "score": box_scores[i], "index": i}
              for i in range(len(preds))]
    by_image = defaultdict(list)
    for person, image in zip(people, image_index.tolist()):
        by_image[image].append(person)
    kept_by_image = {}
    for image, img_kpts in by_image.items():
        for n_p in img_kpts:
            kpt_score, valid_num = 0, 0
            for n_jt in range(preds.shape[1]):
                t_s = n_p["keypoints"][n_jt][2]
                if t_s > in_vis_thre:
                    kpt_score, valid_num = kpt_score + t_s, valid_num + 1
            if valid_num != 0:
                kpt_score = kpt_score / valid_num
            n_p["score"] = kpt_score * n_p["score"]
        keep = (pp().soft_oks_nms if soft else pp().oks_nms)(img_kpts, oks_thre)
        kept_by_image[image] = [p["index"] for p in img_kpts] if len(keep) == 0 else [img_kpts[k]["index"] for k in keep]
    return np.asarray([p["score"] for p in people]), kept_by_image


@pytest.mark.parametrize("soft", [False, True])
def test_nms_eval_groups_by_image(soft, monkeypatch):
    pkg = load_pkg()
    counts = [3, 1, 25, 8, 12, 2]
    parts = [R.clustered(200 + k, n, 17) for k, n in enumerate(counts)]
    pts, boxes, det = (np.concatenate([p[k] for p in parts]) for k in range(3))
    kpts, areas, box_scores = R.engine_to_coco(pts, boxes, det)
    image_index = np.repeat(np.asarray([900, 17, 5, 333, 64, 8]), counts)
    shuffle = np.random.default_rng(1).permutation(len(areas))
    preds, maxvals = kpts[shuffle][:, :, :2], kpts[shuffle][:, :, 2:]
    areas, box_scores, image_index = areas[shuffle], box_scores[shuffle], image_index[shuffle]

    def host_form(self, k, a, s, cnt, thresh, vis, rescore_thre, soft_, sigmas):
        calls.append(len(cnt))
        assert vis is None                                                  # the reference calls oks_nms without a visibility mask
        return pp().pose_nms(kpts=k, areas=a, scores=s, counts=cnt, thresh=thresh, rescore_thre=rescore_thre, soft=soft_, sigmas=sigmas)

    calls = []
    monkeypatch.setattr(pkg.NativeHRNet, "_pose_nms_coco", host_form)
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=1, device=-1)          # plan-only: no GPU is touched
    scores, kept_by_image = net.nms_eval(preds, maxvals, areas, box_scores, image_index, oks_thre=0.7, in_vis_thre=0.2, soft=soft)
    want_scores, want = _coco_loop(preds, maxvals, areas, box_scores, image_index, 0.7, 0.2, soft)
    assert calls == [6]                                                     # one call for all images
    assert np.array_equal(scores.view(np.uint64), want_scores.view(np.uint64))
    assert list(kept_by_image) == list(want)                                # images in order of first appearance
    for image in want:
        assert kept_by_image[image].tolist() == want[image], image
    assert any(len(v) < c for v, c in zip((kept_by_image[i] for i in (900, 17, 5, 333, 64, 8)), counts))
