"""Person ids between two frames, host side: hrn_associate_people (postproc.associate_people) against the reference's own outputs
(tests/golden/tracking_cases.npz) and against postproc.find_person_id_associations, its refusals, its segments, and PersonTracker
against the demo loop.  No GPU."""
import math

import numpy as np
import pytest

from assoc_cases import DEMO, PARAMS, demo_loop, make_case, margins, sequence
from conftest import golden, load_pkg

G = golden("tracking_cases")
pp = load_pkg("postproc")


def run(case, params, **kw):
    return pp.associate_people(case["boxes"].copy(), case["pts"].copy(), case["prev_boxes"], case["prev_pts"], case["prev_ids"],
                               case["next_id"], *params, **kw)


def test_symbols_are_declared_and_exported():
    lib = load_pkg("_lib")
    names = {"hrn_associate_people", "hrn_associate_people_last_error", "hrn_associate_people_dev", "hrn_draw_poses_ids_dev",
             "hrn_assoc_exp", "hrn_associate_similarity"}
    assert names <= set(lib.header_symbols()) and names <= set(lib.SYMBOLS)
    loaded = lib.load()
    for name in names:
        assert hasattr(loaded, name)
    assert "assoc.hip" in lib.SOURCES


def test_own_exp_is_within_two_ulp_of_math_exp():
    """the header's exp against math.exp over a dense grid of [-29, 0]: 2,900,001 points through numpy's exp (the same libm
    function on this platform), every 97th through math.exp itself.  Measured: 1 ulp.  The bound of 2 is the reasoning of
    csrc/assoc_math.h (reduction exact to 2^-53 relative, truncation below 2^-57, Horner's last step adds under 1 ulp) plus the
    1 ulp libm's own exp may err by."""
    lib = load_pkg("_lib").load()
    x = np.linspace(-29.0, 0.0, 2900001)
    got = np.empty_like(x)
    assert lib.hrn_assoc_exp(x.ctypes.data, len(x), got.ctypes.data) == 0
    ref = np.exp(x)
    worst = float((np.abs(got - ref) / np.spacing(ref)).max())
    sample = max(abs(float(g) - math.exp(float(v))) / math.ulp(math.exp(float(v))) for v, g in zip(x[::97], got[::97]))
    print("own exp: max %.2f ulp from numpy's exp, %.2f ulp from math.exp" % (worst, sample))
    assert worst <= 2.0 and sample <= 2.0
    assert got[-1] == 1.0 and np.all(np.diff(got) >= 0)


@pytest.mark.parametrize("k", [int(v) for v in G["track_cases"]])
def test_reference_fixtures(k):
    g = {n: G["track%d_%s" % (k, n)] for n in ("boxes", "pts", "prev_boxes", "prev_pts", "prev_ids", "next_id", "params", "sim_bbox",
                                               "sim_pose", "out_boxes", "out_pts", "out_ids")}
    alpha, thr, smooth = (float(v) for v in g["params"])
    case = dict(g, next_id=int(g["next_id"]))
    boxes, pts, ids, match, next_id, status = run(case, (alpha, thr, smooth))
    np.testing.assert_array_equal(ids, g["out_ids"])
    np.testing.assert_array_equal(boxes, g["out_boxes"])
    np.testing.assert_array_equal(pts, g["out_pts"])
    assert status.tolist() == [0] and next_id.tolist() == [max(int(g["next_id"]), int(ids.max()) + 1)]
    assert all((m >= 0) == (i in g["prev_ids"]) for m, i in zip(match, ids))


@pytest.mark.parametrize("k", [int(v) for v in G["track_cases"]])
def test_every_blended_similarity_is_within_one_ulp_of_the_reference_matrices(k):
    """hrn_associate_similarity gives the (n, m) matrix both entries work on; EVERY entry, matched or not, lies within 1 float32
    ulp of sim_pose * alpha + sim_bbox * (1 - alpha) from the reference's stored matrices (the bound: an exp within a few fp64
    ulp, averaged, rounded to float32, then the same float32 blend), and the cost is (double)(1.0f - sim)."""
    lib = load_pkg("_lib").load()
    g = {n: G["track%d_%s" % (k, n)] for n in ("boxes", "pts", "prev_boxes", "prev_pts", "params", "sim_bbox", "sim_pose")}
    alpha = float(g["params"][0])
    n, m, joints = len(g["boxes"]), len(g["prev_boxes"]), g["pts"].shape[1]
    arrays = [np.ascontiguousarray(g[name]) for name in ("boxes", "pts", "prev_boxes", "prev_pts")]
    cost, sim = np.empty((n, m), np.float64), np.empty((n, m), np.float32)
    assert lib.hrn_associate_similarity(arrays[0].ctypes.data, arrays[1].ctypes.data, n, arrays[2].ctypes.data, arrays[3].ctypes.data, m,
                                        joints, alpha, cost.ctypes.data, sim.ctypes.data) == 0
    want = g["sim_pose"] * alpha + g["sim_bbox"] * (1 - alpha)
    assert want.dtype == np.float32 and want.shape == sim.shape
    lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
    apart = np.abs(sim.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.float32(1e-30)))
    print("track%d: %d of %d entries differ, the farthest by %.2f ulp" % (k, int((sim != want).sum()), sim.size, float(apart.max())))
    assert np.all((sim >= lo) & (sim <= hi))
    assert np.array_equal(cost, (np.float32(1) - sim).astype(np.float64))
    assert lib.hrn_associate_similarity(None, None, 1, None, None, 1, joints, alpha, None, None) == 7


def kept_cases():
    cases, dropped = [], 0
    for n in (0, 1, 2, 3, 5, 9):
        for m in (0, 1, 2, 3, 5, 9):
            for j in (16, 17, 133):
                for p, params in enumerate(PARAMS):
                    case = make_case(1000 * n + 100 * m + j + 7919 * p, n, m, j, jitter=(2.0, 6.0, 25.0)[p])
                    near, gap = margins(case, params[0], params[1])
                    if min(near, gap) < 1e-5:
                        dropped += 1
                    else:
                        cases.append((case, params))
    return cases, dropped


def test_random_cases_equal_find_person_id_associations():
    cases, dropped = kept_cases()
    total = len(cases) + dropped
    assert total == 6 * 6 * 3 * 3 and dropped <= 0.05 * total, "%d of %d cases have a margin under 1e-5" % (dropped, total)
    matched = 0
    for case, (alpha, thr, smooth) in cases:
        want_boxes, want_pts, want_ids = pp.find_person_id_associations(
            case["boxes"].copy(), case["pts"].copy(), case["prev_boxes"], case["prev_pts"], case["prev_ids"],
            next_person_id=case["next_id"], pose_alpha=alpha, similarity_threshold=thr, smoothing_alpha=smooth)
        boxes, pts, ids, match, next_id, status = run(case, (alpha, thr, smooth))
        np.testing.assert_array_equal(ids, want_ids)
        np.testing.assert_array_equal(boxes, want_boxes)
        np.testing.assert_array_equal(pts, want_pts)
        assert status.tolist() == [0]
        assert next_id.tolist() == [max(case["next_id"], int(ids.max()) + 1) if len(ids) else case["next_id"]]
        matched += int((match >= 0).sum())
    assert matched > 100          # (the cases do match people: the comparison is not one of strangers only)


def test_two_zero_boxes_are_reported_not_matched():
    case = make_case(11, 3, 3, 17, jitter=1.0)
    case["boxes"][1] = 0
    case["prev_boxes"][2] = 0
    case["pts"][1] = case["prev_pts"][2]                  # OKS 1: only the NaN of 0 / 0 keeps this pair apart
    boxes, pts, ids, match, next_id, status = run(case, (0.5, 0.1, 0.1))
    assert status.tolist() == [1]
    assert match[1] != 2 and (match >= -1).all() and len(set(ids.tolist())) == 3
    clean = make_case(11, 3, 3, 17, jitter=1.0)
    assert run(clean, (0.5, 0.1, 0.1))[5].tolist() == [0]


def test_sizes_beyond_the_caps_are_refused():
    lib = load_pkg("_lib").load()
    big = make_case(3, 257, 2, 17)
    with pytest.raises(ValueError, match="HRN_MAX_TRACKED"):
        run(big, DEMO)
    with pytest.raises(ValueError, match="HRN_MAX_TRACKED"):
        run(make_case(3, 2, 257, 17), DEMO)
    with pytest.raises(ValueError, match="HRN_MAX_JOINTS"):
        run(make_case(3, 2, 2, 257), DEMO)
    with pytest.raises(ValueError, match="smoothing_alpha"):
        run(make_case(3, 2, 2, 17), (0.2, 0.4, 1.5))
    with pytest.raises(ValueError, match="finite"):
        run(make_case(3, 2, 2, 17), (float("nan"), 0.4, 0.1))
    assert lib.hrn_associate_people(1, None, None, 17, None, None, None, None, None, None, 0.2, 0.4, 0.1, None, None, None) == 7
    ok = make_case(3, 256, 256, 17)                       # the cap itself is served
    assert len(run(ok, DEMO)[2]) == 256


def test_three_problems_in_one_call_equal_three_calls():
    parts = [make_case(21, 4, 3, 17), make_case(22, 0, 2, 17), make_case(23, 5, 6, 17)]
    cat = {k: np.concatenate([p[k] for p in parts]) for k in ("boxes", "pts", "prev_boxes", "prev_pts", "prev_ids")}
    cat["next_id"] = [p["next_id"] for p in parts]
    for params in PARAMS:
        got = run(cat, params, counts=[4, 0, 5], prev_counts=[3, 2, 6])
        single = [run(p, params) for p in parts]
        for k in range(6):
            np.testing.assert_array_equal(got[k], np.concatenate([s[k] for s in single]))
    assert got[4].tolist()[1] == parts[1]["next_id"]        # nobody in the current frame: next_id stays


def test_tracker_equals_the_demo_loop():
    pkg = load_pkg()
    frames = sequence()
    want = demo_loop(frames)
    tracker = pkg.PersonTracker()
    assert (tracker.pose_alpha, tracker.similarity_threshold, tracker.smoothing_alpha) == DEMO
    for step, ((boxes, pts), (want_boxes, want_pts, want_ids, want_next)) in enumerate(zip(frames, want)):
        before = boxes.copy(), pts.copy()
        got_boxes, got_pts, got_ids = tracker.update(boxes, pts)
        assert np.array_equal(boxes, before[0]) and np.array_equal(pts, before[1])       # the arguments are left alone
        np.testing.assert_array_equal(got_ids, want_ids, err_msg="step %d" % step)
        np.testing.assert_array_equal(got_boxes, want_boxes)
        np.testing.assert_array_equal(got_pts, want_pts)
        assert tracker.next_id.tolist() == [want_next], step
    ids = [w[2].tolist() for w in want]
    assert ids[0] == [0, 1, 2] and want[0][3] == 4                                        # the first frame's n + 1
    assert sorted(ids[1]) == [0, 1, 2] and sorted(ids[2]) == [0, 2] and ids[3] == [] and want[3][3] == 4
    assert sorted(ids[4]) == [4, 5, 6] and sorted(ids[5]) == [4, 5, 6]                    # after an empty frame everybody is new
    tracker.reset()
    assert tracker.update(*frames[1])[2].tolist() == [0, 1, 2]


def test_tracker_with_two_streams_equals_two_trackers():
    pkg = load_pkg()
    a, b = sequence(seed=5), sequence(seed=9)[::-1]
    both, one, two = pkg.PersonTracker(), pkg.PersonTracker(), pkg.PersonTracker()
    for (ba, pa), (bb, pb) in zip(a, b):
        got = both.update(np.concatenate([ba, bb]), np.concatenate([pa, pb]), counts=[len(ba), len(bb)])
        ra, rb = one.update(ba, pa), two.update(bb, pb)
        for k in range(3):
            np.testing.assert_array_equal(got[k], np.concatenate([ra[k], rb[k]]))
        assert both.next_id.tolist() == one.next_id.tolist() + two.next_id.tolist()
