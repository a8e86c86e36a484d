"""Joints over time on the host: postproc.filter_poses (hrn_filter_poses, csrc/temporal_math.h) against the numpy float64
restatement of tests/temporal_ref.py -- bit for bit, nothing left out: every operation is a correctly rounded IEEE operation on
both sides -- then what the filter is for (a constant input stays, a steady motion is predicted, jitter shrinks), that the state
follows `match` and not the index, the entry's refusals, and PersonTracker's one_euro option against the hand composition.

MEASURED here (numpy form and host form agree): constant velocity, worst excess of |x(k+1) - pred(k)| over |v| (1 - alpha)^k:
1.2e-4 px (bound: one float32 spacing, 2.4e-4 px below 4096); jitter of a stationary joint under N(0, 1 px) noise: 0.34 / 0.31 px out
(y / x) for 1.00 px in."""
import numpy as np
import pytest

import temporal_ref as ref
from assoc_cases import DEMO
from conftest import load_pkg
from temporal_ref import DEFAULTS, ONE_EURO, PARAM_SETS, bits, random_sequence, run_sequence, tracker_frames


@pytest.fixture(scope="module")
def pp():
    return load_pkg("postproc")


def test_exports():
    pkg, lib = load_pkg(), load_pkg("_lib")
    names = {"hrn_filter_poses", "hrn_filter_poses_last_error", "hrn_filter_poses_dev"}
    assert names <= set(lib.header_symbols()) and names <= set(lib.SYMBOLS)
    assert set(lib.header_symbols()) == set(lib.SYMBOLS)
    assert "temporal.hip" in lib.SOURCES
    assert "filter_poses" in pkg.__all__ and pkg.filter_poses is pkg.postproc.filter_poses
    assert hasattr(pkg.NativeHRNet, "filter_poses")


def assert_same(got, want, what):
    for name, g, w in zip(("pts_out", "pred", "state", "age"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, name)


@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("J", [1, 17, 133])
def test_host_form_equals_the_restatement_bit_for_bit(pp, J, streams):
    renewed = oldest = 0
    for k, params in enumerate(PARAM_SETS):
        seq = random_sequence(100 * J + 10 * streams + k, J, streams)
        assert streams == 1 or any(c[streams // 2] == 0 and c.sum() > 0 for _, _, c, _ in seq)      # an empty stream beside people
        got, want = run_sequence(pp.filter_poses, seq, params, first_match=True), run_sequence(ref.filter_poses, seq, params, first_match=True)
        for f, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, (J, streams, k, f))
            assert np.isfinite(g[2][g[3] > 0]).all()                      # a stored state is always finite
            assert (g[2][g[3] == 0] == 0).all() and not np.signbit(g[2][g[3] == 0]).any()
        for f in range(1, len(seq)):                                      # joints that had a prior and were initialised anew: the +-3e38 jumps
            before = ref.previous_index(seq[f][1], seq[f][2], seq[f - 1][2], len(seq[f][0]), len(seq[f - 1][0]))
            had = np.zeros(got[f][3].shape, bool)
            had[before >= 0] = got[f - 1][3][before[before >= 0]] > 0
            renewed += int((had & (got[f][3] == 1)).sum())
        oldest = max([oldest] + [int(g[3].max(initial=0)) for g in got])
    assert oldest >= 2 and (J == 1 or (oldest >= 3 and renewed > 0))      # states do live on through the matches


def test_a_constant_input_is_a_fixed_point(pp):
    pts = np.asarray([[[123.456, 789.012, 0.9], [0.1, -1e-30, 0.7], [3e38, -3e38, 0.51]]], np.float32)   # (not -0.0: -0.0 + alpha * 0.0 is +0.0)
    state, match = None, None
    for k in range(100):
        out, pred, state = pp.filter_poses(pts, state, match)
        match = np.zeros(1, np.int32)
        assert np.array_equal(bits(out), bits(pts)) and np.array_equal(bits(pred), bits(pts)), k
        assert np.array_equal(bits(state[0][:, :, 0:2]), bits(pts[:, :, :2])) and np.array_equal(bits(state[0][:, :, 2:4]), bits(pts[:, :, :2]))
        assert np.array_equal(bits(state[0][:, :, 4:6]), np.zeros((1, 3, 2), np.uint32)), k           # +0.0, not -0.0
        assert (state[1] == k + 1).all()


@pytest.mark.parametrize("v", [1.0, 5.0, 20.0, 60.0, -37.25])
def test_a_constant_velocity_is_predicted(pp, v):
    """|x(k+1) - pred(k)| <= |v| (1 - alpha(d_cutoff))^k + s for k >= 1: the closed form of the derivative's recursion from
    d_hat = 0, plus one float32 spacing at the largest coordinate for the single rounding of pred"""
    dt = 1 / 30
    xs = (1000.0 + v * np.arange(41)).astype(np.float32)
    assert np.array_equal(xs.astype(np.float64), 1000.0 + v * np.arange(41))                         # exact in float32
    s = float(np.spacing(np.abs(xs).max()))
    assert s <= 2.0 ** -12
    a = ref.alpha(DEFAULTS["d_cutoff"], dt)
    state, worst = None, 0.0
    for k in range(40):
        pts = np.asarray([[[xs[k], 2 * xs[k], 0.9]]], np.float32)
        out, pred, state = pp.filter_poses(pts, state, None if k == 0 else np.zeros(1, np.int32), dt=dt, lookahead=dt, **DEFAULTS)
        if k >= 1:
            err = abs(float(xs[k + 1]) - float(pred[0, 0, 0]))
            closed = abs(v) * (1 - a) ** k
            worst = max(worst, err - closed)
            print("v %g k %d error %.6g closed form %.6g" % (v, k, err, closed))
            assert err <= closed + s, (v, k, err, closed, s)
    print("v %g worst excess over the closed form %.3g (s = %.3g)" % (v, worst, s))


def test_jitter_of_a_stationary_joint_is_more_than_halved(pp):
    noise = np.random.default_rng(0).normal(0.0, 1.0, (2000, 2))
    state, outs = None, []
    for k in range(2000):
        pts = np.asarray([[[500.0 + noise[k, 0], 500.0 + noise[k, 1], 0.9]]], np.float32)
        out, _, state = pp.filter_poses(pts, state, None if k == 0 else np.zeros(1, np.int32), **DEFAULTS)
        outs.append(out[0, 0, :2].astype(np.float64))
    outs = np.asarray(outs)[100:]
    for axis in (0, 1):
        std_in, std_out = float(noise[100:, axis].std()), float(outs[:, axis].std())
        print("axis %d: %.3f px in, %.3f px out" % (axis, std_in, std_out))
        assert std_out < 0.5 * std_in, (axis, std_in, std_out)


def test_the_state_follows_match_not_the_index(pp):
    seq = random_sequence(77, 17, 1, most=7)
    rng = np.random.default_rng(3)
    perms = [rng.permutation(len(pts)) for pts, _, _, _ in seq]
    shuffled = []
    for k, (pts, match, counts, dt) in enumerate(seq):
        inv = np.argsort(perms[k - 1]) if k else np.zeros(0, np.int64)          # where the previous person went
        m2 = np.asarray([inv[t] if 0 <= t < len(inv) else t for t in match[perms[k]]], np.int32).reshape(-1)
        shuffled.append((pts[perms[k]], m2, counts, dt))
    plain, moved = run_sequence(pp.filter_poses, seq, DEFAULTS), run_sequence(pp.filter_poses, shuffled, DEFAULTS)
    for k, (a, b) in enumerate(zip(plain, moved)):
        assert_same(b, [x[perms[k]] for x in a], k)
    assert any(len(p) > 1 and not np.array_equal(p, np.arange(len(p))) for p in perms)


def _raw(lib, pts, match, state, age, tables=((0, 1), (0, 1)), J=None, numbers=(1 / 30, 1.0, 0.007, 1.0, 0.5, 1 / 30), alias=False,
         want_pred=True, fill=None):
    """hrn_filter_poses on arrays as given (no shim in between); outputs pre-filled with `fill`"""
    cur, prev = (np.asarray(t, np.int32) for t in tables)
    n, J = cur[-1] - cur[0], pts.shape[1] if J is None else J
    outs = [pts if alias else np.empty_like(pts), np.empty_like(pts), np.empty((n, pts.shape[1], 6), np.float32), np.empty((n, pts.shape[1]), np.int32)]
    for o in outs[0 if not alias else 1:]:
        if fill is not None:
            o.view(np.uint32)[...] = fill
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    rc = lib.hrn_filter_poses(len(cur) - 1, ptr(cur), ptr(prev), J, ptr(pts), ptr(match), ptr(state), ptr(age), *numbers, ptr(outs[0]),
                              ptr(outs[1]) if want_pred else None, ptr(outs[2]), ptr(outs[3]))
    return rc, outs


def test_in_place_and_without_a_prediction(pp):
    lib = load_pkg("_lib").load()
    rng = np.random.default_rng(5)
    pts0 = np.concatenate([rng.uniform(0, 500, (5, 17, 2)), rng.uniform(0.3, 1.0, (5, 17, 1))], 2).astype(np.float32)
    pts1 = np.ascontiguousarray((pts0 + rng.normal(0, 2, pts0.shape).astype(np.float32))[[3, 0, 4, 1]])
    match, dt = np.asarray([3, 0, -1, 1], np.int32), 1 / 30
    _, _, (values, age) = pp.filter_poses(pts0)
    tables = ((0, len(pts1)), (0, len(pts0)))
    rc, want = _raw(lib, pts1.copy(), match, values, age, tables)
    assert rc == 0 and (want[3] > 1).any()
    rc, got = _raw(lib, pts1.copy(), match, values, age, tables, alias=True)
    assert rc == 0
    assert_same(got, want, "in place")
    rc, got = _raw(lib, pts1.copy(), match, values, age, tables, want_pred=False, fill=0x7fc12345)
    assert rc == 0 and (got[1].view(np.uint32) == 0x7fc12345).all()
    assert_same([got[0], got[2], got[3]], [want[0], want[2], want[3]], "no prediction")


def test_refusals_name_their_cause_and_write_nothing():
    lib = load_pkg("_lib").load()
    pts = np.random.default_rng(1).uniform(1, 100, (3, 4, 3)).astype(np.float32)
    match, state, age = np.zeros(3, np.int32), np.ones((2, 4, 6), np.float32), np.ones((2, 4), np.int32)
    ok = dict(tables=((0, 3), (0, 2)))
    nan, inf = float("nan"), float("inf")
    d = (1 / 30, 1.0, 0.007, 1.0, 0.5, 1 / 30)

    def numbers(**kw):
        names = ("dt", "min_cutoff", "beta", "d_cutoff", "threshold", "lookahead")
        return tuple(kw.get(k, v) for k, v in zip(names, d))

    cases = [(dict(ok, J=0), "J must be"), (dict(ok, J=257), "J must be"), (dict(tables=((0, 3, 2), (0, 1, 2))), "decreases"),
             (dict(tables=((0, 3), (2, 0))), "decreases"), (dict(tables=((-1, 2), (0, 2))), "below zero")]
    for name in ("dt", "min_cutoff", "d_cutoff"):
        cases += [(dict(ok, numbers=numbers(**{name: bad})), "finite and positive") for bad in (0.0, -1.0, nan, inf)]
    for name in ("beta", "lookahead"):
        cases += [(dict(ok, numbers=numbers(**{name: bad})), "finite and not negative") for bad in (-1e-9, nan, inf)]
    for kw, text in cases:
        rc, outs = _raw(lib, pts.copy(), match, state, age, fill=0xdeadbeef, **kw)
        assert rc == 7 and text in lib.hrn_filter_poses_last_error().decode(), (kw, lib.hrn_filter_poses_last_error())
        assert all((o.view(np.uint32) == 0xdeadbeef).all() for o in outs), kw
    # null tables and arrays, null previous arrays beside a match, overlapping states
    base = [1, None, None, 4, pts.ctypes.data, match.ctypes.data, state.ctypes.data, age.ctypes.data, *d]
    cur, prev = np.asarray([0, 3], np.int32), np.asarray([0, 2], np.int32)
    out, new_state, new_age = np.zeros_like(pts), np.zeros((3, 4, 6), np.float32), np.zeros((3, 4), np.int32)
    full = list(base) + [out.ctypes.data, None, new_state.ctypes.data, new_age.ctypes.data]
    assert lib.hrn_filter_poses(*full) == 7 and "null segment tables" in lib.hrn_filter_poses_last_error().decode()
    full[1], full[2] = cur.ctypes.data, prev.ctypes.data
    assert lib.hrn_filter_poses(*full) == 0
    for slot in (4, 14, 16, 17):
        broken = list(full)
        broken[slot] = None
        assert lib.hrn_filter_poses(*broken) == 7 and "null pts" in lib.hrn_filter_poses_last_error().decode(), slot
    for slot in (6, 7):
        broken = list(full)
        broken[slot] = None
        assert lib.hrn_filter_poses(*broken) == 7 and "beside a match" in lib.hrn_filter_poses_last_error().decode(), slot
        broken[5] = None                                                   # without a match nobody reads them
        assert lib.hrn_filter_poses(*broken) == 0
    big = np.ones((5, 4, 6), np.float32)                                   # the new state inside the old one's bytes
    for new, old in ((16, 6), (17, 6), (16, 7), (17, 7)):
        broken = list(full)
        broken[old] = big.ctypes.data
        broken[new] = big.ctypes.data + 24
        assert lib.hrn_filter_poses(*broken) == 7 and "overlap" in lib.hrn_filter_poses_last_error().decode(), (new, old)
    assert (big == 1).all()
    assert lib.hrn_filter_poses(-1, *full[1:]) == 7 and "P is negative" in lib.hrn_filter_poses_last_error().decode()
    assert lib.hrn_filter_poses(0, None, None, *full[3:]) == 0             # no streams: nothing to do
    huge = np.asarray([0, 2 ** 31 - 1], np.int32)                          # judged from the tables, before any array is touched
    assert lib.hrn_filter_poses(1, huge.ctypes.data, *full[2:]) == 7 and "2^31 - 1" in lib.hrn_filter_poses_last_error().decode()


def test_the_shim_refuses_what_does_not_fit(pp):
    pts = np.zeros((2, 17, 3), np.float32)
    with pytest.raises(ValueError, match=r"\(n, J, 3\)"):
        pp.filter_poses(np.zeros((2, 17, 2), np.float32))
    with pytest.raises(ValueError, match="one value per person"):
        pp.filter_poses(pts, match=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="joints per person"):
        pp.filter_poses(pts, (np.zeros((1, 16, 6), np.float32), np.zeros((1, 16), np.int32)), np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="streams"):
        pp.filter_poses(pts, (np.zeros((1, 17, 6), np.float32), np.zeros((1, 17), np.int32)), np.zeros(2, np.int32), counts=[1, 1])
    with pytest.raises(ValueError, match="finite and positive"):
        pp.filter_poses(pts, dt=0.0)
    out, pred, (values, age) = pp.filter_poses(np.zeros((0, 17, 3), np.float32), (np.zeros((4, 17, 6), np.float32), np.ones((4, 17), np.int32)))
    assert out.shape == pred.shape == (0, 17, 3) and values.shape == (0, 17, 6) and age.shape == (0, 17)


# ---- PersonTracker(one_euro=...) --------------------------------------------------------------------------------------------------
def hand_composition(frames, one_euro, dts):
    """what PersonTracker(None, one_euro=...) is defined as: postproc.associate_people, then postproc.filter_poses with its match"""
    pp = load_pkg("postproc")
    filt = {k: v for k, v in (one_euro or {}).items() if k != "rate"}
    prev, state, out = None, None, []
    for (boxes, pts, counts), dt in zip(frames, dts):
        boxes, pts = boxes.copy(), pts.copy()
        n, match = len(boxes), None
        counts = np.asarray([n] if counts is None else counts, np.int64)
        if prev is None:
            ids = np.concatenate([np.arange(c, dtype=np.int32) for c in counts])
            next_id = np.where(counts > 0, counts + 1, 0).astype(np.int32)
        elif n == 0:
            ids = np.zeros(0, np.int32)
        else:
            boxes, pts, ids, match, next_id, _ = pp.associate_people(boxes, pts, prev[0], prev[1], prev[2], next_id, *DEMO, counts=counts,
                                                                     prev_counts=prev[3])
        filtered, pred = pts, None
        if one_euro is not None:
            filtered, pred, state = pp.filter_poses(pts, state, match, counts=counts, prev_counts=None if prev is None else prev[3],
                                                    dt=1 / one_euro["rate"] if dt is None else dt, **filt)
        prev = (boxes, pts, ids, counts)
        out.append((boxes, filtered, ids, pred, state, next_id.copy()))
    return out


@pytest.mark.parametrize("streams", [1, 3])
def test_tracker_with_one_euro_equals_the_hand_composition(streams):
    pkg = load_pkg()
    frames = list(tracker_frames(streams))
    dts = [None, None, 0.05, None, 1 / 30, None]
    want = hand_composition(frames, ONE_EURO, dts)
    tracker = pkg.PersonTracker(None, one_euro=ONE_EURO)
    assert tracker.predicted is None
    moved = 0
    for k, ((boxes, pts, counts), dt) in enumerate(zip(frames, dts)):
        given = boxes.copy(), pts.copy()
        got = tracker.update(boxes, pts, counts=counts, dt=dt)
        assert np.array_equal(given[0], boxes) and np.array_equal(bits(given[1]), bits(pts))           # the arguments are left alone
        w = want[k]
        assert np.array_equal(got[0], w[0]) and np.array_equal(bits(got[1]), bits(w[1])) and np.array_equal(got[2], w[2]), k
        assert np.array_equal(bits(tracker.predicted), bits(w[3])), k
        assert np.array_equal(bits(tracker.filter_state[0]), bits(w[4][0])) and np.array_equal(tracker.filter_state[1], w[4][1]), k
        assert tracker.next_id.tolist() == w[5].tolist()
        if len(pts):
            moved += int((bits(got[1]) != bits(tracker.prev_pts)).sum())                              # the state kept for the association
    assert moved > 0                                                                                  # ... is not the filtered one
    assert max(int(w[4][1].max(initial=0)) for w in want) >= 2
    tracker.reset()
    assert tracker.filter_state is None and tracker.predicted is None
    with pytest.raises(ValueError, match="one_euro"):
        pkg.PersonTracker(None, one_euro=dict(cutoff=1.0))


def test_tracker_without_the_option_makes_no_filter_call(monkeypatch):
    pkg, pp = load_pkg(), load_pkg("postproc")

    def never(*a, **kw):
        raise AssertionError("filter_poses was called")

    monkeypatch.setattr(pp, "filter_poses", never)
    frames = list(tracker_frames(3))
    want = hand_composition(frames, None, [None] * len(frames))
    tracker = pkg.PersonTracker()
    for k, (boxes, pts, counts) in enumerate(frames):
        got = tracker.update(boxes, pts, counts=counts)
        assert np.array_equal(got[0], want[k][0]) and np.array_equal(bits(got[1]), bits(want[k][1])) and np.array_equal(got[2], want[k][2])
        assert tracker.predicted is None and tracker.filter_state is None
