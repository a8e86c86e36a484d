"""The person track table, host side (include/hrnet_mi355.h: hrn_track_people): the host entry against the numpy restatement
(tests/tracks_ref.py) bit for bit over fed-back sequences, the anchor to the reference (max_lost = 0 is PersonTracker as it was;
the stored cases of tests/golden/tracking_cases.npz), the designed cases the table exists for -- an occlusion, a fast mover, the
library's zero row, a full table, an empty stream -- and the refusals.  No GPU."""
import numpy as np
import pytest

import tracks_ref as ref
from assoc_cases import DEMO, make_case, people, sequence
from conftest import golden, load_pkg

pp = load_pkg("postproc")
G = golden("tracking_cases")
OPTIONS = [(ml, coast, sm) for ml in (0, 1, 5) for coast in (False, True) for sm in (0.0, 0.1)]     # 12
SHAPES = [(J, P, C) for J in (1, 17, 133) for P in (1, 3) for C in (4, 16, 256)]                   # 18


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_outputs_equal(got, want, what):
    for name, g, w in zip(("boxes", "pts", "ids", "match_row", "slot", "status"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, name, g.tolist() if g.ndim == 1 else None, w.tolist() if w.ndim == 1 else None)


def test_symbols_are_declared_and_exported():
    lib = load_pkg("_lib")
    names = {"hrn_track_people", "hrn_track_people_last_error", "hrn_track_people_dev"}
    assert names <= set(lib.header_symbols()) and names <= set(lib.SYMBOLS)
    loaded = lib.load()
    for name in names:
        assert hasattr(loaded, name)
    assert "tracks.hip" in lib.SOURCES


@pytest.mark.parametrize("k,shape", list(enumerate(SHAPES)))
def test_sequences_equal_the_restatement(k, shape):
    """12 updates with the table fed back; four of the twelve option sets per shape, every set under at least six shapes"""
    J, P, C = shape
    seen_full = seen_lost = seen_back = False
    for o in range(4):
        max_lost, coast, smoothing = OPTIONS[(4 * k + o) % 12]
        params = (DEMO[0], DEMO[1], smoothing, max_lost, coast, 0.5)
        table, want_table = pp.new_track_table(P, C, J), pp.new_track_table(P, C, J)
        for u, (boxes, pts, counts) in enumerate(ref.sequence_frames(100 * k + o, P, J)):
            want = ref.update(boxes, pts, want_table, *params, counts=counts)
            got = pp.track_people(boxes.copy(), pts.copy(), table, *params, counts=counts)
            assert_outputs_equal(got, want, (shape, params, u))
            ref.assert_tables_equal(table, want_table, (shape, params, u))
            seen_full |= bool((got[5] & 4).any())
            seen_lost |= bool((table["slot_lost"] > 0).any())
            stream = np.repeat(np.arange(P), counts)
            held = got[4] >= 0
            seen_back |= bool((table["slot_hits"][stream[held], got[4][held]][got[3][held] == -1] > 1).any())   # accepted after a gap
    assert not seen_full if C > 4 else seen_full or P == 1                   # C = 4 fills the table, the others never
    keeps = OPTIONS[(4 * k) % 12][0] > 0                                     # (the four option sets of a shape share max_lost)
    assert seen_lost == keeps and (keeps or not seen_back)                   # somebody was lost ...
    assert seen_back or not keeps or P == 1                                  # ... and, among three streams, somebody came back


def tracker_pair(**kw):
    pkg = load_pkg()
    return pkg.PersonTracker(None, **kw), pkg.PersonTracker(None, max_lost=0, **kw)


def assert_trackers_agree(frames, what, **kw):
    old, new = tracker_pair(**kw)
    for u, frame in enumerate(frames):
        boxes, pts = frame[:2]
        extra = {"counts": frame[2]} if len(frame) > 2 else {}
        want, got = old.update(boxes, pts, **extra), new.update(boxes, pts, **extra)
        for name, g, w in zip(("boxes", "pts", "ids"), got, want):
            assert g.dtype == w.dtype and np.array_equal(bits(g), bits(w)), (what, u, name)
        assert np.array_equal(new.next_id, old.next_id), (what, u, new.next_id, old.next_id)


def random_frames(seed, streams=1, J=17, frames=10):
    """people coming and going, every box non-empty; with several streams the counts ride along"""
    rng = np.random.default_rng(seed)
    pools = [people(rng, 6, J)[0] for _ in range(streams)]
    out = []
    for u in range(frames):
        b, p, counts = [], [], []
        for pool in pools:
            who = np.flatnonzero(rng.random(6) < (0.0 if u == 3 else 0.7))
            pts, boxes = people(rng, len(who), J, jitter=2.0, base=pool[rng.permutation(who)])
            b.append(boxes), p.append(pts), counts.append(len(who))
        out.append((np.concatenate(b), np.concatenate(p)) + ((counts,) if streams > 1 else ()))
    return out


@pytest.mark.parametrize("one_euro", [None, dict(min_cutoff=1.5, beta=0.01)])
def test_max_lost_zero_is_the_tracker_as_it_was(one_euro):
    for seed in range(4):
        assert_trackers_agree(random_frames(seed), ("random", seed), one_euro=one_euro)
        assert_trackers_agree(random_frames(10 + seed, streams=3), ("streams", seed), one_euro=one_euro)
    assert_trackers_agree(sequence(), "sequence", one_euro=one_euro)
    assert_trackers_agree(sequence(j=16, seed=9), "sequence16", one_euro=one_euro, smoothing_alpha=0.0)
    # exact ties: every person three times on both sides (the tie rule alone decides)
    base = make_case(77, 4, 4, 17, jitter=0.0)
    first = (np.concatenate([base["prev_boxes"]] * 3), np.concatenate([base["prev_pts"]] * 3))
    second = (np.concatenate([base["boxes"]] * 3), np.concatenate([base["pts"]] * 3))
    assert_trackers_agree([first, second, first, second], "ties", one_euro=one_euro)


@pytest.mark.parametrize("k", [int(v) for v in G["track_cases"]])
def test_reference_fixtures_through_a_loaded_table(k):
    g = {n: G["track%d_%s" % (k, n)] for n in ("boxes", "pts", "prev_boxes", "prev_pts", "prev_ids", "params", "out_boxes", "out_pts", "out_ids")}
    m, J = len(g["prev_boxes"]), g["pts"].shape[1]
    table = pp.new_track_table(1, 8, J)
    table["slot_id"][0, :m], table["slot_row"][0, :m], table["slot_hits"][0, :m] = g["prev_ids"], np.arange(m), 1
    table["slot_boxes"][0, :m], table["slot_pts"][0, :m] = g["prev_boxes"], g["prev_pts"]
    table["next_id"][0] = int(G["track%d_next_id" % k])
    alpha, thr, smooth = (float(v) for v in g["params"])
    boxes, pts, ids, match_row, slot, status = pp.track_people(g["boxes"].copy(), g["pts"].copy(), table, alpha, thr, smooth, 0, False, 0.5)
    np.testing.assert_array_equal(ids, g["out_ids"])
    np.testing.assert_array_equal(boxes, g["out_boxes"])
    np.testing.assert_array_equal(bits(pts), bits(g["out_pts"]))
    assert status.tolist() == [0] and table["next_id"].tolist() == [max(int(G["track%d_next_id" % k]), int(ids.max()) + 1)]


# ---- designed cases ------------------------------------------------------------------------------------------------------------
def walkers(J=17, updates=14, seed=3, speed=3.0):
    """three people at constant velocity: per update (boxes, pts) of all three"""
    rng = np.random.default_rng(seed)
    pts0 = people(rng, 3, J)[0]
    vel = (rng.uniform(-1, 1, (3, 1, 2)) * speed).astype(np.float32)
    out = []
    for u in range(updates):
        pts = pts0.copy()
        pts[:, :, :2] += vel * u
        out.append((ref.boxes_of(pts), pts))
    return out


@pytest.mark.parametrize("coast", [False, True])
@pytest.mark.parametrize("max_lost", [1, 4])
def test_an_occluded_person_keeps_their_id_for_max_lost_updates(max_lost, coast):
    pkg = load_pkg()
    frames = walkers()
    for gap in (1, max_lost, max_lost + 1):
        trk, old = pkg.PersonTracker(None, max_lost=max_lost, coast=coast), pkg.PersonTracker(None)
        for u in range(3):
            ids = trk.update(*frames[u])[2]
            old_ids = old.update(*frames[u])[2]
        assert ids.tolist() == [0, 1, 2] and old_ids.tolist() == [0, 1, 2]
        before = trk.next_id.copy()
        for u in range(3, 3 + gap):                                    # person 1 is behind the pillar
            ids = trk.update(frames[u][0][[0, 2]], frames[u][1][[0, 2]])[2]
            old.update(frames[u][0][[0, 2]], frames[u][1][[0, 2]])
            assert ids.tolist() == [0, 2]
        lost = trk.lost()
        assert lost[0].tolist() == ([1] if gap <= max_lost else []) and lost[3].tolist() == ([gap] if gap <= max_lost else [])
        ids = trk.update(*frames[3 + gap])[2]
        old_ids = old.update(*frames[3 + gap])[2]
        if gap <= max_lost:
            assert ids.tolist() == [0, 1, 2] and np.array_equal(trk.next_id, before), (gap, ids, trk.next_id)
        else:
            assert ids[[0, 2]].tolist() == [0, 2] and ids[1] >= 3 and trk.next_id[0] == ids[1] + 1, (gap, ids)
        assert old_ids[[0, 2]].tolist() == [0, 2] and old_ids[1] >= 3    # the tracker as it was: the returning person is a stranger


def test_a_fast_mover_is_found_again_only_when_coasting():
    """a person whose displacement per update (60 px) exceeds their box (40 px wide), gone for 3 updates.  The speed builds up over
    six updates so that a velocity exists; on return the similarity to the coasted state and to the last-seen state both lie at
    least 0.1 from the threshold (verified below through hrn_associate_similarity)."""
    pkg = load_pkg()
    rng = np.random.default_rng(1)
    J = 17
    shape = np.stack([rng.uniform(0, 200, J), rng.uniform(0, 30, J), rng.uniform(0.5, 1.0, J)], 1).astype(np.float32)
    shape[0, :2], shape[1, :2] = (0, 0), (200, 30)                     # the box: 40 x 210 with the 5 px margin
    speeds = [0, 10, 20, 30, 40, 50, 60, 60, 60]
    xs = np.cumsum(speeds) + 50.0
    bystander = people(np.random.default_rng(2), 1, J)[0]
    bystander[:, :, 0] += 400.0                                        # far below: never confused with the mover

    def frame(x, with_mover=True):
        mover = shape.copy()
        mover[:, 0] += 40
        mover[:, 1] += np.float32(x)
        pts = np.concatenate([mover[None], bystander]) if with_mover else bystander.copy()
        return ref.boxes_of(pts), pts

    back = frame(xs[-1] + 60.0 * 4)
    ids_back = {}
    for coast in (True, False):
        trk = pkg.PersonTracker(None, max_lost=5, coast=coast, smoothing_alpha=0.0, velocity_alpha=1.0)
        for x in xs:
            ids = trk.update(*frame(x))[2]
        mover_id = int(ids[0])
        assert np.array_equal(trk.table["slot_boxes"][0, trk.slot[0]], frame(xs[-1])[0][0])
        if coast:
            assert mover_id == 0 and trk.table["slot_vel"][0, trk.slot[0]].tolist() == [0.0, 60.0]   # velocity_alpha = 1: the last step
        for _ in range(3):
            trk.update(*frame(0, with_mover=False))
        l_ids, l_boxes, l_pts, l_lost = trk.lost()
        assert mover_id in l_ids.tolist() and l_lost[l_ids.tolist().index(mover_id)] == 3
        if coast:
            assert l_ids.tolist() == [mover_id]
        _, sim = ref.similarity(back[0][:1], back[1][:1], l_boxes, l_pts, DEMO[0])   # (without coast: earlier pieces of the track too)
        print("coast %s: similarity of the returning mover to the lost tracks' compared states %s (threshold %.1f)" % (coast, sim[0], DEMO[1]))
        assert (sim[0] >= DEMO[1] + 0.1).all() if coast else (sim[0] <= DEMO[1] - 0.1).all()
        known = int(trk.next_id[0])
        ids_back[coast] = (int(trk.update(*back)[2][0]), mover_id, known)
    assert ids_back[True][0] == ids_back[True][1] and ids_back[False][0] == ids_back[False][2]   # re-identified; a stranger's fresh id


def test_a_zero_row_is_nobody_for_a_hundred_updates():
    pkg = load_pkg()
    frames = walkers(updates=1)
    boxes, pts = np.concatenate([frames[0][0][:1], np.zeros((1, 4), np.int32), frames[0][0][1:]]), \
        np.concatenate([frames[0][1][:1], np.zeros((1, 17, 3), np.float32), frames[0][1][1:]])
    trk, old = pkg.PersonTracker(None, max_lost=2), pkg.PersonTracker(None)
    moved = []
    for u in range(100):
        ids = trk.update(boxes, pts)[2]
        old_ids = old.update(boxes, pts)[2]
        assert ids.tolist() == [0, -1, 1, 2] and trk.slot.tolist() == [0, -1, 1, 2] and trk.next_id.tolist() == [4], (u, ids, trk.next_id)
        moved.append(int(old.next_id[0]))
        if u:
            assert old_ids[1] == moved[-2]                              # the tracker as it was: a fresh id on every frame
    assert moved[1:] == list(range(moved[1], moved[1] + 99))


def test_a_full_table_numbers_the_row_and_leaves_the_slots_alone():
    boxes, pts, table = ref.layout_case(5, 6, 4, 4, 17, packed=True)      # four tracks fill C = 4; two strangers among six rows
    before = ref.copy_table(table)
    want_table = ref.copy_table(table)
    got = pp.track_people(boxes.copy(), pts.copy(), table, *DEMO, 5, False, 0.5)
    want = ref.update(boxes, pts, want_table, *DEMO, 5, False, 0.5)
    assert_outputs_equal(got, want, "full")
    ref.assert_tables_equal(table, want_table, "full")
    ids, slot, status = got[2], got[4], got[5]
    assert status.tolist() == [4] and (slot == -1).sum() == 2 and sorted(ids[slot == -1].tolist()) == [17, 18]
    assert table["next_id"].tolist() == [19] and np.array_equal(table["slot_id"], before["slot_id"])
    assert sorted(slot[slot >= 0].tolist()) == [0, 1, 2, 3]


def test_an_empty_stream_ages_and_retires_its_tracks():
    boxes, pts, table = ref.layout_case(6, 3, 3, 8, 17)
    pp.track_people(boxes, pts, table, *DEMO, 2, True, 0.5)
    live = table["slot_id"][0] >= 0
    assert live.sum() == 3 and (table["slot_lost"][0][live] == 0).all()
    fresh = pp.new_track_table(1, 8, 17)
    nobody = np.zeros((0, 4), np.int32), np.zeros((0, 17, 3), np.float32)
    next_id = table["next_id"].copy()
    for u in (1, 2):
        kept = ref.copy_table(table)
        out = pp.track_people(*nobody, table, *DEMO, 2, True, 0.5)
        assert out[2].shape == (0,) and out[5].tolist() == [0]
        assert (table["slot_lost"][0][live] == u).all() and (table["slot_row"][0] == -1).all()
        for name in ("slot_id", "slot_hits", "slot_boxes", "slot_pts", "slot_vel", "next_id"):
            assert np.array_equal(bits(table[name]), bits(kept[name])), name
    pp.track_people(*nobody, table, *DEMO, 2, True, 0.5)                  # the third update without them: retired
    fresh["next_id"][:] = next_id
    ref.assert_tables_equal(table, fresh, "freed slots are fresh slots, bit for bit")


def test_velocity_alpha_one_is_the_last_displacement():
    frames = walkers(updates=4, speed=0.0)
    table = pp.new_track_table(1, 8, 17)
    shifts = [(0, 0), (7, -3), (2, 9), (-5, 4)]                              # (dx, dy) per update, whole pixels
    for (boxes, pts), (dx, dy) in zip(frames, np.cumsum(shifts, 0)):
        boxes, pts = boxes + np.asarray([dx, dy, dx, dy], np.int32), pts + np.asarray([dy, dx, 0], np.float32)
        pp.track_people(boxes, pts, table, *DEMO[:2], 0.0, 3, True, 1.0)
    assert (table["slot_hits"][0, :3] == 4).all()
    assert table["slot_vel"][0, :3].tolist() == [[4.0, -5.0]] * 3            # (dy, dx) of the last step, exactly


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def refusal_calls():
    """(name, changed arguments, message) over a good call of 2 streams, C = 4, J = 17"""
    return [("P", dict(P=-1), "P is negative"), ("J0", dict(J=0), "HRN_MAX_JOINTS"), ("J257", dict(J=257), "HRN_MAX_JOINTS"),
            ("alpha", dict(pose_alpha=float("nan")), "finite"), ("thr", dict(threshold=float("inf")), "finite"),
            ("smooth", dict(smoothing=1.5), "smoothing_alpha"), ("C0", dict(C=0), "capacity"), ("C257", dict(C=257), "capacity"),
            ("lost-", dict(max_lost=-1), "max_lost"), ("lost+", dict(max_lost=(1 << 20) + 1), "max_lost"), ("coast", dict(coast=2), "coast"),
            ("va0", dict(va=0.0), "velocity_alpha"), ("va2", dict(va=1.5), "velocity_alpha"), ("vanan", dict(va=float("nan")), "velocity_alpha"),
            ("start", dict(start=None), "null segment table"), ("next", dict(next_id=None), "null segment table"),
            ("status", dict(status=None), "null segment table"), ("neg", dict(start=np.asarray([-1, 1, 3], np.int32)), "below zero"),
            ("dec", dict(start=np.asarray([0, 3, 2], np.int32)), "decreases"), ("many", dict(start=np.asarray([0, 257, 258], np.int32)), "HRN_MAX_TRACKED"),
            ("table", dict(slot_pts=None), "null track table"), ("table2", dict(slot_id=None), "null track table"),
            ("rows", dict(boxes=None), "null boxes"), ("out", dict(slot=None), "null boxes")]


def refusal_arguments():
    table = pp.new_track_table(2, 4, 17)
    for name in table:
        table[name][...] = 77
    a = dict(P=2, start=np.asarray([0, 1, 3], np.int32), C=4, J=17, boxes=np.full((3, 4), 77, np.int32), pts=np.full((3, 17, 3), 77, np.float32),
             pose_alpha=0.2, threshold=0.4, smoothing=0.1, max_lost=2, coast=1, va=0.5, ids=np.full(3, 77, np.int32),
             match_row=np.full(3, 77, np.int32), slot=np.full(3, 77, np.int32), status=np.full(2, 77, np.int32))
    a.update(table)
    return a


ORDER = ("boxes", "pts", "slot_id", "slot_lost", "slot_hits", "slot_row", "slot_boxes", "slot_pts", "slot_vel", "next_id")


def call_with(fn, head, a):
    p = lambda v: None if v is None else v.ctypes.data   # noqa: E731
    return fn(*head, a["P"], p(a["start"]), a["C"], a["J"], *[p(a[k]) for k in ORDER], a["pose_alpha"], a["threshold"], a["smoothing"],
              a["max_lost"], a["coast"], a["va"], p(a["ids"]), p(a["match_row"]), p(a["slot"]), p(a["status"]))


def untouched(a):
    return all((v == 77).all() for k, v in a.items() if isinstance(v, np.ndarray) and k != "start")


@pytest.mark.parametrize("name,change,message", refusal_calls())
def test_refusals_name_their_cause_and_write_nothing(name, change, message):
    lib = load_pkg("_lib").load()
    a = dict(refusal_arguments(), **change)
    assert call_with(lib.hrn_track_people, (), a) == 7
    assert message in lib.hrn_track_people_last_error().decode(), (name, lib.hrn_track_people_last_error())
    assert untouched(a), name


def test_refusals_on_a_plan_only_handle():
    net = load_pkg().NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h
    for name, change, message in refusal_calls() + [("good", dict(), "plan-only"), ("nobody", dict(P=0, start=None), "plan-only")]:
        a = dict(refusal_arguments(), **change)
        rc = call_with(lambda *args: L.hrn_track_people_dev(*args, None), (h,), a)
        err = L.hrn_last_error(h).decode()
        assert rc == 7 and message in err, (name, err)
        assert ("plan-only" in err) == (message == "plan-only") and (message == "plan-only" or "hrn_track_people_dev: " in err), (name, err)
        assert untouched(a), name


def test_python_shims_refuse_a_table_that_is_not_one():
    boxes, pts, table = ref.layout_case(1, 2, 2, 4, 17)
    with pytest.raises(ValueError, match="track table"):
        pp.track_people(boxes, pts, {k: v for k, v in table.items() if k != "slot_vel"})
    with pytest.raises(ValueError, match="fit together"):
        pp.track_people(boxes, pts, dict(table, slot_vel=np.zeros((1, 5, 2), np.float32)))
    with pytest.raises(ValueError, match="C-contiguous int32"):
        pp.track_people(boxes, pts, dict(table, slot_id=table["slot_id"].astype(np.int64)))
    with pytest.raises(ValueError, match="streams"):
        pp.track_people(boxes, pts, table, counts=[1, 1])
    with pytest.raises(ValueError, match="hrn_track_people: max_lost"):
        pp.track_people(boxes, pts, table, max_lost=-1)
    with pytest.raises(ValueError, match="capacity"):
        pp.new_track_table(1, 257, 17)
