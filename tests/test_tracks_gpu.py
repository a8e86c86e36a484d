"""The person track table on the GPU: hrn_track_people_dev against the host form bit for bit (both compile csrc/tracks_math.h and
csrc/assoc_math.h) -- every output and the WHOLE table, over sentinel-filled output buffers -- then fed-back sequences,
PersonTracker on device tensors against its host run, and the device video loop against the loop through the host.

Shapes are the smallest that reach each branch of csrc/tracks.hip: no rows / no columns (the assignment is skipped, every barrier
still reached); 63 / 64 / 65 and 255 / 256 on either side (one pass of a wave, one element into the next, the cap); C = 1 / 4 / 65 /
256; J = 1 / 17 / 133 / 256 (float32 sigmas, fp64 sigmas, numpy's pairwise recursion, the cap)."""
import numpy as np
import pytest
import torch

import tracks_ref as ref
from assoc_cases import DEMO
from conftest import load_pkg, state_dict_np

pytestmark = pytest.mark.gpu

pp = load_pkg("postproc")
_NETS = {}
SENTINEL = 77
SKELETON = [[15, 13], [13, 11], [16, 14], [14, 12], [11, 12], [5, 11], [6, 12], [5, 6], [5, 7], [6, 8], [7, 9], [8, 10], [1, 2], [0, 1],
            [0, 2], [1, 3], [2, 4], [3, 5], [4, 6]]
ORDER = ("slot_id", "slot_lost", "slot_hits", "slot_row", "slot_boxes", "slot_pts", "slot_vel", "next_id")


def engine(mode="fp32"):
    if mode not in _NETS:
        _NETS[mode] = load_pkg().NativeHRNet(32, 17, (64, 64), mode, max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    return _NETS[mode]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def to_device(table):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in table.items()}


def to_host(table):
    return {k: v.cpu().numpy() for k, v in table.items()}


def device_update(boxes, pts, table, params, counts=None):
    """hrn_track_people_dev on copies of the inputs, its four output arrays filled with a sentinel first: (outputs, table) as numpy"""
    net = engine()
    P, C, J = pp.track_table_shape(table, lambda a: a.shape)
    n = len(boxes)
    start = np.concatenate([[0], np.cumsum([n] if counts is None else counts)]).astype(np.int32)
    d_boxes, d_pts, d_table = torch.from_numpy(boxes.copy()).cuda(), torch.from_numpy(pts.copy()).cuda(), to_device(table)
    outs = [torch.full((max(n, 1),), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
    status = torch.full((P,), SENTINEL, dtype=torch.int32, device="cuda")
    pose_alpha, threshold, smoothing, max_lost, coast, va = params
    net._launch("hrn_track_people_dev", P, start.ctypes.data, C, J, d_boxes.data_ptr() if n else None, d_pts.data_ptr() if n else None,
                *[d_table[k].data_ptr() for k in ORDER], float(pose_alpha), float(threshold), float(smoothing), int(max_lost), int(coast),
                float(va), *[o.data_ptr() if n else None for o in outs], status.data_ptr())
    if n == 0:
        assert all((o == SENTINEL).all() for o in outs)
    return [d_boxes.cpu().numpy(), d_pts.cpu().numpy()] + [o[:n].cpu().numpy() for o in outs] + [status.cpu().numpy()], to_host(d_table)


def assert_same(got, want, what):
    for name, g, w in zip(("boxes", "pts", "ids", "match_row", "slot", "status"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(bits(g), bits(w)), (what, name, np.argwhere(bits(g) != bits(w))[:4].tolist())


def check(boxes, pts, table, params, what, counts=None):
    """the device against the host form on one update; returns the host outputs and table"""
    want_table = ref.copy_table(table)
    want = pp.track_people(boxes.copy(), pts.copy(), want_table, *params, counts=counts)
    got, got_table = device_update(boxes, pts, table, params, counts)
    assert_same(got, want, what)
    ref.assert_tables_equal(got_table, want_table, what)
    return want, want_table


def options():
    return [(DEMO[0], DEMO[1], sm, ml, coast, 0.5) for ml, coast, sm in ((0, False, 0.1), (5, True, 0.1), (5, False, 0.0), (0, True, 0.0))]


@pytest.mark.parametrize("n,live,C", [(0, 0, 4), (0, 64, 256), (1, 0, 1), (1, 1, 1), (2, 1, 1), (63, 64, 65), (64, 64, 65), (65, 65, 65), (64, 65, 256),
                                      (65, 1, 4), (1, 65, 65), (255, 64, 256), (256, 0, 256), (0, 256, 256), (6, 4, 4)])
def test_sizes_equal_the_host_form(n, live, C):
    for k, params in enumerate(options()):
        boxes, pts, table = ref.layout_case(1000 * n + 10 * live + k, n, live, C, 17, lost_every=3 if live > 1 else 0)
        want, _ = check(boxes, pts, table, params, (n, live, C, params))
        if n and live:
            assert (want[4] >= 0).any() and ((want[2] >= 0) & (want[2] < 3 * live + 5) & (want[2] % 3 == 1)).any()   # ids carried over


@pytest.mark.parametrize("n,live", [(255, 256), (256, 255), (256, 256)])
def test_the_cap_equals_the_host_form(n, live):
    for params in options()[:2]:
        boxes, pts, table = ref.layout_case(n + live, n, live, 256, 17, lost_every=2)
        want, want_table = check(boxes, pts, table, params, (n, live, params))
        assert (want[4] >= 0).sum() >= 200 and (n < 256 or live < 256 or (want[5] & 4).all() == (want[4] < 0).any())


@pytest.mark.parametrize("J", [1, 133, 256])
def test_joint_counts_equal_the_host_form(J):
    for k, params in enumerate(options()):
        for n, live, C in ((5, 7, 16), (9, 4, 4), (33, 40, 65)):
            check(*ref.layout_case(J + k, n, live, C, J, lost_every=2), params, (J, n, live, C, params))


@pytest.mark.parametrize("layout", ["holes", "full", "all lost", "rows absent", "some absent", "ties"])
def test_table_layouts_equal_the_host_form(layout):
    kw = {"holes": dict(n=20, live=24, C=65, lost_every=3), "full": dict(n=70, live=65, C=65, lost_every=4, packed=True),
          "all lost": dict(n=12, live=16, C=65, lost_every=1), "rows absent": dict(n=9, live=12, C=16, lost_every=3, absent_every=1),
          "some absent": dict(n=30, live=24, C=65, lost_every=3, absent_every=4), "ties": dict(n=18, live=12, C=16, lost_every=4, ties=True)}[layout]
    n, live, C = kw.pop("n"), kw.pop("live"), kw.pop("C")
    for k, params in enumerate(options()):
        boxes, pts, table = ref.layout_case(40 + k, n, live, C, 17, **kw)
        want, want_table = check(boxes, pts, table, params, (layout, params))
        if layout == "rows absent":
            assert (want[2] == -1).all() and (want[4] == -1).all() and want_table["next_id"].tolist() == [3 * live + 5]
        if layout == "full":
            assert want[5].tolist() == [4] and (want[4] == -1).sum() >= 5
        if layout == "all lost" and params[3] == 0:
            assert (want[3] == -1).all()


def four_streams(seed, J=17, C=16):
    shapes = [(5, 7), (0, 6), (40, 12), (3, 0)]
    parts = [ref.layout_case(seed + k, n, live, C, J, lost_every=2) for k, (n, live) in enumerate(shapes)]
    table = {k: np.ascontiguousarray(np.concatenate([p[2][k] for p in parts])) for k in parts[0][2]}
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), table, [s[0] for s in shapes], parts


def test_four_streams_in_one_launch_with_an_empty_one():
    for params in options():
        boxes, pts, table, counts, parts = four_streams(7)
        want, want_table = check(boxes, pts, table, params, ("streams", params), counts=counts)
        singles = [pp.track_people(b.copy(), p.copy(), t, *params) for b, p, t in parts]
        for k in range(6):
            assert np.array_equal(bits(want[k]), bits(np.concatenate([s[k] for s in singles]))), k
        assert (want_table["slot_lost"][1][want_table["slot_id"][1] >= 0] >= 1).all()          # the empty stream aged its tracks


def test_a_side_stream_and_scratch_reuse_after_a_larger_call():
    net = engine()
    big = ref.layout_case(3, 200, 180, 256, 17, lost_every=2)
    small = ref.layout_case(4, 5, 6, 16, 17, lost_every=2)
    params = options()[1]
    check(*big, params, "big")
    check(*small, params, "small after big")
    side = torch.cuda.Stream()
    want_table = ref.copy_table(small[2])
    want = pp.track_people(small[0].copy(), small[1].copy(), want_table, *params)
    with torch.cuda.stream(side):
        table = to_device(small[2])
        got = net.track_people(torch.from_numpy(small[0]).cuda(), torch.from_numpy(small[1]).cuda(), table, *params)
    side.synchronize()
    assert_same([t.cpu().numpy() for t in got], want, "side stream")
    ref.assert_tables_equal(to_host(table), want_table, "side stream")


def test_refusals_leave_the_sentinels():
    net = engine()
    boxes, pts, table = ref.layout_case(1, 3, 3, 4, 17)
    d_table = to_device(table)
    d_boxes, d_pts = torch.from_numpy(boxes).cuda(), torch.from_numpy(pts).cuda()
    for kw, message in ((dict(max_lost=-1), "max_lost"), (dict(velocity_alpha=0.0), "velocity_alpha"), (dict(smoothing_alpha=2.0), "smoothing_alpha"),
                        (dict(coast=2), "coast")):
        with pytest.raises(RuntimeError, match=message):
            net.track_people(d_boxes, d_pts, d_table, **kw)
    big = ref.layout_case(2, 257, 2, 4, 17)
    with pytest.raises(RuntimeError, match="HRN_MAX_TRACKED"):
        net.track_people(big[0], big[1], d_table)
    ref.assert_tables_equal(to_host(d_table), table, "refused")
    assert np.array_equal(d_boxes.cpu().numpy(), boxes) and np.array_equal(bits(d_pts.cpu().numpy()), bits(pts))


@pytest.mark.parametrize("J,P,C,k", [(17, 3, 16, 1), (133, 1, 4, 2), (1, 3, 256, 0)])
def test_a_fed_back_sequence_equals_the_host_sequence(J, P, C, k):
    net = engine()
    params = options()[k]
    host, dev = pp.new_track_table(P, C, J), net.new_track_table(P, C, J)
    for u, (boxes, pts, counts) in enumerate(ref.sequence_frames(60 + k, P, J)):
        want = pp.track_people(boxes.copy(), pts.copy(), host, *params, counts=counts)
        got = net.track_people(torch.from_numpy(boxes.copy()).cuda(), torch.from_numpy(pts.copy()).cuda(), dev, *params, counts=counts)
        assert all(t.is_cuda for t in got)
        assert_same([t.cpu().numpy() for t in got], want, (J, P, C, u))
        ref.assert_tables_equal(to_host(dev), host, (J, P, C, u))


@pytest.mark.parametrize("one_euro", [None, dict(min_cutoff=1.5, beta=0.01)])
def test_tracker_on_the_device_equals_the_host_run(one_euro):
    pkg = load_pkg()
    for P in (1, 2):
        host = pkg.PersonTracker(None, max_lost=5, coast=True, one_euro=one_euro)
        dev = pkg.PersonTracker(engine(), max_lost=5, coast=True, one_euro=one_euro)
        for u, (boxes, pts, counts) in enumerate(ref.sequence_frames(21 + P, P, 17, special=False)):
            want = host.update(boxes, pts, counts=counts)
            got = dev.update(torch.from_numpy(boxes).cuda(), torch.from_numpy(pts).cuda(), counts=counts)
            assert all(t.is_cuda for t in got) and dev.next_id.is_cuda
            for g, w in zip(got, want):
                assert np.array_equal(bits(g.cpu().numpy()), bits(w)), (P, u)
            assert dev.next_id.cpu().tolist() == host.next_id.tolist()
            if dev.table is not None:
                ref.assert_tables_equal(to_host(dev.table), host.table, (P, u))
                for g, w in zip(dev.lost(), host.lost()):
                    assert np.array_equal(bits(g.cpu().numpy()), bits(w)), (P, u, "lost")
            if one_euro is not None:
                assert np.array_equal(bits(dev.predicted.cpu().numpy()), bits(host.predicted))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_device_loop_equals_the_loop_through_the_host(mode):
    """predict_frame on frame 0, then track_frame -> PersonTracker.update -> draw_poses(person_ids=ids) over four frames, all on the
    device, against the same loop with the joints downloaded, the host tracker, and its ids uploaded for the overlay"""
    pkg = load_pkg()
    net = engine(mode)
    rng = np.random.default_rng(8)
    frames = [rng.integers(0, 256, (120, 160, 3), dtype=np.uint8) for _ in range(5)]
    dets = np.asarray([[10.2, 8.7, 90.4, 100.1], [60.5, 20.5, 150.0, 70.0], [30.0, 40.0, 120.0, 118.0]], np.float32)
    box_args = dict(threshold=-1.0, min_joints=1)               # synthetic weights: every joint counts
    kw = dict(max_lost=5, coast=True)

    boxes0, pts0 = net.predict_frame(torch.from_numpy(frames[0]).cuda(), dets)
    dev, host = pkg.PersonTracker(net, **kw), pkg.PersonTracker(None, **kw)
    d_boxes, d_pts, d_ids = dev.update(torch.from_numpy(boxes0).cuda(), pts0)
    h_boxes, h_pts, h_ids = host.update(boxes0, pts0.cpu().numpy())
    for k in (1, 2, 3, 4):
        frame = torch.from_numpy(frames[k]).cuda()
        t_boxes, t_pts, _ = net.track_frame(frame, d_pts, **box_args)
        if k == 2:                                              # somebody is missed for a frame: the library's zero row
            t_boxes[1], t_pts[1] = 0, 0
        d_boxes, d_pts, d_ids = dev.update(t_boxes, t_pts)
        canvas = net.draw_poses(frame.clone(), d_pts, SKELETON, person_ids=d_ids)
        assert all(t.is_cuda for t in (d_boxes, d_pts, d_ids, canvas, dev.next_id))
        u_boxes, u_pts, _ = net.track_frame(frame, torch.from_numpy(h_pts).cuda(), **box_args)
        if k == 2:
            u_boxes[1], u_pts[1] = 0, 0
        h_boxes, h_pts, h_ids = host.update(u_boxes.cpu().numpy(), u_pts.cpu().numpy())
        want = net.draw_poses(frame.clone(), h_pts, SKELETON, person_ids=h_ids)
        assert np.array_equal(d_ids.cpu().numpy(), h_ids) and np.array_equal(d_boxes.cpu().numpy(), h_boxes), k
        assert np.array_equal(bits(d_pts.cpu().numpy()), bits(h_pts)), k
        assert torch.equal(canvas, want), k
        assert dev.next_id.cpu().tolist() == host.next_id.tolist()
        if k == 2:
            assert h_ids[1] == -1
