"""Joints over time on the GPU: NativeHRNet.filter_poses against the host form (bit for bit: both compile
csrc/temporal_math.h) for every output -- pts_out, pred, state, age --, a sequence with the state fed back on the device,
PersonTracker(one_euro=...) on device tensors against its host run, and the whole device loop track_frame(predicted) -> update ->
draw_poses on a tiny engine against the loop with downloads and the host forms in between.

Shapes are the smallest that reach each branch of csrc/temporal.hip and its entry: nobody on either side; one joint; fewer and more
previous people than current ones; J = 1 / 17 / 133 / 256; n * J = 255 / 256 / 272 around the block edge; 300 x 17 (several
blocks); 256 x 256 once; four streams with an empty one (the segment table goes through the upload); no match at all; matches out
of range; the poisoned coordinates of the host test."""
import numpy as np
import pytest
import torch

import temporal_ref as ref
from conftest import load_pkg, state_dict_np
from temporal_ref import DEFAULTS, ONE_EURO, bits, random_sequence, run_sequence, tracker_frames

pytestmark = pytest.mark.gpu

_NETS = {}
SKELETON = [[15, 13], [13, 11], [16, 14], [14, 12], [11, 12], [5, 11], [6, 12], [5, 6], [5, 7], [6, 8], [7, 9], [8, 10], [1, 2], [0, 1],
            [0, 2], [1, 3], [2, 4], [3, 5], [4, 6]]
NAMES = ("pts_out", "pred", "state", "age")


def engine(dtype="fp32"):
    if dtype not in _NETS:
        _NETS[dtype] = load_pkg().NativeHRNet(32, 17, (64, 64), dtype, max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    return _NETS[dtype]


def make_case(seed, n, m, J, counts=None, prev_counts=None, match="random", poisoned=False):
    """m previous people two frames old (so that their state holds a velocity), n current ones; `match`: "random" (a partial
    permutation per stream with -1 and values out of range), "wild" (everything out of range) or None"""
    pp = load_pkg("postproc")
    rng = np.random.default_rng(seed)

    def frame(k, base=None):
        pts = np.empty((k, J, 3), np.float32)
        pts[:, :, :2] = rng.uniform(0, 1000, (k, J, 2)) if base is None else base[:, :, :2] + rng.normal(0, 3, (k, J, 2)).astype(np.float32)
        pts[:, :, 2] = np.where(rng.random((k, J)) < 0.2, rng.uniform(0, 0.5, (k, J)), rng.uniform(0.5, 1.0, (k, J)))
        return pts

    older = frame(m)
    old = frame(m, older)
    _, _, state = pp.filter_poses(older, **DEFAULTS)
    cur_counts, before_counts = [n] if counts is None else counts, [m] if prev_counts is None else prev_counts
    same = np.concatenate([np.arange(c, dtype=np.int32) for c in before_counts])
    _, _, state = pp.filter_poses(old, state, same, counts=prev_counts, prev_counts=prev_counts, **DEFAULTS)
    found = None
    if match == "random":
        found = np.concatenate([ref.random_match(rng, c, pc) for c, pc in zip(cur_counts, before_counts)] + [np.zeros(0, np.int32)]).astype(np.int32)
    elif match == "wild":
        found = rng.choice([m, m + 1, -2, 2 ** 31 - 1, -2 ** 31], n).astype(np.int32)
    pts = frame(n)
    before = ref.previous_index(found, cur_counts, before_counts, n, m)
    for i in np.flatnonzero(before >= 0):
        pts[i, :, :2] = old[before[i], :, :2] + rng.normal(0, 3, (J, 2)).astype(np.float32)
    if poisoned:
        pts = ref.poison(rng, pts)
    return dict(pts=pts, state=state, match=found, counts=counts, prev_counts=prev_counts)


def both(case, dt=1 / 30, net=None, **kw):
    """(device results as numpy, host results) of one case: (pts_out, pred, state, age)"""
    pp, net = load_pkg("postproc"), net or engine()
    params = dict(DEFAULTS, dt=dt, counts=case["counts"], prev_counts=case["prev_counts"], **kw)
    w = pp.filter_poses(case["pts"], case["state"], case["match"], **params)
    given = [torch.from_numpy(case["pts"]).cuda(), tuple(torch.from_numpy(s).cuda() for s in case["state"]),
             None if case["match"] is None else torch.from_numpy(case["match"]).cuda()]
    kept = [given[0].clone(), given[1][0].clone(), given[1][1].clone()]
    g = net.filter_poses(*given, **params)
    assert all(t.is_cuda for t in (g[0], g[1], g[2][0], g[2][1]))
    assert torch.equal(kept[0].view(torch.int32), given[0].view(torch.int32)) and torch.equal(kept[1], given[1][0]) and torch.equal(kept[2], given[1][1])
    return [g[0].cpu().numpy(), g[1].cpu().numpy(), g[2][0].cpu().numpy(), g[2][1].cpu().numpy()], [w[0], w[1], w[2][0], w[2][1]]


def assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, name)


@pytest.mark.parametrize("J", [1, 17, 133, 256])
def test_small_shapes_equal_the_host_form(J):
    filtered = 0
    for n, m in ((0, 3), (3, 0), (1, 1), (2, 5), (5, 2)):
        got, want = both(make_case(50 * n + 7 * m + J, n, m, J))
        assert_same(got, want, (n, m, J))
        filtered += int((want[3] > 1).sum())
    assert filtered > 0                                                           # somebody was filtered, not only initialised


@pytest.mark.parametrize("n,J", [(15, 17), (16, 16), (16, 17), (300, 17), (256, 256)])
def test_the_block_edge_and_several_blocks_equal_the_host_form(n, J):
    got, want = both(make_case(n + J, n, n + 3, J, poisoned=True), dt=0.04171)
    assert_same(got, want, (n, J))
    assert (want[3] > 1).sum() >= n * J // 4


def test_four_streams_in_one_launch_equal_the_host_form_and_four_calls():
    counts, prev_counts = [3, 0, 70, 6], [5, 2, 66, 0]
    case = make_case(31, sum(counts), sum(prev_counts), 17, counts, prev_counts, poisoned=True)
    got, want = both(case)
    assert_same(got, want, "streams")
    cur, prev = ref.segments(counts, sum(counts)), ref.segments(prev_counts, sum(prev_counts))
    for p in range(4):
        one = dict(pts=np.ascontiguousarray(case["pts"][cur[p]:cur[p + 1]]), match=np.ascontiguousarray(case["match"][cur[p]:cur[p + 1]]),
                   state=tuple(np.ascontiguousarray(s[prev[p]:prev[p + 1]]) for s in case["state"]), counts=None, prev_counts=None)
        single, _ = both(one)
        assert_same(single, [g[cur[p]:cur[p + 1]] for g in got], p)


def test_no_match_a_wild_match_and_poisoned_coordinates_equal_the_host_form():
    for kind in (None, "wild"):
        got, want = both(make_case(9, 6, 4, 17, match=kind))
        assert_same(got, want, kind)
        assert (want[3] <= 1).all() and (want[3] == 1).any()                          # nobody has a prior
    got, want = both(make_case(10, 9, 9, 17, poisoned=True), lookahead=0.25)
    assert_same(got, want, "poisoned")
    assert (want[3] > 1).any()


def test_a_sequence_with_the_state_on_the_device_equals_the_host_sequence():
    pp, net = load_pkg("postproc"), engine()
    seq = random_sequence(2024, 17, 3)
    want = run_sequence(pp.filter_poses, seq, DEFAULTS)
    got = run_sequence(net.filter_poses, seq, DEFAULTS)
    for k, (g, w) in enumerate(zip(got, want)):
        assert all(t.is_cuda for t in g)
        assert_same([t.cpu().numpy() for t in g], w, k)
    assert max(int(w[3].max(initial=0)) for w in want) >= 3


def test_a_non_default_stream_gives_the_same_bits():
    case = make_case(4, 40, 40, 17)
    plain, want = both(case)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, _ = both(case)
    side.synchronize()
    assert_same(got, want, "side stream")
    assert_same(got, plain, "both streams")


def _raw(net, case, pts_out=None, want_pred=True, numbers=None, J=None, fill=0x7fc54321):
    """hrn_filter_poses_dev through the one launch path, on tensors as given; returns (pts_out, pred, state, age) tensors pre-filled
    with `fill` (pts_out: the tensor passed in, e.g. the input itself)"""
    dev = net.torch_device
    pts = torch.from_numpy(case["pts"]).to(dev)
    n, joints = int(pts.shape[0]), int(pts.shape[1])
    state = [torch.from_numpy(s).to(dev) for s in case["state"]]
    match = torch.from_numpy(case["match"]).to(dev)
    outs = [pts if pts_out == "in place" else torch.full((n, joints, 3), fill, dtype=torch.int32, device=dev).view(torch.float32),
            torch.full((n, joints, 3), fill, dtype=torch.int32, device=dev).view(torch.float32),
            torch.full((n, joints, 6), fill, dtype=torch.int32, device=dev).view(torch.float32), torch.full((n, joints), fill, dtype=torch.int32, device=dev)]
    cur, prev = np.asarray([0, n], np.int32), np.asarray([0, len(case["state"][0])], np.int32)
    numbers = numbers or (1 / 30, 1.0, 0.007, 1.0, 0.5, 1 / 30)
    net._launch("hrn_filter_poses_dev", 1, cur.ctypes.data, prev.ctypes.data, joints if J is None else J, pts.data_ptr(), match.data_ptr(),
                state[0].data_ptr(), state[1].data_ptr(), *numbers, outs[0].data_ptr(), outs[1].data_ptr() if want_pred else None,
                outs[2].data_ptr(), outs[3].data_ptr())
    return outs


def test_in_place_and_without_a_prediction():
    net = engine()
    case = make_case(21, 20, 20, 17)
    want = [t.cpu().numpy() for t in _raw(net, case)]
    _, host = both(case)
    assert_same(want, host, "raw call")
    got = [t.cpu().numpy() for t in _raw(net, case, pts_out="in place")]
    assert_same(got, want, "in place")
    got = [t.cpu().numpy() for t in _raw(net, case, want_pred=False)]
    assert (got[1].view(np.uint32) == 0x7fc54321).all()
    assert_same([got[0], got[2], got[3]], [want[0], want[2], want[3]], "no prediction")


def test_refusals_leave_the_outputs_as_they_were():
    pkg, net = load_pkg(), engine()
    case = make_case(22, 5, 5, 17)
    d = (1 / 30, 1.0, 0.007, 1.0, 0.5, 1 / 30)
    for kw, text in ((dict(J=0), "J must be"), (dict(J=257), "J must be"), (dict(numbers=(0.0,) + d[1:]), "finite and positive"),
                     (dict(numbers=d[:2] + (-1.0,) + d[3:]), "finite and not negative"), (dict(numbers=d[:5] + (float("nan"),)), "not negative")):
        with pytest.raises(RuntimeError, match=text):
            _raw(net, case, **kw)
    pts = torch.from_numpy(case["pts"]).cuda()
    state = [torch.from_numpy(s).cuda() for s in case["state"]]
    match = torch.from_numpy(case["match"]).cuda()
    sentinel = [torch.full(shape, 0x7fc54321, dtype=torch.int32, device="cuda") for shape in ((5, 17, 3), (5, 17, 3), (5, 17, 6), (5, 17))]
    cur = np.asarray([0, 5], np.int32)

    def call(handle, lib, cur_table, prev_table, state0, out_state, dt=1 / 30):
        return lib.hrn_filter_poses_dev(handle, 1, cur_table, prev_table, 17, pts.data_ptr(), match.data_ptr(), state0, state[1].data_ptr(), dt, 1.0,
                                        0.007, 1.0, 0.5, 1 / 30, sentinel[0].data_ptr(), sentinel[1].data_ptr(), out_state, sentinel[3].data_ptr(), 0)

    lib, h = net._lib, net._h
    down = np.asarray([3, 0], np.int32)
    assert call(h, lib, cur.ctypes.data, down.ctypes.data, state[0].data_ptr(), sentinel[2].data_ptr()) == 7 and b"decreases" in lib.hrn_last_error(h)
    assert call(h, lib, None, cur.ctypes.data, state[0].data_ptr(), sentinel[2].data_ptr()) == 7 and b"null segment tables" in lib.hrn_last_error(h)
    assert call(h, lib, cur.ctypes.data, cur.ctypes.data, None, sentinel[2].data_ptr()) == 7 and b"beside a match" in lib.hrn_last_error(h)
    assert call(h, lib, cur.ctypes.data, cur.ctypes.data, state[0].data_ptr(), state[0].data_ptr() + 24) == 7 and b"overlap" in lib.hrn_last_error(h)
    # a plan-only handle is refused, but only after the argument errors
    plan = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=1, device=-1)
    assert call(plan._h, lib, cur.ctypes.data, cur.ctypes.data, state[0].data_ptr(), sentinel[2].data_ptr(), dt=-1.0) == 7
    assert b"finite and positive" in lib.hrn_last_error(plan._h)
    assert call(plan._h, lib, cur.ctypes.data, cur.ctypes.data, state[0].data_ptr(), sentinel[2].data_ptr()) == 7
    assert b"plan-only" in lib.hrn_last_error(plan._h)
    plan.close()
    torch.cuda.synchronize()
    assert all(bool((t == 0x7fc54321).all()) for t in sentinel)
    assert torch.equal(state[0].cpu(), torch.from_numpy(case["state"][0]))
    assert call(h, lib, cur.ctypes.data, cur.ctypes.data, state[0].data_ptr(), sentinel[2].data_ptr()) == 0      # and the same call, accepted
    torch.cuda.synchronize()
    assert not any(bool((t == 0x7fc54321).all()) for t in sentinel)


@pytest.mark.parametrize("streams", [1, 3])
def test_tracker_on_the_device_equals_the_host_run(streams):
    pkg = load_pkg()
    host, dev = pkg.PersonTracker(None, one_euro=ONE_EURO), pkg.PersonTracker(engine(), one_euro=ONE_EURO)
    dts = [None, None, 0.05, None, 1 / 30, None]
    for (boxes, pts, counts), dt in zip(tracker_frames(streams), dts):
        want = host.update(boxes, pts, counts=counts, dt=dt)
        given = torch.from_numpy(boxes).cuda(), torch.from_numpy(pts).cuda()
        got = dev.update(*given, counts=counts, dt=dt)
        assert all(t.is_cuda for t in got) and dev.predicted.is_cuda and all(t.is_cuda for t in dev.filter_state)
        assert torch.equal(given[0].cpu(), torch.from_numpy(boxes)) and torch.equal(given[1].cpu(), torch.from_numpy(pts))
        for g, w in zip(list(got) + [dev.predicted, *dev.filter_state, dev.prev_pts], list(want) + [host.predicted, *host.filter_state, host.prev_pts]):
            assert np.array_equal(bits(g.cpu().numpy()), bits(w))
    assert int(host.filter_state[1].max()) >= 2


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_device_loop_with_prediction_equals_the_loop_through_the_host(dtype):
    """predict_frame on frame 0, then track_frame(frame, tracker.predicted) -> PersonTracker.update -> draw_poses over four frames,
    all on the device, against the same loop with the joints downloaded, the host forms, and an upload in between"""
    pkg = load_pkg()
    net = engine(dtype)
    rng = np.random.default_rng(8)
    frames = [rng.integers(0, 256, (120, 160, 3), dtype=np.uint8) for _ in range(5)]
    dets = np.asarray([[10.2, 8.7, 90.4, 100.1], [60.5, 20.5, 150.0, 70.0], [30.0, 40.0, 120.0, 118.0]], np.float32)
    box_args = dict(threshold=-1.0, min_joints=1)               # synthetic weights: every joint counts, nobody is lost
    one_euro = dict(ONE_EURO, threshold=-1.0)

    boxes0, pts0 = net.predict_frame(torch.from_numpy(frames[0]).cuda(), dets)
    dev, host = pkg.PersonTracker(net, one_euro=one_euro), pkg.PersonTracker(None, one_euro=one_euro)
    dev.update(torch.from_numpy(boxes0).cuda(), pts0)
    host.update(boxes0, pts0.cpu().numpy())
    for k in (1, 2, 3, 4):
        frame = torch.from_numpy(frames[k]).cuda()
        t_boxes, t_pts, t_status = net.track_frame(frame, dev.predicted, **box_args)
        d_boxes, d_pts, d_ids = dev.update(t_boxes, t_pts)
        canvas = net.draw_poses(frame.clone(), d_pts, SKELETON, person_ids=d_ids)
        assert all(t.is_cuda for t in (t_boxes, t_pts, t_status, d_boxes, d_pts, d_ids, canvas, dev.next_id, dev.predicted))
        # the same step through the host
        u_boxes, u_pts, _ = net.track_frame(frame, torch.from_numpy(host.predicted).cuda(), **box_args)
        h_boxes, h_pts, h_ids = host.update(u_boxes.cpu().numpy(), u_pts.cpu().numpy())
        want = net.draw_poses(frame.clone(), h_pts, SKELETON, person_ids=h_ids)
        assert np.array_equal(d_ids.cpu().numpy(), h_ids) and np.array_equal(d_boxes.cpu().numpy(), h_boxes), k
        assert np.array_equal(bits(d_pts.cpu().numpy()), bits(h_pts)), k
        assert np.array_equal(bits(dev.predicted.cpu().numpy()), bits(host.predicted)), k
        assert torch.equal(canvas, want), k
        assert dev.next_id.cpu().tolist() == host.next_id.tolist()
    assert int(host.filter_state[1].max()) >= 2                 # states did live on: joints were filtered, not only initialised
