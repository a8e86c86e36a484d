"""Person ids between two frames on the GPU: NativeHRNet.associate_people against the host form (bit for bit: both compile
csrc/assoc_math.h), PersonTracker on device tensors against its host run, draw_poses with ids on the device against ids from the
host, and the whole device loop on a tiny engine against the loop with downloads and postproc in between.

Shapes are the smallest that reach each branch of csrc/assoc.hip: an empty side; one pair; more columns than rows and the
transposed case; 64 / 65 columns (one pass of the wave, one column into the second) and 70 x 130 (a partial last pass, three
passes); the cap once; J = 17 / 16 / 133 (fp64 sigmas, float32 sigmas, numpy's pairwise recursion)."""
import numpy as np
import pytest
import torch

from assoc_cases import DEMO, PARAMS, make_case, sequence
from conftest import golden, load_pkg, state_dict_np

pytestmark = pytest.mark.gpu

_NETS = {}
SKELETON = [[15, 13], [13, 11], [16, 14], [14, 12], [11, 12], [5, 11], [6, 12], [5, 6], [5, 7], [6, 8], [7, 9], [8, 10], [1, 2], [0, 1],
            [0, 2], [1, 3], [2, 4], [3, 5], [4, 6]]


def engine():
    if "net" not in _NETS:
        _NETS["net"] = load_pkg().NativeHRNet(32, 17, (64, 64), "fp32", max_batch=8, device=0).load_state_dict(state_dict_np(32, 0))
    return _NETS["net"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def both(case, params, **kw):
    """(device results as numpy, host results) of one case"""
    pp = load_pkg("postproc")
    args = [case[k] for k in ("boxes", "pts", "prev_boxes", "prev_pts", "prev_ids")]
    want = pp.associate_people(args[0].copy(), args[1].copy(), *args[2:], case["next_id"], *params, **kw)
    got = engine().associate_people(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args], case["next_id"], *params, **kw)
    assert all(t.is_cuda for t in got)
    return [t.cpu().numpy() for t in got], want


def assert_same(got, want, what):
    for name, g, w in zip(("boxes", "pts", "ids", "match", "next_id", "status"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(bits(g), bits(w)), (what, name)


def test_reference_fixtures_on_the_device():
    G = golden("tracking_cases")
    for k in (int(v) for v in G["track_cases"]):
        case = {n: G["track%d_%s" % (k, n)] for n in ("boxes", "pts", "prev_boxes", "prev_pts", "prev_ids")}
        case["next_id"] = int(G["track%d_next_id" % k])
        got, want = both(case, tuple(float(v) for v in G["track%d_params" % k]))
        assert_same(got, want, k)
        assert np.array_equal(got[2], G["track%d_out_ids" % k]) and np.array_equal(got[0], G["track%d_out_boxes" % k])
        assert np.array_equal(bits(got[1]), bits(G["track%d_out_pts" % k]))


@pytest.mark.parametrize("J", [17, 16, 133])
def test_small_shapes_equal_the_host_form(J):
    for n, m in ((0, 3), (3, 0), (1, 1), (2, 5), (5, 2)):
        for params in (PARAMS[1], DEMO):                       # smoothing_alpha 0 and 0.1
            got, want = both(make_case(50 * n + 7 * m + J, n, m, J), params)
            assert_same(got, want, (n, m, J, params))
            if n and m:
                assert (want[3] >= 0).any(), (n, m, J)         # somebody is matched: ids carried over, smoothing applied


@pytest.mark.parametrize("n,m,J,params", [(64, 64, 17, DEMO), (65, 65, 17, PARAMS[1]), (70, 130, 17, DEMO), (130, 70, 16, DEMO),
                                          (33, 70, 133, DEMO), (256, 256, 17, DEMO)])
def test_columns_past_one_wave_pass_equal_the_host_form(n, m, J, params):
    got, want = both(make_case(n + m + J, n, m, J), params)
    assert_same(got, want, (n, m, J))
    assert (want[3] >= 0).sum() >= min(n, m) // 2


def test_ties_and_zero_boxes_equal_the_host_form():
    # every person three times on both sides: many costs are exactly equal and only the tie rule (lowest column) decides
    base = make_case(77, 4, 4, 17, jitter=0.0)
    dup = {k: np.ascontiguousarray(np.concatenate([base[k]] * 3)) for k in ("boxes", "pts", "prev_boxes", "prev_pts")}
    dup["prev_ids"], dup["next_id"] = np.arange(100, 112, dtype=np.int32), 112
    for params in (PARAMS[1], DEMO):
        got, want = both(dup, params)
        assert_same(got, want, "duplicates")
        assert (want[3] >= 0).all() and len(set(want[2].tolist())) == 12
    # a pair of zero boxes: status 1 on both sides, nobody matched through it
    case = make_case(11, 3, 3, 17, jitter=1.0)
    case["boxes"][1] = 0
    case["prev_boxes"][2] = 0
    case["pts"][1] = case["prev_pts"][2]
    got, want = both(case, (0.5, 0.1, 0.1))
    assert_same(got, want, "zero boxes")
    assert got[5].tolist() == [1] and got[3][1] != 2
    # a previous id of -1 is numbered anew (the reference's quirk), on both sides alike
    quirk = make_case(12, 3, 3, 17, jitter=1.0)
    quirk["prev_ids"][:] = (-1, 8, 3)
    got, want = both(quirk, DEMO)
    assert_same(got, want, "previous id -1")


def test_four_segments_in_one_launch_equal_four_calls():
    shapes = [(3, 5), (0, 2), (70, 66), (6, 0)]
    parts = [make_case(31 + k, n, m, 17) for k, (n, m) in enumerate(shapes)]
    cat = {k: np.concatenate([p[k] for p in parts]) for k in ("boxes", "pts", "prev_boxes", "prev_pts", "prev_ids")}
    cat["next_id"] = [p["next_id"] for p in parts]
    counts, prev_counts = [s[0] for s in shapes], [s[1] for s in shapes]
    got, want = both(cat, DEMO, counts=counts, prev_counts=prev_counts)
    assert_same(got, want, "segments")
    single = [both(p, DEMO)[0] for p in parts]
    for k in range(6):
        assert np.array_equal(bits(got[k]), bits(np.concatenate([s[k] for s in single]))), k


def test_refusals_name_their_cause():
    net = engine()
    big = make_case(3, 257, 2, 17)
    with pytest.raises(RuntimeError, match="HRN_MAX_TRACKED"):
        net.associate_people(big["boxes"], big["pts"], big["prev_boxes"], big["prev_pts"], big["prev_ids"], 0)
    ok = make_case(3, 2, 2, 17)
    with pytest.raises(RuntimeError, match="smoothing_alpha"):
        net.associate_people(ok["boxes"], ok["pts"], ok["prev_boxes"], ok["prev_pts"], ok["prev_ids"], 0, smoothing_alpha=2.0)


def test_tracker_on_the_device_equals_the_host_run():
    pkg = load_pkg()
    for counts_of in (None, lambda a, b: [a, b]):
        frames, other = sequence(), sequence(seed=9)[::-1]
        host, dev = pkg.PersonTracker(), pkg.PersonTracker(engine())
        for (boxes, pts), (boxes2, pts2) in zip(frames, other):
            kw = {}
            if counts_of is not None:
                kw = {"counts": counts_of(len(boxes), len(boxes2))}
                boxes, pts = np.concatenate([boxes, boxes2]), np.concatenate([pts, pts2])
            want = host.update(boxes, pts, **kw)
            given = torch.from_numpy(boxes).cuda(), torch.from_numpy(pts).cuda()
            got = dev.update(*given, **kw)
            assert all(t.is_cuda for t in got) and dev.next_id.is_cuda
            assert torch.equal(given[0].cpu(), torch.from_numpy(boxes)) and torch.equal(given[1].cpu(), torch.from_numpy(pts))
            for g, w in zip(got, want):
                assert np.array_equal(bits(g.cpu().numpy()), bits(w))
            assert dev.next_id.cpu().tolist() == host.next_id.tolist()


@pytest.mark.parametrize("kind", ["bgr", "nv12"])
def test_overlay_with_device_ids_equals_the_host_ids(kind):
    pkg = load_pkg()
    net = engine()
    rng = np.random.default_rng(4)
    pts = np.stack([rng.uniform(5, 115, (7, 17)), rng.uniform(5, 155, (7, 17)), rng.uniform(0.3, 1.0, (7, 17))], 2).astype(np.float32)
    ids = np.asarray([-9, 0, 3, 8, 2147483647, -2147483648, 21], np.int32)      # negative, and larger than the 8-colour palette
    index = np.asarray([0, 1, 1, 0, 1, 0, 1], np.int32)

    def canvases():
        if kind == "bgr":
            return [torch.from_numpy(np.random.default_rng(k).integers(0, 256, (120, 160, 3), dtype=np.uint8)).cuda() for k in (1, 2)]
        return [pkg.YuvFrame(np.random.default_rng(k).integers(0, 256, 120 * 160 * 3 // 2, dtype=np.uint8), 120, 160, "nv12").to(net.torch_device)
                for k in (1, 2)]

    def data(frame):
        return (frame if kind == "bgr" else frame.data).cpu().numpy()

    plain = canvases()
    a = net.draw_poses(canvases(), pts, SKELETON, frame_index=index, person_ids=ids)
    b = net.draw_poses(canvases(), pts, SKELETON, frame_index=index, person_ids=torch.from_numpy(ids).cuda())
    for fa, fb, f0 in zip(a, b, plain):
        assert np.array_equal(data(fa), data(fb))
        assert not np.array_equal(data(fa), data(f0))           # something was drawn
    c = net.draw_poses(canvases(), pts, SKELETON, frame_index=index, person_ids=torch.from_numpy(ids + 1).cuda())
    assert not np.array_equal(data(c[0]), data(a[0]))           # the ids do decide the bone colours


def test_device_loop_equals_the_loop_through_the_host():
    """predict_frame on frame 0, then track_frame -> PersonTracker.update -> draw_poses over three frames, all on the device,
    against the same loop with the joints downloaded and postproc.associate_people's ids uploaded for the overlay"""
    pkg = load_pkg()
    net = engine()
    rng = np.random.default_rng(8)
    frames = [rng.integers(0, 256, (120, 160, 3), dtype=np.uint8) for _ in range(4)]
    dets = np.asarray([[10.2, 8.7, 90.4, 100.1], [60.5, 20.5, 150.0, 70.0], [30.0, 40.0, 120.0, 118.0]], np.float32)
    box_args = dict(threshold=-1.0, min_joints=1)               # synthetic weights: every joint counts, nobody is lost

    boxes0, pts0 = net.predict_frame(torch.from_numpy(frames[0]).cuda(), dets)
    dev, host = pkg.PersonTracker(net), pkg.PersonTracker()
    d_boxes, d_pts, d_ids = dev.update(torch.from_numpy(boxes0).cuda(), pts0)
    h_boxes, h_pts, h_ids = host.update(boxes0, pts0.cpu().numpy())
    for k in (1, 2, 3):
        frame = torch.from_numpy(frames[k]).cuda()
        t_boxes, t_pts, t_status = net.track_frame(frame, d_pts, **box_args)
        d_boxes, d_pts, d_ids = dev.update(t_boxes, t_pts)
        canvas = net.draw_poses(frame.clone(), d_pts, SKELETON, person_ids=d_ids)
        assert all(t.is_cuda for t in (t_boxes, t_pts, t_status, d_boxes, d_pts, d_ids, canvas, dev.next_id))
        # the same step through the host
        u_boxes, u_pts, _ = net.track_frame(frame, torch.from_numpy(h_pts).cuda(), **box_args)
        h_boxes, h_pts, h_ids = host.update(u_boxes.cpu().numpy(), u_pts.cpu().numpy())
        want = net.draw_poses(frame.clone(), h_pts, SKELETON, person_ids=h_ids)
        assert np.array_equal(d_ids.cpu().numpy(), h_ids) and np.array_equal(d_boxes.cpu().numpy(), h_boxes), k
        assert np.array_equal(bits(d_pts.cpu().numpy()), bits(h_pts)), k
        assert torch.equal(canvas, want), k
        assert dev.next_id.cpu().tolist() == host.next_id.tolist()
