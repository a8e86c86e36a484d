"""One handle under callers that alternate streams, for every family of calls that keeps a device array on the handle (crop
pre-path, tracking table, warp, scoring, overlays, person ids, the detector link, frame rotation, the temporal filter, pose NMS,
the track table): the handle's one call frame (csrc/ctx_scratch.inc) must serialise them, and an array must be able to grow while
another stream was its last user."""
import numpy as np
import pytest
import torch

from conftest import load_pkg

H, W, FH, FW, J = 128, 96, 96, 80, 17
SH, SW, LB = 24, 20, 32   # the small frames of the detector link and the rotation, and the detector's input side
SKELETON = [(0, 1), (1, 2), (2, 3), (5, 6), (5, 7), (7, 9), (11, 13), (13, 15)]


def _boxes(rng, n):
    """n detection rows well inside a FH x FW frame"""
    x1, y1 = rng.uniform(0, 30, n), rng.uniform(0, 30, n)
    return np.stack([x1, y1, x1 + rng.uniform(20, 45, n), y1 + rng.uniform(25, 60, n)], 1).astype(np.float32)


def _poses(rng, n):
    """(n, J, 3) (y, x, confidence) inside the frame, most joints above the 0.5 threshold"""
    return np.concatenate([rng.uniform(2, FH - 2, (n, J, 1)), rng.uniform(2, FW - 2, (n, J, 1)), rng.uniform(0.3, 1.0, (n, J, 1))],
                          2).astype(np.float32)


def _arguments(pkg, seed, people=3, table=2, tracked=3, drawn=3, warped=3, scored=3, matched=(2, 1), small=3, turned=3, filtered=(2, 1),
               nms=(2, 1), streams=(2, 1), capacity=8):
    """one argument set: `people` in every call unless a count says otherwise (the large set: past the first call's capacity)"""
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda", 0)
    a = {"frames": [torch.from_numpy(rng.integers(0, 256, (FH, FW, 3), dtype=np.uint8)).to(dev) for _ in range(2)],
         "yuv": [pkg.YuvFrame(torch.from_numpy(rng.integers(0, 256, FH * FW * 3 // 2, dtype=np.uint8)).to(dev), FH, FW, "nv12")
                 for _ in range(2)]}
    a["stack"] = torch.stack(a["frames"])
    a["dets"] = [_boxes(rng, people - people // 2), _boxes(rng, people // 2)]                    # per frame, host
    a["dets_dev"] = torch.from_numpy(_boxes(rng, 3)).to(dev)
    a["index"] = np.asarray([0, 1, 0], np.int32)
    a["table"] = a["frames"] + [None] * (table - 2)                                              # frames nobody is cut from
    a["pts"] = torch.from_numpy(_poses(rng, tracked)).to(dev)
    a["sizes"] = np.stack([rng.integers(60, FH, tracked), rng.integers(50, FW, tracked)], 1).astype(np.int32)
    a["drawn"] = torch.from_numpy(_poses(rng, drawn)).to(dev)
    a["drawn_on"] = rng.integers(0, 2, drawn).astype(np.int32)
    ang, sc = rng.uniform(-0.5, 0.5, warped), rng.uniform(0.8, 1.6, warped)
    a["matrices"] = np.stack([np.stack([sc * np.cos(ang), -sc * np.sin(ang), rng.uniform(-10, 10, warped)], 1),
                              np.stack([sc * np.sin(ang), sc * np.cos(ang), rng.uniform(-10, 10, warped)], 1)], 1)
    a["warp_index"] = rng.integers(0, 2, warped).astype(np.int32)
    a["joints"] = np.concatenate([rng.uniform(-8, W + 8, (scored, J, 1)), rng.uniform(-8, H + 8, (scored, J, 1))], 2)
    a["vis"] = (rng.uniform(0, 1, (scored, J)) > 0.2).astype(np.float32)
    a["heatmaps"] = torch.from_numpy(rng.uniform(0, 1, (scored, J, H // 4, W // 4)).astype(np.float32)).to(dev)
    n, m = sum(matched), sum(matched[::-1])
    a["assoc"] = dict(boxes=_boxes(rng, n).astype(np.int32), pts=_poses(rng, n),
                      prev_boxes=_boxes(rng, m).astype(np.int32), prev_pts=_poses(rng, m),
                      prev_ids=np.arange(m, dtype=np.int32), next_id=np.asarray([100, 200], np.int32), counts=list(matched),
                      prev_counts=list(matched[::-1]), smoothing_alpha=0.25)
    # the families whose table travels only with several frames / people / problems: `small` frames of SH x SW with a rotation code
    # and two detector rows each, `turned` people with a frame size and a code each, and people by problem
    a["small"] = list(torch.from_numpy(rng.integers(0, 256, (small, SH, SW, 3), dtype=np.uint8)).to(dev).unbind(0))
    a["codes"] = rng.integers(0, 3, small).astype(np.int32)
    x1, y1 = rng.uniform(0, LB / 2, 2 * small), rng.uniform(0, LB / 2, 2 * small)
    a["rows"] = np.stack([x1, y1, x1 + rng.uniform(2, LB / 2, 2 * small), y1 + rng.uniform(2, LB / 2, 2 * small),
                          rng.uniform(0, 1, 2 * small), rng.integers(0, 3, 2 * small)], 1).astype(np.float32)
    a["turned"] = dict(pts=_poses(rng, turned), boxes=_boxes(rng, turned).astype(np.int32),
                       frame_hw=np.stack([rng.integers(FH, 2 * FH, turned), rng.integers(FW, 2 * FW, turned)], 1).astype(np.int32),
                       rotation_code=rng.integers(0, 3, turned).astype(np.int32))
    a["filtered"] = dict(pts=_poses(rng, sum(filtered)), counts=list(filtered))
    a["nms"] = dict(pts=_poses(rng, sum(nms)), boxes=_boxes(rng, sum(nms)).astype(np.int32), counts=list(nms), thresh=0.5)
    a["tracked"] = dict(boxes=_boxes(rng, sum(streams)).astype(np.int32), pts=_poses(rng, sum(streams)), counts=list(streams))
    a["capacity"] = capacity
    return a


def _calls(net, a):
    """every call of the families under test on the current stream; the outputs, stream-ordered (nothing is synchronised)"""
    out = {}
    images, _, boxes_dev, _ = net.preprocess_frames(a["frames"], a["dets"])
    out["frames"], out["frames_boxes"] = images, boxes_dev
    images, _, boxes_dev, _ = net.preprocess_frames(a["yuv"], a["dets"])
    out["yuv"], out["yuv_boxes"] = images, boxes_dev
    out["dev"], out["dev_boxes"], out["dev_status"] = net.preprocess_frames_dev(a["table"], a["dets_dev"], a["index"])
    out["pose_boxes"] = net.boxes_from_poses(a["pts"], a["sizes"])
    out["warp"] = net.warp_crops(a["stack"], matrices=a["matrices"], frame_index=a["warp_index"])
    targets, weight = net.generate_targets(a["joints"], a["vis"])
    out["targets"] = targets
    for name, score in (("analytic", net.score_heatmaps(a["heatmaps"], joints=a["joints"], visibility=a["vis"], topk=8)),
                        ("maps", net.score_heatmaps(a["heatmaps"], targets=targets, target_weight=weight, topk=8))):
        for key, value in score.items():
            out["score_%s_%s" % (name, key)] = value
    for k, canvas in enumerate(net.draw_poses([f.clone() for f in a["frames"]], a["drawn"], SKELETON, frame_index=a["drawn_on"])):
        out["draw_%d" % k] = canvas
    for k, value in enumerate(net.associate_people(**a["assoc"])):
        out["assoc_%d" % k] = value
    out["letterbox"], geometry = net.detector_input(a["small"], LB)
    for k, value in enumerate(net.detections_to_frame(a["rows"], geometry, counts=[2] * len(a["small"]), conf_thres=0.3)):
        out["dets_%d" % k] = value
    out["rotated"] = torch.cat([f.reshape(-1) for f in net.rotate_frames(a["small"], a["codes"])])
    out["turned_pts"], out["turned_boxes"] = net.rotate_people(**a["turned"])
    pts, pred, (values, age) = net.filter_poses(**a["filtered"])
    out["filter_pts"], out["filter_pred"], out["filter_values"], out["filter_age"] = pts, pred, values, age
    for key, value in net.pose_nms(**a["nms"]).items():
        out["nms_%s" % key] = value
    table = net.new_track_table(len(a["tracked"]["counts"]), a["capacity"])     # every round starts from the same table
    for k, value in enumerate(net.track_people(table=table, **a["tracked"])):
        out["track_%d" % k] = value
    for key, value in table.items():
        out["track_table_%s" % key] = value
    return out


@pytest.mark.gpu
def test_every_call_family_under_alternating_streams():
    """A functional check that the handle's shared guard serialises its calls and that growing an array under alternation is safe:
    12 rounds rotate three streams and three argument sets -- two of 3 people, so that consecutive calls really rewrite each
    table, and one whose sizes exceed the capacity the first call allocated, issued when another stream was the last user -- and
    every output must equal, bit for bit, what the same arguments gave on the default stream of a fresh handle.  It is NOT a
    race detector: at these sizes a missing wait may well go unnoticed, so the review of the guard's code (CallGuard /
    CallScope / CallFrame in csrc/ctx_scratch.inc) carries that weight."""
    pkg = load_pkg()
    sets = [_arguments(pkg, 1), _arguments(pkg, 2),
            # past the floors of the growth rules: 4096 B of tables (130 frames x 80 B; 600 x 8 B of frame sizes; 400 people drawn), 256
            # warp records, 256 x 17 score records, 65536 B of association scratch (two problems of 60 x 60 x 12 B), and more people
            # than the exactly-sized pre-path arrays held; and of the tables that travel only with several problems: 130 BGR frames
            # x 120 B of letterbox records (kernels.h's LetterboxFrame: a pointer, a 64 B YuvSource, 8 ints, 2 doubles), x 32 B of detection
            # records (letterbox_math.h's DetFrame) and x 48 B of rotation planes (RotPlane, one per BGR frame), 350 people x 12 B of frame sizes and codes,
            # 520 people x 8 B of filter segments, 520 problems x 8 B of pose NMS; and 65536 B of track scratch (a 256 B stream table,
            # then two streams of 45 rows x 64 slots x 12 B)
            _arguments(pkg, 3, people=7, table=130, tracked=600, drawn=400, warped=260, scored=257, matched=(60, 60), small=130, turned=350,
                       filtered=(300, 220), nms=(1,) * 520, streams=(45, 45), capacity=64)]
    net = pkg.NativeHRNet(32, J, (H, W), "fp32", max_batch=4, device=0)
    want = [{k: v.cpu().numpy() for k, v in _calls(net, a).items()} for a in sets]
    torch.cuda.synchronize()
    net.close()
    net = pkg.NativeHRNet(32, J, (H, W), "fp32", max_batch=4, device=0)     # nothing allocated yet: the first calls decide the capacities
    streams = [torch.cuda.Stream() for _ in range(3)]
    got = []
    for it, which in enumerate((0, 1, 0, 1, 2, 0, 1, 2, 1, 0, 2, 1)):
        s = streams[it % 3]
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got.append((which, _calls(net, sets[which])))
    torch.cuda.synchronize()
    for which, outputs in got:
        assert outputs.keys() == want[which].keys()
        for key, value in outputs.items():
            np.testing.assert_array_equal(value.cpu().numpy(), want[which][key], err_msg="%s of argument set %d" % (key, which))
    net.close()
