"""Pose NMS on the GPU, measured: writes DIR/pose_nms.txt (and prints it).  No number here is a gate: what the call costs beside the
host round trip it replaces is a result to record, and the call can lose to the host path (one block, one OKS row per kept
person, serial over the joints: profiles/pose_nms.txt has it losing at 133 joints).

  (a) NativeHRNet.pose_nms(suppress=True) (one launch, hard NMS, thresh 0.9) at 8, 64 and 256 people with J = 17 and at 64 people
      with J = 133, everybody a jittered copy of one of n / 3 bodies, against the host path it replaces: download pts, build the
      reference's entries, postproc.oks_nms, upload a keep mask.  HIP events around back-to-back calls, host side included,
      interleaved (round r runs the candidates in a rotated order), medians.
  (b) NativeHRNet.nms_eval at 5 000 images x 20 people (uploads, one launch, downloads and the grouping included) against the host
      loop of datasets/COCO.py:358-382 over postproc.oks_nms; wall clock, `--eval-rounds` runs each, alternately.
  (c) --ab-root DIR: predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree against the checkout at DIR (the parent commit,
      built): costlib.ab, the protocol of tools/README.md.  Without --ab-root: NOT MEASURED.

usage: python tools/pose_nms_cost.py --out DIR [--rounds R] [--reps K] [--eval-rounds E] [--ab-root DIR]"""
import importlib
import statistics
import sys
import time

import costlib

ap = costlib.parser(__doc__, "pose_nms.txt", rounds=9, reps=20, ab="predict_frame")
ap.add_argument("--eval-rounds", type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, costlib.ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920


def crowd(count, joints, seed, bodies=None, per_image=None):
    """`count` skeletons, each a copy of one of `bodies` (count / 3) bodies jittered by 4 pixels: ((count, J, 3) float32 (y, x,
    confidence), (count, 4) int32 boxes, (count,) float32 detection scores); with `per_image`, every run of that many people
    shares 7 bodies of its own"""
    rng = np.random.default_rng(seed)
    bodies = bodies or (count // per_image * 7 if per_image else max(1, count // 3))
    base = np.empty((bodies, joints, 3), np.float32)
    for i in range(bodies):
        bh = rng.uniform(200, 600)
        bw = bh * rng.uniform(0.3, 0.6)
        x1, y1 = rng.uniform(0, wf - bw), rng.uniform(0, hf - bh)
        base[i, :, 0] = rng.uniform(y1, y1 + bh, joints)
        base[i, :, 1] = rng.uniform(x1, x1 + bw, joints)
    pts = base[np.arange(count) // per_image * 7 + rng.integers(0, 7, count) if per_image else rng.integers(0, bodies, count)]
    pts[..., :2] += rng.normal(0, 4.0, pts[..., :2].shape).astype(np.float32)
    pts[..., 2] = rng.uniform(0.3, 1.0, pts.shape[:2])
    boxes = np.stack([pts[..., 1].min(1), pts[..., 0].min(1), pts[..., 1].max(1), pts[..., 0].max(1)], 1)
    return np.ascontiguousarray(pts), np.round(boxes).astype(np.int32), rng.uniform(0.1, 1.0, count).astype(np.float32)


pkg = importlib.import_module("simple-hrnet_amd")
report = costlib.Report(args.out, "pose_nms.txt", "%9.4f ms  (min %.4f .. max %.4f)")
say, fmt = report.say, report.fmt

say("pose NMS -- tools/pose_nms_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, host side included, medians"
    % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # pose NMS needs no weights
thresh = 0.9

say()
say("(a) pose_nms(suppress=True), hard NMS, thresh %.1f, everybody a copy of one of n / 3 bodies jittered by 4 px;" % thresh)
say("    host path = download pts, the reference's entries, postproc.oks_nms, upload a keep mask")
for count, joints in ((8, 17), (64, 17), (256, 17), (64, 133)):
    pts, boxes, det = crowd(count, joints, count + joints)
    sigmas = None if joints == 17 else np.full(joints, 0.05)
    dev = [torch.from_numpy(v).cuda() for v in (pts, boxes, det)]
    work_pts, work_boxes = dev[0].clone(), dev[1].clone()
    pin_pts = torch.empty_like(dev[0], device="cpu").pin_memory()
    areas = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).astype(np.float64)

    def device_call():
        # (suppress works in place: every call starts from the frame's own joints and boxes, as a video loop's would)
        work_pts.copy_(dev[0]), work_boxes.copy_(dev[1])
        return net.pose_nms(work_pts, work_boxes, dev[2], thresh=thresh, sigmas=sigmas, suppress=True)

    def refresh_only():
        work_pts.copy_(dev[0]), work_boxes.copy_(dev[1])

    def host_call():
        pin_pts.copy_(dev[0], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        p = pin_pts.numpy()
        db = [{"keypoints": np.stack([p[i, :, 1], p[i, :, 0], p[i, :, 2]], 1), "score": det[i], "area": areas[i]} for i in range(count)]
        keep = pkg.postproc.oks_nms(db, thresh, sigmas)
        mask = np.zeros(count, np.bool_)
        mask[keep] = True
        return torch.from_numpy(mask).cuda(non_blocking=True)

    got, mask = device_call(), host_call()
    kept = int(got["num"][0])
    same = sorted(got["keep"][:kept].tolist()) == np.flatnonzero(mask.cpu().numpy()).tolist()
    reps = args.reps if count < 256 else max(2, args.reps // 4)
    s = costlib.timed({"device": device_call, "refresh": refresh_only, "host": host_call}, args.rounds, reps)
    med = {k: statistics.median(v) for k, v in s.items()}
    say("    %3d people, J = %3d (%d kept; the host path keeps %s)" % (count, joints, kept, "the same people" if same else "OTHER people"))
    say("        device call              %s" % fmt(s["device"]))
    say("        the two refresh copies   %s   (included in the device call and not part of a video loop)" % fmt(s["refresh"]))
    say("        host path                %s" % fmt(s["host"]))
    say("        device / host = %.3f" % (med["device"] / med["host"]))

say()
images, per_image = 5000, 20
say("(b) nms_eval, %d images x %d people, J = 17, oks_thre 0.9, in_vis_thre 0.2; wall clock of the whole call (grouping, uploads, one"
    % (images, per_image))
say("    launch, downloads) against the loop of datasets/COCO.py:358-382 over postproc.oks_nms; %d runs each, alternately" % args.eval_rounds)
pts, boxes, det = crowd(images * per_image, 17, 77, per_image=per_image)
preds, maxvals = np.ascontiguousarray(pts[..., 1::-1]).astype(np.float64), pts[..., 2].astype(np.float64)
areas = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).astype(np.float64)
box_scores = det.astype(np.float64)
shuffle = np.random.default_rng(3).permutation(images * per_image)          # the people of an image are not neighbours
preds, maxvals, areas, box_scores = preds[shuffle], maxvals[shuffle], areas[shuffle], box_scores[shuffle]
image_index = np.repeat(np.arange(images), per_image)[shuffle]


def host_eval():
    by_image = {}
    for i, image in enumerate(image_index.tolist()):
        by_image.setdefault(image, []).append({"keypoints": np.concatenate([preds[i], maxvals[i][:, None]], 1), "area": areas[i],
                                               "score": box_scores[i], "index": i})
    kept = {}
    for image, img_kpts in by_image.items():
        for n_p in img_kpts:
            c = n_p["keypoints"][:, 2]
            live = c > 0.2
            kpt_score = 0.0
            for t_s in c[live]:
                kpt_score = kpt_score + t_s
            if live.any():
                kpt_score = kpt_score / int(live.sum())
            n_p["score"] = kpt_score * n_p["score"]
        keep = pkg.postproc.oks_nms(img_kpts, 0.9)
        kept[image] = [img_kpts[k]["index"] for k in keep] if len(keep) else [p["index"] for p in img_kpts]
    return kept


def device_eval():
    out = net.nms_eval(preds, maxvals, areas, box_scores, image_index, oks_thre=0.9, in_vis_thre=0.2)
    torch.cuda.synchronize()
    return out


device_eval()
walls = {"device": [], "host": []}
for _ in range(args.eval_rounds):
    for name, fn in (("device", device_eval), ("host", host_eval)):
        t0 = time.perf_counter()
        res = fn()
        walls[name].append((time.perf_counter() - t0) * 1e3)
        if name == "device":
            dev_kept = res[1]
        else:
            host_kept = res
agree = sum(sorted(dev_kept[i].tolist()) == sorted(host_kept[i]) for i in host_kept)
say("    nms_eval                 %s" % fmt(walls["device"]))
say("    host loop                %s" % fmt(walls["host"]))
say("    device / host = %.4f; images on which both keep the same people: %d of %d"
    % (statistics.median(walls["device"]) / statistics.median(walls["host"]), agree, images))
net.close()

say()
runs = costlib.ab(report, "(c)", ["predict"], args.ab_root, args.ab_pairs, args.rounds, args.reps)
say()
say("Not claimed: how many duplicate tracks a trained network produces -- no trained weights and no video exist where this was measured.")
sys.exit(runs is None)
