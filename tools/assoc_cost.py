"""Person ids on the GPU, measured: writes DIR/assoc_ids.txt (and prints it).  No number here is a gate: what the association
costs beside the host round trip it replaces, and what its single-wave assignment costs at the cap, are results to record.

  (a) NativeHRNet.associate_people (one launch, demo parameters, J = 17) at 8 x 8, 64 x 64 and 256 x 256 people against the host
      path it replaces: download pts and boxes, postproc.find_person_id_associations, upload ids and the smoothed pts and boxes.
      HIP events around back-to-back calls, host side included, interleaved (round r runs the candidates in a rotated order),
      medians.  In the same rotation, per size, the same call on an engine created under HRN_ASSOC_NO_ASSIGN=1 (debug switch: the
      assignment phase is skipped): the difference is the single wave's share.
  (b) draw_poses with ids from the host against ids on the device (8 people, 1080p BGR, resident).
  (c) --ab-root DIR: draw_poses with host ids (8 people, 1080p) and predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree
      against the checkout at DIR (the parent commit, built): costlib.ab, the protocol of tools/README.md.  Without --ab-root:
      NOT MEASURED.

usage: python tools/assoc_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]"""
import importlib
import os
import statistics
import sys

import costlib
from costlib import people_of, timed

args = costlib.parser(__doc__, "assoc_ids.txt", rounds=9, reps=20, ab="draw_poses and predict_frame").parse_args()
sys.path.insert(0, costlib.ROOT)
os.environ["HRN_DEBUG_ENV"] = "1"   # (the library reads switches only in a process that opts in; none is set but for (a)'s second engine)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
COCO = costlib.coco_skeleton()
pkg = importlib.import_module("simple-hrnet_amd")
report = costlib.Report(args.out, "assoc_ids.txt")
say, fmt = report.say, report.fmt

say("person ids -- tools/assoc_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, host side included, medians"
    % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # association and drawing need no weights
os.environ["HRN_ASSOC_NO_ASSIGN"] = "1"
bare = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # the same engine without the assignment phase
del os.environ["HRN_ASSOC_NO_ASSIGN"]
assert "HRN_ASSOC_NO_ASSIGN" in bare.switches() and "HRN_ASSOC_NO_ASSIGN" not in net.switches()
alpha, thr, smooth = 0.2, 0.4, 0.1   # scripts/live-demo.py:122

say()
say("(a) associate_people, J = 17, demo parameters (pose_alpha %.1f, threshold %.1f, smoothing %.1f), everybody a jittered copy of a"
    % (alpha, thr, smooth))
say("    previous person in shuffled order; host path = download pts + boxes, find_person_id_associations, upload ids + pts + boxes")
for count in (8, 64, 256):
    prev_pts, prev_boxes = people_of(count, seed=count)
    order = np.random.default_rng(count).permutation(count)
    cur_pts, cur_boxes = people_of(count, seed=count + 1, jitter=3.0, base=prev_pts[order])
    prev_ids = np.arange(count, dtype=np.int32)
    dev = [torch.from_numpy(v).cuda() for v in (cur_boxes, cur_pts, prev_boxes, prev_pts, prev_ids)]
    work_boxes, work_pts = dev[0].clone(), dev[1].clone()
    next_id = torch.tensor([count], dtype=torch.int32, device="cuda")
    pin_boxes, pin_pts = torch.empty_like(dev[0], device="cpu").pin_memory(), torch.empty_like(dev[1], device="cpu").pin_memory()

    def device_call(engine):
        # (smoothing works in place: every call starts from the frame's own boxes and joints, as a video loop's would)
        work_boxes.copy_(dev[0]), work_pts.copy_(dev[1])
        return engine.associate_people(work_boxes, work_pts, dev[2], dev[3], dev[4], next_id, alpha, thr, smooth)

    def refresh_only():
        work_boxes.copy_(dev[0]), work_pts.copy_(dev[1])

    def host_call():
        pin_boxes.copy_(dev[0], non_blocking=True), pin_pts.copy_(dev[1], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        b, p, ids = pkg.postproc.find_person_id_associations(pin_boxes.numpy(), pin_pts.numpy(), prev_boxes, prev_pts, prev_ids,
                                                             next_person_id=count, pose_alpha=alpha, similarity_threshold=thr,
                                                             smoothing_alpha=smooth)
        work_boxes.copy_(torch.from_numpy(b), non_blocking=True), work_pts.copy_(torch.from_numpy(p), non_blocking=True)
        return torch.from_numpy(ids).cuda(non_blocking=True)

    got = device_call(net)
    matched = int((got[3] >= 0).sum())
    reps = args.reps if count < 256 else max(2, args.reps // 4)
    s = timed({"device": lambda: device_call(net), "bare": lambda: device_call(bare), "refresh": refresh_only, "host": host_call},
              args.rounds, reps)
    med = {k: statistics.median(v) for k, v in s.items()}
    say("    %3d x %3d people (%d matched)" % (count, count, matched))
    say("        device call              %s" % fmt(s["device"]))
    say("        without the assignment   %s   (nobody is matched then: phase 3 has nothing to smooth either)" % fmt(s["bare"]))
    say("        the two refresh copies   %s   (included in both of the above and not part of a video loop)" % fmt(s["refresh"]))
    say("        host path                %s" % fmt(s["host"]))
    say("        device / host = %.3f; single-wave assignment = %.4f ms = %.0f %% of the device call less its refresh copies"
        % (med["device"] / med["host"], med["device"] - med["bare"],
           100.0 * (med["device"] - med["bare"]) / max(med["device"] - med["refresh"], 1e-9)))
bare.close()

say()
bgr = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
pts8 = torch.from_numpy(people_of(8, seed=8)[0]).cuda()
ids_host = np.arange(3, 11, dtype=np.int32)
ids_dev = torch.from_numpy(ids_host).cuda()
s = timed({"host": lambda: net.draw_poses(bgr, pts8, COCO, person_ids=ids_host), "device": lambda: net.draw_poses(bgr, pts8, COCO, person_ids=ids_dev)},
          args.rounds, args.reps)
say("(b) draw_poses, 8 people on a %dx%d BGR frame resident in HBM" % (wf, hf))
say("    ids from the host    %s   (two launches)" % fmt(s["host"]))
say("    ids on the device    %s   (three launches, no host read)" % fmt(s["device"]))
net.close()

say()
runs = costlib.ab(report, "(c)", ["draw8_ids", "predict"], args.ab_root, args.ab_pairs, args.rounds, args.reps)
say()
say("Not claimed: how well these ids follow people on a trained network -- no trained weights and no video exist where this was measured.")
sys.exit(runs is None)
