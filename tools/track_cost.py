"""The tracking link, measured: writes DIR/track_mode.txt (and prints it).  No number here is a gate: what a tracked frame costs
beside a detected one is a result to record.  The end-to-end gain of tracking -- the detector passes that are not run -- depends
on the user's detector and is neither measured nor claimed.

Setup: HRNet-W48 384x288 bf16, a 1080p frame resident in HBM, 8 people.
  (a) track_frame (boxes from the previous joints, crop records and crops on the device, pass) against predict_frame with THE SAME
      boxes as host detections (host geometry, pinned upload of the records, crops, pass): back-to-back calls between HIP events,
      interleaved (round r runs the candidates in a rotated order), medians and spread.  In the same rotation: the pre-paths
      alone (preprocess_frames_dev + boxes_from_poses against preprocess_frame).
  (b) the two new launches alone under `rocprofv3 --kernel-trace --stats`, in a run of its own (a child process of this tool).
  (c) --ab-root DIR: predict_frame (HRNet-W48 384x288) in THIS tree against the checkout at DIR (the parent commit, built):
      costlib.ab, the protocol of tools/README.md.  Without --ab-root: NOT MEASURED.

usage: python tools/track_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR] [--no-trace]
       python tools/track_cost.py --launches-only                 (the child of (b): runs under rocprofv3)"""
import importlib
import os
import shutil
import statistics
import sys
import tempfile

import costlib

ap = costlib.parser(__doc__, "track_mode.txt", rounds=9, reps=20, ab="predict_frame", out_required=False)
ap.add_argument("--no-trace", action="store_true", help="skip (b)")
ap.add_argument("--launches-only", action="store_true", help="run the tracked pre-path 200 times (the child of (b))")
args = ap.parse_args()
if not args.launches_only and not args.out:
    ap.error("--out is needed")
sys.path.insert(0, costlib.ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
RES = (384, 288)
PEOPLE = 8
pkg = importlib.import_module("simple-hrnet_amd")
frame = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
prev = costlib.people_of(PEOPLE, seed=1)[0]
prev_dev = torch.from_numpy(prev).cuda()
if args.launches_only:
    net = pkg.NativeHRNet(48, 17, RES, "bf16", max_batch=PEOPLE, device=0)   # the pre-path needs no weights
    for _ in range(200):
        net.preprocess_frames_dev(frame, net.boxes_from_poses(prev_dev, (hf, wf)))
    torch.cuda.synchronize()
    net.close()
    sys.exit(0)

report = costlib.Report(args.out, "track_mode.txt")
say, fmt = report.say, report.fmt

say("the tracking link -- tools/track_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, medians" % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
net = pkg.NativeHRNet(48, 17, RES, "bf16", max_batch=PEOPLE, device=0).load_state_dict(pkg.synth_state_dict(48, 17, 0))
host_dets = pkg.postproc.pose_boxes(prev, (hf, wf))           # the same boxes, as a detector would hand them over
status = net.track_frame(frame, prev_dev)[2]
assert not status.any(), "the people of this measurement are all trackable"
cands = {"track_frame": lambda: net.track_frame(frame, prev_dev),
         "predict_frame": lambda: net.predict_frame(frame, host_dets),
         "pre-path, device detections": lambda: net.preprocess_frames_dev(frame, net.boxes_from_poses(prev_dev, (hf, wf))),
         "pre-path, host detections": lambda: net.preprocess_frame(frame, host_dets)}
s = costlib.timed(cands, args.rounds, args.reps, warmup=5)
say()
say("(a) one %dx%d BGR frame resident in HBM, %d people, HRNet-W48 %dx%d bf16; back-to-back calls, no synchronisation inside a sample"
    % (wf, hf, PEOPLE, RES[0], RES[1]))
for k in cands:
    say("    %-30s %s" % (k, fmt(s[k])))
med = {k: statistics.median(v) for k, v in s.items()}
spread = max(max(s[k]) - min(s[k]) for k in ("track_frame", "predict_frame"))
diff = med["track_frame"] - med["predict_frame"]
say("    track_frame - predict_frame = %+.4f ms; spread of the samples (the wider side) %.4f ms -> %s"
    % (diff, spread, "inside the spread" if abs(diff) <= spread else ("track_frame is SLOWER" if diff > 0 else "track_frame is faster") + " beyond the spread"))
pre_diff = med["pre-path, device detections"] - med["pre-path, host detections"]
say("    pre-paths alone: device - host detections = %+.4f ms (the device path adds two small launches and sizes the horizontal" % pre_diff)
say("    grid for the tallest crop its frame allows -- spare blocks exit at once; it drops the host geometry and the record upload)")
if abs(diff) > spread and diff > 0:
    say("    where the time goes: the pre-paths differ by %+.4f ms of the %+.4f ms; see (b) for the two launches themselves" % (pre_diff, diff))
net.close()

say()
if args.no_trace or not shutil.which("rocprofv3"):
    say("(b) the two new launches under rocprofv3 --kernel-trace --stats: NOT MEASURED (%s)" % ("--no-trace" if args.no_trace else "no rocprofv3"))
else:
    tmp = tempfile.mkdtemp(prefix="track_trace_")
    costlib.traced([sys.executable, os.path.abspath(__file__), "--launches-only"], tmp, timeout=280)
    found = costlib.kernel_stats(tmp, ("pose_boxes_kernel", "crop_records_kernel", "prepath_horizontal_kernel", "prepath_vertical_kernel"))
    shutil.rmtree(tmp, ignore_errors=True)
    say("(b) rocprofv3 --kernel-trace --stats over 200 tracked pre-paths (boxes_from_poses + preprocess_frames_dev), a run of its own")
    say("    %-34s %8s %12s %12s %12s" % ("kernel", "calls", "mean us", "min us", "max us"))
    for name, (calls, mean, low, high) in found.items():
        say("    %-34s %8d %12.2f %12.2f %12.2f" % (name, calls, mean / 1e3, low / 1e3, high / 1e3))

say()
sys.exit(costlib.ab(report, "(c)", ["predict_w48"], args.ab_root, args.ab_pairs, args.rounds, args.reps) is None)
