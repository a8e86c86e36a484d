"""The tracking link, measured: writes DIR/track_mode.txt (and prints it).  No number here is a gate: what a tracked frame costs
beside a detected one is a result to record.  The end-to-end gain of tracking -- the detector passes that are not run -- depends
on the user's detector and is neither measured nor claimed.

Setup: HRNet-W48 384x288 bf16, a 1080p frame resident in HBM, 8 people.
  (a) track_frame (boxes from the previous joints, crop records and crops on the device, pass) against predict_frame with THE SAME
      boxes as host detections (host geometry, pinned upload of the records, crops, pass): back-to-back calls between HIP events,
      interleaved (round r runs the candidates in a rotated order), medians and spread.  In the same rotation: the pre-paths
      alone (preprocess_frames_dev + boxes_from_poses against preprocess_frame).
  (b) the two new launches alone under `rocprofv3 --kernel-trace --stats`, in a run of its own (a child process of this tool).
  (c) --ab-root DIR: predict_frame in THIS tree against the checkout at DIR (the parent commit, built), each in fresh child
      processes run alternately on the same box; a difference inside the spread of the children's medians is "unchanged" --
      expected, since its code path is untouched.  Without --ab-root: NOT MEASURED.

usage: python tools/track_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR] [--no-trace]
       python tools/track_cost.py --predict-only [--root DIR]     (the child of (c): one JSON line)
       python tools/track_cost.py --launches-only                 (the child of (b): runs under rocprofv3)"""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--out", help="directory track_mode.txt is written to")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=20, help="calls per timed sample")
ap.add_argument("--ab-root", help="checkout of the parent commit, built: predict_frame there against here")
ap.add_argument("--ab-pairs", type=int, default=3, help="child processes per side of the A/B")
ap.add_argument("--no-trace", action="store_true", help="skip (b)")
ap.add_argument("--predict-only", action="store_true", help="time predict_frame of (c) alone and print one JSON line")
ap.add_argument("--launches-only", action="store_true", help="run the tracked pre-path 200 times (the child of (b))")
ap.add_argument("--root", default=ROOT, help="with --predict-only: the checkout whose package is timed")
args = ap.parse_args()
child = args.predict_only or args.launches_only
if not child and not args.out:
    ap.error("--out is needed")
sys.path.insert(0, os.path.abspath(args.root) if args.predict_only else ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
RES = (384, 288)
PEOPLE = 8


def timed(cands, rounds, reps):
    """HIP-event ms per call of every candidate: `rounds` samples of `reps` calls each, interleaved in a rotated order"""
    for fn in cands.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    names = list(cands)
    samples = {k: [] for k in names}
    for r in range(rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                cands[k]()
            b.record()
            b.synchronize()
            samples[k].append(a.elapsed_time(b) / reps)
    return samples


def people_of(count, seed):
    """`count` people of plausible size spread over the frame: (count, 17, 3) (y, x, confidence), all joints confident"""
    rng = np.random.default_rng(seed)
    pts = np.empty((count, 17, 3), np.float32)
    for i in range(count):
        bh = rng.uniform(300, 700)
        bw = bh * rng.uniform(0.3, 0.6)
        x1, y1 = rng.uniform(0, wf - bw), rng.uniform(0, hf - bh)
        pts[i, :, 0] = rng.uniform(y1, y1 + bh, 17)
        pts[i, :, 1] = rng.uniform(x1, x1 + bw, 17)
    pts[..., 2] = 0.9
    return pts


pkg = importlib.import_module("simple-hrnet_amd")
frame = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
prev = people_of(PEOPLE, 1)

if args.predict_only:   # (the parent commit has no pose_boxes: the boxes are made here, as tools/draw_cost.py makes them)
    net = pkg.NativeHRNet(48, 17, RES, "bf16", max_batch=PEOPLE, device=0).load_state_dict(pkg.synth_state_dict(48, 17, 0))
    dets = np.stack([prev[..., 1].min(1), prev[..., 0].min(1), prev[..., 1].max(1), prev[..., 0].max(1)], 1).astype(np.float32)
    s = timed({"predict": lambda: net.predict_frame(frame, dets)}, args.rounds, args.reps)["predict"]
    net.close()
    print(json.dumps({"median_ms": statistics.median(s), "min_ms": min(s), "max_ms": max(s)}))
    sys.exit(0)

prev_dev = torch.from_numpy(prev).cuda()
if args.launches_only:
    net = pkg.NativeHRNet(48, 17, RES, "bf16", max_batch=PEOPLE, device=0)   # the pre-path needs no weights
    for _ in range(200):
        net.preprocess_frames_dev(frame, net.boxes_from_poses(prev_dev, (hf, wf)))
    torch.cuda.synchronize()
    net.close()
    sys.exit(0)

os.makedirs(args.out, exist_ok=True)
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def fmt(s):
    return "%8.4f ms  (min %.4f .. max %.4f)" % (statistics.median(s), min(s), max(s))


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
s = timed(cands, args.rounds, args.reps)
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
rocprof = shutil.which("rocprofv3")
if args.no_trace or not rocprof:
    say("(b) the two new launches under rocprofv3 --kernel-trace --stats: NOT MEASURED (%s)" % ("--no-trace" if args.no_trace else "no rocprofv3"))
else:
    tmp = tempfile.mkdtemp(prefix="track_trace_")
    cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "track", "--", sys.executable,
           os.path.abspath(__file__), "--launches-only"]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
    found = [p for p in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)]
    if run.returncode != 0 or not found:
        say("(b) the two new launches under rocprofv3 --kernel-trace --stats: NOT MEASURED (exit code %d, %d stats files)"
            % (run.returncode, len(found)))
    else:
        say("(b) rocprofv3 --kernel-trace --stats over 200 tracked pre-paths (boxes_from_poses + preprocess_frames_dev), a run of its own")
        say("    %-34s %8s %12s %12s %12s" % ("kernel", "calls", "mean us", "min us", "max us"))
        for row in csv.DictReader(open(found[0])):
            name = row.get("Name", "")
            if any(k in name for k in ("pose_boxes_kernel", "crop_records_kernel", "prepath_horizontal_kernel", "prepath_vertical_kernel")):
                short = name.split("(")[0].split("::")[-1]
                say("    %-34s %8s %12.2f %12.2f %12.2f" % (short, row.get("Calls", "?"), float(row.get("AverageNs", "nan")) / 1e3,
                                                            float(row.get("MinNs", "nan")) / 1e3, float(row.get("MaxNs", "nan")) / 1e3))
    shutil.rmtree(tmp, ignore_errors=True)

say()
if not args.ab_root:
    say("(c) predict_frame, this tree against the parent commit: NOT MEASURED (no --ab-root)")
else:
    sides = {"parent": os.path.abspath(args.ab_root), "this tree": ROOT}
    meds = {k: [] for k in sides}
    for _ in range(args.ab_pairs):
        for k, root in sides.items():    # fresh children, alternately
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--predict-only", "--root", root, "--rounds", str(args.rounds),
                                  "--reps", str(args.reps)], capture_output=True, text=True, timeout=300, check=True).stdout
            meds[k].append(json.loads(out.strip().splitlines()[-1])["median_ms"])
    say("(c) predict_frame (%d people of a %dx%d frame, HRNet-W48 %dx%d bf16): this tree against the parent commit, %d fresh processes"
        % (PEOPLE, wf, hf, RES[0], RES[1], args.ab_pairs))
    say("    per side, alternately, same box")
    for k in sides:
        say("    %-10s medians %s ms -> %.4f ms" % (k, ", ".join("%.4f" % v for v in meds[k]), statistics.median(meds[k])))
    spread = max(max(v) - min(v) for v in meds.values())
    diff = statistics.median(meds["this tree"]) - statistics.median(meds["parent"])
    say("    difference %+.4f ms; spread of the processes' medians (the wider side) %.4f ms -> %s"
        % (diff, spread, "unchanged" if abs(diff) <= spread else ("SLOWER" if diff > 0 else "faster") + " beyond the spread"))
with open(os.path.join(args.out, "track_mode.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
