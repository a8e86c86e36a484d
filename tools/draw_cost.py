"""Pose overlays on the GPU, measured: writes DIR/draw_overlay.txt (and prints it).  No number here is a gate: what an overlay
costs beside the pass, and beside the two copies any host drawing must pay, is a result to record.

  (a) draw_poses of 8 and of 64 people (COCO skeleton: 19 bones + 17 joints each) on a 1080p frame resident in HBM, BGR and NV12.
      HIP events, interleaved (round r runs the candidates in a rotated order), medians.  In the same rotation:
        - an empty launch pair (a whole draw_poses call on a 32x32 view with nobody live: the call's host side, one table upload
          and two launches whose blocks return at once): the floor of a call this small;
        - the download plus upload of the frame alone (pinned host memory): the least a host drawing pays before it draws.
  (b) a 30-frame 1080p clip, 8 people per frame: one draw_poses call for the clip against 30 calls.
  (c) --ab-root DIR: predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree against the checkout at DIR (the parent commit,
      built), each in fresh child processes run alternately on the same box; a difference inside the spread of the children's
      medians is "unchanged" -- expected, since no existing source changes.  Without --ab-root: NOT MEASURED.

usage: python tools/draw_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]
       python tools/draw_cost.py --predict-only [--root DIR]     (the child of (c): one JSON line)"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--out", help="directory draw_overlay.txt is written to")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=20, help="calls per timed sample")
ap.add_argument("--ab-root", help="checkout of the parent commit, built: predict_frame there against here")
ap.add_argument("--ab-pairs", type=int, default=3, help="child processes per side of the A/B")
ap.add_argument("--predict-only", action="store_true", help="time predict_frame of (c) alone and print one JSON line")
ap.add_argument("--root", default=ROOT, help="with --predict-only: the checkout whose package is timed")
args = ap.parse_args()
if not args.predict_only and not args.out:
    ap.error("--out is needed")
sys.path.insert(0, os.path.abspath(args.root) if args.predict_only else ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
# 19 bones over 17 joints: the COCO pairs the tests use (the cost does not depend on which pairs they are)
COCO = json.load(open(os.path.join(ROOT, "tests", "golden", "coco_skeleton.json")))["coco_skeleton"]


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
    """`count` people of plausible size spread over the frame: (count, 17, 3) (y, x, confidence), all joints live"""
    rng = np.random.default_rng(seed)
    pts = np.empty((count, 17, 3), np.float32)
    for i in range(count):
        bh = rng.uniform(300, 900)
        bw = bh * rng.uniform(0.3, 0.6)
        x1, y1 = rng.uniform(0, wf - bw), rng.uniform(0, hf - bh)
        pts[i, :, 0] = rng.uniform(y1, y1 + bh, 17)
        pts[i, :, 1] = rng.uniform(x1, x1 + bw, 17)
    pts[..., 2] = 0.9
    return pts


pkg = importlib.import_module("simple-hrnet_amd")

if args.predict_only:
    net = pkg.NativeHRNet(32, 17, (256, 192), "bf16", max_batch=8, device=0).load_state_dict(pkg.synth_state_dict(32, 17, 0))
    fdev = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
    p = people_of(8, 1)
    dets = np.stack([p[..., 1].min(1), p[..., 0].min(1), p[..., 1].max(1), p[..., 0].max(1)], 1).astype(np.float32)
    s = timed({"predict": lambda: net.predict_frame(fdev, dets)}, args.rounds, args.reps)["predict"]
    net.close()
    print(json.dumps({"median_ms": statistics.median(s), "min_ms": min(s), "max_ms": max(s)}))
    sys.exit(0)

os.makedirs(args.out, exist_ok=True)
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def fmt(s):
    return "%8.4f ms  (min %.4f .. max %.4f)" % (statistics.median(s), min(s), max(s))


say("pose overlays -- tools/draw_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, medians" % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
rng = np.random.default_rng(6)
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # drawing needs no weights
bgr = torch.from_numpy(rng.integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
nv12 = pkg.YuvFrame(rng.integers(0, 256, hf * wf * 3 // 2, dtype=np.uint8), hf, wf, "nv12").to("cuda:0")
pts = {c: torch.from_numpy(people_of(c, c)).cuda() for c in (8, 64)}
host = torch.empty((hf, wf, 3), dtype=torch.uint8).pin_memory()
nobody = torch.zeros((1, 17, 3), dtype=torch.float32, device="cuda")     # confidence 0: both launches run, every tile returns at once


def round_trip():
    host.copy_(bgr, non_blocking=True)
    bgr.copy_(host, non_blocking=True)


cands = {"empty": lambda: net.draw_poses(bgr[:32, :32], nobody, COCO), "copies": round_trip}
for c in (8, 64):
    cands["bgr%d" % c] = lambda c=c: net.draw_poses(bgr, pts[c], COCO)
    cands["nv12%d" % c] = lambda c=c: net.draw_poses(nv12, pts[c], COCO)
s = timed(cands, args.rounds, args.reps)
say()
say("(a) draw_poses on a %dx%d frame resident in HBM, COCO skeleton (36 primitives per person), radius %d, thickness 2" % (wf, hf, hf // 160))
for c in (8, 64):
    say("    %2d people, BGR    %s" % (c, fmt(s["bgr%d" % c])))
    say("    %2d people, NV12   %s" % (c, fmt(s["nv12%d" % c])))
say("    empty launch pair  %s   (one 32x32 tile, nobody live: the call's host side, one table upload, two launches)" % fmt(s["empty"]))
say("    download + upload  %s   (%.1f MB each way, pinned: what a host drawing pays before it draws)" % (fmt(s["copies"]), hf * wf * 3 / 1e6))
say("    8 people, BGR / (download + upload) = %.3f" % (statistics.median(s["bgr8"]) / statistics.median(s["copies"])))

nf = 30
clip = torch.from_numpy(rng.integers(0, 256, (nf, hf, wf, 3), dtype=np.uint8)).cuda()
frames = [clip[k] for k in range(nf)]
cpts = torch.from_numpy(np.concatenate([people_of(8, 100 + k) for k in range(nf)])).cuda()
index = np.repeat(np.arange(nf, dtype=np.int32), 8)


def per_frame():
    for k in range(nf):
        net.draw_poses(frames[k], cpts[8 * k:8 * k + 8], COCO)


s = timed({"one": lambda: net.draw_poses(frames, cpts, COCO, frame_index=index), "thirty": per_frame}, args.rounds, max(1, args.reps // 4))
say()
say("(b) a %d-frame %dx%d clip, 8 people per frame, BGR, resident" % (nf, wf, hf))
say("    one call           %s" % fmt(s["one"]))
say("    %d calls           %s" % (nf, fmt(s["thirty"])))
say("    one call / %d calls = %.3f" % (nf, statistics.median(s["one"]) / statistics.median(s["thirty"])))
net.close()

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
    say("(c) predict_frame (8 people of a %dx%d frame, HRNet-W32 256x192 bf16): this tree against the parent commit, %d fresh processes"
        % (wf, hf, args.ab_pairs))
    say("    per side, alternately, same box")
    for k in sides:
        say("    %-10s medians %s ms -> %.4f ms" % (k, ", ".join("%.4f" % v for v in meds[k]), statistics.median(meds[k])))
    spread = max(max(v) - min(v) for v in meds.values())
    diff = statistics.median(meds["this tree"]) - statistics.median(meds["parent"])
    say("    difference %+.4f ms; spread of the processes' medians (the wider side) %.4f ms -> %s"
        % (diff, spread, "unchanged" if abs(diff) <= spread else ("SLOWER" if diff > 0 else "faster") + " beyond the spread"))
with open(os.path.join(args.out, "draw_overlay.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
