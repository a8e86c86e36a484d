"""Pose overlays on the GPU, measured: writes DIR/draw_overlay.txt (and prints it).  No number here is a gate: what an overlay
costs beside the pass, and beside the two copies any host drawing must pay, is a result to record.

  (a) draw_poses of 8 and of 64 people (COCO skeleton: 19 bones + 17 joints each) on a 1080p frame resident in HBM, BGR and NV12.
      HIP events, interleaved (round r runs the candidates in a rotated order), medians.  In the same rotation:
        - an empty launch pair (a whole draw_poses call on a 32x32 view with nobody live: the call's host side, one table upload
          and two launches whose blocks return at once): the floor of a call this small;
        - the download plus upload of the frame alone (pinned host memory): the least a host drawing pays before it draws.
  (b) a 30-frame 1080p clip, 8 people per frame: one draw_poses call for the clip against 30 calls.
  (c) --ab-root DIR: predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree against the checkout at DIR (the parent commit,
      built): costlib.ab, the protocol of tools/README.md.  Without --ab-root: NOT MEASURED.

usage: python tools/draw_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]"""
import importlib
import statistics
import sys

import costlib

args = costlib.parser(__doc__, "draw_overlay.txt", rounds=9, reps=20, ab="predict_frame").parse_args()
sys.path.insert(0, costlib.ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
COCO = costlib.coco_skeleton()   # 19 bones over 17 joints: the pairs the tests use (the cost does not depend on which pairs they are)
pkg = importlib.import_module("simple-hrnet_amd")
report = costlib.Report(args.out, "draw_overlay.txt")
say, fmt = report.say, report.fmt

say("pose overlays -- tools/draw_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, medians" % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
rng = np.random.default_rng(6)
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # drawing needs no weights
bgr = torch.from_numpy(rng.integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
nv12 = pkg.YuvFrame(rng.integers(0, 256, hf * wf * 3 // 2, dtype=np.uint8), hf, wf, "nv12").to("cuda:0")
pts = {c: torch.from_numpy(costlib.people_of(c, seed=c)[0]).cuda() for c in (8, 64)}
host = torch.empty((hf, wf, 3), dtype=torch.uint8).pin_memory()
nobody = torch.zeros((1, 17, 3), dtype=torch.float32, device="cuda")     # confidence 0: both launches run, every tile returns at once


def round_trip():
    host.copy_(bgr, non_blocking=True)
    bgr.copy_(host, non_blocking=True)


cands = {"empty": lambda: net.draw_poses(bgr[:32, :32], nobody, COCO), "copies": round_trip}
for c in (8, 64):
    cands["bgr%d" % c] = lambda c=c: net.draw_poses(bgr, pts[c], COCO)
    cands["nv12%d" % c] = lambda c=c: net.draw_poses(nv12, pts[c], COCO)
s = costlib.timed(cands, args.rounds, args.reps, warmup=5)
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
cpts = torch.from_numpy(np.concatenate([costlib.people_of(8, seed=100 + k)[0] for k in range(nf)])).cuda()
index = np.repeat(np.arange(nf, dtype=np.int32), 8)


def per_frame():
    for k in range(nf):
        net.draw_poses(frames[k], cpts[8 * k:8 * k + 8], COCO)


s = costlib.timed({"one": lambda: net.draw_poses(frames, cpts, COCO, frame_index=index), "thirty": per_frame}, args.rounds, max(1, args.reps // 4),
                  warmup=5)
say()
say("(b) a %d-frame %dx%d clip, 8 people per frame, BGR, resident" % (nf, wf, hf))
say("    one call           %s" % fmt(s["one"]))
say("    %d calls           %s" % (nf, fmt(s["thirty"])))
say("    one call / %d calls = %.3f" % (nf, statistics.median(s["one"]) / statistics.median(s["thirty"])))
net.close()

say()
sys.exit(costlib.ab(report, "(c)", ["predict"], args.ab_root, args.ab_pairs, args.rounds, args.reps) is None)
