"""Heat-map overlays on the GPU, measured: writes DIR/draw_heatmaps.txt (and prints it).  No number here is a gate: what an
overlay costs beside an empty launch pair, and beside what the host route must pay before it can start, is a result to record.

  (a) draw_heatmaps of 8 and of 64 people (64x48 maps, J = 17, all joints, jet, alpha by value) on a 1080p frame resident in HBM,
      BGR and NV12; maps and boxes on the device.  HIP events, interleaved (round r runs the candidates in a rotated order),
      medians.  In the same rotation:
        - an empty launch pair (a whole draw_heatmaps call on a 32x32 view with one empty box and a 1x1 map: the call's host
          side, one table upload and two launches whose blocks return at once): the floor of a call this small;
        - what the host route pays before it can start: the download of the (n, J, 48, 64) maps plus the download and upload of
          the frame, pinned host memory (the resize, colour map and blend per person come on top of it).
  (b) --ab-root DIR: draw_poses (8 and 64 people, BGR) and predict_frame in THIS tree against the checkout at DIR (the parent
      commit, built): costlib.ab, the protocol of tools/README.md.  The expected verdict is "unchanged"; a draw_poses
      difference beyond the spread would mean that moving block_compact / frame_of_tile into csrc/draw_tile.h changed the code
      of draw.hip.  Without --ab-root: NOT MEASURED.

usage: python tools/heatmaps_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]"""
import importlib
import statistics
import sys

import costlib

args = costlib.parser(__doc__, "draw_heatmaps.txt", rounds=9, reps=20, ab="draw_poses and predict_frame").parse_args()
sys.path.insert(0, costlib.ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf, J, hq, wq = 1080, 1920, 17, 64, 48
pkg = importlib.import_module("simple-hrnet_amd")
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # drawing needs no weights
rng = np.random.default_rng(6)
bgr = torch.from_numpy(rng.integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
nv12 = pkg.YuvFrame(rng.integers(0, 256, hf * wf * 3 // 2, dtype=np.uint8), hf, wf, "nv12").to("cuda:0")
boxes = {c: torch.from_numpy(costlib.people_of(c, seed=c)[1]).cuda() for c in (8, 64)}
maps = {c: torch.from_numpy(rng.uniform(0, 1, (c, J, hq, wq)).astype(np.float32) ** 4).cuda() for c in (8, 64)}   # mostly low, some peaks
report = costlib.Report(args.out, "draw_heatmaps.txt")
say, fmt = report.say, report.fmt

say("heat-map overlays -- tools/heatmaps_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, medians" % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
host_frame = torch.empty((hf, wf, 3), dtype=torch.uint8).pin_memory()
host_maps = {c: torch.empty((c, J, hq, wq), dtype=torch.float32).pin_memory() for c in (8, 64)}
nobody, no_map = torch.zeros((1, 4), dtype=torch.int32, device="cuda"), torch.zeros((1, 1, 1, 1), dtype=torch.float32, device="cuda")


def host_route(c):
    host_maps[c].copy_(maps[c], non_blocking=True)
    host_frame.copy_(bgr, non_blocking=True)
    bgr.copy_(host_frame, non_blocking=True)


cands = {"empty": lambda: net.draw_heatmaps(bgr[:32, :32], no_map, nobody)}
for c in (8, 64):
    cands["bgr%d" % c] = lambda c=c: net.draw_heatmaps(bgr, maps[c], boxes[c])
    cands["nv12%d" % c] = lambda c=c: net.draw_heatmaps(nv12, maps[c], boxes[c])
    cands["host%d" % c] = lambda c=c: host_route(c)
s = costlib.timed(cands, args.rounds, args.reps, warmup=5)
med = {k: statistics.median(v) for k, v in s.items()}
say()
say("(a) draw_heatmaps on a %dx%d frame resident in HBM: %dx%d maps, J = %d, all joints, jet, alpha 0.6 by value, cutoff 0.1" % (wf, hf, hq, wq, J))
for c in (8, 64):
    area = int(((boxes[c][:, 2] - boxes[c][:, 0]).clamp(min=0) * (boxes[c][:, 3] - boxes[c][:, 1]).clamp(min=0)).sum())
    say("    %2d people, BGR    %s   (%.1f MB of maps read once, boxes cover %.2f frames)"
        % (c, fmt(s["bgr%d" % c]), c * J * hq * wq * 4 / 1e6, area / (hf * wf)))
    say("    %2d people, NV12   %s" % (c, fmt(s["nv12%d" % c])))
    say("    %2d people, what the host route pays first  %s   (%.1f MB of maps down, %.1f MB of frame down and up, pinned)"
        % (c, fmt(s["host%d" % c]), c * J * hq * wq * 4 / 1e6, hf * wf * 3 / 1e6))
say("    empty launch pair  %s   (one 32x32 tile, one empty box, a 1x1 map: the call's host side, one table upload, two launches)" % fmt(s["empty"]))
for c in (8, 64):
    say("    %2d people, BGR / empty launch pair = %.3f;  / host route's copies = %.3f;  NV12 / BGR = %.3f"
        % (c, med["bgr%d" % c] / med["empty"], med["bgr%d" % c] / med["host%d" % c], med["nv12%d" % c] / med["bgr%d" % c]))
net.close()

say()
sys.exit(costlib.ab(report, "(b)", ["draw8", "draw64", "predict"], args.ab_root, args.ab_pairs, args.rounds, args.reps) is None)
