"""The face mosaic on the GPU, measured: writes DIR/mosaic.txt (and prints it).  No number here is a gate: what the call costs
beside an empty launch pair, and beside the round trip of the frame that the host route pays before it can blur anything, is a
result to record.

  (a) mosaic of the COCO head joints of 8 and of 64 people on a 1080p frame resident in HBM, BGR and NV12, at cell 8 and 32;
      joints on the device.  HIP events, interleaved (round r runs the candidates in a rotated order), medians.  In the same
      rotation:
        - an empty launch pair (a whole mosaic call on a 32x32 view with one person nobody finds: the call's host side, one
          table upload and two launches whose blocks return at once): the floor of a call this small;
        - what the host route pays first: the download and upload of the frame, pinned host memory (the blur comes on top).
  (b) --ab-root DIR: draw_poses (8 and 64 people, BGR) and predict_frame in THIS tree against the checkout at DIR (the parent
      commit, built): costlib.ab, the protocol of tools/README.md.  The expected verdict is "unchanged": the mosaic adds a
      translation unit and touches no existing kernel.  Without --ab-root: NOT MEASURED.

usage: python tools/mosaic_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]"""
import importlib
import statistics
import sys

import costlib

args = costlib.parser(__doc__, "mosaic.txt", rounds=9, reps=20, ab="draw_poses and predict_frame").parse_args()
sys.path.insert(0, costlib.ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
pkg = importlib.import_module("simple-hrnet_amd")
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # the mosaic needs no weights
rng = np.random.default_rng(6)
bgr = torch.from_numpy(rng.integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
nv12 = pkg.YuvFrame(rng.integers(0, 256, hf * wf * 3 // 2, dtype=np.uint8), hf, wf, "nv12").to("cuda:0")
HEAD = pkg.COCO_HEAD_JOINTS


def people(count):
    """costlib's people with a face: the head joints within a sixth of the person's width around a point near its top"""
    pts = costlib.people_of(count, seed=count)[0]
    top, left, width = pts[..., 0].min(1), pts[..., 1].min(1), pts[..., 1].max(1) - pts[..., 1].min(1)
    face = np.random.default_rng(count)
    for j in HEAD:
        pts[:, j, 0] = top + face.uniform(0, 1, count) * width / 6
        pts[:, j, 1] = left + width / 2 + face.uniform(-1, 1, count) * width / 6
    return pts


host_pts = {c: people(c) for c in (8, 64)}
pts = {c: torch.from_numpy(host_pts[c]).cuda() for c in (8, 64)}
report = costlib.Report(args.out, "mosaic.txt")
say, fmt = report.say, report.fmt

say("face mosaic -- tools/mosaic_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, medians" % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
host_frame = torch.empty((hf, wf, 3), dtype=torch.uint8).pin_memory()
nobody = torch.zeros((1, 17, 3), dtype=torch.float32, device="cuda")     # confidence 0: no region, every block returns after the cull


def host_route():
    host_frame.copy_(bgr, non_blocking=True)
    bgr.copy_(host_frame, non_blocking=True)


cands = {"empty": lambda: net.mosaic(bgr[:32, :32], pts=nobody, joints=HEAD), "host": host_route}
for c in (8, 64):
    for cell in (8, 32):
        cands["bgr%d_%d" % (c, cell)] = lambda c=c, cell=cell: net.mosaic(bgr, pts=pts[c], joints=HEAD, cell=cell)
        cands["nv12%d_%d" % (c, cell)] = lambda c=c, cell=cell: net.mosaic(nv12, pts=pts[c], joints=HEAD, cell=cell)
s = costlib.timed(cands, args.rounds, args.reps, warmup=5)
med = {k: statistics.median(v) for k, v in s.items()}
say()
say("(a) mosaic of the COCO head joints on a %dx%d frame resident in HBM, scale 1 / 1, min_half by the rule" % (wf, hf))
for c in (8, 64):
    regions, status = pkg.postproc.mosaic_regions((hf, wf), pts=host_pts[c], joints=HEAD)
    area = int(((regions[:, 2] - regions[:, 0]) * (regions[:, 3] - regions[:, 1])).sum())
    say("    %2d people: %d with a region, the regions cover %.3f frames" % (c, int((status == 0).sum()), area / (hf * wf)))
    for cell in (8, 32):
        say("    %2d people, cell %2d, BGR    %s" % (c, cell, fmt(s["bgr%d_%d" % (c, cell)])))
        say("    %2d people, cell %2d, NV12   %s" % (c, cell, fmt(s["nv12%d_%d" % (c, cell)])))
say("    empty launch pair  %s   (one 32x32 tile, one person nobody finds: the call's host side, one table upload, two launches)" % fmt(s["empty"]))
say("    what the host route pays first  %s   (%.1f MB of frame down and up, pinned; the blur comes on top)" % (fmt(s["host"]), hf * wf * 3 / 1e6))
for c in (8, 64):
    for cell in (8, 32):
        k = "bgr%d_%d" % (c, cell)
        say("    %2d people, cell %2d: BGR / empty launch pair = %.3f;  / host route's copies = %.3f (%s the round trip it replaces);  NV12 / BGR = %.3f"
            % (c, cell, med[k] / med["empty"], med[k] / med["host"], "beats" if med[k] < med["host"] else "DOES NOT BEAT",
               med["nv12%d_%d" % (c, cell)] / med[k]))
net.close()

say()
sys.exit(costlib.ab(report, "(b)", ["draw8", "draw64", "predict"], args.ab_root, args.ab_pairs, args.rounds, args.reps) is None)
