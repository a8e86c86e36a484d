"""Person labels on the GPU, measured: writes DIR/draw_labels.txt (and prints it).  No number here is a gate: what a label costs
beside an empty launch pair, and beside what a label drawn on the host must pay first, is a result to record.

  (a) draw_labels of 8 and of 64 people (box outline, id and score: plate and digits) on a 1080p frame resident in HBM, BGR and
      NV12; ids, boxes and scores on the device.  HIP events, interleaved (round r runs the candidates in a rotated order),
      medians.  In the same rotation:
        - an empty launch pair (a whole draw_labels call on a 32x32 view with one empty box: the call's host side, one table
          upload and two launches whose blocks return at once): the floor of a call this small;
        - the download plus upload of the frame alone (pinned host memory): what cv2.rectangle / cv2.putText on the host pay
          before they draw.
      And, by the host's clock (a synchronisation is not on any stream): the download of ids, boxes and scores followed by the
      synchronisation a host needs before it can turn an id into text, with the stream idle and behind one draw_poses call.
  (b) --ab-root DIR: draw_poses (8 and 64 people, BGR) in THIS tree against the checkout at DIR (the parent commit, built):
      costlib.ab, the protocol of tools/README.md.  Without --ab-root: NOT MEASURED.

usage: python tools/labels_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]"""
import importlib
import statistics
import sys
import time

import costlib

args = costlib.parser(__doc__, "draw_labels.txt", rounds=9, reps=20, ab="draw_poses").parse_args()
sys.path.insert(0, costlib.ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
COCO = costlib.coco_skeleton()
pkg = importlib.import_module("simple-hrnet_amd")
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # drawing needs no weights
rng = np.random.default_rng(6)
bgr = torch.from_numpy(rng.integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
people = {c: costlib.people_of(c, seed=c) for c in (8, 64)}
pts = {c: torch.from_numpy(people[c][0]).cuda() for c in (8, 64)}
report = costlib.Report(args.out, "draw_labels.txt")
say, fmt = report.say, report.fmt

say("person labels -- tools/labels_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, medians" % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
nv12 = pkg.YuvFrame(rng.integers(0, 256, hf * wf * 3 // 2, dtype=np.uint8), hf, wf, "nv12").to("cuda:0")
boxes = {c: torch.from_numpy(people[c][1]).cuda() for c in (8, 64)}
ids = {c: torch.arange(100, 100 + c, dtype=torch.int32, device="cuda") for c in (8, 64)}
scores = {c: torch.from_numpy(rng.uniform(0, 1, c).astype(np.float32)).cuda() for c in (8, 64)}
host = torch.empty((hf, wf, 3), dtype=torch.uint8).pin_memory()
nobody = torch.zeros((1, 4), dtype=torch.int32, device="cuda")           # the empty box: both launches run, every tile returns at once


def round_trip():
    host.copy_(bgr, non_blocking=True)
    bgr.copy_(host, non_blocking=True)


cands = {"empty": lambda: net.draw_labels(bgr[:32, :32], nobody), "copies": round_trip}
for c in (8, 64):
    cands["bgr%d" % c] = lambda c=c: net.draw_labels(bgr, boxes[c], ids[c], scores[c])
    cands["nv12%d" % c] = lambda c=c: net.draw_labels(nv12, boxes[c], ids[c], scores[c])
s = costlib.timed(cands, args.rounds, args.reps, warmup=5)
say()
say("(a) draw_labels on a %dx%d frame resident in HBM: outline (thickness 2), three id digits, a blank and the score, scale %d"
    % (wf, hf, max(1, hf // 360)))
for c in (8, 64):
    say("    %2d people, BGR    %s" % (c, fmt(s["bgr%d" % c])))
    say("    %2d people, NV12   %s" % (c, fmt(s["nv12%d" % c])))
say("    empty launch pair  %s   (one 32x32 tile, one empty box: the call's host side, one table upload, two launches)" % fmt(s["empty"]))
say("    download + upload  %s   (%.1f MB each way, pinned: what drawing the labels on the host pays before it draws)"
    % (fmt(s["copies"]), hf * wf * 3 / 1e6))
say("    8 people, BGR / empty launch pair = %.3f;  / (download + upload) = %.3f"
    % (statistics.median(s["bgr8"]) / statistics.median(s["empty"]), statistics.median(s["bgr8"]) / statistics.median(s["copies"])))

# what a host pays before it can even form the text: ids, boxes and scores downloaded and the stream synchronised
pinned = {c: [torch.empty_like(t, device="cpu").pin_memory() for t in (boxes[c], ids[c], scores[c])] for c in (8, 64)}


def state_download(c, busy):
    out = []
    for _ in range(args.rounds * args.reps):
        if busy:
            net.draw_poses(bgr, pts[c], COCO)
        t0 = time.perf_counter()
        for dst, src in zip(pinned[c], (boxes[c], ids[c], scores[c])):
            dst.copy_(src, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


say("    ids + boxes + scores to the host and the synchronisation before the text can be formed (host clock, %d calls):" % (args.rounds * args.reps))
for c in (8, 64):
    idle, busy = state_download(c, False), state_download(c, True)
    say("    %2d people          idle stream %s" % (c, fmt(idle)))
    say("                       behind one draw_poses %s" % fmt(busy))
net.close()

say()
sys.exit(costlib.ab(report, "(b)", ["draw8", "draw64"], args.ab_root, args.ab_pairs, args.rounds, args.reps) is None)
