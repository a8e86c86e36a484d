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
  (b) --ab-root DIR: draw_poses (8 and 64 people, BGR) in THIS tree against the checkout at DIR (the parent commit, built), each
      in fresh child processes run alternately on the same box, the parent first and last.  The spread between the parent's own
      runs is stated; a difference inside it is "unchanged".  Without --ab-root: NOT MEASURED.

usage: python tools/labels_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]
       python tools/labels_cost.py --draw-only [--root DIR]     (the child of (b): one JSON line)"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--out", help="directory draw_labels.txt is written to")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=20, help="calls per timed sample")
ap.add_argument("--ab-root", help="checkout of the parent commit, built: draw_poses there against here")
ap.add_argument("--ab-pairs", type=int, default=3, help="child processes of this tree in the A/B (the parent runs once more)")
ap.add_argument("--draw-only", action="store_true", help="time draw_poses of (b) alone and print one JSON line")
ap.add_argument("--root", default=ROOT, help="with --draw-only: the checkout whose package is timed")
args = ap.parse_args()
if not args.draw_only and not args.out:
    ap.error("--out is needed")
sys.path.insert(0, os.path.abspath(args.root) if args.draw_only else ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
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
    """`count` people of plausible size spread over the frame: boxes (count, 4) int32 and joints (count, 17, 3) inside them"""
    rng = np.random.default_rng(seed)
    boxes, pts = np.empty((count, 4), np.int32), np.empty((count, 17, 3), np.float32)
    for i in range(count):
        bh = rng.uniform(300, 900)
        bw = bh * rng.uniform(0.3, 0.6)
        x1, y1 = rng.uniform(0, wf - bw), rng.uniform(0, hf - bh)
        boxes[i] = x1, y1, x1 + bw, y1 + bh
        pts[i, :, 0] = rng.uniform(y1, y1 + bh, 17)
        pts[i, :, 1] = rng.uniform(x1, x1 + bw, 17)
    pts[..., 2] = 0.9
    return boxes, pts


pkg = importlib.import_module("simple-hrnet_amd")
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # drawing needs no weights
rng = np.random.default_rng(6)
bgr = torch.from_numpy(rng.integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
people = {c: people_of(c, c) for c in (8, 64)}
pts = {c: torch.from_numpy(people[c][1]).cuda() for c in (8, 64)}

if args.draw_only:
    s = timed({"bgr%d" % c: (lambda c=c: net.draw_poses(bgr, pts[c], COCO)) for c in (8, 64)}, args.rounds, args.reps)
    net.close()
    print(json.dumps({k: statistics.median(v) for k, v in s.items()}))
    sys.exit(0)

os.makedirs(args.out, exist_ok=True)
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def fmt(s):
    return "%8.4f ms  (min %.4f .. max %.4f)" % (statistics.median(s), min(s), max(s))


say("person labels -- tools/labels_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, medians" % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
nv12 = pkg.YuvFrame(rng.integers(0, 256, hf * wf * 3 // 2, dtype=np.uint8), hf, wf, "nv12").to("cuda:0")
boxes = {c: torch.from_numpy(people[c][0]).cuda() for c in (8, 64)}
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
s = timed(cands, args.rounds, args.reps)
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
if not args.ab_root:
    say("(b) draw_poses, this tree against the parent commit: NOT MEASURED (no --ab-root)")
else:
    sides = {"parent": os.path.abspath(args.ab_root), "this tree": ROOT}
    order = ["parent"] + ["this tree", "parent"] * args.ab_pairs         # fresh children, alternately, the parent first and last
    meds = {k: {"bgr8": [], "bgr64": []} for k in sides}
    for k in order:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--draw-only", "--root", sides[k], "--rounds", str(args.rounds),
                              "--reps", str(args.reps)], capture_output=True, text=True, timeout=300, check=True).stdout
        for name, v in json.loads(out.strip().splitlines()[-1]).items():
            meds[k][name].append(v)
    say("(b) draw_poses on the %dx%d BGR frame: this tree against the parent commit, fresh processes run alternately on the same box" % (wf, hf))
    for name, c in (("bgr8", 8), ("bgr64", 64)):
        for k in sides:
            say("    %2d people, %-10s medians %s ms -> %.4f ms" % (c, k, ", ".join("%.4f" % v for v in meds[k][name]), statistics.median(meds[k][name])))
        spread = max(meds["parent"][name]) - min(meds["parent"][name])
        diff = statistics.median(meds["this tree"][name]) - statistics.median(meds["parent"][name])
        say("    %2d people: difference %+.4f ms; spread between the parent's own runs %.4f ms -> %s"
            % (c, diff, spread, "unchanged" if abs(diff) <= spread else ("SLOWER" if diff > 0 else "faster") + " beyond the spread"))
with open(os.path.join(args.out, "draw_labels.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
