"""Person ids on the GPU, measured: writes DIR/assoc_ids.txt (and prints it).  No number here is a gate: what the association
costs beside the host round trip it replaces, and what its single-wave assignment costs at the cap, are results to record.

  (a) NativeHRNet.associate_people (one launch, demo parameters, J = 17) at 8 x 8, 64 x 64 and 256 x 256 people against the host
      path it replaces: download pts and boxes, postproc.find_person_id_associations, upload ids and the smoothed pts and boxes.
      HIP events around back-to-back calls, host side included, interleaved (round r runs the candidates in a rotated order),
      medians.  In the same rotation, per size, the same call on an engine created under HRN_ASSOC_NO_ASSIGN=1 (debug switch: the
      assignment phase is skipped): the difference is the single wave's share.
  (b) draw_poses with ids from the host against ids on the device (8 people, 1080p BGR, resident).
  (c) --ab-root DIR: draw_poses with host ids (8 people, 1080p) and predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree
      against the checkout at DIR (the parent commit, built), each in fresh child processes run alternately on the same box; a
      difference inside the spread of the children's medians is "unchanged".  Without --ab-root: NOT MEASURED.

usage: python tools/assoc_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]
       python tools/assoc_cost.py --child-only [--root DIR]     (the child of (c): one JSON line)"""
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
ap.add_argument("--out", help="directory assoc_ids.txt is written to")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=20, help="calls per timed sample")
ap.add_argument("--ab-root", help="checkout of the parent commit, built: draw_poses and predict_frame there against here")
ap.add_argument("--ab-pairs", type=int, default=3, help="child processes per side of the A/B")
ap.add_argument("--child-only", action="store_true", help="time draw_poses and predict_frame of (c) alone and print one JSON line")
ap.add_argument("--root", default=ROOT, help="with --child-only: the checkout whose package is timed")
args = ap.parse_args()
if not args.child_only and not args.out:
    ap.error("--out is needed")
sys.path.insert(0, os.path.abspath(args.root) if args.child_only else ROOT)
os.environ["HRN_DEBUG_ENV"] = "1"   # (the library reads switches only in a process that opts in; none is set but for (a)'s second engine)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
COCO = json.load(open(os.path.join(ROOT, "tests", "golden", "coco_skeleton.json")))["coco_skeleton"]


def timed(cands, rounds, reps):
    """HIP-event ms per call of every candidate: `rounds` samples of `reps` calls each, interleaved in a rotated order"""
    for fn in cands.values():
        for _ in range(3):
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


def people_of(count, seed, jitter=0.0, base=None):
    """`count` people spread over the frame: ((count, 17, 3) (y, x, confidence), (count, 4) int32 boxes)"""
    rng = np.random.default_rng(seed)
    if base is None:
        pts = np.empty((count, 17, 3), np.float32)
        for i in range(count):
            bh = rng.uniform(300, 900)
            bw = bh * rng.uniform(0.3, 0.6)
            x1, y1 = rng.uniform(0, wf - bw), rng.uniform(0, hf - bh)
            pts[i, :, 0] = rng.uniform(y1, y1 + bh, 17)
            pts[i, :, 1] = rng.uniform(x1, x1 + bw, 17)
        pts[..., 2] = 0.9
    else:
        pts = base.copy()
        pts[..., :2] += rng.normal(0, jitter, pts[..., :2].shape).astype(np.float32)
    boxes = np.stack([pts[..., 1].min(1), pts[..., 0].min(1), pts[..., 1].max(1), pts[..., 0].max(1)], 1)
    return pts, np.round(boxes).astype(np.int32)


pkg = importlib.import_module("simple-hrnet_amd")

if args.child_only:
    net = pkg.NativeHRNet(32, 17, (256, 192), "bf16", max_batch=8, device=0).load_state_dict(pkg.synth_state_dict(32, 17, 0))
    fdev = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
    p, boxes = people_of(8, 1)
    pdev, ids = torch.from_numpy(p).cuda(), np.arange(8, dtype=np.int32)
    s = timed({"predict": lambda: net.predict_frame(fdev, boxes.astype(np.float32)),
               "draw": lambda: net.draw_poses(fdev, pdev, COCO, person_ids=ids)}, args.rounds, args.reps)
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
    prev_pts, prev_boxes = people_of(count, count)
    order = np.random.default_rng(count).permutation(count)
    cur_pts, cur_boxes = people_of(count, count + 1, jitter=3.0, base=prev_pts[order])
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
pts8 = torch.from_numpy(people_of(8, 8)[0]).cuda()
ids_host = np.arange(3, 11, dtype=np.int32)
ids_dev = torch.from_numpy(ids_host).cuda()
s = timed({"host": lambda: net.draw_poses(bgr, pts8, COCO, person_ids=ids_host), "device": lambda: net.draw_poses(bgr, pts8, COCO, person_ids=ids_dev)},
          args.rounds, args.reps)
say("(b) draw_poses, 8 people on a %dx%d BGR frame resident in HBM" % (wf, hf))
say("    ids from the host    %s   (two launches)" % fmt(s["host"]))
say("    ids on the device    %s   (three launches, no host read)" % fmt(s["device"]))
net.close()

say()
if not args.ab_root:
    say("(c) draw_poses with host ids and predict_frame, this tree against the parent commit: NOT MEASURED (no --ab-root)")
else:
    sides = {"parent": os.path.abspath(args.ab_root), "this tree": ROOT}
    meds = {k: {"draw": [], "predict": []} for k in sides}
    for _ in range(args.ab_pairs):
        for k, root in sides.items():    # fresh children, alternately
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-only", "--root", root, "--rounds", str(args.rounds),
                                  "--reps", str(args.reps)], capture_output=True, text=True, timeout=300, check=True).stdout
            res = json.loads(out.strip().splitlines()[-1])
            for what in ("draw", "predict"):
                meds[k][what].append(res[what])
    say("(c) this tree against the parent commit, %d fresh processes per side, alternately, same box" % args.ab_pairs)
    for what, title in (("draw", "draw_poses, host ids, 8 people, 1080p BGR"), ("predict", "predict_frame, 8 people of a 1080p frame, HRNet-W32 256x192 bf16")):
        say("    %s" % title)
        for k in sides:
            say("        %-10s medians %s ms -> %.4f ms" % (k, ", ".join("%.4f" % v for v in meds[k][what]), statistics.median(meds[k][what])))
        spread = max(max(meds[k][what]) - min(meds[k][what]) for k in sides)
        diff = statistics.median(meds["this tree"][what]) - statistics.median(meds["parent"][what])
        say("        difference %+.4f ms; spread of the processes' medians (the wider side) %.4f ms -> %s"
            % (diff, spread, "unchanged" if abs(diff) <= spread else ("SLOWER" if diff > 0 else "faster") + " beyond the spread"))
say()
say("Not claimed: how well these ids follow people on a trained network -- no trained weights and no video exist where this was measured.")
with open(os.path.join(args.out, "assoc_ids.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
