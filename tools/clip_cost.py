"""Clip mode against the composition it replaces, measured: writes DIR/clip_mode.txt (and prints it).

Workloads: the clip of bench.make_clip (30 frames at 1080p, 8 boxes each, seeded) and a 240-frame clip made the same way -- the
case a video file or a camera wall presents; with 256 people per pass the 30-frame clip is a single group and has nothing to
overlap.  Engine: bench.py's flagship (HRNet-W48, 384x288, bf16, max_batch 256, seeded synthetic weights).

Arms, interleaved in ONE process (round r runs them in a rotated order, so that clock and thermal drift hit them alike), one
warm-up each, the median of --reps repetitions (at least 9), every repetition from pinned host frames to joints on the host:
  A  bench.run_clip(mode="stacked"), called as it stands: one preprocess_frame per frame, torch.cat, one predict_crops, every
     frame uploaded on the compute stream.  Every entry it uses is unchanged by clip mode, so A is also the parent's number.
  B  predict_frames with the frames uploaded inside the timed region on the compute stream: A's work minus the copy of the
     crops and the per-frame calls.
  C  predict_clip from the pinned host frames at people_per_pass 64, 128 and 256: B plus uploads hidden behind the compute.
  D  bench.run_clip(mode="per_frame"): the live loop, for reference (latency path; not what clip mode competes with).
Reported: FPS and persons/s per arm (median, min .. max of the repetitions) and the peak of torch's device allocations per arm
(torch.cuda.max_memory_allocated; the engine's own workspace and pre-path scratch are allocated by the library and the same
for every arm except the pre-path scratch, which grows with the people of one call).

usage: python tools/clip_cost.py --out DIR [--reps R] [--frames 30 240]"""
import argparse
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

import bench         # noqa: E402  (make_clip, run_clip: arm A and D are bench.py's own code)
import costlib       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True, help="directory clip_mode.txt is written to")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--frames", type=int, nargs="+", default=[30, 240])
args = ap.parse_args()
if args.reps < 9:
    ap.error("--reps must be at least 9")

pkg = importlib.import_module("simple-hrnet_amd")
dev = torch.device("cuda", 0)
net = pkg.NativeHRNet(48, 17, (384, 288), "bf16", max_batch=256, device=0).load_state_dict(pkg.synth_state_dict(48, 17, 0))
say = costlib.Report(args.out, "clip_mode.txt").say


def run_frames(clip_host, dets):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    res = net.predict_frames([clip_host[f].to(dev, non_blocking=True) for f in range(len(clip_host))], dets, variant="clamp")
    host = torch.cat([r[1] for r in res]).cpu().numpy()
    torch.cuda.synchronize(dev)
    return host, time.perf_counter() - t0


def run_clip_mode(clip_host, dets, per_pass):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    res = list(net.predict_clip(((clip_host[f], dets[f]) for f in range(len(clip_host))), people_per_pass=per_pass, variant="clamp"))
    host = torch.cat([r[1] for r in res]).cpu().numpy()
    torch.cuda.synchronize(dev)
    return host, time.perf_counter() - t0


say("clip mode: people of many frames in one pre-path launch and pass -- tools/clip_cost.py, %d repetitions per arm, interleaved" % args.reps)
say("device: %s; engine: HRNet-W48 384x288 bf16, max_batch 256, synthetic weights; frames 1920x1080 uint8, pinned host memory"
    % torch.cuda.get_device_name(0))
say("A = bench.run_clip(mode='stacked') unchanged (every entry it calls is unchanged here: A is the parent commit's number)")
say("B = predict_frames, uploads on the compute stream inside the timed region; C = predict_clip from pinned host frames;")
say("D = bench.run_clip(mode='per_frame'), the latency loop, for reference")
verdicts = []
for nf in args.frames:
    clip, dets = bench.make_clip(frames=nf)
    clip_host = torch.from_numpy(clip).pin_memory()
    del clip
    people = int(dets.shape[1])
    arms = {
        "A stacked (bench)": lambda: bench.run_clip(net, clip_host, dets, mode="stacked"),
        "B predict_frames": lambda: run_frames(clip_host, dets),
        "C predict_clip  64": lambda: run_clip_mode(clip_host, dets, 64),
        "C predict_clip 128": lambda: run_clip_mode(clip_host, dets, 128),
        "C predict_clip 256": lambda: run_clip_mode(clip_host, dets, 256),
        "D per_frame (bench)": lambda: bench.run_clip(net, clip_host, dets, mode="per_frame"),
    }
    names = list(arms)
    ref_pts = None
    same = {}
    for k in names:                       # warm-up: scratch, staging, arenas, the allocator's blocks, block maps, clocks
        pts, _ = arms[k]()
        pts = np.asarray(pts).reshape(nf * people, 17, 3)
        if k.startswith("A"):
            ref_pts = pts
        elif not k.startswith("D"):       # (D cuts with the PAD variant: other crops)
            same[k] = bool(np.array_equal(pts, ref_pts))
    secs = {k: [] for k in names}
    peak = {}
    for r in range(args.reps):
        for k in costlib.rotated(names, r):
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            _, dt = arms[k]()
            secs[k].append(dt)
            peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated(dev))
    say()
    say("%d frames x %d people (%d persons per repetition)" % (nf, people, nf * people))
    say("%-22s %10s %22s %12s %14s %s" % ("arm", "FPS median", "FPS min .. max", "persons/s", "torch peak MiB", "joints == A"))
    fps = {}
    for k in names:
        f = sorted(nf / s for s in secs[k])
        fps[k] = (statistics.median(f), f[0], f[-1])
        say("%-22s %10.1f %10.1f .. %-9.1f %12.0f %14.0f %s" % (k, fps[k][0], f[0], f[-1], fps[k][0] * people, peak[k] / 2 ** 20,
                                                               {True: "yes", False: "NO"}.get(same.get(k), "-")))
    a = fps["A stacked (bench)"]
    cand = "B predict_frames" if nf <= 32 else max((k for k in names if k.startswith("C")), key=lambda k: fps[k][0])
    c = fps[cand]
    spread = max(a[2] - a[1], c[2] - c[1])
    ok = c[0] >= a[0] - spread
    verdicts.append("%d frames: %s at %.1f FPS vs A at %.1f FPS (%+.1f %%); repetition spread (max - min, the wider of the two arms) "
                    "%.1f FPS -> %s" % (nf, cand.strip(), c[0], a[0], 100 * (c[0] / a[0] - 1), spread,
                                        "no slower than A" if ok else "SLOWER THAN A BY MORE THAN THE SPREAD"))
    del clip_host
say()
say("condition (B on the 30-frame clip, the best C on the 240-frame clip, each no slower than A by more than the spread):")
for v in verdicts:
    say("  " + v)
net.close()
