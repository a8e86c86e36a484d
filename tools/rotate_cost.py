"""Frame rotation on the GPU, measured: writes DIR/rotate_frames.txt (and prints it).  The one condition: rotate_frames is not slower
than the torch composition at 1080p, for any format and code; everything else is reported as seen.

  (a) NativeHRNet.rotate_frames of a RESIDENT 1080p frame, BGR and NV12, at each of the three codes, against
        - the torch composition on the device: torch.rot90(plane, k).contiguous() per plane (NV12: the Y plane and the (H/2, W/2, 2)
          pair plane; joining the two planes into one buffer again is NOT charged to it), and
        - what a host rotation pays before it rotates anything: the download of the frame and the upload of the result (pinned).
      Beside each rotate_frames timing: the floor of reading and writing the frame's bytes once at 6.15 TB/s, and the multiple.
  (b) one call with 30 frames against 30 calls with one frame and against 30 torch compositions, at each code.
  (c) --ab-root DIR: predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree against the checkout at DIR (the parent commit,
      built), each in fresh child processes run alternately on the same box; a difference inside the spread of the children's
      medians is "unchanged".  Without --ab-root: NOT MEASURED.
  HIP events around back-to-back calls, host side included, interleaved (round r runs the candidates in a rotated order), medians
  with the spread of the samples beside them.

usage: python tools/rotate_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]
       python tools/rotate_cost.py --child-only [--root DIR]     (the child of (c): one JSON line)"""
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
ap.add_argument("--out", help="directory rotate_frames.txt is written to")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=20, help="calls per timed sample")
ap.add_argument("--ab-root", help="checkout of the parent commit, built: predict_frame there against here")
ap.add_argument("--ab-pairs", type=int, default=3, help="child processes per side of the A/B")
ap.add_argument("--child-only", action="store_true", help="time predict_frame of (c) alone and print one JSON line")
ap.add_argument("--root", default=ROOT, help="with --child-only: the checkout whose package is timed")
args = ap.parse_args()
if not args.child_only and not args.out:
    ap.error("--out is needed")
sys.path.insert(0, os.path.abspath(args.root) if args.child_only else ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
HBM = 6.15e12   # bytes per second: the floor printed beside the timings
ROT90_K = {0: -1, 1: 2, 2: 1}
CODE_NAMES = {0: "90 cw ", 1: "180   ", 2: "90 ccw"}


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


pkg = importlib.import_module("simple-hrnet_amd")

if args.child_only:
    net = pkg.NativeHRNet(32, 17, (256, 192), "bf16", max_batch=8, device=0).load_state_dict(pkg.synth_state_dict(32, 17, 0))
    fdev = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
    rng = np.random.default_rng(1)
    x1, y1 = rng.uniform(0, wf - 400, 8), rng.uniform(0, hf - 700, 8)
    boxes = np.stack([x1, y1, x1 + rng.uniform(150, 400, 8), y1 + rng.uniform(300, 700, 8)], 1).astype(np.float32)
    s = timed({"predict": lambda: net.predict_frame(fdev, boxes)}, args.rounds, args.reps)
    net.close()
    print(json.dumps({k: statistics.median(v) for k, v in s.items()}))
    sys.exit(0)

os.makedirs(args.out, exist_ok=True)
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def fmt(s):
    return "%9.4f ms  (min %.4f .. max %.4f)" % (statistics.median(s), min(s), max(s))


say("frame rotation -- tools/rotate_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, host side included, medians"
    % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # rotation needs no weights
bgr = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
nv12 = pkg.YuvFrame(np.random.default_rng(7).integers(0, 256, hf * wf * 3 // 2, dtype=np.uint8), hf, wf, "nv12").to(net.torch_device)
luma = nv12.data[:hf * wf].view(hf, wf)
pairs = nv12.data[hf * wf:].view(hf // 2, wf // 2, 2)
pin = {"bgr": torch.empty(hf * wf * 3, dtype=torch.uint8).pin_memory(), "nv12": torch.empty(hf * wf * 3 // 2, dtype=torch.uint8).pin_memory()}
flat = {"bgr": bgr.view(-1), "nv12": nv12.data}


def transfers(name):
    def run():
        pin[name].copy_(flat[name], non_blocking=True)
        torch.cuda.current_stream().synchronize()          # the host rotation would run here
        return pin[name].cuda(non_blocking=True)
    return run


say()
say("(a) one resident %d x %d frame: rotate_frames against torch.rot90(plane).contiguous() per plane on the device, and against the" % (hf, wf))
say("    transfers a host rotation pays before it rotates (frame down, result up; pinned buffers)")
lost = []
for code in (0, 1, 2):
    k = ROT90_K[code]
    got = net.rotate_frames(bgr, code)
    assert torch.equal(got, torch.rot90(bgr, k, (0, 1))), "rotate_frames disagrees with torch.rot90"
    s = timed({"bgr": lambda: net.rotate_frames(bgr, code), "nv12": lambda: net.rotate_frames(nv12, code),
               "torch bgr": lambda: torch.rot90(bgr, k, (0, 1)).contiguous(),
               "torch nv12": lambda: (torch.rot90(luma, k, (0, 1)).contiguous(), torch.rot90(pairs, k, (0, 1)).contiguous()),
               "host bgr": transfers("bgr"), "host nv12": transfers("nv12")}, args.rounds, args.reps)
    say("    code %d (%s)" % (code, CODE_NAMES[code].strip()))
    for name, frame_bytes in (("bgr", hf * wf * 3), ("nv12", hf * wf * 3 // 2)):
        ours, theirs, host = (statistics.median(s[q]) for q in (name, "torch " + name, "host " + name))
        floor = 2 * frame_bytes / HBM * 1e3
        say("        %-5s rotate_frames      %s   bytes floor %.4f ms (%.1f MB read + written at 6.15 TB/s): %.1f x the floor"
            % (name, fmt(s[name]), floor, 2 * frame_bytes / 1e6, ours / floor))
        say("        %-5s torch composition  %s   rotate_frames / torch = %.3f%s"
            % (name, fmt(s["torch " + name]), ours / theirs, "" if ours <= theirs else "   <-- SLOWER than the composition"))
        say("        %-5s transfers alone    %s   rotate_frames / transfers = %.3f" % (name, fmt(s["host " + name]), ours / host))
        if ours > theirs:
            lost.append("%s code %d" % (name, code))
say("    the condition (not slower than the torch composition for any format and code): %s"
    % ("MET" if not lost else "NOT MET for " + ", ".join(lost)))

say()
say("(b) 30 resident %d x %d BGR frames: ONE call against 30 calls, and against 30 torch compositions -- per frame, the one call shows" % (hf, wf))
say("    what the kernel costs once the host side of a call is shared by 30 frames")
clip = [torch.from_numpy(np.random.default_rng(20 + i).integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda() for i in range(30)]
floor = 30 * 2 * hf * wf * 3 / HBM * 1e3
for code in (0, 1, 2):
    k = ROT90_K[code]
    s = timed({"one call": lambda: net.rotate_frames(clip, code), "30 calls": lambda: [net.rotate_frames(f, code) for f in clip],
               "30 torch": lambda: [torch.rot90(f, k, (0, 1)).contiguous() for f in clip]}, args.rounds, max(args.reps // 4, 2))
    one, many, theirs = (statistics.median(s[q]) for q in ("one call", "30 calls", "30 torch"))
    say("    code %d (%s)" % (code, CODE_NAMES[code].strip()))
    say("        one call of 30 frames    %s   %.4f ms per frame; bytes floor %.4f ms: %.1f x the floor" % (fmt(s["one call"]), one / 30, floor, one / floor))
    say("        30 calls of one frame    %s   one call / 30 calls = %.3f" % (fmt(s["30 calls"]), one / many))
    say("        30 torch compositions    %s   one call / 30 compositions = %.3f" % (fmt(s["30 torch"]), one / theirs))
net.close()

say()
if not args.ab_root:
    say("(c) predict_frame, this tree against the parent commit: NOT MEASURED (no --ab-root)")
else:
    sides = {"parent": os.path.abspath(args.ab_root), "this tree": ROOT}
    meds = {k: [] for k in sides}
    for _ in range(args.ab_pairs):
        for k, root in sides.items():    # fresh children, alternately
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-only", "--root", root, "--rounds", str(args.rounds),
                                  "--reps", str(args.reps)], capture_output=True, text=True, timeout=300, check=True).stdout
            meds[k].append(json.loads(out.strip().splitlines()[-1])["predict"])
    say("(c) predict_frame, 8 people of a 1080p frame, HRNet-W32 256x192 bf16: this tree against the parent commit, %d fresh processes per"
        % args.ab_pairs)
    say("    side, alternately, same box")
    for k in sides:
        say("        %-10s medians %s ms -> %.4f ms" % (k, ", ".join("%.4f" % v for v in meds[k]), statistics.median(meds[k])))
    spread = max(max(meds[k]) - min(meds[k]) for k in sides)
    diff = statistics.median(meds["this tree"]) - statistics.median(meds["parent"])
    say("        difference %+.4f ms; spread of the processes' medians (the wider side) %.4f ms -> %s"
        % (diff, spread, "unchanged" if abs(diff) <= spread else ("SLOWER" if diff > 0 else "faster") + " beyond the spread"))
say()
say("Not claimed: the time of cv2.rotate on a host (cv2 is not installed where this was measured).  Equality with cv2.rotate needs no")
say("cv2: it is a permutation, pinned against np.rot90 (tests/test_rotate_gpu.py).")
with open(os.path.join(args.out, "rotate_frames.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
