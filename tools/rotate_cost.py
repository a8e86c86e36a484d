"""Frame rotation on the GPU, measured: writes DIR/rotate_frames.txt (and prints it).  The one condition: rotate_frames is not slower
than the torch composition at 1080p, for any format and code; everything else is reported as seen.

  (a) NativeHRNet.rotate_frames of a RESIDENT 1080p frame, BGR and NV12, at each of the three codes, against
        - the torch composition on the device: torch.rot90(plane, k).contiguous() per plane (NV12: the Y plane and the (H/2, W/2, 2)
          pair plane; joining the two planes into one buffer again is NOT charged to it), and
        - what a host rotation pays before it rotates anything: the download of the frame and the upload of the result (pinned).
      Beside each rotate_frames timing: the floor of reading and writing the frame's bytes once at 6.15 TB/s, and the multiple.
  (b) one call with 30 frames against 30 calls with one frame and against 30 torch compositions, at each code.
  (c) --ab-root DIR: predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree against the checkout at DIR (the parent commit,
      built): costlib.ab, the protocol of tools/README.md.  Without --ab-root: NOT MEASURED.
  HIP events around back-to-back calls, host side included, interleaved (round r runs the candidates in a rotated order), medians
  with the spread of the samples beside them.

usage: python tools/rotate_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]"""
import importlib
import statistics
import sys

import costlib
from costlib import timed

args = costlib.parser(__doc__, "rotate_frames.txt", rounds=9, reps=20, ab="predict_frame").parse_args()
sys.path.insert(0, costlib.ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
HBM = 6.15e12   # bytes per second: the floor printed beside the timings
ROT90_K = {0: -1, 1: 2, 2: 1}
CODE_NAMES = {0: "90 cw ", 1: "180   ", 2: "90 ccw"}
pkg = importlib.import_module("simple-hrnet_amd")
report = costlib.Report(args.out, "rotate_frames.txt", "%9.4f ms  (min %.4f .. max %.4f)")
say, fmt = report.say, report.fmt

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
runs = costlib.ab(report, "(c)", ["predict"], args.ab_root, args.ab_pairs, args.rounds, args.reps)
say()
say("Not claimed: the time of cv2.rotate on a host (cv2 is not installed where this was measured).  Equality with cv2.rotate needs no")
say("cv2: it is a permutation, pinned against np.rot90 (tests/test_rotate_gpu.py).")
sys.exit(runs is None)
