"""BGR frames back to 4:2:0 YCbCr on the GPU, measured: writes DIR/bgr_to_yuv.txt (and prints it).  The one condition: bgr_to_yuv is
not slower than the torch composition at 1080p, for nv12 and for p010; everything else is reported as seen.

  (a) NativeHRNet.bgr_to_yuv of a RESIDENT 1080p BGR frame to nv12 and to p010, against
        - the floor of its bytes: the frame read once and the result written once at 6.15 TB/s, and
        - a torch composition of the same result on the device: the frame cast to float32, one (H W, 3) x (3, 3) matmul with the
          real-valued matrix, avg_pool2d of the two chroma channels, round, clamp and the casts (p010: x 4 and << 6 in int32);
          joining its planes into one buffer is NOT charged to it.  It is float arithmetic: within one level of ours, not equal.
  (b) what leaves the device afterwards: the download of the BGR frame against the download of the NV12 frame (pinned buffers).
  (c) one call with 30 frames against 30 calls with one frame.
  (d) --ab-root DIR: predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree against the checkout at DIR (the parent commit,
      built): costlib.ab, the protocol of tools/README.md.  Without --ab-root: NOT MEASURED.
  HIP events around back-to-back calls, host side included, interleaved (round r runs the candidates in a rotated order), medians
  with the spread of the samples beside them.

usage: python tools/bgr2yuv_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]"""
import importlib
import statistics
import sys

import costlib
from costlib import timed

args = costlib.parser(__doc__, "bgr_to_yuv.txt", rounds=9, reps=20, ab="predict_frame").parse_args()
sys.path.insert(0, costlib.ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
HBM = 6.15e12   # bytes per second: the floor printed beside the timings
pkg = importlib.import_module("simple-hrnet_amd")
report = costlib.Report(args.out, "bgr_to_yuv.txt", "%9.4f ms  (min %.4f .. max %.4f)")
say, fmt = report.say, report.fmt

say("BGR to YUV -- tools/bgr2yuv_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, host side included, medians"
    % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # the conversion needs no weights
bgr = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()

# BT.601 limited as real numbers, rows (Y, U, V) over columns (B, G, R): the composition's matmul
kr, kb = 0.299, 0.114
kg = 1.0 - kr - kb
sy, sc = 219.0 / 255.0, 224.0 / 255.0
matrix = torch.tensor([[sy * kb, sy * kg, sy * kr],
                       [sc * 0.5, -sc * kg / (2 * (1 - kb)), -sc * kr / (2 * (1 - kb))],
                       [-sc * kb / (2 * (1 - kr)), -sc * kg / (2 * (1 - kr)), sc * 0.5]], dtype=torch.float32, device="cuda")
offset = torch.tensor([16.0, 128.0, 128.0], dtype=torch.float32, device="cuda")


def composition(ten):
    def run():
        yuv = bgr.to(torch.float32).view(-1, 3) @ matrix.t() + offset
        yuv = yuv.view(hf, wf, 3)
        chroma = torch.nn.functional.avg_pool2d(yuv[:, :, 1:].permute(2, 0, 1).unsqueeze(0), 2)[0].permute(1, 2, 0)
        if ten:
            return ((yuv[:, :, 0] * 4).round().clamp(0, 1023).to(torch.int32) << 6).to(torch.int16), \
                   ((chroma * 4).round().clamp(0, 1023).to(torch.int32) << 6).to(torch.int16).contiguous()
        return yuv[:, :, 0].round().clamp(0, 255).to(torch.uint8), chroma.round().clamp(0, 255).to(torch.uint8).contiguous()
    return run


def planes(frame):
    """(Y (H, W), chroma pairs (H/2, W/2, 2)) of an nv12 / p010 YuvFrame, as integers"""
    if frame.format == "p010":
        words = frame.data.view(torch.int16).to(torch.int32) & 0xFFFF
        return words[:hf * wf].view(hf, wf) >> 6, words[hf * wf:].view(hf // 2, wf // 2, 2) >> 6
    return frame.data[:hf * wf].view(hf, wf).to(torch.int32), frame.data[hf * wf:].view(hf // 2, wf // 2, 2).to(torch.int32)


say()
say("(a) one resident %d x %d BGR frame: bgr_to_yuv against the floor of its bytes and against the torch composition on the device" % (hf, wf))
say("    (cast, matmul, avg_pool2d, round, clamp, casts; BT.601 limited)")
lost = []
for name, ten, out_bytes in (("nv12", False, hf * wf * 3 // 2), ("p010", True, hf * wf * 3)):
    ours_y, ours_c = planes(net.bgr_to_yuv(bgr, name))
    theirs_y, theirs_c = composition(ten)()
    theirs_y, theirs_c = (t.to(torch.int32) & 0xFFFF for t in (theirs_y, theirs_c))
    if ten:
        theirs_y, theirs_c = theirs_y >> 6, theirs_c >> 6
    off = max(int((ours_y - theirs_y).abs().max()), int((ours_c - theirs_c).abs().max()))
    assert off <= (2 if ten else 1), "bgr_to_yuv and the float composition differ by %d levels" % off
    s = timed({"ours": lambda: net.bgr_to_yuv(bgr, name), "torch": composition(ten)}, args.rounds, args.reps)
    ours, theirs = statistics.median(s["ours"]), statistics.median(s["torch"])
    moved = hf * wf * 3 + out_bytes
    floor = moved / HBM * 1e3
    say("    %-5s bgr_to_yuv         %s   bytes floor %.4f ms (%.1f MB read + written at 6.15 TB/s): %.1f x the floor"
        % (name, fmt(s["ours"]), floor, moved / 1e6, ours / floor))
    say("    %-5s torch composition  %s   bgr_to_yuv / torch = %.3f%s   (largest difference between the two results: %d level%s)"
        % (name, fmt(s["torch"]), ours / theirs, "" if ours <= theirs else "   <-- SLOWER than the composition", off, "" if off == 1 else "s"))
    if ours > theirs:
        lost.append(name)
say("    the condition (not slower than the torch composition, nv12 and p010): %s" % ("MET" if not lost else "NOT MET for " + ", ".join(lost)))

say()
say("(b) what crosses PCIe afterwards: the download of the BGR frame against the download of its NV12 form (pinned buffers, synchronised)")
nv12 = net.bgr_to_yuv(bgr, "nv12")
pin = {"bgr": torch.empty(hf * wf * 3, dtype=torch.uint8).pin_memory(), "nv12": torch.empty(hf * wf * 3 // 2, dtype=torch.uint8).pin_memory()}
flat = {"bgr": bgr.view(-1), "nv12": nv12.data}


def download(name, convert=False):
    def run():
        src = net.bgr_to_yuv(bgr, "nv12").data if convert else flat[name]
        pin[name].copy_(src, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    return run


s = timed({"bgr": download("bgr"), "nv12": download("nv12"), "convert + nv12": download("nv12", True)}, args.rounds, max(args.reps // 2, 2))
down_bgr, down_nv12, both = (statistics.median(s[q]) for q in ("bgr", "nv12", "convert + nv12"))
say("    BGR frame, %.1f MB           %s" % (hf * wf * 3 / 1e6, fmt(s["bgr"])))
say("    NV12 frame, %.1f MB          %s   NV12 / BGR = %.3f" % (hf * wf * 1.5 / 1e6, fmt(s["nv12"]), down_nv12 / down_bgr))
say("    bgr_to_yuv + NV12 download  %s   (convert + download) / BGR download = %.3f" % (fmt(s["convert + nv12"]), both / down_bgr))

say()
say("(c) 30 resident %d x %d BGR frames to nv12: ONE call against 30 calls -- per frame, the one call shows what the kernel costs once" % (hf, wf))
say("    the host side of a call is shared by 30 frames")
clip = [torch.from_numpy(np.random.default_rng(20 + i).integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda() for i in range(30)]
outs = [pkg.YuvFrame.empty(hf, wf, "nv12", device=net.torch_device) for _ in range(30)]
floor = 30 * (hf * wf * 3 + hf * wf * 3 // 2) / HBM * 1e3
s = timed({"one call": lambda: net.bgr_to_yuv(clip, out=outs), "30 calls": lambda: [net.bgr_to_yuv(f, out=o) for f, o in zip(clip, outs)]},
          args.rounds, max(args.reps // 4, 2))
one, many = statistics.median(s["one call"]), statistics.median(s["30 calls"])
say("    one call of 30 frames    %s   %.4f ms per frame; bytes floor %.4f ms: %.1f x the floor" % (fmt(s["one call"]), one / 30, floor, one / floor))
say("    30 calls of one frame    %s   one call / 30 calls = %.3f" % (fmt(s["30 calls"]), one / many))
net.close()

say()
runs = costlib.ab(report, "(d)", ["predict"], args.ab_root, args.ab_pairs, args.rounds, args.reps)
say()
say("Not claimed: the time or the bits of cv2.cvtColor(COLOR_BGR2YUV_I420) on a host (cv2 is not installed where this was measured).")
sys.exit(runs is None or bool(lost))
