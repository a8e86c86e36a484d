"""The detector link on the GPU, measured: writes DIR/letterbox.txt (and prints it).  No number here is a gate.

  (a) NativeHRNet.detector_input of a RESIDENT 1080p frame to 640 x 640 (style yolov5), float16 and float32, from BGR and from NV12,
      against what ANY host letterbox pays before it computes anything: the download of the frame (NV12: after yuv_to_bgr) and the
      upload of the finished tensor.  cv2 is absent here, so NO host letterbox time is claimed: the host side is a lower bound.
      Beside each timing: the bytes the call must move (frame bytes read once + tensor bytes written) at 6.15 TB/s.
  (b) NativeHRNet.detections_to_frame at 8 / 64 / 700 rows against the host round trip (download, postproc.detections_to_frame,
      upload).
  (c) --ab-root DIR: predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree against the checkout at DIR (the parent commit,
      built), each in fresh child processes run alternately on the same box; a difference inside the spread of the children's
      medians is "unchanged".  Without --ab-root: NOT MEASURED.
  HIP events around back-to-back calls, host side included, interleaved (round r runs the candidates in a rotated order), medians.

usage: python tools/letterbox_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]
       python tools/letterbox_cost.py --child-only [--root DIR]     (the child of (c): one JSON line)"""
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
ap.add_argument("--out", help="directory letterbox.txt is written to")
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


say("the detector link -- tools/letterbox_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, host side included, medians"
    % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # the link needs no weights
size = 640

say()
say("(a) detector_input, one resident %d x %d frame -> %d x %d (yolov5 letterbox), against the transfers ANY host letterbox pays first" % (hf, wf, size, size))
say("    (frame down, tensor up; pinned buffers; NV12: yuv_to_bgr before the download).  cv2 is absent: no host letterbox time is claimed.")
bgr = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (hf, wf, 3), dtype=np.uint8)).cuda()
nv12 = pkg.YuvFrame(np.random.default_rng(7).integers(0, 256, hf * wf * 3 // 2, dtype=np.uint8), hf, wf, "nv12").to(net.torch_device)
pin_frame = torch.empty((hf, wf, 3), dtype=torch.uint8).pin_memory()
for dtype in (torch.float16, torch.float32):
    esize = 2 if dtype == torch.float16 else 4
    pin_tensor = torch.empty((1, 3, size, size), dtype=dtype).pin_memory()

    def transfers_bgr():
        pin_frame.copy_(bgr, non_blocking=True)
        torch.cuda.current_stream().synchronize()          # the host letterbox would run here
        return pin_tensor.cuda(non_blocking=True)

    def transfers_nv12():
        pin_frame.copy_(net.yuv_to_bgr(nv12), non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return pin_tensor.cuda(non_blocking=True)

    s = timed({"bgr": lambda: net.detector_input(bgr, size, "yolov5", dtype=dtype), "nv12": lambda: net.detector_input(nv12, size, "yolov5", dtype=dtype),
               "host bgr": transfers_bgr, "host nv12": transfers_nv12}, args.rounds, args.reps)
    out_bytes = 3 * size * size * esize
    say("    %s" % str(dtype))
    for name, frame_bytes in (("bgr", hf * wf * 3), ("nv12", hf * wf * 3 // 2)):
        floor = (frame_bytes + out_bytes) / HBM * 1e3
        say("        from %-5s detector_input   %s   bytes-moved floor %.4f ms (%.1f MB at 6.15 TB/s)"
            % (name, fmt(s[name]), floor, (frame_bytes + out_bytes) / 1e6))
        say("        from %-5s transfers alone  %s   device / transfers = %.3f"
            % (name, fmt(s["host " + name]), statistics.median(s[name]) / statistics.median(s["host " + name])))

say()
say("(b) detections_to_frame (conf_thres 0.3, classes [0], compact), one 1080p frame at 640, against the host round trip")
say("    (download, postproc.detections_to_frame, upload)")
geometry = pkg.postproc.letterbox_geometry((hf, wf), size, "yolov5")
for n in (8, 64, 700):
    rng = np.random.default_rng(n)
    d = np.concatenate([rng.uniform(0, size, (n, 4)), rng.uniform(0, 1, (n, 1)), rng.integers(0, 3, (n, 1))], 1).astype(np.float32)
    dev = torch.from_numpy(d).cuda()
    pin = torch.empty_like(dev, device="cpu").pin_memory()
    kw = {"conf_thres": 0.3, "classes": [0]}

    def host_call():
        pin.copy_(dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        rows, kept, _ = pkg.postproc.detections_to_frame(pin.numpy(), geometry, **kw)
        return torch.from_numpy(rows).cuda(non_blocking=True)

    got, want = net.detections_to_frame(dev, geometry, **kw), pkg.postproc.detections_to_frame(d, geometry, **kw)
    same = np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    s = timed({"device": lambda: net.detections_to_frame(dev, geometry, **kw), "host": host_call}, args.rounds, args.reps)
    say("    %3d rows (%d kept; the host form gives %s)" % (n, int(want[1][0]), "the same bits" if same else "OTHER bits"))
    say("        device call              %s" % fmt(s["device"]))
    say("        host round trip          %s   device / host = %.3f" % (fmt(s["host"]), statistics.median(s["device"]) / statistics.median(s["host"])))
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
say("Not claimed: the time of a host letterbox (cv2 is not installed where this was measured), and cv2 parity of the tensor (unpinned).")
with open(os.path.join(args.out, "letterbox.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
