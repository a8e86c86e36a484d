"""The detector link on the GPU, measured: writes DIR/letterbox.txt (and prints it).  No number here is a gate.

  (a) NativeHRNet.detector_input of a RESIDENT 1080p frame to 640 x 640 (style yolov5), float16 and float32, from BGR and from NV12,
      against what ANY host letterbox pays before it computes anything: the download of the frame (NV12: after yuv_to_bgr) and the
      upload of the finished tensor.  cv2 is absent here, so NO host letterbox time is claimed: the host side is a lower bound.
      Beside each timing: the bytes the call must move (frame bytes read once + tensor bytes written) at 6.15 TB/s.
  (b) NativeHRNet.detections_to_frame at 8 / 64 / 700 rows against the host round trip (download, postproc.detections_to_frame,
      upload).
  (c) --ab-root DIR: predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree against the checkout at DIR (the parent commit,
      built): costlib.ab, the protocol of tools/README.md.  Without --ab-root: NOT MEASURED.
  HIP events around back-to-back calls, host side included, interleaved (round r runs the candidates in a rotated order), medians.

usage: python tools/letterbox_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]"""
import importlib
import statistics
import sys

import costlib
from costlib import timed

args = costlib.parser(__doc__, "letterbox.txt", rounds=9, reps=20, ab="predict_frame").parse_args()
sys.path.insert(0, costlib.ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

hf, wf = 1080, 1920
HBM = 6.15e12   # bytes per second: the floor printed beside the timings
pkg = importlib.import_module("simple-hrnet_amd")
report = costlib.Report(args.out, "letterbox.txt", "%9.4f ms  (min %.4f .. max %.4f)")
say, fmt = report.say, report.fmt

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
runs = costlib.ab(report, "(c)", ["predict"], args.ab_root, args.ab_pairs, args.rounds, args.reps)
say()
say("Not claimed: the time of a host letterbox (cv2 is not installed where this was measured), and cv2 parity of the tensor (unpinned).")
sys.exit(runs is None)
