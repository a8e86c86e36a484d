"""Detector NMS on the GPU, measured: writes DIR/detector_nms.txt (and prints it).  No number here is a gate: what the call costs
beside the host round trip it replaces, and beside the floor of moving the bytes its scoring pass must touch, is a result to
record -- the call may be launch-bound, and a size may lose to the round trip.

  (a) NativeHRNet.detector_nms with the head's output resident on the GPU, about 200 candidates per image in clusters of 2 - 4:
      (B, N, C) = (1, 25 200, 80) and (16, 25 200, 80) under the yolov5 rule, (1, 10 647, 80) under the yolov3 rule; against the
      round trip it replaces (download into pinned memory, postproc.detector_nms, upload of the rows); against an EMPTY launch pair
      of the same call at N = 256 with nobody passing (what two launches and the host side cost); and against the floor of moving
      the bytes the scoring pass must touch at 6.15 TB/s -- the obj column and the rows that pass (useful bytes), and the same in
      whole 128-byte lines.  HIP events around back-to-back calls, host side included, interleaved (round r runs the candidates in a
      rotated order), medians.
  (b) the two launches alone under `rocprofv3 --kernel-trace --stats`, one traced child process per size.
  (c) --ab-root DIR: predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree against the checkout at DIR (the parent commit,
      built): costlib.ab, the protocol of tools/README.md.  Without --ab-root: NOT MEASURED.

usage: python tools/detector_nms_cost.py --out DIR [--rounds R] [--reps K] [--no-trace] [--ab-root DIR]
       python tools/detector_nms_cost.py --trace-child K         (the child of (b): a few calls of size K, under rocprofv3)"""
import importlib
import os
import shutil
import statistics
import sys
import tempfile

import costlib

ap = costlib.parser(__doc__, "detector_nms.txt", rounds=9, reps=20, ab="predict_frame", out_required=False)
ap.add_argument("--no-trace", action="store_true", help="skip (b)")
ap.add_argument("--trace-child", type=int, help="run a few device calls of size K (under rocprofv3)")
args = ap.parse_args()
if args.trace_child is None and not args.out:
    ap.error("--out is needed")
sys.path.insert(0, costlib.ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

SIZES = ((1, 25200, 80, "yolov5"), (16, 25200, 80, "yolov5"), (1, 10647, 80, "yolov3"))
CANDIDATES, CONF, IOU = 200, 0.25, 0.45
KERNELS = ("dnms_score_kernel", "dnms_image_kernel")
PEAK = 6.15e12   # bytes / s, HBM


def head_output(B, N, C, passing, seed):
    """a (B, N, 5 + C) float32 head output on a 640 x 640 picture of which `passing` rows per image have obj above CONF, in clusters
    of 2 - 4 around one box and one class; everybody else has a low obj and low class scores"""
    rng = np.random.default_rng(seed)
    pred = np.empty((B, N, 5 + C), np.float32)
    pred[..., 0:2] = rng.uniform(0, 640, (B, N, 2))
    pred[..., 2:4] = rng.uniform(10, 200, (B, N, 2))
    pred[..., 4] = rng.uniform(0.0, 0.2, (B, N))
    pred[..., 5:] = rng.uniform(0.0, 0.3, (B, N, C))
    for b in range(B):
        rows = rng.permutation(N)[:passing]
        clusters = max(1, passing // 3)
        k = rng.integers(0, clusters, len(rows))
        centre, size, fav = rng.uniform(60, 580, (clusters, 2)), rng.uniform(30, 160, (clusters, 2)), rng.integers(0, C, clusters)
        pred[b, rows, 0:2] = centre[k] + rng.normal(0, 1, (len(rows), 2)) * size[k] * 0.05
        pred[b, rows, 2:4] = size[k] * rng.uniform(0.9, 1.1, (len(rows), 2))
        pred[b, rows, 4] = rng.uniform(0.55, 1.0, len(rows))
        pred[b, rows, 5 + fav[k]] = rng.uniform(0.9, 1.0, len(rows))
    return pred


pkg = importlib.import_module("simple-hrnet_amd")
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # detector NMS needs no weights

if args.trace_child is not None:
    B, N, C, rule = SIZES[args.trace_child]
    dev = torch.from_numpy(head_output(B, N, C, CANDIDATES, args.trace_child)).cuda()
    for _ in range(30):
        net.detector_nms(dev, rule, CONF, IOU)
    torch.cuda.synchronize()
    net.close()
    sys.exit(0)

report = costlib.Report(args.out, "detector_nms.txt", "%9.4f ms  (min %.4f .. max %.4f)")
say, fmt = report.say, report.fmt

say("detector NMS -- tools/detector_nms_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, host side included, medians"
    % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
say("conf_thres %.2f, iou_thres %.2f, max_det 300, max_candidates 4096; %d rows per image pass, in clusters of 2 - 4" % (CONF, IOU, CANDIDATES))
empty = torch.from_numpy(head_output(1, 256, 80, 0, 99)).cuda()
for k, (B, N, C, rule) in enumerate(SIZES):
    pred = head_output(B, N, C, CANDIDATES, k)
    dev = torch.from_numpy(pred).cuda()
    pin = torch.empty_like(dev, device="cpu").pin_memory()

    def device_call():
        return net.detector_nms(dev, rule, CONF, IOU)

    def empty_call():
        return net.detector_nms(empty, rule, CONF, IOU)

    def host_call():
        pin.copy_(dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        rows, counts, _, _ = pkg.postproc.detector_nms(pin.numpy(), rule, CONF, IOU)
        return torch.from_numpy(rows).cuda(non_blocking=True), counts

    got, want = device_call(), host_call()
    same = np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].cpu().numpy().view(np.uint32)) and \
        np.array_equal(got[1].cpu().numpy(), want[1])
    reps = args.reps if B == 1 else max(2, args.reps // 4)
    s = costlib.timed({"device": device_call, "empty": empty_call, "host": host_call}, args.rounds, reps)
    med = {key: statistics.median(v) for key, v in s.items()}
    stride = 4 * (5 + C)
    useful = B * (4 * N + CANDIDATES * (stride - 4))
    lines_touched = B * (N * min(stride, 128) + CANDIDATES * max(0, stride - 128))
    say()
    say("(a) (B, N, C) = (%d, %d, %d), %s: pred is %.1f MB; %s kept per image; device == host form bit for bit: %s"
        % (B, N, C, rule, pred.nbytes / 1e6, "%d .. %d" % (int(want[1].min()), int(want[1].max())), "yes" if same else "NO"))
    say("      device call (pred resident)                    %s" % fmt(s["device"]))
    say("      the same call on (1, 256, %d) with nobody passing %s   (two launches and the host side)" % (C, fmt(s["empty"])))
    say("      round trip: download, postproc.detector_nms, upload %s" % fmt(s["host"]))
    say("      device / round trip = %.3f%s" % (med["device"] / med["host"], "   (the device call LOSES)" if med["device"] > med["host"] else ""))
    say("      floor at 6.15 TB/s: useful bytes (obj column + the rows that pass) %.3f MB -> %.4f ms; in whole 128-byte lines %.3f MB -> %.4f ms"
        % (useful / 1e6, useful / PEAK * 1e3, lines_touched / 1e6, lines_touched / PEAK * 1e3))
    say("      device call / line floor = %.1f; (device call - empty call) / line floor = %.1f"
        % (med["device"] / (lines_touched / PEAK * 1e3), max(med["device"] - med["empty"], 0.0) / (lines_touched / PEAK * 1e3)))
    if args.no_trace or not shutil.which("rocprofv3"):
        say("(b) the two launches under rocprofv3 --kernel-trace --stats: NOT MEASURED (%s)" % ("--no-trace" if args.no_trace else "no rocprofv3"))
        continue
    d = tempfile.mkdtemp(prefix="dnms_trace_")
    costlib.traced([sys.executable, os.path.abspath(__file__), "--trace-child", str(k)], d)
    found = costlib.kernel_stats(d, KERNELS)
    shutil.rmtree(d, ignore_errors=True)
    if not found:
        say("(b) the two launches under rocprofv3 --kernel-trace --stats: NOT MEASURED (no kernel of the call in the statistics)")
        continue
    say("(b) the two launches (rocprofv3 --kernel-trace --stats, a traced run of its own; average over %d calls):" % max(v[0] for v in found.values()))
    for name in KERNELS:
        if name in found:
            extra = ""
            if name == KERNELS[0]:
                us = found[name][1] / 1e3
                extra = "   %.2f TB/s over the lines touched, %.1f x the line floor" % (lines_touched / (us * 1e-6) / 1e12, us / (lines_touched / PEAK * 1e6))
            say("      %-20s %10.1f us%s" % (name, found[name][1] / 1e3, extra))
        else:
            say("      %-20s not in the trace" % name)
net.close()

say()
runs = costlib.ab(report, "(c)", ["predict"], args.ab_root, args.ab_pairs, args.rounds, args.reps)
say()
say("Not claimed: the candidate count of a trained detector on real video -- no trained weights and no video exist where this was measured.")
sys.exit(runs is None)
