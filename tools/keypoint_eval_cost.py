"""COCO keypoint AP / AR on the GPU, measured: writes DIR/keypoint_eval.txt (and prints it).  No number here is a gate: what the
call costs beside the host forms is a result to record, and the call may lose (the rank kernel is O(S^2)).

  (a) NativeHRNet.keypoint_eval on device-resident inputs at 100 images x 5 detections, 5 000 x 20 and 5 000 x 20 with J = 133
      (8 people per image), against
        - the host C++ form (postproc.keypoint_eval) with the download of the detections and the upload of the statistics that a
          host evaluation of device results pays first; HIP events around the calls, host side included, interleaved, medians;
        - the numpy restatement tests/keypoint_eval_ref.py, wall clock, one run: a STAND-IN for pycocotools' COCOeval, which is
          not installed where this is measured.
  (b) each kernel's share of the device call: `rocprofv3 --kernel-trace --stats`, a traced child of its own per size.
  (c) --ab-root DIR: predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree against the checkout at DIR (the parent commit,
      built): costlib.ab, the protocol of tools/README.md.  Without --ab-root: NOT MEASURED.

usage: python tools/keypoint_eval_cost.py --out DIR [--rounds R] [--ab-root DIR] [--no-trace]
       python tools/keypoint_eval_cost.py --trace-child K       (the child of (b): size K, a few device calls)"""
import importlib
import os
import statistics
import sys
import time

import costlib
from costlib import ROOT

ap = costlib.parser(__doc__, "keypoint_eval.txt", rounds=5, ab="predict_frame", out_required=False)
ap.add_argument("--no-trace", action="store_true", help="skip (b)")
ap.add_argument("--trace-child", type=int, help="run a few device calls of size K (under rocprofv3)")
args = ap.parse_args()
if args.trace_child is None and not args.out:
    ap.error("--out is needed")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np   # noqa: E402
import torch         # noqa: E402

import keypoint_eval_cases as C   # noqa: E402
import keypoint_eval_ref as R     # noqa: E402

pkg = importlib.import_module("simple-hrnet_amd")
SIZES = ((100, 5, 17), (5000, 20, 17), (5000, 20, 133))
PEOPLE = 8
INPUTS = ("dt_kpts", "dt_scores", "gt_kpts", "gt_area", "gt_bbox", "gt_iscrowd")
KERNELS = ("keypoint_eval_match_kernel", "keypoint_eval_rank_kernel", "keypoint_eval_curve_kernel", "keypoint_eval_finish_kernel")


def build(k):
    images, dets, joints = SIZES[k]
    case = C.random_set(1000 + k, joints, counts=[(dets, PEOPLE)] * images)
    dev = {key: torch.as_tensor(v, dtype=torch.int32 if key == "gt_iscrowd" else torch.float64).cuda() if key in INPUTS else v
           for key, v in case.items()}
    return case, dev


net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # the evaluation needs no weights

if args.trace_child is not None:
    _, dev = build(args.trace_child)
    for _ in range(4):
        net.keypoint_eval(**dev)
    torch.cuda.synchronize()
    net.close()
    sys.exit(0)

report = costlib.Report(args.out, "keypoint_eval.txt", "%10.3f ms  (min %.3f .. max %.3f)")
say, fmt = report.say, report.fmt

say("COCO keypoint AP / AR -- tools/keypoint_eval_cost.py; %d samples per candidate, one call each, interleaved, HIP events, host side"
    % args.rounds)
say("included, medians.  device: %s" % torch.cuda.get_device_name(0))
for k, (images, dets, joints) in enumerate(SIZES):
    case, dev = build(k)
    pinned = {key: torch.empty_like(dev[key], device="cpu").pin_memory() for key in ("dt_kpts", "dt_scores")}

    def device_call():
        return net.keypoint_eval(**dev)

    def host_call():
        for key, pin in pinned.items():
            pin.copy_(dev[key], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        out = pkg.postproc.keypoint_eval(**dict(case, dt_kpts=pinned["dt_kpts"].numpy(), dt_scores=pinned["dt_scores"].numpy()))
        return out, torch.from_numpy(out["stats"]).cuda(non_blocking=True)

    got, want = device_call(), host_call()[0]
    same = all(np.array_equal(got[key].cpu().numpy(), want[key], equal_nan=True) for key in ("stats", "precision", "recall", "dt_match", "dt_ignore"))
    s = costlib.timed({"device": device_call, "host": host_call}, args.rounds, warmup=0)
    t0 = time.perf_counter()
    ref = R.keypoint_eval(**case)
    ref_ms = (time.perf_counter() - t0) * 1e3
    med = {key: statistics.median(v) for key, v in s.items()}
    say()
    say("(a) %d images x %d detections, %d people per image, J = %d: %d slots; AP %.4f; device == host form bit for bit: %s"
        % (images, dets, PEOPLE, joints, len(want["slot_person"]), want["stats"][0], "yes" if same else "NO"))
    say("      device call (inputs resident)                  %s" % fmt(s["device"]))
    say("      host C++ form + download / upload              %s" % fmt(s["host"]))
    say("      device / host C++ = %.3f%s" % (med["device"] / med["host"], "   (the device call LOSES)" if med["device"] > med["host"] else ""))
    say("      numpy restatement (stand-in for pycocotools; one run, wall clock) %10.1f ms; AP differs from the host form's by %.1e"
        % (ref_ms, abs(ref["stats"][0] - want["stats"][0])))
    say("      device / numpy stand-in = %.5f" % (med["device"] / ref_ms))
    if args.no_trace:
        say("(b) kernel shares: NOT MEASURED (--no-trace)")
        continue
    d = os.path.join(args.out, "keypoint_eval_trace_%d" % k)
    costlib.traced([sys.executable, os.path.abspath(__file__), "--trace-child", str(k)], d)
    found = costlib.kernel_stats(d, KERNELS)
    total = sum(v[1] for v in found.values()) or 1.0
    say("(b) kernels of one call (rocprofv3 --kernel-trace --stats, a traced run of its own; average over %d calls):"
        % (max(v[0] for v in found.values()) if found else 0))
    for name in KERNELS:
        if name in found:
            say("      %-30s %12.1f us  %5.1f %%" % (name, found[name][1] / 1e3, 100 * found[name][1] / total))
        else:
            say("      %-30s not in the trace" % name)
net.close()

say()
runs = costlib.ab(report, "(c)", ["predict"], args.ab_root, args.ab_pairs, rounds=9, reps=20)   # (the child's own sample counts)
say()
say("Not claimed: parity with pycocotools' COCOeval (not installed here; tests/golden/make_cocoeval_golden.py measures it where it is),")
say("and any AP of trained weights -- no trained weights and no images exist where this was measured.")
sys.exit(runs is None)
