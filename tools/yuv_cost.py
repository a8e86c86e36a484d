"""NV12 input against BGR input, measured: writes DIR/yuv_input.txt (and prints it).  No number here is a gate: whether YUV
input is faster or slower than BGR input per call is a result to record.

  (a) preprocess_frame, 16 people of one 1080p frame at 384x288 (the boxes of bench.py's `prepath` block), the frame resident
      in HBM: from NV12 and from BGR.  HIP events, interleaved (round r runs the candidates in a rotated order), medians.
  (b) yuv_to_bgr of a 1080p NV12 frame against the floor of moving its 3.1 MB in and 6.2 MB out at 6.15 TB/s (the middle of the
      6.0-6.3 TB/s measured on MI355X, as in tools/warp_cost.py).
  (c) a 30-frame 1080p clip, 8 people per frame (bench.make_clip), through predict_clip from pinned host memory to joints on the
      host: host NV12 frames and host BGR frames, with the bytes each uploads.  Engine: bench.py's flagship (HRNet-W48, 384x288,
      bf16, max_batch 256, synthetic weights); wall clock, interleaved, medians.
  (d) the host alternative: the numpy restatement (tests/yuv_ref.py) of one 1080p NV12 -> BGR conversion, single thread of
      numpy -- NOT cv2, which is not installed where this runs.
  (e) --ab-root DIR: BGR preprocess_frame of (a) in THIS tree against the same call in the checkout at DIR (the parent commit,
      built): costlib.ab, the protocol of tools/README.md.  Without --ab-root the pair is reported as NOT MEASURED.

usage: python tools/yuv_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR] [--skip-clip]"""
import importlib
import os
import statistics
import sys
import time

import costlib
from costlib import ROOT

ap = costlib.parser(__doc__, "yuv_input.txt", rounds=9, reps=20, ab="BGR preprocess_frame")
ap.add_argument("--skip-clip", action="store_true", help="leave (c) out (reported as NOT MEASURED)")
args = ap.parse_args()
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
import numpy as np   # noqa: E402
import torch         # noqa: E402

import yuv_ref       # noqa: E402

import bench         # noqa: E402  (make_clip)

h, w, hf, wf, people = 384, 288, 1080, 1920, 16
FLOOR_RATE = 6.15e12
pkg = importlib.import_module("simple-hrnet_amd")
dets16 = costlib.prepath_boxes(people)
report = costlib.Report(args.out, "yuv_input.txt")
say, fmt = report.say, report.fmt

say("YUV (NV12 / I420) input -- tools/yuv_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, medians" % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
rng = np.random.default_rng(6)
nv12_host = rng.integers(0, 256, hf * wf * 3 // 2, dtype=np.uint8)
yuv_dev = pkg.YuvFrame(nv12_host, hf, wf, "nv12").to("cuda:0")
net = pkg.NativeHRNet(32, 17, (h, w), "bf16", max_batch=32, device=0)
bgr_dev = net.yuv_to_bgr(yuv_dev)                      # the same picture on both sides
same = torch.equal(net.preprocess_frame(yuv_dev, dets16)[0], net.preprocess_frame(bgr_dev, dets16)[0])
s = costlib.timed({"nv12": lambda: net.preprocess_frame(yuv_dev, dets16), "bgr": lambda: net.preprocess_frame(bgr_dev, dets16),
                   "to_bgr": lambda: net.yuv_to_bgr(yuv_dev)}, args.rounds, args.reps, warmup=5)
net.close()
say()
say("(a) preprocess_frame, %d people of a %dx%d frame resident in HBM, %dx%d crops (crops equal bit for bit: %s)"
    % (people, wf, hf, h, w, "yes" if same else "NO"))
say("    from NV12  %s" % fmt(s["nv12"]))
say("    from BGR   %s" % fmt(s["bgr"]))
say("    NV12 / BGR = %.3f" % (statistics.median(s["nv12"]) / statistics.median(s["bgr"])))
floor_ms = (hf * wf * 3 // 2 + hf * wf * 3) / FLOOR_RATE * 1e3
say()
say("(b) yuv_to_bgr of a %dx%d NV12 frame: %.1f MB in, %.1f MB out" % (wf, hf, hf * wf * 1.5 / 1e6, hf * wf * 3 / 1e6))
say("    measured   %s   (includes the call's host side and the allocation of the output tensor)" % fmt(s["to_bgr"]))
say("    floor      %8.4f ms  at %.2f TB/s; measured / floor = %.1f" % (floor_ms, FLOOR_RATE / 1e12, statistics.median(s["to_bgr"]) / floor_ms))

say()
if args.skip_clip:
    say("(c) 30-frame clip through predict_clip, host NV12 against host BGR: NOT MEASURED (--skip-clip)")
else:
    nf = 30
    _, dets = bench.make_clip(frames=nf)
    eng = pkg.NativeHRNet(48, 17, (384, 288), "bf16", max_batch=256, device=0).load_state_dict(pkg.synth_state_dict(48, 17, 0))
    conv = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)
    crng = np.random.default_rng(7)
    yuv_items, bgr_items = [], []
    for f in range(nf):                              # the same pictures on both sides: random NV12 and its BGR conversion
        raw = torch.from_numpy(crng.integers(0, 256, hf * wf * 3 // 2, dtype=np.uint8)).pin_memory()
        yf = pkg.YuvFrame(raw, hf, wf, "nv12")
        yuv_items.append((yf, dets[f]))
        bgr_items.append((conv.yuv_to_bgr(yf).cpu().pin_memory(), dets[f]))
    conv.close()

    def run(items):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = list(eng.predict_clip(iter(items), people_per_pass=64, variant="clamp"))
        host = torch.cat([r[1] for r in res]).cpu().numpy()
        torch.cuda.synchronize()
        return host, time.perf_counter() - t0

    arms = {"nv12": lambda: run(yuv_items), "bgr": lambda: run(bgr_items)}
    ref = {k: arms[k]()[0] for k in arms}            # warm-up, and the joints of both sides
    secs = {k: [] for k in arms}
    names = list(arms)
    for r in range(max(args.rounds, 9)):
        for k in names[r % 2:] + names[:r % 2]:
            secs[k].append(arms[k]()[1])
    eng.close()
    say("(c) %d frames %dx%d x %d people through predict_clip (people_per_pass 64), pinned host frames -> joints on the host;"
        % (nf, wf, hf, dets.shape[1]))
    say("    HRNet-W48 384x288 bf16, max_batch 256, synthetic weights; wall clock, %d repetitions, interleaved (joints equal: %s)"
        % (len(secs["bgr"]), "yes" if np.array_equal(ref["nv12"], ref["bgr"]) else "NO"))
    for k, label, nbytes in (("nv12", "host NV12", hf * wf * 3 // 2), ("bgr", "host BGR ", hf * wf * 3)):
        ms = sorted(1e3 * v for v in secs[k])
        say("    %s  %8.2f ms  (min %.2f .. max %.2f)  %6.1f FPS   uploads %.1f MB per clip"
            % (label, statistics.median(ms), ms[0], ms[-1], nf / (statistics.median(ms) / 1e3), nf * nbytes / 1e6))
    say("    NV12 / BGR = %.3f" % (statistics.median(secs["nv12"]) / statistics.median(secs["bgr"])))

say()
t = []
for _ in range(5):
    t0 = time.perf_counter()
    yuv_ref.yuv_to_bgr(nv12_host, hf, wf, "nv12")
    t.append(1e3 * (time.perf_counter() - t0))
say("(d) the host alternative, NUMPY (tests/yuv_ref.py, not cv2): one %dx%d NV12 -> BGR conversion" % (wf, hf))
say("    %8.2f ms  (min %.2f .. max %.2f of 5)" % (statistics.median(t), min(t), max(t)))

say()
sys.exit(costlib.ab(report, "(e)", ["prepath_bgr"], args.ab_root, args.ab_pairs, args.rounds, args.reps) is None)
