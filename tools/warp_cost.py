"""Cost of the evaluation pre-path (NativeHRNet.warp_crops = hrn_warp_crops) against two yardsticks that are not the code under test:
(i) the existing multi-person pre-path, preprocess_frame, on the workload of bench.py's `prepath` block -- one 1080p uint8 frame
resident in HBM, 16 people, 384x288 crops -- timed with HIP events and interleaved (round r runs the candidates in a rotated order)
so that clock and thermal drift hit them alike; the warp does strictly less (one pass, four taps, no uint8 intermediate, no
second launch) and is expected to be no slower; (ii) the floor of writing its own output, n*3*H*W*4 bytes at the 6.0-6.3 TB/s
store rate measured on MI355X, for 256 crops in one call.  warp_crops is timed with ready-made matrices (the host then only
inverts and checks them, as preprocess_frame's C code does its box arithmetic) and, for 16 people, from centers / scales as well
(postproc.affine_matrix in numpy per person, on the host).
usage: python tools/warp_cost.py [--rounds R] [--reps K]   -> one JSON line"""
import argparse, importlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import costlib

pkg = importlib.import_module("simple-hrnet_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=20, help="calls per timed sample")
args = ap.parse_args()
h, w, hf, wf, people, many = 384, 288, 1080, 1920, 16, 256
frame = np.random.default_rng(5).integers(0, 256, (hf, wf, 3), dtype=np.uint8)   # bench.py: prepath_measure
dets = costlib.prepath_boxes(many)
cs = [pkg.postproc.box_to_center_scale((d[0], d[1], d[2] - d[0], d[3] - d[1]), w / h) for d in dets]
centers, scales = np.stack([c for c, _ in cs]), np.stack([s for _, s in cs])
mats = np.stack([pkg.postproc.affine_matrix(centers[i], scales[i], 200, 0, (w, h)) for i in range(many)])
net = pkg.NativeHRNet(32, 17, (h, w), "bf16", max_batch=32, device=0)   # the pre-paths need no weights
fdev = torch.from_numpy(frame).cuda()
cands = {
    "preprocess_frame_16": (people, lambda: net.preprocess_frame(fdev, dets[:people])),
    "warp_crops_16": (people, lambda: net.warp_crops(fdev, matrices=mats[:people])),
    "warp_crops_16_from_centers_scales": (people, lambda: net.warp_crops(fdev, centers[:people], scales[:people])),
    "warp_crops_256": (many, lambda: net.warp_crops(fdev, matrices=mats)),
}
names = list(cands)
samples = costlib.timed({k: fn for k, (_, fn) in cands.items()}, args.rounds, args.reps, warmup=5)   # (staging ring, scratch, blocks, clocks)
net.close()
med = {k: statistics.median(v) for k, v in samples.items()}
floor_ms = {k: cands[k][0] * 3 * h * w * 4 / 6.15e12 * 1e3 for k in names}   # middle of the measured 6.0-6.3 TB/s store rate
print(json.dumps({"workload": "1920x1080 uint8 frame resident in HBM, boxes of bench.py's prepath block, %dx%d crops" % (h, w),
                  "device": torch.cuda.get_device_name(0),
                  "ms_per_call": {k: round(v, 4) for k, v in med.items()},
                  "crops_per_s": {k: round(cands[k][0] / (v / 1e3), 1) for k, v in med.items()},
                  "warp_over_preprocess_16": round(med["warp_crops_16"] / med["preprocess_frame_16"], 4),
                  "store_floor_ms": {k: round(v, 4) for k, v in floor_ms.items()},
                  "time_over_store_floor": {k: round(med[k] / floor_ms[k], 2) for k in names if k.startswith("warp")},
                  "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in samples.items()}}))
