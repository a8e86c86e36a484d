"""fp16 against bf16 on the headline shape (HRNet-W48, 384x288, one micro-batch of 256 crops), timed with HIP events and
interleaved on the same GPU: round r times bf16 then fp16 (odd rounds the other way round), so that clock and thermal drift
hit both alike.  bench.py's --dtype choices are fixed; this is where the fp16 engine's speed is measured.
usage: python tools/fp16_speed.py [--rounds R] [--reps K]   -> one JSON line"""
import argparse, importlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import costlib

pkg = importlib.import_module("simple-hrnet_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--reps", type=int, default=10, help="passes per timed sample")
args = ap.parse_args()
c, h, w, n = 48, 384, 288, 256
sd = pkg.synth_state_dict(c, 17, 0)
crops = torch.randn((n, 3, h, w), generator=torch.Generator(device="cuda").manual_seed(1234), device="cuda")
boxes = torch.from_numpy(pkg.synth_boxes(n)).cuda()
nets = {dt: pkg.NativeHRNet(c, 17, (h, w), dt, max_batch=n, device=0).load_state_dict(sd) for dt in ("bf16", "fp16")}
ms = costlib.timed({dt: (lambda net=net: net.predict_crops(crops, boxes)) for dt, net in nets.items()}, args.rounds, args.reps)
samples = {dt: [n / (v / 1e3) for v in ms[dt]] for dt in nets}   # (the warm-up: block maps, LDS attributes, clocks)
for net in nets.values():
    net.close()
med = {dt: statistics.median(v) for dt, v in samples.items()}
print(json.dumps({"shape": "W48 384x288 batch 256", "crops_per_s": {dt: round(v, 1) for dt, v in med.items()},
                  "fp16_over_bf16": round(med["fp16"] / med["bf16"], 4),
                  "spread": {dt: [round(min(v), 1), round(max(v), 1)] for dt, v in samples.items()}}))
