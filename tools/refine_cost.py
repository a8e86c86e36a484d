"""Cost of the opt-in sub-pixel decoding on the headline shape (HRNet-W48, 384x288, one micro-batch of 256 crops, bf16): one
engine, predict_crops with refine=None, "quarter" and "dark", timed with HIP events and interleaved (round r runs the three modes
in a rotated order) so that clock and thermal drift hit them alike.  A refined pass makes the head write the 256 x 17 heat-maps
(into the handle's scratch) and the decode read a window of each; refine=None is hrn_forward as it is.
usage: python tools/refine_cost.py [--rounds R] [--reps K]   -> one JSON line"""
import argparse, importlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import costlib

pkg = importlib.import_module("simple-hrnet_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=10, help="passes per timed sample")
args = ap.parse_args()
c, h, w, n = 48, 384, 288, 256
crops = torch.randn((n, 3, h, w), generator=torch.Generator(device="cuda").manual_seed(1234), device="cuda")
boxes = torch.from_numpy(pkg.synth_boxes(n)).cuda()
net = pkg.NativeHRNet(c, 17, (h, w), "bf16", max_batch=n, device=0).load_state_dict(pkg.synth_state_dict(c, 17, 0))
samples = costlib.timed({str(mode): (lambda mode=mode: net.predict_crops(crops, boxes, refine=mode)) for mode in (None, "quarter", "dark")},
                        args.rounds, args.reps)   # (the warm-up: block maps, the scratch heat-map buffer, clocks)
net.close()
med = {m: statistics.median(v) for m, v in samples.items()}
print(json.dumps({"shape": "W48 384x288 batch 256 bf16", "ms_per_pass": {m: round(v, 4) for m, v in med.items()},
                  "crops_per_s": {m: round(n / (v / 1e3), 1) for m, v in med.items()},
                  "cost_over_none": {m: round(med[m] / med["None"] - 1.0, 5) for m in ("quarter", "dark")},
                  "spread_ms": {m: [round(min(v), 4), round(max(v), 4)] for m, v in samples.items()}}))
