#!/usr/bin/env python3
"""Store the key order and tensor shapes of the REFERENCE's own ``state_dict()`` for the models the tests pin
``synth.hrnet_state_spec`` / ``synth.poseresnet_state_spec`` to (tests/test_synth.py, tests/test_poseresnet.py).

    python tests/golden/make_state_spec_golden.py --reference <simple-HRNet checkout>

The unmodified ``models_.hrnet.HRNet`` (hrnet.py:74-189) and ``models_.poseresnet.PoseResNet`` (poseresnet.py:16-122)
are built with random init; only the names and shapes of their state dicts are kept (no values), so the tests run
without the reference.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_state_specs.npz")
MODELS = [("HRNet", 32), ("HRNet", 48), ("PoseResNet", 50), ("PoseResNet", 101)]


def shape_str(shape) -> str:
    return "x".join(str(int(d)) for d in shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of stefanopini/simple-HRNet")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    from models_.hrnet import HRNet
    from models_.poseresnet import PoseResNet

    arrays = {}
    for name, size in MODELS:
        sd = (HRNet if name == "HRNet" else PoseResNet)(size, 17).state_dict()
        tag = "%s_%d" % (name, size)
        arrays[tag + "_keys"] = np.asarray(list(sd.keys()))
        arrays[tag + "_shapes"] = np.asarray([shape_str(v.shape) for v in sd.values()])
        print("%s: %d entries" % (tag, len(sd)))
    np.savez_compressed(a.out, **arrays)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
