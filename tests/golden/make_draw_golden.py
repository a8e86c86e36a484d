"""Records the REFERENCE's overlay of a few stored cases and how far this project's integer drawing definition
(include/hrnet_mi355.h: hrn_draw_poses; tests/draw_ref.py) is from it, pixel for pixel.  Needs opencv-python and a
checkout of the reference (whose misc/visualization.py does the drawing; nothing of it is restated here); run wherever both are:

    python tests/golden/make_draw_golden.py --reference DIR      -> tests/golden/cv2_draw_cases.npz

Per case the fixture holds the seed and size the frame and the people are drawn from (`frame`, `people` below: numpy's
generator), the overlay as cv2 drew it, and the number of pixels in which the definition's overlay differs from it.  Pixel
equality is NOT claimed by the definition (cv2.line of thickness 2 is a fixed-point polygon fill with caps of its own); the count
is the record of how close the look is.  The definition's overlay uses the reference's colours as recorded in palettes.json."""
import argparse
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import draw_ref  # noqa: E402

CASES = [(120, 160, 1, 0), (480, 640, 3, 1), (1080, 1920, 8, 2), (97, 131, 5, 3)]     # height, width, people, seed
SKELETON = json.load(open(os.path.join(HERE, "coco_skeleton.json")))["coco_skeleton"]


def frame(height, width, seed):
    return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)


def people(height, width, count, seed):
    rng = np.random.default_rng(1000 + seed)
    pts = np.empty((count, 17, 3), np.float32)
    pts[..., 0] = rng.uniform(-8, height + 8, (count, 17))
    pts[..., 1] = rng.uniform(-8, width + 8, (count, 17))
    pts[..., 2] = rng.uniform(0.2, 1.0, (count, 17))
    return pts


def palette(name, samples):
    """the reference's colours of a palette, as recorded in palettes.json"""
    for case in json.load(open(os.path.join(HERE, "palettes.json")))["cases"]:
        if (case["name"], case["samples"]) == (name, samples):
            return np.asarray(case["bgr"], np.uint8)
    raise KeyError((name, samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference: its misc/visualization.py draws the overlays")
    args = ap.parse_args()
    import cv2
    sys.path.insert(0, args.reference)
    from misc.visualization import draw_points_and_skeleton     # (imports cv2, matplotlib, torch, torchvision and ffmpeg)
    pc, bc = palette("tab20", 16), palette("Set2", 8)
    out = {"ncases": np.int64(len(CASES)), "cv2_version": np.str_(cv2.__version__)}
    for k, (h, w, count, seed) in enumerate(CASES):
        f, p = frame(h, w, seed), people(h, w, count, seed)
        theirs = f.copy()
        for i, person in enumerate(p):      # the demo's loop: everybody with the default palettes, numbered in order
            theirs = draw_points_and_skeleton(theirs, person, SKELETON, person_index=i)
        ours = draw_ref.draw_bgr(f.copy(), p, SKELETON, pc, bc)
        differing = int((ours != theirs).any(-1).sum())
        drawn = int((theirs != f).any(-1).sum())
        print("case %d: %dx%d, %d people: %d of %d drawn pixels differ" % (k, w, h, count, differing, drawn))
        out["case%d_meta" % k] = np.asarray([h, w, count, seed, zlib.crc32(f.tobytes()), differing, drawn], np.int64)
        out["case%d_out" % k] = theirs if theirs.nbytes <= 256 * 1024 else theirs[:128, :256].copy()      # (large frames: a corner)
    np.savez_compressed(os.path.join(HERE, "cv2_draw_cases.npz"), **out)


if __name__ == "__main__":
    main()
