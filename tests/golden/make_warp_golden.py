#!/usr/bin/env python3
"""Golden vectors of ``cv2.warpAffine`` / ``cv2.getAffineTransform`` for the evaluation pre-path (datasets/COCO.py:290-296,
misc/utils.py:46-75, 99-107) -- to be run WHEREVER ``opencv-python`` IS INSTALLED (it is not in the build / GPU images of this
repository, which is why parity of ``hrn_warp_crops`` and ``postproc.affine_matrix`` with cv2 is still "unpinned":
tests/warp_affine_ref.py restates warpAffine's classic 8-bit INTER_LINEAR path, nothing here could check it against a real build).

    pip install opencv-python numpy
    python tests/golden/make_warp_golden.py                      # writes tests/golden/cv2_warp_cases.npz
    python tests/golden/make_warp_golden.py --reference /path/to/simple-HRNet   # additionally checks the point pairs below against
                                                                                 # the reference's get_affine_transform

Commit the .npz: tests/test_warp_host.py::test_restatement_against_cv2_warp_golden and ::test_affine_matrix_against_cv2_golden
consume it when present (and skip, loudly, when absent).  They demand BIT EQUALITY of the images and 1e-12 relative agreement
of the matrices: the restated path is integer arithmetic.  Newer OpenCV releases carry float warpAffine kernels; a build that
differs is a finding to be written down with its version (stored here), not a tolerance to be granted.

Frames are regenerated from seeds by the same function the tests use; their CRC32 is stored so that a consumer whose numpy
draws different numbers notices instead of failing.  Per case: frame (h, w, seed), center, scale, rotation, output (W, H)."""
import argparse
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# (frame h, frame w, seed), center (x, y), scale (w, h) in units of 200 px, rotation in degrees, output (W, H)
CASES = [
    ((480, 640, 1), (320.0, 240.0), (1.2, 1.6), 0.0, (96, 128)),
    ((480, 640, 2), (100.5, 400.25), (0.45, 0.6), 0.0, (96, 128)),       # magnified, partly outside
    ((480, 640, 3), (610.0, 30.0), (2.4, 3.2), 0.0, (96, 128)),          # minified, corner of the frame
    ((480, 640, 4), (320.0, 240.0), (1.2, 1.6), 30.0, (96, 128)),
    ((480, 640, 5), (200.0, 300.0), (0.9, 1.2), -80.0, (96, 128)),
    ((480, 640, 6), (-150.0, -150.0), (0.6, 0.8), 0.0, (96, 128)),       # wholly outside
    ((97, 61, 7), (30.0, 48.0), (0.3, 0.4), 12.5, (96, 128)),
    ((5, 7, 8), (3.0, 2.0), (0.03, 0.04), 0.0, (96, 128)),
    ((1080, 1920, 9), (960.0, 540.0), (3.0, 4.0), 5.0, (96, 128)),
    ((480, 640, 10), (321.7, 239.3), (1.0, 1.0), 45.0, (64, 64)),
    ((480, 640, 11), (320.0, 240.0), (0.32, 0.32), 0.0, (64, 64)),
]
PIXEL_STD = 200


def frame(h, w, seed):
    """== tests/test_resize.py::_frame: edges, texture, saturated pixels"""
    rng = np.random.default_rng(seed)
    smooth = rng.integers(0, 256, (h // 7 + 2, w // 7 + 2, 3)).astype(np.float64)
    up = np.kron(smooth, np.ones((7, 7, 1)))[:h, :w]
    return np.clip(up + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def points(center, scale, rot, output_size):
    """the three float32 point pairs get_affine_transform hands to cv2.getAffineTransform (misc/utils.py:46-68, shift = 0)"""
    scale_tmp = np.array(scale, np.float32) * 1.0 * PIXEL_STD
    src_w, dst_w, dst_h = scale_tmp[0], output_size[0], output_size[1]
    rot_rad = np.pi * rot / 180
    sn, cs = np.sin(rot_rad), np.cos(rot_rad)
    src_dir = [0 * cs - (src_w * -0.5) * sn, 0 * sn + (src_w * -0.5) * cs]
    src, dst = np.zeros((3, 2), np.float32), np.zeros((3, 2), np.float32)
    src[0, :] = np.array(center, np.float32)
    src[1, :] = np.array(center, np.float32) + src_dir
    dst[0, :] = [dst_w * 0.5, dst_h * 0.5]
    dst[1, :] = np.array([dst_w * 0.5, dst_h * 0.5]) + np.array([0, dst_w * -0.5], np.float32)
    for p in (src, dst):
        d = p[0, :] - p[1, :]
        p[2, :] = p[1, :] + np.array([-d[1], d[0]], np.float32)
    return src, dst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="checkout of stefanopini/simple-HRNet: its get_affine_transform must return the same matrices")
    ap.add_argument("--out", default=os.path.join(HERE, "cv2_warp_cases.npz"))
    a = ap.parse_args()
    import cv2

    ref = None
    if a.reference:
        sys.path.insert(0, a.reference)
        from misc.utils import get_affine_transform as ref
    arrays = {"cv2_version": np.asarray(cv2.__version__), "pixel_std": np.asarray(PIXEL_STD)}
    for n, ((h, w, seed), center, scale, rot, size) in enumerate(CASES):
        f = frame(h, w, seed)
        src, dst = points(center, scale, rot, size)
        fwd = cv2.getAffineTransform(np.float32(src), np.float32(dst))
        inv = cv2.getAffineTransform(np.float32(dst), np.float32(src))
        if ref is not None:
            c, s = np.array(center, np.float32), np.array(scale, np.float32)
            assert np.array_equal(ref(c, s, PIXEL_STD, rot, size), fwd) and np.array_equal(ref(c, s, PIXEL_STD, rot, size, inv=1), inv), n
        out = cv2.warpAffine(f, fwd, (int(size[0]), int(size[1])), flags=cv2.INTER_LINEAR)   # exactly the reference's call
        arrays["case%d_meta" % n] = np.asarray([h, w, seed, zlib.crc32(f.tobytes()), size[0], size[1]], np.int64)
        arrays["case%d_csr" % n] = np.asarray([center[0], center[1], scale[0], scale[1], rot], np.float64)
        arrays["case%d_fwd" % n], arrays["case%d_inv" % n], arrays["case%d_out" % n] = fwd, inv, out
    arrays["ncases"] = np.asarray(len(CASES))
    np.savez_compressed(a.out, **arrays)
    print("wrote %s: %d warpAffine cases, cv2 %s" % (a.out, len(CASES), cv2.__version__))


if __name__ == "__main__":
    main()
