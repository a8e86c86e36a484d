#!/usr/bin/env python3
"""Golden vectors of ``cv2.cvtColor(..., COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_I420)`` for the YUV crop pre-path and
``hrn_yuv_to_bgr`` -- to be run WHEREVER ``opencv-python`` IS INSTALLED (it is not in the build / GPU images of this repository,
which is why parity of the BT.601 limited-range table with a cv2 build is still "unpinned": tests/yuv_ref.py restates OpenCV's
published fixed-point form, nothing here could check it against a real cv2 build).

    pip install opencv-python numpy
    python tests/golden/make_yuv_golden.py                      # writes tests/golden/cv2_yuv_cases.npz

Commit the .npz: tests/test_yuv_host.py::test_restatement_against_cv2_golden consumes it when present (and skips, loudly, when
absent) -- the moment it is there, the default table (BT.601, limited range) is pinned to the real thing.  cv2 converts with
that table only; the other three tables are this project's own quantisation of the exact coefficients.

Cases: both layouts x random-byte frames (so the clips and max(0, Y - 16) are exercised) of a few small even sizes, plus one
128 x 128 frame that steps through a 64 x 64 grid of chroma pairs (0 .. 255 in both) against a luma ramp.  Frames are regenerated from seeds by ``frame`` below; their CRC32
is stored so that a consumer whose numpy draws different numbers notices instead of failing."""
import argparse
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(2, 2), (34, 50), (120, 160), (128, 128)]


def frame(h, w, seed):
    """rawvideo bytes of an h x w 4:2:0 frame, pitch = w; seed < 0: the 128 x 128 frame of the chroma grid"""
    if seed < 0:
        y = (np.arange(h * w, dtype=np.int64).reshape(h, w) * 7 % 256).astype(np.uint8)
        steps = np.rint(np.linspace(0, 255, h // 2)).astype(np.uint8)
        u, v = np.meshgrid(steps, steps, indexing="ij")
        return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])   # I420 order; the NV12 case reads it as it is
    return np.random.default_rng(seed).integers(0, 256, h * w * 3 // 2, dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "cv2_yuv_cases.npz"))
    a = ap.parse_args()
    import cv2

    arrays = {"cv2_version": np.asarray(cv2.__version__)}
    n = 0
    for k, (h, w) in enumerate(SIZES):
        for seed in ([k, -1] if (h, w) == (128, 128) else [k]):
            f = frame(h, w, seed)
            for fmt, code in (("nv12", cv2.COLOR_YUV2BGR_NV12), ("i420", cv2.COLOR_YUV2BGR_I420)):
                out = cv2.cvtColor(f.reshape(h * 3 // 2, w), code)
                arrays["case%d_meta" % n] = np.asarray([h, w, 0 if fmt == "nv12" else 1, seed, zlib.crc32(f.tobytes())], np.int64)
                arrays["case%d_out" % n] = out
                n += 1
    arrays["ncases"] = np.asarray(n)
    np.savez_compressed(a.out, **arrays)
    print("wrote %s: %d cvtColor cases, cv2 %s" % (a.out, n, cv2.__version__))


if __name__ == "__main__":
    main()
