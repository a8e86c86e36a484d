#!/usr/bin/env python3
"""Golden vectors of the detector wrappers' ``letterbox`` (cv2.resize(INTER_LINEAR) + cv2.copyMakeBorder; the reference's
``models_/detectors/YOLOv3.py:23-45`` and ``YOLOv5.py:9-39``) -- to be run WHEREVER ``opencv-python`` IS INSTALLED.  It is not in
the build / GPU images of this repository, which is why parity of ``hrn_letterbox_frames`` with cv2 is "unpinned":
``tests/letterbox_ref.py`` restates OpenCV's published 8-bit arithmetic -- the linear path of ``oracle/cv2_resize_oracle.py``, the
copy when the size does not change, and the INTER_AREA fast path cv2.resize takes when a frame is exactly twice the resized size
in both axes -- and nothing here could check that against a real cv2 build.

    pip install opencv-python numpy
    python tests/golden/make_letterbox_golden.py            # writes tests/golden/letterbox_cases.npz

The letterbox below is written from the two rules as ``include/hrnet_mi355.h`` states them, with cv2 doing the pixel work.  A
consumer compares ``case<k>_out`` with ``letterbox_ref.letterbox_u8(frame(h, w, seed), size, style, "bgr")``; frames are regenerated
from seeds and their CRC32 is stored so that a numpy that draws other numbers is noticed.  Until the file exists and a test
consumes it, the README row says cv2 parity is unpinned."""
import argparse
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# (frame h, w), size, style: the cases of tests/test_letterbox_gpu.py and the two sizes deployments run
CASES = [((48, 64), 64, "yolov3"), ((37, 53), 64, "yolov3"), ((90, 160), 64, "yolov3"), ((72, 128), 64, "yolov3"),
         ((128, 72), 64, "yolov3"), ((73, 128), 64, "yolov3"), ((3, 200), 64, "yolov3"), ((50, 100), (64, 96), "yolov5"),
         ((1080, 1920), 416, "yolov3"), ((720, 1280), 640, "yolov5"), ((1080, 1920), 640, "yolov5"), ((480, 640), 640, "yolov5")]


def frame(h, w, seed):
    """edges, texture, saturated pixels (== tests/golden/make_cv2_golden.py: frame)"""
    rng = np.random.default_rng(seed)
    smooth = rng.integers(0, 256, (h // 7 + 2, w // 7 + 2, 3)).astype(np.float64)
    up = np.kron(smooth, np.ones((7, 7, 1)))[:h, :w]
    return np.clip(up + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def letterbox(cv2, img, size, style):
    h, w = img.shape[:2]
    if style == "yolov3":
        out_h = out_w = size
        ratio = float(size) / max(h, w)
        color = (127.5, 127.5, 127.5)
    else:
        out_h, out_w = (size, size) if isinstance(size, int) else size
        ratio = min(out_h / h, out_w / w)
        color = (114, 114, 114)
    new_w, new_h = int(round(w * ratio)), int(round(h * ratio))
    dw, dh = (out_w - new_w) / 2, (out_h - new_h) / 2
    if style == "yolov3" or (w, h) != (new_w, new_h):
        img = cv2.resize(img, (new_w, new_h), interpolation=cv2.INTER_LINEAR)
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return cv2.copyMakeBorder(img, top, bottom, left, right, cv2.BORDER_CONSTANT, value=color)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "letterbox_cases.npz"))
    a = ap.parse_args()
    import cv2

    arrays = {"cv2_version": np.asarray(cv2.__version__), "ncases": np.asarray(len(CASES))}
    for k, ((h, w), size, style) in enumerate(CASES):
        f = frame(h, w, 10 * k)
        out = letterbox(cv2, f, size, style)
        if out.nbytes > 900000:   # committed files stay below 1 MiB: the large cases keep a CRC and the top-left 256 x 256 corner
            arrays["case%d_crc" % k] = np.asarray(zlib.crc32(np.ascontiguousarray(out).tobytes()))
            out = np.ascontiguousarray(out[:256, :256])
        size_hw = (size, size) if isinstance(size, int) else size
        arrays["case%d_meta" % k] = np.asarray([h, w, size_hw[0], size_hw[1], int(style == "yolov5"), 10 * k, zlib.crc32(f.tobytes())], np.int64)
        arrays["case%d_out" % k] = out
    np.savez_compressed(a.out, **arrays)
    print("wrote %s: %d letterbox cases, cv2 %s" % (a.out, len(CASES), cv2.__version__))


if __name__ == "__main__":
    main()
