"""Writes tests/golden/cocoeval_cases.npz: random evaluation sets (tests/keypoint_eval_cases.py) and what pycocotools' COCOeval
computes for them -- precision, recall and the ten statistics for iouType 'keypoints', one category, maxDets 20.  To be run wherever
pycocotools is installed; tests/test_keypoint_eval_host.py::test_cocoeval_golden_when_present reads the file and skips without it.
Until someone has run this, parity of hrn_keypoint_eval with pycocotools is UNPINNED.

usage: python tests/golden/make_cocoeval_golden.py [--sets 12]"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import keypoint_eval_cases as C   # noqa: E402


def cocoeval(case):
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval

    images = sorted(set(case["dt_image"].tolist()) | set(case["gt_image"].tolist()))
    gt = COCO()
    gt.dataset = {"images": [{"id": int(i)} for i in images], "categories": [{"id": 1, "name": "person"}],
                  "annotations": [{"id": k + 1, "image_id": int(case["gt_image"][k]), "category_id": 1,
                                   "keypoints": case["gt_kpts"][k].reshape(-1).tolist(),
                                   "num_keypoints": int((case["gt_kpts"][k][:, 2] > 0).sum()), "area": float(case["gt_area"][k]),
                                   "bbox": case["gt_bbox"][k].tolist(), "iscrowd": int(case["gt_iscrowd"][k])}
                                  for k in range(len(case["gt_image"]))]}
    gt.createIndex()
    dt = gt.loadRes([{"image_id": int(case["dt_image"][k]), "category_id": 1, "keypoints": case["dt_kpts"][k].reshape(-1).tolist(),
                      "score": float(case["dt_scores"][k])} for k in range(len(case["dt_image"]))])
    ev = COCOeval(gt, dt, "keypoints")
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    precision = np.transpose(ev.eval["precision"][:, :, 0, :, 0], (2, 0, 1))   # [T, R, K, A, M] -> (A, T, R)
    recall = np.transpose(ev.eval["recall"][:, 0, :, 0], (1, 0))               # [T, K, A, M] -> (A, T)
    return precision, recall, np.asarray(ev.stats, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=12)
    args = ap.parse_args()
    out = {"sets": np.int64(args.sets)}
    for k in range(args.sets):
        case = C.random_set(5000 + k, 17, max_images=12)
        if len(case["dt_image"]) == 0:          # loadRes refuses an empty result list
            case = C.random_set(6000 + k, 17, max_images=12, counts=[(3, 2)])
        precision, recall, stats = cocoeval(case)
        for name in ("dt_kpts", "dt_scores", "dt_image", "gt_kpts", "gt_area", "gt_bbox", "gt_iscrowd", "gt_image"):
            out["%d_%s" % (k, name)] = case[name]
        out["%d_precision" % k], out["%d_recall" % k], out["%d_stats" % k] = precision, recall, stats
    np.savez_compressed(os.path.join(HERE, "cocoeval_cases.npz"), **out)
    print("wrote %d sets" % args.sets)


if __name__ == "__main__":
    main()
