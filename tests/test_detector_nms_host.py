"""Detector NMS without a GPU: ``hrn_detector_nms`` against the numpy float32 restatement (tests/detector_nms_ref.py) bit for
bit on all four outputs -- 300 random clustered cases per rule and the designed ones -- the float64 checks of the sweep and of the
YOLOv3 merge, float16 input, every refusal (on a plan-only handle as well), the declarations."""
import functools
import os

import numpy as np
import pytest

from conftest import load_pkg
from detector_nms_ref import RULES, designed_cases, detector_nms_ref, greedy_f64, random_cases, random_pred

NEW = {"hrn_detector_nms", "hrn_detector_nms_last_error", "hrn_detector_nms_dev"}
SEEDS = {"yolov3": 20261, "yolov5": 20262}
OUTPUTS = ("rows", "counts", "index", "status")


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    assert len(bad) == 0, "%s: %d words differ, first at %d: %r != %r" % (what, len(bad), bad[0], got.reshape(-1)[bad[0]],
                                                                          want.reshape(-1)[bad[0]])


def same_outputs(got, want, what=""):
    for name, g, w in zip(OUTPUTS, got, want):
        same_bits(g, w, "%s %s" % (what, name))


@functools.lru_cache(maxsize=None)
def cases_of(rule):
    """the 300 random cases of a rule with the restatement's results and details, computed once"""
    out = []
    for pred, conf, iou, agnostic in random_cases(SEEDS[rule]):
        details = []
        want = detector_nms_ref(pred, rule, conf, iou, agnostic=agnostic, details=details)
        out.append((pred, conf, iou, agnostic, want, details))
    return out


def test_symbols_and_sources():
    lib = load_pkg("_lib")
    assert NEW <= set(lib.header_symbols()) and NEW <= set(lib.SYMBOLS)
    assert set(lib.header_symbols()) == set(lib.SYMBOLS)
    assert "detector_nms.hip" in lib.SOURCES
    for f in ("detector_nms.hip", "postproc.cpp", "hrnet_mi355.cpp"):   # one text for the host and the device
        assert '#include "detector_nms_math.h"' in open(os.path.join(lib.CSRC, f)).read(), f
    header = open(os.path.join(lib.INCLUDE, "hrnet_mi355.h")).read()
    assert "HRN_DNMS_YOLOV3 = 0, HRN_DNMS_YOLOV5 = 1" in header and "HRN_DNMS_AGNOSTIC = 1" in header
    pkg, P = load_pkg(), load_pkg("postproc")
    assert hasattr(P, "detector_nms") and hasattr(pkg.NativeHRNet, "detector_nms")
    assert P.DETECTOR_NMS_RULES == {"yolov3": 0, "yolov5": 1}


@pytest.mark.parametrize("rule", RULES)
def test_random_cases_equal_the_restatement_bit_for_bit(rule):
    P = load_pkg("postproc")
    candidates = suppressed = 0
    shapes = set()
    for i, (pred, conf, iou, agnostic, want, details) in enumerate(cases_of(rule)):
        same_outputs(P.detector_nms(pred, rule, conf, iou, agnostic=agnostic), want, "%s case %d" % (rule, i))
        shapes.add((pred.shape[0], pred.shape[2] - 5, agnostic))
        for d in details:
            candidates += len(d["rows"])
            suppressed += len(d["rows"]) - len(d["kept"])
    assert len(shapes) == 3 * 3 * 2, shapes                   # B in 1..3, C in {1, 2, 80}, both agnostic values
    share = suppressed / candidates
    print("%s: %d candidates, %.3f suppressed" % (rule, candidates, share))
    assert 1 / 3 <= share <= 2 / 3, share


@pytest.mark.parametrize("rule", RULES)
def test_cases_off_the_coordinate_grid_and_small_limits(rule):
    """what the 300 cases leave out: coordinates that are not on the 1/64 grid (every difference rounds), max_det and
    max_candidates below the counts, float keys that repeat"""
    P = load_pkg("postproc")
    rng = np.random.default_rng(77)
    for i in range(40):
        B, N, C = int(rng.integers(1, 4)), int(rng.integers(1, 400)), int(rng.choice([1, 3, 80]))
        pred = random_pred(rng, B, N, C)
        pred[..., :4] = (pred[..., :4] * rng.uniform(0.9, 1.1, pred[..., :4].shape)).astype(np.float32)
        if i % 3 == 0:
            pred[..., 4] = np.round(pred[..., 4] * 8) / 8          # few distinct keys: the stable order decides
            pred[..., 5:] = np.where(pred[..., 5:] > 0.5, 1.0, pred[..., 5:])
        kw = dict(max_det=int(rng.choice([1, 7, 300])), max_candidates=int(rng.choice([7, 64, 4096])), agnostic=bool(i & 1))
        kw["max_det"] = min(kw["max_det"], kw["max_candidates"])
        same_outputs(P.detector_nms(pred, rule, 0.25, 0.45, **kw), detector_nms_ref(pred, rule, 0.25, 0.45, **kw), "%s case %d" % (rule, i))


def test_yolov5_kept_index_equals_a_float64_greedy_nms():
    """the kept rows of the 300 random cases against a plain float64 greedy NMS over the same ordered candidates.  Cases in which
    some IoU lies within 1e-6 of iou_thres are left out; they must stay under 5 % (the seed is chosen so that they do)."""
    P = load_pkg("postproc")
    left_out = 0
    cases = cases_of("yolov5")
    for i, (pred, conf, iou, agnostic, _, details) in enumerate(cases):
        rows, counts, index, _ = P.detector_nms(pred, "yolov5", conf, iou, agnostic=agnostic)
        close = False
        want = []
        for b, d in enumerate(details):
            kept, margin = greedy_f64(d["boxes"], d["best"], np.float32(iou), 300, agnostic)
            close |= margin <= 1e-6
            want.append(d["rows"][kept])
        if close:
            left_out += 1
            continue
        for b, w in enumerate(want):
            assert counts[b] == len(w) and np.array_equal(index[b, :len(w)], w), (i, b)
    print("left out: %d of %d" % (left_out, len(cases)))
    assert left_out < 0.05 * len(cases), left_out


def test_yolov3_merge_against_float64():
    """the YOLOv3 rule against a float64 evaluation of the same definition: the kept set and its order are equal, every merged
    coordinate lies within the float32 summation bound (m + 2) * 2^-24 * sum|w_j x_j| / |sum w_j| of a merge set of m rows"""
    P = load_pkg("postproc")
    merged = 0
    for i, (pred, conf, iou, agnostic, _, details) in enumerate(cases_of("yolov3")):
        rows, counts, index, _ = P.detector_nms(pred, "yolov3", conf, iou, agnostic=agnostic)
        for b, d in enumerate(details):
            kept, _ = greedy_f64(d["boxes"], d["best"], np.float32(iou), 300, agnostic, pixel=True)
            assert counts[b] == len(kept) and np.array_equal(index[b, :len(kept)], d["rows"][kept]), (i, b)
            boxes, w = d["boxes"].astype(np.float64), d["obj"].astype(np.float64)
            alive = np.ones(len(boxes), bool)
            for slot, pos in enumerate(kept):       # the merge sets again, in float64: who was alive and is suppressed by pos
                alive[pos] = False
                members = [pos]
                for q in np.flatnonzero(alive[pos + 1:]) + pos + 1:
                    if not agnostic and d["best"][q] != d["best"][pos]:
                        continue
                    iw = max(min(boxes[pos, 2], boxes[q, 2]) - max(boxes[pos, 0], boxes[q, 0]) + 1, 0)
                    ih = max(min(boxes[pos, 3], boxes[q, 3]) - max(boxes[pos, 1], boxes[q, 1]) + 1, 0)
                    area = lambda k: (boxes[k, 2] - boxes[k, 0] + 1) * (boxes[k, 3] - boxes[k, 1] + 1)   # noqa: E731
                    if iw * ih / (area(pos) + area(q) - iw * ih + 1e-16) > float(np.float32(iou)):
                        alive[q] = False
                        members.append(int(q))
                m = len(members)
                merged += m > 1
                want = (w[members, None] * boxes[members]).sum(0) / w[members].sum()
                bound = (m + 2) * 2.0 ** -24 * np.abs(w[members, None] * boxes[members]).sum(0) / abs(w[members].sum())
                assert np.all(np.abs(rows[b, slot, :4].astype(np.float64) - want) <= bound), (i, b, slot, rows[b, slot, :4], want, bound)
    assert merged > 1000, merged


def run_designed(name):
    P = load_pkg("postproc")
    pred, rule, conf, iou, max_det, max_candidates, agnostic = designed_cases()[name]
    got = P.detector_nms(pred, rule, conf, iou, max_det=max_det, max_candidates=max_candidates, agnostic=agnostic)
    same_outputs(got, detector_nms_ref(pred, rule, conf, iou, max_det, max_candidates, agnostic), name)
    return got


@pytest.mark.parametrize("name", sorted(designed_cases()))
def test_designed_cases_equal_the_restatement_bit_for_bit(name):
    rows, counts, index, status = run_designed(name)
    assert rows.shape[:2] == index.shape and np.all(index[np.arange(index.shape[1])[None] >= counts[:, None]] == -1)
    assert not rows[np.arange(index.shape[1])[None] >= counts[:, None]].view(np.uint32).any()   # +0.0, not -0.0


@pytest.mark.parametrize("rule", RULES)
def test_what_the_designed_cases_must_give(rule):
    rows, counts, index, status = run_designed("equal_keys_" + rule)
    # all keys are 0.25: the order is the row order; row 5 overlaps row 4 and goes, row 6 overlaps row 4 too
    assert counts[0] == 5 and index[0, :5].tolist() == [0, 1, 2, 3, 4] and status[0] == 0
    rows, counts, index, status = run_designed("obj_at_threshold_" + rule)
    assert index[0, :counts[0]].tolist() == ([1, 0] if rule == "yolov3" else [1])
    rows, counts, index, status = run_designed("iou_at_threshold_" + rule)
    assert index[0, :counts[0]].tolist() == [0, 1, 2]          # IoU == iou_thres does not suppress; the pair above it does
    rows, counts, index, status = run_designed("cut_ties_" + rule)
    # 10 keys of 0.9, then six of 0.5 of which three take part: the lowest rows (1, 4, 7 hold the first three of them)
    assert status[0] == 1 and counts[0] == 13
    assert sorted(index[0, :13].tolist()) == sorted([2, 5, 8, 11, 14, 17, 19, 21, 22, 23] + [1, 4, 7])
    assert index[0, 10:13].tolist() == [1, 4, 7]
    rows, counts, index, status = run_designed("max_det_survivors_" + rule)
    assert counts[0] == 4 and status[0] == 2 and index[0].tolist() == [0, 1, 2, 3]
    rows, counts, index, status = run_designed("max_det_exact_" + rule)
    assert counts[0] == 4 and status[0] == 0                   # the fifth row is suppressed by row 0: nobody is left
    rows, counts, index, status = run_designed("two_classes_" + rule)
    assert index[0, :counts[0]].tolist() == [0, 1]
    rows, counts, index, status = run_designed("two_classes_agnostic_" + rule)
    assert index[0, :counts[0]].tolist() == [0]
    rows, counts, index, status = run_designed("no_rows_" + rule)
    assert counts.tolist() == [0, 0] and status.tolist() == [0, 0] and rows.shape == (2, 300, 7 if rule == "yolov3" else 6)
    rows, counts, index, status = run_designed("no_images_" + rule)
    assert rows.shape[0] == 0 and counts.shape == (0,)
    rows, counts, index, status = run_designed("nonfinite_" + rule)
    assert bool(status[0] & 4) == (rule == "yolov3")           # a NaN key can only qualify under yolov3 (NaN > t is false)
    rows, counts, index, status = run_designed("zero_area_" + rule)
    if rule == "yolov5":   # 0 / 0 between the two points is NaN: both stay; the line has no area in common with anybody
        assert index[0, :counts[0]].tolist() == [0, 1, 2, 3]
    if rule == "yolov3":   # the merged box of row 0 (with row 4, suppressed by it) is the weighted mean
        rows, counts, index, status = run_designed("max_det_exact_" + rule)
        w0, w4 = np.float32(0.9), np.float32(0.5)
        want = (w0 * np.float32(25) + w4 * np.float32(25)) / (w0 + w4)
        assert rows[0, 0, 0] == want and rows[0, 0, 4] == w0 and rows[0, 0, 5] == 1 and rows[0, 0, 6] == 0


@pytest.mark.parametrize("rule", RULES)
def test_float16_input_equals_float32_input_of_the_converted_values(rule):
    P = load_pkg("postproc")
    rng = np.random.default_rng(5)
    pred = random_pred(rng, 2, 300, 3).astype(np.float16)
    # row 0: subnormals and the largest number in the box, obj 1, classes -inf, NaN, -0: best is the -0, the key is -0
    pred[0, 0] = np.array([0x0001, 0x03FF, 0x0400, 0x7BFF, 0x3C00, 0xFC00, 0x7E00, 0x8000], np.uint16).view(np.float16)
    same_outputs(P.detector_nms(pred, rule, 0.25, 0.45), P.detector_nms(pred.astype(np.float32), rule, 0.25, 0.45), rule)
    same_outputs(P.detector_nms(pred, rule, 0.25, 0.45), detector_nms_ref(pred, rule, 0.25, 0.45), rule)


def test_every_float16_value_widens_exactly():
    """all 65 536 bit patterns as the class score of a row with obj = 1, 4096 at a time (iou_thres = 1: nobody is suppressed); the
    NaNs are dropped, every other value comes back in column 5 as numpy widens it"""
    P = load_pkg("postproc")
    every = np.arange(65536, dtype=np.uint16).view(np.float16)
    wide, seen = every.astype(np.float32), 0
    for first in range(0, 65536, 4096):
        probe = np.zeros((1, 4096, 6), np.float16)
        probe[0, :, 4], probe[0, :, 5] = 1.0, every[first:first + 4096]
        rows, counts, index, status = P.detector_nms(probe, "yolov3", 1.0, 1.0, max_det=4096, max_candidates=4096)
        got, src = rows[0, :counts[0], 5], first + index[0, :counts[0]]
        assert np.array_equal(got.view(np.uint32), wide[src].view(np.uint32))
        assert counts[0] == np.count_nonzero(~np.isnan(wide[first:first + 4096])) and bool(status[0] & 4) == bool(np.isnan(wide[first:first + 4096]).any())
        seen += int(counts[0])
    assert seen == 65536 - 2046


REFUSALS = [
    (dict(dtype=1), "dtype must be HRN_F32 or HRN_F16"), (dict(B=-1), "B is negative"), (dict(N=-1), "N must be in [0, 2^24]"),
    (dict(N=(1 << 24) + 1), "N must be in [0, 2^24]"), (dict(C=0), "C must be in [1, 4096]"), (dict(C=4097), "C must be in [1, 4096]"),
    (dict(rule=2), "rule must be"), (dict(rule=-1), "rule must be"), (dict(flags=2), "unknown flag bits"),
    (dict(conf_thres=float("nan")), "must be finite"), (dict(conf_thres=float("inf")), "must be finite"),
    (dict(iou_thres=float("nan")), "must be finite"), (dict(iou_thres=float("-inf")), "must be finite"),
    (dict(max_candidates=0), "max_candidates must be in [1, 4096]"), (dict(max_candidates=4097), "max_candidates must be in [1, 4096]"),
    (dict(max_det=0), "max_det must be in [1, max_candidates]"), (dict(max_det=65, max_candidates=64), "max_det must be in [1, max_candidates]"),
    (dict(rows=None), "null rows / index / counts / status"), (dict(index=None), "null rows"), (dict(counts=None), "null rows"),
    (dict(status=None), "null rows"), (dict(pred=None), "null pred"),
]


def raw_call(fn, extra, change, last_error):
    """one raw call of either entry with good arguments but for `change`; the outputs are pre-filled with a sentinel"""
    B, N, C, max_det = 2, 40, 3, 8
    pred = random_pred(np.random.default_rng(1), B, N, C)
    bufs = dict(rows=np.full((B, max_det, 7), -7.5, np.float32), index=np.full((B, max_det), -77, np.int32),
                counts=np.full((B,), -77, np.int32), status=np.full((B,), -77, np.int32))
    a = dict(pred=pred, dtype=0, B=B, N=N, C=C, rule=0, flags=0, conf_thres=0.25, iou_thres=0.5, max_candidates=64, max_det=max_det, **bufs)
    a.update(change)
    ptr = lambda v: None if v is None else v.ctypes.data   # noqa: E731
    rc = fn(*extra[:1], ptr(a["pred"]), a["dtype"], a["B"], a["N"], a["C"], a["rule"], a["flags"], a["conf_thres"], a["iou_thres"],
            a["max_candidates"], a["max_det"], ptr(a["rows"]), ptr(a["index"]), ptr(a["counts"]), ptr(a["status"]), *extra[1:])
    untouched = (bufs["rows"] == -7.5).all() and all((bufs[k] == -77).all() for k in ("index", "counts", "status"))
    return rc, last_error().decode(), untouched


def test_every_refusal_is_code_7_with_its_message_and_writes_nothing():
    L = load_pkg("_lib").load()
    for change, text in REFUSALS:
        rc, err, untouched = raw_call(L.hrn_detector_nms, (), change, L.hrn_detector_nms_last_error)
        assert rc == 7 and text in err and untouched, (change, rc, err)
    rc, _, untouched = raw_call(L.hrn_detector_nms, (), {}, L.hrn_detector_nms_last_error)
    assert rc == 0 and not untouched
    # B == 0 needs no pointers at all; N == 0 needs no pred
    assert L.hrn_detector_nms(None, 0, 0, 5, 3, 0, 0, 0.25, 0.5, 64, 8, None, None, None, None) == 0
    rc, _, untouched = raw_call(L.hrn_detector_nms, (), dict(pred=None, N=0), L.hrn_detector_nms_last_error)
    assert rc == 0 and not untouched
    P = load_pkg("postproc")
    with pytest.raises(ValueError, match="max_det must be in"):
        P.detector_nms(np.zeros((1, 4, 6), np.float32), "yolov5", 0.25, 0.5, max_det=0)
    with pytest.raises(ValueError, match="rule must be"):
        P.detector_nms(np.zeros((1, 4, 6), np.float32), "yolov4", 0.25, 0.5)
    with pytest.raises(ValueError, match=r"\(B, N, 5 \+ C\)"):
        P.detector_nms(np.zeros((4, 6), np.float32), "yolov5", 0.25, 0.5)


def test_device_entry_refusals_need_no_gpu():
    """a plan-only handle (device = -1): every argument error is reported as such, before 'plan-only'; a good call as 'plan-only';
    nothing is written either way"""
    pkg = load_pkg()
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h
    last = lambda: L.hrn_last_error(h)   # noqa: E731
    for change, text in REFUSALS:
        rc, err, untouched = raw_call(L.hrn_detector_nms_dev, (h, None), change, last)
        assert rc == 7 and err.startswith("hrn_detector_nms_dev: ") and text in err and "plan-only" not in err and untouched, (change, err)
    for change in ({}, dict(B=0), dict(N=0, pred=None)):
        rc, err, untouched = raw_call(L.hrn_detector_nms_dev, (h, None), change, last)
        assert rc == 7 and "plan-only" in err and untouched, (change, err)
    assert L.hrn_detector_nms_dev(None, None, 0, 0, 5, 3, 0, 0, 0.25, 0.5, 64, 8, None, None, None, None, None) == 1


def test_simple_hrnet_judges_a_raw_detector_before_it_builds_an_engine():
    pkg = load_pkg()

    class Raw:
        size, style, classes = 64, "yolov5", None
        conf_thres, nms_thres = 0.25, 0.45

        def predict_raw(self, x):
            raise AssertionError("not reached")

    def build(**change):
        d = Raw()
        for k, v in change.items():
            setattr(d, k, v)
        return pkg.SimpleHRNet(32, 17, {}, resolution=(64, 64), device="cuda:0", device_detector=d)

    for change, text in ((dict(conf_thres=None), "positive conf_thres"), (dict(conf_thres=0.0), "positive conf_thres"),
                         (dict(conf_thres=-0.5), "positive conf_thres"), (dict(conf_thres=float("nan")), "positive conf_thres"),
                         (dict(nms_thres=None), "needs nms_thres")):
        with pytest.raises(ValueError, match=text):
            build(**change)
    with pytest.raises(ValueError, match="predict_tensor\\(x\\) or predict_raw\\(x\\)"):
        pkg.SimpleHRNet(32, 17, {}, resolution=(64, 64), device="cuda:0", device_detector=object())
