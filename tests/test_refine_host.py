"""Sub-pixel joint decoding (include/hrnet_mi355.h: HRN_REFINE_*) without a GPU: the numpy restatement (tests/subpixel_ref.py)
against the reference's own quarter-pixel step and against Gaussian maps of known centre, the kernel's build, and the
argument checks of the C ABI and the Python options."""
import ctypes
import os

import numpy as np
import pytest

import subpixel_ref as R
from conftest import golden, load_pkg
from test_build_invariants import _resource_usage


def test_quarter_restatement_reproduces_get_final_preds():
    """tests/golden/w32_128x96_fliptta_n3.npz holds the reference's get_final_preds output on its averaged maps"""
    g = golden("w32_128x96_fliptta_n3")
    got = R.refine_coords(g["heatmaps"], g["preds_nopost"], "quarter")
    np.testing.assert_array_equal(got, g["preds"])
    assert np.abs(got - g["preds_nopost"]).max() == 0.25


@pytest.mark.parametrize("h,w", [(96, 72), (64, 48), (32, 24)])
def test_dark_restatement_recovers_gaussian_centres(h, w):
    maps, cx, cy = R.gaussian_maps(200, h, w, np.random.default_rng([h, w]))
    err = []
    for m, x0, y0 in zip(maps, cx, cy):
        px, py, _ = R.argmax_xy(m)
        ox, oy = R.dark_offset(m, px, py)
        err.append(max(abs(px + ox - x0), abs(py + oy - y0)))
    print("\n%dx%d: worst |error| %.2e cell over %d maps" % (h, w, max(err), len(err)))
    assert max(err) < 1e-3


def test_dark_offset_only_inside_the_interior():
    maps, _, _ = R.gaussian_maps(1, 32, 24, np.random.default_rng(0))
    m = maps[0]
    h, w = m.shape
    for px, py in ((1, 10), (w - 2, 10), (10, 1), (10, h - 2), (0, 0), (w - 1, h - 1)):
        assert R.dark_offset(m, px, py) == (0.0, 0.0)
        assert R.dark_terms(m, px, py) is None
    assert R.dark_terms(m, 2, 2) is not None and R.dark_terms(m, w - 3, h - 3) is not None
    # quarter: 1 < px < w-1
    assert R.quarter_offset(m, 1, 10) == (0.0, 0.0) and R.quarter_offset(m, 10, h - 1) == (0.0, 0.0)


def test_dark_no_offset_for_flat_non_concave_and_non_positive_maps():
    h, w = 32, 24
    flat = np.full((h, w), 0.3, np.float32)
    assert R.dark_offset(flat, 12, 16) == (0.0, 0.0)
    # a bowl (L convex) and a saddle (det < 0)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    bowl = (1.0 + 0.01 * ((xs - 12.3) ** 2 + (ys - 16.4) ** 2)).astype(np.float32)
    assert R.dark_terms(bowl, 12, 16)["dxx"] > 0 and R.dark_offset(bowl, 12, 16) == (0.0, 0.0)
    saddle = np.exp(0.05 * ((xs - 12.3) ** 2 - (ys - 16.4) ** 2)).astype(np.float32)
    assert R.dark_terms(saddle, 12, 16)["det"] < 0 and R.dark_offset(saddle, 12, 16) == (0.0, 0.0)
    negative = -np.exp(-((xs - 12.3) ** 2 + (ys - 16.4) ** 2) / 8).astype(np.float32)
    assert R.dark_offset(negative, 12, 16) == (0.0, 0.0)
    assert R.dark_offset(np.zeros((h, w), np.float32), 12, 16) == (0.0, 0.0)


def test_dark_step_is_clamped_to_one_cell():
    """a broad Gaussian whose centre lies 3 cells from the evaluated point: the exact Newton step is 3, the clamp makes it 1"""
    h, w = 64, 48
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    m = np.exp(-((xs - 23.0) ** 2 + (ys - 29.0) ** 2) / (2 * 6.0 ** 2)).astype(np.float32)
    t = R.dark_terms(m, 20, 32)
    assert abs(t["sx"] - 3.0) < 0.05 and abs(t["sy"] + 3.0) < 0.05
    assert R.dark_offset(m, 20, 32) == (1.0, -1.0)


def test_decode_restatement_without_refinement_is_the_plain_decode():
    rng = np.random.default_rng(1)
    hm = rng.standard_normal((2, 17, 32, 24)).astype(np.float32)
    boxes = np.asarray([[10, 20, 250, 340], [-5, 7, 100, 180]], np.int32)
    pts = R.decode(hm, boxes, None)
    idx = hm.reshape(2, 17, -1).argmax(-1)
    want_y = (idx // 24) * 1. / 32 * (boxes[:, 3] - boxes[:, 1])[:, None] + boxes[:, 1][:, None]
    np.testing.assert_array_equal(pts[..., 0], want_y.astype(np.float32))


def test_decode_kernels_compile_without_spills(tmp_path):
    use = _resource_usage("decode.hip", str(tmp_path))
    per_joint = [k for k in use if "decode_kernelILi" in k or "refine_coords_kernel" in k]
    assert len(per_joint) == 4 and len(use) == 5, use      # decode_kernel<RF_NONE / _QUARTER / _DARK>, refine_coords, tta_decode
    for name, u in use.items():
        print(name, u)
        assert u["ScratchSize"] == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) == (0 if name in per_joint else 32), (name, u)   # tta_decode_kernel: its 4 + 4 reduction slots


def test_decode_source_is_built_into_the_library():
    lib = load_pkg("_lib")
    assert "decode.hip" in lib.SOURCES
    assert {"hrn_forward_refined", "hrn_refine_coords"} <= set(lib.header_symbols()) and \
        {"hrn_forward_refined", "hrn_refine_coords"} <= set(lib.SYMBOLS)


def test_plan_only_handle_rejects_both_entries():
    pkg = load_pkg()
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    lib, h = net._lib, net._h
    buf = (ctypes.c_float * 64)()
    rc = lib.hrn_forward_refined(h, ctypes.addressof(buf), 1, ctypes.addressof(buf), 0, 2, ctypes.addressof(buf), None, None)
    assert rc == 7 and "plan-only" in lib.hrn_last_error(h).decode()
    rc = lib.hrn_refine_coords(h, ctypes.addressof(buf), 1, 2, ctypes.addressof(buf), None)
    assert rc == 7 and "plan-only" in lib.hrn_last_error(h).decode()
    for bad in (-1, 3, 99):
        assert lib.hrn_forward_refined(h, ctypes.addressof(buf), 1, ctypes.addressof(buf), 0, bad, ctypes.addressof(buf), None, None) == 7
        assert "HRN_REFINE_NONE" in lib.hrn_last_error(h).decode()
        assert lib.hrn_refine_coords(h, ctypes.addressof(buf), 1, bad, ctypes.addressof(buf), None) == 7
        assert "HRN_REFINE_NONE" in lib.hrn_last_error(h).decode()
    assert lib.hrn_forward_refined(None, None, 0, None, 0, 1, None, None, None) == 1
    assert lib.hrn_refine_coords(None, None, 0, 1, None, None) == 1
    net.close()


def test_python_options_reject_unknown_modes():
    pkg = load_pkg()
    native = load_pkg("native")
    assert [native.refine_code(m) for m in (None, "quarter", "dark")] == [0, 1, 2]
    for bad in ("Dark", "none", "udp", 1, True, ["dark"]):
        with pytest.raises(ValueError, match="refine must be"):
            native.refine_code(bad)
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    import torch
    x, b = torch.zeros((1, 3, 64, 64)), np.zeros((1, 4), np.int32)
    with pytest.raises(ValueError, match="refine must be"):
        net.predict_crops(x, b, refine="half")
    with pytest.raises(ValueError, match="refine must be"):
        net.predict_frame(np.zeros((8, 8, 3), np.uint8), np.zeros((0, 4), np.float32), refine="sub")
    with pytest.raises(ValueError, match="refine must be"):
        net.refine_coords(torch.zeros((1, 17, 16, 16)), torch.zeros((1, 17, 2)), "cubic")
    with pytest.raises(ValueError, match="post_processing"):
        net.predict_flip_tta(x, [], post_processing="quarter")
    net.close()
    with pytest.raises(ValueError, match="refine must be"):
        pkg.SimpleHRNet(32, 17, {}, resolution=(64, 48), multiperson=False, refine="subpixel")
