"""Evaluation pre-path, host side: ``postproc.affine_matrix`` / ``box_to_center_scale`` (``misc/utils.py:46-96``,
``datasets/COCO.py:394-413``), the restatement of ``cv2.warpAffine`` the kernel is pinned to (``tests/warp_affine_ref.py``) and
the argument checks of ``hrn_warp_crops`` / ``NativeHRNet.warp_crops``.

OpenCV is absent from this image, so parity with cv2 is UNPINNED.  The restatement is therefore not its own only witness:
exact properties that follow from the arithmetic (identity, integer shifts, the zero border, channels, constants), and an
independent float64 statement of bilinear sampling -- four explicit taps, ``torch.nn.functional.grid_sample`` -- with bounds
derived from the fixed point, not from what the restatement returns.  The two cv2-golden tests at the end make the pin the
moment ``tests/golden/make_warp_golden.py`` has been run somewhere."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import warp_affine_ref as R
from conftest import GOLDEN, load_pkg


def _frame(h, w, seed):
    """== tests/test_resize.py::_frame: edges, texture, saturated pixels"""
    rng = np.random.default_rng(seed)
    smooth = rng.integers(0, 256, (h // 7 + 2, w // 7 + 2, 3)).astype(np.float64)
    up = np.kron(smooth, np.ones((7, 7, 1)))[:h, :w]
    return np.clip(up + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def similarity(center, zoom, deg, out_hw):
    """forward matrix frame -> crop: rotate by ``deg`` and magnify by ``zoom`` about ``center``, which lands on the crop's centre"""
    H, W = out_hw
    a = np.deg2rad(deg)
    L = zoom * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    t = np.array([W / 2, H / 2]) - L @ np.asarray(center, np.float64)
    return np.concatenate([L, t[:, None]], 1)


def _random_similarities(n, frame_hw, out_hw, seed):
    rng = np.random.default_rng(seed)
    h, w = frame_hw
    return [similarity((rng.uniform(0, w), rng.uniform(0, h)), rng.uniform(0.3, 3.0), rng.uniform(-80, 80), out_hw) for _ in range(n)]


# -- 1. matrices and boxes --------------------------------------------------------------------------------------------------
def test_affine_matrix_inverse_direction_is_inverse_affine_bit_for_bit():
    P = load_pkg().postproc
    rng = np.random.default_rng(0)
    for _ in range(100):
        c = rng.uniform(-50, 700, 2).astype(np.float32)
        s = rng.uniform(0.2, 4, 2).astype(np.float32)
        size = ((72, 96), (48, 64), (16, 16))[int(rng.integers(3))]
        a, b = P.affine_matrix(c, s, 200, 0, size, inv=1), P.inverse_affine(c, s, 200, size)
        assert a.dtype == np.float64 and a.shape == (2, 3)
        np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))
    a = P.affine_matrix(np.float32([10, 20]), 1.5, 200, 0, (72, 96), inv=1)        # a scalar scale, as the reference accepts it
    np.testing.assert_array_equal(a, P.inverse_affine(np.float32([10, 20]), 1.5, 200, (72, 96)))


def test_affine_matrix_directions_compose_to_the_identity():
    P = load_pkg().postproc
    rng = np.random.default_rng(1)
    for _ in range(100):
        c = rng.uniform(-50, 700, 2).astype(np.float32)
        s = rng.uniform(0.2, 4, 2).astype(np.float32)
        rot = rng.uniform(-80, 80)
        fwd, inv = P.affine_matrix(c, s, 200, rot, (288, 384)), P.affine_matrix(c, s, 200, rot, (288, 384), inv=1)
        np.testing.assert_allclose(fwd @ np.vstack([inv, [0, 0, 1]]), np.eye(3)[:2], rtol=0, atol=1e-9)


def test_affine_matrix_quarter_turn_by_hand():
    """centre (100, 80), a 100 px box (scale 0.5 x 200), 64 x 64 crop, rot = 90: get_dir turns (0, -50) into (50, 0), so the image
    point 50 px RIGHT of the centre lands on the middle of the crop's TOP edge; with the third point, image (150, 30) -> crop (0, 0).
    The crop's corners (0,0), (64,0), (0,64), (64,64) therefore come from (150,30), (150,130), (50,30), (50,130)."""
    P = load_pkg().postproc
    fwd = P.affine_matrix(np.float32([100, 80]), np.float32([0.5, 0.5]), 200, 90, (64, 64))
    img = np.array([[150, 30, 1], [150, 130, 1], [50, 30, 1], [50, 130, 1], [100, 80, 1]], np.float64)
    np.testing.assert_allclose(img @ fwd.T, [[0, 0], [64, 0], [0, 64], [64, 64], [32, 32]], rtol=0, atol=1e-4)
    np.testing.assert_allclose(fwd[:, :2], [[0, 0.64], [-0.64, 0]], rtol=0, atol=1e-6)
    # rot = 0: the box's top-left corner is the crop's
    fwd0 = P.affine_matrix(np.float32([100, 80]), np.float32([0.5, 0.5]), 200, 0, (64, 64))
    np.testing.assert_allclose(np.array([[50, 30, 1], [150, 130, 1]], np.float64) @ fwd0.T, [[0, 0], [64, 64]], rtol=0, atol=1e-9)


def test_box_to_center_scale_by_hand():
    P = load_pkg().postproc
    ar = 288 / 384   # 0.75
    for box, center, scale in (
            ((10, 20, 300, 100), (160, 70), (300 / 200 * 1.25, 400 / 200 * 1.25)),       # wide: h grows to 300 / 0.75 = 400
            ((0, 0, 60, 200), (30, 100), (150 / 200 * 1.25, 200 / 200 * 1.25)),          # tall: w grows to 200 * 0.75 = 150
            ((5, 5, 150, 200), (80, 105), (150 / 200 * 1.25, 200 / 200 * 1.25)),         # already 3 : 4
            ((-51, 0, 100, 100), (-1, 50), (100 / 200, np.float32(100 / 0.75 / 200)))):  # center[0] == -1: no 1.25 margin
        c, s = P.box_to_center_scale(box, ar)
        assert c.dtype == np.float32 and s.dtype == np.float32 and c.shape == (2,) and s.shape == (2,)
        np.testing.assert_array_equal(c, np.float32(center))
        np.testing.assert_array_equal(s, np.float32(scale))
    c, s = P.box_to_center_scale((10, 20, 300, 100, 0.9), ar, pixel_std=100)             # extra columns ignored, other unit
    np.testing.assert_array_equal(s, np.float32([3 * 1.25, 4 * 1.25]))


# -- 2. the restatement: exact properties -----------------------------------------------------------------------------------
def test_restatement_exact_properties():
    f = _frame(60, 80, 1)
    H, W = 32, 48
    ident = np.array([[1, 0, 0], [0, 1, 0]], np.float64)
    np.testing.assert_array_equal(R.warp_u8(f, ident, (H, W)), f[:H, :W])
    # forward translation by (tx, ty): crop(y, x) = frame(y - ty, x - tx), zero where that leaves the frame
    for tx, ty in ((5, -3), (-7, 4), (-60, -40), (20, 10)):
        want = np.zeros((H, W, 3), np.uint8)
        for y in range(H):
            for x in range(W):
                if 0 <= y - ty < 60 and 0 <= x - tx < 80:
                    want[y, x] = f[y - ty, x - tx]
        np.testing.assert_array_equal(R.warp_u8(f, np.array([[1, 0, tx], [0, 1, ty]], np.float64), (H, W)), want, err_msg=str((tx, ty)))
    # wholly outside; an identity larger than the frame is the frame in a zero field (the taps beyond the last row / column read 0)
    assert not R.warp_u8(f, np.array([[1, 0, 10000], [0, 1, 0]], np.float64), (H, W)).any()
    big = R.warp_u8(f, ident, (70, 90))
    np.testing.assert_array_equal(big[:60, :80], f)
    assert not big[60:].any() and not big[:, 80:].any()
    # half a pixel: the rounded mean of two neighbours ((a + b) * 512 + 512) >> 10
    half = R.warp_u8(f, np.array([[1, 0, -0.5], [0, 1, 0]], np.float64), (H, W)).astype(int)
    np.testing.assert_array_equal(half, (f[:H, :W].astype(int) + f[:H, 1:W + 1] + 1) >> 1)
    # channels do not mix; a constant frame stays constant wherever all four taps are inside, and never exceeds it
    for M in _random_similarities(6, (60, 80), (H, W), 2):
        out = R.warp_u8(f, M, (H, W))
        np.testing.assert_array_equal(R.warp_u8(f[..., ::-1], M, (H, W)), out[..., ::-1])
        const = R.warp_u8(np.full((60, 80, 3), 137, np.uint8), M, (H, W))
        X, Y = R.source_coords(R.invert(M), H, W)
        sx, sy = X >> 5, Y >> 5
        inside = (sx >= 0) & (sx + 1 < 80) & (sy >= 0) & (sy + 1 < 60)
        assert (const[inside] == 137).all() and const.max() <= 137
    assert inside.any()


def test_invert_is_the_inverse_and_refuses_nothing_silently():
    for M in _random_similarities(10, (480, 640), (128, 96), 3):
        np.testing.assert_allclose(M @ np.vstack([R.invert(M), [0, 0, 1]]), np.eye(3)[:2], rtol=0, atol=1e-9)
    assert not R.invert(np.array([[1, 2, 3], [2, 4, 5]], np.float64))[:, :2].any()   # D = 0: cv::warpAffine goes on with zeros


# -- 3. the restatement against an independent float64 statement ------------------------------------------------------------
def _bilinear_taps(f, xs, ys):
    """float64 bilinear sample of frame f (zero outside) at real coordinates: four explicit taps, no fixed point"""
    h, w = f.shape[:2]
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    ax, ay = (xs - x0)[..., None], (ys - y0)[..., None]

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return f[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.float64) * ok[..., None]
    return (tap(y0, x0) * (1 - ax) * (1 - ay) + tap(y0, x0 + 1) * ax * (1 - ay) + tap(y0 + 1, x0) * (1 - ax) * ay +
            tap(y0 + 1, x0 + 1) * ax * ay)


def _grid_sample(f, xs, ys):
    """the same through torch: align_corners=False puts pixel centres at (2 * s + 1) / size - 1"""
    h, w = f.shape[:2]
    grid = torch.from_numpy(np.stack([(2 * xs + 1) / w - 1, (2 * ys + 1) / h - 1], -1))[None]
    img = torch.from_numpy(f.astype(np.float64)).permute(2, 0, 1)[None]
    out = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return out[0].permute(1, 2, 0).numpy()


def test_restatement_against_float64_bilinear():
    """(a) X / 32 within 17/1024 px of Minv @ (x, y, 1): two rints (1/1024 together) + rounding to the nearest 1/32 after the
    + 16 (16/1024).  (b) at the QUANTISED coordinates the float64 bilinear value, rounded half up, is the restatement exactly
    (weights are multiples of 1/1024: float64 is exact).  (c) at the unquantised coordinates single samples may differ by
    several levels at block edges of a textured frame, so only the per-case MEAN is bounded: below 0.5 grey level (the unbiased
    rounding alone contributes 0.25)."""
    f = _frame(480, 640, 4)
    H, W = 128, 96
    worst_coord, worst_level, worst_mean = 0.0, 0.0, 0.0
    for M in _random_similarities(40, (480, 640), (H, W), 5):
        Minv = R.invert(M)
        X, Y = R.source_coords(Minv, H, W)
        x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        xs = Minv[0, 0] * x + Minv[0, 1] * y + Minv[0, 2]
        ys = Minv[1, 0] * x + Minv[1, 1] * y + Minv[1, 2]
        coord = max(np.abs(X / 32 - xs).max(), np.abs(Y / 32 - ys).max())
        worst_coord = max(worst_coord, coord)
        assert coord <= 17 / 1024
        got = R.warp_u8(f, M, (H, W))
        np.testing.assert_array_equal(np.floor(_bilinear_taps(f, X / 32, Y / 32) + 0.5).astype(np.int64), got)
        exact = _grid_sample(f, xs, ys)
        np.testing.assert_allclose(exact, _bilinear_taps(f, xs, ys), rtol=0, atol=1e-9)      # the two float statements agree
        err = np.abs(got.astype(np.float64) - exact)
        worst_level, worst_mean = max(worst_level, err.max()), max(worst_mean, err.mean())
        assert err.mean() < 0.5
    print("quantised coordinates: max %.7f px off (bound %.7f); grey levels against the float formula: max %.2f, worst per-case mean %.3f"
          % (worst_coord, 17 / 1024, worst_level, worst_mean))


def test_kernel_forms_its_float64_coordinates_without_fused_multiply_add(tmp_path):
    """``M1*y + M2`` is a rounded product and a rounded sum in cv::warpAffine.  A fused multiply-add differs from that in the last
    bit of the float64 only, which moves a coordinate only at an exact tie of the rint that follows -- far too rare for the
    bit-equality tests on the GPU to notice -- so the compiled kernel is looked at instead: no float64 FMA in it."""
    import re
    import shutil
    import subprocess

    lib = load_pkg("_lib")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    asm = str(tmp_path / "warp.s")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", "-I", lib.INCLUDE,
                          "-o", asm, os.path.join(lib.CSRC, "warp.hip")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    text = open(asm).read()
    assert "warp_crops_kernel" in text and len(re.findall(r"\bv_mul_f64", text)) >= 4 and "v_rndne_f64" in text
    assert not re.findall(r"\bv_(?:fma|fmac|mad|mac)_f64", text)


def test_eval_transform_layout():
    f = np.stack([_frame(30, 40, 5), _frame(30, 40, 6)])
    M = np.array([[[1, 0, 0], [0, 1, 0]], [[1, 0, 2], [0, 1, 1]]], np.float64)
    x = R.eval_transform(f, M, None, (24, 16))
    assert x.shape == (2, 3, 24, 16) and x.dtype == np.float32
    np.testing.assert_array_equal(x[0, 0], (f[0, :24, :16, 2].astype(np.float32) / np.float32(255) - R.MEAN[0]) / R.STD[0])   # R first
    np.testing.assert_array_equal(R.eval_transform(f, M[[1, 1]], [1, 0], (24, 16))[0], x[1])
    np.testing.assert_array_equal(R.eval_transform(f[0], M[:1], None, (24, 16)), x[:1])


# -- 4. / 5. the C ABI and the wrapper's argument checks ----------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    lib = load_pkg("_lib")
    assert {"hrn_warp_crops"} <= set(lib.header_symbols()) and "hrn_warp_crops" in lib.SYMBOLS
    assert "warp.hip" in lib.SOURCES
    fn = lib.load().hrn_warp_crops
    assert callable(fn) and fn.restype is ctypes.c_int
    assert fn(None, None, 0, 0, 0, None, None, 0, None, None) == 1             # no handle: refused, nothing touched


def test_no_cpu_path_and_argument_checks():
    """the C ABI refuses to warp on a plan-only handle (there is no CPU path in the product); the Python wrapper checks its
    arguments before it gets there -- every case below is a ValueError although this handle could not run anything"""
    pkg = load_pkg()
    net = pkg.NativeHRNet(32, 17, (64, 32), "fp32", max_batch=2, device=-1)
    m = np.array([[1, 0, 0, 0, 1, 0]], np.float64)
    rc = net._lib.hrn_warp_crops(net._h, 0, 1, 10, 10, None, m.ctypes.data, 1, 0, None)
    assert rc == 7 and b"plan-only" in net._lib.hrn_last_error(net._h)
    ok = np.zeros((10, 12, 3), np.uint8)
    c, s = np.float32([[5, 5], [6, 6]]), np.float32([[0.1, 0.1], [0.1, 0.1]])
    ident = np.array([[[1, 0, 0], [0, 1, 0]]], np.float64)
    for kw in (dict(frames=ok.astype(np.float32), centers=c, scales=s),                        # not uint8
               dict(frames=np.zeros((10, 12, 4), np.uint8), centers=c, scales=s),              # four channels
               dict(frames=np.zeros((10, 12), np.uint8), centers=c, scales=s),
               dict(frames=ok, centers=c, scales=s, frame_index=[0, 1]),                       # one frame only
               dict(frames=ok, centers=c, scales=s, frame_index=[0, -1]),
               dict(frames=ok, centers=c, scales=s, frame_index=[0]),                          # mismatched lengths
               dict(frames=ok, centers=c, scales=s[:1]),
               dict(frames=ok, centers=c, scales=s, rotations=[0.0]),
               dict(frames=np.stack([ok] * 3), centers=c, scales=s),                           # 3 frames, 2 crops, no index
               dict(frames=ok, centers=c),                                                     # neither scales nor matrices
               dict(frames=ok, centers=c, scales=s, matrices=ident),                           # both
               dict(frames=ok, matrices=np.zeros((1, 3, 2))),
               dict(frames=ok, matrices=np.array([[[1, 2, 0], [2, 4, 0]]], np.float64)),       # singular
               dict(frames=ok, matrices=np.array([[[1, 0, np.nan], [0, 1, 0]]])),              # not finite
               dict(frames=ok, matrices=np.array([[[np.inf, 0, 0], [0, 1, 0]]])),
               dict(frames=ok, centers=c, scales=np.float32([[0, 0.1], [0.1, 0.1]]))):         # a zero scale: singular
        with pytest.raises(ValueError):
            net.warp_crops(**kw)
    with pytest.raises(ValueError):
        net.predict_eval(ok, c, s[:1], [])
    net.close()
    assert hasattr(pkg.native.MultiDeviceHRNet, "warp_crops") and hasattr(pkg.native.MultiDeviceHRNet, "predict_eval")


# -- 10. the pin for later ------------------------------------------------------------------------------------------------------
_GOLDEN = os.path.join(GOLDEN, "cv2_warp_cases.npz")
_NO_GOLDEN = ("NO cv2 GOLDEN: run tests/golden/make_warp_golden.py where opencv-python is installed and commit "
              "tests/golden/cv2_warp_cases.npz -- until then %s")


def test_restatement_against_cv2_warp_golden():
    """``tests/golden/cv2_warp_cases.npz`` holds ``cv2.warpAffine(..., flags=cv2.INTER_LINEAR)`` outputs made on a machine WITH
    opencv-python.  Absent (cv2 is in neither image of this repository): skipped, loudly -- parity with cv2 then stays unpinned.
    Present: BIT EQUALITY.  The restated path is integer arithmetic; a cv2 build that differs (newer releases carry float
    warpAffine kernels) is a finding to be recorded with its version, not a tolerance to be granted in advance."""
    if not os.path.exists(_GOLDEN):
        pytest.skip(_NO_GOLDEN % "hrn_warp_crops is pinned to the restatement of OpenCV's 8-bit warpAffine only")
    g = np.load(_GOLDEN)
    checked = 0
    for n in range(int(g["ncases"])):
        h, w, seed, crc, W, H = (int(v) for v in g["case%d_meta" % n])
        f = _frame(h, w, seed)
        if zlib.crc32(f.tobytes()) != crc:
            print("case %d: this numpy regenerates another frame than the golden's (crc differs) -- not comparable, skipped" % n)
            continue
        np.testing.assert_array_equal(R.warp_u8(f, g["case%d_fwd" % n], (H, W)), g["case%d_out" % n],
                                      err_msg="case %d against cv2 %s" % (n, g["cv2_version"]))
        checked += 1
    assert checked > 0


def test_affine_matrix_against_cv2_golden():
    """the same fixture holds ``cv2.getAffineTransform``'s matrices for the reference's point pairs, both directions:
    ``postproc.affine_matrix`` (a float64 LU solve in its place) must agree to 1e-12 relative."""
    if not os.path.exists(_GOLDEN):
        pytest.skip(_NO_GOLDEN % "postproc.affine_matrix / inverse_affine stand on their float64 solve, not on cv2.getAffineTransform")
    P = load_pkg().postproc
    g = np.load(_GOLDEN)
    for n in range(int(g["ncases"])):
        W, H = (int(v) for v in g["case%d_meta" % n][4:6])
        cx, cy, sw, sh, rot = g["case%d_csr" % n]
        c, s = np.float32([cx, cy]), np.float32([sw, sh])
        for inv, key in ((0, "fwd"), (1, "inv")):
            got, want = P.affine_matrix(c, s, int(g["pixel_std"]), rot, (W, H), inv=inv), g["case%d_%s" % (n, key)]
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (n, key, str(g["cv2_version"]))
