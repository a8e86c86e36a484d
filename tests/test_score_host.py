"""Scoring of an evaluation batch, host side: the numpy restatement (``tests/score_ref.py``) against outputs of the unmodified
reference functions (``tests/golden/score_cases.npz``, made by ``tests/golden/make_score_golden.py``), ``hrn_target_centers``
(which needs no GPU) against the same fixture, the C ABI's names and argument checks, and what the compiler made of
``csrc/score.hip``.

Tolerances, none of them taken from the code under test:
* target support and weights: equal.  Target values: within ``g_ulps + 1`` float32 ulps, ``g_ulps`` being the distance the
  generator measured between the reference's float32 SIMD ``exp`` and ``float32(exp(float64))`` on its numpy build (the library
  defines its own table because that ``exp`` is not correctly rounded and differs between builds); + 1 for another build.
* losses against the reference's float64 evaluation, with the reference's Gaussian substituted for the table: relative
  ``2 * (n*h*w + J + 4) * 2^-53`` -- both sides sum the same non-negative doubles in different orders.
* the float32-rounded loss within ``|ref32 - ref64| + 1 ulp`` of the reference's float32 value.
* PCK: preds, targets, acc, avg_acc, cnt equal (the generator asserts no distance is within 1e-4 of the threshold); dists
  within 2 float32 ulps (torch's two-element ``norm`` is not specified to the last bit)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import score_ref as R
from conftest import golden, load_pkg

G = golden("score_cases")
CASES = list(range(int(G["ncases"])))
THR, TOPK = float(G["thr"]), int(G["topk"])


def case(k):
    c = {name[len("case%d_" % k):]: v for name, v in G.items() if name.startswith("case%d_" % k)}
    c["hw"] = c["target"].shape[2:]
    c["jw"] = c["joints_weight"] if int(c["use_jw"]) else None
    return c


def sum_bound(c):
    n, J, h, w = c["target"].shape
    return 2.0 * (n * h * w + J + 4) * 2.0 ** -53


def reference_table(c):
    """the restatement's table with the reference's own values: g[dx^2 + dy^2] read off its (2t+1) x (2t+1) Gaussian"""
    sigma = int(c["sigma"])
    t = 3 * sigma
    g = R.table(sigma).copy()
    d = np.arange(-t, t + 1)
    d2 = d[None] ** 2 + d[:, None] ** 2
    for v in np.unique(d2):
        vals = np.unique(c["g"][d2 == v])
        assert len(vals) == 1                      # the reference's Gaussian is a function of d2 too
        g[v] = vals[0]
    return g


def assert_close_or_nan(got, want, rel, what):
    if np.isnan(want):
        assert np.isnan(got), what
    else:
        assert abs(got - want) <= rel * abs(want), (what, got, want)


@pytest.mark.parametrize("k", CASES)
def test_restated_targets_against_the_reference(k):
    c = case(k)
    tgt, tw = R.generate_targets(c["joints"], c["vis"], c["hw"], int(c["sigma"]), c["jw"])
    np.testing.assert_array_equal(tw, c["target_weight"][:, :, 0])
    np.testing.assert_array_equal(tgt != 0, c["target"] != 0)
    allowed = int(G["g_ulps"]) + 1
    worst = int(R.ulp_distance(tgt, c["target"]).max())
    print("case %d: target values within %d ulp of the reference's (allowed %d)" % (k, worst, allowed))
    assert worst <= allowed
    if "g" in c:   # with the reference's Gaussian in place of the table the maps are the reference's, bit for bit
        np.testing.assert_array_equal(R.generate_targets(c["joints"], c["vis"], c["hw"], int(c["sigma"]), c["jw"], g=reference_table(c))[0],
                                      c["target"])


def test_the_kept_quirk_is_in_the_fixture():
    """``br < 0``, not ``<= 0``: mu = -(t + 1) keeps its weight and draws nothing"""
    seen = 0
    for k in CASES:
        c = case(k)
        mu, weight, _, drawn = R.target_centers(c["joints"], c["vis"], c["hw"], int(c["sigma"]))
        q = (weight > 0.5) & ~drawn
        seen += int(q.sum())
        assert (c["target"][q] == 0).all() and (c["target_weight"][:, :, 0][q] > 0).all()
    assert seen >= 8


@pytest.mark.parametrize("k", CASES)
def test_restated_losses_against_the_reference(k):
    c = case(k)
    g = reference_table(c) if "g" in c else None
    tgt, tw = R.generate_targets(c["joints"], c["vis"], c["hw"], int(c["sigma"]), c["jw"], g=g)
    L = R.map_loss(c["output"], tgt, tw)
    mse, ohkm = R.losses(L, TOPK)
    bound = sum_bound(c)
    ref = c["map_loss64"]
    assert np.array_equal(np.isnan(L), np.isnan(ref))
    ok = np.isfinite(ref)
    assert (np.abs(L[ok] - ref[ok]) <= bound * np.abs(ref[ok])).all()
    np.testing.assert_array_equal(L[np.isinf(ref)], ref[np.isinf(ref)])
    assert_close_or_nan(mse, float(c["loss64"]), bound, "loss")
    assert_close_or_nan(ohkm, float(c["ohkm64"]), bound, "loss_ohkm")
    if not np.isnan(c["loss64"]):
        ref32, ref64 = np.float32(c["loss32"]), float(c["loss64"])
        slack = abs(float(ref32) - ref64) + float(np.spacing(ref32))
        print("case %d: |float32(loss) - ref32| = %.3g, allowed %.3g" % (k, abs(float(np.float32(mse)) - float(ref32)), slack))
        assert abs(float(np.float32(mse)) - float(ref32)) <= slack


@pytest.mark.parametrize("k", CASES)
def test_restated_pck_against_the_reference(k):
    c = case(k)
    for mode in ("analytic", "maps"):
        kw = dict(joints=c["joints"], vis=c["vis"], sigma=int(c["sigma"]), joints_weight=c["jw"]) if mode == "analytic" else \
            dict(targets=c["target"], target_weight=c["target_weight"])
        s = R.score(c["output"], thr=THR, topk=TOPK, **kw)
        np.testing.assert_array_equal(s["joints_preds"], c["pred"], err_msg=mode)
        np.testing.assert_array_equal(s["joints_target"], c["target_pred"], err_msg=mode)
        np.testing.assert_array_equal(s["accs"], c["acc"], err_msg=mode)
        assert s["avg_acc"] == c["avg_acc"] and s["cnt"] == int(c["cnt"]), mode
        assert np.array_equal(s["dists"] == -1, c["dists"] == -1)
        assert R.ulp_distance(np.abs(s["dists"]), np.abs(c["dists"])).max() <= 2, mode


@pytest.mark.parametrize("k", CASES)
def test_target_centers_entry_against_the_reference(k):
    """``hrn_target_centers`` runs on the host: mu recovered from the reference's maps (the arg-max of a window that is wholly
    inside is its centre), weights equal, and everything equal to the restatement"""
    P = load_pkg().postproc
    c = case(k)
    h, w = c["hw"]
    sigma = int(c["sigma"])
    mu, draw, tw = P.target_centers(c["joints"], c["vis"], (4 * h, 4 * w), sigma, c["jw"])
    rmu, rweight, rtw, _ = R.target_centers(c["joints"], c["vis"], c["hw"], sigma, c["jw"])
    np.testing.assert_array_equal(mu, rmu)
    np.testing.assert_array_equal(draw, rweight)
    np.testing.assert_array_equal(tw, rtw)
    np.testing.assert_array_equal(tw, c["target_weight"][:, :, 0])
    peak = R.max_preds(c["target"])[0]
    inside = (c["target"].reshape(*tw.shape, -1).max(-1) == 1)            # the centre cell is on the map
    np.testing.assert_array_equal(mu[inside], peak[inside].astype(np.int32))
    assert inside.sum() >= 5 or not (c["vis"] > 0).any()


def test_target_centers_refuses_bad_arguments():
    P = load_pkg().postproc
    j, v = np.zeros((1, 17, 2)), np.ones((1, 17), np.float32)
    for bad in (dict(sigma=0), dict(sigma=-1), dict(sigma=0.5), dict(sigma=np.nan), dict(resolution=(60, 64))):
        with pytest.raises(ValueError):
            P.target_centers(j, v, **{"resolution": (64, 64), "sigma": 2, **bad})
    for x in (np.nan, np.inf, 1e10, -1e10):
        jj = j.copy()
        jj[0, 3, 1] = x
        with pytest.raises(ValueError, match="joint 3 of person 0"):
            P.target_centers(jj, v, (64, 64), 2)
    assert P.target_centers(j, v, (64, 64), 1 / 3)[0].shape == (1, 17, 2)          # 3 * sigma = 1
    with pytest.raises(ValueError):
        P.target_centers(j, v, (64, 64), 2, joints_weight=np.ones(16))


def test_joints_to_crop():
    P = load_pkg().postproc
    rng = np.random.default_rng(0)
    jt, vis = rng.uniform(0, 400, (3, 17, 2)), (rng.uniform(0, 1, (3, 17)) > 0.3).astype(np.float32)
    c, s = rng.uniform(100, 300, (3, 2)).astype(np.float32), rng.uniform(0.5, 2, (3, 2)).astype(np.float32)
    m = np.stack([P.affine_matrix(c[i], s[i], 200, 0, (48, 64)) for i in range(3)])
    got = P.joints_to_crop(jt, np.stack([vis, vis], -1), m)
    assert got.dtype == np.float64 and got.shape == (3, 17, 2)
    for i in range(3):
        for j in range(17):
            want = m[i] @ np.array([jt[i, j, 0], jt[i, j, 1], 1.0]) if vis[i, j] > 0 else jt[i, j]
            np.testing.assert_allclose(got[i, j], want, rtol=1e-15, atol=1e-12)
    np.testing.assert_array_equal(got[vis == 0], jt[vis == 0])
    # the centre of the box lands on the centre of the crop
    np.testing.assert_allclose(P.joints_to_crop(c[:, None, :].astype(np.float64), np.ones((3, 1)), m)[:, 0], [[24, 32]] * 3, atol=1e-3)
    with pytest.raises(ValueError):
        P.joints_to_crop(jt, vis, m[:2])


def test_symbols_are_declared_and_exported():
    lib = load_pkg("_lib")
    names = {"hrn_target_centers", "hrn_generate_targets", "hrn_score_heatmaps"}
    assert names <= set(lib.header_symbols()) and names <= set(lib.SYMBOLS)
    assert "score.hip" in lib.SOURCES
    L = lib.load()
    assert L.hrn_score_heatmaps(None, None, 0, None, None, None, None, 2.0, None, 0.5, 0, None, None) == 1     # no handle
    assert L.hrn_generate_targets(None, None, None, None, 0, 2.0, None, None, None) == 1
    assert [f[0] for f in lib.ScoreOut._fields_] == ["loss_mse", "loss_ohkm", "avg_acc", "cnt", "acc", "dists", "map_loss", "preds",
                                                     "target_preds", "maxvals"]
    text = open(os.path.join(lib.INCLUDE, "hrnet_mi355.h")).read()
    fields = re.search(r"typedef struct \{([^}]*)\} hrn_score_out;", text).group(1)
    assert re.findall(r"\*(\w+)", fields) == [f[0] for f in lib.ScoreOut._fields_]


def test_no_cpu_path_and_argument_checks():
    pkg = load_pkg()
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    j, v = np.zeros((1, 17, 2)), np.ones((1, 17), np.float32)
    out = load_pkg("_lib").ScoreOut()
    rc = net._lib.hrn_score_heatmaps(net._h, 16, 1, None, j.ctypes.data, v.ctypes.data, None, 2.0, None, 0.5, 0, ctypes.byref(out), None)
    assert rc == 7 and b"plan-only" in net._lib.hrn_last_error(net._h)
    rc = net._lib.hrn_generate_targets(net._h, j.ctypes.data, v.ctypes.data, None, 1, 2.0, 16, None, None)
    assert rc == 7 and b"plan-only" in net._lib.hrn_last_error(net._h)
    net.close()
    for name in ("generate_targets", "score_heatmaps", "score_eval"):
        assert hasattr(pkg.NativeHRNet, name)


def _compile(tmp_path, *extra):
    lib = load_pkg("_lib")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-I", lib.INCLUDE,
                          os.path.join(lib.CSRC, "score.hip")] + list(extra), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stderr


def test_score_kernels_compile_without_scratch(tmp_path):
    err = _compile(tmp_path, "-c", "-o", str(tmp_path / "score.o"), "-Rpass-analysis=kernel-resource-usage")
    use, name = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            use[name] = {}
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            use[name][m.group(1).strip()] = int(m.group(2))
    assert len(use) == 4 and sum("score_kernelILb" in k for k in use) == 2, use     # score_kernel<maps / analytic>, finish, targets
    for name, u in use.items():
        print(name, u)
        assert u["ScratchSize"] == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)


def test_finish_kernel_has_no_float32_fma_and_no_kernel_a_float_atomic(tmp_path):
    """the PCK distances are torch's separate float32 operations: a fused ``dx*dx + dy*dy`` would differ in the last bit.  The
    float32 divisions and the root go through fp64 (exact for float operands), so the kernel's ISA holds no float32 FMA at all;
    and nothing in the file accumulates through floating-point atomics (their order is not reproducible)."""
    asm = str(tmp_path / "score.s")
    _compile(tmp_path, "-S", "-o", asm)
    text = open(asm).read()
    m = re.search(r"^_ZN3hrn19score_finish_kernel\w*:[^\n]*\n(.*?)s_endpgm", text, re.S | re.M)
    assert m, "score_finish_kernel not found in the ISA"
    body = m.group(1)
    assert re.search(r"\bv_(?:pk_)?mul_f32", body) and re.search(r"\bv_(?:pk_)?add_f32", body)   # dx*dx, dy*dy, then their sum
    assert not re.findall(r"\bv_(?:pk_)?(?:fma|fmac|mad|mac)_f32", body)
    assert not re.findall(r"\b(?:global|flat|buffer)_atomic_\w*(?:f32|f64|f16|add_f|pk_add)", text)
