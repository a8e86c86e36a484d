"""Scoring of an evaluation batch on the GPU: ``NativeHRNet.generate_targets`` / ``score_heatmaps`` / ``score_eval``
(``csrc/score.hip``) against the numpy restatement (``tests/score_ref.py``) and against outputs of the unmodified reference
functions (``tests/golden/score_cases.npz``).  Tolerances as in ``tests/test_score_host.py``: the losses within the summation
bound ``2 * (n*h*w + J + 4) * 2^-53`` (relative), the float32-rounded loss within ``|ref32 - ref64| + 1 ulp``, everything of the
PCK equal, distances equal to the restatement's float32 bit for bit (same operations) and within 2 ulps of torch's."""
import ctypes

import numpy as np
import pytest
import torch

import score_ref as R
from conftest import golden, load_pkg, state_dict_np
from test_score_host import CASES, THR, TOPK, assert_close_or_nan, case, sum_bound

pytestmark = pytest.mark.gpu

_NETS = {}


def engine(hw, J):
    """a weightless engine of the case's shape (scoring needs no weights); kept for the module"""
    key = (tuple(hw), J)
    if key not in _NETS:
        _NETS[key] = load_pkg().NativeHRNet(32, J, (4 * hw[0], 4 * hw[1]), "fp32", max_batch=2, device=0)
    return _NETS[key]


def host(d):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def same_bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), what


def check_pck(got, want, what, dists_ulps=0):
    for key in ("joints_preds", "joints_target", "accs"):
        np.testing.assert_array_equal(got[key], want[key], err_msg="%s: %s" % (what, key))
    assert float(got["avg_acc"]) == float(want["avg_acc"]) and int(got["cnt"]) == int(want["cnt"]), what
    assert np.array_equal(got["dists"] == -1, want["dists"] == -1), what
    assert R.ulp_distance(np.abs(got["dists"]), np.abs(want["dists"])).max() <= dists_ulps, what


def check_losses(got, want_L, want_mse, want_ohkm, bound, what):
    L = got["map_loss"]
    assert np.array_equal(np.isnan(L), np.isnan(want_L)), what
    fin = np.isfinite(want_L)
    assert (np.abs(L[fin] - want_L[fin]) <= bound * np.abs(want_L[fin])).all(), what
    np.testing.assert_array_equal(L[np.isinf(want_L)], want_L[np.isinf(want_L)])
    assert_close_or_nan(float(got["loss"]), float(want_mse), bound, what + ": loss")
    assert_close_or_nan(float(got["loss_ohkm"]), float(want_ohkm), bound, what + ": loss_ohkm")


@pytest.mark.parametrize("k", CASES)
def test_generate_targets_equals_the_restatement(k):
    c = case(k)
    net = engine(c["hw"], c["target"].shape[1])
    tgt, tw = net.generate_targets(c["joints"], c["vis"], sigma=int(c["sigma"]), joints_weight=c["jw"])
    want, want_tw = R.generate_targets(c["joints"], c["vis"], c["hw"], int(c["sigma"]), c["jw"])
    assert tgt.is_cuda and tgt.dtype == torch.float32 and tw.shape == c["target_weight"].shape
    same_bits(tgt.cpu().numpy(), want, "targets")
    same_bits(tw[:, :, 0], want_tw, "target_weight")
    np.testing.assert_array_equal(tw, c["target_weight"])
    np.testing.assert_array_equal(tgt.cpu().numpy() != 0, c["target"] != 0)
    assert R.ulp_distance(tgt.cpu().numpy(), c["target"]).max() <= int(golden("score_cases")["g_ulps"]) + 1


@pytest.mark.parametrize("k", CASES)
def test_score_modes_agree_and_meet_the_restatement(k):
    c = case(k)
    sigma = int(c["sigma"])
    net = engine(c["hw"], c["target"].shape[1])
    out = torch.from_numpy(c["output"]).cuda()
    tgt, tw = net.generate_targets(c["joints"], c["vis"], sigma=sigma, joints_weight=c["jw"])
    a = host(net.score_heatmaps(out, joints=c["joints"], visibility=c["vis"], sigma=sigma, joints_weight=c["jw"], thr=THR, topk=TOPK))
    m = host(net.score_heatmaps(out, targets=tgt, target_weight=tw, thr=THR, topk=TOPK))
    assert a["loss"].dtype == np.float64 and a["map_loss"].dtype == np.float64 and a["cnt"].dtype == np.int32
    assert a["accs"].dtype == np.float32 and a["joints_preds"].shape == c["pred"].shape and a["maxvals"].shape == c["pred"].shape[:2] + (1,)
    for key in a:
        same_bits(a[key], m[key], "analytic vs maps: " + key)
    want = R.score(c["output"], joints=c["joints"], vis=c["vis"], sigma=sigma, joints_weight=c["jw"], thr=THR, topk=TOPK)
    check_losses(a, want["map_loss"], want["loss"], want["loss_ohkm"], sum_bound(c), "restatement")
    check_pck(a, want, "restatement")
    same_bits(a["dists"], want["dists"], "dists")
    same_bits(a["maxvals"], want["maxvals"], "maxvals")
    no_topk = host(net.score_heatmaps(out, joints=c["joints"], visibility=c["vis"], sigma=sigma, joints_weight=c["jw"], thr=THR))
    assert np.isnan(no_topk["loss_ohkm"]) and no_topk["loss"].tobytes() == a["loss"].tobytes()


@pytest.mark.parametrize("k", CASES)
def test_score_against_the_reference(k):
    """maps mode fed with the reference's own target maps and weights (no table involved), and the PCK in analytic mode"""
    c = case(k)
    net = engine(c["hw"], c["target"].shape[1])
    out = torch.from_numpy(c["output"]).cuda()
    m = host(net.score_heatmaps(out, targets=c["target"], target_weight=c["target_weight"], thr=THR, topk=TOPK))
    ref = {"joints_preds": c["pred"], "joints_target": c["target_pred"], "accs": c["acc"], "avg_acc": c["avg_acc"], "cnt": c["cnt"],
           "dists": c["dists"]}
    check_losses(m, c["map_loss64"], c["loss64"], c["ohkm64"], sum_bound(c), "reference")
    check_pck(m, ref, "reference, maps", dists_ulps=2)
    if not np.isnan(c["loss64"]):
        ref32, ref64 = np.float32(c["loss32"]), float(c["loss64"])
        got32 = float(np.float32(m["loss"]))
        print("case %d: loss %.17g (reference float64 %.17g), |float32(loss) - ref32| = %.3g" % (k, float(m["loss"]), ref64, abs(got32 - float(ref32))))
        assert abs(got32 - float(ref32)) <= abs(float(ref32) - ref64) + float(np.spacing(ref32))
    a = host(net.score_heatmaps(out, joints=c["joints"], visibility=c["vis"], sigma=int(c["sigma"]), joints_weight=c["jw"], thr=THR))
    check_pck(a, ref, "reference, analytic", dists_ulps=2)


def test_a_map_does_not_depend_on_the_batch_or_its_position():
    c = case(0)
    J = c["target"].shape[1]
    net = load_pkg().NativeHRNet(32, J, (4 * c["hw"][0], 4 * c["hw"][1]), "fp32", max_batch=16, device=0)
    rng = np.random.default_rng(3)
    one = host(net.score_heatmaps(torch.from_numpy(c["output"][1:2]).cuda(), joints=c["joints"][1:2], visibility=c["vis"][1:2], topk=TOPK))
    for n in (1, 3, 250, 257):
        src = rng.integers(0, len(c["output"]), n)
        pos = int(rng.integers(0, n))
        src[pos] = 1
        out = torch.from_numpy(c["output"][src]).cuda()
        s = host(net.score_heatmaps(out, joints=c["joints"][src], visibility=c["vis"][src], topk=TOPK))
        for key in ("map_loss", "joints_preds", "joints_target", "maxvals"):
            same_bits(s[key][pos], one[key][0], "n = %d, position %d: %s" % (n, pos, key))
        want = R.score(c["output"][src], joints=c["joints"][src], vis=c["vis"][src], topk=TOPK)
        bound = 2.0 * (n * c["hw"][0] * c["hw"][1] + J + 4) * 2.0 ** -53
        check_losses(s, want["map_loss"], want["loss"], want["loss_ohkm"], bound, "n = %d" % n)
        check_pck(s, want, "n = %d" % n)
        same_bits(s["map_loss"], host(net.score_heatmaps(out, joints=c["joints"][src], visibility=c["vis"][src]))["map_loss"], "repeat")
    net.close()


def test_nan_and_inf_cells_decode_like_torch_max():
    c = case(5)
    net = engine(c["hw"], c["target"].shape[1])
    s = host(net.score_heatmaps(torch.from_numpy(c["output"]).cuda(), joints=c["joints"], visibility=c["vis"], thr=THR, topk=TOPK))
    values, index = torch.max(torch.from_numpy(c["output"]).reshape(2, 17, -1), dim=2)
    np.testing.assert_array_equal(s["joints_preds"], c["pred"])
    same_bits(s["maxvals"][:, :, 0], values.numpy(), "maxvals against torch.max")
    assert int(index[0, 1]) == 7 * c["hw"][1] + 2                                                # the first NaN of the map
    assert np.isnan(s["maxvals"][0, 0, 0]) and (s["joints_preds"][0, 0] == 0).all()             # a NaN maximum is not > 0
    assert s["maxvals"][0, 2, 0] == -np.inf and (s["joints_preds"][0, 2] == 0).all()
    assert s["maxvals"][1, 3, 0] == np.inf and (s["joints_preds"][1, 3] == 0).all()              # +inf at cell (0, 0)
    assert np.isnan(s["loss"]) and np.isnan(s["loss_ohkm"]) and np.isnan(s["map_loss"][0, 0])
    assert np.isfinite(s["map_loss"][1, 5])


def test_library_refuses_before_it_launches():
    c = case(0)
    net = engine(c["hw"], 17)
    n, J = c["vis"].shape
    hm = torch.from_numpy(c["output"]).cuda()
    tg = torch.from_numpy(c["target"]).cuda()
    f32, f64 = dict(dtype=torch.float32, device="cuda"), dict(dtype=torch.float64, device="cuda")
    t = {"loss_mse": torch.full((), 7.0, **f64), "loss_ohkm": torch.full((), 7.0, **f64), "avg_acc": torch.full((), 7.0, **f32),
         "cnt": torch.full((), 7, dtype=torch.int32, device="cuda"), "acc": torch.full((J,), 7.0, **f32), "dists": torch.full((J, n), 7.0, **f32),
         "map_loss": torch.full((n, J), 7.0, **f64), "preds": torch.full((n, J, 2), 7.0, **f32), "target_preds": torch.full((n, J, 2), 7.0, **f32),
         "maxvals": torch.full((n, J), 7.0, **f32)}
    out = load_pkg("_lib").ScoreOut(**{k: v.data_ptr() for k, v in t.items()})
    jt, vis, tw = np.ascontiguousarray(c["joints"]), np.ascontiguousarray(c["vis"]), np.ascontiguousarray(c["target_weight"].reshape(-1))

    def call(n=n, targets=None, joints=jt, vis=vis, sigma=2.0, tw=None, thr=0.5, topk=0, out=out, hm=hm.data_ptr()):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return net._lib.hrn_score_heatmaps(net._h, hm, n, targets, p(joints), p(vis), None, sigma, p(tw), thr, topk,
                                           None if out is None else ctypes.byref(out), None)
    bad = jt.copy()
    bad[1, 2, 0] = np.nan
    far = jt.copy()
    far[0, 0, 1] = 1e11
    partial = load_pkg("_lib").ScoreOut(**{k: v.data_ptr() for k, v in t.items() if k != "dists"})
    for what, rc in (("n < 0", call(n=-1)), ("both sources", call(targets=tg.data_ptr(), tw=tw)), ("neither", call(joints=None, vis=None)),
                     ("maps without weights", call(targets=tg.data_ptr(), joints=None, vis=None)),
                     ("joints without visibility", call(vis=None)), ("sigma 0", call(sigma=0.0)), ("sigma -1", call(sigma=-1.0)),
                     ("3 sigma not an integer", call(sigma=0.5)), ("sigma nan", call(sigma=float("nan"))), ("nan joint", call(joints=bad)),
                     ("joint beyond int32", call(joints=far)), ("topk > J", call(topk=J + 1)), ("thr nan", call(thr=float("nan"))),
                     ("thr inf", call(thr=float("inf"))), ("no out", call(out=None)), ("a NULL field", call(out=partial)),
                     ("unaligned maps", call(hm=hm.data_ptr() + 4))):
        assert rc == 7, what
        assert net._lib.hrn_last_error(net._h), what
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in t.values())                         # nothing was launched
    assert call(topk=J) == 0 and call(targets=tg.data_ptr(), joints=None, vis=None, tw=tw) == 0
    torch.cuda.synchronize()
    assert float(t["loss_mse"]) != 7.0
    with pytest.raises(ValueError):
        net.score_heatmaps(hm)
    with pytest.raises(ValueError):
        net.score_heatmaps(hm, joints=jt, visibility=vis, targets=tg, target_weight=tw)
    with pytest.raises(ValueError):
        net.score_heatmaps(hm[:, :5], joints=jt, visibility=vis)
    with pytest.raises(ValueError):
        net.score_heatmaps(hm, joints=jt[:2], visibility=vis[:2])
    with pytest.raises(RuntimeError, match="not finite"):
        net.score_heatmaps(hm, joints=bad, visibility=vis)
    empty = host(net.score_heatmaps(hm[:0], joints=jt[:0], visibility=vis[:0]))     # n = 0: NaN losses, no accuracy
    assert np.isnan(empty["loss"]) and int(empty["cnt"]) == 0 and (empty["accs"] == -1).all() and float(empty["avg_acc"]) == 0


def test_one_engine_scored_against_another_and_the_workspace_is_untouched():
    """maps mode with heat-maps as the target: bf16 against fp32 on the seeded W32 checkpoint, and a tensor against itself"""
    pkg = load_pkg()
    sd = state_dict_np(32, 0)
    crops = torch.from_numpy(pkg.synth_crops(3, 64, 64, seed=4)).cuda()
    f32 = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=0).load_state_dict(sd)
    b16 = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=2, device=0).load_state_dict(sd)
    ref, low = f32(crops), b16(crops)
    before = ref.cpu().numpy()
    ones = np.ones((3, 17), np.float32)
    same = host(f32.score_heatmaps(ref, targets=ref, target_weight=ones, thr=THR, topk=TOPK))
    assert float(same["loss"]) == 0 and float(same["loss_ohkm"]) == 0 and (same["map_loss"] == 0).all()
    np.testing.assert_array_equal(same["joints_preds"], same["joints_target"])
    assert ((same["joints_target"] > 1).all(-1)).any(), "no arg-max beyond cell 1 on both axes: the accuracy below would be vacuous"
    assert float(same["avg_acc"]) == 1 and int(same["cnt"]) >= 1 and (same["accs"][same["accs"] >= 0] == 1).all()
    cross = host(f32.score_heatmaps(low, targets=ref, target_weight=ones, thr=THR, topk=TOPK))
    want = R.score(low.cpu().numpy(), targets=before, target_weight=ones, thr=THR, topk=TOPK)
    check_losses(cross, want["map_loss"], want["loss"], want["loss_ohkm"], 2.0 * (3 * 256 + 21) * 2.0 ** -53, "bf16 against fp32")
    check_pck(cross, want, "bf16 against fp32")
    assert float(cross["loss"]) > 0
    print("bf16 against fp32 on the seeded W32 checkpoint: loss %.3g, PCK@%.1f %.3f over %d joints" %
          (float(cross["loss"]), THR, float(cross["avg_acc"]), int(cross["cnt"])))
    assert f32.pad_violations() == 0 and b16.pad_violations() == 0
    same_bits(f32(crops).cpu().numpy(), before, "a forward pass after scoring")
    f32.close()
    b16.close()


def test_score_eval_is_predict_eval_then_score_heatmaps():
    from test_warp_gpu import TTA, _people
    from test_warp_host import _frame
    g = golden(TTA)
    pkg = load_pkg()
    P = pkg.postproc
    c_, h, w = int(g["c"]), int(g["h"]), int(g["w"])
    net = pkg.NativeHRNet(c_, 17, (h, w), "bf16", max_batch=4, device=0).load_state_dict(state_dict_np(c_, int(g["weight_seed"])))
    frames = np.stack([_frame(480, 640, 8), _frame(480, 640, 9)])
    fi = np.array([0, 1, 1, 0, 1])
    c, s = _people(5, 10)
    rng = np.random.default_rng(2)
    gt = c[:, None, :].astype(np.float64) + rng.uniform(-1, 1, (5, 17, 2)) * (s[:, None, :] * 200 * 0.6)    # some joints leave the crop
    vis = (rng.uniform(0, 1, (5, 17)) > 0.2).astype(np.float32)
    jw = np.linspace(1, 1.5, 17).astype(np.float32)
    plain = net.predict_eval(frames, c, s, g["flip_pairs"], frame_index=fi)
    out, score = net.score_eval(frames, c, s, g["flip_pairs"], gt, np.stack([vis, vis], -1), frame_index=fi, sigma=3, joints_weight=jw,
                                thr=THR, topk=TOPK)
    np.testing.assert_array_equal(out[0], plain[0])
    same_bits(out[1].cpu().numpy(), plain[1].cpu().numpy(), "maxvals")
    same_bits(out[2].cpu().numpy(), plain[2].cpu().numpy(), "heat-maps")
    m = np.stack([P.affine_matrix(c[i], s[i], 200, 0, (w, h)) for i in range(5)])
    want = host(net.score_heatmaps(plain[2], joints=P.joints_to_crop(gt, vis, m), visibility=vis, sigma=3, joints_weight=jw, thr=THR, topk=TOPK))
    got = host(score)
    for key in want:
        same_bits(got[key], want[key], key)
    assert (got["joints_target"] > 0).any() and int(got["cnt"]) > 0
    assert net.pad_violations() == 0
    net.close()
