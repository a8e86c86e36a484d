"""Heads with more than 32 joints on the MI355X (include/hrnet_mi355.h: HRN_MAX_JOINTS): whole-body 133, face 68, the ragged
counts around a joint group of 32.  References: outputs of the unmodified reference (tests/golden/j*.npz, written by
tests/golden/make_joints_golden.py, which asserts a top-1/top-2 gap above 4e-4 for every stored map, so identical coordinates
can be demanded of every joint), the oracle, and the numpy restatements the 17-joint tests use -- with their tolerances.

The two invariants of the header are tested directly: a joint's numbers do not depend on how many other joints the model has
(test_a_joint_does_not_depend_on_the_other_joints), and J <= 32 is untouched (the existing suite)."""
import os

import numpy as np
import pytest
import torch

import score_ref as SR
import subpixel_ref as R
from conftest import golden, load_pkg
from oracle import hrnet_torch_oracle as T
from test_refine_gpu import _cells, check_dark
from test_score_gpu import check_losses, check_pck, host, same_bits

pytestmark = pytest.mark.gpu

HM_ATOL_F32 = 2e-4
FIXTURES = ["j133_w32_64x64_n2", "j133_w48_128x96_n2", "j68_w32_64x96_n3", "j33_w48_64x64_n2"]
TTA = "j133_w32_128x96_fliptta_n3"
MAX_JOINTS = 256


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    assert torch.cuda.is_available(), "GPU tests need a GPU: the HIP path has no CPU fallback"
    return p


_SD = {}


def sd_np(pkg, c, J, seed, model="HRNet"):
    key = (c, J, seed, model)
    if key not in _SD:
        _SD[key] = pkg.synth_state_dict(c, J, seed, model=model)
    return _SD[key]


def rows_of(sd, rows):
    part = dict(sd)
    part["final_layer.weight"] = np.ascontiguousarray(sd["final_layer.weight"][rows])
    part["final_layer.bias"] = np.ascontiguousarray(sd["final_layer.bias"][rows])
    return part


def fixture(pkg, name):
    g = golden(name)
    c, J, h, w, n = (int(g[k]) for k in ("c", "J", "h", "w", "n"))
    crops = pkg.synth_crops(n, h, w, seed=int(g["crop_seed"]))
    assert float(g["min_gap"]) > 2 * HM_ATOL_F32
    return g, c, J, h, w, n, crops


def check_fp32(pkg, name):
    g, c, J, h, w, n, crops = fixture(pkg, name)
    crops = torch.from_numpy(crops).cuda()
    net = pkg.NativeHRNet(c, J, (h, w), "fp32", max_batch=2, device=0).load_state_dict(sd_np(pkg, c, J, int(g["weight_seed"])))
    hm, pts = net.predict_crops(crops, g["boxes"], return_heatmaps=True)
    hm, pts = hm.cpu().numpy(), pts.cpu().numpy()
    ref_hm, ref_pts = g["heatmaps"], g["pts"].reshape(pts.shape)
    assert hm.shape == (n, J, h // 4, w // 4) and np.isfinite(hm).all()
    print("\n[fp32 %s] max|dH| = %.3g, coordinates differing: %d of %d" %
          (name, np.abs(hm - ref_hm).max(), (pts[..., :2] != ref_pts[..., :2]).any(-1).sum(), n * J))
    np.testing.assert_allclose(hm, ref_hm, rtol=0, atol=HM_ATOL_F32)
    np.testing.assert_array_equal(pts[..., :2], ref_pts[..., :2])
    np.testing.assert_allclose(pts[..., 2], ref_pts[..., 2], rtol=0, atol=HM_ATOL_F32)
    np.testing.assert_array_equal(net(crops).cpu().numpy(), hm)
    assert net.pad_violations() == 0
    net.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_fp32_matches_reference_outputs(pkg, name):
    check_fp32(pkg, name)


@pytest.mark.parametrize("name", FIXTURES)
def test_fp32_matches_reference_outputs_with_the_mfma_head_disabled(pkg, name, monkeypatch):
    assert os.environ.get("HRN_DEBUG_ENV") == "1"        # the switch is read when a handle is created, in a process that opted in
    monkeypatch.setenv("HRN_DISABLE_HEAD_MFMA", "1")
    check_fp32(pkg, name)


@pytest.mark.parametrize("head", ["mfma", "valu"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_16bit_bounded_error_and_argmax(pkg, name, dtype, head, monkeypatch):
    """head = "valu": HRN_DISABLE_HEAD_MFMA=1, the 16-bit engines on head_kernel, whose weight stage holds one joint group at a time"""
    g, c, J, h, w, n, crops = fixture(pkg, name)
    crops = torch.from_numpy(crops).cuda()
    if head == "valu":
        monkeypatch.setenv("HRN_DISABLE_HEAD_MFMA", "1")
    else:
        monkeypatch.delenv("HRN_DISABLE_HEAD_MFMA", raising=False)
    net = pkg.NativeHRNet(c, J, (h, w), dtype, max_batch=4, device=0).load_state_dict(sd_np(pkg, c, J, int(g["weight_seed"])))
    hm, pts = net.predict_crops(crops, g["boxes"], return_heatmaps=True)
    alone = net.predict_crops(crops, g["boxes"])
    assert torch.equal(alone, pts)                                       # the same pts bits without the heat-map output
    hm, pts = hm.cpu().numpy(), pts.cpu().numpy()
    ref_hm = g["heatmaps"]
    assert np.isfinite(hm).all()
    err = np.abs(hm - ref_hm).max()
    flat, rflat = hm.reshape(n, J, -1), ref_hm.reshape(n, J, -1)
    am, ram = flat.argmax(-1), rflat.argmax(-1)
    top2 = np.sort(rflat, -1)[..., -2:]
    gap = top2[..., 1] - top2[..., 0]
    sigma = ref_hm.std()
    print("\n[%s %s %s] max|dH|=%.4f (sigma %.2f)  argmax agree %d/%d" % (dtype, head, name, err, sigma, (am == ram).sum(), am.size))
    assert err < 0.05 * sigma + 0.05
    assert (am == ram)[gap > 4 * err].all()
    np.testing.assert_array_equal(pts[..., :2], T.decode_heatmaps(hm, g["boxes"])[..., :2])
    np.testing.assert_array_equal(pts[..., 2], flat.max(-1))
    net.close()


INVARIANT_SHAPES = [(32, 64, 64, 3, 2), (48, 384, 288, 3, 2), (48, 128, 96, 5, 8), (48, 384, 288, 30, 30)]   # (c, h, w, n, max_batch)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("c,h,w,n,mb", INVARIANT_SHAPES)
def test_a_joint_does_not_depend_on_the_other_joints(pkg, dtype, c, h, w, n, mb):
    """joints [32g, 32g + 32) of the 133-joint engine against an engine that holds only those rows of final_layer (the last
    one has 5 joints): heat-maps and pts bit-equal.  384x288 at n = 3 runs the head on 27 slabs of 256 pixels per crop (the
    small-call split), at n = 30 on 7 slabs of 1024; 128x96 at n = 5 with max_batch 8 is one chunk, 64x64 at max_batch 2 two"""
    J = 133
    sd = sd_np(pkg, c, J, 2)
    crops = torch.from_numpy(pkg.synth_crops(n, h, w, seed=11)).cuda()
    boxes = pkg.synth_boxes(n, seed=5)
    full = pkg.NativeHRNet(c, J, (h, w), dtype, max_batch=mb, device=0).load_state_dict(sd)
    hm, pts = full.predict_crops(crops, boxes, return_heatmaps=True)
    assert torch.equal(full.predict_crops(crops, boxes), pts)
    for g in range((J + 31) // 32):
        rows = slice(32 * g, min(32 * g + 32, J))
        part = pkg.NativeHRNet(c, rows.stop - rows.start, (h, w), dtype, max_batch=mb, device=0).load_state_dict(rows_of(sd, rows))
        assert part.launches_per_pass() == full.launches_per_pass()
        hm_g, pts_g = part.predict_crops(crops, boxes, return_heatmaps=True)
        assert torch.equal(hm_g, hm[:, rows]), "group %d: heat-maps differ" % g
        assert torch.equal(pts_g, pts[:, rows]), "group %d: pts differ" % g
        part.close()
    assert full.pad_violations() == 0
    full.close()


def test_a_joint_does_not_depend_on_the_other_joints_without_the_mfma_head(pkg, monkeypatch):
    J, c, h, w, n = 133, 32, 128, 96, 3
    sd = sd_np(pkg, c, J, 2)
    crops = torch.from_numpy(pkg.synth_crops(n, h, w, seed=11)).cuda()
    boxes = pkg.synth_boxes(n, seed=5)
    monkeypatch.setenv("HRN_DISABLE_HEAD_MFMA", "1")
    full = pkg.NativeHRNet(c, J, (h, w), "bf16", max_batch=2, device=0).load_state_dict(sd)
    hm, pts = full.predict_crops(crops, boxes, return_heatmaps=True)
    for g in (0, 3, 4):
        rows = slice(32 * g, min(32 * g + 32, J))
        part = pkg.NativeHRNet(c, rows.stop - rows.start, (h, w), "bf16", max_batch=2, device=0).load_state_dict(rows_of(sd, rows))
        hm_g, pts_g = part.predict_crops(crops, boxes, return_heatmaps=True)
        assert torch.equal(hm_g, hm[:, rows]) and torch.equal(pts_g, pts[:, rows])
        part.close()
    full.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_subpixel_decoding_at_133_joints(pkg, dtype):
    c, J, h, w, n = 32, 133, 128, 96, 3
    net = pkg.NativeHRNet(c, J, (h, w), dtype, max_batch=2, device=0).load_state_dict(sd_np(pkg, c, J, 9))
    crops = torch.from_numpy(pkg.synth_crops(n, h, w, seed=11)).cuda()
    boxes = pkg.synth_boxes(n, seed=7)
    hm0, pts0 = net.predict_crops(crops, boxes, return_heatmaps=True)
    hm = hm0.cpu().numpy()
    np.testing.assert_array_equal(pts0.cpu().numpy(), R.decode(hm, boxes, None))
    for mode in ("quarter", "dark"):
        hmr, pts = net.predict_crops(crops, boxes, return_heatmaps=True, refine=mode)
        assert torch.equal(hmr, hm0)
        assert torch.equal(net.predict_crops(crops, boxes, refine=mode), pts)       # the head writes into the handle's scratch
        pts, want = pts.cpu().numpy(), R.decode(hm, boxes, mode)
        np.testing.assert_array_equal(pts[..., 2], want[..., 2])
        if mode == "quarter":
            np.testing.assert_array_equal(pts, want)
            assert (np.abs(pts[..., :2] - pts0.cpu().numpy()[..., :2]).max(-1) > 0).sum() > J
        else:
            check_dark(hm, _cells(pts, boxes, h, w), _cells(want, boxes, h, w), "J=133 %s" % dtype)
    # refine_coords on the same maps
    idx = hm.reshape(n, J, -1).argmax(-1)
    coords = np.stack([idx % (w // 4), idx // (w // 4)], -1).astype(np.float32)
    q = net.refine_coords(hm0, coords, "quarter").cpu().numpy()
    np.testing.assert_array_equal(q, R.refine_coords(hm, coords, "quarter"))
    d = net.refine_coords(hm0, coords, "dark").cpu().numpy()
    check_dark(hm, d, R.refine_coords(hm, coords, "dark"), "refine_coords J=133 %s" % dtype)
    # predict_stream: the same joints batch by batch
    host_crops = crops.cpu()
    batches = [(host_crops[:2], boxes[:2]), (host_crops[2:], boxes[2:])]
    got = [p.cpu().numpy() for p in net.predict_stream(batches, refine="quarter")]
    np.testing.assert_array_equal(np.concatenate(got), R.decode(hm, boxes, "quarter"))
    net.close()


def tta_fixture(pkg):
    g = golden(TTA)
    g["heatmaps"] = np.concatenate([g["heatmaps"], golden(TTA + "_b")["heatmaps"]])
    c, J, h, w, n = (int(g[k]) for k in ("c", "J", "h", "w", "n"))
    assert g["heatmaps"].shape == (n, J, h // 4, w // 4) and float(g["min_gap"]) > 2 * HM_ATOL_F32
    return g, c, J, h, w, n, torch.from_numpy(pkg.synth_crops(n, h, w, seed=int(g["crop_seed"]))).cuda()


def test_oracle_flip_tta_matches_the_133_joint_fixture(pkg):
    g, c, J, h, w, n, crops = tta_fixture(pkg)
    sd = pkg.synth.to_torch_state_dict(sd_np(pkg, c, J, int(g["weight_seed"])))
    hm = T.flip_tta_heatmaps(sd, crops.cpu(), g["flip_pairs"].tolist()).numpy()
    np.testing.assert_allclose(hm, g["heatmaps"], rtol=0, atol=1e-6)
    preds, maxvals = T.max_preds_refined(g["heatmaps"], True)
    np.testing.assert_array_equal(preds, g["preds"])
    np.testing.assert_array_equal(maxvals, g["maxvals"])


@pytest.mark.parametrize("mb", [2, 8])
def test_flip_tta_fp32_matches_reference(pkg, mb):
    g, c, J, h, w, n, crops = tta_fixture(pkg)
    pairs = g["flip_pairs"]
    assert len(np.unique(pairs)) == pairs.size == 120 and pairs.max() >= 128
    net = pkg.NativeHRNet(c, J, (h, w), "fp32", max_batch=mb, device=0).load_state_dict(sd_np(pkg, c, J, int(g["weight_seed"])))
    hm, preds, maxvals = net.predict_flip_tta(crops, pairs)
    hm, preds, maxvals = hm.cpu().numpy(), preds.cpu().numpy(), maxvals.cpu().numpy()
    np.testing.assert_allclose(hm, g["heatmaps"], rtol=0, atol=2e-4)
    np.testing.assert_allclose(maxvals, g["maxvals"], rtol=0, atol=2e-4)
    ref_preds, ref_max = T.max_preds_refined(hm, True)
    np.testing.assert_array_equal(preds, ref_preds)
    np.testing.assert_array_equal(maxvals, ref_max)
    same = np.abs(preds - g["preds"]) < 1e-6
    assert same.mean() > 0.97 and np.abs(preds - g["preds"]).max() <= 0.5
    raw = net.predict_flip_tta(crops, pairs, post_processing=False)[1].cpu().numpy()
    np.testing.assert_array_equal(raw, g["preds_nopost"])
    assert tuple(net.predict_flip_tta(torch.zeros((0, 3, h, w)).cuda(), [])[1].shape) == (0, J, 2)
    net.close()


def test_flip_tta_bf16_bounded_and_dark(pkg):
    g, c, J, h, w, n, crops = tta_fixture(pkg)
    net = pkg.NativeHRNet(c, J, (h, w), "bf16", max_batch=4, device=0).load_state_dict(sd_np(pkg, c, J, int(g["weight_seed"])))
    hm_t, preds, maxvals = net.predict_flip_tta(crops, g["flip_pairs"])
    hm = hm_t.cpu().numpy()
    assert np.abs(hm - g["heatmaps"]).max() < 0.05 * g["heatmaps"].std() + 0.05
    np.testing.assert_array_equal(preds.cpu().numpy(), T.max_preds_refined(hm, True)[0])
    raw = net.predict_flip_tta(crops, g["flip_pairs"], post_processing=False)[1].cpu().numpy()
    dark = net.predict_flip_tta(crops, g["flip_pairs"], post_processing="dark")[1].cpu().numpy()
    check_dark(hm, dark, R.refine_coords(hm, raw, "dark"), "flip-TTA J=133 bf16")
    net.close()


def test_flip_pair_tables_are_checked_before_anything_is_launched(pkg):
    """an index >= J (or < 0) fails with code 7 and untouched outputs.  Pairs that share a joint -- a table listing a pair
    twice among them -- are NOT an error: they compose in order as flip_back's in-place swaps do, which is what the
    17-joint engine has always done (tests/test_round2_gpu.py); the same holds past 32 joints."""
    c, J, h, w, n = 32, 133, 64, 64, 2
    sd = sd_np(pkg, c, J, 9)
    net = pkg.NativeHRNet(c, J, (h, w), "fp32", max_batch=2, device=0).load_state_dict(sd)
    crops = torch.from_numpy(pkg.synth_crops(n, h, w, seed=13)).cuda()
    hm = torch.full((n, J, h // 4, w // 4), 7.0, device="cuda")
    preds = torch.full((n, J, 2), 7.0, device="cuda")
    mv = torch.full((n, J), 7.0, device="cuda")
    for bad in ([[1, 2], [40, J]], [[-1, 3]], [[130, 133]], [[5, 256]]):
        fp = np.ascontiguousarray(bad, np.int32)
        rc = net._lib.hrn_forward_flip_tta(net._h, crops.data_ptr(), n, fp.ctypes.data, len(fp), 1, hm.data_ptr(), preds.data_ptr(),
                                           mv.data_ptr(), None)
        assert rc == 7 and b"flip pair" in net._lib.hrn_last_error(net._h), bad
        with pytest.raises(RuntimeError, match="flip pair"):
            net.predict_flip_tta(crops, bad)
    torch.cuda.synchronize()
    assert bool((hm == 7).all()) and bool((preds == 7).all()) and bool((mv == 7).all())          # nothing was launched
    shared = [(1, 2), (2, 3), (100, 132), (100, 132), (40, 131), (131, 64)]
    ref = T.flip_tta_heatmaps(pkg.synth.to_torch_state_dict(sd), crops.cpu(), shared).numpy()
    got = net.predict_flip_tta(crops, shared)[0].cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-4)
    net.close()


def score_fixture():
    g = golden("j133_score_case")
    out_nan = g["plain_output"].copy()
    for (i, j), m in zip(g["nan_maps_index"], g["nan_maps"]):
        out_nan[i, j] = m
    return g, {"plain": g["plain_output"], "nan": out_nan}


@pytest.mark.parametrize("tag", ["plain", "nan"])
@pytest.mark.parametrize("topk", [8, 40])
def test_scoring_at_133_joints(pkg, tag, topk):
    g, outputs = score_fixture()
    n, J, h, w = (int(g[k]) for k in ("n", "J", "h", "w"))
    assert topk in g["topk"].tolist() and outputs[tag].shape == (n, J, h, w)
    sigma, thr = int(g["sigma"]), float(g["thr"])
    net = pkg.NativeHRNet(32, J, (4 * h, 4 * w), "fp32", max_batch=2, device=0)
    out = torch.from_numpy(outputs[tag]).cuda()
    jt, vis, jw = g["joints"], g["vis"], g["joints_weight"]
    bound = 2.0 * (n * h * w + J + 4) * 2.0 ** -53
    # the targets: the restatement's bits, the reference's support and weights
    tgt, tw = net.generate_targets(jt, vis, sigma=sigma, joints_weight=jw)
    want_t, want_tw = SR.generate_targets(jt, vis, (h, w), sigma, jw)
    same_bits(tgt.cpu().numpy(), want_t, "targets")
    np.testing.assert_array_equal(tw, g["target_weight"])
    np.testing.assert_array_equal(tgt.cpu().numpy() != 0, g["target"] != 0)
    assert SR.ulp_distance(tgt.cpu().numpy(), g["target"]).max() <= int(golden("score_cases")["g_ulps"]) + 1
    # analytic and maps mode: the same bits, and the restatement
    a = host(net.score_heatmaps(out, joints=jt, visibility=vis, sigma=sigma, joints_weight=jw, thr=thr, topk=topk))
    m = host(net.score_heatmaps(out, targets=tgt, target_weight=tw, thr=thr, topk=topk))
    for key in a:
        same_bits(a[key], m[key], "analytic vs maps: " + key)
    want = SR.score(outputs[tag], joints=jt, vis=vis, sigma=sigma, joints_weight=jw, thr=thr, topk=topk)
    check_losses(a, want["map_loss"], want["loss"], want["loss_ohkm"], bound, "restatement")
    check_pck(a, want, "restatement")
    same_bits(a["dists"], want["dists"], "dists")
    # maps mode on the reference's own targets against the reference's numbers
    r = host(net.score_heatmaps(out, targets=g["target"], target_weight=g["target_weight"], thr=thr, topk=topk))
    ref = {"joints_preds": g[tag + "_pred"], "joints_target": g[tag + "_target_pred"], "accs": g[tag + "_acc"], "avg_acc": g[tag + "_avg_acc"],
           "cnt": g[tag + "_cnt"], "dists": g[tag + "_dists"]}
    check_losses(r, g[tag + "_map_loss64"], g[tag + "_loss64"], g[tag + "_ohkm64_top%d" % topk], bound, "reference")
    check_pck(r, ref, "reference, maps", dists_ulps=2)
    if tag == "plain":
        ref32, ref64 = np.float32(g["plain_loss32"]), float(g["plain_loss64"])
        assert abs(float(np.float32(r["loss"])) - float(ref32)) <= abs(float(ref32) - ref64) + float(np.spacing(ref32))
    else:
        assert np.isnan(r["loss"]) and np.isnan(r["loss_ohkm"]) and np.isnan(r["map_loss"][0, 40])
        assert np.isnan(r["maxvals"][0, 40, 0]) and (r["joints_preds"][0, 40] == 0).all() and r["maxvals"][0, 100, 0] == -np.inf
    # a map's loss is the loss of that map scored alone: one joint of a 1-joint engine, same bits
    one = pkg.NativeHRNet(32, 1, (4 * h, 4 * w), "fp32", max_batch=2, device=0)
    for i, j in ((0, 0), (0, 40), (1, 32), (2, 132), (1, 77)):
        s = host(one.score_heatmaps(out[i:i + 1, j:j + 1].contiguous(), targets=g["target"][i:i + 1, j:j + 1],
                                    target_weight=g["target_weight"][i:i + 1, j:j + 1], thr=thr))
        same_bits(s["map_loss"][0, 0], r["map_loss"][i, j], "map (%d, %d) alone" % (i, j))
        same_bits(s["maxvals"][0, 0], r["maxvals"][i, j], "maxval (%d, %d) alone" % (i, j))
    one.close()
    net.close()


def test_ohkm_topk_any_k_up_to_the_bound(pkg):
    """J = HRN_MAX_JOINTS with ties, NaNs and topk in {1, 32, 33, J}: the restatement (torch.topk's order: NaN first)"""
    J, n, h, w = MAX_JOINTS, 3, 16, 16
    rng = np.random.default_rng(8)
    out = (rng.integers(0, 4, (n, J, h, w)) / 4.0).astype(np.float32)
    tgt = (rng.integers(0, 4, (n, J, h, w)) / 4.0).astype(np.float32)
    out[:, 50:90] = tgt[:, 50:90]                     # forty tied zero losses
    out[:, 200:230] = out[:, 10:40]                   # thirty tied pairs
    tgt[:, 200:230] = tgt[:, 10:40]
    out[1, 7, 2, 2] = np.nan
    out[1, 250, 3, 3] = np.nan
    tw = np.ones((n, J), np.float32)
    net = pkg.NativeHRNet(32, J, (4 * h, 4 * w), "fp32", max_batch=2, device=0)
    for topk in (1, 32, 33, 200, J):
        s = host(net.score_heatmaps(torch.from_numpy(out).cuda(), targets=tgt, target_weight=tw, topk=topk))
        want = SR.score(out, targets=tgt, target_weight=tw, topk=topk)
        check_losses(s, want["map_loss"], want["loss"], want["loss_ohkm"], 2.0 * (n * h * w + J + 4) * 2.0 ** -53, "topk %d" % topk)
        fin = host(net.score_heatmaps(torch.from_numpy(out[[0, 2]]).cuda(), targets=tgt[[0, 2]], target_weight=tw[[0, 2]], topk=topk))
        want = SR.score(out[[0, 2]], targets=tgt[[0, 2]], target_weight=tw[[0, 2]], topk=topk)
        assert np.isfinite(fin["loss_ohkm"])
        check_losses(fin, want["map_loss"], want["loss"], want["loss_ohkm"], 2.0 * (2 * h * w + J + 4) * 2.0 ** -53, "finite, topk %d" % topk)
    net.close()


def test_poseresnet_68_joints(pkg):
    c, J, h, w, n = 50, 68, 128, 96, 2
    sd = sd_np(pkg, c, J, 3, model="PoseResNet")
    crops = pkg.synth_crops(n, h, w, seed=17)
    boxes = pkg.synth_boxes(n, seed=5)
    with torch.no_grad():
        ref = T.poseresnet_forward(pkg.synth.to_torch_state_dict(sd), torch.from_numpy(crops), c).numpy()
    assert ref.shape == (n, J, h // 4, w // 4)
    x = torch.from_numpy(crops).cuda()
    net = pkg.NativeHRNet(c, J, (h, w), "fp32", max_batch=1, device=0, model_name="PoseResNet").load_state_dict(sd)
    hm, pts = net.predict_crops(x, boxes, return_heatmaps=True)
    print("\n[PoseResNet-50 J=68 fp32] max|dH| = %.3g (sigma %.3g)" % (np.abs(hm.cpu().numpy() - ref).max(), ref.std()))
    np.testing.assert_allclose(hm.cpu().numpy(), ref, rtol=0, atol=2e-5)
    np.testing.assert_array_equal(pts.cpu().numpy()[..., :2], T.decode_heatmaps(hm.cpu().numpy(), boxes)[..., :2])
    net.close()
    net = pkg.NativeHRNet(c, J, (h, w), "bf16", max_batch=4, device=0, model_name="PoseResNet").load_state_dict(sd)
    hm, pts = net.predict_crops(x, boxes, return_heatmaps=True)
    err = np.abs(hm.cpu().numpy() - ref).max()
    print("[PoseResNet-50 J=68 bf16] max|dH| = %.3g (sigma %.3g)" % (err, ref.std()))
    assert err < 0.08 * ref.std() + 0.004, err
    np.testing.assert_array_equal(pts.cpu().numpy()[..., :2], T.decode_heatmaps(hm.cpu().numpy(), boxes)[..., :2])
    net.close()


def test_simple_hrnet_with_133_joints(pkg):
    from test_prepath import DETS_SINGLE
    from test_simple_hrnet import TableDetector, _frames

    J = 133
    frame = _frames()[0]
    model = pkg.SimpleHRNet(48, J, sd_np(pkg, 48, J, 0), resolution=(128, 96), multiperson=True, return_heatmaps=True,
                            return_bounding_boxes=True, device="cuda:0", detector=TableDetector({0: DETS_SINGLE}))
    hm, boxes, pts = model.predict(frame)
    n = len(DETS_SINGLE)
    assert pts.shape == (n, J, 3) and hm.shape == (n, J, 32, 24) and np.asarray(boxes).shape == (n, 4)
    np.testing.assert_array_equal(pts[..., :2], T.decode_heatmaps(np.asarray(hm), np.asarray(boxes))[..., :2])
    plain = pkg.SimpleHRNet(48, J, sd_np(pkg, 48, J, 0), resolution=(128, 96), multiperson=True, device="cuda:0",
                            detector=TableDetector({0: DETS_SINGLE}))
    np.testing.assert_array_equal(plain.predict(frame), pts)
    model.model.close()
    plain.model.close()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_predict_eval_is_the_composition_at_133_joints(pkg, dtype):
    import warp_affine_ref as W
    from test_warp_gpu import _people
    from test_warp_host import _frame

    g, c_, J, h, w, _, _ = tta_fixture(pkg)
    P = pkg.postproc
    net = pkg.NativeHRNet(c_, J, (h, w), dtype, max_batch=4, device=0).load_state_dict(sd_np(pkg, c_, J, int(g["weight_seed"])))
    frames = np.stack([_frame(480, 640, 8), _frame(480, 640, 9)])
    fi = np.array([0, 1, 1, 0, 1])
    c, s = _people(5, 10)
    m = np.stack([P.affine_matrix(c[i], s[i], 200, 0, (w, h)) for i in range(5)])
    crops = torch.from_numpy(W.eval_transform(frames, m, fi, (h, w))).cuda()
    for pp in (True, False, "dark"):
        hm, preds, maxvals = net.predict_flip_tta(crops, g["flip_pairs"], post_processing=pp)
        got = net.predict_eval(frames, c, s, g["flip_pairs"], frame_index=fi, post_processing=pp)
        assert got[0].dtype == np.float32 and got[0].shape == (5, J, 2) and tuple(got[1].shape) == (5, J, 1)
        np.testing.assert_array_equal(got[0], P.final_preds(preds, c, s, 200, (w // 4, h // 4)), err_msg=str(pp))
        np.testing.assert_array_equal(got[1].cpu().numpy(), maxvals.cpu().numpy())
        np.testing.assert_array_equal(got[2].cpu().numpy(), hm.cpu().numpy())
    # score_eval = predict_eval, then score_heatmaps
    rng = np.random.default_rng(2)
    gt = c[:, None, :].astype(np.float64) + rng.uniform(-1, 1, (5, J, 2)) * (s[:, None, :] * 200 * 0.6)
    vis = (rng.uniform(0, 1, (5, J)) > 0.2).astype(np.float32)
    plain = net.predict_eval(frames, c, s, g["flip_pairs"], frame_index=fi)
    out, score = net.score_eval(frames, c, s, g["flip_pairs"], gt, np.stack([vis, vis], -1), frame_index=fi, sigma=2, thr=0.5, topk=40)
    same_bits(out[2].cpu().numpy(), plain[2].cpu().numpy(), "heat-maps")
    want = host(net.score_heatmaps(plain[2], joints=P.joints_to_crop(gt, vis, m), visibility=vis, sigma=2, thr=0.5, topk=40))
    got = host(score)
    for key in want:
        same_bits(got[key], want[key], key)
    # forward_tap: the tensor the head reads, and heat-maps beside it
    tap = net.forward_tap(crops[:2], "stem")
    assert tap.shape[0] == 2 and torch.isfinite(tap).all()
    assert net.pad_violations() == 0
    net.close()


def test_ragged_joint_counts_and_two_engines_alive(pkg):
    c, h, w, n = 32, 64, 64, 3
    crops = torch.from_numpy(pkg.synth_crops(n, h, w, seed=11)).cuda()
    boxes = pkg.synth_boxes(n, seed=5)
    alive = []
    for J in (33, 48, 64, 65, MAX_JOINTS):
        sd = sd_np(pkg, c, J, 6)
        f32 = pkg.NativeHRNet(c, J, (h, w), "fp32", max_batch=2, device=0).load_state_dict(sd)
        b16 = pkg.NativeHRNet(c, J, (h, w), "bf16", max_batch=2, device=0).load_state_dict(sd)
        alive.append((J, f32, b16))
    with torch.no_grad():
        sd = sd_np(pkg, c, 65, 6)
        oracle_hm, oracle_pts = T.predict_crops(pkg.synth.to_torch_state_dict(sd), crops.cpu(), boxes)
    results = {}
    for J, f32, b16 in alive:                     # every engine was created before any of them ran
        ref, ref_pts = f32.predict_crops(crops, boxes, return_heatmaps=True)
        hm, pts = b16.predict_crops(crops, boxes, return_heatmaps=True)
        ref, hm = ref.cpu().numpy(), hm.cpu().numpy()
        assert ref.shape == (n, J, h // 4, w // 4) and np.isfinite(hm).all()
        err, sigma = np.abs(hm - ref).max(), ref.std()
        print("\n[J = %d] bf16 against fp32: max|dH| = %.4f (sigma %.2f)" % (J, err, sigma))
        assert err < 0.05 * sigma + 0.05
        np.testing.assert_array_equal(pts.cpu().numpy()[..., :2], T.decode_heatmaps(hm, boxes)[..., :2])
        np.testing.assert_array_equal(ref_pts.cpu().numpy()[..., :2], T.decode_heatmaps(ref, boxes)[..., :2])
        results[J] = ref
    np.testing.assert_allclose(results[65], oracle_hm, rtol=0, atol=HM_ATOL_F32)
    for J, f32, b16 in alive:                     # and again, interleaved: the engines do not disturb one another
        np.testing.assert_array_equal(f32(crops).cpu().numpy(), results[J])
    for J, f32, b16 in alive:
        assert f32.pad_violations() == 0 and b16.pad_violations() == 0
        f32.close()
        b16.close()
