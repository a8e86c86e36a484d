"""Sub-pixel joint decoding on the MI355X (include/hrnet_mi355.h: HRN_REFINE_*; csrc/decode.hip) against the numpy
restatement of tests/subpixel_ref.py, run on the engine's own heat-maps.  QUARTER must be equal; DARK (fp64 on both sides)
within 1e-3 heat-map cell, except joints where another evaluation order may legitimately decide otherwise (an ill-conditioned
Hessian, a definiteness or clamp decision within 1e-5 of its threshold): those are counted, printed and kept under 2 %."""
import numpy as np
import pytest
import torch

import subpixel_ref as R
from conftest import golden, load_pkg, state_dict_np

pytestmark = pytest.mark.gpu

DARK_TOL = 1e-3   # heat-map cells


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    assert torch.cuda.is_available(), "GPU tests need a GPU: the HIP path has no CPU fallback"
    return p


def _state_dict(pkg, model, c):
    return pkg.synth_state_dict(c, 17, 0, model="PoseResNet") if model == "PoseResNet" else state_dict_np(c, 0)


def _boxes(pkg, n, kind):
    b = pkg.synth_boxes(n, seed=7)
    return b if kind == "int" else b.astype(np.float32) + np.asarray([0.25, 0.75, 0.5, 0.125], np.float32)


def _cells(pts, boxes, h, w):
    """joints (y, x) back in heat-map cells: (y - y1) / (y2 - y1) * h"""
    b = boxes.astype(np.float64)
    y = (pts[..., 0] - b[:, 1:2]) / (b[:, 3:4] - b[:, 1:2]) * h
    x = (pts[..., 1] - b[:, 0:1]) / (b[:, 2:3] - b[:, 0:1]) * w
    return np.stack([x, y], -1)


def check_dark(hm, got_cells, want_cells, tag):
    """|engine - restatement| <= DARK_TOL cell except on borderline joints (< 2 %); returns the number of borderline joints"""
    n, nj = hm.shape[:2]
    bad = np.abs(got_cells - want_cells).max(-1) > DARK_TOL
    borderline = []
    for i, j in zip(*np.nonzero(bad)):
        px, py, _ = R.argmax_xy(hm[i, j])
        assert R.borderline(hm[i, j], px, py), "%s: crop %d joint %d off by %.3g cell and not borderline" % (
            tag, i, j, np.abs(got_cells[i, j] - want_cells[i, j]).max())
        borderline.append((int(i), int(j)))
    print("\n[dark] %s: %d joints, %d borderline %s, worst |d| elsewhere %.2e cell" % (
        tag, n * nj, len(borderline), borderline, np.abs(got_cells - want_cells).max(-1)[~bad].max(initial=0.0)))
    assert len(borderline) <= 0.02 * n * nj
    return len(borderline)


CASES = [("HRNet", 32, (128, 96), "fp32", 5, 2, "int"),
         ("HRNet", 32, (128, 96), "bf16", 5, 2, "float"),
         ("HRNet", 32, (64, 64), "fp16", 3, 2, "float"),
         ("HRNet", 48, (128, 96), "bf16", 4, 4, "int"),
         ("HRNet", 48, (128, 96), "fp16", 5, 3, "int"),
         ("HRNet", 48, (64, 64), "fp32", 2, 2, "float"),
         ("PoseResNet", 50, (128, 96), "bf16", 3, 2, "int"),
         ("PoseResNet", 50, (128, 96), "fp32", 2, 2, "float")]


@pytest.mark.parametrize("model,c,res,dtype,n,mb,box", CASES)
def test_refined_decode_equals_restatement_on_engine_heatmaps(pkg, model, c, res, dtype, n, mb, box):
    h, w = res
    net = pkg.NativeHRNet(c, 17, res, dtype, max_batch=mb, device=0, model_name=model).load_state_dict(_state_dict(pkg, model, c))
    launches = net.launches_per_pass()
    crops = torch.from_numpy(pkg.synth_crops(n, h, w, seed=11)).cuda()
    boxes = _boxes(pkg, n, box)
    hm0, pts0 = net.predict_crops(crops, boxes, return_heatmaps=True)
    # refine=None: hrn_forward as it is, bit for bit
    hmn, ptsn = net.predict_crops(crops, boxes, return_heatmaps=True, refine=None)
    assert torch.equal(ptsn, pts0) and torch.equal(hmn, hm0)
    hm = hm0.cpu().numpy()
    np.testing.assert_array_equal(pts0.cpu().numpy(), R.decode(hm, boxes, None))
    for mode in ("quarter", "dark"):
        hmr, pts = net.predict_crops(crops, boxes, return_heatmaps=True, refine=mode)
        assert torch.equal(hmr, hm0)                                  # the maps do not change
        alone = net.predict_crops(crops, boxes, refine=mode)          # the head writes into the handle's scratch instead
        assert torch.equal(alone, pts)
        pts = pts.cpu().numpy()
        want = R.decode(hm, boxes, mode)
        np.testing.assert_array_equal(pts[..., 2], want[..., 2])     # confidence: the raw maximum
        if mode == "quarter":
            np.testing.assert_array_equal(pts, want)
            moved = np.abs(pts[..., :2] - pts0.cpu().numpy()[..., :2]).max(-1) > 0
            print("\n[quarter] %s W%d %s %s: %d of %d joints moved" % (model, c, dtype, box, moved.sum(), moved.size))
        else:
            check_dark(hm, _cells(pts, boxes, h, w), _cells(want, boxes, h, w), "%s-%d %s %s n=%d mb=%d" % (model, c, dtype, box, n, mb))
    assert net.launches_per_pass() == launches
    assert net.pad_violations() == 0
    net.close()


def test_refine_coords_recovers_gaussian_centres(pkg):
    """synthetic sigma-2 maps of known fractional centre through hrn_refine_coords: no joint excluded"""
    for res in ((384, 288), (256, 192), (128, 96)):
        h, w = res[0] // 4, res[1] // 4
        net = pkg.NativeHRNet(32, 17, res, "bf16", max_batch=1, device=0)
        n = 12
        maps, cx, cy = R.gaussian_maps(n * 17, h, w, np.random.default_rng([h, w, 1]))
        hm = maps.reshape(n, 17, h, w)
        idx = hm.reshape(n, 17, -1).argmax(-1)
        coords = np.stack([idx % w, idx // w], -1).astype(np.float32)
        got = net.refine_coords(torch.from_numpy(hm).cuda(), torch.from_numpy(coords).cuda(), "dark").cpu().numpy()
        err = np.abs(got - np.stack([cx, cy], -1).reshape(n, 17, 2)).max()
        print("\n[dark] %dx%d synthetic maps: worst |error| %.2e cell" % (h, w, err))
        assert err < 2e-3
        np.testing.assert_allclose(got, R.refine_coords(hm, coords, "dark"), rtol=0, atol=1e-5)
        # quarter on the same maps: equal to the restatement
        q = net.refine_coords(torch.from_numpy(hm).cuda(), torch.from_numpy(coords).cuda(), "quarter").cpu().numpy()
        np.testing.assert_array_equal(q, R.refine_coords(hm, coords, "quarter"))
        net.close()


def test_refine_coords_edge_cases_match_the_restatement(pkg):
    """flat, convex, saddle and non-positive windows (no offset), the clamp, points off the interior and off the map"""
    h, w = 32, 24
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    maps = [np.full((h, w), 0.3), 1.0 + 0.01 * ((xs - 12.3) ** 2 + (ys - 16.4) ** 2), np.exp(0.05 * ((xs - 12.3) ** 2 - (ys - 16.4) ** 2)),
            -np.exp(-((xs - 12.3) ** 2 + (ys - 16.4) ** 2) / 8), np.exp(-((xs - 15.0) ** 2 + (ys - 13.0) ** 2) / 72.0)]
    hm = np.zeros((1, 17, h, w), np.float32)
    coords = np.zeros((1, 17, 2), np.float32)
    pts = [(12, 16), (12, 16), (12, 16), (12, 16), (12, 16), (1, 16), (w - 2, 3), (12, h - 1), (-1, 5), (w, 5), (3, 2), (w - 3, h - 3)]
    for j, (px, py) in enumerate(pts):
        hm[0, j] = maps[j % len(maps)]
        coords[0, j] = (px, py)
    want = R.refine_coords(hm, coords, "dark")
    assert tuple(want[0, 4]) == (13.0, 15.0)                               # clamped: the centre is 3 cells away in x and y
    np.testing.assert_array_equal(want[0, :4], coords[0, :4])
    net = pkg.NativeHRNet(32, 17, (128, 96), "fp32", max_batch=1, device=0)
    got = net.refine_coords(torch.from_numpy(hm).cuda(), torch.from_numpy(coords).cuda(), "dark").cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
    np.testing.assert_array_equal(got[0, :4], coords[0, :4])
    assert tuple(got[0, 4]) == (13.0, 15.0)
    np.testing.assert_array_equal(net.refine_coords(torch.from_numpy(hm).cuda(), torch.from_numpy(coords).cuda(), None).cpu().numpy(),
                                  coords)
    assert tuple(net.refine_coords(torch.zeros((0, 17, 32, 24)), torch.zeros((0, 17, 2)), "dark").shape) == (0, 17, 2)
    net.close()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_refined_pts_do_not_depend_on_batch_micro_batch_or_position(pkg, dtype):
    c, h, w, n = 32, 128, 96, 6
    sd = state_dict_np(c, 0)
    crops = torch.from_numpy(pkg.synth_crops(n, h, w, seed=4)).cuda()
    boxes = _boxes(pkg, n, "float")
    perm = np.asarray([4, 0, 5, 2, 1, 3])
    for mode in ("quarter", "dark"):
        outs = []
        for mb in (1, 4, 6):
            net = pkg.NativeHRNet(c, 17, (h, w), dtype, max_batch=mb, device=0).load_state_dict(sd)
            outs.append(net.predict_crops(crops, boxes, refine=mode).cpu().numpy())
            shuffled = net.predict_crops(crops[torch.from_numpy(perm).cuda()], boxes[perm], refine=mode).cpu().numpy()
            np.testing.assert_array_equal(shuffled, outs[-1][perm])
            single = np.concatenate([net.predict_crops(crops[i:i + 1], boxes[i:i + 1], refine=mode).cpu().numpy() for i in range(n)])
            np.testing.assert_array_equal(single, outs[-1])
            net.close()
        for o in outs[1:]:
            np.testing.assert_array_equal(o, outs[0])
        # two lanes of one GPU (MultiDeviceHRNet): every range on its own handle, same joints
        md = load_pkg("native").MultiDeviceHRNet([0, 0], c, 17, (h, w), dtype, max_batch=4).load_state_dict(sd)
        np.testing.assert_array_equal(md.predict_crops(crops, boxes, refine=mode).cpu().numpy(), outs[0])
        md.close()


def test_flip_tta_dark_matches_restatement_on_averaged_maps(pkg):
    g = golden("w32_128x96_fliptta_n3")
    c, h, w = int(g["c"]), int(g["h"]), int(g["w"])
    for dtype in ("fp32", "bf16"):
        net = pkg.NativeHRNet(c, 17, (h, w), dtype, max_batch=2, device=0).load_state_dict(state_dict_np(c, int(g["weight_seed"])))
        x = torch.from_numpy(g["crops"]).cuda()
        hm, raw, mv = net.predict_flip_tta(x, g["flip_pairs"], post_processing=False)
        hmd, dark, mvd = net.predict_flip_tta(x, g["flip_pairs"], post_processing="dark")
        assert torch.equal(hmd, hm) and torch.equal(mvd, mv)
        hm, raw, dark = hm.cpu().numpy(), raw.cpu().numpy(), dark.cpu().numpy()
        want = R.refine_coords(hm, raw, "dark")
        check_dark(hm, dark, want, "flip-TTA %s" % dtype)
        # quarter through refine_coords = the flip-TTA kernel's own post-processing
        q = net.refine_coords(torch.from_numpy(hm).cuda(), torch.from_numpy(raw).cuda(), "quarter").cpu().numpy()
        np.testing.assert_array_equal(q, net.predict_flip_tta(x, g["flip_pairs"])[1].cpu().numpy())
        net.close()


def _one_cell(pts, pts0, boxes, h, w):
    """refined joints differ from the unrefined ones by at most one heat-map cell"""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    cell = np.stack([(b[:, 3] - b[:, 1]) / h, (b[:, 2] - b[:, 0]) / w], -1)[:, None, :]
    d = np.abs(pts[..., :2].astype(np.float64) - pts0[..., :2]) / cell
    assert d.max() <= 1.0 + 1e-4, d.max()
    np.testing.assert_array_equal(pts[..., 2], pts0[..., 2])
    return d


def test_predict_frame_and_simple_hrnet_refine(pkg):
    from test_prepath import DETS_BATCH, DETS_SINGLE
    from test_simple_hrnet import TableDetector, _frames

    frame = _frames()[0]
    g = golden("cfg1_w32_256x192_predict_multi")
    net = pkg.NativeHRNet(32, 17, (256, 192), "fp32", max_batch=4, device=0).load_state_dict(state_dict_np(32, 0))
    boxes, pts0 = net.predict_frame(frame, DETS_SINGLE, refine=None)
    np.testing.assert_array_equal(boxes, g["boxes"])
    np.testing.assert_array_equal(pts0.cpu().numpy()[..., :2], g["pts"][..., :2])
    for mode in ("quarter", "dark"):
        boxes, pts, hm = net.predict_frame(frame, DETS_SINGLE, return_heatmaps=True, refine=mode)
        pts = pts.cpu().numpy()
        _one_cell(pts, pts0.cpu().numpy(), boxes, 64, 48)
        if mode == "quarter":
            np.testing.assert_array_equal(pts, R.decode(hm.cpu().numpy(), boxes, "quarter"))
    net.close()

    # SimpleHRNet(refine=...): all four predict() paths
    frames = _frames()
    sd32, sd48 = state_dict_np(32, 0), state_dict_np(48, 0)
    cases = [(dict(c=32, sd=sd32, resolution=(256, 192), multiperson=True, detector=TableDetector({0: DETS_SINGLE})), frames[0],
              "cfg1_w32_256x192_predict_multi"),
             (dict(c=32, sd=sd32, resolution=(128, 96), multiperson=False), frames[1], "w32_128x96_predict_single"),
             (dict(c=48, sd=sd48, resolution=(128, 96), multiperson=False, max_batch_size=2), frames[2], "w48_128x96_predict_batch5"),
             (dict(c=32, sd=sd32, resolution=(128, 96), multiperson=True,
                   detector=TableDetector({0: DETS_BATCH[0], 1: None, 2: DETS_BATCH[2]})), frames[3], "w32_128x96_predict_batch_multi")]
    for kw, image, fixture in cases:
        kw = dict(kw)
        c, sd = kw.pop("c"), kw.pop("sd")
        ref = golden(fixture)
        h, w = kw["resolution"][0] // 4, kw["resolution"][1] // 4
        out = {}
        for mode in (None, "quarter", "dark"):
            model = pkg.SimpleHRNet(c, 17, sd, return_heatmaps=True, return_bounding_boxes=True, device="cuda:0", refine=mode, **kw)
            hm, boxes, pts = model.predict(image)
            if isinstance(pts, list):
                pts, boxes = np.concatenate(pts, 0), np.concatenate(boxes, 0)
            out[mode] = pts.reshape(-1, 17, 3), np.asarray(boxes)
            model.model.close()
        np.testing.assert_array_equal(out[None][0][..., :2], ref["pts"].reshape(-1, 17, 3)[..., :2])
        for mode in ("quarter", "dark"):
            d = _one_cell(out[mode][0], out[None][0], out[None][1], h, w)
            print("\n[SimpleHRNet %s] %s: %d joints, largest move %.3f cell" % (mode, fixture, d.shape[0] * 17, d.max()))
