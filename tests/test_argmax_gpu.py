"""The arg-max of the head, the decode and the score kernels on heat-maps with designed ties (tests/wired.py; held on the CPU
oracles by tests/test_wired_host.py).  Every case asserts the same things, with no tolerance and nothing exempted:

  1. the returned heat-maps equal the closed form bit for bit (wired cases), and hold the designed number of equal maxima;
  2. pts[..., :2] == decode_heatmaps(returned maps, boxes)[..., :2] (np.argmax: the first maximum), pts[..., 2] == the maximum's bits;
  3. the call without return_heatmaps gives the same pts;
  4. no pad violation afterwards, and a plain pass on random crops is what it was before the wired calls;

and which head kernel and slab size it ran (dtype, ``switches()``, ``hrn_plan_head_slabs``).  Not held here: a non-finite cell inside a
finite map (not designable through zero weights), and ties in ``tta_decode_kernel`` (tests/test_flip_exact_gpu.py, part C)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import score_ref as SR
import subpixel_ref as R
import wired as W
from conftest import load_pkg
from test_refine_gpu import _boxes, _cells, check_dark
from test_wired_host import check_designed_maps, check_zero_set_census, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    assert torch.cuda.is_available(), "GPU tests need a GPU: the HIP path has no CPU fallback"
    return p


def _T():
    from oracle import hrnet_torch_oracle as T
    return T


_SD = {}


def wired_sd(c, J):
    if (c, J) not in _SD:
        _SD[c, J] = (W.set_head(W.wired_state_dict(c, J, 0), W.default_mix(J), W.default_bias(J)), W.default_mix(J), W.default_bias(J))
    return _SD[c, J]


def make_net(pkg, case, sd, monkeypatch, model="HRNet"):
    monkeypatch.delenv("HRN_DISABLE_HEAD_MFMA", raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    net = pkg.NativeHRNet(case["c"], case["J"], (case["h"], case["w"]), case["dtype"], max_batch=case["max_batch"], device=0,
                          model_name=model).load_state_dict(sd)
    # which kernel and which slabs: the form from the dtype and the switches the handle saw, the slab size from the plan
    form, slab_px = W.case_walk(case)
    assert ("HRN_DISABLE_HEAD_MFMA" in net.switches()) == bool(case["env"])
    assert W.head_form(net.dtype, net.switches()) == form
    hw = (case["h"] // 4) * (case["w"] // 4)
    for k in range(0, case["n"], case["max_batch"]):
        px = ctypes.c_int32()
        slabs = net._lib.hrn_plan_head_slabs(net._h, min(case["max_batch"], case["n"] - k), ctypes.byref(px))
        assert (px.value, slabs) == (slab_px, (hw + slab_px - 1) // slab_px)
    return net, form, slab_px


def check_decode(net, crops, boxes, hm, pts):
    """2. and 3. on the maps the call returned"""
    hm, pts = hm.cpu().numpy(), pts.cpu().numpy()
    np.testing.assert_array_equal(pts[..., :2], _T().decode_heatmaps(hm, boxes)[..., :2])
    assert same_bits(pts[..., 2], hm.reshape(hm.shape[0], hm.shape[1], -1).max(-1))
    assert torch.equal(net.predict_crops(crops, boxes).cpu(), torch.from_numpy(pts))
    return hm, pts


@pytest.mark.parametrize("case", W.gpu_cases(), ids=W.case_id)
def test_designed_ties_decode_to_the_first_maximum(pkg, case, monkeypatch):
    t0 = time.time()
    c, J, h, w, n = case["c"], case["J"], case["h"], case["w"], case["n"]
    sd, mix, bias = wired_sd(c, J)
    net, form, slab_px = make_net(pkg, case, sd, monkeypatch)
    ds = W.designs(h // 4, w // 4, slab_px, form)
    boxes = _boxes(pkg, n, case["boxes"])
    rand = torch.from_numpy(pkg.synth_crops(3, h, w, seed=5)).cuda()
    before = net(rand)
    for first in range(0, len(ds), n * W.S):
        planes, idx = W.planes_for(ds, n, h // 4, w // 4, first)
        crops = torch.from_numpy(W.wired_crops(planes, h, w)).cuda()
        hm, pts = net.predict_crops(crops, boxes, return_heatmaps=True)
        hm, pts = check_decode(net, crops, boxes, hm, pts)
        check_designed_maps(hm, ds, idx, mix, bias, planes)                                   # 1.
        if n <= 5:   # decode_kernel<RF_QUARTER> merges the slabs like decode_kernel<RF_NONE>: twins, edges and blobs, exactly
            hmq, ptsq = net.predict_crops(crops, boxes, return_heatmaps=True, refine="quarter")
            assert same_bits(hmq.cpu().numpy(), hm)
            np.testing.assert_array_equal(ptsq.cpu().numpy(), R.decode(hm, boxes, "quarter"))
    assert net.pad_violations() == 0                                                          # 4.
    assert torch.equal(net(rand), before)
    per = {k: sum(d.cls == k for d in ds) for k in W.CLASSES}
    print("\n[argmax] %-40s %-28s slab_px %4d  designs %2d  twins per class %s  %.1f s" % (
        W.case_id(case), W.head_kernel_name(net.dtype, net.switches(), J), slab_px, len(ds), per, time.time() - t0))
    net.close()


@pytest.mark.parametrize("dtype,h,w", [("bf16", 64, 96), ("fp32", 160, 128)])
def test_dark_decode_takes_the_first_of_two_equal_blobs(pkg, dtype, h, w, monkeypatch):
    """decode_kernel<RF_DARK> on maps of two equal blobs in different slabs, through the rule of tests/test_refine_gpu.py"""
    case = dict(c=32, J=17, h=h, w=w, n=3, max_batch=3, dtype=dtype, env={})
    sd, mix, bias = wired_sd(32, 17)
    net, form, slab_px = make_net(pkg, case, sd, monkeypatch)
    ds = [d for d in W.designs(h // 4, w // 4, slab_px, form) if d.name == "blobs"]
    second = int(np.flatnonzero(ds[0].plane == 7)[1])
    assert W.tie_class(ds[0].cell, second, ds[0].plane.size, slab_px, form) == "slab"
    planes, idx = W.planes_for(ds, 3, h // 4, w // 4)
    crops = torch.from_numpy(W.wired_crops(planes, h, w)).cuda()
    boxes = _boxes(pkg, 3, "float")
    hm, pts0 = net.predict_crops(crops, boxes, return_heatmaps=True)
    hm, _ = check_decode(net, crops, boxes, hm, pts0)
    check_designed_maps(hm, ds, idx, mix, bias, planes)
    pts = net.predict_crops(crops, boxes, refine="dark").cpu().numpy()
    want = R.decode(hm, boxes, "dark")
    assert same_bits(pts[..., 2], want[..., 2])
    check_dark(hm, _cells(pts, boxes, h // 4, w // 4), _cells(want, boxes, h // 4, w // 4), "blobs %s %dx%d" % (dtype, h, w))
    moved = np.abs(pts[..., :2] - pts0.cpu().numpy()[..., :2]).max(-1) > 0
    assert moved.any()                              # the asymmetric blob does move its joints: the offset was taken somewhere
    assert net.pad_violations() == 0
    net.close()


ZERO_SET = [("PoseResNet", 50, 64, 128, 96, 2, "bf16"), ("PoseResNet", 50, 64, 128, 96, 2, "fp32"), ("HRNet", 32, 133, 64, 96, 2, "bf16")]


@pytest.mark.parametrize("model,c,J,h,w,n,dtype", ZERO_SET)
def test_zero_set_heads_decode_to_the_first_maximum(pkg, model, c, J, h, w, n, dtype, monkeypatch):
    """the selection runs on the engine's own tap; PoseResNet: the c = 256 head (MFMA in bf16, the one-group weight stage of
    head_groups_kernel in fp32)"""
    t0 = time.time()
    case = dict(c=c, J=J, h=h, w=w, n=n, max_batch=n, dtype=dtype, env={})
    sd = pkg.synth_state_dict(c, J, 0, model=model)
    crops = torch.from_numpy(pkg.synth_crops(n, h, w, seed=1)).cuda()
    boxes = _boxes(pkg, n, "int")
    net, form, slab_px = make_net(pkg, case, sd, monkeypatch, model)
    x = net.forward_tap(crops, W.HEAD_TAP[model]).cpu().numpy()
    net.close()
    assert x.min() >= 0                                                  # post-ReLU
    weight, masks = W.zero_set_heads(x, J)
    bias = W.default_bias(J)
    net, form, slab_px = make_net(pkg, case, W.zero_set_state_dict(sd, weight, bias), monkeypatch, model)
    before = net(crops.flip(0))
    hm, pts = net.predict_crops(crops, boxes, return_heatmaps=True)
    hm, _ = check_decode(net, crops, boxes, hm, pts)
    line = check_zero_set_census(hm, bias, masks, slab_px, form, "%s-%d J=%d %dx%d n=%d %s engine" % (model, c, J, h, w, n, dtype))
    assert net.pad_violations() == 0
    assert torch.equal(net(crops.flip(0)), before)
    print("[argmax] %s  %s  %.1f s" % (W.head_kernel_name(net.dtype, net.switches(), J), line, time.time() - t0))
    net.close()


_SCORE_NETS = {}


@pytest.mark.parametrize("J", [17, 133])
@pytest.mark.parametrize("h,w", [(16, 16), (64, 48), (96, 72)])
def test_score_argmax_takes_the_first_maximum(pkg, h, w, J):
    """block_argmax and the scan of score_kernel: ties across the cells of a float4, across threads, waves and trips; both target
    modes, and once the targets' own arg-max (maps mode) on the same tied maps"""
    ds = W.score_designs(h, w)
    assert {d.cls for d in ds if d.cls} == ({"cell", "thread"} if h * w <= 256 else {"cell", "thread", "wave", "trip"})
    n = (2 * len(ds) + J - 1) // J + 1
    maps = np.stack([ds[k % len(ds)].plane for k in range(n * J)]).reshape(n, J, h, w)
    cells = np.asarray([ds[k % len(ds)].cell for k in range(n * J)]).reshape(n, J)
    assert np.array_equal(maps.reshape(n, J, -1).argmax(-1), cells) and (W.tie_counts(maps) >= 1).all()
    net = pkg.NativeHRNet(32, J, (4 * h, 4 * w), "fp32", max_batch=2, device=0)
    rng = np.random.default_rng([h, w, J])
    joints = rng.uniform(0, 4 * min(h, w), (n, J, 2))
    vis = (rng.uniform(size=(n, J)) > 0.2).astype(np.float32)
    want_preds = np.stack([cells % w, cells // w], -1).astype(np.float32)
    a = {k: v.cpu().numpy() for k, v in net.score_heatmaps(torch.from_numpy(maps).cuda(), joints=joints, visibility=vis).items()}
    ref = SR.score(maps, joints=joints, vis=vis)
    targets = np.ascontiguousarray(maps[::-1, ::-1])                     # other tied maps per (person, joint): the targets' arg-max
    tw = np.ones((n, J, 1), np.float32)
    m = {k: v.cpu().numpy() for k, v in net.score_heatmaps(torch.from_numpy(maps).cuda(), targets=targets, target_weight=tw).items()}
    refm = SR.score(maps, targets=targets, target_weight=tw)
    for got, want in ((a, ref), (m, refm)):
        np.testing.assert_array_equal(got["joints_preds"], want_preds)
        assert same_bits(got["joints_preds"], want["joints_preds"]) and same_bits(got["maxvals"], want["maxvals"])
        assert same_bits(got["joints_target"], want["joints_target"])
    np.testing.assert_array_equal(m["joints_target"], want_preds[::-1, ::-1])
    net.close()
