"""Evaluation pre-path on the GPU: ``hrn_warp_crops`` / ``NativeHRNet.warp_crops`` against the restatement of
``cv2.warpAffine`` (``tests/warp_affine_ref.py``) BIT FOR BIT, and ``predict_eval`` against the composition it stands for --
restated crops -> the existing ``predict_flip_tta`` -> ``postproc.final_preds`` -- bit for bit as well (same kernels on the same
bits).  Parity of the restatement with a cv2 build is a matter of ``tests/test_warp_host.py``."""
import numpy as np
import pytest
import torch

import warp_affine_ref as R
from conftest import golden, load_pkg, state_dict_np
from test_warp_host import _frame, similarity

pytestmark = pytest.mark.gpu

TTA = "w32_128x96_fliptta_n3"   # flip pairs and weight seed of the flip-TTA fixture


def _matrices(frame_hw, out_hw, seed, n_random=20):
    """at least 24 forward matrices for one frame size: magnification 0.3-3, rotation 0 and +-(5..80) degrees, centres inside, at and
    beyond the border (crops partly and wholly outside), the identity, an integer and a half-pixel translation, an anisotropic map"""
    rng = np.random.default_rng(seed)
    h, w = frame_hw
    ms = []
    for k in range(n_random):
        center = (rng.uniform(-0.3 * w, 1.3 * w), rng.uniform(-0.3 * h, 1.3 * h))
        deg = 0.0 if k % 4 == 0 else rng.uniform(5, 80) * (1 if k % 2 else -1)
        ms.append(similarity(center, rng.uniform(0.3, 3.0), deg, out_hw))
    ms.append(similarity((w / 2, -0.02 * h), 1.0, 0.0, out_hw))                       # straddles the top border
    ms.append(similarity((3 * w + 500, 3 * h + 500), 1.0, 10.0, out_hw))              # wholly outside
    ms.append(similarity((-4.0 * w - 300, h / 2), 2.0, 0.0, out_hw))                  # wholly outside, left
    ms.append(np.array([[1, 0, 0], [0, 1, 0]], np.float64))                           # identity
    ms.append(np.array([[1, 0, 5], [0, 1, -3]], np.float64))                          # integer translation
    ms.append(np.array([[1, 0, -0.5], [0, 1, 0.5]], np.float64))                      # half-pixel translation
    ms.append(np.array([[0.7, 0.2, 3.25], [-0.1, 1.9, -7.5]], np.float64) @ np.diag([min(1, w / 60), min(1, h / 60), 1]))  # anisotropic, sheared
    return np.stack(ms)


@pytest.mark.parametrize("res", [(128, 96), (64, 64), (384, 288)])
def test_kernel_equals_the_restatement(res):
    pkg = load_pkg()
    H, W = res
    net = pkg.NativeHRNet(32, 17, res, "fp32", max_batch=4, device=0)
    rebuilds, launches = net.map_rebuilds(), net.launches_per_pass()
    # one frame, many crops (n far above max_batch)
    f = _frame(480, 640, 1)
    m = _matrices((480, 640), res, 11)
    assert len(m) >= 24 > net.max_batch
    got = net.warp_crops(f, matrices=m)
    assert got.shape == (len(m), 3, H, W) and got.dtype == torch.float32 and got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy(), R.eval_transform(f, m, None, res), err_msg="480x640, one frame")
    # 1080p: n = 7 crops of one device-resident frame
    f = _frame(1080, 1920, 2)
    m = _matrices((1080, 1920), res, 12, n_random=3)[[0, 1, 2, 3, 6, 8, 9]]
    got = net.warp_crops(torch.from_numpy(f).cuda(), matrices=m.reshape(7, 6))
    np.testing.assert_array_equal(got.cpu().numpy(), R.eval_transform(f, m, None, res), err_msg="1080x1920")
    # one frame per crop (nframes == n), odd frame size
    fs = np.stack([_frame(97, 61, 20 + k) for k in range(7)])
    m = _matrices((97, 61), res, 13, n_random=4)[[0, 1, 2, 3, 4, 7, 10]]
    np.testing.assert_array_equal(net.warp_crops(fs, matrices=m).cpu().numpy(), R.eval_transform(fs, m, None, res), err_msg="97x61 stack")
    # a 5x7 frame: n = 1, then every matrix of the set
    f = _frame(5, 7, 3)
    m = _matrices((5, 7), res, 14, n_random=20)
    m[:20, :, :2] *= 8                                                                  # magnify: the frame is a few pixels
    m[:20, :, 2] = np.array([W / 2, H / 2]) - np.einsum("nij,j->ni", m[:20, :, :2], [3.5, 2.5]) + np.random.default_rng(4).uniform(-20, 20, (20, 2))
    np.testing.assert_array_equal(net.warp_crops(f, matrices=m[:1]).cpu().numpy(), R.eval_transform(f, m[:1], None, res), err_msg="5x7, n=1")
    np.testing.assert_array_equal(net.warp_crops(f, matrices=m).cpu().numpy(), R.eval_transform(f, m, None, res), err_msg="5x7")
    # explicit frame_index with repeats; several calls queued without a synchronisation in between (the staging ring has 4 images)
    fs = np.stack([_frame(480, 640, 30 + k) for k in range(3)])
    calls = []
    for k in range(6):
        mk = _matrices((480, 640), res, 40 + k, n_random=2)[[0, 1, 5, 6, 7, 8, 2][:1 + k]]
        fi = np.array([2, 0, 2, 1, 1, 0, 2][:1 + k])
        calls.append((mk, fi, net.warp_crops(fs, matrices=mk, frame_index=fi)))
    for k, (mk, fi, out) in enumerate(calls):
        np.testing.assert_array_equal(out.cpu().numpy(), R.eval_transform(fs, mk, fi, res), err_msg="queued call %d" % k)
    assert net.pad_violations() == 0
    assert net.map_rebuilds() == rebuilds and net.launches_per_pass() == launches     # the pre-path plans nothing
    assert net.warp_crops(f, matrices=np.zeros((0, 2, 3))).shape == (0, 3, H, W)
    net.close()


def test_centers_scales_rotations_build_the_reference_matrices():
    pkg = load_pkg()
    P = pkg.postproc
    res = (128, 96)
    net = pkg.NativeHRNet(32, 17, res, "fp32", max_batch=4, device=0)
    f = _frame(480, 640, 5)
    rng = np.random.default_rng(6)
    boxes = np.stack([rng.uniform(-40, 560, 9), rng.uniform(-40, 400, 9), rng.uniform(20, 300, 9), rng.uniform(20, 300, 9)], 1)
    cs = [P.box_to_center_scale(b, 96 / 128) for b in boxes]
    c, s = np.stack([v[0] for v in cs]), np.stack([v[1] for v in cs])
    rot = np.array([0, 0, 0, 10.0, -25.0, 40.0, -80.0, 5.0, 0])
    m = np.stack([P.affine_matrix(c[i], s[i], 200, rot[i], (96, 128)) for i in range(9)])
    want = R.eval_transform(f, m, None, res)
    np.testing.assert_array_equal(net.warp_crops(f, c, s, rot).cpu().numpy(), want)
    m0 = np.stack([P.affine_matrix(c[i], s[i], 200, 0, (96, 128)) for i in range(9)])
    np.testing.assert_array_equal(net.warp_crops(f, c, s).cpu().numpy(), R.eval_transform(f, m0, None, res))
    np.testing.assert_array_equal(net.warp_crops(f, c, s[:, 0] * 0 + 1.5).cpu().numpy(),                       # one scale per crop
                                  R.eval_transform(f, np.stack([P.affine_matrix(c[i], 1.5, 200, 0, (96, 128)) for i in range(9)]), None, res))
    net.close()


def test_library_refuses_before_it_launches():
    pkg = load_pkg()
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=0)
    frames = torch.from_numpy(_frame(40, 50, 7)).cuda()
    out = torch.full((2, 3, 64, 64), 7.0, device="cuda")
    ident = [1.0, 0, 0, 0, 1, 0]

    def call(mats, n=2, nframes=1, fh=40, fw=50, index=None):
        m = np.ascontiguousarray(mats, np.float64)
        fi = None if index is None else np.ascontiguousarray(index, np.int32)
        return net._lib.hrn_warp_crops(net._h, frames.data_ptr(), nframes, fh, fw, None if fi is None else fi.ctypes.data, m.ctypes.data, n,
                                       out.data_ptr(), None)
    for what, rc in (("singular", call([ident, [1, 2, 0, 2, 4, 0]])), ("nan", call([ident, [1, 0, np.nan, 0, 1, 0]])),
                     ("inf", call([[np.inf, 0, 0, 0, 1, 0], ident])), ("far", call([ident, [1, 0, 3e6, 0, 1, 0]])),
                     ("tiny determinant", call([ident, [1e-200, 0, 0, 0, 1e-200, 0]])),
                     ("index high", call([ident, ident], index=[0, 1])), ("index negative", call([ident, ident], index=[-1, 0])),
                     ("frames != n", call([ident, ident], nframes=3)), ("n < 0", call([ident, ident], n=-1)),
                     ("frame too high", call([ident, ident], fh=32767)), ("frame too wide", call([ident, ident], fw=40000))):
        assert rc == 7, what
        assert net._lib.hrn_last_error(net._h)
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                        # nothing was launched
    assert call([ident, ident]) == 0
    np.testing.assert_array_equal(out.cpu().numpy(), R.eval_transform(frames.cpu().numpy(), [ident, ident], None, (64, 64)))
    net.close()


def _people(n, seed):
    P = load_pkg().postproc
    rng = np.random.default_rng(seed)
    boxes = np.stack([rng.uniform(-30, 500, n), rng.uniform(-30, 330, n), rng.uniform(60, 260, n), rng.uniform(80, 300, n)], 1)
    cs = [P.box_to_center_scale(b, 96 / 128) for b in boxes]
    return np.stack([v[0] for v in cs]), np.stack([v[1] for v in cs])


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_predict_eval_is_the_composition(dtype):
    g = golden(TTA)
    pkg = load_pkg()
    P = pkg.postproc
    from oracle import hrnet_torch_oracle as T
    c_, h, w = int(g["c"]), int(g["h"]), int(g["w"])
    sd = state_dict_np(c_, int(g["weight_seed"]))
    net = pkg.NativeHRNet(c_, 17, (h, w), dtype, max_batch=4, device=0).load_state_dict(sd)
    frames = np.stack([_frame(480, 640, 8), _frame(480, 640, 9)])
    fi = np.array([0, 1, 1, 0, 1])
    c, s = _people(5, 10)                                                             # 5 people: two passes of max_batch = 4
    m = np.stack([P.affine_matrix(c[i], s[i], 200, 0, (w, h)) for i in range(5)])
    crops = torch.from_numpy(R.eval_transform(frames, m, fi, (h, w))).cuda()
    for pp in (True, False, "dark"):
        hm, preds, maxvals = net.predict_flip_tta(crops, g["flip_pairs"], post_processing=pp)
        got = net.predict_eval(frames, c, s, g["flip_pairs"], frame_index=fi, post_processing=pp)
        assert isinstance(got[0], np.ndarray) and got[0].dtype == np.float32 and got[0].shape == (5, 17, 2)
        np.testing.assert_array_equal(got[0], P.final_preds(preds, c, s, 200, (w // 4, h // 4)), err_msg=str(pp))
        np.testing.assert_array_equal(got[1].cpu().numpy(), maxvals.cpu().numpy())
        np.testing.assert_array_equal(got[2].cpu().numpy(), hm.cpu().numpy())
        assert tuple(got[1].shape) == (5, 17, 1)
    # flip=False: one plain pass, then the reference's decode of those maps (get_max_preds + the quarter-pixel rule)
    hm = net(crops)
    for pp in (True, False):
        want_preds, want_max = T.max_preds_refined(hm.cpu().numpy(), pp)
        got = net.predict_eval(frames, c, s, g["flip_pairs"], frame_index=fi, flip=False, post_processing=pp)
        np.testing.assert_array_equal(got[0], P.final_preds(want_preds, c, s, 200, (w // 4, h // 4)), err_msg="no flip, %s" % pp)
        np.testing.assert_array_equal(got[1].cpu().numpy(), want_max)
        np.testing.assert_array_equal(got[2].cpu().numpy(), hm.cpu().numpy())
    raw = T.max_preds_refined(hm.cpu().numpy(), False)[0]
    got = net.predict_eval(frames, c, s, g["flip_pairs"], frame_index=fi, flip=False, post_processing="dark")
    np.testing.assert_array_equal(got[0], P.final_preds(net.refine_coords(hm, raw, "dark"), c, s, 200, (w // 4, h // 4)))
    assert np.abs(got[0] - P.final_preds(raw, c, s, 200, (w // 4, h // 4))).max() > 0   # the offset is exercised
    assert net.pad_violations() == 0
    net.close()


def test_predict_eval_against_the_torch_oracle():
    """the bounds of tests/test_flip_tta.py for the same oracle path: heat-maps and maxima within 2e-4, preds equal to the
    oracle's decode of the engine's own heat-maps -- here on restated crops and through the inverse affine"""
    g = golden(TTA)
    pkg = load_pkg()
    P = pkg.postproc
    from oracle import hrnet_torch_oracle as T
    c_, h, w = int(g["c"]), int(g["h"]), int(g["w"])
    sd = state_dict_np(c_, int(g["weight_seed"]))
    net = pkg.NativeHRNet(c_, 17, (h, w), "fp32", max_batch=2, device=0).load_state_dict(sd)
    frame = _frame(480, 640, 12)
    c, s = _people(3, 13)
    m = np.stack([P.affine_matrix(c[i], s[i], 200, 0, (w, h)) for i in range(3)])
    crops = R.eval_transform(frame, m, None, (h, w))
    want_hm = T.flip_tta_heatmaps(pkg.synth.to_torch_state_dict(sd), torch.from_numpy(crops), g["flip_pairs"].tolist()).numpy()
    preds, maxvals, hm = net.predict_eval(frame, c, s, g["flip_pairs"])
    hm, maxvals = hm.cpu().numpy(), maxvals.cpu().numpy()
    np.testing.assert_allclose(hm, want_hm, rtol=0, atol=2e-4)
    np.testing.assert_allclose(maxvals, T.max_preds_refined(want_hm, True)[1], rtol=0, atol=2e-4)
    ref_preds, ref_max = T.max_preds_refined(hm, True)
    np.testing.assert_array_equal(preds, P.final_preds(ref_preds, c, s, 200, (w // 4, h // 4)))
    np.testing.assert_array_equal(maxvals, ref_max)
    # joints come out in image pixels: inside the (1.25 x enlarged) box of their person
    half = s * 200 / 2
    assert (np.abs(preds - c[:, None, :]) <= half[:, None, :] + 1e-3).all()
    net.close()


def test_two_lanes_give_the_same_batch_and_joints():
    g = golden(TTA)
    pkg = load_pkg()
    c_, h, w = int(g["c"]), int(g["h"]), int(g["w"])
    sd = state_dict_np(c_, int(g["weight_seed"]))
    one = pkg.NativeHRNet(c_, 17, (h, w), "fp32", max_batch=4, device=0).load_state_dict(sd)
    two = load_pkg("native").MultiDeviceHRNet([0, 0], c_, 17, (h, w), "fp32", max_batch=4).load_state_dict(sd)
    frames = np.stack([_frame(480, 640, 14), _frame(480, 640, 15)])
    fi = np.array([0, 1, 1, 0, 1, 0, 0])
    c, s = _people(7, 16)
    a, b = one.warp_crops(frames, c, s, frame_index=fi), two.warp_crops(frames, c, s, frame_index=fi)
    assert b.device == one.torch_device
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    m = _matrices((480, 640), (h, w), 17, n_random=2)[:5]
    np.testing.assert_array_equal(one.warp_crops(frames[0], matrices=m).cpu().numpy(), two.warp_crops(frames[0], matrices=m).cpu().numpy())
    for kw in (dict(), dict(post_processing="dark"), dict(flip=False)):
        x, y = one.predict_eval(frames, c, s, g["flip_pairs"], frame_index=fi, **kw), two.predict_eval(frames, c, s, g["flip_pairs"], frame_index=fi, **kw)
        np.testing.assert_array_equal(x[0], y[0], err_msg=str(kw))
        np.testing.assert_array_equal(x[1].cpu().numpy(), y[1].cpu().numpy())
        np.testing.assert_array_equal(x[2].cpu().numpy(), y[2].cpu().numpy())
    assert tuple(two.warp_crops(frames, matrices=np.zeros((0, 6)), frame_index=np.zeros(0, np.int32)).shape) == (0, 3, h, w)
    assert all(n.pad_violations() == 0 for n in two.nets) and one.pad_violations() == 0
    one.close()
    two.close()
