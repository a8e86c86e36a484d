"""Flip test-time augmentation (``predict_flip_tta``: csrc/hrnet_mi355.cpp hrn_forward_flip_tta, the ``flip`` reads of the five stem
kernels, csrc/decode.hip tta_decode_kernel) pinned exactly.

A. The mirrored pass differs from the plain pass in the stem's column index only, so on any engine the mirrored pass on ``X`` is
   the plain pass on the host-flipped crops, bit for bit; the combine is one fp32 addition and a multiplication by 0.5.  Hence,
   with ``a = net(X)`` and ``b = net(X[..., ::-1])``,  ``predict_flip_tta(X, pairs)[0] == (a + flip_back(b, pairs)) * 0.5``  with
   tolerance ZERO -- in fp32, bf16 and fp16, for HRNet and PoseResNet, every stem kernel (fused stem, stem_mfma_kernel, stem_kernel,
   stem7_mfma_kernel, stem7_kernel), crop widths 32 .. 320 and map sizes 8x8 .. 96x72, ragged micro-batches.  The decode is numpy's
   decode of those maps (tests/flip_ref.py).  Each case asserts which stem kernel its engine runs.
B. Against the independent fp32 reference (the oracle), with the tolerances the plain pass already has.
C. Adversarial maps through tta_decode_kernel: exact ties between cells (crops that equal their mirror image: tests/test_flip_ref.py
   shows on the CPU that each self-paired map then holds its maximum exactly twice), and NaN / -inf / constant maps from the real head.
   (Not constructed: a map with +inf next to its maximum -- numpy's sign(inf - inf) is NaN there, the kernel steps by 0.)"""
import os

import numpy as np
import pytest
import torch

import flip_ref as F
from conftest import golden, load_pkg
from oracle import hrnet_torch_oracle as T

pytestmark = pytest.mark.gpu

HM_ATOL_F32 = 2e-4          # HRNet fp32 against the oracle (tests/test_flip_tta.py, tests/test_joints_gpu.py)
RESNET_ATOL_F32 = 2e-5      # PoseResNet fp32 against the oracle (tests/test_poseresnet.py)
FUSE_OFF, MFMA_OFF = "HRN_DISABLE_STEM_FUSE", "HRN_DISABLE_STEM_MFMA"


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    assert torch.cuda.is_available(), "GPU tests need a GPU: the HIP path has no CPU fallback"
    return p


_SD = {}


def sd_np(pkg, model, c, joints, seed=0):
    key = (model, c, joints, seed)
    if key not in _SD:
        _SD[key] = pkg.synth_state_dict(c, joints, seed, model=model)
    return _SD[key]


def engine(pkg, monkeypatch, model, c, joints, hw, dtype, mb, switch=None, fused=False, sd=None):
    """one engine with exactly ``switch`` set (the switches are read when the handle is created), checked to be the plan meant"""
    for k in [k for k in os.environ if k.startswith("HRN_") and k != "HRN_DEBUG_ENV"]:
        monkeypatch.delenv(k)
    if switch:
        monkeypatch.setenv(switch, "1")
    net = pkg.NativeHRNet(c, joints, hw, dtype, max_batch=mb, device=0, model_name=model)
    net.load_state_dict(sd if sd is not None else sd_np(pkg, model, c, joints))
    assert net.switches() == (switch + "=1;" if switch else ""), net.switches()
    assert net.stem_fused() == fused, "this case is meant to run %s the fused stem" % ("on" if fused else "without")
    return net


def host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def check_identity(net, x, pairs):
    """the identity of the header on one engine; returns the averaged maps"""
    x = x.cuda()
    a, b = host(net(x), net(torch.flip(x, dims=[-1]).contiguous()))
    want = F.flip_tta_expected(a, b, pairs)
    hm = None
    for pp in (True, False):
        hm, preds, maxvals = host(*net.predict_flip_tta(x, pairs, post_processing=pp))
        np.testing.assert_array_equal(hm, want)
        ref_preds, ref_max = F.max_preds(hm, pp)
        np.testing.assert_array_equal(preds, ref_preds)
        np.testing.assert_array_equal(maxvals, ref_max)
        assert net.pad_violations() == 0
    np.testing.assert_array_equal(net(x).cpu().numpy(), a)        # the scratch maps and the workspace are shared
    assert np.isfinite(a).all() and np.abs(a - b[..., ::-1]).max() > 0        # (not a degenerate case: the passes differ)
    return hm


# ------------------------------------------------------------------------------------------------------------ A. the identity
HRNET_CASES = [
    # (dtype, switch, fused, c, H, W, n, max_batch)                                     the stem kernel exercised
    ("bf16", None, True, 48, 32, 32, 7, 4),                                            # stem_fused_kernel
    ("bf16", None, True, 32, 128, 96, 4, 4),
    ("bf16", None, True, 48, 96, 160, 3, 2),
    ("bf16", None, True, 32, 96, 288, 3, 2),
    ("bf16", None, True, 32, 160, 224, 2, 2),
    ("bf16", None, True, 48, 224, 32, 2, 1),
    ("bf16", None, False, 32, 64, 320, 2, 2),                                          # too wide to fuse: stem_mfma_kernel
    ("bf16", FUSE_OFF, False, 48, 32, 32, 7, 4),                                       # stem_mfma_kernel
    ("bf16", FUSE_OFF, False, 32, 96, 288, 3, 2),
    ("bf16", FUSE_OFF, False, 32, 160, 224, 2, 2),
    ("bf16", MFMA_OFF, False, 32, 64, 96, 5, 2),                                       # stem_kernel<bf16>
    ("fp16", None, True, 32, 128, 96, 3, 2),                                           # the fused stem in fp16
    ("fp16", None, True, 48, 224, 32, 2, 1),
    ("fp32", None, False, 32, 32, 32, 3, 2),                                           # stem_kernel<fp32>
    ("fp32", None, False, 32, 64, 96, 5, 2),
    ("fp32", None, False, 32, 96, 32, 1, 4),
    ("fp32", None, False, 32, 128, 160, 2, 2),
    ("bf16", None, True, 48, 384, 288, 3, 2),                                          # 96x72 maps: 27 trips of the decode's scan
]


@pytest.mark.parametrize("dtype,switch,fused,c,h,w,n,mb", HRNET_CASES)
def test_hrnet_flip_tta_is_the_two_plain_passes_exactly(pkg, monkeypatch, dtype, switch, fused, c, h, w, n, mb):
    net = engine(pkg, monkeypatch, "HRNet", c, 17, (h, w), dtype, mb, switch, fused)
    check_identity(net, torch.from_numpy(pkg.synth_crops(n, h, w, seed=51)), F.COCO_PAIRS)
    net.close()


@pytest.mark.parametrize("joints,pairs", [(16, "none"), (133, "fixture"), (17, "shared")])
def test_hrnet_flip_tta_identity_joint_counts_and_pair_tables(pkg, monkeypatch, joints, pairs):
    """the head's joint groups (16, 133 = four groups of 32 and a ragged one) and the composition of pairs that share a joint"""
    pairs = {"none": [], "shared": F.SHARED_PAIRS, "fixture": golden("j133_w32_128x96_fliptta_n3")["flip_pairs"].tolist()}[pairs]
    net = engine(pkg, monkeypatch, "HRNet", 32, joints, (64, 64), "bf16", 2, None, True)
    check_identity(net, torch.from_numpy(pkg.synth_crops(2, 64, 64, seed=52)), pairs)
    net.close()


RESNET_CASES = [
    # (dtype, switch, H, W, n, max_batch)
    ("fp32", None, 32, 32, 3, 2),                                                      # stem7_kernel<fp32>
    ("fp32", None, 128, 96, 3, 2),
    ("fp32", None, 64, 160, 2, 1),
    ("bf16", None, 32, 32, 3, 2),                                                      # stem7_mfma_kernel
    ("bf16", None, 128, 96, 5, 2),
    ("bf16", None, 64, 160, 2, 1),
    ("fp16", None, 32, 32, 3, 2),
    ("fp16", None, 128, 96, 5, 2),
    ("fp16", None, 64, 160, 2, 1),
    ("bf16", MFMA_OFF, 128, 96, 3, 2),                                                 # stem7_kernel<bf16>
]


@pytest.mark.parametrize("dtype,switch,h,w,n,mb", RESNET_CASES)
def test_poseresnet_flip_tta_is_the_two_plain_passes_exactly(pkg, monkeypatch, dtype, switch, h, w, n, mb):
    net = engine(pkg, monkeypatch, "PoseResNet", 50, 17, (h, w), dtype, mb, switch)
    check_identity(net, torch.from_numpy(pkg.synth_crops(n, h, w, seed=53)), F.COCO_PAIRS)
    net.close()


# ------------------------------------------------------------------------------------- B. against the independent fp32 reference
@pytest.mark.parametrize("h,w", [(128, 96), (32, 32)])
def test_poseresnet_fp32_flip_tta_meets_the_oracle(pkg, monkeypatch, h, w):
    x = torch.from_numpy(pkg.synth_crops(3, h, w, seed=54))
    sd = pkg.synth.to_torch_state_dict(sd_np(pkg, "PoseResNet", 50, 17))
    with torch.no_grad():
        a = T.poseresnet_forward(sd, x, 50).numpy()
        b = T.poseresnet_forward(sd, torch.flip(x, dims=[-1]), 50).numpy()
    ref = F.flip_tta_expected(a, b, F.COCO_PAIRS)
    net = engine(pkg, monkeypatch, "PoseResNet", 50, 17, (h, w), "fp32", 2)
    hm, preds, maxvals = host(*net.predict_flip_tta(x.cuda(), F.COCO_PAIRS))
    np.testing.assert_allclose(hm, ref, rtol=0, atol=RESNET_ATOL_F32)
    ref_preds, ref_max = F.max_preds(hm)
    np.testing.assert_array_equal(preds, ref_preds)
    np.testing.assert_array_equal(maxvals, ref_max)
    net.close()


@pytest.mark.parametrize("h,w", [(32, 32), (64, 96)])
def test_hrnet_fp32_flip_tta_meets_the_oracle(pkg, monkeypatch, h, w):
    x = torch.from_numpy(pkg.synth_crops(3, h, w, seed=55))
    ref = T.flip_tta_heatmaps(pkg.synth.to_torch_state_dict(sd_np(pkg, "HRNet", 32, 17)), x, F.COCO_PAIRS).numpy()
    net = engine(pkg, monkeypatch, "HRNet", 32, 17, (h, w), "fp32", 2)
    hm, preds, maxvals = host(*net.predict_flip_tta(x.cuda(), F.COCO_PAIRS))
    np.testing.assert_allclose(hm, ref, rtol=0, atol=HM_ATOL_F32)
    ref_preds, ref_max = F.max_preds(hm)
    np.testing.assert_array_equal(preds, ref_preds)
    np.testing.assert_array_equal(maxvals, ref_max)
    net.close()


# ------------------------------------------------------------------------------------------------- C. adversarial maps: exact ties
TIE_PAIRS = [(1, 2), (3, 4)]
TIE_CASES = [
    # (model, c, dtype, fused, H, W, n)
    ("HRNet", 32, "bf16", True, 32, 32, 2),          # 8x8 maps: 64 cells, three of the decode's four waves hold the sentinel only
    ("HRNet", 32, "bf16", True, 128, 96, 2),         # 32x24: three trips of the scan, ties across waves and trips
    ("HRNet", 32, "fp32", False, 64, 96, 2),
    ("HRNet", 48, "bf16", True, 384, 288, 1),        # 96x72: 27 trips
    ("PoseResNet", 50, "bf16", False, 128, 96, 2),
]


@pytest.mark.parametrize("model,c,dtype,fused,h,w,n", TIE_CASES)
def test_exact_ties_decode_to_the_first_maximum(pkg, monkeypatch, model, c, dtype, fused, h, w, n):
    """crops that equal their mirror image: every self-paired joint's averaged map is exactly mirror-symmetric, so its maximum is
    attained (at least) twice, in two cells of one row -- the decode has to return the left one, like np.argmax"""
    xs = F.symmetric_crops(pkg.synth_crops(n, h, w, seed=56))
    np.testing.assert_array_equal(xs, xs[..., ::-1])
    own = [j for j in range(17) if j not in (1, 2, 3, 4)]
    net = engine(pkg, monkeypatch, model, c, 17, (h, w), dtype, 2, None, fused)
    x = torch.from_numpy(xs).cuda()
    a = net(x).cpu().numpy()
    want = F.flip_tta_expected(a, a, TIE_PAIRS)             # the mirrored crops ARE the crops
    wq = w // 4
    for pp in (True, False):
        hm, preds, maxvals = host(*net.predict_flip_tta(x, TIE_PAIRS, post_processing=pp))
        np.testing.assert_array_equal(hm, want)
        np.testing.assert_array_equal(hm[:, own], hm[:, own][..., ::-1])
        for p0, p1 in TIE_PAIRS:
            np.testing.assert_array_equal(hm[:, p0], hm[:, p1][..., ::-1])
        flat = hm[:, own].reshape(n, len(own), -1)
        assert ((flat == flat.max(-1, keepdims=True)).sum(-1) >= 2).all()          # the ties are there
        seen = maxvals[:, own, 0] > 0
        assert seen.any() and (np.floor(preds[:, own, 0])[seen] < wq // 2).all()
        ref_preds, ref_max = F.max_preds(hm, pp)
        np.testing.assert_array_equal(preds, ref_preds)
        np.testing.assert_array_equal(maxvals, ref_max)
    assert net.pad_violations() == 0
    net.close()


# ------------------------------------------------------------------------------- C. adversarial maps: NaN, -inf and constant maps
@pytest.mark.parametrize("pairs", [[(3, 5), (7, 9)], []], ids=["mixed", "own-mirror"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_non_finite_and_flat_maps_decode_like_numpy(pkg, monkeypatch, dtype, pairs):
    """maps produced by the real head -- joint 3: NaN, joint 5: -inf, joint 7: +1 everywhere, joint 9: -1 everywhere -- averaged with
    another kind ("mixed": NaN + -inf = NaN, 1 + -1 = 0) or with their own mirror image: index 0, the value numpy finds, coordinates
    zero wherever ``maxval > 0`` is false, never coordinates formed from the scan's 'nothing seen' sentinel"""
    c, h, w, n = 32, 64, 64, 3
    sd = {k: np.array(v, copy=True) for k, v in sd_np(pkg, "HRNet", c, 17).items()}
    sd["final_layer.bias"][3] = np.nan
    sd["final_layer.bias"][5] = -np.inf
    for j, v in ((7, 1.0), (9, -1.0)):
        sd["final_layer.weight"][j] = 0.0
        sd["final_layer.bias"][j] = v
    net = engine(pkg, monkeypatch, "HRNet", c, 17, (h, w), dtype, 2, None, dtype == "bf16", sd=sd)
    x = torch.from_numpy(pkg.synth_crops(n, h, w, seed=57)).cuda()
    a, b = host(net(x), net(torch.flip(x, dims=[-1]).contiguous()))
    for t in (a, b):
        assert np.isnan(t[:, 3]).all() and np.isneginf(t[:, 5]).all() and (t[:, 7] == 1.0).all() and (t[:, 9] == -1.0).all()
        assert np.isfinite(np.delete(t, (3, 5), 1)).all()
    want = F.flip_tta_expected(a, b, pairs)
    if pairs:
        kinds = {3: np.nan, 5: np.nan, 7: 0.0, 9: 0.0}
    else:
        kinds = {3: np.nan, 5: -np.inf, 7: 1.0, 9: -1.0}
    special = sorted(kinds)
    raw = None
    for pp in (True, False):
        hm, preds, maxvals = host(*net.predict_flip_tta(x, pairs, post_processing=pp))
        np.testing.assert_array_equal(hm, want)                               # (NaN == NaN here)
        ref_preds, ref_max = F.max_preds(hm, pp)
        np.testing.assert_array_equal(preds, ref_preds)
        np.testing.assert_array_equal(maxvals, ref_max)
        for j, v in kinds.items():
            np.testing.assert_array_equal(hm[:, j], np.full_like(hm[:, j], v))
            np.testing.assert_array_equal(maxvals[:, j, 0], np.full(n, v, np.float32))
        np.testing.assert_array_equal(preds[:, special], np.zeros((n, len(special), 2), np.float32))      # index 0
        raw = preds
    hm, dark, maxvals = host(*net.predict_flip_tta(x, pairs, post_processing="dark"))
    np.testing.assert_array_equal(hm, want)
    np.testing.assert_array_equal(maxvals, F.max_preds(hm, False)[1])
    np.testing.assert_array_equal(dark[:, special], raw[:, special])          # DARK leaves these joints where they are
    assert np.isfinite(dark).all() and np.abs(dark - raw).max() <= 1.0
    assert net.pad_violations() == 0
    net.close()
