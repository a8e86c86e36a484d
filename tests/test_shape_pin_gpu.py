"""The per-operation pin at the crop widths where the plan changes kernels (tests/plan_census.py: PIN_SHAPES).

tests/test_bf16_pin.py, tests/test_fp16_gpu.py and tests/test_poseresnet.py tie every kernel form to the engine-arithmetic emulation,
but only at square or 4:3 crops no wider than 288 pixels.  The planner chooses a kernel by the row pitch of each feature map, so wide
crops (panoramic frames, ``resize_frames`` on 16:9 input) and one-pixel-wide or -high branches run regimes those shapes never reach:
the 384-pixel tiles of the staged kernels, the generic kernel on 3x3 convolutions too wide to stage, the two-launch stem, slab tiles of
two rows, slab tiles that do not divide the image.  tests/test_plan_census.py proves on plan-only handles that the shapes below reach
every form any legal resolution reaches; here each of them runs on the GPU, three crops in a handle of ``max_batch`` 4 (the flat row
index crosses image boundaries and the last tile is ragged), in the two variants of plan_census.VARIANTS, and EVERY operation is
compared with the emulation by ``test_bf16_pin.Pinner`` unchanged, with the project's own bounds (ULP, NOISE, MAX_DIFF_FRAC, the
on-chip-input rule, the fp16 ulp, 1e-4 of the range in fp32).  profiles/shape_pins.txt records what an MI355X run measured."""
import re
import time

import numpy as np
import pytest
import torch

import plan_census as C
import test_bf16_pin as P
from conftest import load_pkg, state_dict_np
from test_fp16_gpu import ULP16, _f16r

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    assert torch.cuda.is_available(), "GPU tests need a GPU: the HIP path has no CPU fallback"
    return p


def _T():
    from oracle import hrnet_torch_oracle as T
    return T


# What each shape is in the table FOR: forms (plan_census keys) that must be in the LIVE handle's census in the named variant -- the
# test fails if a planner change takes them away from the shape, instead of passing on some other form.
CHOSEN_FOR = {
    ("HRNet", 48, 32, 32, "bf16"): {"why": "branch 3 is one pixel wide and high (wp = 2); one-slab head",
                                    "both": [("head", 256, 1), ("stem_fused", 1)],
                                    "forced": [("tile", 2, 48, 3, 0, 512, "fused"), ("slab", 64, 3, "whole"), ("slab", 48, 3, "whole")]},
    ("HRNet", 48, 224, 32, "bf16"): {"why": "one-pixel-wide branch 3 under seven rows; slab tiles that divide the image",
                                     "forced": [("slab", 64, 3, "even")]},
    ("HRNet", 48, 32, 224, "bf16"): {"why": "one-pixel-high branch 3; two-row slab tiles of the stem's conv2",
                                     "both": [("head", 256, 2)], "forced": [("slab", 64, 2, "even")]},
    ("HRNet", 48, 32, 256, "bf16"): {"why": "branch 1 leaves compact enumeration; the stem's conv2 leaves the slab kernel",
                                     "both": [("conv", 3, 1, 3, 32, 6, 0), ("conv", 3, 2, 0, 0, 4, 0)],
                                     "default": [("tile", 3, 32, 6, 0, 128, "small")], "forced": [("tile", 3, 32, 6, 0, 512, "plain")]},
    ("HRNet", 48, 32, 320, "bf16"): {"why": "two-launch stem; branch 0 on two plain launches; 384-pixel tiles of the (48, 3) and (32, 3) forms",
                                     "both": [("stem_fused", 0), ("conv", 3, 1, 1, 48, 3, 0)],
                                     "default": [("tile", 1, 48, 3, 0, 128, "small")],
                                     "forced": [("tile", 1, 48, 3, 0, 384, "plain"), ("tile", 1, 32, 3, 0, 384, "plain")]},
    ("HRNet", 48, 32, 448, "bf16"): {"why": "branch 0's BasicBlock convolutions on the generic kernel (nr 3); ragged slab tiles",
                                     "both": [("conv", 3, 1, 0, 0, 3, 0)], "forced": [("slab", 48, 3, "ragged")]},
    ("HRNet", 48, 64, 576, "bf16"): {"why": "layer1.0's 3x3 and transition1 on the generic kernel (nr 4); two-row slab tiles at cin 48",
                                     "both": [("conv", 3, 1, 0, 0, 4, 0)], "forced": [("slab", 48, 2, "even")]},
    ("HRNet", 48, 32, 672, "bf16"): {"why": "the nr-3 slab convolutions on the generic kernel", "both": [("conv", 3, 2, 0, 0, 3, 0)]},
    ("HRNet", 48, 32, 832, "bf16"): {"why": "384-pixel tiles of the 96-cout form (branch 1) beside 512-pixel ones (branches 2, 3)",
                                     "forced": [("tile", 3, 32, 6, 0, 384, "plain"), ("tile", 3, 32, 6, 0, 512, "plain")]},
    ("HRNet", 48, 64, 32, "bf16"): {"why": "the stem's conv2 on slab tiles that do not divide the image", "forced": [("slab", 64, 3, "ragged")]},
    ("HRNet", 48, 160, 128, "bf16"): {"why": "48-channel slab problems of several even tiles per image", "forced": [("slab", 48, 3, "even")]},
    ("HRNet", 32, 32, 32, "bf16"): {"why": "W32 with a one-pixel branch 3; 512-pixel tiles of the (32, 2) form; one-slab head",
                                    "both": [("head", 256, 1), ("stem_fused", 1)],
                                    "forced": [("tile", 1, 32, 2, 0, 512, "plain"), ("slab", 64, 3, "whole")]},
    ("HRNet", 32, 64, 32, "bf16"): {"why": "ragged slab tiles of the stem's conv2", "forced": [("slab", 64, 3, "ragged")]},
    ("HRNet", 32, 32, 192, "bf16"): {"why": "two-row slab tiles of the stem's conv2", "forced": [("slab", 64, 2, "even")]},
    ("HRNet", 32, 224, 32, "bf16"): {"why": "even slab tiles of the stem's conv2; one-pixel-wide branch 3", "forced": [("slab", 64, 3, "even")]},
    ("HRNet", 32, 32, 320, "bf16"): {"why": "two-launch stem; 384-pixel tiles of the (32, 2) form",
                                     "both": [("stem_fused", 0)], "forced": [("tile", 1, 32, 2, 0, 384, "plain")]},
    ("HRNet", 32, 64, 448, "bf16"): {"why": "32-channel slab problems of several even tiles per image", "forced": [("slab", 32, 3, "even")]},
    ("HRNet", 32, 32, 576, "bf16"): {"why": "68 staged convolutions on the generic kernel (nr 4); ragged 32-channel slab tiles",
                                     "both": [("conv", 3, 1, 0, 0, 4, 0)], "forced": [("slab", 32, 3, "ragged")]},
    ("HRNet", 32, 32, 704, "bf16"): {"why": "two-row slab tiles at cin 32", "forced": [("slab", 32, 2, "even")]},
    ("HRNet", 32, 32, 992, "bf16"): {"why": "every stride-2 convolution of branch 0 on the generic kernel (nr 2)", "both": [("conv", 3, 2, 0, 0, 2, 0)]},
    ("PoseResNet", 50, 32, 32, "bf16"): {"why": "layer4 is one pixel; one-slab head", "both": [("head", 256, 1)]},
    ("PoseResNet", 50, 32, 576, "bf16"): {"why": "layer1's staged 3x3 convolutions on the generic kernel", "both": [("conv", 3, 1, 0, 0, 4, 0)]},
    ("HRNet", 48, 32, 448, "fp16"): {"why": "fp16 twins: generic nr 3, 384-pixel tiles, ragged slab tiles",
                                     "both": [("conv", 3, 1, 0, 0, 3, 0)], "forced": [("tile", 1, 32, 3, 0, 384, "plain"), ("slab", 48, 3, "ragged")]},
    ("HRNet", 48, 32, 672, "fp16"): {"why": "fp16 twins: nr-3 slab convolutions on the generic kernel", "both": [("conv", 3, 2, 0, 0, 3, 0)]},
    ("HRNet", 48, 32, 32, "fp32"): {"why": "fp32 with a one-pixel branch 3; 512-pixel tiles of conv3x3_f32_kernel",
                                    "both": [("head", 256, 1)], "forced": [("tile", 1, 16, 2, 0, 512, "plain")]},
    ("HRNet", 48, 32, 320, "fp32"): {"why": "384-pixel tiles of both forms of conv3x3_f32_kernel",
                                     "forced": [("tile", 1, 16, 2, 0, 384, "plain"), ("tile", 1, 16, 3, 0, 384, "plain")]},
    ("HRNet", 48, 32, 576, "fp32"): {"why": "69 convolutions leave conv3x3_f32_kernel for the generic kernel",
                                     "both": [("conv", 3, 1, 0, 0, 3, 0), ("conv", 3, 1, 0, 0, 4, 0)]},
    ("HRNet", 32, 32, 32, "fp32"): {"why": "W32 fp32 with a one-pixel branch 3", "both": [("head", 256, 1)]},
    ("HRNet", 32, 32, 320, "fp32"): {"why": "384-pixel tiles of conv3x3_f32_kernel", "forced": [("tile", 1, 16, 2, 0, 384, "plain")]},
    ("HRNet", 32, 32, 576, "fp32"): {"why": "staged fp32 convolutions on the generic kernel", "both": [("conv", 3, 1, 0, 0, 2, 0), ("conv", 3, 1, 0, 0, 4, 0)]},
    ("PoseResNet", 50, 32, 32, "fp32"): {"why": "layer4 is one pixel; one-slab head", "both": [("head", 256, 1)]},
    ("PoseResNet", 50, 32, 320, "fp32"): {"why": "384-pixel tiles of conv3x3_f32_kernel", "forced": [("tile", 1, 16, 2, 0, 384, "plain")]},
    ("PoseResNet", 50, 32, 576, "fp32"): {"why": "layer1's staged 3x3 convolutions on the generic kernel", "both": [("conv", 3, 1, 0, 0, 4, 0)]},
}

# the only tensors a plan may keep on-chip: the projection shortcut and the 3x3s the chain kernel computes in front of conv3
# (layer1), and conv1 of a fused BasicBlock (branch 0 of W48, forced variant)
ON_CHIP = re.compile(r"^(layer1\.0\.downsample\.0|layer1\.[1-3]\.conv2|stage\d\.\d\.branches\.0\.\d\.conv1)$")


def _id(shape):
    model, c, h, w, dtype, n = shape
    return "%s%d-%dx%d-%s-n%d" % ("W" if model == "HRNet" else "R", c, h, w, dtype, n)


def _weights(pkg, model, c):
    return state_dict_np(c) if model == "HRNet" else pkg.synth_state_dict(c, 17, 7, model="PoseResNet")


def _net(pkg, shape, variant, monkeypatch):
    model, c, h, w, dtype, n = shape
    P._clear(monkeypatch)
    for k in C.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in C.VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    net = pkg.NativeHRNet(c, 17, (h, w), dtype, max_batch=C.MAX_BATCH, device=0, model_name=model).load_state_dict(_weights(pkg, model, c))
    sw = net.switches()
    assert all("%s=%s" % kv in sw for kv in C.VARIANTS[variant].items()) and (variant != "default" or not any(k in sw for k in C.SWITCHES)), sw
    return net


def _assert_chosen_forms(net, shape, variant):
    """the forms this shape was chosen for are in the LIVE handle's plan, and the live plan is the one the census test looked at"""
    model, c, h, w, dtype, n = shape
    want = CHOSEN_FOR[shape[:5]]
    live = C.census_of(net, n)
    missing = [k for k in want.get("both", []) + want.get(variant, []) if k not in live]
    assert not missing, "%s (%s): chosen for %s, but the live plan lacks %s" % (_id(shape), variant, want["why"], missing)
    assert live == C.census(model, c, h, w, dtype, C.MAX_BATCH, n, C.VARIANTS[variant])
    return live


_EMU = {}


def _emulation(pkg, T, model, c, dtype):
    """one emulation per (model, width, rounding): it caches its folded and rounded weights"""
    key = (model, c, dtype)
    if key not in _EMU:
        sd = pkg.synth.to_torch_state_dict(_weights(pkg, model, c))
        exact = dtype == "fp32"
        _EMU[key] = (T.EngineEmulation(sd, not exact, not exact) if model == "HRNet" else T.PoseResNetEmulation(sd, c, not exact, not exact))
    return _EMU[key]


SHAPES_16 = [s for s in C.PIN_SHAPES if s[4] != "fp32"]
SHAPES_32 = [s for s in C.PIN_SHAPES if s[4] == "fp32"]


@pytest.mark.parametrize("variant", list(C.PIN_VARIANTS))
@pytest.mark.parametrize("shape", SHAPES_16, ids=_id)
def test_every_operation_at_a_covering_shape(pkg, monkeypatch, shape, variant):
    """bf16 / fp16: every operation against the emulation on the engine's own stored inputs (Pinner, unchanged bounds); then, end to
    end, joints == decode_heatmaps of the engine's own heat-maps and no pad position written"""
    t0 = time.time()
    model, c, h, w, dtype, n = shape
    T = _T()
    if dtype == "fp16":           # (the rounding patch of tests/test_fp16_gpu.py)
        monkeypatch.setattr(T, "_bf16r", _f16r)
        monkeypatch.setattr(P, "ULP", ULP16)
    emu = _emulation(pkg, T, model, c, dtype)
    net = _net(pkg, shape, variant, monkeypatch)
    live = _assert_chosen_forms(net, shape, variant)
    infos = net.conv_infos()
    x = torch.from_numpy(pkg.synth_crops(n, h, w, seed=41)).cuda()
    pin = P.Pinner(pkg, net, emu, x)
    # what stays on-chip in THIS call: no tap at all (chain kernel), or conv1 of a fused BasicBlock when the fused pass runs
    fused = {bytes(i.name).decode() for i in infos if i.algo == 2 and bytes(i.name).endswith(b".conv1")} if variant == "forced" else set()
    on_chip = {nm for nm in emu.order if nm != emu.HEAD and nm not in pin.tapped} | fused
    assert all(ON_CHIP.match(nm) for nm in on_chip), sorted(on_chip)
    if variant == "forced":
        assert bool(fused) == any(k[0] == "tile" and k[-1] == "fused" for k in live)
        assert all(k[0] != "slab_fallback" for k in live) and not any(k[0] == "tile" and k[-1] == "small" for k in live)
        for nm in sorted(fused)[:1] + sorted(fused)[-1:]:
            assert pin.native(nm) is None, "%s: the fused pass keeps it in LDS, the tap must refuse it" % nm
    else:
        assert not any(k[0] == "slab" or (k[0] == "tile" and k[-1] == "fused") for k in live)
    done = pin.check_all()
    assert done == len(emu.order) - len(on_chip), (done, len(emu.order), sorted(on_chip))
    # (an op with an input kept on-chip falls under Pinner's on-chip-input rule -- a few elements within one ulp of the largest term --
    # so its fraction of the per-element bound may pass 1; every other op's may not)
    loose = {nm for nm in emu.order if any(i in on_chip for i in emu.inputs_of(nm))}
    stored = [s for s in pin.stats if s[0] not in loose]
    worst = max(stored, key=lambda s: s[1])
    assert worst[1] <= 1.0, worst
    worst_loose = max([s for s in pin.stats if s[0] in loose], key=lambda s: s[1])
    differ = max([s for s in pin.stats if s[0] != emu.HEAD], key=lambda s: s[2])
    # end to end
    boxes = pkg.synth_boxes(n, seed=42)
    hm, pts = net.predict_crops(x, boxes, return_heatmaps=True)
    hm, pts = hm.cpu().numpy(), pts.cpu().numpy()
    assert np.array_equal(hm, pin.hm.cpu().numpy())
    np.testing.assert_array_equal(pts[..., :2], T.decode_heatmaps(hm, boxes)[..., :2])
    assert net.pad_violations() == 0
    net.close()
    print("\n[shape pin] %s %s: %d ops; worst %s at %.3f of its bound (on-chip input: %s at %.2f); most elements differing %.3f %% (%s); %.1f s"
          % (_id(shape), variant, done, worst[0], worst[1], worst_loose[0], worst_loose[1], 100 * differ[2], differ[0], time.time() - t0))


@pytest.mark.parametrize("variant", list(C.PIN_VARIANTS))
@pytest.mark.parametrize("shape", SHAPES_32, ids=_id)
def test_fp32_taps_at_a_covering_shape(pkg, monkeypatch, shape, variant):
    """fp32: the comparator of test_bf16_pin.test_fp32_engine_taps_meet_the_unrounded_emulation as it stands -- every tap within 1e-4
    of the tensor's range of the emulation with its roundings off (= the reference, tests/test_oracle.py)"""
    t0 = time.time()
    model, c, h, w, dtype, n = shape
    T = _T()
    emu = _emulation(pkg, T, model, c, dtype)
    net = _net(pkg, shape, variant, monkeypatch)
    live = _assert_chosen_forms(net, shape, variant)
    if variant == "forced":
        assert not any(k[0] == "tile" and k[-1] == "small" for k in live)
    crops = torch.from_numpy(pkg.synth_crops(n, h, w, seed=41))
    emu_hm, want_all = emu.forward(crops, taps="all")
    x = crops.cuda()
    taps = net.tap_infos()
    assert {t.name.decode() for t in taps} == set(emu.order) - {emu.HEAD}      # fp32 keeps nothing on-chip
    worst, worst_name, hm = 0.0, "", None
    for t in taps:
        name = t.name.decode()
        got, hm = net.forward_tap(x, name, return_heatmaps=True)
        want = want_all[name]
        rel = float((got.cpu() - want).abs().max() / want.abs().max())
        if rel > worst:
            worst, worst_name = rel, name
        assert rel < 1e-4, (name, rel)
    rel = float((hm.cpu() - emu_hm).abs().max() / emu_hm.abs().max())
    assert rel < 1e-4, ("heatmaps", rel)
    assert net.pad_violations() == 0
    net.close()
    print("\n[shape pin] %s %s: %d taps; worst %s at %.3g of its range (allowed 1e-4); heat-maps %.3g; %.1f s"
          % (_id(shape), variant, len(taps), worst_name, worst, rel, time.time() - t0))
