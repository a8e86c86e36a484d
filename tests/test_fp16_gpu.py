"""The fp16 engine on the MI355X: the bf16 plan and kernels with fp16 elements.

Pinned the way tests/test_bf16_pin.py pins bf16, operation by operation, against the same engine-arithmetic emulation with its
rounding switched to fp16 (``oracle.hrnet_torch_oracle._bf16r`` patched to ``.to(torch.float16)`` inside these tests):

    |native - emulation| <= one fp16 ulp of the value  +  2^-16 * (sum of |terms|),   at most 1 % of a tensor's elements differ.

Then the invariants the bf16 engine keeps (batch / micro-batch / position independence, every scheduling switch bit-identical,
pad rows zero), the accuracy against the fp32 oracle that motivates the mode, the peaked checkpoint, flip-TTA and SimpleHRNet."""
import numpy as np
import pytest
import torch

import test_bf16_pin as P
from conftest import golden, load_pkg, state_dict_np

pytestmark = pytest.mark.gpu

ULP16 = 2.0 ** -10       # adjacent fp16 values a < b (normal range): (b - a) / b <= 2^-10


def _f16r(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float16).to(torch.float32)


@pytest.fixture
def T(monkeypatch):
    """the oracle module with the engine emulation rounding to fp16 (and the pin's ulp set to fp16's)"""
    from oracle import hrnet_torch_oracle as T
    monkeypatch.setattr(T, "_bf16r", _f16r)
    monkeypatch.setattr(P, "ULP", ULP16)
    return T


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    assert torch.cuda.is_available(), "GPU tests need a GPU: the HIP path has no CPU fallback"
    return p


def _report(pin, tag):
    worst = max(pin.stats, key=lambda s: s[1])
    fr = [s[2] for s in pin.stats]
    print("\n[fp16 pin, per op] %s: %d ops; worst %s at %.2f of its bound; elements that differ at all: mean %.4f %%, worst %.3f %%"
          % (tag, len(pin.stats), worst[0], worst[1], 100 * float(np.mean(fr)), 100 * max(fr)))


@pytest.mark.parametrize("c,h,w,n", [(48, 128, 96, 3), (32, 128, 96, 2), (48, 64, 64, 1)])
def test_fp16_every_operation_of_a_small_call(pkg, T, monkeypatch, c, h, w, n):
    P._clear(monkeypatch)
    emu = T.EngineEmulation(pkg.synth.to_torch_state_dict(state_dict_np(c)))
    net = pkg.NativeHRNet(c, 17, (h, w), "fp16", max_batch=n, device=0).load_state_dict(state_dict_np(c))
    pin = P.Pinner(pkg, net, emu, torch.from_numpy(pkg.synth_crops(n, h, w, seed=5)).cuda())
    assert pin.check_all() >= 300
    _report(pin, "W%d %dx%d n=%d" % (c, h, w, n))
    assert net.pad_violations() == 0
    net.close()


@pytest.mark.parametrize("variant", ["default", "no_n96", "no_bbf", "no_s2", "generic_only"])
def test_fp16_batch256_w48_384x288_every_operation(pkg, T, monkeypatch, variant):
    """configs[2]'s code path (one micro-batch of 256 crops of W48 384x288) in its plan variants, crops 1, 128, 255"""
    P._clear(monkeypatch)
    for k, v in P.VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    c, h, w, n = 48, 384, 288, 256
    g = torch.Generator(device="cuda").manual_seed(1234)
    crops = torch.randn((n, 3, h, w), generator=g, device="cuda", dtype=torch.float32)
    emu = T.EngineEmulation(pkg.synth.to_torch_state_dict(state_dict_np(c)))
    net = pkg.NativeHRNet(c, 17, (h, w), "fp16", max_batch=n, device=0).load_state_dict(state_dict_np(c))
    algos = [i.algo for i in net.conv_infos()]
    if variant == "default":
        assert algos.count(2) > 0 and algos.count(3) >= 144 and algos.count(4) > 0   # fused pass, 96-cout form, slab kernel
    pin = P.Pinner(pkg, net, emu, crops, crop0=1, ncrops=3, crop_step=127)
    pin.check_all()
    _report(pin, "W48 384x288 micro-batch 256, %s" % variant)
    e2e = emu.forward(crops[pin.idx].cpu())
    hm = pin.hm[pin.idx].cpu()
    drift = float((hm - e2e).abs().max() / e2e.abs().max())
    agree = float((hm.flatten(2).argmax(-1) == e2e.flatten(2).argmax(-1)).float().mean())
    print("[fp16 pin, end to end] %s: max |dH| / max|H| = %.4f, arg-max agreement with the fp16 emulation %.3f" % (variant, drift, agree))
    assert drift < 0.05
    assert net.pad_violations() == 0
    net.close()


@pytest.mark.parametrize("h,w,n", [(256, 192, 3), (128, 96, 1)])
def test_fp16_poseresnet50_every_operation(pkg, T, monkeypatch, h, w, n):
    """PoseResNet-50 (7x7 MFMA stem, max-pool, chain kernels, transposed-conv phases, head) against PoseResNetEmulation in fp16"""
    P._clear(monkeypatch)
    sd_np = pkg.synth_state_dict(50, 17, 7, model="PoseResNet")
    emu = T.PoseResNetEmulation(pkg.synth.to_torch_state_dict(sd_np), 50)
    net = pkg.NativeHRNet(50, 17, (h, w), "fp16", max_batch=n, device=0, model_name="PoseResNet").load_state_dict(sd_np)
    x = torch.from_numpy(pkg.synth_crops(n, h, w, seed=29)).cuda()
    pin = P.Pinner(pkg, net, emu, x, crop0=0, ncrops=min(n, 2), crop_step=max(1, n - 1))
    pin.check_all()
    _report(pin, "PoseResNet-50 %dx%d n=%d" % (h, w, n))
    assert net.pad_violations() == 0
    net.close()


# ---- invariants ----------------------------------------------------------------------------------------------------------------
def test_fp16_results_do_not_depend_on_batch_micro_batch_or_position(pkg, monkeypatch):
    P._clear(monkeypatch)
    c, h, w = 48, 128, 96
    x = torch.from_numpy(pkg.synth_crops(13, h, w, seed=21)).cuda()
    outs = []
    for mb in (13, 5, 1):
        net = pkg.NativeHRNet(c, 17, (h, w), "fp16", max_batch=mb, device=0).load_state_dict(state_dict_np(c))
        outs.append(net(x).cpu())
        outs.append(net(x[7:9]).cpu())
        assert net.pad_violations() == 0
        net.close()
    for o in outs[2::2]:
        assert torch.equal(o, outs[0])
    for o in outs[1::2]:
        assert torch.equal(o, outs[0][7:9])


# Switches that select another kernel FORM with another arithmetic: the 96-cout form and the LDS-staged kernels sum K in another
# order than their fallbacks, the VALU stem / head keep fp32 weights where the MFMA ones round them (tests/test_n96.py,
# tests/test_gpu_parity.py bound these in bf16 rather than equate them).  Every other switch only reschedules: bit-identical.
ARITHMETIC_SWITCHES = ("HRN_DISABLE_N96", "HRN_DISABLE_LDS", "HRN_DISABLE_LDS32", "HRN_DISABLE_STEM_MFMA", "HRN_DISABLE_HEAD_MFMA")


@pytest.mark.parametrize("key", P.ENV_KEYS)
def test_fp16_every_scheduling_switch_on_against_off(pkg, monkeypatch, key):
    P._clear(monkeypatch)
    c, h, w, n = 48, 128, 96, 4
    x = torch.from_numpy(pkg.synth_crops(n, h, w, seed=8)).cuda()
    net = pkg.NativeHRNet(c, 17, (h, w), "fp16", max_batch=n, device=0).load_state_dict(state_dict_np(c))
    ref = net(x).cpu()
    net.close()
    monkeypatch.setenv(key, "0" if key == "HRN_BBF" else "1")
    net = pkg.NativeHRNet(c, 17, (h, w), "fp16", max_batch=n, device=0).load_state_dict(state_dict_np(c))
    got = net(x).cpu()
    assert net.pad_violations() == 0
    net.close()
    if key in ARITHMETIC_SWITCHES:
        d = float((got - ref).abs().max())
        print("[fp16 switch] %s: max|dH| %.4g at max|H| %.3g" % (key, d, float(ref.abs().max())))
        assert d <= 0.005 * float(ref.abs().max()) + 1e-3, key
    else:
        assert torch.equal(got, ref), key


# ---- accuracy: what the mode is for ----------------------------------------------------------------------------------------------
def test_fp16_is_closer_to_the_fp32_oracle_than_bf16(pkg):
    from oracle import hrnet_torch_oracle as T0
    c, h, w, n = 48, 256, 192, 16
    sdn = pkg.synth_state_dict(c, 17, 0)
    crops = torch.from_numpy(pkg.synth_crops(n, h, w))
    ref = T0.hrnet_forward(pkg.synth.to_torch_state_dict(sdn), crops)
    res = {}
    for dt in ("bf16", "fp16"):
        net = pkg.NativeHRNet(c, 17, (h, w), dt, max_batch=n, device=0).load_state_dict(sdn)
        hm = net(crops.cuda()).cpu()
        net.close()
        agree = float((hm.flatten(2).argmax(-1) == ref.flatten(2).argmax(-1)).float().mean())
        res[dt] = (agree, float((hm - ref).abs().max()))
    print("\n[fp16 accuracy, W48 256x192, 16 crops] arg-max agreement with fp32: fp16 %.3f, bf16 %.3f; max|dH|: fp16 %.4f, bf16 %.4f"
          % (res["fp16"][0], res["bf16"][0], res["fp16"][1], res["bf16"][1]))
    assert res["fp16"][0] >= 0.90 and res["fp16"][0] > res["bf16"][0]
    assert res["fp16"][1] <= 0.05


def test_fp16_peaked_checkpoint_all_on_cell(pkg):
    from oracle import hrnet_torch_oracle as T0
    S = pkg.synth
    c, h, w, n = 48, 384, 288, 8
    sdn = S.peaked_state_dict(c, 17, 0)
    crops, cen = S.peaked_crops(n, h, w, seed=5, on_cell=True)
    net = pkg.NativeHRNet(c, 17, (h, w), "fp16", max_batch=n, device=0).load_state_dict(sdn)
    hm = net(torch.from_numpy(crops).cuda()).cpu().numpy()
    net.close()
    w4 = w // 4
    am = hm.reshape(n, 17, -1).argmax(-1)
    py, px = am // w4, am % w4
    d = np.min(np.maximum(np.abs(py[:, :, None] - cen[:, None, :, 0] / 4.0), np.abs(px[:, :, None] - cen[:, None, :, 1] / 4.0)), -1)
    print("[fp16 peaked] %d of %d joints on their blob's cell" % (int((d == 0).sum()), d.size))
    assert d.size == 136 and (d == 0).all()
    ref = T0.hrnet_forward(S.to_torch_state_dict(sdn), torch.from_numpy(crops[:2])).numpy()
    assert (ref.reshape(2, 17, -1).argmax(-1) == am[:2]).all()


def test_fp16_flip_tta_meets_the_fp16_emulation(pkg, T):
    g = golden("w32_128x96_fliptta_n3")
    c, h, w = int(g["c"]), int(g["h"]), int(g["w"])
    sdn = state_dict_np(c, int(g["weight_seed"]))
    sd = pkg.synth.to_torch_state_dict(sdn)
    crops = torch.from_numpy(g["crops"])
    net = pkg.NativeHRNet(c, 17, (h, w), "fp16", max_batch=4, device=0).load_state_dict(sdn)
    hm, preds, _ = net.predict_flip_tta(crops.cuda(), g["flip_pairs"])
    hm = hm.cpu().numpy()
    def emu(x):
        out = T.hrnet_forward_engine(sd, x)
        return out[0] if isinstance(out, tuple) else out

    a = emu(crops)
    b = torch.flip(emu(torch.flip(crops, dims=[-1])), dims=[-1]).clone()
    for i, j in g["flip_pairs"].tolist():
        b[:, [i, j]] = b[:, [j, i]]
    want = ((a + b) * 0.5).numpy()
    err = float(np.abs(hm - want).max())
    print("[fp16 flip-TTA] max|dH| vs the fp16 emulation %.4g (heat-map std %.3g); vs the fp32 reference %.4g"
          % (err, want.std(), float(np.abs(hm - g["heatmaps"]).max())))
    assert err < 0.02 * want.std() + 0.01
    ref_preds, _ = T.max_preds_refined(hm, True)
    np.testing.assert_array_equal(preds.cpu().numpy(), ref_preds)
    assert net.pad_violations() == 0
    net.close()


def test_simple_hrnet_predict_in_fp16(pkg):
    """SimpleHRNet(dtype="fp16").predict on the reference predict() fixtures (tests/test_simple_hrnet.py): the structure and
    dtypes of the fp32 engine's results, joints printed against the reference's"""
    from test_simple_hrnet import _frames
    _, frame, frames5, _ = _frames()
    for c, img, name, mb in ((32, frame, "w32_128x96_predict_single", 32), (48, frames5, "w48_128x96_predict_batch5", 2)):
        g = golden(name)
        res = {}
        for dt in ("fp32", "fp16"):
            model = pkg.SimpleHRNet(c, 17, state_dict_np(c, 0), resolution=(128, 96), multiperson=False, return_heatmaps=True,
                                    return_bounding_boxes=True, max_batch_size=mb, device="cuda:0", dtype=dt)
            assert model.model.dtype == dt
            res[dt] = model.predict(img)
        for a, b in zip(res["fp16"], res["fp32"]):
            assert type(a) is type(b) and a.dtype == b.dtype and a.shape == b.shape
        hm, boxes, pts = res["fp16"]
        np.testing.assert_array_equal(boxes, g["boxes"])
        agree = float((pts[..., :2] == g["pts"][..., :2]).all(-1).mean())
        err = float(np.abs(hm - g["heatmaps"]).max())
        print("[fp16 SimpleHRNet.predict] %s: joints equal to the reference's %.3f; max|dH| %.4f" % (name, agree, err))
        assert err < 0.05 * g["heatmaps"].std() + 0.01
