"""The engine outside order-one numbers (DESIGN.md "numeric contract"; helpers and reasoning in tests/range_ref.py, the reference
side of every property in tests/test_range_host.py).

  1. exact scaling -- bias-free weights, crops * 2^k, k = -48, -16, +16, +48: heat-maps, joints and flip-TTA results scale bit for
     bit in bf16 and fp32, in every plan variant.  An absolute epsilon, a clamp or a detour through fp16 anywhere breaks it.
  2. the small end of fp16 -- the per-op pin of tests/test_fp16_gpu.py on crops * 2^-10 / 2^-12, where 39 % / 63 % of the stored
     activations are fp16 subnormals: a kernel that flushes them is 6e-5 off against a bound of order 1e-7.
  3. the large end of fp16 -- one operation per kernel family scaled so that its own store overflows: +-inf exactly where the
     emulation's unrounded value is beyond 65520, the ordinary bound everywhere else, no saturation, no NaN; and with the overflow
     confined to one crop, the crop next to it keeps its bits.
  4. poison -- one crop of a batch of five carries a NaN / inf pixel, is all NaN, or overflows inside the net: every OTHER crop's
     heat-maps, joints and confidences are bit-equal to the clean batch's, no pad or guard position of the workspace keeps
     anything, and a clean call afterwards is bit-equal to a fresh handle's.  What the poisoned crop itself returns is printed,
     not pinned (the one-instruction ReLU turns NaN into 0: DESIGN.md)."""
import numpy as np
import pytest
import torch

import range_ref as R
import test_bf16_pin as P
from conftest import load_pkg, state_dict_np
from test_bbf_carry import LONG_BLOCKS

pytestmark = pytest.mark.gpu

SWITCHES = tuple(P.ENV_KEYS) + ("HRN_S2_MIN_TILES", "HRN_BBF_TPB_DIV", "HRN_HALF_STAGES", "HRN_DISABLE_STEM_FUSE", "HRN_DISABLE_F32LDS",
                                "HRN_LONG_FACTOR", "HRN_LONG_SHARE", "HRN_DISABLE_COMPACT")
# plan variants: each selects other kernels.  16-bit plans and fp32 plans.
PLANS16 = {"default": {}, "fused_small": R.FUSED, "long_blocks": LONG_BLOCKS, "no_stem_fuse": {"HRN_DISABLE_STEM_FUSE": "1"},
           "generic_only": P.VARIANTS["generic_only"]}
PLANS32 = {"default": {}, "no_f32lds": {"HRN_DISABLE_F32LDS": "1"}}
FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    assert torch.cuda.is_available(), "GPU tests need a GPU: the HIP path has no CPU fallback"
    return p


@pytest.fixture
def T16(monkeypatch):
    """the oracle module with the engine emulation rounding to fp16, and the pin's ulp set to fp16's"""
    from oracle import hrnet_torch_oracle as T
    monkeypatch.setattr(T, "_bf16r", R.f16r)
    monkeypatch.setattr(P, "ULP", R.ULP16)
    return T


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


_WEIGHTS = {}


def _weights(pkg, model, c, free):
    key = (model, c, free)
    if key not in _WEIGHTS:
        sd = state_dict_np(c) if model == "HRNet" else pkg.synth_state_dict(c, 17, 7, model="PoseResNet")
        _WEIGHTS[key] = R.bias_free(sd) if free else sd
    return _WEIGHTS[key]


def _net(pkg, model, c, h, w, dtype, mb, sd):
    return pkg.NativeHRNet(c, 17, (h, w), dtype, max_batch=mb, device=0, model_name=model).load_state_dict(sd)


def _check_plan(net, model, c, dtype, plan):
    """the forms the variant is about are really in the plan (conv_infos().algo: 2 = fused pass, 3 = 96-cout form, 4 = slab kernel)"""
    algos = [i.algo for i in net.conv_infos()]
    sw = net.switches()
    if model != "HRNet":
        return
    if dtype == "fp32":
        assert (algos.count(1) == 0) == (plan == "no_f32lds") and not net.stem_fused()
        return
    assert net.stem_fused() == (plan != "no_stem_fuse")
    if plan == "generic_only":
        assert set(algos) == {0}
        return
    assert algos.count(4) > 0 and algos.count(1) > 0
    if c == 48:
        assert algos.count(2) == 64 and algos.count(3) == 144
    if plan in ("fused_small", "long_blocks"):
        assert "HRN_BBF_MIN_TILES=1" in sw
    if plan == "fused_small":
        assert "HRN_S2_MIN_TILES=1" in sw


def _fused_pass_runs(net, x):
    """at this call size conv1 of a 48-channel BasicBlock stays on-chip: the fused pass, not its two-launch fallback, ran"""
    with pytest.raises(RuntimeError, match="stays in LDS"):
        net.forward_tap(x, "stage2.0.branches.0.1.conv1")


def _all_paths(net, x, boxes):
    """every way a batch of crops goes through the engine -> {path: [tensors with the crop index first]} on the host"""
    out = {"net": [net(x)]}
    for refine in (None, "quarter", "dark"):
        hm, pts = net.predict_crops(x, boxes, return_heatmaps=True, refine=refine)
        out["predict_crops(%s)" % refine] = [hm, pts]
    out["flip_tta"] = list(net.predict_flip_tta(x, FLIP_PAIRS))
    return {k: [t.cpu() for t in v] for k, v in out.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. exact scaling ------------------------------------------------------------------------------------------------------------
SCALING = [("HRNet", c, h, w, n, dt, plan) for c in (48, 32) for (h, w, n) in ((64, 64, 3), (128, 96, 2))
           for dt, plans in (("bf16", PLANS16), ("fp32", PLANS32)) for plan in plans]
SCALING += [("PoseResNet", 50, 128, 96, 2, dt, "default") for dt in ("bf16", "fp32")]


@pytest.mark.parametrize("model,c,h,w,n,dtype,plan", SCALING, ids=lambda v: str(v))
def test_power_of_two_scaling_is_exact(pkg, monkeypatch, model, c, h, w, n, dtype, plan):
    _env(monkeypatch, (PLANS32 if dtype == "fp32" else PLANS16)[plan])
    net = _net(pkg, model, c, h, w, dtype, n, _weights(pkg, model, c, True))
    _check_plan(net, model, c, dtype, plan)
    x = torch.from_numpy(pkg.synth_crops(n, h, w, seed=91)).cuda()
    boxes = pkg.synth_boxes(n, seed=92)
    if model == "HRNet" and c == 48 and plan in ("fused_small", "long_blocks"):
        _fused_pass_runs(net, x)
    hm0 = net(x)
    hm1, pts0 = net.predict_crops(x, boxes, return_heatmaps=True)
    thm0, preds0, mv0 = net.predict_flip_tta(x, FLIP_PAIRS)
    assert torch.equal(hm0, hm1) and bool(torch.isfinite(hm0).all()) and float(hm0.abs().max()) > 0 and bool(torch.isfinite(thm0).all())
    assert float(mv0.max()) > 0 and float(preds0.max()) > 0          # (get_max_preds zeroes the coordinates of a joint whose maximum is <= 0)
    for k in R.SCALES:
        s = 2.0 ** k
        xs = x * s
        assert torch.equal(net(xs), hm0 * s), "heat-maps at 2^%d" % k
        hm, pts = net.predict_crops(xs, boxes, return_heatmaps=True)
        assert torch.equal(hm, hm0 * s), "predict_crops heat-maps at 2^%d" % k
        assert torch.equal(pts[..., :2], pts0[..., :2]), "joints at 2^%d" % k
        assert torch.equal(pts[..., 2], pts0[..., 2] * s), "confidences at 2^%d" % k
        thm, preds, mv = net.predict_flip_tta(xs, FLIP_PAIRS)
        assert torch.equal(thm, thm0 * s), "flip-TTA heat-maps at 2^%d" % k
        assert torch.equal(preds, preds0), "flip-TTA quarter-refined coordinates at 2^%d" % k
        assert torch.equal(mv, mv0 * s), "flip-TTA maxima at 2^%d" % k
    assert net.pad_violations() == 0
    net.close()


# ---- 2. fp16 at the small end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-10, -12])
@pytest.mark.parametrize("model,c,h,w,n", [("HRNet", 48, 128, 96, 2), ("HRNet", 32, 64, 64, 2), ("PoseResNet", 50, 128, 96, 1)])
def test_fp16_every_operation_on_small_crops(pkg, T16, monkeypatch, model, c, h, w, n, k):
    """tests/test_fp16_gpu.py: test_fp16_every_operation_of_a_small_call with bias-free weights on crops * 2^k: the same bound (the sum
    of |terms| scales with the input) + the subnormal spacing 2^-24 where the value is below 2^-14; at most 1 % may differ at all."""
    _env(monkeypatch, {})
    sd = _weights(pkg, model, c, True)
    tsd = pkg.synth.to_torch_state_dict(sd)
    emu = T16.EngineEmulation(tsd) if model == "HRNet" else T16.PoseResNetEmulation(tsd, 50)
    net = _net(pkg, model, c, h, w, "fp16", n, sd)
    x = torch.from_numpy(pkg.synth_crops(n, h, w, seed=5) * np.float32(2.0 ** k)).cuda()
    pin = P.Pinner(pkg, net, emu, x, subnormal_step=R.F16_SUBNORMAL_STEP)
    assert pin.check_all() >= (300 if model == "HRNet" else 50)
    stored = torch.cat([t.flatten() for nm, t in pin.cache.items() if t is not None and nm != emu.INPUT])
    assert bool(torch.isfinite(stored).all()) and bool(torch.isfinite(pin.hm).all())
    sub = float(((stored != 0) & (stored.abs() < R.F16_MIN_NORMAL)).float().mean())
    worst = max(pin.stats, key=lambda s: s[1])
    print("\n[fp16 small end] %s-%d %dx%d crops * 2^%d: %d ops, %.1f %% of the ENGINE's stored activations subnormal; worst %s at %.2f of its bound; "
          "differing elements: worst %.3f %%" % (model, c, h, w, k, len(pin.stats), 100 * sub, worst[0], worst[1], 100 * max(s[2] for s in pin.stats)))
    assert sub >= (0.25 if k == -10 else 0.45)                      # the engine keeps them (tests/test_range_host.py: the emulation's floor)
    assert net.pad_violations() == 0
    net.close()


# ---- 3. fp16 at the large end: overflow where the op stores -------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(R.OVERFLOW_CASES))
def test_fp16_store_overflows_to_inf(pkg, T16, monkeypatch, family):
    model, c, h, w, n, env, op, scales, algo, check = R.OVERFLOW_CASES[family]
    _env(monkeypatch, env)
    sd = R.overflow_weights(pkg.synth, family)
    tsd = pkg.synth.to_torch_state_dict(sd)
    emu = T16.EngineEmulation(tsd) if model == "HRNet" else T16.PoseResNetEmulation(tsd, 50)
    net = _net(pkg, model, c, h, w, "fp16", n, sd)
    x = torch.from_numpy(R.overflow_crops(pkg.synth, family)).cuda()
    infos = {i.name.decode(): i for i in net.conv_infos()}
    if algo is not None:
        assert infos[op].algo == algo and infos[check].algo == algo, (infos[op].algo, infos[check].algo)
    if family == "fused_stem":
        assert net.stem_fused()
    if family == "s2_slab":
        assert "HRN_S2_MIN_TILES=1" in net.switches() and infos[op].stride == 2 and infos[op].relu == 0
    if family == "generic_1x1":
        assert infos[op].ksize == 1 and infos[op].relu == 0
    pin = P.Pinner(pkg, net, emu, x)
    ins = pin.inputs(op)
    assert all(bool(torch.isfinite(v).all()) for v in ins.values()), "an input of %s is not finite on the engine" % op
    y, mag, pre = emu.eval_node(op, ins, magnitude=True, unrounded=True)
    if family != "fused_bb_conv1":
        if family == "fused_bb_conv2":
            assert pin.native("stage2.0.branches.0.0.conv1") is None            # conv1 stayed in LDS: the fused pass ran
        got = pin.native(op)
        assert got is not None
        st = R.compare_with_overflow(got, pre, mag, name=op, emulated_input=any(pin.native(i) is None for i in emu.inputs_of(op)))
        print("\n[fp16 overflow] %s (%s): %s" % (family, op, st))
        assert st["inf_due"] >= 16                                               # on the engine's own inputs too
        if family in ("generic_1x1", "s2_slab"):
            assert st["neg_inf_due"] >= 16
    else:
        # conv1 overflows in LDS; conv2 is what reaches HBM.  Where conv2's 3x3 window holds no overflowed (or possibly overflowed)
        # conv1 element it must meet the ordinary bound -- an inf must not reach beyond its footprint; the rest is counted only.
        assert pin.native(op) is None                                            # kept in LDS: the fused pass ran
        assert int(torch.isinf(y).sum()) >= 16
        nd = emu.graph[check]
        got = pin.native(check)
        clean = R.clean_window_mask(pre, mag, got.shape[1])
        assert bool(torch.isfinite(got[clean]).all()), "conv2 is not finite at %d outputs whose window holds no overflow" % int((~torch.isfinite(got) & clean).sum())
        assert not bool(torch.isfinite(got[~clean]).all())                       # (the overflow did happen on the engine)
        ins2 = {op: torch.where(torch.isfinite(y), y, torch.zeros_like(y)), nd["res"]: pin.native(nd["res"])}
        assert pin.check(check, got=got, ins=ins2, mask=clean)
        print("\n[fp16 overflow] %s: conv2 pinned at %d outputs (%.2f of its bound at worst), %d outputs under an overflowed window left unpinned"
              % (family, int(clean.sum()), pin.stats[-1][1], int((~clean).sum())))
        assert bool(clean[1].all())                                              # the neighbouring crop: all of it pinned
    # Isolation where the non-finite values arise DEEP in the net (a poisoned input pixel is gone after the first ReLUs: section 4
    # never shows one to this kernel family or to its consumers): crop 0 keeps its large values and overflows at this op, the
    # other crop is an ordinary order-one crop -- its heat-maps must be the bits it has next to an ordinary neighbour.
    quiet = torch.from_numpy(pkg.synth_crops(n, h, w, seed=R.OVERFLOW_SEED + 1)).cuda()
    mixed = quiet.clone()
    mixed[0] = x[0]
    assert not bool(torch.isfinite(net.forward_tap(mixed, check, crop0=0, ncrops=1)).all())     # the overflow is there, in crop 0 ...
    assert bool(torch.isfinite(net.forward_tap(mixed, check, crop0=1, ncrops=1)).all())         # ... and only there
    want = net(quiet)
    got = net(mixed)
    assert bool(torch.isfinite(want).all())
    assert torch.equal(_bits(got[1:]), _bits(want[1:])), "%s: an overflow in crop 0 changed its neighbour's heat-maps" % family
    assert net.pad_violations() == 0
    assert torch.equal(_bits(net(quiet)), _bits(want))                             # and nothing stays behind
    net.close()


# ---- 4. poison stays in its crop and in its call ------------------------------------------------------------------------------------
POISON = [("HRNet", c, h, w, dt, plan) for (c, h, w) in ((48, 128, 96), (32, 64, 64))
          for dt, plans in (("bf16", PLANS16), ("fp16", PLANS16), ("fp32", PLANS32)) for plan in plans]
POISON += [("PoseResNet", 50, 128, 96, dt, "default") for dt in ("bf16", "fp16", "fp32")]


@pytest.mark.parametrize("mb", [5, 3])
@pytest.mark.parametrize("model,c,h,w,dtype,plan", POISON, ids=lambda v: str(v))
def test_poison_stays_in_its_crop_and_in_its_call(pkg, monkeypatch, model, c, h, w, dtype, plan, mb):
    _env(monkeypatch, (PLANS32 if dtype == "fp32" else PLANS16)[plan])
    n = 5
    sd = _weights(pkg, model, c, False)
    net = _net(pkg, model, c, h, w, dtype, mb, sd)
    _check_plan(net, model, c, dtype, plan)
    crops = torch.from_numpy(pkg.synth_crops(n, h, w, seed=93))
    boxes = pkg.synth_boxes(n, seed=94)
    x = crops.cuda()
    fresh = _all_paths(net, x, boxes)                                 # the handle's first calls: what a fresh handle returns
    assert all(bool(torch.isfinite(t).all()) for v in fresh.values() for t in v) and net.pad_violations() == 0
    seen = {}
    for kind in R.POISONS:
        for slot in (0, 2, 4):
            xp = crops.clone()
            xp[slot] = R.poison(crops[slot], kind)
            got = _all_paths(net, xp.cuda(), boxes)
            others = [i for i in range(n) if i != slot]
            for path, tensors in got.items():
                for t, t0 in zip(tensors, fresh[path]):
                    assert torch.equal(_bits(t[others]), _bits(t0[others])), "%s: %s in crop %d changed another crop (max_batch %d)" % (path, kind, slot, mb)
            assert net.pad_violations() == 0, "%s in crop %d left something in a pad / guard position" % (kind, slot)
            hm = got["net"][0][slot]
            seen.setdefault(kind, []).append("%d/%d" % (int(torch.isnan(hm).sum()), int(torch.isinf(hm).sum())))
        again = _all_paths(net, x, boxes)                             # no persistence: the next clean call is a fresh handle's
        for path, tensors in again.items():
            for t, t0 in zip(tensors, fresh[path]):
                assert torch.equal(_bits(t), _bits(t0)), "%s: a clean call after %s differs from a fresh handle's" % (path, kind)
    print("\n[poison, observed, not pinned] %s-%d %s %s mb=%d: NaN / inf elements among the %d of the poisoned crop's heat-maps (slot 0, 2, 4): %s"
          % (model, c, dtype, plan, mb, fresh["net"][0][0].numel(), "; ".join("%s %s" % (k, " ".join(v)) for k, v in seen.items())))
    net.close()
