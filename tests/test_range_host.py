"""The reference side of the numeric-range tests (tests/test_range_gpu.py), on the CPU: what those tests hold the engine to is a
property of the emulation itself, their overflow cases are not vacuous, and their comparator rejects what it has to reject.

  * exact scaling: with bias-free weights the emulation (roundings on and off) and the plain fp32 restatement satisfy
    net(x * 2^k) == net(x) * 2^k bit for bit, HRNet W32 / W48 and PoseResNet-50 -- so a GPU failure is the engine's;
  * the small end of fp16: at crops * 2^-10 / 2^-12 at least 25 % / 45 % of the fp16 emulation's stored activations are subnormal (W48: 39 % / 63 %) and
    nothing is non-finite -- so flushing them cannot hide in the pin's noise term;
  * every (op, m) of range_ref.OVERFLOW_CASES overflows where the op stores and nowhere before;
  * a NaN pixel stays in its crop in the emulation;
  * compare_with_overflow on constructed arrays."""
import numpy as np
import pytest
import torch

import range_ref as R
from conftest import load_pkg, state_dict_np


def _T():
    from oracle import hrnet_torch_oracle as T
    return T


@pytest.fixture
def T16(monkeypatch):
    """the oracle module with the engine emulation rounding to fp16"""
    T = _T()
    monkeypatch.setattr(T, "_bf16r", R.f16r)
    return T


@pytest.fixture(scope="module")
def synth():
    return load_pkg("synth")


def _pose_sd(synth):
    return synth.synth_state_dict(50, 17, 7, model="PoseResNet")


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def test_bias_free_zeroes_every_folded_bias_and_nothing_else(synth):
    T = _T()
    sd0 = state_dict_np(32)
    sd = R.bias_free(sd0)
    assert sd0["bn1.bias"].any() and sd0["final_layer.bias"].any()          # a copy: the cached checkpoint is untouched
    for k, v in sd.items():
        if k.endswith(".bias") or k.endswith(".running_mean"):
            assert not v.any(), k
        else:
            np.testing.assert_array_equal(v, sd0[k])
    emu = T.EngineEmulation(synth.to_torch_state_dict(sd))
    for name, nd in emu.graph.items():
        if nd["op"] == "conv":
            assert not bool(emu._fold(name, nd["bn"])[1].any()), name


def test_scale_op_scales_one_batchnorm(synth):
    sd0 = state_dict_np(32)
    sd = R.scale_op(sd0, "stage2.0.branches.0.0.bn1", 5)
    for k, v in sd.items():
        if k == "stage2.0.branches.0.0.bn1.weight":
            np.testing.assert_array_equal(v, sd0[k] * np.float32(32))
        else:
            np.testing.assert_array_equal(v, sd0[k])


def test_eval_node_unrounded_is_the_value_before_the_store(synth):
    T = _T()
    emu = T.EngineEmulation(synth.to_torch_state_dict(state_dict_np(32)))
    x = torch.from_numpy(synth.synth_crops(1, 32, 32, seed=1))
    y = emu.eval_node("stem", {emu.INPUT: x})
    y2, mag = emu.eval_node("stem", {emu.INPUT: x}, magnitude=True)
    y3, pre = emu.eval_node("stem", {emu.INPUT: x}, unrounded=True)
    y4, mag4, pre4 = emu.eval_node("stem", {emu.INPUT: x}, magnitude=True, unrounded=True)
    assert torch.equal(y, y2) and torch.equal(y, y3) and torch.equal(y, y4) and torch.equal(mag, mag4) and torch.equal(pre, pre4)
    assert torch.equal(T._bf16r(pre), y) and not torch.equal(pre, y)
    c2, pre2 = emu.eval_node("conv2", {"stem": y}, unrounded=True)
    assert torch.equal(T._bf16r(pre2), c2) and bool((pre2 >= 0).all())      # after bias, residual and ReLU


# ---- 1. exact scaling belongs to the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [32, 48])
@pytest.mark.parametrize("rounded", [True, False])
def test_emulation_scales_exactly_hrnet(synth, c, rounded):
    T = _T()
    sd = synth.to_torch_state_dict(R.bias_free(state_dict_np(c)))
    emu = T.EngineEmulation(sd, round_weights=rounded, round_acts=rounded)
    x = torch.from_numpy(synth.synth_crops(1, 64, 64, seed=81))
    base, taps = emu.forward(x, taps="all")
    assert bool(torch.isfinite(base).all()) and float(base.abs().max()) > 0
    smallest = min(float(t[t > 0].min()) for t in taps.values() if bool((t > 0).any()))
    assert smallest * 2.0 ** -48 > 2.0 ** -100                      # 2^-48 stays far from fp32's subnormals (2^-126)
    for k in R.SCALES:
        s = 2.0 ** k
        assert torch.equal(emu.forward(x * s), base * s), k
    if not rounded:                                                 # the plain fp32 restatement (BatchNorm not folded) has the property too
        ref = T.hrnet_forward(sd, x)
        for k in (-48, 48):
            assert torch.equal(T.hrnet_forward(sd, x * 2.0 ** k), ref * 2.0 ** k), k


@pytest.mark.parametrize("rounded", [True, False])
def test_emulation_scales_exactly_poseresnet(synth, rounded):
    T = _T()
    sd = synth.to_torch_state_dict(R.bias_free(_pose_sd(synth)))
    emu = T.PoseResNetEmulation(sd, 50, round_weights=rounded, round_acts=rounded)
    x = torch.from_numpy(synth.synth_crops(1, 64, 64, seed=82))
    base = emu.forward(x)
    assert bool(torch.isfinite(base).all()) and float(base.abs().max()) > 0
    for k in (-48, 48):
        assert torch.equal(emu.forward(x * 2.0 ** k), base * 2.0 ** k), k


# ---- 2. the small end of fp16 is really exercised ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k,least", [(-10, 0.25), (-12, 0.45)])
@pytest.mark.parametrize("model,c,h,w", [("HRNet", 48, 64, 64), ("HRNet", 32, 64, 64), ("PoseResNet", 50, 128, 96)])
def test_small_crops_fill_the_fp16_subnormal_range(synth, T16, model, c, h, w, k, least):
    sd = synth.to_torch_state_dict(R.bias_free(state_dict_np(c) if model == "HRNet" else _pose_sd(synth)))
    emu = T16.EngineEmulation(sd) if model == "HRNet" else T16.PoseResNetEmulation(sd, 50)
    x = torch.from_numpy(synth.synth_crops(1, h, w, seed=5)) * 2.0 ** k
    hm, taps = emu.forward(x, taps="all")
    allv = torch.cat([t.flatten() for t in taps.values()])
    assert bool(torch.isfinite(allv).all()) and bool(torch.isfinite(hm).all())
    sub = float(((allv != 0) & (allv.abs() < R.F16_MIN_NORMAL)).float().mean())
    print("\n[fp16 small end] %s-%d crops * 2^%d: %.1f %% of the stored activations are subnormal, %.1f %% zero"
          % (model, c, k, 100 * sub, 100 * float((allv == 0).float().mean())))
    assert sub >= least


# ---- 3. every overflow case overflows where its op stores, and only there --------------------------------------------------------
def _emulation(T, synth, family):
    model = R.OVERFLOW_CASES[family][0]
    sd = synth.to_torch_state_dict(R.overflow_weights(synth, family))
    return T.EngineEmulation(sd) if model == "HRNet" else T.PoseResNetEmulation(sd, 50)


@pytest.mark.parametrize("family", list(R.OVERFLOW_CASES))
def test_overflow_case_preconditions(synth, T16, family):
    """The op's unrounded maximum lies between 2x and 8x 65504, at least 16 elements are clearly beyond 65520, at most 1 % of the
    tensor is ambiguous, every input of the op is finite.  The fuse sum cannot reach 2x: its T terms are stored fp16 tensors, each
    below 65504 where finite, whose maxima fall on different elements -- there the maximum only has to be 25 % beyond 65504 (the
    ambiguous band is 0.1 % wide), and below T x."""
    model, c, h, w, n, env, op, scales, algo, check = R.OVERFLOW_CASES[family]
    emu = _emulation(T16, synth, family)
    assert float(max(emu._fold(nm, nd["bn"])[0].abs().max() for nm, nd in emu.graph.items() if nd["op"] == "conv")) < R.F16_MAX   # fp16 weights too
    ins, (y, mag, pre) = R.forward_until(emu, torch.from_numpy(R.overflow_crops(synth, family)), op)
    f = R.overflow_preconditions(ins, pre, mag)
    print("\n[fp16 overflow case] %s: %s" % (family, f))
    lo, hi = (1.25, float(len(emu.graph[op]["terms"]))) if emu.graph[op]["op"] == "fuse" else (2.0, 8.0)
    assert f["inputs_finite"]
    assert lo <= f["max_over_f16max"] <= hi
    assert f["clear"] >= 16
    assert f["ambiguous_frac"] <= R.MAX_DIFF_FRAC
    assert int(torch.isinf(y).sum()) >= f["clear"]
    if family in ("generic_1x1", "s2_slab"):                        # no ReLU: both signs overflow
        assert f["clear_neg"] >= 16 and bool((y == float("-inf")).any())
    if family == "fused_bb_conv1":
        cout = emu._fold(check, emu.graph[check]["bn"])[0].shape[0]
        clean = R.clean_window_mask(pre, mag, cout)
        frac = float(clean.float().mean())
        print("[fp16 overflow case] %s: %.1f %% of conv2's outputs have a window free of overflow" % (family, 100 * frac))
        assert 0.25 <= frac < 1.0
        assert bool(clean[1].all()) and not bool(clean[0, :, -1].all())   # the overflow touches the pad row the two crops share


# ---- 4. the reference keeps crops independent -----------------------------------------------------------------------------------
def test_emulation_keeps_a_nan_pixel_in_its_crop(synth):
    T = _T()
    emu = T.EngineEmulation(synth.to_torch_state_dict(state_dict_np(32)))
    x = torch.from_numpy(synth.synth_crops(3, 64, 64, seed=83))
    base = emu.forward(x)
    xp = x.clone()
    xp[1] = R.poison(x[1], "nan_pixel")
    got = emu.forward(xp)
    assert torch.equal(got[0], base[0]) and torch.equal(got[2], base[2])
    assert bool(torch.isnan(got[1]).all())


def test_poison_kinds():
    x = torch.randn(3, 8, 8)
    for kind in R.POISONS:
        p = R.poison(x, kind)
        assert p.shape == x.shape and (kind == "huge_crop" or not bool(torch.isfinite(p).all()))
    assert int(torch.isnan(R.poison(x, "nan_pixel")).sum()) == 1 and int(torch.isinf(R.poison(x, "ninf_pixel")).sum()) == 1
    assert bool(torch.isfinite(R.poison(x, "huge_crop")).all()) and float(R.poison(x, "huge_crop").abs().min()) == pytest.approx(3e38)
    assert bool(torch.isfinite(x).all())


# ---- 5. the comparator rejects what it has to -----------------------------------------------------------------------------------
def _arrays():
    """64 x 64 values: ordinary ones, 32 clear overflows of either sign, a few subnormals; got = exactly what fp16 stores"""
    g = torch.Generator().manual_seed(3)
    wu = torch.randn(64, 64, generator=g) * 100.0
    wu[0, :16] = 1.0e5
    wu[0, 16:32] = -2.0e5
    wu[1, :8] = 3.0e-6            # subnormal in fp16
    wu[1, 8:16] = -4.5e-7
    mag = wu.abs() * 4 + 1e-5
    return R.f16r(wu), wu, mag


def _next_f16(t):
    """the fp16 neighbour of larger magnitude"""
    return (t.half().contiguous().view(torch.int16) + 1).view(torch.float16).float()


def test_comparator_accepts_the_exact_store_and_a_one_ulp_neighbour():
    got, wu, mag = _arrays()
    st = R.compare_with_overflow(got, wu, mag)
    assert st["inf_due"] == 32 and st["neg_inf_due"] == 16 and st["ambiguous"] == 0 and st["differ_frac"] == 0
    near = got.clone()
    near[5, 5] = _next_f16(got[5, 5])
    assert near[5, 5] != got[5, 5]
    assert R.compare_with_overflow(near, wu, mag)["differ_frac"] > 0


def _rejects(got, wu, mag, what, **kw):
    with pytest.raises(AssertionError, match=what):
        R.compare_with_overflow(got, wu, mag, **kw)


def test_comparator_rejects_a_wrong_inf_sign():
    got, wu, mag = _arrays()
    got[0, 20] = float("inf")
    _rejects(got, wu, mag, "break the fp16 store rule")


def test_comparator_rejects_a_finite_value_where_inf_is_due():
    got, wu, mag = _arrays()
    got[0, 3] = R.F16_MAX                                           # a saturating conversion
    _rejects(got, wu, mag, "1 finite where inf is due")


def test_comparator_rejects_an_inf_or_nan_where_a_finite_value_is_due():
    for v in (float("inf"), float("nan")):
        got, wu, mag = _arrays()
        got[7, 7] = v
        _rejects(got, wu, mag, "1 wrong or non-finite")


def test_comparator_rejects_a_flushed_subnormal():
    got, wu, mag = _arrays()
    assert 0 < float(got[1, 9].abs()) < R.F16_MIN_NORMAL
    got[1, 9] = 0.0                                                # 4.5e-7 flushed: 7.5 subnormal steps
    _rejects(got, wu, mag, "1 wrong or non-finite")
    got, wu, mag = _arrays()
    got[1, 9] += R.F16_SUBNORMAL_STEP                              # one subnormal step off is within the bound
    R.compare_with_overflow(got, wu, mag)


def test_comparator_rejects_an_ambiguous_share_above_the_cap():
    got, wu, mag = _arrays()
    wu[10:12] = R.F16_OVERFLOW - 1.0                               # 128 of 4096 = 3 % sit on the threshold
    mag = wu.abs() * 4 + 1e-5
    got = R.f16r(wu)
    _rejects(got, wu, mag, "decides nothing")
    st = R.compare_with_overflow(got, wu, mag, max_ambiguous_frac=0.05)
    assert st["ambiguous"] == 128
    got[10, 0] = float("nan")                                      # but never a NaN there
    _rejects(got, wu, mag, "break the fp16 store rule", max_ambiguous_frac=0.05)


def test_comparator_rejects_too_many_differing_elements():
    got, wu, mag = _arrays()
    got[20:22] = _next_f16(got[20:22])                             # 3 % one ulp off: each within its bound
    _rejects(got, wu, mag, "differ from the emulation")
