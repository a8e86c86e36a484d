"""The designed heat-maps of tests/wired.py on the CPU oracles: the wired checkpoint equals its closed form bit for bit, the designs
cover every place two cells can meet in the head kernels' walks and would catch a tie resolved by arrival order, and zero-set heads
produce tied maps on both models.  Everything tests/test_argmax_gpu.py feeds the MI355X is held here first, without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import wired as W
from conftest import load_pkg


def _T():
    from oracle import hrnet_torch_oracle as T
    return T


def _f16r(t):
    return t.to(torch.float16).to(torch.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_designed_maps(hm, ds, idx, mix, bias, planes):
    """hm equals the closed form bit for bit; per plane, the +1 joints peak on the designed cell with the designed number of ties and
    the -1 joints on the plane's first minimum"""
    want = W.closed_form(mix, bias, planes)
    assert same_bits(hm, want), "max |d| %.3g" % np.abs(hm - want).max()
    am, ties = hm.reshape(hm.shape[0], hm.shape[1], -1).argmax(-1), W.tie_counts(hm)
    for j in range(len(mix) - 2):                 # (the last two joints sum two planes: the closed form above holds them)
        s, sign = j % W.S, mix[j, j % W.S]
        for i in range(hm.shape[0]):
            d = ds[idx[i, s]]
            if sign > 0:
                assert am[i, j] == d.cell and ties[i, j] == d.ties, (d, i, j, am[i, j], ties[i, j])
            else:
                assert am[i, j] == int(np.argmin(d.plane)) and ties[i, j] == int((d.plane == d.plane.min()).sum()), (d, i, j)
    return want


@pytest.mark.parametrize("c", [32, 48])
@pytest.mark.parametrize("h,w", [(32, 32), (64, 96)])
def test_wired_checkpoint_equals_its_closed_form_on_the_oracles(c, h, w, monkeypatch):
    T = _T()
    J = 17
    ds = W.designs(h // 4, w // 4, 256, "mfma")
    assert {"twin", "edge", "flat", "shelf", "every-unit"} <= {d.name.split("(")[0] for d in ds}
    n = (len(ds) + W.S - 1) // W.S
    planes, idx = W.planes_for(ds, n, h // 4, w // 4)
    mix, bias = W.default_mix(J), W.default_bias(J)
    sd = W.set_head(W.wired_state_dict(c, J, 0), mix, bias)
    tsd = load_pkg("synth").to_torch_state_dict(sd)
    crops = torch.from_numpy(W.wired_crops(planes, h, w))
    check_designed_maps(T.hrnet_forward(tsd, crops).numpy(), ds, idx, mix, bias, planes)          # fp32: the reference's arithmetic
    hm, taps = T.hrnet_forward_engine(tsd, crops, taps={W.HEAD_TAP["HRNet"]})                      # bf16 storage and weights
    check_designed_maps(hm.numpy(), ds, idx, mix, bias, planes)
    other = taps[W.HEAD_TAP["HRNet"]].numpy()[:, W.S:]
    assert (other != 0).mean() > 0.5 and other.max() > 1                                           # the random trunk is alive
    monkeypatch.setattr(T, "_bf16r", _f16r)
    check_designed_maps(T.hrnet_forward_engine(tsd, crops).numpy(), ds, idx, mix, bias, planes)   # fp16


def test_identity_variance_is_what_makes_the_fold_exact():
    """1 / sqrt(float32(1 - 1e-5) + 1e-5) rounds to 1.0f; with var = 1 the scale is 0.999995f and four identities miss the design"""
    assert np.float32(1.0 / np.sqrt(np.float64(W.IDENTITY_VAR) + 1e-5)) == np.float32(1)
    assert np.float32(1.0 / np.sqrt(1.0 + 1e-5)) != np.float32(1)


WALKS = sorted({W.case_walk(c) + (c["h"] // 4, c["w"] // 4) for c in W.gpu_cases()})


def test_the_gpu_matrix_reaches_both_slab_sizes_in_both_forms():
    assert {(f, px) for f, px, _, _ in WALKS} == {("mfma", 256), ("mfma", 1024), ("valu", 256), ("valu", 1024)}
    by_class = {}
    for form, px, h, w in WALKS:
        for k in W.reachable(h * w, px, form):
            by_class.setdefault((form, px), set()).add(k)
    assert by_class[("mfma", 256)] == by_class[("mfma", 1024)] == by_class[("valu", 1024)] == set(W.CLASSES)
    assert by_class[("valu", 256)] == {"lane", "wave", "slab"}          # a 256-cell slab is one trip of the VALU form


def test_plan_only_handles_choose_the_slab_size_the_cases_expect():
    pkg = load_pkg()
    for case in W.gpu_cases():
        net = pkg.NativeHRNet(case["c"], case["J"], (case["h"], case["w"]), case["dtype"], max_batch=case["max_batch"], device=-1)
        hw = (case["h"] // 4) * (case["w"] // 4)
        for k in range(0, case["n"], case["max_batch"]):
            nb, px = min(case["max_batch"], case["n"] - k), ctypes.c_int32()
            slabs = net._lib.hrn_plan_head_slabs(net._h, nb, ctypes.byref(px))
            assert px.value == W.case_walk(case)[1] and slabs == (hw + px.value - 1) // px.value, (case, nb, px.value, slabs)
        net.close()


@pytest.mark.parametrize("form,slab_px,h,w", WALKS)
def test_designs_cover_every_class_and_have_teeth(form, slab_px, h, w):
    """with the order of argmax.h the model of the walk returns np.argmax on every design; with a tie resolved by arrival order at
    least one twin of every class that rule can change returns another cell (and no twin of a class it cannot change does)"""
    hw = h * w
    ds = W.designs(h, w, slab_px, form)
    twins = [d for d in ds if d.cls]
    reach = W.reachable(hw, slab_px, form)
    assert hw > slab_px or "slab" not in reach                     # a map of one slab has no slab class
    assert form == "mfma" or slab_px > 256 or "trip" not in reach  # a 256-cell slab has no trip in the VALU form
    assert {d.cls for d in twins} == reach
    for k in reach:                                                # one pair across the unit boundary: p the last cell, q the first
        near = [d for d in twins if d.cls == k and np.flatnonzero(d.plane == 7).tolist()[1] - d.cell == 1]
        assert near or k == "trip", k                              # (cells of one lane are never adjacent)
    for d in twins:
        p, q = np.flatnonzero(d.plane == 7).tolist()
        assert W.tie_class(p, q, hw, slab_px, form) == d.cls and d.ties == 2
    for d in ds:
        assert W.model_argmax(d.plane, slab_px, form) == d.cell == int(np.argmax(d.plane)), d
    for rule in ("incumbent", "challenger", "scan>="):
        hit = W.affected(rule, slab_px, form, reach)
        wrong = {k: [W.model_argmax(d.plane, slab_px, form, rule) != d.cell for d in twins if d.cls == k] for k in reach}
        for k in reach:
            assert any(wrong[k]) if k in hit else not any(wrong[k]), (rule, k, wrong[k])
    # every class is hit by some rule; the families of many ties fall to every rule that touches one of their classes
    assert set().union(*(W.affected(r, slab_px, form, reach) for r in ("incumbent", "challenger", "scan>="))) == reach
    flat = [d for d in ds if d.name == "flat"][0]
    assert W.model_argmax(flat.plane, slab_px, form, "challenger") != 0


def test_tie_class_reads_the_walks_of_kernels_hip():
    # MFMA, 256-cell slabs: waves of 64 cells, trips of 16
    assert W.tie_class(5, 9, 384, 256, "mfma") == "lane" and W.tie_class(5, 21, 384, 256, "mfma") == "trip"
    assert W.tie_class(9, 21, 384, 256, "mfma") == "lane" and W.tie_level(9, 21, 384, 256, "mfma") == "trip"
    assert W.tie_class(63, 64, 384, 256, "mfma") == "wave" and W.tie_class(255, 256, 384, 256, "mfma") == "slab"
    assert W.tie_class(255, 256, 384, 1024, "mfma") == "wave" and W.tie_class(5, 245, 384, 1024, "mfma") == "trip"
    # VALU: thread = r % 256
    assert W.tie_class(5, 9, 384, 256, "valu") == "lane" and W.tie_class(63, 64, 384, 256, "valu") == "wave"
    assert W.tie_class(5, 261, 384, 1024, "valu") == "trip" and W.tie_class(67, 261, 384, 1024, "valu") == "wave"
    assert W.tie_class(255, 256, 384, 1024, "valu") == "wave" and W.tie_class(255, 256, 384, 256, "valu") == "slab"
    assert W.plan_slab_px(384, 191) == 256 and W.plan_slab_px(384, 192) == 1024 and W.plan_slab_px(1280, 96) == 1024


ZERO_SET = [("PoseResNet", 50, 64, 128, 96, 2), ("HRNet", 32, 133, 64, 96, 2)]


def check_zero_set_census(hm, bias, masks, slab_px, form, tag):
    """>= 90 % of the (crop, joint) maps hold >= 2 equal maxima and every reachable level of distance holds >= 8 maps; -> the report"""
    n, J = hm.shape[:2]
    assert (hm <= bias[None, :, None, None]).all()
    assert ((hm.reshape(n, J, -1) == bias[None, :, None]) | ~masks).all()        # == b_j on the common zero set
    share, level = W.tie_census(hm, slab_px, form, W.tie_level)
    _, cls = W.tie_census(hm, slab_px, form)
    line = "%s %s slab %d: %.0f %% of %d maps tied; by level %s; by deciding merge %s" % (tag, form, slab_px, 100 * share, n * J, level, cls)
    print("\n[zero-set] " + line)
    assert share >= 0.9, line
    for k in W.reachable(hm.shape[2] * hm.shape[3], slab_px, form, W.tie_level):
        assert level[k] >= 8, line
    return line


@pytest.mark.parametrize("model,c,J,h,w,n", ZERO_SET)
def test_zero_set_heads_tie_on_the_emulations(model, c, J, h, w, n):
    """Classes here are ``tie_level`` (distance by coordinates): where the trunk puts its zeros is not designed, and two tied cells of
    one lane in different trips -- the only pairs ``takes`` decides -- are a handful of maps (printed); the twins hold that class."""
    T, synth = _T(), load_pkg("synth")
    sd = synth.synth_state_dict(c, J, 0, model=model)
    crops = torch.from_numpy(synth.synth_crops(n, h, w, seed=1))
    make = (lambda s: T.PoseResNetEmulation(synth.to_torch_state_dict(s), c)) if model == "PoseResNet" else \
        (lambda s: T.EngineEmulation(synth.to_torch_state_dict(s)))
    tap = W.HEAD_TAP[model]
    _, taps = make(sd).forward(crops, taps={tap})
    weight, masks = W.zero_set_heads(taps[tap].numpy(), J)
    bias = W.default_bias(J)
    hm = make(W.zero_set_state_dict(sd, weight, bias)).eval_node("heatmaps", {tap: taps[tap]}).numpy()
    assert (W.tie_counts(hm) >= 2).all() and (masks.sum(-1) >= 2).all()
    for form in ("mfma", "valu"):
        check_zero_set_census(hm, bias, masks, 256, form, "%s-%d J=%d %dx%d n=%d emulation" % (model, c, J, h, w, n))
