"""The loops only a large call runs -- blocks that walk several tiles -- in calls of a few crops (tests/plan_census.py: walk keys).

Every kernel family has a second code path that only a large call takes: a staged or fused block that holds two or more tiles makes the
tile-to-tile transition (the next slab prefetched under the current tile, the buffer swap, the fused pass's carried halo rows), may end on
a ragged tile that comes after others, and is dealt from the tensor's end in every odd launch; a slab or stem block walks a run of tiles;
a chain-kernel wave loops over fragments; the generic kernel takes more M fragments per wave.  tests/test_plan_census.py proves on
plan-only handles that ``plan_census.WALK_CASES`` (with the shape pins of tests/test_shape_pin_gpu.py) reach every such walk any legal
resolution reaches in a production call of 64 or 256 crops.  Here

* every walk case runs on the GPU and EVERY operation is compared with the engine-arithmetic emulation by ``test_bf16_pin.Pinner``
  unchanged, with the project's own bounds (ULP, NOISE, MAX_DIFF_FRAC, the on-chip-input rule, the fp16 ulp, 1e-4 of the range in fp32);
  the walk keys a case is in the table for (``WALK_FOR``) are asserted on the live handle first;
* at every legal width (H = 32) a call on long blocks (plan_census.VARIANTS["long"], and "long_unfused" / "long_small" where production
  walks forms that variant replaces) gives, bit for bit, what the same call gives on one-unit blocks (plan_census.one_unit: one tile per
  staged block as in the shape pins, but with both block caps raised, not at their defaults): walking several tiles only reschedules work.

profiles/walk_pins.txt records what an MI355X run measured.  One finding is recorded there that is no property of a walk: a 128-crop
call of W48 at 96 x 1120 misses Pinner's on-chip-input rule at layer1.0.conv3 (7 of 5.16 M elements, worst 0.00586 against 0.00523) with
the default switches as well; that call is not among the cases."""
import time

import numpy as np
import pytest
import torch

import plan_census as C
import test_bf16_pin as P
from conftest import load_pkg
from test_fp16_gpu import ULP16, _f16r
from test_shape_pin_gpu import ON_CHIP, _T, _emulation, _weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    assert torch.cuda.is_available(), "GPU tests need a GPU: the HIP path has no CPU fallback"
    return p


def _net(pkg, model, c, h, w, dtype, max_batch, env, monkeypatch):
    P._clear(monkeypatch)
    for k in C.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net = pkg.NativeHRNet(c, 17, (h, w), dtype, max_batch=max_batch, device=0, model_name=model).load_state_dict(_weights(pkg, model, c))
    sw = net.switches()
    assert all("%s=%s" % kv in sw for kv in env.items()) and (env or not any(k in sw for k in C.SWITCHES)), sw
    return net


def _assert_walks(net, case):
    """the walks this case is in the table for are in the LIVE handle's plan (a planner change fails here instead of moving the case onto
    one-tile blocks), and the live plan is the one the cover test looked at"""
    model, c, h, w, dtype, n = case[:6]
    live = C.walk_of(net, n)
    missing = [k for k in C.WALK_FOR[case] if k not in live]
    assert not missing, "%s: in the table for %s, but the live plan lacks them" % (C.case_id(case), missing)
    assert live == C.walk(model, c, h, w, dtype, n, n, C.case_env(case))
    return live


def _crops_of(n, h, w):
    """Pinner's crop selection: every crop of a call of up to 16 crops and a quarter of a megapixel, else three crops that END on the
    call's last one -- the tensor's last tile, which the n = 128 / 256 cases are in the table for, lies there: crops 1, 64, 127 of 128 as
    test_bf16_pin takes 1, 128, 255 of 256 (the emulation of the selected crops runs on the CPU)"""
    if n <= 16 and n * h * w <= 1 << 18:
        return dict(crop0=0, ncrops=None, crop_step=1)
    step = (n - 1) // 2
    sel = dict(crop0=n - 1 - 2 * step, ncrops=3, crop_step=step)
    assert sel["crop0"] + 2 * step == n - 1 and sel["crop0"] in (0, 1)
    return sel


CASES_16 = [k for k in C.WALK_CASES if k[4] != "fp32"]
CASES_32 = [k for k in C.WALK_CASES if k[4] == "fp32"]


@pytest.mark.parametrize("case", CASES_16, ids=C.case_id)
def test_every_operation_on_long_blocks(pkg, monkeypatch, case):
    """bf16 / fp16: every operation against the emulation on the engine's own stored inputs (Pinner, unchanged bounds); then, end to
    end, joints == decode_heatmaps of the engine's own heat-maps and no pad position written"""
    t0 = time.time()
    model, c, h, w, dtype, n, variant, _ = case
    T = _T()
    if dtype == "fp16":           # (the rounding patch of tests/test_fp16_gpu.py)
        monkeypatch.setattr(T, "_bf16r", _f16r)
        monkeypatch.setattr(P, "ULP", ULP16)
    emu = _emulation(pkg, T, model, c, dtype)
    net = _net(pkg, model, c, h, w, dtype, n, C.case_env(case), monkeypatch)
    _assert_walks(net, case)
    form = C.census_of(net, n)
    x = torch.from_numpy(pkg.synth_crops(n, h, w, seed=43)).cuda()
    pin = P.Pinner(pkg, net, emu, x, **_crops_of(n, h, w))
    # what stays on-chip in THIS call: no tap at all (chain kernel), or conv1 of a fused BasicBlock when the fused pass runs
    runs_fused = any(k[0] == "tile" and k[-1] == "fused" for k in form)
    assert variant != "default" or not runs_fused
    fused = {bytes(i.name).decode() for i in net.conv_infos() if i.algo == 2 and bytes(i.name).endswith(b".conv1")} if runs_fused else set()
    on_chip = {nm for nm in emu.order if nm != emu.HEAD and nm not in pin.tapped} | fused
    assert all(ON_CHIP.match(nm) for nm in on_chip), sorted(on_chip)
    for nm in sorted(fused)[:1] + sorted(fused)[-1:]:
        assert pin.native(nm) is None, "%s: the fused pass keeps it in LDS, the tap must refuse it" % nm
    done = pin.check_all()
    assert done == len(emu.order) - len(on_chip), (done, len(emu.order), sorted(on_chip))
    # (an op with an input kept on-chip falls under Pinner's on-chip-input rule, so its fraction of the per-element bound may pass 1;
    # every other op's may not)
    loose = {nm for nm in emu.order if any(i in on_chip for i in emu.inputs_of(nm))}
    worst = max([s for s in pin.stats if s[0] not in loose], key=lambda s: s[1])
    assert worst[1] <= 1.0, worst
    differ = max([s for s in pin.stats if s[0] != emu.HEAD], key=lambda s: s[2])
    boxes = pkg.synth_boxes(n, seed=44)
    hm, pts = net.predict_crops(x, boxes, return_heatmaps=True)
    hm, pts = hm.cpu().numpy(), pts.cpu().numpy()
    assert np.array_equal(hm, pin.hm.cpu().numpy())
    np.testing.assert_array_equal(pts[..., :2], T.decode_heatmaps(hm, boxes)[..., :2])
    assert net.pad_violations() == 0
    net.close()
    print("\n[walk pin] %s: %d ops on %d crops; worst %s at %.3f of its bound; most elements differing %.3f %% (%s); %.1f s"
          % (C.case_id(case), done, len(pin.idx), worst[0], worst[1], 100 * differ[2], differ[0], time.time() - t0))


@pytest.mark.parametrize("case", CASES_32, ids=C.case_id)
def test_fp32_taps_on_long_blocks(pkg, monkeypatch, case):
    """fp32: the comparator of test_bf16_pin.test_fp32_engine_taps_meet_the_unrounded_emulation as it stands -- every tap within 1e-4
    of the tensor's range of the emulation with its roundings off"""
    t0 = time.time()
    model, c, h, w, dtype, n, variant, _ = case
    emu = _emulation(pkg, _T(), model, c, dtype)
    net = _net(pkg, model, c, h, w, dtype, n, C.case_env(case), monkeypatch)
    _assert_walks(net, case)
    sel = _crops_of(n, h, w)
    idx = list(range(n)) if sel["ncrops"] is None else [sel["crop0"] + k * sel["crop_step"] for k in range(3)]
    crops = torch.from_numpy(pkg.synth_crops(n, h, w, seed=43))
    emu_hm, want_all = emu.forward(crops[idx], taps="all")
    x = crops.cuda()
    taps = net.tap_infos()
    assert {t.name.decode() for t in taps} == set(emu.order) - {emu.HEAD}      # fp32 keeps nothing on-chip
    worst, worst_name, hm = 0.0, "", None
    for t in taps:
        name = t.name.decode()
        got, hm = net.forward_tap(x, name, return_heatmaps=True, **sel)
        want = want_all[name]
        rel = float((got.cpu() - want).abs().max() / want.abs().max())
        if rel > worst:
            worst, worst_name = rel, name
        assert rel < 1e-4, (name, rel)
    rel = float((hm[idx].cpu() - emu_hm).abs().max() / emu_hm.abs().max())
    assert rel < 1e-4, ("heatmaps", rel)
    assert net.pad_violations() == 0
    net.close()
    print("\n[walk pin] %s: %d taps on %d crops; worst %s at %.3g of its range (allowed 1e-4); heat-maps %.3g; %.1f s"
          % (C.case_id(case), len(taps), len(idx), worst_name, worst, rel, time.time() - t0))


def _last_of_every_branch(net):
    """the last stored tensor of every branch of every stage module: conv2 of the branch's last BasicBlock"""
    names = sorted(t.name.decode() for t in net.tap_infos())
    blocks = {}
    for nm in names:
        p = nm.split(".")
        if len(p) == 6 and p[2] == "branches" and p[5] == "conv2":
            key = tuple(p[:4])
            blocks[key] = max(blocks.get(key, 0), int(p[4]))
    return ["%s.%d.conv2" % (".".join(k), b) for k, b in sorted(blocks.items())]


@pytest.mark.parametrize("c,dtype,w", C.SWEEP_WIDTHS, ids=lambda v: str(v))
def test_long_blocks_give_the_bits_of_one_unit_blocks(pkg, monkeypatch, c, dtype, w):
    """heat-maps, joints and the last tensor of every branch of every stage module, bit for bit, long blocks against one-unit blocks;
    both plans are asserted first (plan_census.sweep_call: the classes claimed; the baseline has no block of more than one unit).  The
    long variant runs at every width; where production walks several tiles per block with a form that variant replaces -- the plain
    (48, 3) form below the fused pass's threshold, 128-pixel tiles -- "long_unfused" / "long_small" run as well.  The one family left
    below three tiles per block is written down (plan_census.SWEEP_DROPPED) and asserted."""
    t0 = time.time()
    h = C.SWEEP_H
    runs, dropped = C.sweep_call("HRNet", c, w, dtype)
    assert dropped == C.sweep_dropped(c, dtype, w), dropped
    assert runs[0][0] == "long"
    for variant, n, families in runs:
        x = torch.from_numpy(pkg.synth_crops(n, h, w, seed=45)).cuda()
        boxes = pkg.synth_boxes(n, seed=46)
        outs, classes = [], None
        for env in (C.VARIANTS[variant], C.one_unit(variant)):
            net = _net(pkg, "HRNet", c, h, w, dtype, n, env, monkeypatch)
            walks = C.walk_of(net, n)
            if not outs:
                C.assert_long_plan(walks, families)
                classes = C.staged_blocks_per_class(net, n)
            else:
                C.assert_one_unit_plan(walks)
            hm, pts = net.predict_crops(x, boxes, return_heatmaps=True)
            taps = [net.forward_tap(x, nm).cpu().numpy() for nm in _last_of_every_branch(net)]
            assert len(taps) == 2 + 4 * 3 + 3 * 4
            assert net.pad_violations() == 0
            outs.append((hm.cpu().numpy(), pts.cpu().numpy(), taps))
            net.close()
        assert np.isfinite(outs[0][0]).all() and np.abs(outs[0][0]).max() > 0
        np.testing.assert_array_equal(outs[0][0], outs[1][0])
        np.testing.assert_array_equal(outs[0][1], outs[1][1])
        for a, b in zip(outs[0][2], outs[1][2]):
            np.testing.assert_array_equal(a, b)
        print("\n[walk sweep] W%d %s %dx%d %s n=%d: %d families on three or more units; staged blocks per class %s; %.1f s"
              % (c, dtype, h, w, variant, n, len(families), classes, time.time() - t0))
