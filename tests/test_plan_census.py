"""The shapes the per-operation pins run at reach every kernel form any legal resolution reaches (tests/plan_census.py).

Plan-only handles, no GPU: for W48, W32 and PoseResNet-50 in bf16 and fp32 the census of every legal (H, W) -- H up to 512, W up
to the first width past which the set of forms of a width has not changed for eight steps of 32 -- is compared with the census of
``PIN_SHAPES``, under the switches the GPU tests set (plan_census.VARIANTS), for the call they make (three crops, ``max_batch`` 4).
fp16 plans are the bf16 plans (tests/test_fp16_host.py at the standard shapes, here at the corners of the sweep).  A second test
writes down the widths at which the forms of a 32-row crop change: a planner change that moves a threshold fails it loudly instead
of silently uncovering a regime."""
import functools
import time

import pytest

import plan_census as C

CONFIGS = [("HRNet", 48, "bf16"), ("HRNet", 48, "fp32"), ("HRNet", 32, "bf16"), ("HRNet", 32, "fp32"),
           ("PoseResNet", 50, "bf16"), ("PoseResNet", 50, "fp32")]
HEIGHTS = list(range(32, 513, 32))     # hrn_create takes any multiple of 32
STEP, STABLE_STEPS = 32, 8

# Where each sweep ends: the first width past which the union over H of the forms at a width has not changed for STABLE_STEPS
# steps.  The widest change is W32's at 992 (its last stride-2 convolutions leave the slab kernel), so the sweep covers W <= 1248.
SWEEP_END = {("HRNet", 48, "bf16"): 1184, ("HRNet", 48, "fp32"): 896, ("HRNet", 32, "bf16"): 1248, ("HRNet", 32, "fp32"): 896,
             ("PoseResNet", 50, "bf16"): 416, ("PoseResNet", 50, "fp32"): 896}

# Forms the sweep reaches that no pin shape runs, key -> reason.  At most three, and none of conv3x3_lds_kernel,
# conv_s2_slab_kernel, conv3x3_f32_kernel, stem_fused_kernel or the chain kernels ("tile", "slab", "stem_fused" keys and the
# "conv" keys of algo 1 - 4).
EXEMPT = {}


@functools.lru_cache(maxsize=None)
def sweep(model, c, dtype):
    """-> ({form: first (H, W) it shows at}, {W: forms of the 32-row crop}, last W swept, CPU seconds)"""
    t0 = time.process_time()
    first, low, prev, last_change, W = {}, {}, None, STEP, STEP
    while True:
        at_w = set()
        for H in HEIGHTS:
            keys = C.census_both(model, c, H, W, dtype)
            if H == HEIGHTS[0]:
                low[W] = keys
            for k in keys - at_w:
                first.setdefault(k, (H, W))
            at_w |= keys
        if prev is not None and at_w != prev:
            last_change = W
        prev = at_w
        if W - last_change >= STABLE_STEPS * STEP:
            break
        W += STEP
    return first, low, W, time.process_time() - t0


def _pins(model, c, dtype):
    keys = set()
    for m, cc, H, W, dt, n in C.PIN_SHAPES:
        if (m, cc, dt) == (model, c, dtype):
            keys |= C.census_both(m, cc, H, W, dt, n=n)
    return keys


def test_pin_shapes_cover_every_reachable_form():
    assert len(EXEMPT) <= 3
    for key in EXEMPT:
        assert key[0] in ("head", "slab_fallback", "slab_parts") or (key[0] == "conv" and key[3] == 0), "a hand-scheduled form may not be exempt: %s" % (key,)
    cpu = 0.0
    for cfg in CONFIGS:
        first, _, end, seconds = sweep(*cfg)
        cpu += seconds
        assert end == SWEEP_END[cfg], (cfg, end)
        pins = _pins(*cfg)
        missing = {k: hw for k, hw in first.items() if k not in pins and k not in EXEMPT}
        assert not missing, "%s %d %s: no pin shape runs %s (form: first (H, W) of the sweep that does)" % (cfg + (missing,))
    assert max(SWEEP_END.values()) >= 1056
    print("\n[plan census] %d resolutions swept in %.1f s of CPU time" % (sum(len(HEIGHTS) * (e // STEP) for e in SWEEP_END.values()), cpu))
    assert cpu < 30.0


def test_pin_shapes_state_what_they_are_for():
    """the table of tests/test_shape_pin_gpu.py (what each shape was chosen for, asserted there on the live handle) names forms the
    plan of that shape and variant really has"""
    from test_shape_pin_gpu import CHOSEN_FOR
    assert {s[:5] for s in C.PIN_SHAPES} == set(CHOSEN_FOR) and len(C.PIN_SHAPES) == len(CHOSEN_FOR)
    assert all(s[5] == C.N_CROPS for s in C.PIN_SHAPES)
    for (model, c, H, W, dtype), want in CHOSEN_FOR.items():
        assert want["why"] and set(want) <= {"why", "both", "default", "forced"}
        for variant, env in C.VARIANTS.items():
            have = C.census(model, c, H, W, dtype, env=env)
            for key in want.get("both", []) + want.get(variant, []):
                assert key in have, (model, c, H, W, dtype, variant, key)


def test_fp16_plans_are_bf16_plans_at_the_corners_of_the_sweep():
    for model, c, dtype in CONFIGS:
        if dtype != "bf16":
            continue
        for H in (HEIGHTS[0], HEIGHTS[-1]):
            for W in (STEP, SWEEP_END[(model, c, dtype)]):
                for env in C.VARIANTS.values():
                    assert C.census(model, c, H, W, "fp16", env=env) == C.census(model, c, H, W, "bf16", env=env), (model, c, H, W)
    # ... and every fp16 pin shape stands for its bf16 twin
    for m, c, H, W, dt, n in C.PIN_SHAPES:
        if dt == "fp16":
            assert C.census_both(m, c, H, W, "fp16", n=n) == C.census_both(m, c, H, W, "bf16", n=n)


# The widths at which the forms of a 32-row crop change (both variants, three crops), W -> (forms gained, forms lost) against the
# width 32 below.  W48 bf16: at 256 branch 1 leaves compact enumeration and the stem's conv2 the slab kernel; at 320 the stem is no
# longer fused and branch 0 goes from the fused pass to two launches, on 384-pixel tiles; at 448 branch 0 leaves the LDS-staged
# kernel (generic, nr 3); at 576 layer1.0's 3x3 and transition1 follow (nr 4); at 672 the nr-3 slab convolutions fall back to the
# generic kernel; at 704 branch 1's 96-cout form drops to 384-pixel tiles.  The "slab" and "head" entries in between are the
# call-size classes of the richer key (rows per tile, tiles per image, slabs per heat-map).
THRESHOLDS = {
    ('HRNet', 48, 'bf16'): {
        64: ([('slab', 64, 3, 'ragged')],
              [('slab', 64, 3, 'whole')]),
        160: ([('head', 256, 2)],
              [('head', 256, 1)]),
        192: ([('slab', 64, 2, 'even')],
              [('slab', 64, 3, 'ragged')]),
        256: ([('conv', 3, 1, 3, 32, 6, 0), ('conv', 3, 2, 0, 0, 4, 0), ('tile', 3, 32, 6, 0, 128, 'small'), ('tile', 3, 32, 6, 0, 512, 'plain')],
              [('conv', 3, 2, 4, 0, 4, 0), ('slab', 64, 2, 'even'), ('slab_fallback', 64), ('slab_parts', 64, 2)]),
        320: ([('conv', 3, 1, 1, 48, 3, 0), ('stem_fused', 0), ('tile', 1, 32, 3, 0, 384, 'plain'), ('tile', 1, 48, 3, 0, 384, 'plain')],
              [('conv', 3, 1, 2, 48, 3, 0), ('stem_fused', 1), ('tile', 1, 32, 3, 0, 512, 'plain'), ('tile', 2, 48, 3, 0, 512, 'fused')]),
        384: ([('slab', 48, 3, 'ragged')],
              [('slab', 48, 3, 'whole')]),
        448: ([('conv', 3, 1, 0, 0, 3, 0)],
              [('conv', 3, 1, 1, 48, 3, 0), ('tile', 1, 48, 3, 0, 128, 'small'), ('tile', 1, 48, 3, 0, 384, 'plain')]),
        480: ([('slab', 48, 2, 'even')],
              [('slab', 48, 3, 'ragged')]),
        576: ([('conv', 3, 1, 0, 0, 4, 0)],
              [('conv', 3, 1, 1, 32, 3, 0), ('conv', 3, 1, 1, 32, 4, 0), ('tile', 1, 32, 3, 0, 128, 'small'), ('tile', 1, 32, 3, 0, 384, 'plain'), ('tile', 1, 32, 4, 0, 128, 'small'), ('tile', 1, 32, 4, 0, 384, 'plain')]),
        672: ([('conv', 3, 2, 0, 0, 3, 0)],
              [('slab', 48, 2, 'even'), ('slab_parts', 48, 2), ('slab_parts', 48, 3)]),
        704: ([('tile', 3, 32, 6, 0, 384, 'plain')],
              [('tile', 3, 32, 6, 0, 512, 'plain')]),
        832: ([('tile', 3, 32, 6, 0, 512, 'plain')],
              []),
    },
    ('HRNet', 48, 'fp32'): {
        160: ([('head', 256, 2)],
              [('head', 256, 1)]),
        320: ([('tile', 1, 16, 2, 0, 384, 'plain'), ('tile', 1, 16, 3, 0, 384, 'plain')],
              [('tile', 1, 16, 2, 0, 512, 'plain')]),
        576: ([('conv', 3, 1, 0, 0, 3, 0), ('conv', 3, 1, 0, 0, 4, 0)],
              [('conv', 3, 1, 1, 16, 2, 0), ('tile', 1, 16, 2, 0, 128, 'small'), ('tile', 1, 16, 2, 0, 384, 'plain'), ('tile', 1, 16, 3, 0, 384, 'plain')]),
        640: ([('tile', 1, 16, 3, 0, 384, 'plain')],
              []),
    },
    ('HRNet', 32, 'bf16'): {
        64: ([('slab', 64, 3, 'ragged')],
              [('slab', 64, 3, 'whole')]),
        160: ([('head', 256, 2)],
              [('head', 256, 1)]),
        192: ([('slab', 64, 2, 'even')],
              [('slab', 64, 3, 'ragged')]),
        256: ([],
              [('slab', 64, 2, 'even'), ('slab_parts', 64, 2)]),
        320: ([('stem_fused', 0), ('tile', 1, 32, 2, 0, 384, 'plain')],
              [('stem_fused', 1), ('tile', 1, 32, 2, 0, 512, 'plain')]),
        576: ([('conv', 3, 1, 0, 0, 4, 0), ('slab', 32, 3, 'ragged')],
              [('conv', 3, 1, 1, 32, 2, 0), ('slab', 32, 3, 'whole'), ('tile', 1, 32, 2, 0, 128, 'small'), ('tile', 1, 32, 2, 0, 384, 'plain')]),
        704: ([('slab', 32, 2, 'even')],
              [('slab', 32, 3, 'ragged')]),
        960: ([],
              [('slab', 64, 2, 'whole'), ('slab_parts', 64, 4), ('slab_parts', 64, 6)]),
        992: ([('conv', 3, 2, 0, 0, 2, 0)],
              [('slab', 32, 2, 'even'), ('slab_parts', 32, 2), ('slab_parts', 32, 3)]),
    },
    ('HRNet', 32, 'fp32'): {
        160: ([('head', 256, 2)],
              [('head', 256, 1)]),
        320: ([('tile', 1, 16, 2, 0, 384, 'plain')],
              []),
        576: ([('conv', 3, 1, 0, 0, 2, 0), ('conv', 3, 1, 0, 0, 4, 0)],
              [('tile', 1, 16, 2, 0, 384, 'plain')]),
        640: ([('tile', 1, 16, 2, 0, 384, 'plain')],
              []),
    },
    ('PoseResNet', 50, 'bf16'): {
        160: ([('head', 256, 2)],
              [('head', 256, 1)]),
    },
    ('PoseResNet', 50, 'fp32'): {
        160: ([('head', 256, 2)],
              [('head', 256, 1)]),
        320: ([('tile', 1, 16, 2, 0, 384, 'plain')],
              []),
        576: ([('conv', 3, 1, 0, 0, 4, 0)],
              [('tile', 1, 16, 2, 0, 384, 'plain')]),
        640: ([('tile', 1, 16, 2, 0, 384, 'plain')],
              []),
    },
}


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "%s%d-%s" % c)
def test_threshold_widths_are_where_the_table_says(cfg):
    _, low, end, _ = sweep(*cfg)
    moved = {}
    for W in range(2 * STEP, end + 1, STEP):
        if low[W] != low[W - STEP]:
            moved[W] = (sorted(low[W] - low[W - STEP], key=str), sorted(low[W - STEP] - low[W], key=str))
    want = THRESHOLDS[cfg]
    assert sorted(moved) == sorted(want), "the plan changes at widths %s, the table says %s" % (sorted(moved), sorted(want))
    for W in want:
        assert moved[W] == want[W], "W = %d: gained / lost %s, the table says %s" % (W, moved[W], want[W])
