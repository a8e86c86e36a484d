"""The shapes the per-operation pins run at reach every kernel form any legal resolution reaches (tests/plan_census.py).

Plan-only handles, no GPU: for W48, W32 and PoseResNet-50 in bf16 and fp32 the census of every legal (H, W) -- H up to 512, W up
to the first width past which the set of forms of a width has not changed for eight steps of 32 -- is compared with the census of
``PIN_SHAPES``, under the switches the GPU tests set (plan_census.VARIANTS), for the call they make (three crops, ``max_batch`` 4).
fp16 plans are the bf16 plans (tests/test_fp16_host.py at the standard shapes, here at the corners of the sweep).  A second test
writes down the widths at which the forms of a 32-row crop change: a planner change that moves a threshold fails it loudly instead
of silently uncovering a regime.

The call-size axis (plan_census.walk_of): a second sweep, with the default switches and ``n = max_batch`` = 64 and 256 -- the two batch
sizes BASELINE.json names -- collects how the blocks of every kernel family walk their work in a production call, and asserts that the
walk cases of tests/test_walk_pin_gpu.py reach every such walk."""
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
        for variant in C.PIN_VARIANTS:
            have = C.census(model, c, H, W, dtype, env=C.VARIANTS[variant])
            for key in want.get("both", []) + want.get(variant, []):
                assert key in have, (model, c, H, W, dtype, variant, key)


def test_fp16_plans_are_bf16_plans_at_the_corners_of_the_sweep():
    for model, c, dtype in CONFIGS:
        if dtype != "bf16":
            continue
        for H in (HEIGHTS[0], HEIGHTS[-1]):
            for W in (STEP, SWEEP_END[(model, c, dtype)]):
                for env in (C.VARIANTS[v] for v in C.PIN_VARIANTS):
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


# ---- the call-size axis

WALK_BATCHES = (64, 256)      # BASELINE.json's two batch sizes


@functools.lru_cache(maxsize=None)
def walk_sweep(model, c, dtype):
    """-> ({walk key: first (H, W, n) it shows at}, CPU seconds): default switches, n = max_batch, the resolutions of ``sweep``"""
    t0 = time.process_time()
    first = {}
    for W in range(STEP, SWEEP_END[(model, c, dtype)] + 1, STEP):
        for H in HEIGHTS:
            for n in WALK_BATCHES:
                for k in C.walk(model, c, H, W, dtype, n, n):
                    first.setdefault(k, (H, W, n))
    return first, time.process_time() - t0


def _walk_pins(model, c, dtype):
    """the walks the per-operation pins run: the walk cases, and the shape pins' two variants (one-tile blocks, three crops)"""
    keys = set()
    for case in C.WALK_CASES:
        if (case[0], case[1], case[4]) == (model, c, dtype):
            keys |= C.case_walk(case)
    for m, cc, H, W, dt, n in C.PIN_SHAPES:
        if (m, cc, dt) == (model, c, dtype):
            for variant in C.PIN_VARIANTS:
                keys |= C.walk(m, cc, H, W, dt, C.MAX_BATCH, n, C.VARIANTS[variant])
    return keys


def test_walk_cases_cover_every_walk_a_production_call_makes():
    """Every walk key a call of 64 or 256 crops makes at any legal resolution (same resolutions, models and dtypes as the form sweep:
    2768 resolutions x 2 batch sizes, the FULL product) is made by a walk case or a shape pin of the same model and dtype.  There is
    no exemption list.

    Measured on the build machine (one core): the form sweep 8.9 s of CPU time, this sweep 48 s -- block maps of 256 crops are larger
    and there is one handle per batch size.  The reduced sweep (all widths at the heights 32, 64, 256 and 512, all heights at the
    widths of PIN_SHAPES) took 18 s but LOST six walk keys the full product finds (first at 352 x 96, 416 x 288 and 96 x 1152:
    one-tile fused blocks that end ragged in a backward launch, two-tile compact blocks likewise, two-tile blocks of 128-pixel
    tiles), so the full product stays: nothing is left out."""
    cpu, total = 0.0, 0
    for cfg in CONFIGS:
        first, seconds = walk_sweep(*cfg)
        cpu += seconds
        total += len(first)
        pins = _walk_pins(*cfg)
        missing = {k: hwn for k, hwn in first.items() if k not in pins}
        assert not missing, "%s %d %s: no pinned case makes %s (walk: first (H, W, n) of the sweep that does)" % (cfg + (missing,))
    # every pitch the fused pass runs at slides in production, and a walk case slides at each
    assert {k[1] for k in walk_sweep("HRNet", 48, "bf16")[0] if k[0] == "slide"} == set(range(25, 74, 8))
    print("\n[walk census] %d walk keys over %d calls swept in %.1f s of CPU time" % (
        total, sum(len(WALK_BATCHES) * len(HEIGHTS) * (e // STEP) for e in SWEEP_END.values()), cpu))
    assert cpu < 240.0


def test_every_walk_case_is_needed_and_states_what_it_is_for():
    """WALK_FOR names, per case, walks that ONLY that case makes among the pins of its model and dtype -- so deleting any one case
    uncovers them and fails the cover test -- and the plan of the case really has them (tests/test_walk_pin_gpu.py asserts the same
    on the live handle).  The fp16 twins are in the table and their plans are their bf16 twins'."""
    assert len(set(C.WALK_CASES)) == len(C.WALK_CASES)
    walks = {case: C.case_walk(case) for case in C.WALK_CASES}
    for case, want in C.WALK_FOR.items():
        assert want and all(k in walks[case] for k in want), (C.case_id(case), [k for k in want if k not in walks[case]])
        if case in C.FP16_TWINS:
            twin = case[:4] + ("bf16",) + case[5:]
            assert twin in walks and walks[case] == walks[twin] and want == C.WALK_FOR[twin]
            continue
        cfg = (case[0], case[1], case[4])
        first, _ = walk_sweep(*cfg)
        others = set()
        for m, cc, H, W, dt, n in C.PIN_SHAPES:
            if (m, cc, dt) == cfg:
                for variant in C.PIN_VARIANTS:
                    others |= C.walk(m, cc, H, W, dt, C.MAX_BATCH, n, C.VARIANTS[variant])
        for other, keys in walks.items():
            if other != case and (other[0], other[1], other[4]) == cfg:
                others |= keys
        only = [k for k in want if k in first and k not in others]
        assert only, "%s: every walk it is in the table for is made by another case too" % C.case_id(case)
    assert set(C.FP16_TWINS) <= set(C.WALK_CASES)
    # the cover the issue names: bf16 for all three models, the fp32 LDS kernel on several 512- and 384-pixel tiles per block
    have = {(case[0], case[1], case[4]) for case in C.WALK_CASES}
    assert {("HRNet", 48, "bf16"), ("HRNet", 32, "bf16"), ("PoseResNet", 50, "bf16"), ("HRNet", 48, "fp16")} <= have
    fp32 = set().union(*[walks[k] for k in C.WALK_CASES if k[4] == "fp32"])
    for px in (512, 384):
        assert any(k[0] == "walk" and k[2] == 16 and k[5] == px and k[7] == 3 for k in fp32), px


def test_long_variant_reaches_class_3_within_the_block_map_caps():
    """the long variant's HRN_HALF_STAGES gives every staged form -- the 96-cout one at cin 384 included -- blocks of three tiles in a
    small launch, and a headline call under it stays inside what a block-map entry can hold (walk_of asserts the caps on every plan)"""
    keys = C.walk("HRNet", 48, 128, 1248, "bf16", 16, 16, C.VARIANTS["long"]) | C.walk("HRNet", 48, 384, 288, "bf16", 16, 16, C.VARIANTS["long"])
    forms = {k[1:7] for k in keys if k[0] == "walk"}
    assert (3, 32, 6, 0, 512, "plain") in forms and (2, 48, 3, 0, 512, "fused") in forms
    assert all(any(k[0] == "walk" and k[1:7] == f and k[7] == 3 for k in keys) for f in forms), sorted(keys, key=str)
    assert {u for u in map(C.unit_class, keys) if u and u[0][0] in ("run", "stem_run", "chain")} >= {(("stem_run",), 3), (("chain", "conv2"), 3)}
    for n in (64, 256):
        C.walk("HRNet", 48, 384, 288, "bf16", n, n, C.VARIANTS["long"])
        C.walk("HRNet", 48, 384, 288, "fp32", n, n, C.VARIANTS["long"])
    assert int(C.VARIANTS["long"]["HRN_HALF_STAGES"]) * 4 <= C.STAGED_TILES_CAP     # (x the long-block factor, HRN_LONG_FACTOR)


# The n at which the blocks of each staged form first hold two tiles, default switches, at the headline shapes (a handle of max_batch
# 256): form (algo, ks, nr, compact, pixels, mode) -> n.  A moved block-length rule (group_blocks: the 512-block target, the half-stage
# count, HRN_BBF_TPB_DIV) fails here.
FIRST_TWO_TILES = {
    ("HRNet", 48, 384, 288, "bf16"): {(1, 48, 3, 0, 384, "plain"): 34, (1, 32, 4, 0, 384, "plain"): 56, (3, 32, 6, 0, 512, "plain"): 80,
                                      (3, 32, 6, 1, 512, "plain"): 80, (2, 48, 3, 0, 512, "fused"): 80, (1, 32, 3, 0, 512, "plain"): 111},
    ("HRNet", 32, 256, 192, "bf16"): {(1, 32, 4, 0, 384, "plain"): 79, (1, 32, 2, 0, 512, "plain"): 165},
    ("PoseResNet", 50, 256, 192, "bf16"): {(1, 32, 4, 0, 128, "small"): 80, (1, 32, 4, 0, 384, "plain"): 124},
    ("HRNet", 48, 384, 288, "fp32"): {(1, 16, 3, 0, 128, "small"): 7, (1, 16, 2, 0, 128, "small"): 10, (1, 16, 3, 0, 512, "plain"): 26,
                                      (1, 16, 2, 0, 512, "plain"): 37},
}


@pytest.mark.parametrize("shape", list(FIRST_TWO_TILES), ids=lambda s: "%s%d-%dx%d-%s" % s)
def test_blocks_first_hold_two_tiles_where_the_table_says(shape):
    model, c, H, W, dtype = shape
    net = C._handle(model, c, H, W, dtype, 256, {})
    try:
        table, first = C.conv_table(net), {}
        for n in range(1, 257):
            for k in C.walk_of(net, n, table):
                if k[0] == "walk" and k[7] >= 2:
                    first.setdefault(k[1:7], n)
    finally:
        net.close()
    assert first == FIRST_TWO_TILES[shape]


@pytest.mark.parametrize("c,dtype,w", [(48, "bf16", 32), (48, "bf16", 96), (48, "bf16", 288), (48, "bf16", 1248), (32, "bf16", 1248), (48, "fp32", 32)],
                         ids=lambda v: str(v))
def test_pitch_sweep_calls_take_the_families_they_claim(c, dtype, w):
    """the calls of the GPU pitch sweep (plan_census.sweep_call) at a few widths: the long variant always runs; a family production
    walks on two or more units per block is either taken to three or more by one of the variants or is the one written down
    (SWEEP_DROPPED); every baseline is a plan of one-unit blocks"""
    runs, dropped = C.sweep_call("HRNet", c, w, dtype)
    assert runs[0][0] == "long" and dropped == C.sweep_dropped(c, dtype, w)
    assert [v for v, _, _ in runs] == {(48, "bf16", 32): ["long", "long_unfused"], (48, "bf16", 96): ["long", "long_unfused"],
                                       (48, "bf16", 288): ["long", "long_unfused"], (48, "bf16", 1248): ["long"],
                                       (32, "bf16", 1248): ["long", "long_small"], (48, "fp32", 32): ["long", "long_small"]}[(c, dtype, w)]
    for variant, n, families in runs:
        C.assert_long_plan(C.walk("HRNet", c, C.SWEEP_H, w, dtype, n, n, C.VARIANTS[variant]), families)
        C.assert_one_unit_plan(C.walk("HRNet", c, C.SWEEP_H, w, dtype, n, n, C.one_unit(variant)))
