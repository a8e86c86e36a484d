"""Which kernel FORMS a plan runs, as a set of keys, and the table of shapes the per-operation pins run at.

The planner picks a kernel by the row pitch ``wp = w + 1`` of every feature map, not by channel counts alone (ctx_plan.inc:
``conv3x3_lds_bm``, the 96-cout form's slab rows, ``conv3x3_lds_bbf_ok``, the compact-enumeration rule, ``s2_rows``,
``stem_fused_fits``, ``conv3x3_f32_bm``), and a call picks tile sizes by its size.  ``census`` names every form a call of ``n``
crops runs, from the plan queries of the C ABI on a plan-only handle; tests/test_plan_census.py sweeps every legal resolution and
asserts that ``PIN_SHAPES`` -- the shapes tests/test_shape_pin_gpu.py pins against the engine-arithmetic emulation, operation by
operation -- reaches every form the sweep reaches.

A form key is one of

    ("conv", ksize, stride, algo, ks, nr, compact)     per convolution (hrn_get_conv_info, hrn_conv_compact)
    ("tile", algo, ks, nr, compact, pixels, mode)      per staged 3x3 form: the M-tile length its blocks walk in this call
                                                       (512 / 384, or 128 in a small call) and the mode of the block -- "plain",
                                                       "fused" (the fused BasicBlock pass) or "small" (hrn_plan_block_map); a member
                                                       of a fusable BasicBlock (algo 2) that runs unfused counts as the plain form, algo 1
    ("slab", cin, rows, tiling)                        per problem of the stride-2 slab kernel that a call of n crops runs
                                                       (hrn_plan_s2_map): rows per tile as a class (1, 2, 3 = three or more -- the
                                                       kernel's row loop is generic past that) and how the tiles cut an image: "whole"
                                                       (one tile), "even", or "ragged" (the last tile is short)
    ("slab_fallback", cin)                             a slab problem whose call is too small: the same convolutions on the generic kernel
    ("slab_parts", cin, parts)                         the number of cout parts that share a slab problem's input (waves per part)
    ("stem_fused", 0 / 1)                              hrn_stem_fused
    ("head", slab pixels, slabs)                       the head / decode split of the call (hrn_plan_head_slabs); slabs as a class
                                                       (1, 2 = two or more)

Classes instead of raw counts keep the key about code paths: the raw rows per tile of the slab kernel is a different number at
nearly every width, and no finite table of shapes could reach each of them.
"""
import contextlib
import ctypes
import os

import numpy as np

from conftest import load_pkg
from walk_cases import WALK_FOR

# every switch a test sets (tests/test_bf16_pin.py: ENV_KEYS) and the call-size switches: a census starts from none of them
SWITCHES = ("HRN_DISABLE_N96", "HRN_BBF", "HRN_BBF_MIN_TILES", "HRN_DISABLE_LDS", "HRN_DISABLE_LDS32", "HRN_DISABLE_CHAIN",
            "HRN_DISABLE_CHAIN_DS", "HRN_DISABLE_S2", "HRN_DISABLE_STEM_MFMA", "HRN_DISABLE_HEAD_MFMA", "HRN_DISABLE_GROUP",
            "HRN_DISABLE_DGROUP", "HRN_SMALL_TILES", "HRN_DISABLE_FGROUP", "HRN_S2_MIN_TILES", "HRN_DISABLE_COMPACT",
            "HRN_DISABLE_STEM_FUSE", "HRN_HALF_STAGES", "HRN_BBF_TPB_DIV", "HRN_CHAIN_BLOCKS", "HRN_S2_BLOCKS", "HRN_LONG_FACTOR",
            "HRN_LONG_SHARE", "HRN_ALTERNATE", "HRN_BLOCK_ORDER")

# The two variants every pin shape runs in.  "default": at these sizes the call-size rules send branch 0 and the stride-2
# convolutions to their small-call paths (two plain launches per BasicBlock, the generic kernel, 128-pixel tiles).  "forced": the
# fused pass and the slab kernel really run at that pitch, and the staged kernels walk the full tiles (512 / 384 pixels) the plan
# chose for the pitch -- with 128-pixel tiles the 512 -> 384 switch would never execute in a call of three narrow crops.
#
# "long" (tests/test_walk_pin_gpu.py): the forced variant plus the block-length switches, so that a call of a few crops runs the loops
# only a large call runs otherwise -- staged and fused blocks of many tiles, slab and stem blocks that walk a run of tiles, chain-kernel
# waves that loop over fragments.  HRN_HALF_STAGES: group_blocks divides conv3_tiles_per_block by up to 64 in a small launch, and the
# form with the fewest tiles per half-stage is the 96-cout one at cin 384 (12 slices): 6144 * 7 / (18 * 12) / 64 = 3 tiles, the fp32
# form at 32 slices 6144 / 32 / 64 = 3; times the long-block factor 4 the (32, 2) form's 6144 stay below STAGED_TILES_CAP.
VARIANTS = {"default": {},
            "forced": {"HRN_BBF_MIN_TILES": "1", "HRN_S2_MIN_TILES": "1", "HRN_SMALL_TILES": "0"},
            "long": {"HRN_BBF_MIN_TILES": "1", "HRN_S2_MIN_TILES": "1", "HRN_SMALL_TILES": "0", "HRN_HALF_STAGES": "6144",
                     "HRN_BBF_TPB_DIV": "1", "HRN_CHAIN_BLOCKS": "2", "HRN_S2_BLOCKS": "1"}}
# "long_unfused": the same with the fused pass left to its call-size rule (the plain (48, 3) form on 512-pixel tiles, which a production
# call below HRN_BBF_MIN_TILES runs on several tiles per block); "long_small": the same with 128-pixel tiles left to theirs.
VARIANTS["long_unfused"] = {k: v for k, v in VARIANTS["long"].items() if k != "HRN_BBF_MIN_TILES"}
VARIANTS["long_small"] = {k: v for k, v in VARIANTS["long"].items() if k != "HRN_SMALL_TILES"}
# "staged*": the long staged and fused blocks alone, the chain kernel and the slab kernel at their default block counts -- for the calls
# of 128 and 256 crops (the only ones whose last tile is full, see WALK_CASES), where one block for the whole stem or two for layer1
# would take seconds per pass.
VARIANTS["staged"] = {k: v for k, v in VARIANTS["long"].items() if k not in ("HRN_CHAIN_BLOCKS", "HRN_S2_BLOCKS")}
VARIANTS["staged_unfused"] = {k: v for k, v in VARIANTS["staged"].items() if k != "HRN_BBF_MIN_TILES"}
VARIANTS["staged_small"] = {k: v for k, v in VARIANTS["staged"].items() if k != "HRN_SMALL_TILES"}
PIN_VARIANTS = ("default", "forced")      # the two every shape of PIN_SHAPES runs in

N_CROPS, MAX_BATCH = 3, 4     # three crops: the flat row index crosses image boundaries and the last tile is ragged


@contextlib.contextmanager
def switches(env):
    """the HRN_* switches of ``env`` and no others, for handles created inside the block (the library reads them at hrn_create)"""
    saved = {k: os.environ[k] for k in SWITCHES if k in os.environ}
    try:
        for k in saved:
            del os.environ[k]
        os.environ.update(env)
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


_BLOCKS = np.zeros((1 << 20, 6), np.int32)        # the block maps of all grouped launches of a call, one behind the other
_MEMBERS = np.zeros((256, 512), np.int32)         # per launch: descriptor -> convolution
_S2_BLOCKS = (ctypes.c_int32 * (3 * 65536))()
_S2_PARTS = (ctypes.c_int32 * (5 * 256))()
_MODES = {0: "plain", 1: "fused", 2: "small"}


def conv_table(net):
    """per convolution (algo, ks, nr, compact, cin, out_h), and the "conv" keys: what of ``conv_infos()`` the census reads, as plain
    tuples (the two variants of a shape share it: their switches move call-size thresholds, not the convolution table)"""
    lib, h = net._lib, net._h
    i, table = load_pkg("_lib").ConvInfo(), []
    ref = ctypes.byref(i)
    for k in range(lib.hrn_conv_count(h)):
        assert lib.hrn_get_conv_info(h, k, ref) == 0
        algo = i.algo
        table.append((algo, i.ks, i.nr, lib.hrn_conv_compact(h, k) if algo == 3 else 0, i.cin, i.out_h, i.ksize, i.stride, i.out_w))   # (only the
                                                                                                                        # 96-cout form can be compact)
    return table, {("conv", ksize, stride, algo, ks, nr, compact) for algo, ks, nr, compact, _, _, ksize, stride, _ in table}


def census_of(net, n, table=None):
    """the form keys of a call of ``n`` crops on ``net`` (a plan-only or a live handle); ``table``: its ``conv_table`` when the
    caller has it already"""
    lib, h = net._lib, net._h
    table, conv_keys = conv_table(net) if table is None else table
    assert lib.hrn_conv_count(h) == len(table)
    keys = set(conv_keys)
    keys.add(("stem_fused", int(net.stem_fused())))
    # every grouped launch of the staged kernels: its block map behind the previous one's, then ONE pass over all of them
    base, mbase, cap = _BLOCKS.ctypes.data, _MEMBERS.ctypes.data, len(_BLOCKS)
    counts, used = [], 0
    while True:
        nb = lib.hrn_plan_block_map(h, len(counts), n, 0, base + 24 * used, cap - used, mbase + 2048 * len(counts), 512)
        if nb < 0:
            break
        assert nb <= cap - used and len(counts) < len(_MEMBERS) - 1, "raise the census buffers"
        counts.append(nb)
        used += nb
    b = _BLOCKS[:used].astype(np.int64)
    code = b[:, 0] | (b[:, 4] << 8) | (b[:, 5] << 20) | (np.repeat(np.arange(len(counts)), counts) << 22)   # descriptor < 256, pixels < 4096, two flag bits
    for v in np.unique(code).tolist():
        algo, ks, nr, compact = table[int(_MEMBERS[v >> 22, v & 255]) & ((1 << 30) - 1)][:4]
        mode = _MODES[1 if (v >> 20) & 1 else (v >> 20) & 2]
        # (algo 2 = a member of a fusable BasicBlock: in a call too small for the fused pass it runs as the plain (48, 3) form, algo 1)
        keys.add(("tile", 1 if algo == 2 and mode != "fused" else algo, ks, nr, compact, (v >> 8) & 4095, mode))
    active = ctypes.c_int32()
    group = 0
    while True:
        r = lib.hrn_plan_s2_map(h, group, n, _S2_BLOCKS, 65536, _S2_PARTS, 256, ctypes.byref(active))
        if r < 0:
            break
        parts, nparts = _S2_PARTS[:5 * (r >> 20)], {}
        for k in range(0, len(parts), 5):
            nparts[parts[k]] = nparts.get(parts[k], 0) + 1
        for k in range(0, len(parts), 5):
            prob, conv, _, rows, tiles = parts[k:k + 5]
            count = nparts.pop(prob, 0)               # (the first part of a problem stands for it)
            if count:
                cin, out_h = table[conv][4:6]
                keys.add(("slab_parts", cin, count))
                if active.value:
                    keys.add(("slab", cin, _cls(rows, 3), "whole" if tiles == 1 else "ragged" if out_h % rows else "even"))
                else:
                    keys.add(("slab_fallback", cin))
        group += 1
    px = ctypes.c_int32()
    slabs = lib.hrn_plan_head_slabs(h, n, ctypes.byref(px))
    assert slabs > 0
    keys.add(("head", px.value, _cls(slabs, 2)))
    return keys


def _cls(v, top):
    return min(int(v), top)


# What the block maps can hold, read from the code: a staged block's tile count travels in the upper 16 bits of a signed int32
# (ctx_memory.inc: ``tiles << 16``; conv3x3_lds.inc / conv3x3_f32.hip: ``bm.x >> 16``) and its first tile in 29 bits; s2_blocks clamps
# a slab block's run to 64 tiles, and the fused stem's run (one problem cut into HRN_S2_BLOCKS blocks, not clamped) travels in 24 bits
# (``cnt << 8``).  ``walk_of`` asserts them on every plan it reads.
STAGED_TILES_CAP, STAGED_FIRST_CAP, SLAB_RUN_CAP, STEM_RUN_CAP = (1 << 15) - 1, (1 << 29) - 1, 64, (1 << 23) - 1
_WALK = (ctypes.c_int32 * 5)()
_CHAIN_FORMS = {0: "plain", 1: "shortcut", 2: "conv2", 3: "conv2_last"}


def walk_of(net, n, table=None):
    """the walk keys of a call of ``n`` crops on ``net``: how a block of every kernel family loops over its work

        ("walk", algo, ks, nr, compact, pixels, mode, tiles, direction, tail)
                                      per staged form (the fields of its "tile" key) and kind of block: ``tiles`` per block as a class
                                      (1, 2, 3 = three or more -- from the third tile on a block repeats the transition it made into the
                                      second); ``direction`` "fwd" / "back" as the pass walks that launch (every odd launch backwards:
                                      the blocks are dealt from the tensor's end, hrn_plan_launch_walk); ``tail``: "none", or the block
                                      holds the tensor's last tile, which is "full" or "ragged"
        ("slide", wp)                 a fused block of two or more tiles at row pitch wp: the tiles after its first carry conv1's halo
                                      rows over (raw pitch: the carry arithmetic is a function of it, and there are nine)
        ("run", cin, tiles)           slab kernel: the run of tiles of a block, as a class (hrn_plan_s2_map)
        ("stem_run", tiles)           the fused stem likewise
        ("chain", form, frags, direction)   chain kernel: fragments per wave of its grid-stride loop as a class (hrn_plan_launch_walk)
        ("direct", ksize, stride, nr, mr)   generic kernel, grouped launches: the M fragments per wave the call size selects
    """
    lib, h = net._lib, net._h
    table = (conv_table(net) if table is None else table)[0]
    keys = set()
    group = 0
    while lib.hrn_plan_launch_walk(h, 0, group, n, _WALK) == 0:
        back = _WALK[1]
        nb = lib.hrn_plan_block_map(h, group, n, back, _BLOCKS.ctypes.data, len(_BLOCKS), _MEMBERS.ctypes.data, 512)
        assert 0 <= nb <= len(_BLOCKS), "raise the census buffers"
        b = _BLOCKS[:nb].astype(np.int64)
        assert nb == 0 or (b[:, 2].max() <= STAGED_TILES_CAP and b[:, 2].min() >= 1 and b[:, 3].max() <= STAGED_FIRST_CAP)
        code = b[:, 0] | (b[:, 4] << 8) | (b[:, 5] << 20)
        for v in np.unique(code).tolist():
            algo, ks, nr, compact, _, out_h, _, _, out_w = table[int(_MEMBERS[0, v & 255]) & ((1 << 30) - 1)]
            px, mode = (v >> 8) & 4095, _MODES[1 if (v >> 20) & 1 else (v >> 20) & 2]
            m = n * out_h * out_w if compact else n * (out_h + 1) * (out_w + 1)       # (ctx_memory.inc: m_pixels)
            mtiles = -(-m // px)
            rows = b[code == v]
            assert (rows[:, 3] + rows[:, 2] <= mtiles).all()
            last = rows[:, 3] + rows[:, 2] == mtiles
            form = (1 if algo == 2 and mode != "fused" else algo, ks, nr, compact, px, mode)
            for c in np.unique(np.minimum(rows[:, 2], 3) * 2 + last).tolist():
                keys.add(("walk",) + form + (c >> 1, "back" if back else "fwd", ("ragged" if m % px else "full") if c & 1 else "none"))
            if mode == "fused" and rows[:, 2].max() >= 2:
                keys.add(("slide", out_w + 1))
        group += 1
    active, on_slab = ctypes.c_int32(), set()       # on_slab: the convolutions the slab kernel or the fused stem computes in this call
    group = -1 if net.stem_fused() else 0
    while True:
        r = lib.hrn_plan_s2_map(h, group, n, _S2_BLOCKS, 65536, _S2_PARTS, 256, ctypes.byref(active))
        if r < 0:
            break
        nb = r & ((1 << 20) - 1)
        assert nb <= 65536
        if active.value or group < 0:
            on_slab.update(_S2_PARTS[k + 1] for k in range(0, 5 * (r >> 20), 5))
            blocks = np.frombuffer(_S2_BLOCKS, np.int32, 3 * nb).reshape(nb, 3)
            cin_of = {_S2_PARTS[k]: table[_S2_PARTS[k + 1]][4] for k in range(0, 5 * (r >> 20), 5)}
            assert blocks[:, 1].min() >= 1 and blocks[:, 1].max() <= (STEM_RUN_CAP if group < 0 else SLAB_RUN_CAP)
            for prob, run in {(int(p), _cls(t, 3)) for p, t in np.unique(blocks[:, :2], axis=0)}:
                keys.add(("stem_run", run) if group < 0 else ("run", cin_of[prob], run))
        group += 1
    chain = 0
    while lib.hrn_plan_launch_walk(h, 1, chain, n, _WALK) == 0:
        keys.add(("chain", _CHAIN_FORMS[_WALK[4]], _cls(-(-_WALK[3] // _WALK[2]), 3), "back" if _WALK[1] else "fwd"))
        chain += 1
    px, group = ctypes.c_int32(), 0
    while True:
        _MEMBERS[0] = -1
        if lib.hrn_plan_direct_map(h, group, n, None, 0, _MEMBERS.ctypes.data, 512, ctypes.byref(px)) < 0:
            break
        # (hrn_plan_direct_map also lists the groups that are only the fallback of a slab launch: they do not run while it is active)
        for conv in _MEMBERS[0][_MEMBERS[0] >= 0].tolist():
            if conv not in on_slab:
                keys.add(("direct", table[conv][6], table[conv][7], table[conv][2], px.value // 64))
        group += 1
    return keys


def walk(model, c, H, W, dtype, max_batch, n, env=None):
    net = _handle(model, c, H, W, dtype, max_batch, env or {})
    try:
        return walk_of(net, n)
    finally:
        net.close()


def _handle(model, c, H, W, dtype, max_batch, env):
    with switches(env):
        return load_pkg().NativeHRNet(c, 17, (H, W), dtype, max_batch=max_batch, device=-1, model_name=model)


def census(model, c, H, W, dtype, max_batch=MAX_BATCH, n=N_CROPS, env=None):
    """the set of form keys of a call of ``n`` crops on a plan-only handle of this geometry, created under the switches ``env``"""
    net = _handle(model, c, H, W, dtype, max_batch, env or {})
    try:
        return census_of(net, n)
    finally:
        net.close()


def census_both(model, c, H, W, dtype, max_batch=MAX_BATCH, n=N_CROPS):
    """the forms of the two variants the pins run"""
    keys, table = set(), None
    for variant in PIN_VARIANTS:
        net = _handle(model, c, H, W, dtype, max_batch, VARIANTS[variant])
        try:
            table = conv_table(net) if table is None else table
            keys |= census_of(net, n, table)
        finally:
            net.close()
    return keys


# (model, c, H, W, dtype, n): the shapes tests/test_shape_pin_gpu.py runs, each in both variants.  What each is there for is
# stated -- and asserted on the live handle -- in that file (CHOSEN_FOR); test_plan_census.py asserts the cover.
PIN_SHAPES = [
    ("HRNet", 48, 32, 32, "bf16", 3),
    ("HRNet", 48, 224, 32, "bf16", 3),
    ("HRNet", 48, 32, 224, "bf16", 3),
    ("HRNet", 48, 32, 256, "bf16", 3),
    ("HRNet", 48, 32, 320, "bf16", 3),
    ("HRNet", 48, 32, 448, "bf16", 3),
    ("HRNet", 48, 64, 576, "bf16", 3),
    ("HRNet", 48, 32, 672, "bf16", 3),
    ("HRNet", 48, 32, 832, "bf16", 3),
    ("HRNet", 48, 64, 32, "bf16", 3),
    ("HRNet", 48, 160, 128, "bf16", 3),
    ("HRNet", 32, 32, 32, "bf16", 3),
    ("HRNet", 32, 64, 32, "bf16", 3),
    ("HRNet", 32, 32, 192, "bf16", 3),
    ("HRNet", 32, 224, 32, "bf16", 3),
    ("HRNet", 32, 32, 320, "bf16", 3),
    ("HRNet", 32, 64, 448, "bf16", 3),
    ("HRNet", 32, 32, 576, "bf16", 3),
    ("HRNet", 32, 32, 704, "bf16", 3),
    ("HRNet", 32, 32, 992, "bf16", 3),
    ("PoseResNet", 50, 32, 32, "bf16", 3),
    ("PoseResNet", 50, 32, 576, "bf16", 3),
    ("HRNet", 48, 32, 448, "fp16", 3),
    ("HRNet", 48, 32, 672, "fp16", 3),
    ("HRNet", 48, 32, 32, "fp32", 3),
    ("HRNet", 48, 32, 320, "fp32", 3),
    ("HRNet", 48, 32, 576, "fp32", 3),
    ("HRNet", 32, 32, 32, "fp32", 3),
    ("HRNet", 32, 32, 320, "fp32", 3),
    ("HRNet", 32, 32, 576, "fp32", 3),
    ("PoseResNet", 50, 32, 32, "fp32", 3),
    ("PoseResNet", 50, 32, 320, "fp32", 3),
    ("PoseResNet", 50, 32, 576, "fp32", 3),
]


# ---- the walk cases: calls of a few crops whose blocks walk the way a production call's do (tests/walk_cases.py: the table and what
# each case is in it for; tests/test_walk_pin_gpu.py pins each against the emulation; tests/test_plan_census.py asserts the cover).
# A case is (model, c, H, W, dtype, n, variant, HRN_HALF_STAGES or None = the variant's own): the handle has max_batch = n.  A case
# lowers HRN_HALF_STAGES where the walk it is there for needs blocks of exactly two tiles, or a tensor that holds several long blocks
# (a block that does NOT end on the tensor's last tile).  n = 128: the only small calls whose last tile is FULL -- an image of branches
# 0 to 2 is an odd number of flat rows, so n * rows is a multiple of the 128-, 384- or 512-pixel tile only when 128 divides n.
WALK_CASES = list(WALK_FOR)
# fp16 twins of the fused form (wp 57, 73) and of the 384-pixel tiles of the (48, 3) / (32, 3) and 96-cout forms
FP16_TWINS = [("HRNet", 48, 32, 224, "fp16", 3, "long", 256), ("HRNet", 48, 32, 288, "fp16", 3, "long", 256),
              ("HRNet", 48, 64, 352, "fp16", 3, "long", 1024), ("HRNet", 48, 32, 704, "fp16", 3, "long", 1024)]


def case_env(case):
    env = dict(VARIANTS[case[6]])
    if case[7] is not None:
        assert "HRN_HALF_STAGES" in env
        env["HRN_HALF_STAGES"] = str(case[7])
    return env


def case_id(case):
    model, c, h, w, dtype, n, variant, hs = case
    return "%s%d-%dx%d-%s-n%d-%s%s" % ("W" if model == "HRNet" else "R", c, h, w, dtype, n, variant, "" if hs is None else "-hs%d" % hs)


def case_walk(case):
    model, c, h, w, dtype, n = case[:6]
    return walk(model, c, h, w, dtype, n, n, case_env(case))


def unit_class(key):
    """(family, class) of a walk key that carries a units-per-block class, else None"""
    if key[0] == "walk":
        return key[:7], key[7]
    if key[0] in ("run", "chain"):
        return key[:2], key[2]
    if key[0] == "stem_run":
        return key[:1], key[1]
    return None


# ---- the pitch sweep of tests/test_walk_pin_gpu.py: at H = 32 and every legal width, long blocks against one-unit blocks, bit for bit.
# ONE_UNIT: the long variant's switches with one half-stage per staged block, and the two block caps so high that a slab or stem block
# holds one tile and a chain-kernel wave one fragment at EVERY call size (at their defaults, 256 and 512, that holds for the calls of up
# to about 30 crops only: the compact 96-cout form needs up to 86 crops of 32 x 96 for a block of three tiles, and the stem's 8 tiles per
# crop then exceed 256 blocks).  The block maps are sized for one tile per block (setup_s2groups), so no cap is passed.
def one_unit(variant):
    return dict(VARIANTS[variant], HRN_HALF_STAGES="1", HRN_CHAIN_BLOCKS="65536", HRN_S2_BLOCKS="65536")


ONE_UNIT = one_unit("long")
SWEEP_H = 32
_W16 = list(range(32, 1249, 32))
# fp16: a spread over the plan's thresholds (tests/test_plan_census.py: THRESHOLDS); fp32: conv3x3_f32_kernel is taken at EVERY width
# (the deep branches stay on it), so the widths are those at which its forms change (320, 576, 640), their lower neighbours, the
# narrowest and the widest of the fp32 sweep
SWEEP_WIDTHS = ([(c, "bf16", w) for c in (48, 32) for w in _W16] +
                [(c, "fp16", w) for c in (48, 32) for w in (32, 160, 288, 320, 416, 544, 704, 832, 1248)] +
                [(c, "fp32", w) for c in (48, 32) for w in (32, 288, 320, 544, 576, 608, 640, 896)])
_SWEEP_PROD_H, _SWEEP_MAX_N = (32, 128, 256, 384, 512), 64


SWEEP_VARIANTS = ("long", "long_unfused", "long_small")
# The only family production runs on several tiles per block that the sweep leaves at one or two: the compact 96-cout form of W48 from
# width 96 on -- at height 32 the branches it enumerates compactly hold fewer than three 512-pixel tiles of real pixels in any call of
# up to 64 crops.  (The walk cases pin that form on three and more tiles per block against the emulation, at heights 64 and 96.)
SWEEP_DROPPED = ("walk", 3, 32, 6, 1, 512, "plain")


def sweep_dropped(c, dtype, w):
    return {SWEEP_DROPPED} if c == 48 and dtype != "fp32" and w >= 96 else set()


def sweep_call(model, c, w, dtype):
    """-> (runs, dropped).  The families (``unit_class``) whose blocks hold two or more units in a production call (default switches,
    64 or 256 crops, heights 32 ... 512) at width ``w`` are dealt to the variants of SWEEP_VARIANTS in that order: ``runs`` is a list of
    (variant, n, families) -- the families the variant runs at (32, w) that no earlier variant took, and the fewest crops n with which
    it gives every one of them a block of three or more units; "long" always runs, "long_unfused" where production runs the plain
    (48, 3) form on several tiles per block below the fused pass's threshold (the long variant fuses those blocks), "long_small" where
    it runs 128-pixel tiles so.  ``dropped``: the families no variant takes to three units per block in a call of up to 64 crops of height 32
    (tests/test_plan_census.py writes them down)."""
    prod = set()
    for h in _SWEEP_PROD_H:
        for n in (64, 256):
            prod |= {u[0] for u in map(unit_class, walk(model, c, h, w, dtype, n, n)) if u and u[1] >= 2}
    runs, left = [], set(prod)
    for variant in SWEEP_VARIANTS:
        best = None       # the call that takes the most of the families to blocks of three or more units; the fewest crops of those
        for n in range(2, _SWEEP_MAX_N + 1):
            have = [u for u in map(unit_class, walk(model, c, SWEEP_H, w, dtype, n, n, VARIANTS[variant])) if u]
            want = {f for f in left if (f, 3) in have}
            if best is None or len(want) > len(best[1]):
                best = (n, want)
            if not left or n >= best[0] + 12:      # (nothing to take, or a dozen more crops have taken no further family)
                break
        if best[1] or variant == "long":
            runs.append((variant, best[0], best[1]))
            left -= best[1]
    return runs, left


def assert_long_plan(walks, families):
    have = {u for u in map(unit_class, walks) if u}
    missing = [f for f in families if (f, 3) not in have]
    assert families and not missing, "no block of three or more units for %s" % (missing,)


def assert_one_unit_plan(walks):
    long_ones = [k for k in walks if k[0] == "slide" or (unit_class(k) and unit_class(k)[1] != 1)]
    assert not long_ones, "the baseline has blocks of more than one unit: %s" % (long_ones,)


def staged_blocks_per_class(net, n):
    """[blocks of 1, of 2, of 3 or more tiles] over the staged launches of a call of n crops"""
    counts, group = [0, 0, 0], 0
    while True:
        nb = net._lib.hrn_plan_block_map(net._h, group, n, 0, _BLOCKS.ctypes.data, len(_BLOCKS), _MEMBERS.ctypes.data, 512)
        if nb < 0:
            return counts
        for k, v in zip(*np.unique(np.minimum(_BLOCKS[:nb, 2], 3), return_counts=True)):
            counts[int(k) - 1] += int(v)
        group += 1
