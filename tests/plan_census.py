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

# every switch a test sets (tests/test_bf16_pin.py: ENV_KEYS) and the call-size switches: a census starts from none of them
SWITCHES = ("HRN_DISABLE_N96", "HRN_BBF", "HRN_BBF_MIN_TILES", "HRN_DISABLE_LDS", "HRN_DISABLE_LDS32", "HRN_DISABLE_CHAIN",
            "HRN_DISABLE_CHAIN_DS", "HRN_DISABLE_S2", "HRN_DISABLE_STEM_MFMA", "HRN_DISABLE_HEAD_MFMA", "HRN_DISABLE_GROUP",
            "HRN_DISABLE_DGROUP", "HRN_SMALL_TILES", "HRN_DISABLE_FGROUP", "HRN_S2_MIN_TILES", "HRN_DISABLE_COMPACT",
            "HRN_DISABLE_STEM_FUSE")

# The two variants every pin shape runs in.  "default": at these sizes the call-size rules send branch 0 and the stride-2
# convolutions to their small-call paths (two plain launches per BasicBlock, the generic kernel, 128-pixel tiles).  "forced": the
# fused pass and the slab kernel really run at that pitch, and the staged kernels walk the full tiles (512 / 384 pixels) the plan
# chose for the pitch -- with 128-pixel tiles the 512 -> 384 switch would never execute in a call of three narrow crops.
VARIANTS = {"default": {},
            "forced": {"HRN_BBF_MIN_TILES": "1", "HRN_S2_MIN_TILES": "1", "HRN_SMALL_TILES": "0"}}

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


_BLOCKS = np.zeros((1 << 18, 6), np.int32)        # the block maps of all grouped launches of a call, one behind the other
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
        table.append((algo, i.ks, i.nr, lib.hrn_conv_compact(h, k) if algo == 3 else 0, i.cin, i.out_h, i.ksize, i.stride))   # (only the 96-cout
                                                                                                                                #  form can be compact)
    return table, {("conv", ksize, stride, algo, ks, nr, compact) for algo, ks, nr, compact, _, _, ksize, stride in table}


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
    for env in VARIANTS.values():
        net = _handle(model, c, H, W, dtype, max_batch, env)
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
