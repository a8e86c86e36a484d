"""Helpers of the numeric-range tests (tests/test_range_host.py, tests/test_range_gpu.py): weights that make the network exactly
homogeneous, one operation scaled into fp16's overflow range, and the comparison rule for a 16-bit store that may overflow.

Why bias-free weights: with every BatchNorm beta / running mean and the head's bias at 0 every folded bias is exactly 0, so the
network is a composition of convolutions, sums, ReLUs, max-pools and nearest up-sampling: positively homogeneous of degree 1.  For
s = 2^k every product and every sum scales exactly (a power of two only moves the exponent) as long as nothing leaves the normal
range of fp32, and a rounding to bf16 commutes with it, so net(x * s) == net(x) * s bit for bit.  An absolute constant (an epsilon,
a clamp), or a detour through a narrower format anywhere on the way, breaks that equality at 2^+-48 and is invisible at order one."""
from collections import OrderedDict

import numpy as np
import torch

ULP16 = 2.0 ** -10            # adjacent fp16 values a < b (normal range): (b - a) / b <= 2^-10
NOISE = 2.0 ** -16            # tests/test_bf16_pin.py: fp32 summation in two orders, relative to sum |terms|
MAX_DIFF_FRAC = 0.01          # tests/test_bf16_pin.py: elements of one tensor that may differ at all
F16_MAX = 65504.0             # largest finite fp16
F16_OVERFLOW = 65520.0        # round-to-nearest-even: |x| >= 65520 = 65504 + half an ulp (the tie goes to the even side: inf) -> inf
F16_MIN_NORMAL = 2.0 ** -14
F16_SUBNORMAL_STEP = 2.0 ** -24   # spacing of the fp16 subnormals (and of the first normal binade)

SCALES = (-48, -16, 16, 48)   # k of s = 2^k in the exact-scaling tests


def bias_free(sd_np):
    """copy of a synth state dict with every ``*.bias`` (BatchNorm beta, ``final_layer.bias``) and ``*.running_mean`` at 0"""
    out = OrderedDict()
    for k, v in sd_np.items():
        a = np.array(v)
        if k.endswith(".bias") or k.endswith(".running_mean"):
            a[...] = 0
        out[k] = a
    return out


def scale_op(sd_np, bn_prefix, m):
    """copy with BatchNorm ``bn_prefix``'s ``.weight`` multiplied by 2^m: the output of the operation it belongs to (before a
    residual is added) scales by 2^m, exactly"""
    out = OrderedDict((k, np.array(v)) for k, v in sd_np.items())
    out[bn_prefix + ".weight"] = (out[bn_prefix + ".weight"] * np.float32(2.0 ** m)).astype(np.float32)
    return out


def f16r(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float16).to(torch.float32)


def compare_with_overflow(got, want_unrounded, mag, ulp=ULP16, noise=NOISE, max_diff_frac=MAX_DIFF_FRAC, max_ambiguous_frac=MAX_DIFF_FRAC,
                          mask=None, name="tensor", emulated_input=False):
    """The fp16 comparison of ONE operation whose inputs are finite: ``got`` is what the engine stored, ``want_unrounded`` the
    emulation's fp32 value before its storing rounding, ``mag`` the sum of |terms| per element.

    Per element b = one fp16 ulp of the value + noise * mag  (+ 2^-24, the subnormal spacing, where |fp16(want)| < 2^-14):
      |want_unrounded| >= 65520 + b   ->  got must be inf with want's sign
      |want_unrounded| <= 65520 - b   ->  got must be finite and within b of fp16(want_unrounded)
      in between                      ->  either (a NaN, or an inf of the wrong sign, never); counted as ambiguous, and their
                                          share of the tensor is capped.
    At most ``max_diff_frac`` of the elements may differ from the emulation at all.  ``mask``: elements to look at (default all).
    ``emulated_input``: an input of the op never reaches HBM and was emulated from ITS stored inputs; the engine rounded its own
    value of it, so -- exactly as tests/test_bf16_pin.py allows -- max(4, 2e-4 of the tensor) finite elements may miss b, by no more
    than one ulp of the sum of |terms|.
    Raises AssertionError; returns the counts."""
    got, wu, mag = got.double(), want_unrounded.double(), mag.double()
    assert bool(torch.isfinite(wu).all()) and bool(torch.isfinite(mag).all()), "%s: the emulation's own value is not finite (an input was not)" % name
    if mask is None:
        mask = torch.ones_like(got, dtype=torch.bool)
    total = int(mask.sum())
    assert total > 0, "%s: nothing to compare" % name
    w16 = f16r(want_unrounded.float()).double()
    gfin = torch.isfinite(got)
    gabs = torch.where(gfin, got.abs(), torch.zeros_like(got))
    b = ulp * torch.maximum(gabs, wu.abs()) + noise * mag
    b = b + F16_SUBNORMAL_STEP * (w16.abs() < F16_MIN_NORMAL).double()
    must_inf = (wu.abs() >= F16_OVERFLOW + b) & mask
    must_fin = (wu.abs() <= F16_OVERFLOW - b) & mask
    amb = mask & ~must_inf & ~must_fin
    right_inf = torch.isinf(got) & (torch.sign(got) == torch.sign(wu))
    w16f = torch.where(torch.isfinite(w16), w16, torch.zeros_like(w16))
    bad_inf = must_inf & ~right_inf
    bad_fin = must_fin & ~(gfin & ((got - w16f).abs() <= b))
    if emulated_input:
        loose = bad_fin & gfin & ((got - w16f).abs() <= ulp * mag)
        if int(loose.sum()) <= max(4, int(2e-4 * total)):
            bad_fin = bad_fin & ~loose
    bad_amb = amb & ~(gfin | right_inf)
    bad = bad_inf | bad_fin | bad_amb
    differ = (must_fin & ~(gfin & (got == w16f))) | bad_inf
    stats = dict(total=total, inf_due=int(must_inf.sum()), neg_inf_due=int((must_inf & (wu < 0)).sum()), ambiguous=int(amb.sum()),
                 differ_frac=float(differ.sum()) / total, bad=int(bad.sum()))
    if stats["bad"]:
        idx = torch.nonzero(bad)[:6]
        where = "; ".join("%s got %.8g want %.8g (fp16 %.8g) bound %.3g" % (tuple(int(v) for v in ix), float(got[tuple(ix)]), float(wu[tuple(ix)]),
                                                                              float(w16[tuple(ix)]), float(b[tuple(ix)])) for ix in idx)
        raise AssertionError("%s: %d of %d elements break the fp16 store rule (%d finite where inf is due or wrong sign, %d wrong or non-finite "
                             "where a finite value is due, %d NaN / wrong-sign inf near the threshold); first: %s"
                             % (name, stats["bad"], total, int(bad_inf.sum()), int(bad_fin.sum()), int(bad_amb.sum()), where))
    assert stats["ambiguous"] <= max_ambiguous_frac * total, "%s: %d of %d elements are within the bound of the overflow threshold (allowed %.2f %%): the case decides nothing" % (
        name, stats["ambiguous"], total, 100 * max_ambiguous_frac)
    assert stats["differ_frac"] <= max_diff_frac, "%s: %.2f %% of the elements differ from the emulation (allowed %.2f %%)" % (
        name, 100 * stats["differ_frac"], 100 * max_diff_frac)
    return stats


# ---- one operation per kernel family pushed over fp16's range -----------------------------------------------------------------------
# Per family: the call (model, c, h, w, n, switches), the op that overflows, the BatchNorm(s) scaled by 2^m, the conv_infos().algo the
# GPU test expects of the op (None: recognised otherwise, e.g. by what the plan keeps on-chip) and the tensor that is compared (the
# op itself, or for conv1 of a fused BasicBlock -- never stored -- the block's conv2).  m was chosen on the CPU from the fp16
# emulation; tests/test_range_host.py asserts the conditions for every row, so a changed generator cannot quietly empty a case.
# The fuse sum has no BatchNorm of its own: each of its three terms is scaled to just below 65504 (fractional m) so that every
# input stays finite and only the sum overflows.
FUSED = {"HRN_BBF_MIN_TILES": "1", "HRN_S2_MIN_TILES": "1"}
OVERFLOW_CASES = {
    # family:            model,        c,  h,   w,  n, env,   op,                               {bn: m},                                   algo, check
    "fused_stem":       ("HRNet",      48, 128, 96, 2, {},    "conv2",                          {"bn2": 7},                                None, "conv2"),
    "layer1_chain":     ("HRNet",      48, 128, 96, 2, {},    "layer1.2.conv1",                 {"layer1.2.bn1": 9},                        0, "layer1.2.conv1"),
    "lds_basicblock":   ("HRNet",      32, 64,  64, 2, {},    "stage2.0.branches.0.0.conv1",    {"stage2.0.branches.0.0.bn1": 11},          1, "stage2.0.branches.0.0.conv1"),
    "fused_bb_conv2":   ("HRNet",      48, 128, 96, 2, FUSED, "stage2.0.branches.0.0.conv2",    {"stage2.0.branches.0.0.bn2": 12},          2, "stage2.0.branches.0.0.conv2"),
    "fused_bb_conv1":   ("HRNet",      48, 128, 96, 2, FUSED, "stage2.0.branches.0.1.conv1",    {"stage2.0.branches.0.1.bn1": 11},          2, "stage2.0.branches.0.1.conv2"),
    "n96":              ("HRNet",      48, 128, 96, 2, {},    "stage2.0.branches.1.0.conv1",    {"stage2.0.branches.1.0.bn1": 11},          3, "stage2.0.branches.1.0.conv1"),
    "s2_slab":          ("HRNet",      48, 128, 96, 2, FUSED, "stage2.0.fuse_layers.1.0.0.0",   {"stage2.0.fuse_layers.1.0.0.1": 10},       4, "stage2.0.fuse_layers.1.0.0.0"),
    "generic_1x1":      ("HRNet",      48, 128, 96, 2, {},    "stage2.0.fuse_layers.0.1.0",     {"stage2.0.fuse_layers.0.1.1": 10},         0, "stage2.0.fuse_layers.0.1.0"),
    "fuse_sum":         ("HRNet",      48, 128, 96, 2, {},    "stage3.0.fuse.0",                {"stage3.0.branches.0.3.bn2": 9.75, "stage3.0.fuse_layers.0.1.1": 8.8, "stage3.0.fuse_layers.0.2.1": 9.8}, None, "stage3.0.fuse.0"),
    "deconv_phase":     ("PoseResNet", 50, 128, 96, 2, {},    "deconv_layers.0",                {"deconv_layers.1": 11},                    None, "deconv_layers.0"),
}
OVERFLOW_SEED = 5
# The crops of these cases are N(0, 1) * 2^10: fp16 keeps the folded WEIGHTS too, so a BatchNorm scale alone cannot lift an order-0.1
# activation over 65504 without overflowing the weights first (|W'| ~ 0.1 * 2^m).  The bias-free net is homogeneous, so the larger
# input lifts every tensor to order 100 (stem: 4e3, all finite) and the op's own 2^m stays within the weights' range.
OVERFLOW_INPUT_SCALE = 2.0 ** 10


def overflow_weights(synth, family):
    """numpy state dict of the case: the synth checkpoint, bias-free, the case's BatchNorm(s) scaled"""
    model, c, h, w, n, env, op, scales, algo, check = OVERFLOW_CASES[family]
    sd = bias_free(synth.synth_state_dict(c, 17, 0) if model == "HRNet" else synth.synth_state_dict(c, 17, 7, model="PoseResNet"))
    for bn, m in scales.items():
        sd = scale_op(sd, bn, m)
    return sd


def overflow_crops(synth, family):
    model, c, h, w, n = OVERFLOW_CASES[family][:5]
    x = synth.synth_crops(n, h, w, seed=OVERFLOW_SEED) * np.float32(OVERFLOW_INPUT_SCALE)
    if family == "fused_bb_conv1":
        # conv2 reads all 48 channels of a 3x3 window of conv1: with overflow spread evenly no window would be free of it.  So the
        # crops are quiet (1 / 16 of the amplitude) except for one patch at the bottom edge of crop 0: conv1 overflows under the
        # patch only -- next to the pad row crop 0 shares with crop 1 -- and everything else must come out as if nothing had happened.
        gain = np.full((n, 1, h, w), 1.0 / 16.0, np.float32)
        gain[0, :, h - 48:, 24:72] = 1.0
        x = x * gain
    return x


def forward_until(emu, crops, name):
    """the emulation run from the crops up to and including node ``name``: {node: stored value} of ``name``'s inputs, and what
    ``eval_node(name, ..., magnitude=True, unrounded=True)`` returns"""
    vals = {emu.INPUT: crops.to(torch.float32)}
    needed = set()

    def need(n):
        if n in needed or n == emu.INPUT:
            return
        needed.add(n)
        for i in emu.inputs_of(n):
            need(i)

    need(name)
    for nd in emu.order:
        if nd in needed and nd != name:
            vals[nd] = emu.eval_node(nd, vals)
    ins = {i: vals[i] for i in emu.inputs_of(name)}
    return ins, emu.eval_node(name, ins, magnitude=True, unrounded=True)


def overflow_preconditions(ins, want_unrounded, mag):
    """the figures the issue's four conditions are about, for one (op, m)"""
    wu, mag = want_unrounded.double(), mag.double()
    b = ULP16 * wu.abs() + NOISE * mag
    clear = wu.abs() >= F16_OVERFLOW + b
    amb = (wu.abs() > F16_OVERFLOW - b) & ~clear
    return dict(max_over_f16max=float(wu.abs().max()) / F16_MAX, clear=int(clear.sum()), clear_neg=int((clear & (wu < 0)).sum()),
                ambiguous_frac=float(amb.double().mean()), inputs_finite=all(bool(torch.isfinite(v).all()) for v in ins.values()))


def clean_window_mask(conv1_unrounded, conv1_mag, cout):
    """for conv2 of a fused BasicBlock whose conv1 overflowed in LDS: (n, cout, h, w) bool, True where the 3x3 window of the output
    pixel holds no conv1 element (any channel) that overflows or may overflow by the emulation"""
    wu = conv1_unrounded.double().abs()
    b = ULP16 * wu + NOISE * conv1_mag.double()
    dirty = (wu > F16_OVERFLOW - b).any(1, keepdim=True).float()
    dirty = torch.nn.functional.max_pool2d(dirty, 3, 1, 1) > 0
    return (~dirty).expand(-1, cout, -1, -1)


# ---- poison ------------------------------------------------------------------------------------------------------------------------
POISONS = ("nan_pixel", "pinf_pixel", "ninf_pixel", "nan_crop", "huge_crop")


def poison(crop: torch.Tensor, kind: str) -> torch.Tensor:
    """a copy of one (3, H, W) crop with the poison of ``kind``; the pixel kinds hit one interior pixel of the middle plane"""
    c = crop.clone()
    _, h, w = c.shape
    if kind == "nan_pixel":
        c[1, h // 2 + 1, w // 2 - 1] = float("nan")
    elif kind == "pinf_pixel":
        c[1, h // 2 + 1, w // 2 - 1] = float("inf")
    elif kind == "ninf_pixel":
        c[1, h // 2 + 1, w // 2 - 1] = float("-inf")
    elif kind == "nan_crop":
        c[...] = float("nan")
    elif kind == "huge_crop":    # +-3e38: finite in fp32, overflows at the first accumulation (and at the 16-bit conversion of the stem)
        c = torch.where(c >= 0, torch.full_like(c, 3e38), torch.full_like(c, -3e38))
    else:
        raise ValueError(kind)
    return c
