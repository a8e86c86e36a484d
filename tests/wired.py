"""Heat-maps with designed values, through the real network: the inputs of tests/test_wired_host.py (CPU oracles) and
tests/test_argmax_gpu.py (the head, decode and score kernels on the MI355X).

The head's arg-max follows np.argmax (SimpleHRNet.py:300): among equal maxima the first cell in row-major order wins.
csrc/argmax.h states that order twice -- ``takes`` for a scan that visits cells in increasing order, ``better`` for every merge of
two candidates -- and a heat-map of a random trunk never holds two equal cells, so neither limb decides anything on random data.
Two constructions put chosen values into chosen cells of a map the real kernels produce:

**Wired checkpoint** (HRNet).  ``synth_state_dict`` with S = 3 signal channels laid through the identity paths
``synth.peaked_state_dict`` names, exactly: every convolution that WRITES channels [:S] of a signal-carrying tensor has those rows
(and the BatchNorm bias / running_mean) zeroed, four of them carry an identity tap instead (conv1, conv2, transition1.0.0 on the
centre tap, layer1.0.downsample.0 on its only tap; BatchNorm weight 1 and running_var = float32(1 - 1e-5), whose folded scale
1 / sqrt(var + 1e-5) rounds to exactly 1.0f -- with var = 1 it is 0.999995 and the fp32 network misses the design by 1.4e-4);
every convolution that READS such a tensor has the input slice [:, :S] zeroed on its other rows, so the random trunk never sees
the signal either.  ``final_layer`` reads only the signals: weight[:, :S] = mix, entries in {-1, 0, +1}.  Crops are
``synth_crops`` (the trunk stays alive in the other channels) with ``crops[:, :, ::4, ::4]`` overwritten by the designed planes
(the two stride-2 / pad-1 centre taps read exactly those pixels).  Planes hold small non-negative integers -- exact in bf16 and
fp16, and passed by every ReLU -- so

    heatmaps[n, j, y, x] = sum_s mix[j, s] * plane[n, s, y, x] + bias[j]      exactly, in fp32, bf16 and fp16.

Non-finite values cannot be designed this way (a zero weight times inf is NaN in every other channel's sum): they stay with the
bias-based tests (tests/test_round2_gpu.py, tests/test_score_gpu.py).

**Zero-set heads** (any model; PoseResNet has no identity path).  The tensor the head reads is post-ReLU and holds exact zeros.
Pass 1 taps it; ``zero_set_heads`` picks per joint a channel set whose common zero cells are few but at least two in every crop;
the head gets weight -1 on that set, 0 elsewhere, bias b_j.  Map j of pass 2 is <= b_j everywhere and == b_j on the common zero
set: at least two equal maxima, wherever the trunk put them.

**Where two cells meet** (``walk`` / ``tie_class``), read from csrc/kernels.hip.  A block owns one slab of ``slab_px`` cells of one
crop; ``decode_kernel`` merges the slabs' candidates.  Within a slab (r = px % slab_px):

  MFMA head (head_mfma_group; bf16 / fp16):   wave = r // (slab_px / 4);  trip = (r % (slab_px / 4)) // 16;  lane = px % 16.
      A lane scans its cell of every trip of its wave (``takes``), a 4-step butterfly merges the 16 lanes (``better``), thread j
      merges the 4 waves in wave order through LDS (``better``).
  VALU head (head_group; fp32, or HRN_DISABLE_HEAD_MFMA=1):   thread = r % 256;  wave = thread // 64;  trip = r // 256.
      A thread scans its cell of every trip (``takes``), a 6-step butterfly merges the 64 threads of a wave, then the 4 waves.

Two cells p < q meet where their paths join:  different slabs -> ``slab`` (decode_kernel);  else different waves -> ``wave`` (the
LDS merge);  else different lanes / threads -> ``lane`` (the butterfly: each was first taken by the scan of its own lane, whatever
its trip);  else -> ``trip`` (one lane's scan sees both, ``takes`` decides).  ``tie_level`` is the coarser key by coordinates
alone (slab, wave, trip, lane in that order): it says how far apart two cells sit, not which instruction decides.
"""
import importlib
import re

import numpy as np

S = 3
NO_IDX = 0x7fffffff
CLASSES = ("lane", "trip", "wave", "slab")
STAGES = (("stage2.0", 2, 2), ("stage3.0", 3, 3), ("stage3.1", 3, 3), ("stage3.2", 3, 3), ("stage3.3", 3, 3),
          ("stage4.0", 4, 4), ("stage4.1", 4, 4), ("stage4.2", 4, 1))
HEAD_TAP = {"HRNet": "stage4.2.fuse.0", "PoseResNet": "deconv_layers.6"}


def _synth():
    return importlib.import_module("simple-hrnet_amd.synth")


# ------------------------------------------------------------------------------------------------------------ the wired checkpoint
def _bn_of(conv):
    if conv in ("conv1", "conv2"):
        return "bn" + conv[-1]
    if re.search(r"\.conv\d$", conv):
        return conv[:-6] + ".bn" + conv[-1]
    return conv[:-1] + "1"          # "x.0" -> "x.1"


IDENTITY_VAR = np.float32(1 - 1e-5)


def wired_state_dict(c, nof_joints, seed=0):
    """the seeded random checkpoint with S isolated signal channels; the head is still the random one (``set_head``)"""
    sd = _synth().synth_state_dict(c, nof_joints, seed)

    def writer(conv, tap=None):
        w, bn = sd[conv + ".weight"], _bn_of(conv)
        w[:S] = 0
        sd[bn + ".bias"][:S] = 0
        sd[bn + ".running_mean"][:S] = 0
        if tap is not None:
            for s in range(S):
                w[(s, s) + tap] = 1.0
            sd[bn + ".weight"][:S] = 1.0
            sd[bn + ".running_var"][:S] = IDENTITY_VAR

    def reader(conv, own_rows):
        sd[conv + ".weight"][S if own_rows else 0:, :S] = 0     # (rows [:S] of an identity keep their tap)

    writer("conv1", (1, 1))
    reader("conv2", True)
    writer("conv2", (1, 1))
    for k in range(4):
        reader("layer1.%d.conv1" % k, False)
        writer("layer1.%d.conv3" % k)
    reader("layer1.0.downsample.0", True)
    writer("layer1.0.downsample.0", (0, 0))
    reader("transition1.0.0", True)
    writer("transition1.0.0", (1, 1))
    reader("transition1.1.0.0", False)
    for name, nbranch, nout in STAGES:
        for k in range(4):
            reader("%s.branches.0.%d.conv1" % (name, k), False)
            writer("%s.branches.0.%d.conv2" % (name, k))
        for j in range(1, nbranch):
            writer("%s.fuse_layers.0.%d.0" % (name, j))
        for i in range(1, nout):
            reader("%s.fuse_layers.%d.0.0.0" % (name, i), False)
    return sd


def set_head(sd, mix, bias):
    """final_layer reads the signals alone: weight[:, :S, 0, 0] = mix (J, S), bias (J,)"""
    w = sd["final_layer.weight"]
    w[:] = 0
    w[:, :S, 0, 0] = mix
    sd["final_layer.bias"][:] = bias
    return sd


def default_mix(nof_joints):
    """joint j reads plane j % 3 with +1 (j // 3 even) or -1 (odd); the last two joints sum two planes.  Every joint carries a
    design, so with J > 32 joints 0, 31, 32, 33 and the last one do: the group loop and its ``again`` barrier carry ties too."""
    mix = np.zeros((nof_joints, S), np.float32)
    for j in range(nof_joints):
        mix[j, j % S] = 1.0 if (j // S) % 2 == 0 else -1.0
    mix[nof_joints - 2] = (1, 1, 0)
    mix[nof_joints - 1] = (0, 1, 1)
    return mix


def default_bias(nof_joints, seed=0):
    """odd multiples of 0.5 in [-3.5, 3.5]: exact, and no cell of a map is ever zero (so 'bit for bit' has no signed zero in it)"""
    return (np.random.default_rng([seed, nof_joints]).integers(-4, 4, nof_joints) + 0.5).astype(np.float32)


def wired_crops(planes, h, w, seed=1):
    """``synth_crops`` with the designed planes (n, S, h/4, w/4) on the pixels the identity path reads"""
    planes = np.asarray(planes, np.float32)
    crops = _synth().synth_crops(len(planes), h, w, seed=seed)
    crops[:, :, ::4, ::4] = planes
    return crops


def closed_form(mix, bias, planes):
    """the heat-maps of the wired checkpoint: exact in float32 (small integers and half-integers)"""
    return (np.einsum("js,nsyx->njyx", np.asarray(mix, np.float32), np.asarray(planes, np.float32))
            + np.asarray(bias, np.float32)[None, :, None, None]).astype(np.float32)


def tie_counts(hm):
    """(n, J) number of cells equal to the map's maximum"""
    flat = hm.reshape(hm.shape[0], hm.shape[1], -1)
    return (flat == flat.max(-1, keepdims=True)).sum(-1)


# ------------------------------------------------------------------------------------------------------------ the kernels' walks
def head_form(dtype, switches=""):
    """which head kernel a handle runs (launch_head): 'mfma' for the 16-bit modes unless HRN_DISABLE_HEAD_MFMA is set, else 'valu'"""
    return "valu" if dtype == "fp32" or "HRN_DISABLE_HEAD_MFMA" in switches else "mfma"


def head_kernel_name(dtype, switches, nof_joints):
    base = "head_mfma" if head_form(dtype, switches) == "mfma" else "head"
    return "%s%s_kernel<%s>" % (base, "_groups" if nof_joints > 32 else "", dtype)


def plan_slab_px(hw, nb):
    """hrn_plan_head_slabs for a pass of nb crops: 1024-cell slabs when nb * ceil(hw / 1024) >= 192, else 256 (hrnet_mi355.cpp)"""
    return 1024 if nb * ((hw + 1023) // 1024) >= 192 else 256


def walk(px, slab_px, form):
    """(slab, wave, lane, trip) of cell(s) px; ``lane`` is the lane of the MFMA head and the thread of the VALU head"""
    px = np.asarray(px)
    r = px % slab_px
    if form == "mfma":
        per_wave = slab_px // 4
        return px // slab_px, r // per_wave, px % 16, (r % per_wave) // 16
    assert form == "valu", form
    t = r % 256
    return px // slab_px, t // 64, t, r // 256


def tie_class(p, q, hw, slab_px, form):
    """where cells p < q of a map of hw cells meet (see the module docstring): 'slab', 'wave', 'lane' or 'trip'"""
    assert 0 <= p < q < hw, (p, q, hw)
    (sp, wp, lp, tp), (sq, wq, lq, tq) = walk(p, slab_px, form), walk(q, slab_px, form)
    if sp != sq:
        return "slab"
    if wp != wq:
        return "wave"
    if lp != lq:
        return "lane"
    assert tp != tq
    return "trip"


def tie_level(p, q, hw, slab_px, form):
    """the first coordinate, in the order slab, wave, trip, lane, in which p < q differ: how far apart they sit.  A 'trip' pair of
    different lanes is decided by the butterfly (``tie_class`` says 'lane'); this key only sorts maps the trunk made by distance."""
    assert 0 <= p < q < hw, (p, q, hw)
    (sp, wp, lp, tp), (sq, wq, lq, tq) = walk(p, slab_px, form), walk(q, slab_px, form)
    return "slab" if sp != sq else "wave" if wp != wq else "trip" if tp != tq else "lane"


def reachable(hw, slab_px, form, key=tie_class):
    """the classes some pair of cells of the map falls into, by enumeration"""
    out = set()
    cells = np.arange(hw)
    sl, wv, ln, tr = walk(cells, slab_px, form)
    for p in range(hw - 1):
        q = cells[p + 1:]
        ds, dw, dl, dt = sl[q] != sl[p], wv[q] != wv[p], ln[q] != ln[p], tr[q] != tr[p]
        if key is tie_class:
            m = {"slab": ds, "wave": ~ds & dw, "lane": ~ds & ~dw & dl, "trip": ~ds & ~dw & ~dl}
        else:
            m = {"slab": ds, "wave": ~ds & dw, "trip": ~ds & ~dw & dt, "lane": ~ds & ~dw & ~dt}
        out |= {k for k, v in m.items() if v.any()}
        if len(out) == 4:
            break
    return out


# -- a numpy model of the two walks with a pluggable tie rule (the designs' teeth: tests/test_wired_host.py)
def _scan_right(v, bv, bi):
    return v > bv or bi == NO_IDX


def _merge_right(ov, oi, v, i):
    return ov > v or (ov == v and oi < i)


RULES = {
    "argmax.h": (_scan_right, _merge_right),
    # the three ways to resolve a tie by arrival order
    "incumbent": (_scan_right, lambda ov, oi, v, i: ov > v or (i == NO_IDX and oi != NO_IDX)),       # merges keep what they hold
    "challenger": (_scan_right, lambda ov, oi, v, i: oi != NO_IDX and (ov >= v or i == NO_IDX)),    # merges take what arrives
    "scan>=": (lambda v, bv, bi: v >= bv or bi == NO_IDX, _merge_right),                            # the scan takes the last maximum
}


def affected(rule, slab_px, form, classes):
    """the classes a wrong rule can change.  A merge whose incumbent always holds the lower cell is immune to 'incumbent': the slabs
    in decode_kernel, and the waves wherever a wave's cells all lie below the next wave's -- not so in the VALU form with trips."""
    if rule == "scan>=":
        hit = {"trip"}
    elif rule == "challenger":
        hit = {"lane", "wave", "slab"}
    else:
        hit = {"lane"} | ({"wave"} if form == "valu" and "trip" in classes else set())
    return hit & set(classes)


def model_argmax(plane, slab_px, form, rule="argmax.h"):
    """the cell the head + decode walk returns for one flat map under a tie rule: scan -> lanes -> waves -> slabs"""
    scan, merge = RULES[rule]
    plane = np.asarray(plane, np.float32).reshape(-1)
    hw = len(plane)
    lanes, steps = (16, (8, 4, 2, 1)) if form == "mfma" else (64, (32, 16, 8, 4, 2, 1))
    v, i = -np.inf, NO_IDX
    for slab in range((hw + slab_px - 1) // slab_px):
        red = []
        for wave in range(4):
            bv, bi = [-np.inf] * lanes, [NO_IDX] * lanes
            if form == "mfma":
                per_wave = slab_px // 4
                cells = [[slab * slab_px + wave * per_wave + it * 16 + li for it in range(per_wave // 16)] for li in range(16)]
            else:
                cells = [list(range(slab * slab_px + wave * 64 + li, (slab + 1) * slab_px, 256)) for li in range(64)]
            for li in range(lanes):
                for px in cells[li]:
                    if px < hw and scan(plane[px], bv[li], bi[li]):
                        bv[li], bi[li] = plane[px], px
            for off in steps:   # every lane exchanges with lane ^ off at once
                nv, ni = list(bv), list(bi)
                for li in range(lanes):
                    if merge(bv[li ^ off], bi[li ^ off], bv[li], bi[li]):
                        nv[li], ni[li] = bv[li ^ off], bi[li ^ off]
                bv, bi = nv, ni
            red.append((bv[0], bi[0]))
        sv, si = red[0]
        for w in range(1, 4):
            if merge(red[w][0], red[w][1], sv, si):
                sv, si = red[w]
        if merge(sv, si, v, i):
            v, i = sv, si
    return 0 if i == NO_IDX else int(i)


# ------------------------------------------------------------------------------------------------------------ designs
class Design:
    """one plane: ``plane`` (hw,) float32 of small non-negative integers, its arg-max ``cell``, the number ``ties`` of cells equal to
    the maximum, and for a twin the class ``cls`` in which its two maxima meet"""

    def __init__(self, name, plane, cell, cls=None):
        self.name, self.plane, self.cell, self.cls = name, np.asarray(plane, np.float32), int(cell), cls
        assert self.plane.min() >= 0 and self.plane.max() <= 7 and int(np.argmax(self.plane)) == self.cell, name
        self.ties = int((self.plane == self.plane.max()).sum())

    def __repr__(self):
        return "Design(%s, cell %d, %d ties%s)" % (self.name, self.cell, self.ties, ", " + self.cls if self.cls else "")


def _background(hw, tag):
    """integers 0..4, seeded; cell 1 is zero so that the -1 joints have a first zero to peak on (and cell 0 is not: the first zero
    is not the corner)"""
    bg = np.random.default_rng([hw, tag]).integers(0, 5, hw).astype(np.float32)
    bg[0], bg[1] = 2, 0
    return bg


def twin_pairs(hw, slab_px, form):
    """candidate (name, p, q) per class: an interior pair, a pair that straddles the unit boundary (q the first cell of its unit, p
    the last cell of the unit before), and pairs whose lower cell sits where an arrival-order rule would lose it"""
    per_wave = slab_px // 4 if form == "mfma" else 64
    lanes = 16 if form == "mfma" else 64
    step = 16 if form == "mfma" else 256                  # the distance between a lane's cells of consecutive trips
    trips = (slab_px // 4) // 16 if form == "mfma" else slab_px // 256
    nslab = (hw + slab_px - 1) // slab_px
    c = [("slab", 5, slab_px + 3), ("slab", slab_px - 1, slab_px), ("slab", (nslab - 1) * slab_px - 1, (nslab - 1) * slab_px),
         ("slab", 5, hw - 1),
         ("wave", 5, per_wave + 3), ("wave", per_wave - 1, per_wave), ("wave", 3 * per_wave - 1, 3 * per_wave),
         ("wave", 5, 3 * per_wave + 3),
         ("lane", 5, 9), ("lane", lanes - 1, lanes), ("lane", 0, 1), ("lane", 2, 3), ("lane", 6, lanes - 1),
         ("trip", 5, 5 + step), ("trip", lanes - 1, lanes - 1 + (trips - 1) * step), ("trip", 0, step)]
    if form == "valu":   # with trips a higher wave can hold the lower cell, and the last thread of a trip is followed by thread 0
        c += [("wave", 64 + 3, 256 + 5), ("wave", 255, 256), ("lane", 255, 256 + 192), ("lane", 9, 256 + 5)]
    else:
        c += [("lane", 9, 16 + 5), ("lane", 15, 16)]      # the lower cell in the higher lane, across trips
    out, seen = [], set()
    for cls, p, q in c:
        if 0 <= p < q < hw and (p, q) not in seen and tie_class(p, q, hw, slab_px, form) == cls:
            seen.add((p, q))
            out.append((cls, p, q))
    return out


def designs(h, w, slab_px, form):
    """every design family for a map of (h, w) cells walked in slabs of slab_px by the ``form`` head"""
    hw = h * w
    out = []
    for k, (cls, p, q) in enumerate(twin_pairs(hw, slab_px, form)):
        pl = _background(hw, k)
        pl[[p, q]] = 7
        out.append(Design("twin(%d,%d)" % (p, q), pl, p, cls))
    edge_cells = [0, hw - 1] + [x for k in range(1, (hw + slab_px - 1) // slab_px) for x in (k * slab_px - 1, k * slab_px)]
    for k, cell in enumerate(sorted(set(x for x in edge_cells if 0 <= x < hw))):
        pl = _background(hw, 100 + k)
        pl[cell] = 7
        out.append(Design("edge(%d)" % cell, pl, cell))
    out.append(Design("flat", np.full(hw, 3, np.float32), 0))
    p = min(hw - 2, max(1, (hw * 5) // 8 + 3))
    pl = _background(hw, 200)
    pl[p:] = 7
    out.append(Design("shelf(%d)" % p, pl, p))
    # the same maximum on the last cell of every wave's range and of every slab: the earliest wins
    pl = _background(hw, 201)
    per_wave = slab_px // 4 if form == "mfma" else 64
    ends = sorted(set([x for x in range(per_wave - 1, hw, per_wave)] + [hw - 1]))
    pl[ends] = 7
    out.append(Design("every-unit", pl, ends[0]))
    if h >= 12 and w >= 12:   # one 5x5 integer blob stamped twice in the interior (for the refined decodes): two equal peaks
        blob = np.asarray([[1, 2, 3, 2, 1], [2, 4, 5, 4, 2], [3, 5, 7, 6, 3], [2, 4, 5, 4, 2], [1, 2, 3, 2, 1]], np.float32)
        pl = np.zeros((h, w), np.float32)
        (y0, x0), (y1, x1) = (3, 4), (h - 4, w - 5)
        pl[y0 - 2:y0 + 3, x0 - 2:x0 + 3] = blob
        pl[y1 - 2:y1 + 3, x1 - 2:x1 + 3] = blob
        out.append(Design("blobs", pl.reshape(-1), y0 * w + x0))
    return out


def planes_for(ds, n, h, w, first=0):
    """(n, S, h, w) planes: plane s of crop i holds design (first + i * S + s) % len(ds); -> planes, the (n, S) design indices"""
    idx = (first + np.arange(n * S)) % len(ds)
    return np.stack([ds[k].plane for k in idx]).reshape(n, S, h, w), idx.reshape(n, S)


# ------------------------------------------------------------------------------------------------------------ zero-set heads
def zero_set_heads(x, nof_joints, seed=0, lo=0.02, hi=0.98, keep=2, stop=6):
    """channel sets for ``nof_joints`` heads from the tensor x (n, c, h, w) >= 0 the head reads.  Per joint: walk the channels whose
    zero fraction lies in (lo, hi) in a seeded order, add a channel while every crop keeps >= ``keep`` common zero cells, stop once no
    crop has more than ``stop``.  -> weight (J, c, 1, 1) of -1 / 0, zero-set masks (n, J, h*w) bool"""
    x = np.asarray(x)
    n, c = x.shape[:2]
    z = (x == 0).reshape(n, c, -1)
    frac = z.mean((0, 2))
    live = np.flatnonzero((frac > lo) & (frac < hi))
    rng = np.random.default_rng([seed, nof_joints, c])
    weight = np.zeros((nof_joints, c, 1, 1), np.float32)
    masks = np.ones((n, nof_joints, z.shape[2]), bool)
    for j in range(nof_joints):
        m = masks[:, j]
        for k in rng.permutation(live):
            m2 = m & z[:, k]
            if m2.sum(1).min() >= keep:
                m[:] = m2
                weight[j, k] = -1.0
            if m.sum(1).max() <= stop:
                break
    return weight, masks


def zero_set_state_dict(sd, weight, bias):
    sd = dict(sd)
    sd["final_layer.weight"] = np.ascontiguousarray(weight, np.float32)
    sd["final_layer.bias"] = np.ascontiguousarray(bias, np.float32)
    return sd


def tie_census(hm, slab_px, form, key=tie_class):
    """over the (crop, joint) maps of hm: the share with >= 2 equal maxima, and per class the number of maps in which the first
    maximum meets another one in that class"""
    n, J, h, w = hm.shape
    flat = hm.reshape(n * J, h * w)
    tied, per = 0, dict.fromkeys(CLASSES, 0)
    for m in flat:
        cells = np.flatnonzero(m == m.max())
        if len(cells) >= 2:
            tied += 1
            for k in {key(int(cells[0]), int(q), h * w, slab_px, form) for q in cells[1:]}:
                per[k] += 1
    return tied / float(n * J), per


# ------------------------------------------------------------------------------------------------------------ the GPU matrix
# (crop h, w, crops of the call): the smallest shapes at which each walk exists.  max_batch = n, so the call is one pass of n crops.
SHAPES = [(32, 32, 3),      # 8x8 map: one slab; only wave 0 holds cells (MFMA: in 4 trips)
          (64, 64, 3),      # 16x16: exactly one full 256-slab, four waves
          (64, 96, 3),      # 16x24: slabs of 256 and 128 cells; waves 2-3 of the second see no cell
          (64, 96, 192),    # one 1024-slab, more than half empty; trips in the VALU form
          (160, 128, 3),    # 40x32: five 256-slabs
          (160, 128, 96)]   # slabs of 1024 and 256 cells
# (dtype, environment switches) of the W32 table
HEADS = [("bf16", {}), ("fp16", {}), ("fp32", {}), ("bf16", {"HRN_DISABLE_HEAD_MFMA": "1"})]


def gpu_cases():
    """dicts: c, J, h, w, n, max_batch, dtype, env, boxes ('int' / 'float'); tests/test_argmax_gpu.py runs them, tests/test_wired_host.py
    checks that their designs cover every class each walk can reach"""
    out = []
    for h, w, n in SHAPES:
        for dtype, env in HEADS:
            out.append(dict(c=32, J=17, h=h, w=w, n=n, max_batch=n, dtype=dtype, env=env))
    for dtype in ("bf16", "fp32"):            # c = 48: the MFMA head's second K chunk is half padding
        out.append(dict(c=48, J=17, h=64, w=96, n=3, max_batch=3, dtype=dtype, env={}))
    for J in (33, 133):                       # the groups kernels
        for dtype in ("bf16", "fp32"):
            out.append(dict(c=32, J=J, h=64, w=96, n=3, max_batch=3, dtype=dtype, env={}))
    out.append(dict(c=32, J=17, h=64, w=96, n=5, max_batch=2, dtype="bf16", env={}))   # the designed crops land in different micro-batches
    for k, case in enumerate(out):
        case["boxes"] = "int" if k % 2 == 0 else "float"
    return out


def case_id(case):
    return "W%d-J%d-%dx%d-n%d-mb%d-%s%s-%s" % (case["c"], case["J"], case["h"], case["w"], case["n"], case["max_batch"], case["dtype"],
                                               "-valu" if case["env"] else "", case["boxes"])


def case_walk(case):
    """(form, slab_px) of the case's passes: every micro-batch of a case gets the same slab size"""
    hw = (case["h"] // 4) * (case["w"] // 4)
    sizes = {min(case["max_batch"], case["n"] - k) for k in range(0, case["n"], case["max_batch"])}
    px = {plan_slab_px(hw, nb) for nb in sizes}
    assert len(px) == 1, case
    return head_form(case["dtype"], ";".join(case["env"])), px.pop()


# ------------------------------------------------------------------------------------------------------------ score_heatmaps
def score_walk(px):
    """score_kernel (csrc/score.hip): a 256-thread block owns a map and reads it in float4 groups q = px // 4; thread = q % 256,
    wave = thread // 64, trip = q // 256, element = px % 4.  A thread scans its groups' cells in increasing order (``takes``), then
    ``block_argmax``: a 6-step butterfly per wave and the 4 waves in order (``better``).  -> (wave, thread, trip, element)"""
    q = np.asarray(px) // 4
    return (q % 256) // 64, q % 256, q // 256, np.asarray(px) % 4


def score_tie_class(p, q):
    """'cell' (two cells of one float4), 'trip' (one thread, two trips), 'thread' (one wave: the butterfly) or 'wave'"""
    (wp, tp, rp, _), (wq, tq, rq, _) = score_walk(p), score_walk(q)
    if wp != wq:
        return "wave"
    if tp != tq:
        return "thread"
    return "trip" if rp != rq else "cell"


class ScoreDesign(Design):
    def __init__(self, name, plane, cell, cls=None):
        self.name, self.plane, self.cell, self.cls = name, np.asarray(plane, np.float32), int(cell), cls
        assert self.plane.min() > 0 and int(np.argmax(self.plane)) == self.cell, name
        self.ties = int((self.plane == self.plane.max()).sum())


def score_designs(h, w):
    """positive maps (get_max_preds zeroes a joint whose maximum is not > 0) of the families twin, flat, shelf and every-unit"""
    hw = h * w
    pairs = [(4, 7), (5, 6), (3, 4), (0, 1), (8, 16), (255, 256), (5, 259), (1023, 1024), (1020 + 3, 2048 + 1), (5, 1029), (1027, 2051),
             (260, 1024 + 5), (hw - 2, hw - 1), (0, hw - 1)]
    out = []
    for k, (p, q) in enumerate(pairs):
        if 0 <= p < q < hw:
            pl = _background(hw, 300 + k) + 1
            pl[[p, q]] = 8
            out.append(ScoreDesign("twin(%d,%d)" % (p, q), pl, p, score_tie_class(p, q)))
    out.append(ScoreDesign("flat", np.full(hw, 3, np.float32), 0))
    p = (hw * 5) // 8 + 3
    pl = _background(hw, 400) + 1
    pl[p:] = 8
    out.append(ScoreDesign("shelf(%d)" % p, pl, p))
    pl = _background(hw, 401) + 1
    ends = sorted(set(list(range(255, hw, 256)) + [hw - 1]))     # the last cell of every wave's share of a trip
    pl[ends] = 8
    out.append(ScoreDesign("every-unit", pl, ends[0]))
    return out
