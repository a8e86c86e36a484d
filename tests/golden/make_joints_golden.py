#!/usr/bin/env python3
"""Golden vectors for heads with more than 32 joints (whole-body 133, face 68, the first count past one joint group: 33),
produced by RUNNING THE UNMODIFIED REFERENCE in the build container -- ``models_.hrnet.HRNet(c, J)`` plus the reference's decode
(SimpleHRNet.py:297-308), ``flip_back`` / ``get_final_preds`` (misc/utils.py) for the flip-TTA fixture, and
``_generate_target`` / the losses / ``evaluate_pck_accuracy`` for the score fixture.  Built like make_golden.py and
make_score_golden.py, whose stand-ins and helpers it imports (it edits neither).

    python tests/golden/make_joints_golden.py            ->  tests/golden/j*.npz

Weights, crops and boxes are not stored where a seed regenerates them: ``synth_state_dict(c, J, seed)``,
``synth_crops(n, h, w, seed=11)`` (13 for flip-TTA), ``synth_boxes(n, seed=5)``.

The fp32 engine is held to heat-maps within HM_ATOL_F32 = 2e-4 and IDENTICAL coordinates.  Coordinates can only be demanded
where the reference's own decision is not inside that noise, and 133 near-flat random-init maps do come closer than that on
some seeds.  So the generator ASSERTS, for every (crop, joint) it stores -- none excluded -- that the top-1 minus top-2 gap of
the map exceeds 2 * HM_ATOL_F32 = 4e-4; the (c, J, h, w, n, weight seed) below were picked so that it holds.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG          # noqa: E402  (stand-ins, ref_decode, save; puts the reference and the repository on sys.path)
import make_score_golden as MS    # noqa: E402  (stand-ins of the dataset imports, make_joints)

synth = MG.synth
HM_ATOL_F32 = 2e-4
MIN_GAP = 2 * HM_ATOL_F32

# (name, c, J, h, w, n, weight seed)
HEATMAP_CASES = [("j133_w32_64x64_n2", 32, 133, 64, 64, 2, 9),
                 ("j133_w48_128x96_n2", 48, 133, 128, 96, 2, 0),
                 ("j68_w32_64x96_n3", 32, 68, 64, 96, 3, 5),
                 ("j33_w48_64x64_n2", 48, 33, 64, 64, 2, 1)]
TTA_CASE = ("j133_w32_128x96_fliptta_n3", 32, 133, 128, 96, 3)
TTA_WEIGHT_SEEDS = (36,)            # the first of 0, 1, ... whose averaged maps meet the gap assertion (0 .. 35: 2e-6 .. 3.4e-4)
TTA_PAIR_SEED = 7
SCORE_J, SCORE_N, SCORE_HW, SCORE_SIGMA = 133, 3, (32, 24), 2
SCORE_TOPK = (8, 40)                # the second crosses 32 joints
THR = 0.5


def min_gap(maps):
    """smallest top-1 minus top-2 gap over all (crop, joint) maps"""
    flat = np.sort(maps.reshape(maps.shape[0], maps.shape[1], -1), -1)
    return float((flat[..., -1] - flat[..., -2]).min())


def ref_model(c, J, seed):
    from models_.hrnet import HRNet

    m = HRNet(c, J).eval()
    m.load_state_dict(synth.to_torch_state_dict(synth.synth_state_dict(c, J, seed)))
    return m


def heatmap_case(name, c, J, h, w, n, seed):
    m = ref_model(c, J, seed)
    x = synth.synth_crops(n, h, w, seed=11)
    with torch.no_grad():
        y = m(torch.from_numpy(x)).numpy()
    gap = min_gap(y)
    assert gap > MIN_GAP, "%s: top-1/top-2 gap %.3g does not exceed %.3g: pick another weight seed" % (name, gap, MIN_GAP)
    boxes = synth.synth_boxes(n, seed=5)
    print("%s: min gap %.3g, heat-map sigma %.3g" % (name, gap, y.std()))
    MG.save(name, c=c, J=J, n=n, h=h, w=w, weight_seed=seed, crop_seed=11, box_seed=5, heatmaps=y, boxes=boxes,
            pts=MG.ref_decode(y, boxes, h // 4, w // 4), min_gap=np.float64(gap))


def seeded_pairs(J, seed, paired=120):
    """disjoint flip pairs over `paired` of the J joints, the rest unpaired"""
    perm = np.random.default_rng(seed).permutation(J)[:paired]
    return np.sort(perm.reshape(-1, 2), 1).astype(np.int32)


def flip_tta_case(name, c, J, h, w, n):
    """as make_golden.flip_tta_case, at J joints with a seeded pair table; the heat-maps go into two files (crops [0, 2) and
    [2, n)) so that each stays below the size of the largest fixture"""
    if "munkres" not in sys.modules:
        sys.modules["munkres"] = types.ModuleType("munkres")
    import misc.utils as U

    pairs = seeded_pairs(J, TTA_PAIR_SEED)
    assert len(np.unique(pairs)) == pairs.size == 120
    x = torch.from_numpy(synth.synth_crops(n, h, w, seed=13))
    for seed in TTA_WEIGHT_SEEDS:
        m = ref_model(c, J, seed)
        with torch.no_grad():
            out = m(x)
            out_f = U.flip_back(m(U.flip_tensor(x, dim=-1)), pairs.tolist())
            avg = (out + out_f) * 0.5
        gap = min_gap(avg.numpy())
        print("%s: weight seed %d: min gap of the averaged maps %.3g" % (name, seed, gap))
        if gap > MIN_GAP:
            break
    else:
        raise AssertionError("no weight seed meets the gap assertion")
    U.transform_preds = lambda coords, center, scale, pixel_std, output_size: coords
    none = [None] * n
    preds, maxvals = U.get_final_preds(True, avg.clone(), none, none, 200)
    preds_raw, _ = U.get_final_preds(False, avg.clone(), none, none, 200)
    avg = avg.numpy()
    MG.save(name, c=c, J=J, n=n, h=h, w=w, weight_seed=seed, crop_seed=13, heatmaps=avg[:2], preds=preds.numpy(),
            preds_nopost=preds_raw.numpy(), maxvals=maxvals.numpy(), flip_pairs=pairs, min_gap=np.float64(gap))
    MG.save(name + "_b", heatmaps=avg[2:])


def score_case(name):
    """one batch at J = 133 with the quantities and the planted joints of make_score_golden.py (off the map, the br < 0 quirk),
    NaN maps, and the OHKM loss at two topk"""
    MS.install_stubs()
    from datasets.COCO import COCODataset
    from losses import loss as LOSS
    from misc import utils as U

    J, n, (h, w), sigma = SCORE_J, SCORE_N, SCORE_HW, SCORE_SIGMA
    rng = np.random.default_rng(33)
    H, W, t = 4 * h, 4 * w, 3 * sigma
    joints, vis = MS.make_joints(rng, n, J, H, W, t)
    jw = (1 + rng.integers(0, 3, J) * 0.25).astype(np.float32).reshape(J, 1)
    ds = types.SimpleNamespace(nof_joints=J, heatmap_type="gaussian", heatmap_size=(w, h), heatmap_sigma=sigma, image_size=(W, H),
                               use_different_joints_weight=True, joints_weight=jw)
    tgt, tw = zip(*[COCODataset._generate_target(ds, joints[i].copy(), vis[i].copy()) for i in range(n)])
    target, target_weight = np.stack(tgt), np.stack(tw)
    mu = np.trunc(joints / 4.0 + 0.5).astype(np.int64)
    weighted = target_weight[:, :, 0] > 0
    empty = target.reshape(n, J, -1).max(-1) == 0
    quirk = weighted & empty
    assert (quirk & (mu[..., 0] == -(t + 1))).any() and (quirk & (mu[..., 1] == -(t + 1))).any(), "the br < 0 quirk does not occur"
    assert ((vis[:, :, 0] > 0) & ~weighted).any(), "no visible joint wholly off the map"
    output = np.empty_like(target)
    for i in range(n):
        for j in range(J):
            dy, dx = rng.integers(-5, 6, 2)
            output[i, j] = np.roll(target[i, j], (dy, dx), (0, 1)) * np.float32(rng.choice([0.5, 0.75, 1.0, 1.25]))
    output += (rng.integers(-2, 3, output.shape) / 16.0).astype(np.float32) * (rng.uniform(0, 1, output.shape) < 0.3)
    out = {}
    for tag, special in (("plain", False), ("nan", True)):
        o_np = output.copy()
        if special:                      # NaN maps on both sides of joint 32 of person 0; persons 1 .. stay finite
            o_np[0, 0, 3, 5] = np.nan
            o_np[0, 40, 7, 2] = np.nan
            o_np[0, 40, 9, 4] = np.nan   # the first NaN wins
            o_np[0, 100, :, :] = -np.inf
            o_np[1, 3, 0, 0] = np.inf
        o, tg, twt = torch.from_numpy(o_np), torch.from_numpy(target), torch.from_numpy(target_weight)
        mse = LOSS.JointsMSELoss(use_target_weight=True)
        loss32, loss64 = mse(o, tg, twt), mse(o.double(), tg.double(), twt.double())
        assert np.isnan(float(loss64)) == special
        for topk in SCORE_TOPK:
            mats = []
            oh = LOSS.JointsOHKMMSELoss(use_target_weight=True, topk=topk)
            oh.ohkm = lambda loss, k: (mats.append(loss), LOSS.ohkm(loss, k))[1]
            out["%s_ohkm64_top%d" % (tag, topk)] = np.float64(float(oh(o.double(), tg.double(), twt.double())))
            out["%s_ohkm32_top%d" % (tag, topk)] = np.float32(float(oh(o, tg, twt)))
        acc, avg_acc, cnt, pred, tpred = U.evaluate_pck_accuracy(o, tg, thr=THR)
        norm = torch.ones((n, 2)) * torch.tensor([h, w], dtype=torch.float32) / 10
        dists = U.calc_dists(pred, tpred, norm)
        dv = dists[dists != -1].numpy()
        assert not (np.abs(dv - THR) < 1e-4).any(), "a distance within 1e-4 of the threshold: reseed"
        for key, v in (("output", o_np), ("loss32", np.float32(float(loss32))), ("loss64", np.float64(float(loss64))),
                       ("map_loss64", mats[0].numpy()), ("acc", acc.numpy()), ("avg_acc", np.float32(float(avg_acc))),
                       ("cnt", np.int32(cnt)), ("pred", pred.numpy()), ("target_pred", tpred.numpy()), ("dists", dists.numpy())):
            out["%s_%s" % (tag, key)] = v
        print("score %s: loss %.6g ohkm(8) %.6g ohkm(40) %.6g avg_acc %.4f cnt %d" %
              (tag, float(loss64), out[tag + "_ohkm64_top8"], out[tag + "_ohkm64_top40"], float(avg_acc), cnt))
    # the NaN variant differs from the plain one in five maps only: store those, not the whole tensor twice
    diff = np.argwhere((out["nan_output"].view(np.int32) != out["plain_output"].view(np.int32)).reshape(n, J, -1).any(-1))
    out["nan_maps_index"] = diff.astype(np.int32)
    out["nan_maps"] = np.stack([out["nan_output"][i, j] for i, j in diff])
    del out["nan_output"]
    out.update(joints=joints, vis=vis[:, :, 0].copy(), joints_weight=jw.reshape(-1), sigma=np.int32(sigma), target_weight=target_weight,
               thr=np.float32(THR), topk=np.asarray(SCORE_TOPK, np.int32), h=np.int32(h), w=np.int32(w), J=np.int32(J), n=np.int32(n))
    out["target"] = target           # (mostly zeros: it compresses to a few per cent)
    MG.save(name, **out)


def main():
    torch.set_num_threads(os.cpu_count())
    MG.install_stubs()
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("all", "heatmaps"):
        for case in HEATMAP_CASES:
            heatmap_case(*case)
    if which in ("all", "fliptta"):
        flip_tta_case(*TTA_CASE)
    if which in ("all", "score"):
        score_case("j133_score_case")


if __name__ == "__main__":
    main()
