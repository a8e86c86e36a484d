"""Golden vectors for the scoring of an evaluation batch (testing/Test.py:141-157): Gaussian targets, loss and PCK, produced by
CALLING THE UNMODIFIED REFERENCE FUNCTIONS in the build container --
``COCODataset._generate_target`` (datasets/COCO.py:460-515) on a plain namespace carrying the seven attributes it reads,
``JointsMSELoss`` (losses/loss.py:20-54) in float32 and on ``.double()`` inputs, ``JointsOHKMMSELoss.forward`` (:73-92) with the
module-level ``ohkm`` it means bound to the instance (its ``self.ohkm`` does not exist; the binding also records the (n, J) loss
matrix the forward builds), ``evaluate_pck_accuracy`` and ``calc_dists`` (misc/utils.py:185-244).
Stand-ins only for imports that are absent here and are not the code under test (cv2, munkres, json_tricks, pycocotools,
torchvision, tqdm, the compiled nms extensions).

The generator asserts, ON THE REFERENCE ALONE: every kind of joint occurs (windows cut by each edge, wholly off the map, the
``br < 0`` quirk on both axes: weight kept, nothing drawn), no distance lies within 1e-4 of the threshold (so that tests can
demand equal accuracies), and it measures how far the reference's float32 ``exp`` is from ``float32(exp(float64))`` on this
numpy build (``g_ulps``: the tests allow that + 1).

    python tests/golden/make_score_golden.py      ->  tests/golden/score_cases.npz
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
THR, TOPK = 0.5, 8
# (heat-map h, w, sigma, J, n, joints_weight, all invisible, NaN / -inf cells, seed)
CASES = [(64, 48, 2, 17, 4, False, False, False, 11),
         (96, 72, 3, 17, 3, True, False, False, 12),
         (16, 16, 2, 16, 8, False, False, False, 13),
         (64, 48, 3, 16, 3, False, False, False, 14),
         (96, 72, 2, 17, 2, False, True, False, 15),
         (64, 48, 2, 17, 2, False, False, True, 16)]


def install_stubs():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    absent = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("not under test"))  # noqa: E731
    module("cv2")
    module("munkres", Munkres=absent)
    module("json_tricks")
    module("pycocotools")
    module("pycocotools.coco", COCO=absent)
    module("pycocotools.cocoeval", COCOeval=absent)
    module("tqdm", tqdm=absent)
    module("cpu_nms", cpu_nms=absent)
    module("gpu_nms", gpu_nms=absent)
    try:
        import torchvision  # noqa: F401
    except Exception:  # noqa: BLE001
        module("torchvision", transforms=module("torchvision.transforms", Compose=absent, ToTensor=absent, Normalize=absent))


def make_joints(rng, n, J, H, W, t):
    """joints in crop pixels from [-40, W + 40) x [-40, H + 40), visibility 0 for about a fifth; the first joints of persons 0
    and 1 are planted: the quirk on x and on y (mu = -(t + 1)), a window cut by each edge, one wholly off the map"""
    joints = np.stack([rng.uniform(-40, W + 40, (n, J)), rng.uniform(-40, H + 40, (n, J))], -1)
    vis = (rng.uniform(0, 1, (n, J)) > 0.2).astype(np.float32)
    cell = lambda mu: 4.0 * mu + (0.7 if mu >= 0 else -3.3)              # noqa: E731  (int(cell(mu) / 4 + 0.5) == mu: int() truncates)
    planted = [(cell(-(t + 1)), H / 2), (W / 2, cell(-(t + 1))),         # the quirk: mu = -(t + 1)
               (cell(1), H / 2), (cell(W // 4 - 2), H / 3), (W / 2, cell(1)), (W / 3, cell(H // 4 - 2)),
               (cell(-(t + 3)), H / 2), (cell(W // 4 + t + 2), H / 2), (cell(W // 8), cell(H // 8))]   # ..., off the map twice, the map's centre
    for k, (x, y) in enumerate(planted):
        i, j = k % min(n, 2), k // min(n, 2)
        joints[i, j] = (x, y)
        vis[i, j] = 1
    return joints, np.stack([vis, vis], -1)


def main():
    install_stubs()
    sys.path.insert(0, REF)
    import torch
    from datasets.COCO import COCODataset
    from losses import loss as LOSS
    from misc import utils as U

    out, g_ulps = {}, 0
    for k, (h, w, sigma, J, n, use_jw, invisible, special, seed) in enumerate(CASES):
        rng = np.random.default_rng(seed)
        H, W, t = 4 * h, 4 * w, 3 * sigma
        joints, vis = make_joints(rng, n, J, H, W, t)
        if invisible:
            vis[:] = 0
        jw = (1 + rng.integers(0, 3, J) * 0.25).astype(np.float32).reshape(J, 1)
        ds = types.SimpleNamespace(nof_joints=J, heatmap_type="gaussian", heatmap_size=(w, h), heatmap_sigma=sigma, image_size=(W, H),
                                   use_different_joints_weight=use_jw, joints_weight=jw)
        tgt, tw = zip(*[COCODataset._generate_target(ds, joints[i].copy(), vis[i].copy()) for i in range(n)])
        target, target_weight = np.stack(tgt), np.stack(tw)                  # (n,J,h,w) float32, (n,J,1) float32
        assert target.dtype == np.float32 and target_weight.dtype == np.float32
        # ---- what occurs (asserted on the reference's outputs)
        mu = np.trunc(joints / 4.0 + 0.5).astype(np.int64)
        weighted = target_weight[:, :, 0] > 0
        empty = target.reshape(n, J, -1).max(-1) == 0
        if not invisible:
            quirk = weighted & empty
            assert (quirk & (mu[..., 0] == -(t + 1))).any() and (quirk & (mu[..., 1] == -(t + 1))).any(), "the br < 0 quirk does not occur"
            drawn = weighted & ~empty
            assert (drawn & (mu[..., 0] < t)).any() and (drawn & (mu[..., 0] >= w - t)).any(), "no window cut left / right"
            assert (drawn & (mu[..., 1] < t)).any() and (drawn & (mu[..., 1] >= h - t)).any(), "no window cut top / bottom"
            assert ((vis[:, :, 0] > 0) & ~weighted).any(), "no visible joint wholly off the map"
            # ---- the reference's exp against float32(exp(float64)): a window wholly inside shows the whole table
            inside = drawn & (mu[..., 0] >= t) & (mu[..., 0] < w - t) & (mu[..., 1] >= t) & (mu[..., 1] < h - t)
            assert inside.any()
            i, j = np.argwhere(inside)[0]
            win = target[i, j, mu[i, j, 1] - t:mu[i, j, 1] + t + 1, mu[i, j, 0] - t:mu[i, j, 0] + t + 1]
            d = np.arange(-t, t + 1, dtype=np.float64)
            exact = np.exp(-(d[None] ** 2 + d[:, None] ** 2) / (2.0 * sigma ** 2)).astype(np.float32)
            ulps = np.abs(win.view(np.int32).astype(np.int64) - exact.view(np.int32).astype(np.int64))
            g_ulps = max(g_ulps, int(ulps.max()))
            out["case%d_g" % k] = win.copy()                                   # the reference's (2t+1) x (2t+1) Gaussian
        else:
            assert not weighted.any() and empty.all()
        # ---- outputs: the targets rolled by a few cells, scaled, plus coarse noise (multiples of 1/16)
        output = np.empty_like(target)
        for i in range(n):
            for j in range(J):
                dy, dx = rng.integers(-5, 6, 2)
                output[i, j] = np.roll(target[i, j], (dy, dx), (0, 1)) * np.float32(rng.choice([0.5, 0.75, 1.0, 1.25]))
        output += (rng.integers(-2, 3, output.shape) / 16.0).astype(np.float32) * (rng.uniform(0, 1, output.shape) < 0.3)
        if special:
            output[0, 0, 3, 5] = np.nan                    # a NaN is a maximum: (5, 3) is reported as non-positive -> (0, 0)
            output[0, 1, 7, 2] = np.nan
            output[0, 1, 9, 4] = np.nan                    # the first NaN wins
            output[0, 2, :, :] = -np.inf                   # a map of -inf everywhere decodes to index 0
            output[1, 0, 10, 10] = -np.inf
            output[1, 3, 0, 0] = np.inf
        o, tg, twt = torch.from_numpy(output), torch.from_numpy(target), torch.from_numpy(target_weight)
        mse = LOSS.JointsMSELoss(use_target_weight=True)
        loss32 = mse(o, tg, twt)
        loss64 = mse(o.double(), tg.double(), twt.double())
        mats = []
        oh = LOSS.JointsOHKMMSELoss(use_target_weight=True, topk=TOPK)
        oh.ohkm = lambda loss, topk: (mats.append(loss), LOSS.ohkm(loss, topk))[1]
        ohkm64 = oh(o.double(), tg.double(), twt.double())
        ohkm32 = oh(o, tg, twt)
        acc, avg_acc, cnt, pred, tpred = U.evaluate_pck_accuracy(o, tg, thr=THR)
        norm = torch.ones((n, 2)) * torch.tensor([h, w], dtype=torch.float32) / 10
        dists = U.calc_dists(pred, tpred, norm)
        dv = dists[dists != -1].numpy()
        assert not special or (np.isnan(float(loss64)) and np.isnan(float(loss32)))
        assert special or np.isfinite(float(loss64))
        assert not (np.abs(dv - THR) < 1e-4).any(), "a distance within 1e-4 of the threshold: reseed case %d" % k
        if invisible:
            assert (acc.numpy() == -1).all() and float(avg_acc) == 0 and cnt == 0
        for name, v in (("joints", joints), ("vis", vis[:, :, 0].copy()), ("joints_weight", jw.reshape(-1)), ("use_jw", np.int32(use_jw)),
                        ("sigma", np.int32(sigma)), ("target", target), ("target_weight", target_weight), ("output", output),
                        ("loss32", np.float32(float(loss32))), ("loss32_bits", loss32.detach().numpy().astype(np.float32)),
                        ("loss64", np.float64(float(loss64))),
                        ("ohkm64", np.float64(float(ohkm64))), ("ohkm32", np.float32(float(ohkm32))), ("map_loss64", mats[0].numpy()),
                        ("acc", acc.numpy()), ("avg_acc", np.float32(float(avg_acc))), ("cnt", np.int32(cnt)), ("pred", pred.numpy()),
                        ("target_pred", tpred.numpy()), ("dists", dists.numpy())):
            out["case%d_%s" % (k, name)] = v
        print("case %d: %dx%d sigma %d J %d n %d: loss %.6g ohkm %.6g avg_acc %.4f cnt %d, nearest |d - thr| %.3g"
              % (k, h, w, sigma, J, n, float(loss64), float(ohkm64), float(avg_acc), cnt, np.abs(dv - THR).min() if dv.size else np.nan))
    out.update(ncases=np.int32(len(CASES)), thr=np.float32(THR), topk=np.int32(TOPK), g_ulps=np.int32(g_ulps),
               numpy_version=np.array(np.__version__), torch_version=np.array(torch.__version__))
    path = os.path.join(HERE, "score_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f KB); the reference's exp is within %d ulp of float32(exp(float64)) here" % (path, os.path.getsize(path) / 1024, g_ulps))


if __name__ == "__main__":
    main()
