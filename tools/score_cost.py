"""Cost of scoring an evaluation batch on the GPU (NativeHRNet.score_heatmaps = hrn_score_heatmaps) against yardsticks that are not
the code under test, at the headline shape (256 crops of 384x288: 17 heat-maps of 96x72 each) and at 16 crops, interleaved
(round r runs the candidates in a rotated order) and timed with HIP events, per CALL as a user issues it:
  * score_heatmaps in analytic mode (joints + visibility; the targets exist only inside the kernel) and in maps mode;
  * yardstick 1: the floor of reading the output maps once (twice the bytes in maps mode) at 6.15 TB/s, the achievable HBM rate
    the project uses elsewhere (profiles/warp_prepath.txt).  120 MB of maps fit in the 256 MiB Infinity Cache, so the candidates
    walk over --buffers distinct batches (3 x 120 MB by default) and every call reads maps that have left the cache;
  * yardstick 2: the same quantities by torch operations on the same device tensors with the targets already resident --
    JointsMSELoss as the reference composes it (a Python loop over the joints: 17 MSELoss calls), get_max_preds with torch.max
    on both tensors, the distances and accuracies vectorised (not the reference's Python double loop, which would flatter the
    kernel) -- and what the analytic mode removes: building the 256 targets in numpy on the host and copying them in;
  * the share of a 256-crop predict_eval pass (W48, bf16, flip-TTA) the score adds.
usage: python tools/score_cost.py [--rounds R] [--reps K] [--buffers B] [--skip-network]   -> one JSON line"""
import argparse, importlib, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

pkg = importlib.import_module("simple-hrnet_amd")
import costlib
import score_ref as R   # the numpy restatement: the host-side target builder of yardstick 2

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=10, help="calls per timed sample")
ap.add_argument("--buffers", type=int, default=3, help="distinct heat-map batches the candidates rotate over")
ap.add_argument("--skip-network", action="store_true", help="leave out the predict_eval share (no W48 engine is built)")
args = ap.parse_args()
H, W, J, many, few, sigma = 384, 288, 17, 256, 16, 3
h, w = H // 4, W // 4
rng = np.random.default_rng(5)
joints = np.stack([rng.uniform(-20, W + 20, (many, J)), rng.uniform(-20, H + 20, (many, J))], -1)
vis = (rng.uniform(0, 1, (many, J)) > 0.2).astype(np.float32)
net = pkg.NativeHRNet(32, J, (H, W), "bf16", max_batch=32, device=0)          # scoring needs no weights
targets, tw = net.generate_targets(joints, vis, sigma=sigma)
tw_dev = torch.from_numpy(tw).cuda()
outs = [(targets.roll((k + 1, -k), (2, 3)) * 0.8 + 0.05 * torch.randn_like(targets)).contiguous() for k in range(args.buffers)]
turn = {"i": 0}


def nxt():
    turn["i"] += 1
    return outs[turn["i"] % len(outs)]


def torch_score(o, t, twd, thr=0.5):
    """yardstick 2 (not the code under test): the reference's quantities from resident tensors, by torch operations"""
    n = o.shape[0]
    crit = torch.nn.MSELoss(reduction="mean")
    op, tp = o.reshape(n, J, -1), t.reshape(n, J, -1)
    loss = 0
    for j in range(J):                                  # JointsMSELoss.forward composes it this way
        loss = loss + 0.5 * crit(op[:, j] * twd[:, j], tp[:, j] * twd[:, j])
    loss = loss / J

    def max_preds(x):
        mv, idx = torch.max(x, dim=2)
        p = torch.stack([(idx % w).float(), torch.floor(idx.float() / w)], -1)
        return p * (mv > 0).unsqueeze(-1).float()
    pred, tgt = max_preds(op), max_preds(tp)
    norm = torch.tensor([h, w], dtype=torch.float32, device=o.device) / 10
    d = torch.linalg.vector_norm(pred / norm - tgt / norm, dim=-1)
    ok = (tgt[..., 0] > 1) & (tgt[..., 1] > 1)
    below, valid = ((d < thr) & ok).sum(0).float(), ok.sum(0).float()
    acc = torch.where(valid > 0, below / valid.clamp(min=1), torch.full_like(valid, -1))
    good = acc >= 0
    return loss, acc, torch.where(good, acc, torch.zeros_like(acc)).sum() / good.sum().clamp(min=1), good.sum()


def numpy_targets_and_upload(k):
    t, _ = R.generate_targets(joints[:k], vis[:k], (h, w), sigma)
    return torch.from_numpy(t).cuda()


cands = {}
for k, tag in ((many, "256"), (few, "16")):
    cands["score_analytic_" + tag] = (k, 1, lambda k=k: net.score_heatmaps(nxt()[:k], joints=joints[:k], visibility=vis[:k], sigma=sigma, topk=8))
    cands["score_maps_" + tag] = (k, 2, lambda k=k: net.score_heatmaps(nxt()[:k], targets=targets[:k], target_weight=tw[:k], topk=8))
    cands["torch_ops_resident_targets_" + tag] = (k, 2, lambda k=k: torch_score(nxt()[:k], targets[:k], tw_dev[:k]))
names = list(cands)
samples = costlib.timed({k: fn for k, (_, _, fn) in cands.items()}, args.rounds, args.reps)   # (warm-up: staging ring, the table, blocks, clocks)
med = {k: statistics.median(v) for k, v in samples.items()}
floor_ms = {k: cands[k][0] * cands[k][1] * J * h * w * 4 / 6.15e12 * 1e3 for k in names if k.startswith("score")}
host = {}
for k, tag in ((many, "256"), (few, "16")):   # what the analytic mode removes: numpy targets on the host + the copy (host clock, synchronised)
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        numpy_targets_and_upload(k)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    host["numpy_targets_and_upload_" + tag] = round(statistics.median(ts), 3)
net.close()
result = {"workload": "%d / %d crops of %dx%d: %d heat-maps of %dx%d each, sigma %d; %d rotating batches" % (many, few, H, W, J, h, w, sigma, len(outs)),
          "device": torch.cuda.get_device_name(0),
          "ms_per_call": {k: round(v, 4) for k, v in med.items()},
          "read_floor_ms": {k: round(v, 4) for k, v in floor_ms.items()},
          "time_over_read_floor": {k: round(med[k] / floor_ms[k], 2) for k in floor_ms},
          "torch_over_score": {t: round(med["torch_ops_resident_targets_" + t] / med["score_maps_" + t], 2) for t in ("256", "16")},
          "host_ms": host,
          "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in samples.items()}}
if not args.skip_network:    # the share of a whole predict_eval pass at the headline shape
    big = pkg.NativeHRNet(48, J, (H, W), "bf16", max_batch=many, device=0).load_state_dict(pkg.synth_state_dict(48, J, 0))
    frame = torch.from_numpy(rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)).cuda()
    boxes = np.stack([rng.uniform(0, 1500, many), rng.uniform(0, 400, many), rng.uniform(150, 400, many), rng.uniform(300, 650, many)], 1)
    cs = [pkg.postproc.box_to_center_scale(b, W / H) for b in boxes]
    centers, scales = np.stack([c for c, _ in cs]), np.stack([s for _, s in cs])
    mats = np.stack([pkg.postproc.affine_matrix(centers[i], scales[i], 200, 0, (W, H)) for i in range(many)])
    pairs = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
    t_pass, t_score = [], []
    for r in range(4):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        images = big.warp_crops(frame, matrices=mats)
        hm, preds, maxvals = big.predict_flip_tta(images, pairs)
        ev[1].record()
        big.score_heatmaps(hm, joints=joints, visibility=vis, sigma=sigma, topk=8)
        ev[2].record()
        ev[2].synchronize()
        if r:                                           # the first round warms up
            t_pass.append(ev[0].elapsed_time(ev[1])), t_score.append(ev[1].elapsed_time(ev[2]))
    big.close()
    result["predict_eval_256"] = {"warp_plus_flip_tta_ms": round(statistics.median(t_pass), 3), "score_ms": round(statistics.median(t_score), 4),
                                  "score_share": round(statistics.median(t_score) / statistics.median(t_pass), 5)}
print(json.dumps(result))
