"""numpy restatement of the scoring contract (include/hrnet_mi355.h: hrn_target_centers, hrn_generate_targets,
hrn_score_heatmaps): Gaussian targets with the library's table, the losses in float64, the PCK in float32.

Imported by tests/test_score_host.py (the restatement against the reference's fixture, on the CPU) and
tests/test_score_gpu.py (the kernels against it)."""
import numpy as np

F32 = np.float32


def table(sigma):
    """g[d2] = float32(exp(-float64(d2) / (2 sigma^2))), d2 = 0 .. 2 t^2, t = 3 sigma"""
    t = int(3 * sigma)
    return np.exp(-np.arange(2 * t * t + 1, dtype=np.float64) / (2.0 * float(sigma) ** 2)).astype(F32)


def target_centers(joints, vis, hw, sigma, joints_weight=None):
    """-> mu (n,J,2) int64 (x, y), weight (n,J) float32 before joints_weight, target_weight (n,J) float32, drawn (n,J) bool"""
    h, w = hw
    t = int(3 * sigma)
    joints, vis = np.asarray(joints, np.float64), np.asarray(vis, F32)
    mu = np.trunc(joints / 4.0 + 0.5).astype(np.int64)            # int(): towards zero
    off = (mu[..., 0] - t >= w) | (mu[..., 1] - t >= h) | (mu[..., 0] + t + 1 < 0) | (mu[..., 1] + t + 1 < 0)
    weight = np.where(off, F32(0), vis).astype(F32)
    drawn = (weight > 0.5) & (mu[..., 0] + t + 1 > 0) & (mu[..., 1] + t + 1 > 0)
    tw = weight if joints_weight is None else (weight * np.asarray(joints_weight, F32).reshape(1, -1)).astype(F32)
    return mu, weight, tw, drawn


def generate_targets(joints, vis, hw, sigma, joints_weight=None, g=None):
    """-> targets (n,J,h,w) float32, target_weight (n,J) float32.  ``g``: another table of the same length (the host test
    substitutes the reference's values for one comparison)"""
    h, w = hw
    t = int(3 * sigma)
    g = table(sigma) if g is None else g
    mu, _, tw, drawn = target_centers(joints, vis, hw, sigma, joints_weight)
    n, J = drawn.shape
    out = np.zeros((n, J, h, w), F32)
    ys, xs = np.mgrid[0:h, 0:w]
    for i in range(n):
        for j in range(J):
            if drawn[i, j]:
                dx, dy = xs - mu[i, j, 0], ys - mu[i, j, 1]
                inside = (np.abs(dx) <= t) & (np.abs(dy) <= t)
                out[i, j][inside] = g[(dx * dx + dy * dy)[inside]]
    return out, tw


def map_loss(out, tgt, tw):
    """L[i,j] = 0.5 / (h*w) * sum_p (float64(o) * w - float64(t) * w)^2"""
    n, J, h, w = out.shape
    wd = np.asarray(tw, np.float64).reshape(n, J, 1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = out.astype(np.float64) * wd - np.asarray(tgt).astype(np.float64) * wd
        return 0.5 * (d * d).reshape(n, J, -1).sum(-1) / (h * w)


def losses(L, topk):
    """JointsMSELoss = mean(L); JointsOHKMMSELoss = mean_i mean(topk largest of L[i]) (NaN counts as largest; NaN for topk <= 0)"""
    with np.errstate(invalid="ignore"):
        mse = L.mean() if L.size else np.float64(np.nan)
        if topk <= 0:
            return mse, np.float64(np.nan)
        top = -np.sort(-L, axis=1)[:, :topk]             # descending, NaN last in numpy's order ...
        top = np.where(np.isnan(L).any(1, keepdims=True), np.nan, top)   # ... but first in torch's: such a row sums to NaN
        return mse, (top.sum(1) / topk).mean() if len(L) else np.float64(np.nan)


def max_preds(maps):
    """get_max_preds: (x, y) float32 of the first maximum (a NaN is a maximum), zeroed where the maximum is not > 0; maxvals (n,J,1)"""
    n, J, h, w = maps.shape
    flat = maps.reshape(n, J, -1)
    idx = flat.argmax(-1)
    mv = np.take_along_axis(flat, idx[..., None], -1)
    preds = np.stack([idx % w, idx // w], -1).astype(F32)
    with np.errstate(invalid="ignore"):
        preds = preds * (mv > 0).astype(F32)
    return preds, mv


def analytic_target_preds(joints, vis, hw, sigma):
    """the arg-max of the analytic target maps without the maps: mu clamped to the map where the window is drawn, else (0, 0)"""
    h, w = hw
    mu, _, _, drawn = target_centers(joints, vis, hw, sigma)
    p = np.stack([np.clip(mu[..., 0], 0, w - 1), np.clip(mu[..., 1], 0, h - 1)], -1).astype(F32)
    return p * drawn[..., None].astype(F32)


def pck(preds, tpreds, hw, thr):
    """calc_dists / dist_acc / evaluate_pck_accuracy in float32: -> dists (J,n), acc (J,), avg_acc, cnt"""
    h, w = hw
    norm = np.array([F32(h) / F32(10), F32(w) / F32(10)], F32)
    p, t = np.asarray(preds, F32), np.asarray(tpreds, F32)
    d = p / norm - t / norm
    dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F32)
    ok = (t[..., 0] > 1) & (t[..., 1] > 1)
    dists = np.where(ok, dist, F32(-1)).astype(F32).T.copy()
    J = dists.shape[0]
    acc = np.full(J, -1, F32)
    for j in range(J):
        valid = dists[j] != -1
        if valid.sum() > 0:
            acc[j] = F32((dists[j][valid] < F32(thr)).sum()) / F32(valid.sum())
    good = acc >= 0
    cnt = int(good.sum())
    avg = F32(0)
    for a in acc[good]:
        avg = F32(avg + a)
    avg = F32(avg / F32(cnt)) if cnt else F32(0)
    return dists, acc, avg, cnt


def score(out, joints=None, vis=None, targets=None, target_weight=None, sigma=2, joints_weight=None, thr=0.5, topk=0):
    """hrn_score_heatmaps in both target modes -> dict with the keys of NativeHRNet.score_heatmaps (numpy values)"""
    n, J, h, w = out.shape
    if targets is None:
        targets, tw = generate_targets(joints, vis, (h, w), sigma, joints_weight)
        tpreds = analytic_target_preds(joints, vis, (h, w), sigma)
    else:
        tw = np.asarray(target_weight, F32).reshape(n, J)
        tpreds = max_preds(np.asarray(targets, F32))[0]
    L = map_loss(out, targets, tw)
    mse, ohkm = losses(L, topk)
    preds, mv = max_preds(out)
    dists, acc, avg, cnt = pck(preds, tpreds, (h, w), thr)
    return {"loss": mse, "loss_ohkm": ohkm, "accs": acc, "avg_acc": avg, "cnt": cnt, "joints_preds": preds, "joints_target": tpreds,
            "dists": dists, "maxvals": mv, "map_loss": L}


def ulp_distance(a, b):
    """distance in float32 ulps between two arrays of finite non-negative float32"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
