"""The wave-parallel assignment of csrc/assoc.hip (phase 2), restated lane by lane in Python and held against hrn_assignment
without a GPU: 64 lanes, lane l owning the columns l + 1, l + 65, ... in ascending order with strict `<`, the xor butterfly that
keeps the lower value and on equal values the lower column, the elementwise update, the serial augmenting walk.  Python floats
are IEEE doubles and nothing is fused, so every number is the kernel's.  What this pins without hardware is the lane ownership
and the tie rule: the matching must be hrn_assignment's on random matrices and on matrices with few cost levels (many exact
ties), at the sizes where the column passes change (64, 65, a partial last pass, the transposed case, the cap)."""
import numpy as np
import pytest

from conftest import load_pkg

INF = float("inf")


def wave_assignment(cost):
    """row -> column (or -1) of an (n, m) cost matrix, by the kernel's steps"""
    n, m = cost.shape
    tr = n > m
    c = (cost.T if tr else cost).tolist()             # c[i][j]: the smaller side indexes rows
    nn, mm = (m, n) if tr else (n, m)
    u, v = [0.0] * (nn + 1), [0.0] * (mm + 1)
    p, way = [0] * (mm + 1), [0] * (mm + 1)
    for i in range(1, nn + 1):
        minv, used = [INF] * (mm + 1), [False] * (mm + 1)
        p[0] = i
        j0 = 0
        while True:
            used[j0] = True
            i0 = p[j0]
            ui0 = u[i0]
            best, bestj = [INF] * 64, [0] * 64
            for lane in range(64):
                for j in range(lane + 1, mm + 1, 64):
                    if used[j]:
                        continue
                    cur = c[i0 - 1][j - 1] - ui0 - v[j]
                    mv = minv[j]
                    if cur < mv:
                        mv = minv[j] = cur
                        way[j] = j0
                    if mv < best[lane]:
                        best[lane], bestj[lane] = mv, j
            o = 32
            while o:
                nb, nj = list(best), list(bestj)
                for lane in range(64):
                    wv, wj = best[lane ^ o], bestj[lane ^ o]
                    if wv < best[lane] or (wv == best[lane] and wj < bestj[lane]):
                        nb[lane], nj[lane] = wv, wj
                best, bestj = nb, nj
                o >>= 1
            assert len(set(bestj)) == 1 and len(set(best)) == 1          # every lane holds the wave's result
            j1, delta = bestj[0], best[0]
            assert j1 != 0, "no augmenting path on finite costs"
            for j in range(mm + 1):                                       # (column 0 is always used: lane 0's extra element)
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    out = [-1] * n
    for j in range(1, mm + 1):
        if p[j]:
            small, big = p[j] - 1, j - 1
            if tr:
                out[big] = small
            else:
                out[small] = big
    return out


def reference(cost):
    out = [-1] * cost.shape[0]
    for r, col in load_pkg("postproc").assignment(cost):
        out[r] = col
    return out


def matrix(rng, n, m, levels):
    """costs as the entries make them, (double)(1.0f - sim): `levels` distinct similarities (few: many exact ties)"""
    sim = (rng.integers(0, levels, (n, m)) / np.float32(levels)).astype(np.float32)
    return (np.float32(1.0) - sim).astype(np.float64)


@pytest.mark.parametrize("levels", [2, 3, 1000000])
def test_lane_restatement_equals_hrn_assignment_on_small_matrices(levels):
    rng = np.random.default_rng(levels)
    for _ in range(60):
        n, m = (int(v) for v in rng.integers(1, 21, 2))
        cost = matrix(rng, n, m, levels)
        assert wave_assignment(cost) == reference(cost), (n, m, levels)


@pytest.mark.parametrize("n,m", [(64, 64), (65, 65), (70, 130), (130, 70), (1, 200), (200, 1), (256, 256)])
def test_lane_restatement_equals_hrn_assignment_past_one_wave_pass(n, m):
    rng = np.random.default_rng(n * 1000 + m)
    for levels in (3, 1000000) if n * m < 30000 else (1000000,):    # (the cap once: the restatement is Python)
        cost = matrix(rng, n, m, levels)
        assert wave_assignment(cost) == reference(cost), (n, m, levels)
    if n * m >= 30000:
        return
    dup = np.tile(matrix(rng, (n + 2) // 3, (m + 2) // 3, 1000000), (3, 3))[:n, :m]   # everybody three times: only the tie rule decides
    assert wave_assignment(dup) == reference(dup)
