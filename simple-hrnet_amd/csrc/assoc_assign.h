// hrn_assignment's shortest augmenting paths on ONE wave (postproc.cpp, step for step): the text assoc_kernel (assoc.hip) and
// tracks_kernel (tracks.hip) both compile.  u, v, minv, p, way and used live in LDS; lane l owns the columns l + 1, l + 65, ... in
// ascending order, and the wave's minimum keeps the lower column on equal values, so every step is elementwise or that argmin:
// the matching is hrn_assignment's by construction, not by tolerance.
#pragma once

#include <hip/hip_runtime.h>

#include "assoc_math.h"

namespace hrn {

// orders the LDS traffic of the lanes of ONE wave (its DS instructions execute in order; this keeps the compiler from moving
// them across and waits for the ones in flight)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct AssignLds {
    double u[kMaxTracked + 1], v[kMaxTracked + 1], minv[kMaxTracked + 1];
    int p[kMaxTracked + 1], way[kMaxTracked + 1];
    unsigned char used[kMaxTracked + 1];
};

// Called by all 64 lanes of one wave with wave-uniform n, m in [1, kMaxTracked]: the minimum-cost assignment of the dense (n, m)
// matrix `cost` (row pitch m).  col[r] = the column of row r for every assigned row; the caller has filled col[0 .. n) with -1 and
// reads it after a block barrier.  Returns false (col untouched) when there was no augmenting path: cannot happen with finite costs.
__device__ inline bool assoc_assign_wave(const double *cost, int n, int m, int lane, AssignLds &L, int *col) {
#pragma clang fp contract(off)
    const bool tr = n > m;                          // rows > cols: work on the transposed matrix
    const int nn = tr ? m : n, mm = tr ? n : m;     // nn <= mm
    const double inf = __builtin_huge_val();
    for (int j = lane; j <= mm; j += 64) L.v[j] = 0.0, L.p[j] = 0, L.way[j] = 0;
    for (int i = lane; i <= nn; i += 64) L.u[i] = 0.0;
    bool ok = true;
    for (int i = 1; i <= nn; ++i) {
        for (int j = lane; j <= mm; j += 64) L.minv[j] = inf, L.used[j] = 0;
        if (lane == 0) L.p[0] = i;
        wave_sync();
        int j0 = 0;
        for (;;) {
            if (lane == 0) L.used[j0] = 1;
            wave_sync();
            const int i0 = __builtin_amdgcn_readfirstlane(L.p[j0]);
            const double ui0 = L.u[i0];
            double best = inf;
            int bestj = 0;
            for (int j = lane + 1; j <= mm; j += 64) {
                if (L.used[j]) continue;
                const double c = tr ? cost[(size_t)(j - 1) * m + (i0 - 1)] : cost[(size_t)(i0 - 1) * m + (j - 1)];
                const double cur = c - ui0 - L.v[j];
                double mv = L.minv[j];
                if (cur < mv) mv = cur, L.minv[j] = cur, L.way[j] = j0;
                if (mv < best) best = mv, bestj = j;
            }
            for (int o = 32; o > 0; o >>= 1) {      // the lower value; on equal values the lower column
                const double wv = __shfl_xor(best, o);
                const int wj = __shfl_xor(bestj, o);
                if (wv < best || (wv == best && wj < bestj)) best = wv, bestj = wj;
            }
            const int j1 = __builtin_amdgcn_readfirstlane(bestj);
            const double delta = best;
            if (j1 == 0) {                          // no augmenting path (cannot happen with finite costs): the loop still ends
                ok = false;
                break;
            }
            // (ui0 above is every lane's read of u[i0]; the writes below come later in the wave's program order, and no
            // wave_sync is needed between them only because one wave64 runs in lockstep: keep the ui0 load ABOVE this update)
            if (lane == 0) L.u[L.p[0]] += delta, L.v[0] -= delta;   // column 0 is always used
            for (int j = lane + 1; j <= mm; j += 64) {
                if (L.used[j])
                    L.u[L.p[j]] += delta, L.v[j] -= delta;          // (the rows of used columns are distinct)
                else
                    L.minv[j] -= delta;
            }
            j0 = j1;
            wave_sync();
            if (__builtin_amdgcn_readfirstlane(L.p[j0]) == 0) break;
        }
        if (!ok) break;
        if (lane == 0) {
            do {
                const int j1 = L.way[j0];
                L.p[j0] = L.p[j1];
                j0 = j1;
            } while (j0);
        }
        wave_sync();
    }
    if (!ok) return false;
    for (int j = lane + 1; j <= mm; j += 64)
        if (L.p[j]) {
            const int small = L.p[j] - 1, big = j - 1;
            if (tr)
                col[big] = small;
            else
                col[small] = big;
        }
    return true;
}

}  // namespace hrn
