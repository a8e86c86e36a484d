// Arg-max order shared by the head kernels (kernels.hip) and the decode kernels (decode.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace hrn {

// Arg-max order of np.argmax / torch.max (SimpleHRNet.py:300): the first maximum wins and a NaN is a maximum (numpy
// returns the index of the first NaN).  `kNoIdx` marks "nothing seen yet": any real candidate beats it, so a map of
// -inf everywhere decodes to index 0 like numpy, not to the sentinel.
constexpr int kNoIdx = 0x7fffffff;
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    return v > bv || ((v == bv || vn) && i < bi);
}
// scan step for candidates visited in increasing index order
__device__ __forceinline__ bool takes(float v, float bv, int bi) { return v > bv || bi == kNoIdx || (v != v && bv == bv); }

}  // namespace hrn
