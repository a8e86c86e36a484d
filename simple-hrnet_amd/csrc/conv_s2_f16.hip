// fp16 instantiation of the stride-2 slab kernel (conv_s2.hip: design notes; conv_s2.inc: the body) on v_mfma_f32_16x16x32_f16 /
// v_cvt_pk_f16_f32.  A translation unit of its own, so that conv_s2.hip still compiles to exactly one (bf16) slab kernel.
#include "kernels.h"
#include "elem.h"

namespace hrn {

#include "conv_s2.inc"

// (called by launch_conv_s2, conv_s2.hip)
hipError_t launch_conv_s2_f16(const S2Problem *probs_dev, const void *map_dev, int nblocks, hipStream_t s) {
    return launch_conv_s2_t<DT_F16>(probs_dev, map_dev, nblocks, s);
}

}  // namespace hrn
