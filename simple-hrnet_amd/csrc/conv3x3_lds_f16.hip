// fp16 instantiations of the LDS-staged 3x3 convolution kernels (conv3x3_lds.hip: design notes; conv3x3_lds.inc: the bodies):
// <48, 3> with the 96-cout form and the fused BasicBlock, <32, 4>, <32, 3> and <32, 2>, on v_mfma_f32_16x16x32_f16.  A translation
// unit of its own, so that conv3x3_lds.hip still compiles to exactly the bf16 kernel set.
#include "kernels.h"
#include "elem.h"

// (the per-block timing probes are a bf16 debug aid of conv3x3_lds.hip, which owns their device symbols)
#undef HRN_Q_TIMING
#undef HRN_C3_TIMING

namespace hrn {

#include "conv3x3_lds.inc"

// (called by launch_conv3x3_lds, conv3x3_lds.hip)
hipError_t launch_conv3x3_lds_f16(const Conv3Problem *probs_dev, const void *blockmap_dev, int nblocks, int nb, int ks,
                                  int nrb, hipStream_t s) {
    return launch_conv3x3_lds_t<DT_F16>(probs_dev, blockmap_dev, nblocks, nb, ks, nrb, s);
}

}  // namespace hrn
