// fp16 instantiations of the layer1 chain kernels (bottleneck_chain.hip: design notes; bottleneck_chain.inc: the bodies) on
// v_mfma_f32_16x16x32_f16.  A translation unit of its own, so that bottleneck_chain.hip still compiles to exactly four (bf16) kernels.
#include <stdlib.h>

#include "kernels.h"
#include "elem.h"

namespace hrn {

#include "bottleneck_chain.inc"

// (called by launch_bottleneck_chain, bottleneck_chain.hip)
hipError_t launch_bottleneck_chain_f16(const ChainArgs &a, hipStream_t s) { return launch_bottleneck_chain_t<DT_F16>(a, s); }

}  // namespace hrn
