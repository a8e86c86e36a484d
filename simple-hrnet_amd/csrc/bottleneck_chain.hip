// Bottleneck tail + next Bottleneck head in one pass (layer1, modules.py:20-40), bf16, gfx950.
//
//   y  = relu( W3 * t2 + b3 + residual )        conv3 + bn3 + shortcut + ReLU of block b      (64 -> 256)
//   t' = relu( W1' * y + b1' )                  conv1 + bn1 + ReLU of block b+1              (256 -> 64)
//
// Both are 1x1 convolutions whose cost is memory: run separately, y (0.9 GB per 256 crops) is written by the first
// and read back by the second.  Here a wave keeps its 16 pixels x 256 channels of y in registers: the D fragments
// of the first product, rounded to bf16 exactly as they are stored, ARE the B operand of the second one.
//   * W3 is packed with 32-cout groups (generic image, NR = 2): lane (li, g) then owns channels j*32 + g*8 + [0,8)
//     of pixel li for j = 0..7 -- which is the K slice (chunk j, k-group g) the second MFMA wants from that lane.
//     No cross-lane movement, no LDS round trip, natural K order (bit-identical to the two separate kernels).
//   * W1' uses the generic image with NR = 4: a lane ends with 16 contiguous output channels.
//   * Both weight images (32 KiB each) and the biases sit in LDS; every MFMA reads its A fragment from there.
//   * Block 0's shortcut is itself a 1x1 conv of the block input (downsample, 64 -> 256, no ReLU).  The DS variant
//     computes it here, in its own accumulators, rounds it to bf16 exactly where the separate kernel would store
//     it, and adds it -- the 0.9 GB tensor is neither written nor read.
//   * No barrier after the weights are staged: each wave walks its own 16-pixel fragments (2 blocks = 8 waves per
//     CU keep ~80 KiB of loads in flight, which is what the HBM pipe needs).
//   * Round 5 (C3): the Bottleneck's 3x3 convolution (conv2 + bn2 + ReLU, 64 -> 64) in FRONT of conv3, for the blocks without a
//     projection shortcut:  t2 = relu( W2 (*) t1 + b2 )  is computed per 16-pixel fragment from conv1's output t1 -- the nine taps
//     are nine constant row shifts of the flat padded layout, 18 fragment loads of 16 B per lane that L1 / L2 serve (a pixel's
//     128-byte row is one cache line, neighbouring taps share 15 of their 16 lines) -- in the GENERIC kernel's arithmetic
//     (k = tap * 64 + ci in 32-wide chunks, accumulators from zero, bias added last; W2 in the generic image with NR = 2), so
//     its D fragments, rounded to bf16 exactly where conv_direct_kernel would store them, ARE conv3's B operand: t2 (0.23 GB
//     per 256 crops) is neither written nor read, and the launch of the 3x3 kernel (0.15 ms) is gone.  HBM traffic of the
//     launch is unchanged (t1 is read instead of t2); W2 (72 KiB) joins W3 / W1' in LDS: one 8-wave block per CU.
//     C3 = 2: the last Bottleneck of the layer -- no conv1 of a next block behind it.
#include <stdlib.h>

#include "kernels.h"
#include "elem.h"

namespace hrn {

// (the kernel bodies: bottleneck_chain.inc, shared with the fp16 instantiations in bottleneck_chain_f16.hip)
#include "bottleneck_chain.inc"

hipError_t launch_bottleneck_chain_f16(const ChainArgs &a, hipStream_t s);   // bottleneck_chain_f16.hip

hipError_t launch_bottleneck_chain(int dtype, const ChainArgs &a, hipStream_t s) {
    if (dtype == DT_F16) return launch_bottleneck_chain_f16(a, s);
    return dtype == DT_BF16 ? launch_bottleneck_chain_t<DT_BF16>(a, s) : hipErrorInvalidValue;
}

}  // namespace hrn
