// 3x3 / stride-2 / pad-1 convolutions with 48 (HRNet-W48, branch 0) or 32 / 64 (HRNet-W32, branches 0 / 1) input channels: the
// first convs of the fuse-down chains and the chain convs that follow them (models_/hrnet.py:36-51) as an LDS-staged implicit GEMM on bf16 MFMA, written for gfx950.
//
// Why its own kernel (DESIGN.md §5 "stride-2 slab kernel"): a stride-2 tile touches FOUR input pixels per output pixel and
// the 16 pixels of an MFMA fragment sit two input columns apart, so neither the stride-1 kernel's slab (one contiguous run
// of flat rows, 96-byte lane pitch) nor its tiling (512 pixels x 48 couts per block) carries over: the slab per output
// pixel is 4x larger and a lane pitch of 192 bytes is a 2-way bank conflict.  What pays here is the opposite split:
//   * M tile = R full output rows of one image (R*(Wo+1) flat output rows incl. the pad column).  Its input footprint --
//     virtual input rows 2*h0-1 .. 2*(h0+R-1)+1, each from column -1 to column W -- is staged ONCE per block in LDS by
//     LDS-DMA, de-interleaved by column parity on the way in: slot(vrow, plane, j) holds input column 2*j-1+plane, so the
//     16 pixels of a fragment are 16 consecutive 96-byte slots for every tap (96 = 32 mod 64 dwords*4: conflict-free, like
//     the stride-1 slab) and a tap is a constant slot shift  dh*2*Wop + (dw&1)*Wop + (dw>>1).  Round 4: an output row's two
//     virtual rows are followed by 0..7 pad slots (kernels.h: s2_pair_pad) so that a fragment that WRAPS an output row keeps
//     its 16 slot numbers consecutive mod 8 -- without them such fragments conflicted (32 % of the LDS cycles).
//   * N = ALL output channels of ALL convolutions that read this tensor at this fuse level (the 48->96 and the two 48->48
//     first convs of a stage-4 module: 192 couts), split over the waves in groups of 48: a wave keeps its group's whole
//     weight matrix (48 x 432 -> 14 K chunks x 3 fragments = 168 VGPRs) IN REGISTERS for the block's lifetime, so the K loop
//     has no weight traffic at all, no barrier, and one ds_read_b128 per three MFMAs; the slab crosses L2 -> LDS once per
//     tile for all 192 couts.
//   * two slab buffers (2 x 78 KiB): the next tile's slab lands while this one is computed; one barrier per tile.
//   * only REAL output rows are written (pad column included, as zeros); the pad row below an image's last row and the tail
//     guard rows are never touched -- they keep the zeros the buffer was allocated with (the workspace invariant stated at
//     hrn_ctx::new_tensor, ctx_plan.inc: buffers are zeroed once and reused by tensors of one geometry only).
// K order and MFMA operand layout are those of the generic kernel (k = tap*48 + ci in 32-wide chunks, accumulators from
// zero, bias added in the epilogue), so results are BIT-IDENTICAL to conv_direct_kernel on the same convolution -- which is
// how the small-call fallback (too few tiles to fill the chip -> generic kernel) keeps a crop's result independent of the
// batch it arrives in, and how tests check this kernel element by element.
#include "kernels.h"
#include "elem.h"

namespace hrn {

// (the kernel body: conv_s2.inc, shared with the fp16 instantiation in conv_s2_f16.hip)
#include "conv_s2.inc"

hipError_t launch_conv_s2_f16(const S2Problem *probs_dev, const void *map_dev, int nblocks, hipStream_t s);   // conv_s2_f16.hip

hipError_t launch_conv_s2(int dtype, const S2Problem *probs_dev, const void *map_dev, int nblocks, hipStream_t s) {
    if (dtype == DT_F16) return launch_conv_s2_f16(probs_dev, map_dev, nblocks, s);
    return dtype == DT_BF16 ? launch_conv_s2_t<DT_BF16>(probs_dev, map_dev, nblocks, s) : hipErrorInvalidValue;
}

}  // namespace hrn
