// 3x3 / stride-1 / pad-1 convolution (the BasicBlock convs = 84 % of HRNet-W48 FLOPs) as an LDS-staged,
// software-pipelined implicit GEMM on bf16 MFMA, written for gfx950.
//
// Data movement
//   * The flat padded NHWC layout turns the nine taps into nine constant row shifts of ONE
//     activation matrix, so a block stages a single contiguous "slab" of rows
//         [p0 - (Wp+1), p0 + BM + (Wp+1))  x  KS input channels
//     in LDS and serves all nine taps of that channel slice from it (activations cross L2->LDS once per
//     slice, not nine times).  KS = 48 -> 96-byte LDS row pitch; 96 = 32 (mod 64) makes each 16-lane
//     ds_read_b128 group (16 consecutive pixels x two 16-byte k-groups) cover all 64 banks exactly once, so
//     the natural, unswizzled image is conflict-free and is written by global_load_lds (LDS-DMA) directly.
//   * Weights of (cout tile, slice) come from a pre-packed fragment-major image (pack_conv_lds in
//     hrnet_mi355.cpp): a linear LDS-DMA copy, read back with lane*16 addressing.
//   * K is flattened per slice, k = tap*KS + ci, in 32-wide MFMA chunks: 432 -> 14 chunks (last one half
//     zero; the 16x16x16 MFMA that would avoid the padding costs the same 16 cycles on gfx950 -- measured).
// Pipeline (one block per CU, 8 waves = 2 per SIMD, persistent over `tiles_per_block` M tiles)
//   * unit of work = half a slice (7 chunks).  LDS holds two weight half-buffers (2 x 21 KiB) and two slab
//     buffers (2 x 56 KiB).  At the top of half-stage h every wave waits for its own LDS-DMA (vmcnt 0), the
//     block meets at ONE barrier, the loads of half-stage h+1 (next weight half; next slab when a new slice
//     or tile starts) are issued, then half-stage h is computed -- so every load has a full compute phase
//     (>= 1344 MFMA cycles) to land, also across tile boundaries and under the epilogue.
//   * single-slice problems (cin == 48) keep both weight halves resident across tiles.
//   * an LDS-DMA instruction costs its wave ~100+ issue cycles and the epilogue is store-latency bound, so
//     two waves share each SIMD: while one issues loads / stores, the other keeps the MFMA pipe busy.
//     The residual tile is requested before the last half-stage's MFMAs and is in registers by the epilogue.
// Tile: wave = 16*MR pixels x 48 couts (MR = 4: BM = 512, MR = 3: BM = 384 for the 96x72 branch whose halo
// would not fit twice); operands swapped (D = W * X^T) so a lane owns 12 contiguous channels of one pixel.
// One launch covers a GROUP of independent convolutions (the k-th conv of every branch of a stage module).
// The kernel bodies live in conv3x3_lds.inc, templated on the element format; this file instantiates the bf16 ones
// (conv3x3_lds_f16.hip: the fp16 ones).
#include "kernels.h"
#include "elem.h"

namespace hrn {

#include "conv3x3_lds.inc"

#ifdef HRN_C3_TIMING
// debug: per-block phase cycle counters of the most recent launch (tools/c3_timing.py)
extern "C" int hrn_debug_c3_timing(long long *host_out, int max_blocks) {
    static long long *buf = nullptr;
    if (!buf) {
        if (hipMalloc((void **)&buf, (size_t)max_blocks * 512) != hipSuccess) return -1;
        (void)hipMemset(buf, 0, (size_t)max_blocks * 512);
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_c3_timing), &buf, sizeof(buf));
        return 0;
    }
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(host_out, buf, (size_t)max_blocks * 512, hipMemcpyDeviceToHost);
    return 1;
}
#endif

#ifdef HRN_Q_TIMING
// first call: allocate + arm; later calls: copy out [slot][block][4] = {t0, grid | seq << 32, t1, CU id}
extern "C" int hrn_debug_q_timing(long long *host_out) {
    static long long *buf = nullptr;
    const size_t bytes = (size_t)kQSlots * kQBlocks * 4 * sizeof(long long);
    if (!buf) {
        if (hipMalloc((void **)&buf, bytes) != hipSuccess) return -1;
        (void)hipMemset(buf, 0, bytes);
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_q_timing), &buf, sizeof(buf));
        return 0;
    }
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(host_out, buf, bytes, hipMemcpyDeviceToHost);
    return 1;
}
#endif

int conv3x3_n96_ch64() { return N96_CH64; }
int conv3x3_n96_max_rows() { return N96_MAXROWS; }

// X of a tile fits XY, and so do the whole 64-lane LDS-DMA pieces of a sliding tile's last 2 halo rows (bbf_run: fetch_x)
int conv3x3_lds_bbf_ok(int wp) {
    const int cunits = 2 * (wp + 1) * 6;
    return (512 + 4 * (wp + 1)) * 6 <= BBF_XY / 16 && 3072 + cunits + (cunits + 63) / 64 * 64 <= BBF_XY / 16;
}

// pixels per M tile for a (KS, wp) pair: 512, or 384 when two 512-row slabs (+ halo) would not fit in LDS; 0 = unsupported
int conv3x3_lds_bm(int ks, int nrb, int wp) {
    if (ks == 16) return conv3x3_f32_bm(wp);   // fp32 kernel
    // (96-cout form: the last LDS-DMA piece of a slab is written in whole 16-row chunks -- the rows, rounded up to 16, must fit the buffer)
    if (ks == 32 && nrb == 6) {
        auto fits = [&](int bm) { return (bm + 2 * wp + 2 + 15) / 16 * 16 <= N96_MAXROWS; };
        return fits(512) ? 512 : fits(384) ? 384 : 0;
    }
    const int maxrows = ks == 48 ? C3Cfg<48, 3>::MAXROWS : C3Cfg<32, 4>::MAXROWS;
    if (nrb != 4 && 512 + 2 * wp + 2 <= maxrows) return 512;
    if (384 + 2 * wp + 2 <= maxrows) return 384;
    return 0;
}

hipError_t launch_conv3x3_lds_f16(const Conv3Problem *probs_dev, const void *blockmap_dev, int nblocks, int nb, int ks, int nrb,
                                  hipStream_t s);   // conv3x3_lds_f16.hip

hipError_t launch_conv3x3_lds(int dtype, const Conv3Problem *probs_dev, const void *blockmap_dev, int nblocks, int nb, int ks,
                              int nrb, hipStream_t s) {
    if (dtype == DT_F16) return launch_conv3x3_lds_f16(probs_dev, blockmap_dev, nblocks, nb, ks, nrb, s);
    if (nblocks > 0 && ks == 16) return launch_conv3x3_f32(probs_dev, blockmap_dev, nblocks, nb, nrb, s);
    return launch_conv3x3_lds_t<DT_BF16>(probs_dev, blockmap_dev, nblocks, nb, ks, nrb, s);
}

}  // namespace hrn
