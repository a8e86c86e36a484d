// Device-side interface of the HRNet hot path: argument blocks + launchers.
// Everything here is gfx950 (CDNA4) only; see DESIGN.md for layouts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cstdlib>
#include <cstring>

namespace hrn {

// Kernels that use more than 64 KiB of dynamic LDS: hipFuncAttributeMaxDynamicSharedMemorySize is a property of the function ON
// ONE DEVICE, so it is set once per (kernel, device) -- a process-wide "done" flag left every device but the first handle's without
// it (one process driving several GPUs: native.MultiDeviceHRNet).  `done` = one bit per device ordinal.
inline hipError_t set_dynamic_lds(const void *func, int bytes, std::atomic<unsigned long long> &done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return e;
}
// ... and the launch of such a kernel: the attribute set to attr_bytes (>= lds_bytes: a kernel whose launches differ in size asks for
// its largest layout once), then the launch.  `done` is a static of this template: one mask per kernel instantiation.
template <auto Kernel, class... Args>
inline hipError_t launch_large_lds(int attr_bytes, dim3 grid, dim3 block, int lds_bytes, hipStream_t s, const Args &...args) {
    static std::atomic<unsigned long long> done{0};
    const hipError_t e = set_dynamic_lds((const void *)Kernel, attr_bytes, done);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, s, args...);
    return hipGetLastError();
}

// The HRN_* switches exist for same-box A/B runs and the bit-identity tests.  In production NONE of them is
// read: the library's behaviour does not depend on the caller's environment.  A process that sets HRN_DEBUG_ENV=1 (the test suite,
// tools/ab.sh) opts in; the switches are then read ONCE, when a handle is created (hrn_create snapshots what it saw:
// hrn_switches()), never during a call.
inline const char *hrn_env(const char *name) {
    static const bool debug = [] {
        const char *v = getenv("HRN_DEBUG_ENV");
        return v && *v && strcmp(v, "0") != 0;
    }();
    return debug ? getenv(name) : nullptr;
}

enum { DT_F32 = 0, DT_BF16 = 1, DT_F16 = 2 };   // = HRN_F32 / HRN_BF16 / HRN_F16 (include/hrnet_mi355.h)

// Activation tensors use the "flat padded NHWC" layout:
//   row(n, r, c) = n*Hp*Wp + r*Wp + c,  Wp = W+1, Hp = H+1, C channels per row,
//   the extra column / row of every image hold zeros, as do the guard rows before
//   image 0 and after the last image.  A 3x3/pad-1 tap (dh,dw) is then the constant
//   row shift dh*Wp+dw -- no boundary tests in the inner loop.
struct ConvArgs {
    const void *in;     // row 0 of the input tensor
    void *out;          // row 0 of the output tensor
    const void *w;      // packed weights (fragment-major, see pack_conv_weights)
    const float *bias;  // folded BN bias, fp32[cout]
    const void *res;    // residual tensor (same geometry as out) or nullptr
    int cin, cout;
    int in_wp, in_hpwp;                     // input row pitch / image pitch (rows)
    int out_h, out_w, out_wp, out_hpwp;     // output geometry
    int m;                                  // rows to produce = n * out_hpwp
    int ksize, stride, relu;
    int kchunks;                            // padded K / (32 bf16 | 16 f32)
    int rev;                                // walk the M tiles backwards (see hrn_ctx::alternate)
    int pre_mode;                           // K = 64 1x1 convs with a residual: 0, or 1: the residual is fetched before the K loop (kernels.hip: PRE)
    int wlds;                               // bf16, full-size tiles: weights staged through LDS once per block (kernels.hip: WL)
    int xlds;                               // ... and, for the stride-2 3x3 convolutions with cin % 32 == 0, the pixel fragments through a per-wave LDS ring (kernels.hip: XL)
    // one phase (a, b) of a ConvTranspose2d(4, stride 2, padding 1) run as a 3x3 conv on the input grid: the result of
    // pixel (ho, wo) is stored at (2*ho + a, 2*wo + b) of the twice-as-large tensor (poseresnet.py:84-100)
    int up, up_a, up_b, up_wp, up_hpwp;
    int taps[4];                            // ksize == 2: row shift of the four live taps (tap-major K = 4*cin)
};

// LDS-staged 3x3 stride-1 convolution (conv3x3_lds.hip); input and output share one geometry.
// One device-resident descriptor per convolution; a launch covers a group of them.
struct Conv3Problem {
    const void *in;
    void *out;
    const void *w;      // slice-major packed weights: [cout tile][slice][chunk][frag][lane][16 B]
    const float *bias;
    const void *res;
    int cin, cout;
    int h, wd, wp, hpwp;
    int relu;
    int slices;         // cin / KS
    int ntiles;         // cout / (16*NRB)
    int tiles_per_block;  // consecutive M tiles one block walks (weights stay in LDS when slices == 1)
    int bm;               // pixels per M tile: 512, or 256 when two 512-row slabs would not fit in LDS
    // x / d == (x * magic) >> shift for x < 2^27, magic = floor(2^shift / d) + 1, shift = 30 + ceil(log2 d)
    unsigned magic_hpwp, magic_wp;
    int shift_hpwp, shift_wp;
    // fused BasicBlock (conv3x3_lds.hip: bbf_run): this problem is conv1, w2 / bias2 are conv2's, `out` is the block's
    // output and `in` doubles as the residual
    const void *w2;
    const float *bias2;
    // 96-cout form (conv3x3_n96.inc): KS = 32, ntiles = cout / 96, bm = 512 or 384
    int n96;
    // ... with the COMPACT enumeration of M (round 4): tiles of real pixels only; hw = h * wd; fast divisions by hw and wd;
    // rows of a tile's slab (the longest run of flat rows a tile of `bm` / of 128 pixels spans, + 2 wp + 2)
    int compact, hw;
    unsigned magic_hw, magic_w;
    int shift_hw, shift_w;
    int slab_rows, slab_rows_small;
};
int conv3x3_n96_ch64();           // output-channel permutation of the 96-cout form's weight image (conv3x3_n96.inc)
int conv3x3_lds_bbf_ok(int wp);  // the fused BasicBlock kernel fits this row pitch
int conv3x3_n96_max_rows();   // rows (of 64 bytes) one slab buffer of the 96-cout form holds
int conv3x3_lds_bm(int ks, int nrb, int wp);  // (32, 6) = the 96-cout form; ks = 16: the fp32 kernel (conv3x3_f32.hip)
int conv3x3_f32_bm(int wp);
hipError_t launch_conv3x3_f32(const Conv3Problem *probs_dev, const void *blockmap_dev, int nblocks, int nb, int nrb, hipStream_t s);

// Stride-2 slab kernel (conv_s2.hip): every 3x3 / stride-2 convolution with 48 (HRNet-W32: 32 / 64) input channels that reads ONE tensor at
// one fuse level contributes "parts" (48 (32) output channels each) to one problem; a block stages the input slab of `rows`
// output rows once and its waves keep the parts' weights in registers.
constexpr int kS2SlabBytes = 79872;   // one slab buffer: 832 sub-slots of 96 bytes (two of them + the biases fill the 160 KiB)
constexpr int s2_frags_per_part(int cin) { return cin == 48 ? 3 : 2; }   // 16-cout fragments a wave keeps in registers
// a pixel's cin * 2 bytes are kept in LDS as sub-slots of 96 (cin = 48, 96) or 32 (cin = 32, 64) bytes, one region per sub-slot
// index; a region is a whole number of 1-KiB LDS-DMA pieces
constexpr int s2_subslot_bytes(int cin) { return cin % 48 == 0 ? 96 : 32; }
constexpr int s2_region_bytes(int cin) { return kS2SlabBytes / (cin * 2 / s2_subslot_bytes(cin)) / 1024 * 1024; }
constexpr int s2_slot_capacity(int cin) { return s2_region_bytes(cin) / s2_subslot_bytes(cin); }   // input pixels one slab buffer holds
// The slab keeps TWO virtual input rows (4 wop slots: both column parities of both rows) + `pad` empty slots per output row, so
// that the 16 pixels of a fragment that wraps an output row stay on disjoint LDS banks: the wrap jumps 3 wop + 1 + pad slots,
// and sub-slots of 96 (32) bytes are conflict-free for 16 lanes iff their slot numbers are consecutive mod 8 (round 4: the
// unpadded slab measured a 32 % LDS bank-conflict rate, profiles/round3_pmc_s2.txt).
constexpr int s2_pair_pad(int wop) { return (8 - (3 * wop) % 8) % 8; }
constexpr int s2_pair_pitch(int wop) { return 4 * wop + s2_pair_pad(wop); }   // slots per output row of the slab
constexpr int kS2MaxParts = 8;
struct S2Part {
    const void *w;      // [K chunks][frags][64 lanes][16 B]: the (cin, frags) image of pack_conv_lds for this cout tile (k = tap * cin + ci)
    const float *bias;  // the convolution's folded bias (indexed with ch0 + c)
    void *out;          // row 0 of the convolution's output tensor
    int cout, ch0;      // channels per row of that tensor, first channel of this part
    int relu, pad_;
};
struct S2Problem {
    const void *in;     // row 0 of the input tensor
    int cin;            // 32, 48 or 64
    int in_wp, in_hpwp;
    int ho, wo, wop, out_hpwp;   // output geometry (shared by all parts)
    int rows;                    // output rows per tile
    int tiles_per_image;         // ceil(ho / rows)
    int nparts;                  // cout groups (of 16 * s2_frags_per_part(cin) channels)
    // wave w works on part wave_part[w] (0xff: idle) and on the pixel fragments wave_f0[w], + wave_fs[w], ... of every tile
    unsigned char wave_part[8], wave_f0[8], wave_fs[8];
    unsigned magic_wop;          // x / wop == (x * magic) >> shift
    int shift_wop;
    S2Part part[kS2MaxParts];
};
hipError_t launch_conv_s2(int dtype, const S2Problem *probs_dev, const void *map_dev, int nblocks, hipStream_t s);

// The stem as one kernel (stem_fused.hip, round 4, bf16): conv1 computed into the stride-2 slab's LDS layout, conv2 from there;
// one output row of conv2 per tile.  `probs_dev[.]` = conv2 as a slab-kernel problem with rows = 1 (its `in` is not read),
// `stem` = conv1's arguments (its `out` is not written).
constexpr int kStemFuseRegionBytes = 15360;   // one 16-channel region of a slab buffer: 480 sub-slots of 32 bytes
constexpr int kStemFusePatchBytes = 12544;    // one patch buffer: 7 crop rows x 3 colours x (W + 8) bf16 (W <= 288: the slab's limit)
int stem_fused_fits(int wop, int w_in);

// layer1: conv3 (+shortcut, ReLU) of one Bottleneck and conv1 (+ReLU) of the next in one pass (bottleneck_chain.hip)
struct ChainArgs {
    const void *in;        // conv2 output of block b: [rows][64]
    const void *res;       // shortcut of block b: [rows][256]
    void *out_y;           // block b output: [rows][256]
    void *out_t;           // conv1 output of block b+1: [rows][64]
    const void *w3;        // 256 x 64, generic fragment image with NR = 2
    const float *b3;
    const void *w1;        // 64 x 256, generic fragment image with NR = 4 (nullptr with w2: the layer's last block, no next conv1)
    const float *b1;
    const void *in3;       // round 5 (w2 != nullptr): conv1's output t1 [rows][64]; conv2 (3x3) is computed here, `in` is not read
    const void *w2;        // 64 x 576, generic fragment image with NR = 2 (k = tap * 64 + ci), or nullptr
    const float *b2;
    const void *x;         // block 0 only (wds != nullptr): the block input [rows][64]; the shortcut is Wds*x + bds
    const void *wds;       // 256 x 64, generic fragment image with NR = 2, or nullptr (shortcut read from `res`)
    const float *bds;
    int m, h, w, wp, hpwp; // rows to produce = n*hpwp; geometry for the pad mask
    int rev;
    int max_blocks;        // persistent blocks of the launch (512: two per CU)
};
// the grid of a chain-kernel launch (bottleneck_chain.inc: launch_chain_t; hrn_plan_launch_walk reports it): waves per block of the
// kernel form (projection shortcut folded in: `ds`; the 3x3 in front of conv3: `c3`) and the persistent blocks of a call of m rows
constexpr int chain_waves(bool ds, bool c3) { return c3 || ds ? 8 : 4; }
inline int chain_grid(int m, bool ds, bool c3, int max_blocks) {
    const int blocks_env = max_blocks > 0 ? max_blocks : 512;
    const int waves = chain_waves(ds, c3), mfrags = (m + 15) / 16;
    const int blocks = (mfrags + waves - 1) / waves;
    const int cap = (ds || c3) ? (blocks_env / 2 > 1 ? blocks_env / 2 : 1) : blocks_env;   // (HRN_CHAIN_BLOCKS < 2 must not give a zero grid)
    return blocks > cap ? cap : blocks;
}
hipError_t launch_bottleneck_chain(int dtype, const ChainArgs &a, hipStream_t s);

struct StemArgs {          // conv1 3->64 3x3 s2 + BN + ReLU, NCHW fp32 in, flat padded out
    const float *images;   // (n,3,H,W)
    void *out;
    const float *w;        // [27][64] fp32, folded
    const float *bias;     // [64]
    const void *wp;        // bf16 mode: MFMA image of the weights, [4 frags][64 lanes][8 bf16], K = 27 padded to 32
    int n, H, W;           // input size
    int out_h, out_w, out_wp, out_hpwp;
    int flip;              // read the crops mirrored left-right (flip-TTA: misc/utils.py flip_tensor(image, dim=-1))
};

hipError_t launch_stem_fused(int dtype, const S2Problem *probs_dev, const void *map_dev, int nblocks, const StemArgs &stem, hipStream_t s);

// Crop pre-path (prepath.hip): one person's slice of its frame, its zero padding and where its horizontal pass lives
struct CropParams {
    int x1, y1, w_crop, h_crop;   // slice of the frame that is actually read (numpy clamps the stop index)
    int pad_top, pad_left;        // zero rows / columns in front of it (np.pad)
    int h_pad, w_pad;             // size of the padded crop = input of the resize
    long long tmp_off;            // byte offset of this crop's [h_pad][W][3] uint8 intermediate
    const unsigned char *frame;   // the frame this person is cut from: (frame_h, frame_w, 3) uint8 BGR, device
    int frame_w, frame_h;
};
// crops [0, n) of crops_dev, each from its own frame, into images_dev[0, n); any n (sliced by the grid's y limit)
hipError_t launch_prepath(const CropParams *crops_dev, int n, int max_h_pad, unsigned char *tmp_dev, float *images_dev, int H, int W,
                          hipStream_t s);
// The same pre-path cut from 4:2:0 YCbCr frames (NV12 / NV21 / I420, 10-bit P010 / I010): person i's CropParams (frame = nullptr, frame_w / frame_h the
// frame's size) plus this record of its own -- CropParams, the BGR kernels and their launch stay exactly as they are.
struct YuvSource {
    const unsigned char *y, *u, *v;   // planes of the person's frame, device; NV12 / NV21 / P010: u = the interleaved plane, v unused
    int pitch_y, pitch_c;             // bytes between rows of the Y plane / of a chroma plane (10-bit layouts: rows of 16-bit words)
    int format;                       // HRN_PIX_NV12 (1), _I420 (2), _NV21 (4), _P010 (5) or _I010 (6): yuv_px.h's kPix*
    int coef[6];                      // y0, CY, CUB, CUG, CVG, CVR of hrn_yuv_coefficients: 20-bit fixed point
    int pad_;
};
// as launch_prepath, the horizontal pass reading every tap through the YUV -> RGB conversion; the vertical pass is the same kernel
hipError_t launch_prepath_yuv(const CropParams *crops_dev, const YuvSource *src_dev, int n, int max_h_pad, unsigned char *tmp_dev,
                              float *images_dev, int H, int W, hipStream_t s);
// a whole frame to contiguous (height, width, 3) uint8 BGR (prepath.hip): height and width even
hipError_t launch_yuv_to_bgr(const YuvSource &src, int height, int width, unsigned char *bgr_dev, hipStream_t s);
// single-person pre-path (prepath.hip): cv2.resize of whole frames; one entry per output column, then per output row
struct ResizeTaps {
    int ofs;       // first source index of the window (may lie outside: replicate border)
    short c[4];    // fixed-point coefficients, 11 bits
};
// the scale of an axis, as cv2's resize() forms it: 1 / ((double)dst / src) (the host passes it to the kernels: resize_taps.h)
inline double resize_scale(int dst, int src) { return 1.0 / ((double)dst / (double)src); }
hipError_t launch_resize_frames(const unsigned char *frames_dev, int n, int src_h, int src_w, int interp, ResizeTaps *taps_dev,
                                float *images_dev, int H, int W, hipStream_t s);
// evaluation pre-path (warp.hip): cv2.warpAffine(INTER_LINEAR, zero border) of one crop out of one frame of the stack
struct WarpParams {
    double m[6];   // the INVERSE 2x3 matrix (crop -> frame), row-major, inverted on the host as cv::warpAffine does
    int frame;     // index into the frame stack
    int pad_;
};
hipError_t launch_warp_crops(const unsigned char *frames_dev, int frame_h, int frame_w, const WarpParams *params_dev, int n,
                             float *images_dev, int H, int W, hipStream_t s);

struct Stem7Args {         // PoseResNet conv1: 3->64 7x7 s2 p3 + BN + ReLU, NCHW fp32 in, flat padded out (poseresnet.py:25-27)
    const float *images;
    void *out;
    const float *w;        // [147][64] fp32, folded, k = (ci*7 + kh)*7 + kw
    const float *bias;     // [64]
    const void *wp;        // bf16 mode: MFMA image [5 chunks][4 frags][64 lanes][8 bf16], K = 147 padded to 160
    int n, H, W;
    int out_h, out_w, out_wp, out_hpwp;
    int flip;
};
struct PoolArgs {          // MaxPool2d(3, stride 2, padding 1) on a post-ReLU tensor (poseresnet.py:28): zero pads == -inf pads
    const void *in;
    void *out;
    int c, n;
    int in_wp, in_hpwp;
    int out_h, out_w, out_wp, out_hpwp;
};
hipError_t launch_stem7(int dtype, const Stem7Args &a, hipStream_t s);
hipError_t launch_maxpool(int dtype, const PoolArgs &a, hipStream_t s);

struct FuseTerm {
    const void *ptr;
    int shift;      // nearest-upsample factor 2^shift (0 = same resolution)
    int wp, hpwp;   // geometry of the term tensor
};
struct FuseArgs {          // out = relu(sum_j term_j) in order j = 0..nterms-1
    FuseTerm t[4];
    int nterms;
    void *out;
    int c, h, w, wp, hpwp;
    int m;                 // n * hpwp
    int rev;               // walk the rows backwards
};

struct FuseGroupArgs {     // up to four independent fuse outputs in one launch; block b belongs to f[k] with block_end[k-1] <= b < block_end[k]
    FuseArgs f[4];
    int nf;
    int block_end[4];
};
hipError_t launch_fuse_group(int dtype, FuseGroupArgs &g, hipStream_t s);

constexpr int kMaxJoints = 256;   // = HRN_MAX_JOINTS (include/hrnet_mi355.h): joints of a head, worked in groups of 32 (kernels.hip)
struct HeadArgs {          // final 1x1 conv (+bias) and per-(crop, joint) partial arg-max
    const void *in;        // fused branch 0, flat padded, c channels
    const float *wgt;      // [joints][c] fp32
    const void *wimg;      // bf16 mode: MFMA image of the weights, [ceil(joints/32) groups][2 frags][ceil(c/32) chunks][64 lanes][8 bf16]
    const float *bias;     // [joints]
    float *heatmaps;       // (n,joints,h,w) fp32 NCHW or nullptr
    float *part_val;       // [n][joints][slabs]
    int *part_idx;
    int n, c, joints, h, w, wp, hpwp, slabs, slab_px;
};

// Heat-map to joint decoding (decode.hip).  The sub-pixel modes move the integer arg-max by a quarter cell towards the higher
// neighbour (get_final_preds) or by DARK's Newton step on the log of the Gaussian-blurred map (include/hrnet_mi355.h: HRN_REFINE_*).
enum { RF_NONE = 0, RF_QUARTER = 1, RF_DARK = 2 };   // = HRN_REFINE_NONE / _QUARTER / _DARK
struct DecodeArgs {        // SimpleHRNet.py:297-308
    const float *part_val; // decode_kernel: the head's slab candidates
    const int *part_idx;
    const void *boxes;     // decode_kernel: (n,4) int32 or fp32
    int box_is_float;
    float *pts;            // decode_kernel: (n,joints,3) (y, x, confidence)
    int n, joints, h, w, slabs, mode;
    const float *heatmaps; // (n,joints,h,w) fp32, as the head wrote them: read where mode != RF_NONE
    float *coords;         // refine_coords_kernel: (n,joints,2) (x, y) in heat-map cells, integer-valued in, refined in place
};
hipError_t launch_decode(const DecodeArgs &a, hipStream_t s);   // decode_kernel<mode>
hipError_t launch_refine_coords(const DecodeArgs &a, hipStream_t s);

struct TtaArgs {           // flip-TTA combine + get_max_preds + quarter-pixel refinement (misc/utils.py:19-29, 125-175; decode.hip)
    float *hm;             // (n,joints,h,w): plain pass in, average out
    const float *hm_flipped;  // the mirrored crops' heat-maps
    float *preds;          // (n,joints,2): x, y in heat-map pixels
    float *maxvals;        // (n,joints)
    int pair[kMaxJoints];  // joint j of the mirrored output is joint pair[j] (flip_back); 1 KiB of the 4-KiB kernel-argument segment
    int n, joints, h, w, post_processing;
};
hipError_t launch_tta_decode(const TtaArgs &a, hipStream_t s);

// Scoring of an evaluation batch (score.hip; include/hrnet_mi355.h: hrn_score_heatmaps, hrn_generate_targets)
struct ScoreJoint {        // one (crop, joint), prepared on the host (datasets/COCO.py:477-488)
    int mu_x, mu_y;        // centre of the Gaussian in heat-map cells; meaningful where draw != 0
    float weight;          // target_weight[i][j] as the dataset returns it (visibility, 0 off the map, times joints_weight)
    int draw;              // 1: the window [mu - t, mu + t] is drawn and meets the map; 0: the target map is all zero
};
struct ScoreArgs {
    const float *heatmaps;     // (n,J,h,w) fp32: the output maps
    const float *targets;      // maps mode: (n,J,h,w) fp32; analytic mode: nullptr
    const ScoreJoint *joints;  // n*J entries (maps mode reads `weight` only)
    const float *table;        // analytic mode: g[d2] = float32(exp(-d2 / (2 sigma^2))), d2 = 0 .. 2 t^2
    int t;                     // 3 * sigma
    int n, J, h, w;
    double *map_loss;          // (n,J)
    float *preds, *target_preds;   // (n,J,2) (x, y), zeroed where the maximum is not positive (get_max_preds)
    float *maxvals;            // (n,J)
    // the finish: scalars and the PCK
    double *loss_mse, *loss_ohkm;
    float *avg_acc, *acc, *dists;  // (), (J), (J,n)
    int *cnt;
    float pck_thr;
    int ohkm_topk;
};
hipError_t launch_score(const ScoreArgs &a, hipStream_t s);            // score_kernel<analytic | maps>, then score_finish_kernel
hipError_t launch_targets(const ScoreArgs &a, float *targets_out, hipStream_t s);   // targets_kernel: (n,J,h,w) from joints / table

// Pose overlays (draw.hip; include/hrnet_mi355.h: hrn_draw_poses).  The host uploads one table per call -- the canvases somebody
// is drawn on, the people grouped by canvas in call order, colours and skeleton -- and two launches do the rest.
constexpr int kDrawTile = 32;      // a block rasterises one 32 x 32 tile, a thread one 2 x 2 block of it (= one 4:2:0 chroma sample)
constexpr int kDrawMaxBones = 65535;
struct DrawFrame {                 // one canvas that at least one person refers to
    unsigned char *p0, *p1, *p2;   // BGR: the pixels; NV12: Y, interleaved UV; I420: Y, U, V
    int height, width, pitch0, pitch1;
    int format;                    // HRN_PIX_BGR (0), HRN_PIX_NV12 (1) or HRN_PIX_I420 (2)
    int radius;                    // of a joint's disc on this canvas (hrn_draw_labels_dev: the canvas's glyph scale)
    int tile_start, tiles_x;       // first tile of the launch that belongs to this canvas, tiles per tile row
    int person_start, person_count;   // its people: order[person_start .. + person_count), in call order
};
struct DrawArgs {
    const float *pts;              // (n, J, 3) (y, x, confidence), device: where the decode left them
    int n, J, K, Cp, nframes, total_tiles, thickness;
    float threshold;
    const DrawFrame *frames;       // nframes entries
    const int *order;              // n person indices grouped by canvas, call order kept inside a canvas
    const int *person_frame;       // n: index into frames
    const unsigned *bone_colour;   // n: the three colour bytes of the person's bones, byte 0 first
    const unsigned *point_colour;  // Cp
    const unsigned *skeleton;      // K: a | b << 16
    // written by the build launch, read by the rasteriser
    short2 *xy;                    // (n, J): truncated (x, y)
    unsigned *live;                // (n, kMaxJoints / 32): bit j = joint j is live
    int4 *box;                     // n: bounding box of the live joints grown by max(radius, ceil(T / 2)); (1, 1, 0, 0) when nobody is
};
hipError_t launch_draw(const DrawArgs &a, hipStream_t s);   // draw_build_kernel, then draw_raster_kernel

// Person labels (draw.hip; include/hrnet_mi355.h: hrn_draw_labels_dev; the arithmetic: draw_labels_math.h).  The table is
// hrn_draw_poses' -- canvases, people by canvas -- with DrawFrame::radius holding the canvas's glyph scale, and the two palettes.
struct LabelRecord;                // draw_labels_math.h
struct LabelArgs {
    const int *boxes;              // (n, 4) int32 (x1, y1, x2, y2), device: where the tracker / pre-path left them
    const int *ids;                // n int32, device, or nullptr: the colour index is i and no id is printed
    const float *scores;           // person i's score at scores[i * score_stride], device, or nullptr
    int score_stride, n, Cb, nframes, total_tiles, thickness;
    const DrawFrame *frames;       // nframes entries
    const int *order;              // n person indices grouped by canvas, call order kept inside a canvas
    const int *person_frame;       // n: index into frames
    const unsigned *colour, *text_colour;   // Cb each: three bytes, byte 0 first
    // written by the build launch, read by the rasteriser
    LabelRecord *records;          // n
    int4 *reach;                   // n: outline and plate together, corners inclusive; (1, 1, 0, 0): nothing to draw
};
hipError_t launch_draw_labels(const LabelArgs &a, hipStream_t s);   // label_build_kernel, then label_raster_kernel

// Heat-map overlays (heat.hip; include/hrnet_mi355.h: hrn_draw_heatmaps_dev; the arithmetic: heat_math.h).  The table is
// hrn_draw_poses' -- canvases, people by canvas -- and the colour table; the joint mask and the scalars travel in the arguments.
struct HeatArgs {
    const float *maps;             // (n, J, hq, wq) float32, device: where the pass left them
    const int *boxes;              // (n, 4) int32 (x1, y1, x2, y2), device
    int n, J, hq, wq, nframes, total_tiles;
    float lo, k;                   // k = 255 / (hi - lo), formed once on the host in float32
    int alpha, mode, cutoff;
    int njoints;                   // >= 1
    unsigned char joints[kMaxJoints];   // the joints that take part in the maximum, ascending (an index fits a byte)
    const DrawFrame *frames;       // nframes entries (DrawFrame::radius is unused)
    const int *order;              // n person indices grouped by canvas
    const unsigned *lut;           // 256: three bytes, byte 0 first
    unsigned char *q;              // (n, hq, wq): written by the reduce launch, read by the rasteriser
};
hipError_t launch_draw_heatmaps(const HeatArgs &a, hipStream_t s);   // heat_reduce_kernel, then heat_raster_kernel

// The face mosaic (mosaic.hip; include/hrnet_mi355.h: hrn_mosaic_dev; the arithmetic: mosaic_math.h).  The table is
// hrn_draw_poses' -- canvases, people by canvas -- with DrawFrame::radius holding the canvas's cell size, and the listed joints
// as a bit set.
struct MosaicArgs {
    const float *pts;              // (n, J, 3) (y, x, confidence), device, or nullptr: the people come from boxes
    const int *boxes;              // (n, 4) int32 (x1, y1, x2, y2), device, or nullptr
    int n, J, nframes, total_tiles;
    float threshold;
    int scale_num, scale_den, min_half;
    const DrawFrame *frames;       // nframes entries
    const int *order;              // n person indices grouped by canvas
    const int *person_frame;       // n: index into frames
    const unsigned *listed;        // kMaxJoints / 32 words: bit j = joint j is in the list
    int *status;                   // n, device, or nullptr
    int4 *region;                  // n: written by the build launch, read by the rasteriser; (0, 0, 0, 0): no region
};
hipError_t launch_mosaic(const MosaicArgs &a, hipStream_t s);   // mosaic_build_kernel, then mosaic_raster_kernel

// The tracking link (track.hip; include/hrnet_mi355.h: hrn_boxes_from_poses, hrn_preprocess_frames_dev): boxes from the joints
// where the decode left them, and the crop records of the pre-path from detections on the device -- one launch each.
struct PoseBoxArgs {
    const float *pts;              // (n, J, 3) (y, x, confidence), device
    int n, J;
    const int *frame_hw;           // per person: (n, 2) (height, width), device; nullptr: frame_h / frame_w for everybody
    int frame_h, frame_w;
    float threshold;
    int min_joints;
    double scale, min_side;
    float *dets;                   // out: (n, 5) (x1, y1, x2, y2, score)
};
hipError_t launch_pose_boxes(const PoseBoxArgs &a, hipStream_t s);   // pose_boxes_kernel: one wave per person
struct TrackFrame {                // one frame of the call's table
    const unsigned char *bgr;      // BGR frames: the pixels; YUV frames: nullptr
    int height, width;
    YuvSource yuv;                 // YUV frames: planes, pitches and coefficients
};
struct CropRecordArgs {
    const float *dets;             // (n, det_stride) float32, device
    int det_stride, n, H, W, variant, yuv;
    TrackFrame frame0;             // frame_index == nullptr: everybody's frame, in the kernel arguments (nothing is uploaded)
    const TrackFrame *frames;      // else the table and each person's entry of it, device
    const int *frame_index;
    long long slot_bytes;          // person i's intermediate lies at i * slot_bytes
    CropParams *crops;             // out: the records launch_prepath(_yuv) reads
    YuvSource *srcs;               // out (yuv != 0)
    int *boxes;                    // out: (n, 4)
    int *status;                   // out: n
};
hipError_t launch_crop_records(const CropRecordArgs &a, hipStream_t s);   // crop_records_kernel: one thread per person

// Person re-identification between two frames (assoc.hip; include/hrnet_mi355.h: hrn_associate_people_dev): similarity, optimal
// assignment, ids and smoothing of P independent problems in one launch, one block per problem (the arithmetic: assoc_math.h).
struct AssocProblem {              // one problem: n current people from cur0, m previous people from prev0
    int cur0, n, prev0, m;
    long long scratch;             // byte offset of its n * m costs (double), then n * m similarities (float), in AssocArgs::scratch
};
struct AssocArgs {
    int P, J;
    int no_assign;                 // debug (HRN_ASSOC_NO_ASSIGN): phase 2 is skipped and nobody is matched -- what the other phases cost
    AssocProblem one;              // P == 1: the problem, in the kernel arguments (nothing is uploaded)
    const AssocProblem *table;     // else P entries, device
    int *boxes;                    // (n, 4) int32, in / out
    float *pts;                    // (n, J, 3) float32, in / out
    const int *prev_boxes;
    const float *prev_pts;
    const int *prev_ids;
    int *next_id;                  // P, in / out
    double pose_alpha, similarity_threshold, smoothing_alpha;
    int *ids, *match, *status;     // out: n, n, P
    char *scratch;
};
hipError_t launch_assoc(const AssocArgs &a, hipStream_t s);   // assoc_kernel: P blocks of 256 threads
// bone[i] = palette[ids[i] mod Cb] (Python's modulo) for hrn_draw_poses_ids_dev: the ids never leave the device
hipError_t launch_bone_ids(const int *ids, int n, const unsigned *palette, int Cb, unsigned *bone, hipStream_t s);

// The person track table (tracks.hip; include/hrnet_mi355.h: hrn_track_people_dev): one update of P per-stream tables in one
// launch, one block per stream (the arithmetic: tracks_math.h over assoc_math.h).
struct TrackProblem {              // one stream: n rows from cur0
    int cur0, n;
    long long scratch;             // byte offset of its piece of TracksArgs::scratch: n * C costs (double), n * C similarities (float),
                                   // then (coast) C compared boxes (4 int32) and C * J * 3 compared joint values (float)
};
struct TracksArgs {
    int P, C, J, max_lost, coast;
    TrackProblem one;              // P == 1: the stream, in the kernel arguments (nothing is uploaded)
    const TrackProblem *table;     // else P entries, device
    int *boxes;                    // (n, 4) int32, in / out
    float *pts;                    // (n, J, 3) float32, in / out
    int *slot_id, *slot_lost, *slot_hits, *slot_row;   // (P, C), in / out
    int *slot_boxes;               // (P, C, 4), in / out
    float *slot_pts;               // (P, C, J, 3), in / out
    float *slot_vel;               // (P, C, 2), in / out
    int *next_id;                  // P, in / out
    double pose_alpha, similarity_threshold, smoothing_alpha, velocity_alpha;
    int *ids, *match_row, *slot, *status;   // out: n, n, n, P
    char *scratch;
};
hipError_t launch_tracks(const TracksArgs &a, hipStream_t s);   // tracks_kernel: P blocks of 256 threads

// Pose NMS (pose_nms.hip; include/hrnet_mi355.h: hrn_pose_nms_dev): rescoring, ordering and hard or soft OKS NMS of P independent
// problems in one launch, one block per problem (the arithmetic: pose_nms_math.h).
struct PoseNmsProblem {            // one problem: n people from `first`
    int first, n;
};
struct PoseNmsArgs {
    int P, J, flags;               // flags: HRN_POSE_NMS_SOFT | _SUPPRESS | _ENGINE
    PoseNmsProblem one;            // P == 1: the problem, in the kernel arguments (nothing is uploaded)
    const PoseNmsProblem *table;   // else P entries, device
    void *kpts;                    // COCO layout: (n, J, 3) double (x, y, score); engine layout: float (y, x, confidence), in / out
    void *areas;                   // COCO layout: n double; engine layout: (n, 4) int32 boxes, in / out
    const void *scores;            // COCO layout: n double; engine layout: n float or nullptr (1.0)
    const double *sigmas;          // J, or nullptr: COCO's 17
    double thresh, in_vis_thre, rescore_thre;
    int *keep, *num;               // out: n (kept people in selection order, then -1), P
    double *scores_out;            // out: n
    int *suppressor, *status;      // out: n, P
};
hipError_t launch_pose_nms(const PoseNmsArgs &a, hipStream_t s);   // pose_nms_kernel: P blocks of 256 threads

// Detector NMS (detector_nms.hip; include/hrnet_mi355.h: hrn_detector_nms_dev): the raw (B, N, 5 + C) output of a YOLO head to kept
// rows in two launches (the arithmetic: detector_nms_math.h).
struct DnmsCand;                   // detector_nms_math.h: one candidate, 32 bytes
constexpr int kDnmsChunk = 256;    // rows of pred per block of the scoring launch
struct DetectorNmsArgs {
    const void *pred;              // (B, N, 5 + C), float or half
    int dtype, B, N, C, rule, flags, max_candidates, max_det;
    int nchunks;                   // ceil(N / kDnmsChunk)
    float conf_thres, iou_thres;
    DnmsCand *cand;                // scratch: (B, N): chunk c of image b keeps its candidates from (b * N + c * kDnmsChunk), in row order
    int *chunk_info;               // scratch: (B, nchunks): the chunk's candidate count; bit 30: it dropped a NaN key
    int *chunk_off;                // scratch: (B, nchunks): the per-image launch's exclusive scan of the counts
    float *rows;                   // out: (B, max_det, 6 | 7)
    int *index, *counts, *status;  // out: (B, max_det), B, B
};
size_t detector_nms_lds_bytes(int max_candidates);
hipError_t launch_detector_nms(const DetectorNmsArgs &a, hipStream_t s);   // the scoring launch, then one block per image

// COCO keypoint AP / AR (keypoint_eval.hip; include/hrnet_mi355.h: hrn_keypoint_eval_dev): matching per image, the set-wide order,
// the precision / recall curves and the statistics in four launches (the arithmetic: keypoint_eval_math.h).
struct EvalImage;                  // keypoint_eval_math.h: one image's detections, people and slots
struct KeypointEvalArgs {
    int P, J, S;                   // images, joints, slots of the set
    const EvalImage *images;       // P entries, device
    const double *dt_kpts, *dt_scores, *gt_kpts, *gt_area, *gt_bbox;
    const int *gt_iscrowd;
    const double *sigmas;          // J, or nullptr: COCO's 17
    int *set_order;                // scratch, S: the slots in set order
    double *stats, *precision, *recall;   // out: 10, (3, 10, 101), (3, 10)
    int *slot_person;              // out: S
    double *slot_score;            // out: S
    int *dt_match;                 // out: (3, 10, S)
    unsigned char *dt_ignore;      // out: (3, 10, S)
    int *npig, *status;            // out: (P, 3), P
};
hipError_t launch_keypoint_eval(const KeypointEvalArgs &a, hipStream_t s);   // match (P blocks), rank (S / 256), curve (30), finish (1)

// The detector link (letterbox.hip; include/hrnet_mi355.h: hrn_letterbox_frames, hrn_detections_to_frame_dev).
enum { LB_MODE_LINEAR = 0, LB_MODE_COPY = 1, LB_MODE_AREA = 2 };   // how an interior pixel is formed (cv2.resize's three paths)
struct LetterboxFrame {            // one frame of the call, prepared on the host (letterbox_math.h's geometry)
    const unsigned char *bgr;      // BGR frames: the pixels; YUV frames: nullptr
    YuvSource yuv;                 // YUV frames: planes, pitches and coefficients
    int src_h, src_w, new_h, new_w, top, left, mode, pad_;
    double scale_x, scale_y;       // resize_scale(new, src): LB_MODE_LINEAR reads them
};
struct LetterboxArgs {
    int n, out_h, out_w, form, order, yuv;   // form = HRN_LB_*, order = HRN_LB_RGB / _BGR; yuv: 0 BGR frames, 1 YUV frames that are
                                             // all NV12 / I420 (the two-way kernel), 2 YUV frames of any of the five layouts
    unsigned char pad[4];          // pad[c] in output channel order
    LetterboxFrame one;            // n == 1: the frame, in the kernel arguments (nothing is uploaded)
    const LetterboxFrame *table;   // else n entries, device
    void *out;
};
hipError_t launch_letterbox(const LetterboxArgs &a, hipStream_t s);   // letterbox_kernel<form, source>: one launch, blockIdx.y = frame
struct DetFrame;
struct DetFilter;
struct DetArgs {
    int P, compact;
    const DetFrame *table;         // P entries, device (P == 1: `one` of the launcher's arguments instead)
    const float *dets;
    float *out;
    int *counts, *status;
};
hipError_t launch_detections_to_frame(const DetArgs &a, const DetFrame &one, const DetFilter &q, hipStream_t s);   // P blocks of 256

// Frame rotation (rotate.hip; include/hrnet_mi355.h: hrn_rotate_frames, hrn_rotate_people_dev).
constexpr int kRotTile = 64;       // elements per tile side, in destination coordinates
constexpr int kRotRows180 = 16;    // ... but 64 x 16 at 180 degrees: one four-element group per thread
struct RotPlane {                  // one plane of one frame of the call: BGR 1, NV12 2 (Y; the UV pairs), I420 3
    const unsigned char *src;
    unsigned char *dst;
    int hs, ws;                    // the SOURCE plane, in elements
    int es;                        // bytes per element: 1 (Y, U, V), 2 (NV12's UV pair), 3 (a BGR pixel)
    int code;                      // HRN_ROTATE_*
    int spitch, dpitch;            // bytes between rows
    int tile_start, tiles_x;       // the plane's first tile of the launch; tiles per row of tiles of the DESTINATION
};
struct RotArgs {
    int nplanes, total_tiles;
    RotPlane one[3];               // table == nullptr: the planes of the call's only frame, in the kernel arguments
    const RotPlane *table;         // else nplanes entries, device
};
hipError_t launch_rotate(const RotArgs &a, hipStream_t s);   // rotate_kernel: total_tiles blocks of 256 threads
struct RotPeopleArgs {
    int n, J, hs, ws, code;        // hs, ws, code: for everybody, where the per-person array is null
    const int *frame_hw, *codes;   // (n, 2) / n on the device, or nullptr
    const float *pts;              // (n, J, 3) or nullptr
    const int *boxes;              // (n, 4) or nullptr
    float *pts_out;
    int *boxes_out;
};
hipError_t launch_rotate_people(const RotPeopleArgs &a, hipStream_t s);   // one thread per joint and per box

// BGR frames to 4:2:0 YCbCr frames (yuv_out.hip; include/hrnet_mi355.h: hrn_bgr_to_yuv_frames; the arithmetic: yuv_fwd.h).
constexpr int kYuvOutTileW = 256;  // pixels per tile row: 64 groups of 4 pixels, one wavefront wide
constexpr int kYuvOutTileH = 8;    // rows per tile: 4 groups of 2 rows
struct YuvOutFrame {               // one frame of the call
    const unsigned char *src;      // (height, width, 3) BGR, rows spitch bytes apart
    unsigned char *y, *u, *v;      // the destination's planes (v: I420 / I010 only)
    int height, width;             // even
    int spitch, pitch_y, pitch_c;  // bytes between rows
    int format;                    // HRN_PIX_NV12 / _I420 / _NV21 / _P010 / _I010
    int tile_start, tiles_x;       // the frame's first tile of the launch; tiles per row of tiles
    int coef[10];                  // yuv_fwd.h's table of the destination's matrix and range
};
struct YuvOutArgs {
    int nframes, total_tiles;
    YuvOutFrame one;               // table == nullptr: the call's only frame, in the kernel arguments
    const YuvOutFrame *table;      // else nframes entries, device
};
hipError_t launch_bgr_to_yuv(const YuvOutArgs &a, hipStream_t s);   // bgr_to_yuv_kernel: total_tiles blocks of 256 threads

// Joints over time (temporal.hip; include/hrnet_mi355.h: hrn_filter_poses_dev): the One-Euro filter and the motion lookahead of
// every joint of the call in one launch, one thread per (person, joint) (the arithmetic: temporal_math.h).
struct TemporalParams;
struct TemporalSegment {           // where one current person's previous people lie: m of them from prev0
    int prev0, m;
};
struct TemporalArgs {
    int J, first, total;           // people first .. of the arrays; total = people * J threads
    TemporalSegment one;           // table == nullptr: everybody's segment, in the kernel arguments (nothing is uploaded)
    const TemporalSegment *table;  // else one entry per person of the call, device
    const float *pts;              // (n, J, 3)
    const int *match;              // n, or nullptr: nobody has a prior
    const float *prev_state;       // (m, J, 6)
    const int *prev_age;           // (m, J)
    float *pts_out, *pred_out;     // (n, J, 3); pts_out may be pts, pred_out may be nullptr
    float *state;                  // out: (n, J, 6)
    int *age;                      // out: (n, J)
};
hipError_t launch_temporal(const TemporalArgs &a, const TemporalParams &prm, hipStream_t s);   // temporal_kernel: 256-thread blocks

struct TapArgs {           // debug tap: crops crop0, crop0 + crop_step, ... of a flat padded tensor -> (ncrops, c, h, w) fp32
    const void *in;
    float *dst;
    int c, h, w, wp, hpwp, crop0, ncrops, crop_step;
};
hipError_t launch_tap(int dtype, const TapArgs &a, hipStream_t s);

struct PadCheckArgs {      // debug: one workspace buffer (guard rows + nmax images of (h + 1) x (w + 1) rows of c channels)
    const void *buf;       // allocation start (NOT row 0 of image 0)
    unsigned long long *count;
    long rows, lead_rows;  // rows of the buffer, guard rows in front of image 0
    int c, h, w, wp, hpwp, nmax;
};
hipError_t launch_pad_check(int dtype, const PadCheckArgs &a, hipStream_t s);

hipError_t launch_conv(int dtype, const ConvArgs &a, int nr, hipStream_t s);
// grouped launch of the generic kernel: device-resident ConvArgs[], block map entries (prob | cout tile << 8, M tile)
hipError_t launch_conv_group(int dtype, const ConvArgs *probs_dev, const void *map_dev, int nblocks, int nr, int mr, int wlds,
                             hipStream_t s);
hipError_t launch_conv3x3_lds(int dtype, const Conv3Problem *probs_dev, const void *blockmap_dev, int nblocks, int nb, int ks,
                              int nrb, hipStream_t s);
hipError_t launch_stem(int dtype, const StemArgs &a, hipStream_t s);
hipError_t launch_fuse(int dtype, const FuseArgs &a, hipStream_t s);
hipError_t launch_head(int dtype, const HeadArgs &a, hipStream_t s);

// rows per block of the conv kernels: buffers keep this many guard rows after the last image
// -- and the longest slab a compact tile of the 96-cout form may read past the last image (a last tile that holds a single
// real pixel still stages its whole slab, up to conv3x3_n96_max_rows() = 700 rows; a flat tile reads at most 512 + halo)
constexpr int kConvBlockRows = 704;

}  // namespace hrn
