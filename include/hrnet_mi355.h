/*
 * hrnet_mi355.h -- C ABI of the MI355X-native HRNet pose-inference hot path.
 *
 * This is the drop-in boundary behind SimpleHRNet.predict() of stefanopini/simple-HRNet.
 * The reference has no native interface on this path: the seam is the Python attribute
 * `self.model`, invoked as `self.model(images)` (SimpleHRNet.py:284-294, 419-429) and already
 * swapped for a foreign engine by the reference itself (TRTModule, SimpleHRNet.py:143-147);
 * the closest native precedent is `void _nms(int*, int*, const float*, int, int, float, int)`
 * (misc/nms/gpu_nms.hpp:1).  Every entry point below names the reference behaviour it replaces.
 *
 * Conventions
 *   - plain C types only: raw pointers + sizes; no torch / HIP types in signatures
 *     (`stream` is a hipStream_t passed as void*, NULL = the default stream);
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from hrn_last_error() (the reference raises Python exceptions:
 *     SimpleHRNet.py:107,114,139,210 -- the ctypes shim turns our codes back into them);
 *   - a handle is bound to one GPU; it is not thread-safe, distinct handles are;
 *   - all work is stream-ordered on `stream`; nothing allocates inside hrn_forward().  A handle has ONE workspace: calls
 *     on different streams are serialised on the device by the handle itself (a call on another stream than the previous
 *     one first waits for that one's last kernel) -- concurrency comes from several handles, not from several streams;
 */
#ifndef HRNET_MI355_H
#define HRNET_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hrn_ctx *hrn_handle;

enum { HRN_F32 = 0, HRN_BF16 = 1, HRN_F16 = 2 }; /* arithmetic / activation storage type: fp32,
                                                  bf16 or fp16 storage (fp32 accumulation);
                                                  HRN_F16 runs the bf16 plan and kernels  */
enum { HRN_BOX_I32 = 0, HRN_BOX_F32 = 1 };     /* boxes dtype: SimpleHRNet.py:230 vs :223      */
enum { HRN_T_F32 = 0, HRN_T_I64 = 1 };         /* hrn_tensor_desc.dtype                        */

/* One state_dict entry, exactly as `torch.load(checkpoint)` yields it
 * (SimpleHRNet.py:117-121): name, shape, contiguous host data (conv weights OIHW fp32). */
typedef struct {
    const char *name;
    const void *data;
    int32_t ndim;
    int64_t dims[4];
    int32_t dtype;
} hrn_tensor_desc;

/* Static description of one convolution of the compiled graph (for tests / tooling). */
typedef struct {
    char name[96];        /* state_dict prefix of the conv, e.g. "stage3.1.branches.2.0.conv1" */
    int32_t cin, cout, ksize, stride, relu, has_residual;   /* ksize 2 = one phase of a ConvTranspose2d(4, s2, p1) */
    int32_t in_h, in_w, out_h, out_w;
    int32_t kpad;         /* K = ksize*ksize*cin rounded up to the MFMA K-chunk                 */
    int32_t nr;           /* 16-wide cout fragments per group (packing parameter)              */
    int32_t algo;         /* 0 generic MFMA kernel, 1 pipelined LDS-staged 3x3 stride-1 kernel, 2 = 1 as half of a fused BasicBlock (HRN_BBF=1), 3 = the 96-cout form of 1 (ks 32, nr 6), 4 = generic plan + the stride-2 slab kernel (conv_s2.hip) for calls large enough */
    int32_t ks;           /* algo 1: input channels per LDS slice (k = tap*ks + ci inside one)  */
    int64_t w_offset;     /* byte offset of the packed weights in the blob                     */
    int64_t w_bytes;
    int64_t b_offset;     /* byte offset of the folded fp32 bias                                */
    double flops;         /* 2*MAC per crop                                                    */
} hrn_conv_info;

/* Largest nof_joints a handle takes (COCO 17, face 68 / 98 / 106, COCO-WholeBody 133, Halpe 136 ...).  The head works the
 * joints in groups of 32 (two 16-row MFMA fragments); the bound is the size of flip-TTA's pair table, a kernel argument.
 * Two invariants hold for every nof_joints in [1, HRN_MAX_JOINTS], in all three dtypes:
 *   1. A joint's numbers do not depend on how many other joints the model has: its heat-map value is the same dot
 *      product in the same K order plus its bias, and its arg-max follows the same order (first maximum; a NaN is a
 *      maximum), whether it is one of 17 or of 133 -- a model holding only rows [32g, 32g + 32) of final_layer returns the
 *      bits of those joints of the full model.
 *   2. For nof_joints <= 32 the head is one group: the same kernels, grid, weight blob, launches per pass and bits as a
 *      build without groups.
 * The tail of the weight blob is final_layer: [nof_joints][c] fp32 weights, nof_joints fp32 biases, then (each padded to
 * 256 bytes) the MFMA image, ceil(nof_joints / 32) groups of [2 fragments][ceil(c / 32) chunks][64 lanes][8 x 16 bit],
 * group g = joints 32g .. 32g + 31 exactly as a head of those joints alone packs them, rows past the last joint zero.
 * Cost at large J: a refined decode without caller heat-maps, and flip-TTA, keep max_batch * nof_joints * (H/4) * (W/4)
 * fp32 of scratch in the handle, allocated on first use (256 x 133 x 96 x 72: 940 MB); size max_batch accordingly. */
#define HRN_MAX_JOINTS 256

/* Replaces `HRNet(c, nof_joints)` + `.to(device).eval()` (SimpleHRNet.py:110,141-142; graph of
 * models_/hrnet.py:75-155).  nof_joints in [1, HRN_MAX_JOINTS].  height/width = network input resolution (multiples of 32),
 * max_batch = largest micro-batch one internal pass will process (workspace is sized for it;
 * hrn_forward accepts any n and chunks internally like SimpleHRNet.py:285-294).
 * device_id >= 0: HIP device.  device_id < 0: plan-only handle (no GPU touched; graph,
 * folding and packing run on the host so the host logic is testable on a CPU-only box;
 * hrn_forward fails on such a handle -- there is NO CPU compute path). */
int hrn_create(hrn_handle *out, int c, int nof_joints, int height, int width, int dtype, int max_batch,
               int device_id);

/* The other model SimpleHRNet offers (model_name='PoseResNet', SimpleHRNet.py:111-112; models_/poseresnet.py:16-122):
 * c is then the ResNet size (50 / 101 / 152).  hrn_create(...) == hrn_create_model(HRN_MODEL_HRNET, ...).
 * Everything else of the interface is model independent. */
enum { HRN_MODEL_HRNET = 0, HRN_MODEL_POSERESNET = 1 };
int hrn_create_model(hrn_handle *out, int model, int c, int nof_joints, int height, int width, int dtype, int max_batch,
                     int device_id);
void hrn_destroy(hrn_handle h);
const char *hrn_last_error(hrn_handle h); /* h may be NULL: error of the last failed hrn_create */

/* Replaces `model.load_state_dict(checkpoint)` (SimpleHRNet.py:117-121).  Folds every
 * (conv, BatchNorm) pair (eps 1e-5), repacks to the MFMA fragment layout and uploads.
 * 16-bit handles store the folded weights rounded to nearest even (biases stay fp32); an HRN_F16 handle fails
 * when a folded weight exceeds 65504 in magnitude (no fp16 representation) instead of storing inf.
 * The blob of an HRN_F16 handle has the bf16 handle's layout and size, not its bytes: ranks of one job must
 * share the dtype (dist.ShardedHRNet checks it before the broadcast). */
int hrn_load_weights(hrn_handle h, const hrn_tensor_desc *descs, int n);

/* Multi-GPU weight distribution (replaces DataParallel's per-forward `replicate`,
 * SimpleHRNet.py:135): the packed blob is one contiguous device buffer that rank 0 fills via
 * hrn_load_weights and the other ranks receive by ONE RCCL broadcast, then adopt. */
int64_t hrn_weight_blob_bytes(hrn_handle h);
void *hrn_weight_blob_ptr(hrn_handle h);            /* device pointer (host pointer if plan-only) */
int hrn_adopt_weights(hrn_handle h);                /* mark an externally filled blob as loaded   */
int hrn_weight_blob_read(hrn_handle h, int64_t offset, void *dst_host, int64_t nbytes);

/* Replaces the model call + decode loop, SimpleHRNet.py:281-308 (dup. 416-443):
 *   images_dev  (n,3,H,W) fp32 NCHW device pointer -- what SimpleHRNet hands to self.model
 *   boxes_dev   (n,4) [x1,y1,x2,y2] device pointer, int32 or fp32 per box_dtype; may be NULL
 *               when pts_dev is NULL
 *   pts_dev     (n,joints,3) fp32 device pointer (y, x, confidence) or NULL
 *   heatmaps_dev (n,joints,H/4,W/4) fp32 NCHW device pointer or NULL (return_heatmaps,
 *               and the level-1 "self.model(images)" seam)
 * At least one of pts_dev / heatmaps_dev must be non-NULL. */
int hrn_forward(hrn_handle h, const void *images_dev, int n, const void *boxes_dev, int box_dtype, float *pts_dev,
                float *heatmaps_dev, void *stream);

/* Crop pre-path of the single-image multi-person branch (SimpleHRNet.py:236-278): for each
 * detector box -- round, correct the aspect ratio by padding (:243-272), slice the BGR frame as RGB (:274), zero-pad
 * (:276), Resize((H,W)) with Pillow's antialiased bilinear filter, ToTensor, Normalize (:167-172) -- written straight
 * into the (n,3,H,W) fp32 batch hrn_forward reads.  Bit-identical to the reference's transform.
 *   frame_dev   (frame_h, frame_w, 3) uint8 BGR, device
 *   dets_host   (n, det_stride) float32 on the HOST, columns 0..3 = x1,y1,x2,y2 as the detector returns them
 *   images_dev  out: (n,3,H,W) float32, device
 *   boxes_host  out: (n,4) int32 [x1,y1,x2,y2] = the padded boxes the decode scales by (may be NULL)
 *   boxes_dev   out: the same on the device, ready for hrn_forward(..., HRN_BOX_I32, ...) (may be NULL)
 *   variant     HRN_CROP_PAD (0): single-image path, aspect ratio corrected by zero padding (:243-276);
 *               HRN_CROP_CLAMP (1): the batch path's enlarge-and-clamp, no padding (SimpleHRNet.py:383-412) -- call once
 *               per image of the stack
 * Boxes must lie inside the frame after rounding (the detector wrappers clamp them: YOLOv3.py:49-56) and be
 * non-degenerate; otherwise the call fails (the reference would wrap around / divide by zero). */
enum { HRN_CROP_PAD = 0, HRN_CROP_CLAMP = 1 };
int hrn_preprocess_frame(hrn_handle h, const uint8_t *frame_dev, int frame_h, int frame_w, const float *dets_host,
                         int det_stride, int n, int variant, float *images_dev, int32_t *boxes_host, int32_t *boxes_dev,
                         void *stream);

/* Crop pre-path for the people of MANY frames in one call: the multi-frame form of hrn_preprocess_frame.  Replaces the
 * per-image loop of the stack path, SimpleHRNet.py:383-412 (HRN_CROP_CLAMP: one call instead of one hrn_preprocess_frame per
 * image of the stack plus the `torch.cat` of :409-412 -- the crops are written once, where the model reads them), and the
 * same loop around :236-278 (HRN_CROP_PAD) that scripts/extract-keypoints.py:88-123 runs frame after frame over a video file.
 * One pair of launches cuts, pads, resizes and normalises every person; the frames may differ in size.
 *   frames_host       nframes entries on the HOST: device pointer of a contiguous (height, width, 3) uint8 BGR frame and its size;
 *                     a frame nobody refers to may be null
 *   dets_host         (n, det_stride) float32 on the HOST, as hrn_preprocess_frame
 *   frame_index_host  n entries on the HOST: person i is cut from frames_host[frame_index_host[i]]; people come in any order
 *                     and the outputs keep the given order.  NULL: nframes == 1, everybody is cut from that frame
 *   images_dev / boxes_host / boxes_dev / variant   as hrn_preprocess_frame; any n (not bounded by max_batch)
 * Person for person the arithmetic, and so every bit of the result, is hrn_preprocess_frame's on that person's frame: both
 * entries run the same two kernels, hrn_preprocess_frame with a one-frame table.
 * Fails with code 7 and nothing launched on: a variant other than HRN_CROP_PAD / HRN_CROP_CLAMP; n < 0, det_stride < 4 or a
 * null table / detections / output; a frame index outside [0, nframes); a frame a person refers to that is null or has a
 * non-positive side; a plan-only handle; a detection that is degenerate, starts outside its frame, or is degenerate after
 * clamping (the three failures of hrn_preprocess_frame, with its texts).  The arguments are judged before the handle's device
 * is touched, so a plan-only handle reports a bad index or table as such. */
typedef struct { const uint8_t *data; int32_t height, width; } hrn_frame;   /* device pointer, (height, width, 3) uint8 BGR, contiguous */
int hrn_preprocess_frames(hrn_handle h, const hrn_frame *frames_host, int nframes, const float *dets_host, int det_stride,
                          const int32_t *frame_index_host /* n entries; NULL: nframes == 1 */, int n, int variant,
                          float *images_dev, int32_t *boxes_host, int32_t *boxes_dev, void *stream);

/* The crop pre-path from VIDEO frames as decoders deliver them: 4:2:0 YCbCr, 8 bits, NV12 (a Y plane and one plane of
 * interleaved U, V pairs) or I420 (Y, U and V planes), each plane with a row pitch in bytes.  The frame crosses PCIe at 1.5 bytes
 * per pixel, or not at all when a decoder left it on the device, and is never converted as a whole: the horizontal pass reads
 * every tap through the conversion.
 *
 * The conversion is cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420)'s form: the chroma sample of a 2x2 block is shared by its four
 * pixels (nearest, no interpolation), 20-bit fixed point in int32 with an arithmetic shift:
 *   yy = max(0, Y - y0) * CY;  u = U - 128;  v = V - 128;  h = 1 << 19
 *   B = clip8((yy + h + CUB*u) >> 20);  G = clip8((yy + h + CVG*v + CUG*u) >> 20);  R = clip8((yy + h + CVR*v) >> 20)
 * hrn_yuv_coefficients writes (y0, CY, CUB, CUG, CVG, CVR) of a matrix and a range; it needs no handle and no GPU.  BT.601
 * limited -- the default of every video source that says nothing else -- is OpenCV's published table verbatim
 * (16, 1220542, 2116026, -409993, -852492, 1673527); the other three are floor(x * 2^20 + 0.5) of the exact coefficients
 * (Kr / Kb = 0.299 / 0.114 or 0.2126 / 0.0722; luma x 255/219 and chroma x 255/224 for limited range, y0 = 16; both 1 and
 * y0 = 0 for full range).  No sum leaves int32 for any byte triple.
 * PINNED: the kernels equal the numpy restatement of these lines (tests/yuv_ref.py) bit for bit, and crops cut from a YUV
 * frame equal the BGR path's crops of that restatement's BGR frame bit for bit, images and boxes.  The restatement is within
 * one grey level of the rounded float64 formula for all 2^24 byte triples.  UNPINNED: equality with a cv2 build, which is not
 * available where this library is tested (tests/golden/make_yuv_golden.py makes the pin wherever opencv-python is installed).
 *
 * hrn_yuv_to_bgr converts a whole frame to contiguous (height, width, 3) uint8 BGR on the device, for the consumer that needs
 * BGR (the detector), so that the frame still crosses PCIe once.
 * hrn_preprocess_frames_yuv is hrn_preprocess_frames over a table of such frames: the same contract, word for word -- box
 * arithmetic (hrn_crop_geometry's), staging, any n, outputs, failure codes and texts; padding is zero AFTER the conversion
 * (RGB 0, not the conversion of YUV 0).  The people of one call come all from YUV frames or all from BGR frames.
 * Both fail with code 7 and nothing launched, beyond hrn_preprocess_frames' failures, on a frame (that a person refers to)
 * with: an unknown format, matrix or range; an odd or non-positive width or height; pitch_y < width; pitch_c < width (NV12)
 * or < width / 2 (I420); a null plane (y, u; v for I420).  Everything is judged before the device is touched, so a plan-only
 * handle reports argument errors as such and a good call as "plan-only".
 *
 * THREE MORE LAYOUTS, through the same entries (these two, hrn_preprocess_frames_yuv_dev, hrn_letterbox_frames_yuv and
 * hrn_rotate_frames; frames of all five layouts may share a call).  Value 3 is unassigned and stays "unknown".
 *   HRN_PIX_NV21 (4)  8-bit; a Y plane and one plane of interleaved (V, U) pairs (ffmpeg nv21, Android cameras).  NV12's
 *                     arithmetic with V = pair[0], U = pair[1]; validated as NV12.
 *   HRN_PIX_P010 (5)  10-bit; 16-bit little-endian words, the sample in the TOP 10 bits (s = word >> 6; the low six bits are
 *                     ignored, whatever they hold); a Y plane and one plane of interleaved (U, V) words (p010le: what a
 *                     hardware decoder delivers for 10-bit HEVC / AV1).
 *   HRN_PIX_I010 (6)  10-bit; 16-bit little-endian words, the sample in the LOW 10 bits (s = word & 1023; the high six bits are
 *                     ignored); Y, U and V planes (yuv420p10le: what a software decoder delivers).
 * Pitches stay in BYTES.  10-bit planes are read as aligned 16-bit words: pitch_y >= 2 * width; pitch_c >= 2 * width (P010)
 * or >= width (I010); every plane address and both pitches even -- otherwise code 7, nothing launched, the text naming "odd
 * plane address or pitch on a 10-bit frame".
 * A 10-bit triple becomes 8-bit B, G, R through the SAME table, in exact integers, with one rounding from the 10-bit samples:
 *   yy = max(0, Y - 4*y0) * CY;  u = U - 512;  v = V - 512;  h = 1 << 21
 *   B = clip8((yy + h + CUB*u) >> 22);  G = clip8((yy + h + CVG*v + CUG*u) >> 22);  R = clip8((yy + h + CVR*v) >> 22)
 * (arithmetic shift; one chroma sample per 2x2 block).  These sums do NOT fit int32 -- BT.709 limited: yy + h + CUB*u reaches
 * 2 304 855 561 -- and are evaluated in 64 bits.  PINNED (tests/yuv10_ref.py, tests/test_yuv10_*.py): for samples that are
 * multiples of 4 the result equals the 8-bit conversion of s / 4 bit for bit (every term scales by 4), so a P010 frame made from
 * an NV12 frame by << 8 converts and crops to the same bits; the form is within one grey level of clip(rint(float64 formula));
 * the kernels equal the numpy restatement bit for bit.  HDR transfer functions (PQ / HLG) and BT.2020 are not offered: such content
 * goes through the chosen matrix as it is.  The output of every entry stays 8-bit. */
enum { HRN_PIX_NV12 = 1, HRN_PIX_I420 = 2, HRN_PIX_NV21 = 4, HRN_PIX_P010 = 5, HRN_PIX_I010 = 6 };
enum { HRN_YUV_BT601 = 0, HRN_YUV_BT709 = 1 };
enum { HRN_YUV_LIMITED = 0, HRN_YUV_FULL = 1 };
typedef struct { const uint8_t *y, *u, *v;     /* device; NV12 / NV21 / P010: u = the interleaved chroma plane, v ignored */
                 int32_t height, width, pitch_y, pitch_c, format, matrix, range; } hrn_yuv_frame;
int hrn_yuv_coefficients(int matrix, int range, int32_t out[6]);
int hrn_yuv_to_bgr(hrn_handle h, const hrn_yuv_frame *frame_host, uint8_t *bgr_dev, void *stream);
int hrn_preprocess_frames_yuv(hrn_handle h, const hrn_yuv_frame *frames_host, int nframes, const float *dets_host,
                              int det_stride, const int32_t *frame_index_host, int n, int variant,
                              float *images_dev, int32_t *boxes_host, int32_t *boxes_dev, void *stream);

/* The box arithmetic of the two entries above on the HOST, without a handle or a GPU: per detection -- round (half to even),
 * correct the aspect ratio to height / width (SimpleHRNet.py:243-272 by padding, HRN_CROP_PAD; :396-407 by enlarging and
 * clamping to the frame, HRN_CROP_CLAMP), slice as numpy does (:274, :408).
 *   frame_hw       (n, 2) int32 (height, width) of each person's frame when per_person_hw != 0, else (1, 2) for all
 *   height, width  the network's input size
 *   boxes_out      (n, 4) int32 [x1,y1,x2,y2]: the boxes the decode scales by (may be NULL)
 *   slice_out      (n, 8) int32: x1, y1, w_crop, h_crop = the part of the frame that is read; pad_top, pad_left = zero rows /
 *                  columns in front of it; h_pad, w_pad = the size of the padded crop, the resize's input (may be NULL)
 * Returns 0, or 7 with hrn_crop_geometry_last_error() (per thread) = "detection i is degenerate", "detection i starts outside
 * the frame", "detection i is degenerate after clamping", "variant must be HRN_CROP_PAD or HRN_CROP_CLAMP" or
 * "bad frame / detections / n"; outputs of the detections before the failing one are written. */
int hrn_crop_geometry(const float *dets, int det_stride, int n, const int32_t *frame_hw /* (n,2) or (1,2) */, int per_person_hw,
                      int height, int width, int variant, int32_t *boxes_out /* (n,4) */,
                      int32_t *slice_out /* (n,8): x1,y1,w_crop,h_crop,pad_top,pad_left,h_pad,w_pad */);
const char *hrn_crop_geometry_last_error(void);

/* ---- the tracking link: people followed between two detector runs, on the device ----
 * A top-down video pipeline runs its detector on every K-th frame only and, in between, cuts the next frame's crops from the
 * previous frame's joints.  The two parts below make that chain -- pts(k) -> boxes -> crop records -> crops(k+1) -> pass ->
 * pts(k+1) -- run on the device, stream-ordered, with no host read in between.  What is PINNED is that the chain equals, bit for
 * bit, the host composition it replaces (download pts, hrn_pose_boxes, hrn_preprocess_frames with host detections); how well
 * such boxes track on a trained network is not claimed.
 *
 * 1. Boxes from joints.  pts (n, J, 3) float32 (y, x, confidence) as hrn_forward writes them; each person's frame (height, width).
 * Joint j is LIVE iff confidence > threshold (a float32 compare: equality and NaN are not live) and y and x are finite; a live
 * coordinate enters as (double)v + 0.0 (no negative zero).  nlive < min_joints: the row is five zeros.  Otherwise, in double and in
 * this order (no contraction):
 *     xmin, xmax, ymin, ymax over the live joints;  cx = (xmin + xmax) * 0.5;  w = max((xmax - xmin) * scale, min_side);
 *     x1 = max(0, cx - w * 0.5);  x2 = min(frame_w, cx + w * 0.5);  y likewise with frame_h;
 *     score = (sum of the live confidences, as doubles, in joint order) / nlive
 * (max(a, b) = a > b ? a : b, min(a, b) = a < b ? a : b: a zero result is +0), each of the five rounded once to float32.  The
 * row (x1, y1, x2, y2, score) is a detection row as the detector wrappers return them: det_stride 5.  scale = 1.25 is the factor
 * of the datasets' _box2cs.  A box lies inside its frame unless every live joint lies on one side of it (then x2 < x1 or
 * y2 < y1: a degenerate detection, status 1 below).  tests/pose_boxes_ref.py restates the definition in numpy float64.
 *   frame_hw   (n, 2) int32 (height, width) per person when per_person_hw != 0, else (1, 2) for everybody; HOST in both entries
 *   threshold  float32; min_joints >= 1; scale finite and > 0; min_side finite and >= 0
 * hrn_pose_boxes is the host form: no handle, no GPU (pts and dets_out on the host); 0, or 7 with hrn_pose_boxes_last_error()
 * (per thread) naming the argument.  hrn_boxes_from_poses is ONE launch, one wave per person, over pts_dev where the decode left
 * them, into dets_dev (n, 5) float32 on the device; both compile one function text (csrc/track_geometry.h).  n == 0 succeeds and
 * launches nothing.  Fails with code 7 and nothing launched, naming the cause, on: n < 0; J outside [1, HRN_MAX_JOINTS];
 * min_joints < 1; a non-finite or non-positive scale; a negative or non-finite min_side; null tables (n > 0); a non-positive
 * frame side; and, after these, a plan-only handle. */
int hrn_pose_boxes(const float *pts /* (n,J,3) */, int n, int J, const int32_t *frame_hw /* (n,2) or (1,2) */, int per_person_hw,
                   float threshold, int min_joints, double scale, double min_side, float *dets_out /* (n,5) */);
const char *hrn_pose_boxes_last_error(void);
int hrn_boxes_from_poses(hrn_handle h, const float *pts_dev, int n, int J, const int32_t *frame_hw_host /* (n,2) or (1,2) */,
                         int per_person_hw, float threshold, int min_joints, double scale, double min_side,
                         float *dets_dev /* (n,5) */, void *stream);

/* 2. The crop pre-path from detections ON THE DEVICE.  hrn_preprocess_frames_dev / _yuv_dev follow the contract of
 * hrn_preprocess_frames / _yuv with these differences: dets_dev (n, det_stride) float32 lies on the device (det_stride >= 4);
 * there is no boxes_host; boxes_dev (n, 4) int32 and status_dev (n) int32 are required.  The frame table and frame_index_host stay
 * on the host: which frame a person belongs to is known without reading the device.
 * A record kernel, one thread per person, runs hrn_crop_geometry's arithmetic (the same function text, csrc/track_geometry.h)
 * and writes the crop record the host path would have uploaded; the horizontal and vertical kernels of the host-detection path
 * then run unchanged on those records, so images and boxes equal hrn_preprocess_frames' bit for bit.
 * SCRATCH.  The host sizes grid and scratch without knowing the boxes: with hcap(frame) = max(frame_h, ceil(H * frame_w / W)) + 2
 * rows -- what a box inside the frame can need -- and hcap = the maximum over the frames people refer to (at least H), person i's
 * intermediate lies at i * roundup(hcap * W * 3, 256): n * hcap * W * 3 bytes, about 2.2 MB per person at 1080p / 384x288 (the
 * host-detection path allocates what the boxes need, usually much less).  It is kept by the handle and grown on demand.
 * STATUS.  A person cannot make a stream-ordered call fail, so the call reports it in status_dev:
 *     0  ok
 *     1  degenerate                                  }
 *     2  starts outside the frame                    }  the three refusals of hrn_preprocess_frames, with its predicates
 *     3  degenerate after clamping (HRN_CROP_CLAMP)  }
 *     4  padded crop taller than hcap of its frame (HRN_CROP_PAD; cannot happen for a box inside its frame, which every box of
 *        hrn_boxes_from_poses is)
 *     5  a coordinate that is not finite or exceeds 2^30 in magnitude (judged first)
 * A five-zero row of part 1 gives status 1.  A person with status != 0 gets box (0, 0, 0, 0) and the all-padding crop -- an empty
 * slice, h_pad = H, w_pad = W: Normalize(0) per channel; its neighbours are untouched, and its joints after the pass are
 * meaningless, which the status says.  The padded WIDTH is not bounded, as in the host path: the cost of a crop grows with it.
 * Argument errors are code 7, judged before the device is touched, word for word those of the host-detection entries minus the
 * per-detection ones ("bad frames / detections / n" covers the null outputs); then a plan-only handle.  n == 0 launches nothing. */
int hrn_preprocess_frames_dev(hrn_handle h, const hrn_frame *frames_host, int nframes, const float *dets_dev, int det_stride,
                              const int32_t *frame_index_host /* n entries; NULL: nframes == 1 */, int n, int variant,
                              float *images_dev, int32_t *boxes_dev, int32_t *status_dev, void *stream);
int hrn_preprocess_frames_yuv_dev(hrn_handle h, const hrn_yuv_frame *frames_host, int nframes, const float *dets_dev,
                                  int det_stride, const int32_t *frame_index_host, int n, int variant, float *images_dev,
                                  int32_t *boxes_dev, int32_t *status_dev, void *stream);

/* ---- person ids between two frames: association, smoothing and numbering, on the host and on the device ----
 * What the demo loop does after every frame (scripts/live-demo.py:114-130): find_person_id_associations (misc/utils.py:387-429)
 * decides who of the previous frame is who of this one, carries the ids over, smooths matched boxes and joints and numbers the new
 * people; then next_id = max(next_id, max(ids) + 1).  Both entries solve P independent problems (one video: P = 1; the streams of
 * a camera wall: one problem each): problem p has the current people [cur_start[p], cur_start[p + 1]) and the previous people
 * [prev_start[p], prev_start[p + 1]) of the arrays below.  The arithmetic is csrc/assoc_math.h's, one text for both entries
 * (its header states every expression and its rounding): box IoU and OKS as hrn_pose_similarity computes them, except that exp is
 * the header's own (at most 1 ulp from libm's on [-29, 0], measured; host and device agree to the bit); the float32 blend
 * sim_pose * f32(pose_alpha) + sim_box * f32(1 - pose_alpha); cost (double)(1.0f - sim); hrn_assignment's matching (ties go to the
 * lowest column); a matched pair is ACCEPTED iff sim > f32(similarity_threshold); an accepted person takes the previous id and,
 * when smoothing_alpha != 0, joints f32(1 - a) * now + f32(a) * before (float32, all three components) and box
 * (1 - a) * now + a * before in fp64 truncated towards zero; everybody whose id is then -1 is numbered in index order from
 * next_id[p].  A NON-FINITE blended similarity (two zero boxes: IoU 0 / 0) counts as 0 in the cost and is never accepted.
 *   cur_start, prev_start  P + 1 int32 each, non-decreasing, on the HOST in both entries (counts are shapes: known without a read)
 *   boxes      (n, 4) int32 (x1, y1, x2, y2), in / out        pts       (n, J, 3) float32 (y, x, confidence), in / out
 *   prev_boxes, prev_pts, prev_ids (int32)                    the previous frame; must not overlap the current arrays
 *   next_id    P int32, in / out (a problem with nobody in the current frame leaves it)
 *   pose_alpha, similarity_threshold  finite;  smoothing_alpha in [0, 1]
 *   ids        n int32 out;   match  n int32 out: the accepted previous person, counted from prev_start[p], or -1
 *   status     P int32 out: 0 clean; bit 0: a non-finite similarity was replaced; bit 1: the assignment found no path (nobody
 *              matched; cannot happen while every cost is finite)
 * At most HRN_MAX_TRACKED people on either side of one problem and J in [1, HRN_MAX_JOINTS]: more is code 7, like every other
 * argument error (null tables, a decreasing segment table, parameters out of range), judged before anything is written;
 * hrn_associate_people_last_error() (per thread) / hrn_last_error(h) names it.
 * hrn_associate_people is the host form: no handle, no GPU.  hrn_associate_people_dev has every array except the two segment
 * tables in device memory: ONE launch, one 256-thread block per problem (similarities by all threads, the assignment by one wave,
 * ids and smoothing by the block), stream-ordered, no host read; its results equal the host form's bit for bit.  It keeps
 * 12 * n * m bytes of scratch per problem in the handle (at most 768 KiB), grown on demand.  For P > 1 the problem table goes
 * through one upload; P == 1 uploads nothing.  P == 0 launches nothing.
 * hrn_assoc_exp (no GPU): the header's exp of n doubles, for measuring it.  hrn_associate_similarity (no GPU): the (n, m) costs
 * (double) and blended similarities (float32, NaN where the blend was not finite) of one problem exactly as both entries compute
 * them, for measuring them against the reference's matrices; 0, or 7 on null tables or sizes out of range. */
#define HRN_MAX_TRACKED 256
int hrn_associate_people(int P, const int32_t *cur_start, const int32_t *prev_start, int J, int32_t *boxes, float *pts,
                         const int32_t *prev_boxes, const float *prev_pts, const int32_t *prev_ids, int32_t *next_id, double pose_alpha,
                         double similarity_threshold, double smoothing_alpha, int32_t *ids, int32_t *match, int32_t *status);
const char *hrn_associate_people_last_error(void);
int hrn_associate_people_dev(hrn_handle h, int P, const int32_t *cur_start_host, const int32_t *prev_start_host, int J,
                             int32_t *boxes_dev, float *pts_dev, const int32_t *prev_boxes_dev, const float *prev_pts_dev,
                             const int32_t *prev_ids_dev, int32_t *next_id_dev, double pose_alpha, double similarity_threshold,
                             double smoothing_alpha, int32_t *ids_dev, int32_t *match_dev, int32_t *status_dev, void *stream);
int hrn_assoc_exp(const double *x, int n, double *out);
int hrn_associate_similarity(const int32_t *boxes, const float *pts, int n, const int32_t *prev_boxes, const float *prev_pts, int m, int J,
                             double pose_alpha, double *cost_out /* (n,m) */, float *sim_out /* (n,m) */);

/* ---- person ids through occlusions: a per-stream track table, on the host and on the device ----
 * hrn_associate_people compares this frame with the previous frame and nothing else: a person missing for one frame returns as a
 * stranger, and the library's "nobody" row (all zeros: track_frame's lost person, pose_nms' suppressed one, detections_to_frame's
 * dropped one) is numbered anew on every frame.  A TRACK TABLE replaces the pair "previous frame's arrays + hrn_associate_people":
 * one update per frame, lost tracks stay for up to max_lost updates, and with coast a track is compared where a constant-velocity
 * model expects it.  The arithmetic is csrc/tracks_math.h's over csrc/assoc_math.h's (unchanged), one text for both entries.
 *
 * TABLE.  Stream p of P has capacity C, 1 <= C <= HRN_MAX_TRACKED.  All arrays are in / out, C-contiguous:
 *   slot_id    (P, C) int32      -1: the slot is free            slot_lost  (P, C) int32   updates since the track was last accepted
 *   slot_hits  (P, C) int32      accepted updates, saturating at 2^30 (a new track starts at 1)
 *   slot_row   (P, C) int32      the track's row in the latest update, counted from cur_start[p]; -1 when it was not seen
 *   slot_boxes (P, C, 4) int32   the last accepted observation, after smoothing       slot_pts  (P, C, J, 3) float32  likewise
 *   slot_vel   (P, C, 2) float32 box-centre velocity (dy, dx) per update               next_id   (P) int32  the stream's id counter
 * A fresh table has slot_id -1, slot_row -1 and every other value 0 (all bits); a freed slot is written back to exactly that.
 *
 * ONE UPDATE of stream p, with the rows [cur_start[p], cur_start[p + 1]) of boxes (n, 4) int32 and pts (n, J, 3) float32 (in / out):
 *  1. A row is PRESENT iff x2 > x1 && y2 > y1.  An absent row takes part in nothing: ids = match_row = slot = -1, its box and joints
 *     keep their bits.
 *  2. The COLUMNS are the live slots (slot_id >= 0): first those with slot_lost == 0 in ascending (slot_row, slot index), then the
 *     others in ascending slot index.  The rows are the present rows in row order.  (While nobody is lost this is the previous
 *     frame's row order, so ties in the assignment fall as in hrn_associate_people.)
 *  3. COMPARED STATE of a column: k = coast ? (double)slot_lost + 1 : 0.  k == 0: the stored bits.  Otherwise a box component is
 *     t = (double)b + (double)v * k with v = dx for x1, x2 and dy for y1, y2 (product and sum each rounded once); NaN: b; else
 *     clamped to [-2^31, 2^31 - 1] and truncated towards zero.  A joint's y and x are (float)((double)c + (double)v * k); the
 *     confidence is copied.
 *  4. ASSOCIATION: assoc_pair on (row, compared state) over (present rows x columns), hrn_assignment's matching, acceptance
 *     sim > f32(similarity_threshold) -- hrn_associate_people's, expression for expression.
 *  5. ACCEPTED pair (row i, slot s): ids[i] = slot_id[s]; match_row[i] = the slot's OLD slot_row if its old slot_lost was 0, else
 *     -1; slot[i] = s.  Velocity first, from the RAW current box and the STORED box (not the compared one): centres
 *     ((double)lo + (double)hi) / 2 per axis, d = (c_now - c_stored) / ((double)old_lost + 1); old slot_hits == 1: vel = (float)d,
 *     otherwise vel = (float)((double)vel + va * (d - (double)vel)), va = velocity_alpha; a non-finite component becomes +0.0f.
 *     Then, when smoothing_alpha != 0, assoc_smooth_box / assoc_smooth_joint of the row against the COMPARED state (all three
 *     joint components, as today).  The result is written to boxes / pts and into the slot (without smoothing the slot takes the
 *     row as it is).  slot_lost = 0, slot_hits = min(hits + 1, 2^30), slot_row = i.
 *  6. UNACCEPTED live slot: freed when slot_lost + 1 > max_lost; otherwise slot_lost += 1, slot_row = -1 and its observation and
 *     velocity keep their bits.
 *  7. NEW PEOPLE, the present rows not accepted, take in row order the free slots in ascending slot index (those freed in step 6
 *     included) and are numbered assoc_fresh_id(next_id, rank) in row order.  A new slot: observation = the row, vel = 0,
 *     slot_lost = 0, slot_hits = 1, slot_row = i.  With no slot left the row is still numbered, gets slot = -1 and status bit 2.
 *  8. next_id = assoc_next_id(next_id, max id among this update's present rows); a stream without a present row leaves it (steps
 *     2 and 6 still run: lost tracks age).
 *   cur_start  P + 1 int32, non-decreasing, on the HOST in both entries;  ids, match_row, slot  n int32 out;  status  P int32 out:
 *   bits 0 and 1 as in hrn_associate_people, bit 2: the table was full.
 *   pose_alpha, similarity_threshold finite; smoothing_alpha in [0, 1]; max_lost in [0, 2^20]; coast 0 or 1; velocity_alpha in (0, 1].
 * A table the caller filled is taken as it is (it cannot be read before a stream-ordered launch): slot_lost and slot_hits are
 * expected non-negative; no value leads to an access outside the arrays.
 * Code 7, judged before anything is written and named by hrn_track_people_last_error() (per thread) / hrn_last_error(h): the set
 * of hrn_associate_people (P < 0, J, the parameters, null or decreasing segment table, null arrays), C out of range, max_lost /
 * coast / velocity_alpha out of range, null table arrays, more than HRN_MAX_TRACKED rows in a stream; then, for the device entry,
 * a plan-only handle.
 * hrn_track_people is the host form: no handle, no GPU.  hrn_track_people_dev has every array in device memory and cur_start on the
 * host: ONE launch, one 256-thread block per stream that owns the stream's table and updates it in place (columns ranked by
 * counting, rows compacted by ballot, pairs by all threads, the assignment by one wave -- the text hrn_associate_people_dev runs,
 * csrc/assoc_assign.h -- steps 5-8 by the block), stream-ordered, no host read, no atomics; equal to the host form bit for bit.
 * The live-column count is known only on the device, so the handle keeps scratch for n x C per stream: 12 * n * C bytes (at most
 * 768 KiB) plus, with coast, 16 * C + 12 * C * J bytes of compared state (at most 772 KiB), grown on demand.  For P > 1 the stream
 * table goes through one upload.  P == 0 launches nothing. */
int hrn_track_people(int P, const int32_t *cur_start, int C, int J, int32_t *boxes, float *pts, int32_t *slot_id, int32_t *slot_lost,
                     int32_t *slot_hits, int32_t *slot_row, int32_t *slot_boxes, float *slot_pts, float *slot_vel, int32_t *next_id,
                     double pose_alpha, double similarity_threshold, double smoothing_alpha, int max_lost, int coast,
                     double velocity_alpha, int32_t *ids, int32_t *match_row, int32_t *slot, int32_t *status);
const char *hrn_track_people_last_error(void);
int hrn_track_people_dev(hrn_handle h, int P, const int32_t *cur_start_host, int C, int J, int32_t *boxes_dev, float *pts_dev,
                         int32_t *slot_id_dev, int32_t *slot_lost_dev, int32_t *slot_hits_dev, int32_t *slot_row_dev,
                         int32_t *slot_boxes_dev, float *slot_pts_dev, float *slot_vel_dev, int32_t *next_id_dev, double pose_alpha,
                         double similarity_threshold, double smoothing_alpha, int max_lost, int coast, double velocity_alpha,
                         int32_t *ids_dev, int32_t *match_row_dev, int32_t *slot_dev, int32_t *status_dev, void *stream);

/* ---- joints over time: One-Euro smoothing and motion lookahead, on the host and on the device ----
 * The One-Euro filter (Casiez, Roussel, Vogel, CHI 2012) of every joint, a first-order low-pass whose cut-off rises with the
 * filtered speed, and the prediction its derivative estimate gives: next frame's joints ~ this frame's RAW joints + filtered
 * velocity * lookahead (what hrn_boxes_from_poses / the tracking link should be fed instead of where the joints were).  The state
 * follows people through `match` as hrn_associate_people(_dev) writes it, so on the device it never passes through the host.
 * Both entries serve P independent streams with segment tables as in hrn_associate_people: stream p has the current people
 * [cur_start[p], cur_start[p + 1]) and the previous people [prev_start[p], prev_start[p + 1]).  The arithmetic is
 * csrc/temporal_math.h's, one text for both entries: plain C++, fp contraction off, doubles, the operation order below, no library
 * call -- every operation one correctly rounded IEEE operation.
 *   Per call   dt (seconds since the previous frame), min_cutoff, beta, d_cutoff, lookahead as doubles; threshold as a float.
 *   State      state (n, J, 6) float32 = (y_raw, x_raw, y_hat, x_hat, dy_hat, dx_hat); age (n, J) int32: 0 no state, 1 initialised
 *              by this update, otherwise the previous age + 1, saturating at 2^30.
 *   alpha      TWO_PI = 6.283185307179586;  alpha(fc) = 1.0 / (1.0 + (1.0 / (TWO_PI * fc)) / dt), in exactly this order.
 *   LIVE       joint (i, j) of this frame is live iff confidence > threshold and y, x are finite.  The compare is in float32, so
 *              equality and NaN are not live: hrn_pose_boxes' predicate.
 *   PRIOR      the joint has a prior iff person i's match lies in [0, m_p) of its stream AND that previous person's age[j] > 0.
 *              A match outside [-1, m_p) counts as -1.  match == NULL: nobody has a prior.
 *   Not live   pts_out and pred_out carry the input through, bit for bit; the six state values are +0.0f and age is 0.
 *   Live without a prior   raw = hat = v (the input's bits), d_hat = +0.0f, age = 1; output and prediction equal the input.
 *   Live with a prior      per axis, y then x, with x = (double)v and r, p, d the previous raw, hat, d_hat widened:
 *                  raw_d = (x - r) / dt                       the derivative of RAW samples, as in the paper's reference code
 *                  dh    = d + alpha(d_cutoff) * (raw_d - d)
 *                  fc    = min_cutoff + beta * fabs(dh)
 *                  xh    = p + alpha(fc) * (x - p)            the lerp form: a constant input is a fixed point, exactly
 *                  store (float)xh, (float)dh, raw = v;  age = min(previous age + 1, 2^30)
 *                  pred  = (float)(x + (double)(float)dh * lookahead)
 *              pts_out holds (float)xh.  If (float)xh or (float)dh of either axis is not finite, the whole joint is re-initialised
 *              as "live without a prior": a stored state is always finite.  A non-finite pred component becomes the input's.
 *   The confidence is copied untouched into pts_out and pred_out.
 * THE PREDICTION STARTS FROM THE RAW POSITION on purpose: on steady motion the filtered position lags (about 4 px at 1 px/frame and
 * 21 px at 60 px/frame with min_cutoff 1, beta 0.007, d_cutoff 1 at 30 frames/s) while raw + velocity converges to zero error.
 * The lag is the filter's known trade, tuned by beta.
 *   pts        (n, J, 3) float32 (y, x, confidence)           match     n int32, counted from prev_start[p]; NULL: no priors
 *   prev_state (m, J, 6), prev_age (m, J)                     the state the previous call wrote
 *   pts_out    (n, J, 3); may be pts itself                   pred_out  (n, J, 3) or NULL: not wanted
 *   state      (n, J, 6) out, age (n, J) out
 * Code 7 for both, judged before anything is written, named by hrn_filter_poses_last_error() (per thread) / hrn_last_error(h): P < 0;
 * J outside [1, HRN_MAX_JOINTS]; dt, min_cutoff or d_cutoff not finite or not positive; beta or lookahead not finite or negative;
 * null segment tables with P > 0; a table that starts below zero or decreases; null pts / pts_out / state / age with n > 0; more than
 * 2^31 - 1 (person, joint) pairs in one call; state / age overlapping prev_state / prev_age; m > 0 with null previous arrays while
 * match is given; then, for the device entry, a plan-only handle.  There is no cap on people per stream.
 * hrn_filter_poses is the host form: no handle, no GPU.  hrn_filter_poses_dev has every array in device memory and the two segment
 * tables on the HOST: ONE launch, one thread per (person, joint), 256-thread blocks, the state gathered through match; no atomics,
 * no scratch, one writer per byte, stream-ordered, no host read; its results equal the host form's bit for bit.  P == 1 uploads
 * nothing; P > 1 sends one table (8 bytes per person) through one upload; P == 0 or n == 0 launches nothing. */
int hrn_filter_poses(int P, const int32_t *cur_start, const int32_t *prev_start, int J, const float *pts, const int32_t *match,
                     const float *prev_state, const int32_t *prev_age, double dt, double min_cutoff, double beta, double d_cutoff,
                     float threshold, double lookahead, float *pts_out, float *pred_out, float *state, int32_t *age);
const char *hrn_filter_poses_last_error(void);
int hrn_filter_poses_dev(hrn_handle h, int P, const int32_t *cur_start_host, const int32_t *prev_start_host, int J,
                         const float *pts_dev, const int32_t *match_dev, const float *prev_state_dev, const int32_t *prev_age_dev,
                         double dt, double min_cutoff, double beta, double d_cutoff, float threshold, double lookahead,
                         float *pts_out_dev, float *pred_out_dev, float *state_dev, int32_t *age_dev, void *stream);

/* ---- pose NMS: rescoring and OKS non-maximum suppression per image or stream, on the host and on the device ----
 * What the evaluation does after the last batch (datasets/COCO.py:353-382: every person's score becomes box score times the mean
 * confidence of its joints above in_vis_thre, then oks_nms or soft_oks_nms per image, misc/nms/nms.py:75-177), and what a video
 * loop needs between two detector runs, when two tracks have drifted onto one body.  Both entries solve P independent problems:
 * problem p has the people [start[p], start[p + 1]) of the arrays below.  The arithmetic is csrc/pose_nms_math.h's, one text for
 * both entries (its header states every expression and its rounding); in short:
 *   layout     flags & HRN_POSE_NMS_ENGINE: kpts = pts (n, J, 3) float32 (y, x, confidence), areas = boxes (n, 4) int32 with area
 *              (x2 - x1) * (y2 - y1) in fp64, scores = det_scores (n) float32 or NULL = 1.0 -- what hrn_forward and the tracking
 *              link write.  Otherwise the COCO layout, hrn_oks_nms's: kpts (n, J, 3) float64 (x, y, score), areas (n) float64,
 *              scores (n) float64.  Every value is widened exactly to fp64 before any arithmetic.
 *   rescoring  rescore_thre NaN: off.  Else score = mean of the confidences > rescore_thre (sequential fp64 sum in joint order;
 *              0 when there is none) * score.
 *   order      descending score, STABLE: equal scores keep index order; NaN scores come last, in index order, and set status bit 0
 *              (a definition of this library: numpy's argsort()[::-1] is not stable)
 *   OKS        of a candidate d against a kept person g: e_j = (dx^2 + dy^2) / (2 sigma_j)^2 / ((a_g + a_d) / 2 + spacing(1)) / 2;
 *              mean of exp(-e_j) over the joints with c_d > in_vis_thre (the CANDIDATE's mask only, the reference's quirk; NaN: all
 *              joints) in numpy's pairwise summation order; 0.0 without any; exp is assoc_math.h's (at most 1 ulp from libm's).
 *              sigmas: J fp64 values, or NULL for COCO's 17 (then J must be 17).  A non-finite OKS counts as 0 (status bit 1).
 *   hard       walk the order; a person still alive is kept and removes every later alive person with OKS > thresh
 *   soft       flags & HRN_POSE_NMS_SOFT: at most 20 are kept; after each pick every remaining score becomes
 *              s * exp(-(o * o) / thresh) and the rest is re-ordered (descending, equal scores keeping their positions)
 *   suppress   flags & HRN_POSE_NMS_SUPPRESS (engine layout only): every person who is not kept gets all J confidences and all
 *              four box values set to 0 -- what the tracking link gives a lost person, so hrn_draw_poses skips it and the next
 *              hrn_boxes_from_poses reports it lost.  Nothing else of kpts / areas is written.
 * Outputs, indices counted from the problem's first person:
 *   keep        n int32: each problem's segment holds its kept people in selection order, then -1
 *   num         P int32: how many were kept          scores_out  n fp64: the scores after rescoring
 *   suppressor  n int32: -1 kept; hard: the kept person that removed it; soft: -2 for the people left over at the cap of 20
 *   status      P int32: bit 0 a NaN score was ordered last; bit 1 a non-finite OKS was counted as 0
 * At most HRN_MAX_TRACKED people per problem, J in [1, HRN_MAX_JOINTS]; start holds P + 1 non-decreasing int32 on the HOST in both
 * entries.  Argument errors are code 7, judged before anything is written: null tables, a decreasing segment table, more people
 * or joints than that, non-finite thresh, thresh <= 0 with soft NMS, J != 17 without sigmas, suppress in the COCO layout, unknown
 * flag bits; hrn_pose_nms_last_error() (per thread) / hrn_last_error(h) names the cause.
 * hrn_pose_nms is the host form: no handle, no GPU.  hrn_pose_nms_dev has every array except the segment table in device memory
 * (sigmas included): ONE launch, one 256-thread block per problem, stream-ordered, no host read, no atomics; its results equal the
 * host form's bit for bit.  The block computes one OKS row per KEPT person, one thread per candidate, serial over the joints: a
 * latency link, not a throughput kernel -- 256 people with 133 joints cost up to 256 serial rows of 133 exps per thread on one
 * CU.  For P > 1 the problem table goes through one upload; P == 1 uploads nothing; P == 0 launches nothing.
 * hrn_pose_nms_oks_row (no GPU): the OKS of all n people of one problem against its person g exactly as both entries compute it,
 * for measuring it against the reference's oks_iou; 0, or 7 on null tables or sizes out of range. */
#define HRN_POSE_NMS_SOFT 1
#define HRN_POSE_NMS_SUPPRESS 2
#define HRN_POSE_NMS_ENGINE 4
int hrn_pose_nms(int P, const int32_t *start, int J, int flags, void *kpts, void *areas, const void *scores, double thresh,
                 double in_vis_thre, double rescore_thre, const double *sigmas, int32_t *keep, int32_t *num, double *scores_out,
                 int32_t *suppressor, int32_t *status);
const char *hrn_pose_nms_last_error(void);
int hrn_pose_nms_dev(hrn_handle h, int P, const int32_t *start_host, int J, int flags, void *kpts_dev, void *areas_dev,
                     const void *scores_dev, double thresh, double in_vis_thre, double rescore_thre, const double *sigmas_dev,
                     int32_t *keep_dev, int32_t *num_dev, double *scores_out_dev, int32_t *suppressor_dev, int32_t *status_dev,
                     void *stream);
int hrn_pose_nms_oks_row(int n, int J, int flags, const void *kpts, const void *areas, int g, double in_vis_thre, const double *sigmas,
                         double *oks_out /* n */);

/* ---- COCO keypoint AP / AR: OKS matching per image and precision / recall accumulation over the set, host and device ----
 * The number evaluate_overall_accuracy returns (datasets/COCO.py:574-588): the ten statistics AP, AP .5, AP .75, AP (M), AP (L),
 * AR, AR .5, AR .75, AR (M), AR (L) that the reference gets from pycocotools' COCOeval (iouType 'keypoints', one category,
 * maxDets 20).  pycocotools is not available where this library is built and tested, so THE CONTRACT IS THE DEFINITION in
 * csrc/keypoint_eval_math.h -- one text for both entries, every expression and its rounding -- and parity with pycocotools is NOT
 * pinned (tests/golden/make_cocoeval_golden.py measures it wherever pycocotools is installed).  In short:
 *   inputs     P images in ascending image-id order; dt_start / gt_start hold P + 1 non-decreasing int32 on the HOST in both
 *              entries; dt_kpts (N, J, 3) fp64 (x, y, score), dt_scores (N) fp64; gt_kpts (M, J, 3) fp64 (x, y, v), gt_area (M) fp64,
 *              gt_bbox (M, 4) fp64 (x, y, w, h), gt_iscrowd (M) int32; sigmas J fp64 or NULL for COCO's 17 (then J must be 17)
 *   constants  iouThrs = np.linspace(0.5, 0.95, 10), recThrs = np.linspace(0, 1, 101), maxDet = 20, area ranges all [0, 1e10],
 *              medium [32^2, 96^2], large [96^2, 1e10]
 *   slots      per image the detections in descending score, STABLE, NaN last (status bit 0); the first 20 are the image's slots,
 *              the rest take no part; a detection's area is (max x - min x) * (max y - min y) over all J joints
 *   OKS(d, g)  k1 = g's joints with v > 0.  k1 > 0: dx = x_d - x_g, dy likewise, over g's joints with v > 0.  k1 = 0: the distance
 *              to the doubled box, dx = max(0, (bx - bw) - x_d) + max(0, x_d - (bx + 2 bw)), dy likewise, over all J joints.
 *              e_j = (dx dx + dy dy) / (2 sigma_j)^2 / (area_g + spacing(1)) / 2; the mean of exp(-e_j) in numpy's pairwise order
 *              with assoc_math.h's exp.  A non-finite OKS counts as 0 (status bit 1).
 *   flags      ignore_g = iscrowd_g or k1 == 0; in range a: ig_g = ignore_g or area_g outside [lo_a, hi_a]; people are visited
 *              ig = 0 first, then ig = 1, each part in index order
 *   matching   per (range a, threshold t), slots in order: best = min(t, 1 - 1e-10); walk the people: skip a taken non-crowd; stop
 *              when a counted match is held and the ignored part begins; skip OKS < best; else take it (equal replaces).  A match
 *              on an ignored person makes the slot ignored; an unmatched slot with its own area outside the range is ignored.
 *   curve      per (a, t) all slots of the set in descending score, stably (ties: image order, then slot order; NaN last); tp / fp
 *              running counts of matched / unmatched slots that are not ignored; npig_a = people with ig = 0; rc = tp / npig_a,
 *              pr = tp / (fp + tp + spacing(1)), pr made non-increasing from the end; precision(a, t, r) = pr at the first index
 *              with rc >= recThr_r, or 0; recall(a, t) = the last rc, or 0 without slots; npig_a == 0: both are -1 for the range
 *   stats      each the mean over the entries > -1 of its slice (sequential fp64 sum in (t, r) order, one division), -1 if none
 * Outputs, S = the sum over the images of min(detections, 20), slots in image order then slot order:
 *   stats (10) fp64; precision (3, 10, 101) fp64; recall (3, 10) fp64
 *   slot_person (S) int32: the detection's index in dt_kpts; slot_score (S) fp64
 *   dt_match (3, 10, S) int32: the matched person's index in gt_kpts, or -1; dt_ignore (3, 10, S) uint8
 *   npig (P, 3) int32; status (P) int32
 * At most HRN_MAX_TRACKED detections and HRN_MAX_TRACKED ground-truth people per image, J in [1, HRN_MAX_JOINTS].  Argument errors
 * are code 7, judged before anything is launched or written: a bad J, J != 17 without sigmas, null arrays, decreasing segment
 * tables, more than that on either side; hrn_keypoint_eval_last_error() (per thread) / hrn_last_error(h) names the cause.
 * hrn_keypoint_eval is the host form: no handle, no GPU.  hrn_keypoint_eval_dev has every array except the two segment tables in
 * device memory (sigmas included); stream-ordered, no host read, no atomics, every byte has one writer; its results equal the
 * host form's bit for bit.  Four launches: MATCH, one 256-thread block per image (the order, the <= 20 x <= 256 OKS matrix in
 * LDS with one thread per pair and serial joints, the people's orders, the 30 matchings on 30 lanes); RANK, every slot's place in
 * the set-wide order by counting the slots before it (O(S^2) compares through LDS tiles, no sort); CURVE, one block per (a, t):
 * the totals, then one pass from the end with block scans of the exact integer counts, the envelope and the 101 look-ups;
 * FINISH, one block: the ten statistics.  The image table goes through one upload; with P == 0 only CURVE and FINISH run.
 * hrn_keypoint_eval_oks (no GPU): the OKS of all n_d x n_g pairs of one image exactly as both entries compute it (a non-finite
 * value as 0.0); hrn_keypoint_eval_constants (no GPU): the tables above; both 0, or 7 on null tables or sizes out of range. */
int hrn_keypoint_eval(int P, const int32_t *dt_start, const int32_t *gt_start, int J, const double *dt_kpts, const double *dt_scores,
                      const double *gt_kpts, const double *gt_area, const double *gt_bbox, const int32_t *gt_iscrowd,
                      const double *sigmas, double *stats, double *precision, double *recall, int32_t *slot_person,
                      double *slot_score, int32_t *dt_match, uint8_t *dt_ignore, int32_t *npig, int32_t *status);
const char *hrn_keypoint_eval_last_error(void);
int hrn_keypoint_eval_dev(hrn_handle h, int P, const int32_t *dt_start_host, const int32_t *gt_start_host, int J,
                          const double *dt_kpts_dev, const double *dt_scores_dev, const double *gt_kpts_dev, const double *gt_area_dev,
                          const double *gt_bbox_dev, const int32_t *gt_iscrowd_dev, const double *sigmas_dev, double *stats_dev,
                          double *precision_dev, double *recall_dev, int32_t *slot_person_dev, double *slot_score_dev,
                          int32_t *dt_match_dev, uint8_t *dt_ignore_dev, int32_t *npig_dev, int32_t *status_dev, void *stream);
int hrn_keypoint_eval_oks(int n_d, int n_g, int J, const double *dt_kpts, const double *gt_kpts, const double *gt_area,
                          const double *gt_bbox, const double *sigmas, double *oks_out /* n_d x n_g */);
int hrn_keypoint_eval_constants(double *iou_thrs /* 10 */, double *rec_thrs /* 101 */, double *area_ranges /* 3 x (lo, hi) */);

/* ---- pose overlays on the GPU: the joints and bones of every person, drawn into frames that stay on the device ----
 * Replaces, for every frame of the two demo programs (scripts/live-demo.py:135-138, scripts/extract-keypoints.py's sibling loop),
 *   for i, pt in enumerate(pts): frame = draw_points_and_skeleton(frame, pt, skeleton, person_index=i, ...)
 * (misc/visualization.py:71-192: cv2.line per bone, thickness 2, then cv2.circle per joint, filled) -- the one step that still
 * forced a decoded frame through the host.  OpenCV is not available where this library is built and tested, and cv2.line's
 * fixed-point polygon fill cannot be restated blind, so THE CONTRACT IS THIS INTEGER DEFINITION, which looks like the reference's
 * overlay; pixel equality with a cv2 build is NOT claimed (tests/golden/make_draw_golden.py counts the differing pixels wherever
 * opencv-python is installed).  tests/draw_ref.py restates the definition in numpy; the kernels equal it byte for byte.
 *
 * Inputs.  pts (n, J, 3) float32 (y, x, confidence), as hrn_forward writes them.  A joint is LIVE iff confidence > threshold
 * (float32; equality and NaN are not live), y and x are finite, and X = trunc(x), Y = trunc(y) (towards zero, Python's int():
 * -0.7 -> 0) lie in [-8192, 16383].  Frame sides are at most 8192.  With these bounds every expression below fits signed 64 bits:
 * |w| < 2^14 and |d| < 2^14.6 per component, 4 cross^2 < 2^62.
 * Joint disc.  Radius r >= 1 (radius = 0: the reference's max(1, min(height, width) / 160), per canvas).  The disc of a live joint
 * covers pixel (px, py) iff (px - X)^2 + (py - Y)^2 <= r*r + r: the 3x3 square for r = 1, the 5x5 without corners for r = 2, row
 * half-widths 3, 3, 2, 1 for r = 3.
 * Bone.  Bone k = (a, b) of the skeleton is drawn iff both joints are live; thickness T.  With P0 = (Xa, Ya), P1 = (Xb, Yb),
 * d = P1 - P0, L2 = d.d, w = p - P0, t = w.d it covers p iff
 *     t <= 0  and 4 |w|^2 <= T^2,   or   t >= L2 and 4 |p - P1|^2 <= T^2,   or otherwise   4 (wx dy - wy dx)^2 <= T^2 L2
 * -- a capsule of radius T / 2 around the segment (T = 2: a horizontal bone is 3 rows thick with one-pixel tips; P0 == P1: a plus).
 * Order.  Primitives are numbered person-major in call order, inside a person the bones k = 0 .. K-1, then the joints
 * j = 0 .. J-1; a pixel takes the colour of the HIGHEST-numbered primitive that covers it (the reference's loop: later draws
 * overwrite).  Joint j takes point_colors[j % Cp]; every bone of person i takes bone_colors[person_index[i] mod Cb] (Python's
 * modulo: never negative; person_index NULL: i).
 * Untouched pixels are NOT WRITTEN: the call is in place, every other byte of a buffer (pitch padding included) keeps its value.
 * YUV canvases (NV12 / I420, even sides, any pitch): colours are (Y, U, V) bytes (hrn_yuv_from_bgr); a covered pixel's Y byte takes
 * the winner's Y; the chroma sample of a 2x2 block is written iff at least one of its four pixels is covered, and takes U and V of
 * the highest-numbered primitive that covers any of the four.  HRN_PIX_NV21, _P010 and _I010 canvases are refused as an unknown
 * format, here and in hrn_draw_labels_dev (colours are 8-bit triples: a 10-bit overlay wants a definition of its own); a pipeline
 * of such frames draws on the BGR frame hrn_yuv_to_bgr gives it, and hrn_bgr_to_yuv_frames carries the drawn frame back to its layout.
 *
 *   canvases_host     nframes entries on the HOST; hrn_canvas has hrn_yuv_frame's fields with writable planes.  HRN_PIX_BGR: y = the
 *                     (height, width, 3) uint8 pixels, pitch_y = bytes between rows >= 3 * width (a view into a larger buffer
 *                     works), the other fields unused.  NV12 / I420: as hrn_yuv_frame; matrix and range are documentation only.
 *                     All canvases people refer to are BGR, or all are YUV; one nobody refers to may be null.
 *                     The canvases people refer to must NOT OVERLAP in memory (each byte has one writer, in no order between
 *                     canvases): two entries with the same first plane are refused, overlapping views are the caller's to avoid.
 *   pts_dev           (n, J, 3) float32 on the device, J in [1, HRN_MAX_JOINTS]
 *   frame_index_host  n entries: person i is drawn on canvases_host[frame_index_host[i]]; NULL: nframes == 1
 *   skeleton_host     K pairs of int32 joint indices in [0, J), K in [0, 65535]
 *   point_colors_host / bone_colors_host   Cp / Cb colours of three bytes, in the canvas's channel order (B, G, R or Y, U, V)
 *   radius in [0, 64], thickness in [1, 16]
 * Two launches whatever n and nframes (build: one record per person from the joints where they lie, no host synchronisation;
 * rasterise: one block per 32 x 32 tile of the canvases referred to), stream-ordered.  n == 0 succeeds and launches nothing.
 * Fails with code 7 and nothing launched, each failure naming its cause, on: null tables; n < 0; J, K, Cp, Cb, radius or thickness
 * out of range; a skeleton index outside [0, J); a frame index outside [0, nframes); a referenced canvas that is null, has an
 * unknown format, a non-positive, odd-for-YUV or over-8192 side, or too small a pitch; mixed formats; two referenced canvases
 * that name the same buffer; a plan-only handle.
 * Everything is judged before the device is touched, as in hrn_preprocess_frames_yuv.
 *
 * hrn_yuv_from_bgr (no handle, no GPU): n (B, G, R) colours to (Y, U, V) by the float64 forward formula of the matrix and range
 * that hrn_yuv_coefficients quantises: Y' = Kr R + Kg G + Kb B; Y = y0 + sy Y'; U = 128 + sc (B - Y') / (2 (1 - Kb));
 * V = 128 + sc (R - Y') / (2 (1 - Kr)); sy = 219/255 and sc = 224/255 for limited range (y0 = 16), 1 for full; each clip8(rint(.)).
 * Through the conversion above the round trip errs by at most 2 grey levels (limited) / 1 (full) over all 2^24 colours. */
enum { HRN_PIX_BGR = 0 };
typedef struct { uint8_t *y, *u, *v;           /* device; BGR: y = the pixels; NV12: u = the UV plane */
                 int32_t height, width, pitch_y, pitch_c, format, matrix, range; } hrn_canvas;
int hrn_draw_poses(hrn_handle h, const hrn_canvas *canvases_host, int nframes, const float *pts_dev, int n, int J,
                   const int32_t *frame_index_host /* n entries; NULL: nframes == 1 */, const int32_t *skeleton_host, int K,
                   const uint8_t *point_colors_host, int Cp, const uint8_t *bone_colors_host, int Cb,
                   const int32_t *person_index_host /* n entries or NULL */, int radius /* 0: the reference's rule */,
                   int thickness, float threshold, void *stream);
/* hrn_draw_poses with the person indices ON THE DEVICE (the ids hrn_associate_people_dev wrote): person_index_dev holds n int32
 * and is required; everything else, the checks and the drawn bytes are hrn_draw_poses'.  The bone palette is uploaded with the
 * call's table and one small launch behind the copy fills each person's bone colour, bone_colors[person_index mod Cb] (Python's
 * modulo), before the two launches of hrn_draw_poses: three launches, no host read. */
int hrn_draw_poses_ids_dev(hrn_handle h, const hrn_canvas *canvases_host, int nframes, const float *pts_dev, int n, int J,
                           const int32_t *frame_index_host, const int32_t *skeleton_host, int K, const uint8_t *point_colors_host,
                           int Cp, const uint8_t *bone_colors_host, int Cb, const int32_t *person_index_dev, int radius,
                           int thickness, float threshold, void *stream);

/* ---- person labels on the GPU: the box, the id and the score of every person, drawn beside it ----
 * The overlay above shows skeletons; the state of the tracking chain -- the id that hrn_associate_people_dev / hrn_track_people_dev
 * gives a person, the box the next crop is cut from, the person's score -- is printed by this entry, from the device memory where
 * it lies, with no host read: the decimal digits are formed, laid out and rasterised on the device.  (The reference's demo has
 * its cv2.rectangle commented out, scripts/live-demo.py:140-141.)  As with hrn_draw_poses, pixel equality with cv2.rectangle /
 * cv2.putText is NOT claimed (Hershey fonts cannot be restated blind): THE CONTRACT IS THIS INTEGER DEFINITION.
 * tests/label_ref.py restates it in numpy; the kernels equal it byte for byte.  One text, csrc/draw_labels_math.h, is compiled
 * into the kernels and into hrn_label_layout / hrn_label_covers.
 *
 * Inputs per person i.  box[i] = (x1, y1, x2, y2) int32 -- the boxes hrn_preprocess_frames*, hrn_associate_people_dev and
 * hrn_track_people_dev write; optional id[i] int32; optional score[i] float32, read at scores_dev[i * score_stride] (column 4
 * of an (n, 5) detection tensor is passed where it lies, score_stride = 5).
 * Drawn iff all four coordinates lie in [-8192, 16383] and x2 > x1 and y2 > y1; the library's empty box (0, 0, 0, 0), "nobody", is
 * therefore never drawn.  Frame sides are at most 8192.  Every expression fits 32 bits: |coordinate| < 2^14, a plate is at most
 * 16 * 85 = 1360 wide.
 * Colour index.  c = id[i] when ids are given, else i.  The person's colour is colors[c mod Cb], the person's text colour
 * text_colors[c mod Cb] (Python's modulo: id -1 takes Cb - 1); both palettes have Cb entries of three bytes in the canvas's
 * channel order (B, G, R or Y, U, V).
 * Text.  A row of D <= 14 cells, each a digit or a blank.  With id[i] >= 0: its decimal digits, most significant first (1 to 10
 * cells; a negative id prints nothing).  With a score v = score[i]: NaN gives no score field; v < 0 is taken as 0 and v > 1 as 1;
 * p = (int)(v * 100.0f + 0.5f) -- two float32 operations, each rounded once, never contracted into an FMA -- lies in 0 .. 100; the
 * cells are one blank when id digits precede, then the decimal digits of p.  No cells at all: no plate and no ink.
 * Glyphs.  5 columns x 7 rows, rows top to bottom, bit 4 = the leftmost column (the HD44780 digit set):
 *     0: 0E 11 13 15 19 11 0E    5: 1F 10 1E 01 01 11 0E
 *     1: 04 0C 04 04 04 04 0E    6: 06 08 10 1E 11 11 0E
 *     2: 0E 11 01 02 04 08 1F    7: 1F 01 02 04 08 08 08
 *     3: 1F 02 04 02 01 11 0E    8: 0E 11 11 0E 11 11 0E
 *     4: 02 06 0A 12 1F 02 02    9: 0E 11 11 0F 01 02 0C
 * Scale s in [1, 16]: a glyph dot is s x s pixels.  scale = 0: min(16, max(1, min(height, width) / 360)) per canvas (the rule
 * of radius = 0 above, bounded by the range of s).  Thickness T in [0, 16].
 * Primitives of person i, in this order:
 *   0. Outline: the pixels with x1 <= px <= x2 and y1 <= py <= y2 (both corners inclusive) that do NOT satisfy
 *      x1 + T <= px <= x2 - T and y1 + T <= py <= y2 - T.  T = 0 gives none; a box narrower than 2 T is filled.  The person's colour.
 *   1. Plate: with D cells, width = s (6 D + 1) and height = 9 s; left = x1; top = y1 - 9 s when y1 - 9 s >= 0 (above the box),
 *      else top = y1 (inside it).  It covers left <= px < left + width and top <= py < top + height.  The person's colour.
 *   2. Ink: the digit d in cell k covers (px, py) iff, with u = px - left - s (1 + 6 k) and v = py - top - s, 0 <= u < 5 s and
 *      0 <= v < 7 s and bit 4 - u / s of row v / s of glyph d is set.  The person's text colour.  A blank cell has no ink.
 * Order.  Primitives are numbered person-major in call order; a pixel takes the HIGHEST-numbered primitive that covers it.
 * As in hrn_draw_poses: everything is clipped by the canvas; untouched pixels are NOT WRITTEN, pitch padding never is; on NV12 /
 * I420 a covered pixel's Y byte takes the winner's Y, and the chroma sample of a 2x2 block is written iff at least one of its four
 * pixels is covered, and takes U and V of the highest-numbered primitive that covers any of the four.
 *
 * hrn_label_layout (no handle, no GPU): the record of one person from (box, id, score, scale in [1, 16], thickness in [0, 16]).
 * hrn_label_record is 16 int32: drawn (0: nothing of this person is drawn, every other field 0); x1, y1, x2, y2 and thickness of
 * the outline; the plate's left, top, width, height (no cells: 0); scale; ncells = D; cells_lo, cells_hi: cell k in the four bits
 * at 4 k of (cells_hi : cells_lo), 0 .. 9 a digit, 15 a blank; colour, text_colour: filled on the device from the palettes, 0 here.
 * hrn_label_covers: what the record puts on pixel (px, py) -- 0 nothing, 1 the person's colour (plate or outline), 2 the person's
 * text colour (ink).  Both return 7 on bad arguments, with hrn_label_last_error() (per thread) = "null box / record",
 * "scale must be in [1, 16]", "thickness must be in [0, 16]", "null record" or "the record is not one hrn_label_layout wrote".
 *
 * hrn_draw_labels_dev.  canvases_host, frame_index_host and their rules are hrn_draw_poses'; boxes_dev (n, 4) int32, ids_dev n
 * int32 or NULL, scores_dev or NULL, all on the device; colors_host / text_colors_host Cb colours each, on the host.  Two launches
 * whatever n and nframes, stream-ordered, no host read of device data: a build launch (one thread per person writes the record)
 * and a rasteriser of hrn_draw_poses' geometry (one 256-thread block per 32 x 32 tile of the canvases referred to, a thread per
 * 2x2 block; a tile culls its frame's people 256 at a time from the end of the call order and resolves the survivors last person
 * first -- any number of people on one tile loses none; no atomics, one writer per byte).  n == 0 succeeds and launches nothing.
 * Fails with code 7 and nothing launched, each failure naming its cause, on: n < 0; Cb < 1; scale outside [0, 16]; thickness
 * outside [0, 16]; score_stride < 1 with scores; null tables; several frames without frame_index; a frame index outside
 * [0, nframes); every canvas refusal of hrn_draw_poses (null, unknown format, bad side or pitch, mixed formats, the same buffer
 * twice); after those, a plan-only handle.  Everything is judged before the device is touched. */
typedef struct { int32_t drawn, x1, y1, x2, y2, thickness, left, top, width, height, scale, ncells;
                 uint32_t cells_lo, cells_hi, colour, text_colour; } hrn_label_record;
int hrn_label_layout(const int32_t *box /* 4 */, int has_id, int32_t id, int has_score, float score, int scale, int thickness,
                     hrn_label_record *record_out);
int hrn_label_covers(const hrn_label_record *record, int px, int py);
const char *hrn_label_last_error(void);
int hrn_draw_labels_dev(hrn_handle h, const hrn_canvas *canvases_host, int nframes,
                        const int32_t *boxes_dev /* (n,4) */, const int32_t *ids_dev /* n or NULL */,
                        const float *scores_dev /* or NULL */, int score_stride, int n,
                        const int32_t *frame_index_host /* n entries; NULL: nframes == 1 */,
                        const uint8_t *colors_host, const uint8_t *text_colors_host, int Cb,
                        int scale /* 0: the rule */, int thickness, void *stream);

/* ---- heat-map overlays on the GPU: what the network sees, blended into the frame ----
 * hrn_forward's heat-maps (n, J, hq, wq) never had a picture: the reference leaves it as a "# Heatmaps  # ToDo"
 * (misc/visualization.py:261-266).  This entry reduces a person's maps over the chosen joints, stretches them over the person's
 * box, colours them through a 256-entry table and blends them into the frame, from the device memory where maps, boxes and frame
 * lie.  cv2 cannot be the reference where it is not installed: as with hrn_draw_poses, THE CONTRACT IS THIS INTEGER DEFINITION.
 * tests/heat_ref.py restates it in numpy; the kernels and hrn_draw_heatmaps_host equal it byte for byte.  One text,
 * csrc/heat_math.h, is compiled into the kernels and into the two host entries.
 *
 * Inputs.  Canvases, frame_index and their refusals are hrn_draw_poses' (HRN_PIX_BGR, _NV12, _I420; the other layouts stay "unknown
 * format").  heatmaps (n, J, hq, wq) float32, hq and wq in [1, 1024]; boxes (n, 4) int32 (x1, y1, x2, y2), where hrn_boxes_from_poses /
 * hrn_preprocess_frames_dev leave them; joint_mask J bytes, non-zero = the joint takes part (NULL: all; all zero: refused);
 * lo < hi finite float32; lut (256, 3) uint8 in the canvas's own colour space (B, G, R, or Y, U, V: the caller converts, as for
 * the palettes); alpha in [0, 255]; alpha_mode HRN_HEAT_ALPHA_CONST or HRN_HEAT_ALPHA_VALUE; cutoff in [1, 255].
 * The span of a person's maps on the frame is the decode's (SimpleHRNet.py:306-307): cell (r, c) sits at x = x1 + c bw / wq,
 * y = y1 + r bh / hq with bw = x2 - x1, bh = y2 - y1, so a peak lies under the disc hrn_draw_poses draws for it.  A person with
 * bw <= 0, bh <= 0 or a coordinate outside [-8192, 16383] is skipped (the labels' rule).
 * 1. Reduce and quantise, per person and cell.  v = the maximum over the masked joints, where a NaN never wins a comparison and
 *    all-NaN gives NaN.  t = (v - lo) * k in float32, the subtraction and the product each rounded on their own (no fused
 *    multiply-add), k = 255.0f / (hi - lo) formed once on the host in float32.  Q = 0 unless t > 0; Q = 255 if t >= 255; otherwise
 *    Q = (int)(t + 0.5f) (one more float32 sum).  So NaN and -inf give 0, +inf gives 255.  Q is (n, hq, wq) uint8.
 * 2. Sample, for frame pixel (px, py) with x1 <= px < x2 and y1 <= py < y2, all in integers:
 *    ux = min(((px - x1) wq 256) / bw, (wq - 1) 256) (the product in 64 bits -- or 32 unsigned: on a canvas it stays below 2^32 --
 *    the division floors); c0 = ux >> 8, fx = ux & 255, c1 = min(c0 + 1, wq - 1); uy, r0, r1, fy likewise from py, y1, hq, bh;
 *    top = Q[r0][c0] (256 - fx) + Q[r0][c1] fx, bot the same on r1; S = (top (256 - fy) + bot fy + 32768) >> 16.
 * 3. Combine.  V(px, py) = the maximum of S over the people of that canvas whose box holds the pixel, 0 where nobody's does.  A
 *    maximum has no order: the result depends neither on the call order nor on scheduling.
 * 4. Blend.  a = alpha (CONST) or (alpha V + 127) / 255 (VALUE).  A pixel is written iff V >= cutoff and a > 0; every written
 *    byte is (src (255 - a) + lut[V][ch] a + 127) / 255.  Untouched pixels are NOT WRITTEN, pitch padding never is.  On NV12 / I420
 *    the Y byte is blended per pixel with lut[V][0]; a 2x2 block with at least one written pixel blends its chroma sample once,
 *    with Vc = (V0 + V1 + V2 + V3 + 2) >> 2 over all four pixels, written or not, a_c from Vc by the same mode rule without the
 *    cutoff, U with lut[Vc][1] and V with lut[Vc][2]; the sample is not written when a_c = 0.
 *
 * hrn_draw_heatmaps_dev: two launches whatever n and nframes, stream-ordered, no host read of device data and no atomics -- a
 * reduce launch (the one pass over the fp32 maps, writes Q into the handle's call scratch) and a rasteriser of hrn_draw_poses'
 * geometry (one 256-thread block per 32 x 32 tile of the canvases referred to, a thread per 2x2 block; a tile culls its canvas's
 * people by box 256 at a time and folds each chunk into the running maximum: any number of boxes on a tile loses nobody).  n == 0
 * succeeds and launches nothing.  Fails with code 7 and nothing launched, each failure naming its cause, on: n < 0; J outside
 * [1, HRN_MAX_JOINTS]; hq or wq outside [1, 1024]; lo or hi not finite; hi <= lo; a mask that selects no joint; alpha, alpha_mode
 * or cutoff out of range; null tables; several frames without frame_index; every canvas refusal of hrn_draw_poses; after those, a
 * plan-only handle.
 * hrn_heatmap_quantise (no handle, no GPU): step 1 on host memory, out (n, hq, wq) uint8.  hrn_draw_heatmaps_host (no handle, no
 * GPU): the whole definition on the CPU -- canvases (planes on the HOST), maps and boxes in host memory, the same arguments and
 * refusals.  Both return 7 with hrn_heatmap_last_error() (per thread) naming the cause.
 * Not built: heat-maps on NV21 / P010 / I010 canvases, per-joint colours, contour lines. */
enum { HRN_HEAT_ALPHA_CONST = 0, HRN_HEAT_ALPHA_VALUE = 1 };
int hrn_draw_heatmaps_dev(hrn_handle h, const hrn_canvas *canvases_host, int nframes,
                          const float *heatmaps_dev /* (n,J,hq,wq) */, const int32_t *boxes_dev /* (n,4) */, int n, int J, int hq, int wq,
                          const int32_t *frame_index_host /* n entries; NULL: nframes == 1 */,
                          const uint8_t *joint_mask_host /* J bytes or NULL */, float lo, float hi,
                          const uint8_t *lut_host /* (256,3) */, int alpha, int alpha_mode, int cutoff, void *stream);
int hrn_heatmap_quantise(const float *maps /* (n,J,hq,wq), host */, int n, int J, int hq, int wq,
                         const uint8_t *joint_mask /* J bytes or NULL */, float lo, float hi, uint8_t *out /* (n,hq,wq) */);
int hrn_draw_heatmaps_host(const hrn_canvas *canvases_host /* planes on the host */, int nframes, const float *heatmaps_host,
                           const int32_t *boxes_host, int n, int J, int hq, int wq, const int32_t *frame_index_host,
                           const uint8_t *joint_mask_host, float lo, float hi, const uint8_t *lut_host, int alpha, int alpha_mode,
                           int cutoff);
const char *hrn_heatmap_last_error(void);

/* ---- anonymise people on the GPU: a mosaic over the face, from the head joints ----
 * What a deployment on public footage must do before it may store or show a frame is hide the faces.  After hrn_forward / the
 * tracking link, nose, eyes and ears lie in pts on the device; this entry pixelates, IN PLACE, a square around chosen joints of
 * every person -- or given boxes -- on BGR / NV12 / I420 canvases that stay on the device.  There is no cv2 here, and equality
 * with cv2.blur or a resize down and up is NOT claimed: THE CONTRACT IS THIS INTEGER DEFINITION.  tests/mosaic_ref.py restates
 * it in numpy; the kernels and hrn_mosaic_host equal it byte for byte.  One text, csrc/mosaic_math.h, is compiled into the
 * kernels and into the host entries.
 * WHAT THIS IS NOT: a mosaic with small cells is not irreversible anonymisation (a face can be guessed from 2 x 2 means); the
 * caller chooses `cell`.  It hides what the joints find: a face the network misses is not covered.  ORDER: the mosaic goes
 * BEFORE hrn_draw_heatmaps_dev / hrn_draw_poses / hrn_draw_labels_dev, which then draw on top of it.
 *
 * Inputs.  Canvases, frame_index and their refusals are hrn_draw_poses' (HRN_PIX_BGR, _NV12, _I420; all BGR or all YUV; even sides
 * for YUV; sides <= 8192; no two entries on one buffer; an entry nobody refers to may be null; the other layouts stay "unknown
 * format").  People come from exactly one of
 *   pts (n, J, 3) float32 (y, x, confidence) with a joint list of K indices in [0, J), K in [1, 256] (a repeated index counts once);
 *   boxes (n, 4) int32 (x1, y1, x2, y2), half-open as everywhere in this library.
 * Region of a person from joints.  A joint is LIVE by hrn_draw_poses' predicate, literally: confidence > threshold in float32
 * (equality and NaN are not live), y and x finite, X = trunc(x) and Y = trunc(y) in [-8192, 16383].  Over the live joints of the
 * list: X0 = min X, X1 = max X, Y0, Y1 likewise, E = max(X1 - X0, Y1 - Y0).  Over ALL live joints of the person (all J): the same
 * extent, P.  No listed joint live: the person has no region, status 1.  The half side is
 *     R = max(rmin, (E scale_num + scale_den - 1) / scale_den),    scale_num, scale_den in [1, 64]
 * (1 / 1: a square of side 2 E + 1 -- for a frontal face twice the ear-to-ear width), with rmin = min_half when min_half is in
 * [1, 4096], and for min_half == 0 the rule rmin = (P + 15) / 16: the head of a standing person is about an eighth of their
 * height, which keeps a face in profile, whose joints nearly coincide, from getting a dot.  With cx2 = X0 + X1, cy2 = Y0 + Y1
 * the rectangle is x_lo = (cx2 >> 1) - R, x_hi = ((cx2 + 1) >> 1) + R + 1 (half-open), likewise in y; >> is an arithmetic shift
 * (floor).  Every intermediate fits int32: E <= 16383 + 8192 = 24575, E * 64 < 2^21, |cx2| <= 32766.
 * Region from a box.  The box itself (any int32); x2 <= x1 or y2 <= y1 -- an all-zero box is one -- has no region, status 1.
 * Clipping.  The region is clipped to the person's canvas: [max(x_lo, 0), min(x_hi, width)) x [max(y_lo, 0), min(y_hi, height)).
 * Nothing left: status 2; otherwise status 0.  A person without status 0 has the region (0, 0, 0, 0).
 * Cells.  One cell size s per call from cell in {0, 2, 4, 8, 16, 32}; 0 means, per canvas, the largest power of two not above
 * clamp(min(height, width) / 64, 8, 32): 16 at 1080p, 8 at 720p, 32 at 2160p.  The cells are the canvas-aligned s x s grid (a
 * power of two up to 32 keeps every cell inside one 32 x 32 tile of the drawing family).  A cell is MARKED iff it intersects the
 * clipped region of at least one person of that canvas: covering more than the region, never less, is the point.
 * Pixels.  A marked cell with c pixels inside the canvas (edge cells are partial: c = min(s, width - x0) min(s, height - y0))
 * gets every pixel set, per channel byte, to (sum + (c >> 1)) / c over those pixels.  On NV12 / I420: Y over the cell, U and V
 * each over the cell's (s/2) x (s/2) chroma samples (sides are even: c / 4 of them).  Sums fit int32 (32 * 32 * 255).  Every
 * byte of a marked cell is written; no byte of an unmarked cell, and no pitch padding, is written.
 * What follows.  The result is a function of the SET of marked cells alone: it depends neither on the order of the people, nor on
 * overlaps, nor on scheduling -- no blend, no "later over earlier".  Each mean is taken from the bytes the call found (a cell has
 * one owner, which reads it whole before it writes it: in place is safe), and a second identical call changes no byte.
 *
 * hrn_mosaic_dev: two launches whatever n and nframes, stream-ordered, no host read of device data, no atomics and no scratch of
 * frame size -- a build launch (one wave per person for joints, one thread per person for boxes: the clipped region and the
 * status, from pts or boxes where they lie) and a rasteriser of hrn_draw_poses' geometry (one 256-thread block per 32 x 32 tile of
 * the canvases referred to, a thread per 2x2 block; a tile culls its canvas's people by region 256 at a time into a cell mask, so
 * no number of people on a tile loses anybody; a tile with an empty mask reads no frame byte).  status_dev: n int32 on the device,
 * or NULL.  n == 0 succeeds and launches nothing.  Fails with code 7 and nothing launched, each failure naming its cause, on:
 * n < 0; both or neither of pts_dev / boxes_dev; with pts: J outside [1, HRN_MAX_JOINTS], K outside [1, 256], a null list, a joint
 * index outside [0, J); scale_num or scale_den outside [1, 64]; min_half outside [0, 4096]; cell not one of the six values; null
 * canvases; several frames without frame_index; every canvas refusal of hrn_draw_poses; after those, a plan-only handle.
 * hrn_mosaic_regions (no handle, no GPU; hrn_pose_boxes' sibling): pts or boxes on the host and each person's canvas size
 * canvas_hw (n, 2) (height, width), sides in [1, 8192], to regions_out (n, 4) clipped rectangles and status_out n.
 * hrn_mosaic_host (no handle, no GPU): the whole definition on the CPU -- canvases (planes on the HOST), pts or boxes in host
 * memory, the same arguments and refusals; status_out n int32 or NULL.  Both return 7 with hrn_mosaic_last_error() (per thread)
 * naming the cause.
 * Not built: NV21 / P010 / I010 canvases, Gaussian blur, ellipses, a cell size per person. */
int hrn_mosaic_dev(hrn_handle h, const hrn_canvas *canvases_host, int nframes, const float *pts_dev /* (n,J,3) or NULL */, int n, int J,
                   const int32_t *joints_host /* K indices */, int K, const int32_t *boxes_dev /* (n,4) or NULL */,
                   const int32_t *frame_index_host /* n entries; NULL: nframes == 1 */, float threshold, int scale_num, int scale_den,
                   int min_half /* 0: the rule */, int cell /* 0: the rule */, int32_t *status_dev /* n or NULL */, void *stream);
int hrn_mosaic_regions(const float *pts /* (n,J,3) or NULL, host */, int n, int J, const int32_t *joints /* K indices */, int K,
                       const int32_t *boxes /* (n,4) or NULL, host */, const int32_t *canvas_hw /* (n,2) */, float threshold,
                       int scale_num, int scale_den, int min_half, int32_t *regions_out /* (n,4) */, int32_t *status_out /* n */);
int hrn_mosaic_host(const hrn_canvas *canvases_host /* planes on the host */, int nframes, const float *pts_host, int n, int J,
                    const int32_t *joints_host, int K, const int32_t *boxes_host, const int32_t *frame_index_host, float threshold,
                    int scale_num, int scale_den, int min_half, int cell, int32_t *status_out /* n or NULL */);
const char *hrn_mosaic_last_error(void);
int hrn_yuv_from_bgr(int matrix, int range, const uint8_t *bgr /* (n,3) */, int n, uint8_t *yuv_out /* (n,3) */);

/* ---- the detector link on the GPU: the letterboxed detector tensor, and the detector's boxes back in frame coordinates ----
 * Replaces the host code AROUND an injected person detector (the network stays the caller's; its NMS is hrn_detector_nms_dev below):
 * models_/detectors/YOLOv3.py:23-76 (letterbox + prepare_data before the network, filter_classes + scale_coords after it) and
 * models_/detectors/YOLOv5.py:9-39, 88-98 (letterbox before; confidence / class filter and (x - dw) / ratio after).
 *
 * GEOMETRY (csrc/letterbox_math.h, one text for both rules; round = nearest, ties to even, on a double -- Python's round):
 *   HRN_LETTERBOX_MAX_SIDE   YOLOv3's letterbox(mode='square'): out_h == out_w == S; ratio = (double)S / max(h, w)
 *   HRN_LETTERBOX_MIN_RATIO  YOLOv5's letterbox(auto=False, scaleFill=False, scaleup=True): ratio = min((double)out_h / h,
 *                            (double)out_w / w); the output may be rectangular
 *   new_w = round(w * ratio), new_h = round(h * ratio); dw = (out_w - new_w) / 2.0, dh = (out_h - new_h) / 2.0;
 *   top = round(dh - 0.1), bottom = round(dh + 0.1), left = round(dw - 0.1), right = round(dw + 0.1).
 *   top + new_h + bottom == out_h and left + new_w + right == out_w (asserted).  new_w == 0 or new_h == 0 (a 1 x 200 frame at
 *   S = 64) fails with code 7: cv2.resize would raise there.
 * hrn_letterbox keeps the doubles `ratio` and dw / dh BEFORE rounding beside the integers: YOLOv5's inverse uses those.
 * hrn_letterbox_geometry needs no handle and no GPU; its failure text: hrn_letterbox_last_error().
 *
 * hrn_letterbox_frames / hrn_letterbox_frames_yuv: n frames (a host table of hrn_frame / hrn_yuv_frame, sizes may differ, as
 * in hrn_preprocess_frames; n <= 65535) to ONE detector tensor in ONE launch, no frame-sized scratch, one writer per byte.
 *   interior pixel   cv2.resize(frame, (new_w, new_h), INTER_LINEAR): bit for bit the arithmetic of hrn_resize_frames with
 *                    HRN_INTER_LINEAR (csrc/resize_taps.h is compiled into both kernels), plus the two cases that entry never meets:
 *                    new size == frame size: a copy (YOLOv5's wrapper skips the resize; cv2.resize copies);
 *                    frame_w == 2 * new_w and frame_h == 2 * new_h (every 1280 x 720 frame at 640): cv2.resize switches
 *                    INTER_LINEAR to its INTER_AREA fast path, (a + b + c + d + 2) >> 2 over the 2 x 2 block.
 *                    OpenCV is not available where this library is built and tested: all three are restated from the published
 *                    resize.cpp, the 2:1 rule without even a restating oracle of older standing; equality with a cv2 build is
 *                    NOT pinned (tests/golden/make_letterbox_golden.py makes the pin wherever opencv-python is installed).
 *   padding pixel    pad[c], c in OUTPUT channel order; no frame byte is read.  (The wrappers' 127.5 is 128 under cv2's
 *                    round-half-even saturation; YOLOv5 uses 114.)
 *   order            HRN_LB_RGB (what both wrappers feed the network) or HRN_LB_BGR
 *   form             HRN_LB_F32 / _F16 / _BF16: (n, 3, out_h, out_w) planar, value = (float)v / 255.0f (true float32 division:
 *                    torchvision's ToTensor), the 16-bit forms that float rounded to nearest even;
 *                    HRN_LB_U8_HWC: (n, out_h, out_w, 3) uint8, the byte itself
 *   YUV frames       every tap is read through the conversion of hrn_preprocess_frames_yuv: the result equals, bit for bit, the
 *                    BGR entry on the converted frame; padding is pad[], not a conversion of anything
 *   geometry_host    optional out: n hrn_letterbox
 * Code 7 and nothing launched, each failure naming its cause: an unknown rule / order / form, out_h or out_w outside
 * [1, 16384], MAX_SIDE with out_h != out_w, n < 0 or n > 65535, null tables, a frame that is null or malformed (the texts of
 * hrn_preprocess_frames / _yuv), a frame whose geometry fails, a plan-only handle.  n == 0 succeeds and launches nothing.
 *
 * BOXES BACK: hrn_detections_to_frame (host, no handle; failure text: hrn_letterbox_last_error()) and
 * hrn_detections_to_frame_dev (one launch, one 256-thread block per frame, stream-ordered, no host read).
 *   dets          (n, det_stride >= 5) float32 rows (x1, y1, x2, y2, ...) in LETTERBOX coordinates, after the detector's NMS
 *   start_host    P + 1 ascending row offsets on the HOST (start[0] = 0): frame p owns rows [start[p], start[p + 1])
 *   geometry_host / frame_hw_host   the P hrn_letterbox the forward call returned and the P (height, width) of the frames
 *   conf_col in [4, det_stride), conf_thres: a row is kept iff row[conf_col] >= conf_thres in float32 (-inf: everybody)
 *   class_col     column of the class id; negative counts from the end (detections[:, -1]); == det_stride: no class filter.
 *                 classes_host: nclasses <= 16 accepted ids; a row passes iff row[class_col] == (float)id for one of them
 *   status (n)    per INPUT row: 0 kept; 5 a coordinate or the confidence is not finite; else 1 below the threshold; else 2 other class
 *   inverse       MAX_SIDE (scale_coords): gain = (double)max(out_h, out_w) / max(h, w); pad_x = (out_w - w * gain) / 2,
 *                 pad_y = (out_h - h * gain) / 2 in double; each cast to float32; v' = max((v - pad) / gain, 0) in float32, for all
 *                 four coordinates (x2 / y2 are not cut to the frame, as in the reference; a negative result, and -0, become +0).
 *                 MIN_RATIO: v' = (v - (float)dw) / (float)ratio, no clamp.
 *                 The division is a TRUE float32 division, torch's CPU behaviour and the definition here; torch's GPU kernel
 *                 multiplies by a reciprocal, so the reference disagrees with itself by an ulp between devices.
 *   dets_out      a separate (n, det_stride) buffer (overlapping the input is refused).  A kept row: the four mapped coordinates,
 *                 every other column unchanged.  A row that is not kept: all zeros -- the "lost person" row
 *                 hrn_preprocess_frames_dev reports as status 1.  With HRN_DET_COMPACT the kept rows of a frame move to the front
 *                 of that frame's segment in their order and the zero rows follow; counts (P) = kept rows per frame either way. */
enum { HRN_LETTERBOX_MAX_SIDE = 0, HRN_LETTERBOX_MIN_RATIO = 1 };
enum { HRN_LB_F32 = 0, HRN_LB_F16 = 1, HRN_LB_BF16 = 2, HRN_LB_U8_HWC = 3 };
enum { HRN_LB_RGB = 0, HRN_LB_BGR = 1 };
enum { HRN_DET_COMPACT = 1 };
enum { HRN_DET_MAX_CLASSES = 16 };
typedef struct { int32_t new_w, new_h, left, top; double ratio_w, ratio_h, dw, dh; } hrn_letterbox;
int hrn_letterbox_geometry(int rule, const int32_t *frame_hw /* (n, 2) height, width */, int n, int out_h, int out_w,
                           hrn_letterbox *out /* n */);
const char *hrn_letterbox_last_error(void);
int hrn_letterbox_frames(hrn_handle h, const hrn_frame *frames_host, int n, int rule, int out_h, int out_w,
                         const uint8_t *pad /* 3 */, int order, int form, void *out_dev, hrn_letterbox *geometry_host /* n or NULL */,
                         void *stream);
int hrn_letterbox_frames_yuv(hrn_handle h, const hrn_yuv_frame *frames_host, int n, int rule, int out_h, int out_w,
                             const uint8_t *pad /* 3 */, int order, int form, void *out_dev,
                             hrn_letterbox *geometry_host /* n or NULL */, void *stream);
int hrn_detections_to_frame(int rule, const float *dets, int det_stride, const int32_t *start /* P + 1 */, int P,
                            const hrn_letterbox *geometry, const int32_t *frame_hw /* (P, 2) */, int out_h, int out_w,
                            int conf_col, float conf_thres, int class_col, const int32_t *classes, int nclasses, int flags,
                            float *dets_out, int32_t *counts_out /* P */, int32_t *status_out /* n */);
int hrn_detections_to_frame_dev(hrn_handle h, int rule, const float *dets_dev, int det_stride, const int32_t *start_host, int P,
                                const hrn_letterbox *geometry_host, const int32_t *frame_hw_host, int out_h, int out_w,
                                int conf_col, float conf_thres, int class_col, const int32_t *classes_host, int nclasses, int flags,
                                float *dets_out_dev, int32_t *counts_dev, int32_t *status_dev, void *stream);

/* ---- detector NMS: the raw output of a YOLO head to kept rows, on the host or without leaving the device ----
 * The step between the detector NETWORK and hrn_detections_to_frame: the reference takes it from non_max_suppression of its
 * YOLOv3 submodule (models_/detectors/YOLOv3.py:13,135) and from ultralytics' AutoShape, i.e. torchvision.ops.nms
 * (models_/detectors/YOLOv5.py:85-87).  hrn_detector_nms is the host form (no handle, no GPU; failure text:
 * hrn_detector_nms_last_error(), per thread); hrn_detector_nms_dev has every array in device memory, is stream-ordered, makes
 * no host read and equals the host form bit for bit on all four outputs.  csrc/detector_nms_math.h is the one text both compile:
 * float32 throughout, every operation rounded on its own (no FMA), no library call.
 *
 * INPUT   pred (B, N, 5 + C) contiguous, dtype HRN_F32 or HRN_F16 (widened to float32 exactly on load).  A row is
 *         cx, cy, w, h, obj, cls_0 .. cls_{C-1}.
 * BOX     x1 = cx - w / 2, y1 = cy - h / 2, x2 = cx + w / 2, y2 = cy + h / 2.
 * BEST    the FIRST maximum of the classes: best = 0, cls_conf = cls_0; for c = 1 .. C-1: if cls_c > cls_conf: best = c,
 *         cls_conf = cls_c.  (A NaN cls_0 stays; a NaN elsewhere is passed over; of -0 and +0 the first one stays.)
 * min / max below: max(a, b) = a > b ? a : b, min(a, b) = a < b ? a : b -- with a NaN operand the result is b.
 *
 * HRN_DNMS_YOLOV5  ultralytics' non_max_suppression with multi_label=False:
 *   candidate iff obj > conf_thres and conf = obj * cls_conf > conf_thres; the sort key is conf;
 *   the output row is x1, y1, x2, y2, conf, best: 6 floats;
 *   iw = max(min(ax2, bx2) - max(ax1, bx1), 0), ih likewise; inter = iw * ih; area = (x2 - x1) * (y2 - y1);
 *   iou = inter / (area_a + area_b - inter), a the kept box.
 *   Classes are separated by LABEL EQUALITY, not by ultralytics' `+ class * max_wh` offset of the boxes: on boxes of one class
 *   the offset only changes the rounding of an IoU that sits at the threshold, and boxes of two classes never overlap with it.
 * HRN_DNMS_YOLOV3  the YOLOv3 wrapper's non_max_suppression, its weighted merge included:
 *   candidate iff obj >= conf_thres; the sort key is obj * cls_conf;
 *   the output row is x1, y1, x2, y2 (merged), obj, cls_conf, best: 7 floats;
 *   the pixel convention: iw = max(min(ax2, bx2) - max(ax1, bx1) + 1, 0), ih likewise; area = (x2 - x1 + 1) * (y2 - y1 + 1);
 *   iou = inter / (area_a + area_b - inter + 1e-16f).
 *   The yolo submodule is not part of the reference tree: this rule is a definition of this library, written from the wrapper's
 *   call site and the published algorithm; parity with the submodule is UNPINNED.
 *
 * COMMON TO BOTH RULES
 *   A candidate whose key is NaN is dropped and sets status bit 2 of its image.
 *   The order is descending key; equal keys (-0 equals +0) go by ascending row: the order is stable and total.
 *   Only the first max_candidates of that order take part (ultralytics' max_nms); status bit 0: more rows qualified.
 *   The sweep is greedy in that order: a candidate is kept unless an earlier KEPT candidate of the same class (flag
 *   HRN_DNMS_AGNOSTIC: of any class) has iou > iou_thres with it.  A NaN IoU never suppresses.  The IoU is always taken on the
 *   original boxes.  The sweep stops after max_det kept rows; status bit 1: a candidate that is not suppressed remains after
 *   the last keeper.
 * THE YOLOV3 MERGE  Each kept row's box becomes sum(w_j * box_j) / sum(w_j), w = obj, over its merge set: the keeper itself,
 *   always, plus every candidate that was still alive when it was taken and that it suppressed -- in ascending order position,
 *   starting from the keeper's own term (acc = w * v; then acc = acc + w_j * v_j), float32, product and sum rounded separately.
 *   (The submodule loops forever on a keeper whose own IoU is NaN; here the keeper always leaves the list.)
 * A NaN in an output row is written as the quiet NaN 0x7FC00000, whatever payload the arithmetic left.
 *
 * OUTPUTS, all written for every image
 *   rows    (B, max_det, 6 | 7) float32, kept rows in sweep order; rows beyond the count are all zero
 *   index   (B, max_det) int32: the row of pred each kept row came from; -1 beyond the count
 *   counts  (B,) int32;  status (B,) int32: the bits above
 *
 * LIMITS: B >= 0; N in [0, 2^24]; C in [1, 4096]; max_candidates in [1, 4096]; max_det in [1, max_candidates]; conf_thres and
 * iou_thres finite; a known rule, dtype and flag bits; non-null outputs when B > 0, non-null pred when B * N > 0.  Anything else
 * is code 7 with its message, judged before anything is written or launched; then a plan-only handle is refused (code 7).
 *
 * THE DEVICE ENTRY: two launches, no atomics on global memory, one writer per output byte.  The scoring launch (256 rows per
 * block) reads pred once: the obj column first, the classes and the box only of rows whose obj passes, one wave per such row
 * with a lane per class; it leaves each block's candidates compacted in row order, with their count.  The per-image launch (one
 * block per image) scans the counts, selects the first max_candidates exactly when more qualified (a radix select over the key
 * bits, integer histogram counts in LDS; the equal keys at the cut by row), ranks the candidates by counting, then sweeps, merges
 * and writes with the candidates in LDS.  The scratch (32 bytes per row of pred, 8 per block of 256 rows) lives in the handle
 * and grows on demand; calls on different streams are serialised on it. */
enum { HRN_DNMS_YOLOV3 = 0, HRN_DNMS_YOLOV5 = 1 };
enum { HRN_DNMS_AGNOSTIC = 1 };
int hrn_detector_nms(const void *pred, int dtype, int B, int N, int C, int rule, int flags, float conf_thres, float iou_thres,
                     int max_candidates, int max_det, float *rows, int32_t *index, int32_t *counts, int32_t *status);
const char *hrn_detector_nms_last_error(void);
int hrn_detector_nms_dev(hrn_handle h, const void *pred_dev, int dtype, int B, int N, int C, int rule, int flags, float conf_thres,
                         float iou_thres, int max_candidates, int max_det, float *rows_dev, int32_t *index_dev,
                         int32_t *counts_dev, int32_t *status_dev, void *stream);

/* ---- frame rotation on the GPU: cv2.rotate for BGR, NV12 / NV21, I420, P010 and I010 frames, and people between the two orientations ----
 * Replaces `frame = cv2.rotate(frame, rotation_code)` at the head of the reference's frame loops (scripts/live-demo.py:102-103,
 * scripts/extract-keypoints.py:96-97; the code comes from the video's rotation tag, misc/visualization.py:271-293): a portrait
 * video is stored sideways, a hardware decoder hands over the stored orientation.  The codes are cv2.ROTATE_*'s values.
 *
 * THE PIXEL RULE.  cv2.rotate is a pure permutation of elements, np.rot90 its exact restatement.  A source plane has (Hs, Ws)
 * elements, dst(i, j) is the element of destination row i, column j:
 *   HRN_ROTATE_90_CW  (0)   dst is (Ws, Hs):  dst(i, j) = src(Hs-1-j, i)
 *   HRN_ROTATE_180    (1)   dst is (Hs, Ws):  dst(i, j) = src(Hs-1-i, Ws-1-j)
 *   HRN_ROTATE_90_CCW (2)   dst is (Ws, Hs):  dst(i, j) = src(j, Ws-1-i)
 * An element is: BGR -- the three bytes of a pixel, kept in order; the Y plane -- one byte; NV12's chroma plane -- the (U, V)
 * byte pair, on (H/2, W/2); I420 -- the U and the V plane, one byte each, on (H/2, W/2).  2 x 2 luma blocks map onto 2 x 2 blocks,
 * so converting a rotated YUV frame to BGR equals rotating the converted frame, bit for bit.
 * HRN_PIX_NV21 rotates as NV12 (its pair is (V, U)).  The 10-bit layouts: an element of a Y, U or V plane is the 16-bit word (2
 * bytes), of P010's chroma plane the (U, V) word pair (4 bytes); a word travels with all 16 bits, the ignored ones included.
 * Both sides of a 10-bit frame need even plane addresses and pitches (code 7: "odd plane address or pitch on a 10-bit frame").
 * Bytes of a destination row beyond its elements (pitch padding) are NOT written; every other byte of dst has exactly one writer;
 * no atomics; source planes are only read.
 *
 * hrn_rotate_frames: src_host / dst_host are nframes hrn_canvas entries each, on the HOST, planes on the device; frames may differ
 * in size, format and code (codes_host: nframes entries).  dst[k] has src[k]'s format and the rotated size, any pitch that
 * holds its rows; matrix and range are documentation only.  ONE launch whatever nframes, no frame-sized scratch, stream-ordered;
 * one block per 64 x 64-element tile of a plane (64 x 16 at 180 degrees), found through a per-call table (one frame: in the kernel arguments; more: uploaded
 * through the handle's guarded table and pinned ring).  The 90-degree codes go through an LDS tile of padded pitch: source rows are
 * read and destination rows written in whole dwords wherever a plane's base and pitch are multiples of 4, in bytes otherwise; 180
 * degrees reverses the elements of four-element groups in registers.  Offsets inside a plane are 32-bit.  nframes == 0 succeeds
 * and launches nothing.
 * Fails with code 7, names the cause and launches nothing on: nframes < 0; null tables with nframes > 0; a code outside {0, 1, 2};
 * formats that differ between src[k] and dst[k]; an unknown format; a null plane; a non-positive side; an odd side on a YUV frame;
 * a destination whose size is not the rotated size; a pitch below the row's bytes; a plane with pitch * rows >= 2^31; a source
 * and a destination, or two destinations, that name the same first plane (in-place rotation is not offered; overlapping views
 * are the caller's to avoid); after all these, a plan-only handle.  Everything is judged before the device is touched.
 *
 * PEOPLE BETWEEN THE TWO ORIENTATIONS (csrc/rotate_math.h, one text for host and device).  (Hs, Ws) is the SOURCE frame.  A joint
 * (y, x, c) is float32: each result is one float32 subtraction or a copy, c is copied; inf goes through the subtraction, a NaN
 * coordinate is copied with its bits (host and device then agree on its sign).  A box (x1, y1, x2, y2) is int32, a half-open pixel range (the slice hrn_crop_geometry cuts): the rotated box is
 * the range the rotated slice occupies; the all-zero box of a lost person stays all-zero.
 *   code 0:  y' = x;  x' = (float)(Hs-1) - y                     box (Hs - y2, x1, Hs - y1, x2)
 *   code 1:  y' = (float)(Hs-1) - y;  x' = (float)(Ws-1) - x     box (Ws - x2, Hs - y2, Ws - x1, Hs - y1)
 *   code 2:  y' = (float)(Ws-1) - x;  x' = y                     box (y1, Ws - x2, y2, Ws - x1)
 * There is no inverse flag: THE WAY BACK is code 2 - c with the ROTATED frame's (height, width); it returns every box and every
 * integer-valued joint exactly.
 * frame_hw: one (height, width) for everybody, or n of them (per_person_hw); codes: one, or n (per_person_code); pts (n, J, 3)
 * and / or boxes (n, 4) -- a null input skips its output; an output may be its input.
 * hrn_rotate_people: host, no handle; failure text: hrn_rotate_people_last_error().  hrn_rotate_people_dev: pts / boxes on the
 * device, sizes and codes on the HOST (per-person ones travel through the pinned ring); one launch, one thread per joint and
 * per box, stream-ordered; n == 0 launches nothing.
 * Code 7 for both, naming the cause: n < 0; J outside [1, HRN_MAX_JOINTS]; pts and boxes both null; an input without its output;
 * null sizes / codes with n > 0; a code outside {0, 1, 2}; a non-positive side; (device form, last) a plan-only handle. */
enum { HRN_ROTATE_90_CW = 0, HRN_ROTATE_180 = 1, HRN_ROTATE_90_CCW = 2 };   /* the values of cv2.ROTATE_* */
int hrn_rotate_frames(hrn_handle h, const hrn_canvas *src_host, const hrn_canvas *dst_host, int nframes,
                      const int32_t *codes_host /* nframes entries */, void *stream);
int hrn_rotate_people(int n, int J, const int32_t *frame_hw /* (n,2) or (1,2): the SOURCE frame */, int per_person_hw,
                      const int32_t *codes /* n or 1 */, int per_person_code,
                      const float *pts /* (n,J,3) or NULL */, const int32_t *boxes /* (n,4) or NULL */,
                      float *pts_out, int32_t *boxes_out);
const char *hrn_rotate_people_last_error(void);
int hrn_rotate_people_dev(hrn_handle h, int n, int J, const int32_t *frame_hw_host, int per_person_hw,
                          const int32_t *codes_host, int per_person_code, const float *pts_dev, const int32_t *boxes_dev,
                          float *pts_out_dev, int32_t *boxes_out_dev, void *stream);

/* ---- BGR frames back to 4:2:0 YCbCr on the GPU: NV12 / NV21, I420 and 10-bit P010 / I010 -- the annotated frame in the encoder's layout ----
 * The inverse direction of hrn_yuv_to_bgr, for a pipeline that draws on BGR (every pipeline whose frames start as BGR, and the
 * NV21 / P010 / I010 pipelines the overlays refuse): decode -> pose -> draw on BGR -> back to the stream's own layout -> an encoder,
 * a recorder or `ffmpeg -f rawvideo -pix_fmt nv12|nv21|yuv420p|p010le|yuv420p10le`.  On 8-bit output half the bytes cross PCIe.
 *
 * THE TABLE (csrc/yuv_fwd.h, one text for the host entries and the kernel).  hrn_yuv_forward_coefficients writes ten int32:
 * y0, CYR CYG CYB, CUR CUG CUB, CVR CVG CVB -- the rows (R, G, B) of Y, U and V at scale 2^20, q(x) = floor(x * 2^20 + 0.5) (the
 * rounding of hrn_yuv_coefficients) of the exact forward coefficients: Kr / Kb = 0.299 / 0.114 (BT.601) or 0.2126 / 0.0722
 * (BT.709), Kg = 1 - Kr - Kb; limited range sy = 219/255, sc = 224/255, y0 = 16; full range sy = sc = 1, y0 = 0:
 *   CYR = q(sy Kr)                  CYG = q(sy Kg)                  CYB = q(sy Kb)
 *   CUR = q(-sc Kr / (2 (1 - Kb)))  CUG = q(-sc Kg / (2 (1 - Kb)))  CUB = -(CUR + CUG)
 *   CVG = q(-sc Kg / (2 (1 - Kr)))  CVB = q(-sc Kb / (2 (1 - Kr)))  CVR = -(CVG + CVB)
 * Each chroma row sums to zero: a grey pixel gives exactly 128 / 512.  BT.601 limited follows the same rule; it is NOT OpenCV's
 * forward table (which is coarser and cannot be consulted where this library is tested): equality with
 * cv2.cvtColor(COLOR_BGR2YUV_I420) is NOT pinned, as with the other cv2 pins.
 *
 * THE PIXEL RULE.  All integers, arithmetic shift, one rounding each; every sum fits int32 (the largest is exactly 2^30).
 *   8-bit luma, per pixel:        Y = clip8 ((CYR R  + CYG G  + CYB B  + (y0  << 20) + (1 << 19)) >> 20)
 *   8-bit chroma, per 2x2 block:  U = clip8 ((CUR Rs + CUG Gs + CUB Bs + (128 << 22) + (1 << 21)) >> 22),  V likewise
 *   10-bit luma:                  Y = clip10((CYR R  + CYG G  + CYB B  + (y0  << 20) + (1 << 17)) >> 18)
 *   10-bit chroma:                U = clip10((CUR Rs + CUG Gs + CUB Bs + (128 << 22) + (1 << 19)) >> 20),  V likewise
 * Rs, Gs, Bs are the SUMS over the four pixels of the block (0 .. 1020): the chroma sample is the conversion of the block's mean
 * (MPEG-1 centre siting) -- a definition of this library, like the table.  The 10-bit samples come from the same 8-bit BGR with
 * one rounding, not from the 8-bit samples.  P010 stores s << 6 (the low six bits zero), I010 stores s (the high six bits zero),
 * NV21 is NV12 with the pair written (V, U).  In limited range no clip engages (Y in 16 .. 235, U, V in 16 .. 240; x 4 for 10 bits);
 * in full range exactly two values meet one: pure blue's U and pure red's V are 256 before the 8-bit clip (128 + 127.5).
 * PINNED (tests/bgr2yuv_ref.py, tests/test_bgr2yuv_*.py), over all 2^24 colours and the four tables: a block of four equal pixels
 * converts as one pixel; Y, U, V are within 1 of hrn_yuv_from_bgr's float64 formula; through hrn_yuv_to_bgr's 8-bit form a
 * uniform block comes back within 2 levels in B and 1 in G and R (limited) or 1 in all three (full); through its 10-bit form
 * exactly, except B within 1 for BT.601 limited (OpenCV's inverse table is not an exact inverse); |s10 - 4 s8| <= 2.
 *
 * hrn_bgr_to_yuv_blocks (no handle, no GPU): the host form -- n 2x2 blocks, (n, 4, 3) uint8 (B, G, R) of the four pixels
 * row-major, to (n, 6) uint16 sample values Y00 Y01 Y10 Y11 U V (not shifted: 0 .. 255 or 0 .. 1023); depth is 8 or 10.
 * Both return 7 on an unknown matrix or range (the blocks: also depth, n < 0, null arrays with n > 0).
 *
 * hrn_bgr_to_yuv_frames follows hrn_rotate_frames' contract: src_host / dst_host are nframes hrn_canvas entries each, on the
 * HOST, planes on the device.  src[k] is an HRN_PIX_BGR canvas (pitched views are allowed); dst[k] is any of the five YUV
 * layouts, of the same size, any pitch that holds its rows; its matrix and range fields are READ here: they choose the table.
 * Frames of one call may differ in size, format, matrix and range.  ONE launch whatever nframes, no frame-sized scratch,
 * stream-ordered, no atomics; one block per 256 x 8-pixel tile of a frame, found through a per-call table (one frame: in the
 * kernel arguments; more: uploaded through the handle's guarded table and pinned ring).  A thread owns 2 rows x 4 pixels: three
 * dword loads per row, one dword of Y per row (two for 10 bits) and its two chroma samples in one dword (NV12 / NV21; I010: one per
 * plane; P010: two; I420: one 16-bit store per plane) wherever a plane's base and pitch are multiples of 4, bytes (16-bit words for
 * 10 bits) otherwise and for the 2-pixel group that ends a row whose width is not a multiple of 4.  Every destination byte that
 * belongs to a sample has exactly one writer; pitch padding is never written; sources are only read.  Offsets inside a plane are
 * 32-bit.  nframes == 0 succeeds and launches nothing.
 * Fails with code 7, names the cause and launches nothing on: nframes < 0; null tables with nframes > 0; a source that is not
 * BGR; a destination with an unknown format (0, 3, 7, ...), matrix or range; a null plane; a non-positive, odd or over-8192
 * side; sizes that differ between src[k] and dst[k]; a pitch below the row's bytes; a plane with pitch * rows >= 2^31; an odd
 * plane address or pitch on a 10-bit destination; a source and a destination, or two destinations, that name the same first
 * plane (overlapping views are the caller's to avoid); after all these, a plan-only handle.  Everything is judged before the
 * device is touched.
 * NOT BUILT: 4:2:2 / 4:4:4 output, dithering, HDR transfer functions, a fused draw + convert; the overlays still refuse NV21,
 * P010 and I010 canvases. */
int hrn_yuv_forward_coefficients(int matrix, int range, int32_t out[10]);
int hrn_bgr_to_yuv_blocks(int matrix, int range, int depth /* 8 | 10 */, const uint8_t *bgr /* (n,4,3): a 2x2 block, row-major */,
                          int n, uint16_t *out /* (n,6): Y00 Y01 Y10 Y11 U V, sample values */);
int hrn_bgr_to_yuv_frames(hrn_handle h, const hrn_canvas *src_host, const hrn_canvas *dst_host, int nframes, void *stream);

/* Single-person pre-path on the GPU: replaces, for every frame of a call with multiperson=False,
 *   cv2.resize(image, (W, H), interpolation=self.interpolation); cv2.cvtColor(image, cv2.COLOR_BGR2RGB); self.transform(image)
 * (SimpleHRNet.py:213-222 for one frame, :355-366 for a stack; default interpolation cv2.INTER_CUBIC, :27) and writes the
 * (n,3,H,W) fp32 batch hrn_forward reads.  The boxes of this path are the whole frame: [0, 0, frame_w, frame_h] (:223, :369).
 *   frames_dev     (n, frame_h, frame_w, 3) uint8 BGR, device
 *   interpolation  HRN_INTER_* = the cv2.INTER_* value of the same name; anything else fails (the reference would pass it on)
 * OpenCV is not available where this library is built and tested: the arithmetic follows the published generic 8-bit path of
 * modules/imgproc/src/resize.cpp (oracle/cv2_resize_oracle.py restates it, the kernel equals that restatement bit for bit);
 * equality with a given cv2 build -- IPP / OpenCL builds differ among themselves -- is NOT pinned.  Specifically, for
 * HRN_INTER_CUBIC this is OpenCV's SCALAR cubic path (float32 coefficients, saturate_cast<short>(c * 2048), one rounding after
 * the vertical pass); the SIMD (AVX2 / NEON) builds shipped in the opencv-python wheels round the vertical pass differently and
 * can differ from it by +-1 grey level per sample (nearest and linear are bit-equal).  A deployment that needs equality with ITS
 * cv2 checks it there: tests/golden/make_cv2_golden.py produces the fixture wherever opencv-python is installed. */
enum { HRN_INTER_NEAREST = 0, HRN_INTER_LINEAR = 1, HRN_INTER_CUBIC = 2 };
int hrn_resize_frames(hrn_handle h, const uint8_t *frames_dev, int n, int frame_h, int frame_w, int interpolation,
                      float *images_dev, void *stream);

/* Evaluation pre-path on the GPU: replaces, for every person of a batch of the dataset path (testing/Test.py through
 * datasets/COCO.py:290-304; misc/utils.py:99-107 is the same call),
 *   trans = get_affine_transform(center, scale, pixel_std, rot, image_size)           (misc/utils.py:46-75)
 *   image = cv2.warpAffine(image, trans, (W, H), flags=cv2.INTER_LINEAR); image = ToTensor + Normalize
 * and writes the (n,3,H,W) fp32 batch hrn_forward / hrn_forward_flip_tta read: the frames cross PCIe once as uint8.
 *   frames_dev        (nframes, frame_h, frame_w, 3) uint8 BGR, device (sides up to 32 766: OpenCV saturates coordinates to int16)
 *   frame_index_host  n entries on the HOST: the frame crop i is cut from; NULL: crop i reads frame i (nframes == n) or
 *                     frame 0 (nframes == 1)
 *   matrices_host     (n, 6) float64 on the HOST: the FORWARD 2x3 matrices (frame -> crop), row-major, as
 *                     get_affine_transform(..., inv=0) returns them (postproc.affine_matrix)
 *   images_dev        out: (n,3,H,W) float32, device.  Any n: it is not bounded by max_batch.
 * The arithmetic is warpAffine's classic 8-bit INTER_LINEAR path, integer throughout:
 *   the matrix is inverted in float64 as cv::warpAffine does (D = M0*M4 - M1*M3; D = 1/D; A11 = M4*D; A22 = M0*D; M0 = A11;
 *   M1 *= -D; M3 *= -D; M4 = A22; b1 = -M0*M2 - M1*M5; b2 = -M3*M2 - M4*M5; M2 = b1; M5 = b2 -- no fused multiply-add);
 *   X = (rint((M1*y + M2) * 1024) + 16 + rint(M0*x * 1024)) >> 5, Y likewise with M4, M5 and M3 (1/32 pixel, rint = round half
 *   to even); sx = X >> 5, fx = X & 31, likewise sy, fy;
 *   v = (p00*(32-fx)*(32-fy) + p01*fx*(32-fy) + p10*(32-fx)*fy + p11*fx*fy + 512) >> 10 per channel, every tap outside the frame
 *   reading 0 (BORDER_CONSTANT, value 0: the reference passes no border arguments); then BGR -> RGB, v / 255, (x - mean) / std
 *   in float32 as hrn_resize_frames.
 * Fails (code 7, nothing launched) on a plan-only handle, n < 0, a frame side above 32 766, a frame index outside [0, nframes),
 * and a matrix that is not finite, is singular (the reference would sample one pixel everywhere), or maps a corner of the crop
 * further than 2^20 pixels from the frame's origin (the fixed point would overflow).
 * OpenCV is not available where this library is built and tested: tests/warp_affine_ref.py restates the arithmetic above and
 * the kernel equals that restatement bit for bit; parity with a cv2 build is NOT pinned (newer releases carry float warpAffine
 * kernels).  tests/golden/make_warp_golden.py produces the fixture wherever opencv-python is installed. */
int hrn_warp_crops(hrn_handle h, const uint8_t *frames_dev, int nframes, int frame_h, int frame_w,
                   const int32_t *frame_index_host, const double *matrices_host, int n, float *images_dev, void *stream);

/* Flip test-time augmentation + evaluation decode (testing/Test.py:132-140,
 * training/COCO.py:206-230, misc/utils.py:9-29 flip_tensor / flip_back, :125-151 get_max_preds, :154-175 the
 * post-processing of get_final_preds):
 *   heatmaps = (model(images) + flip_back(model(flip(images)), flip_pairs)) * 0.5      -> heatmaps_dev (n,J,h,w)
 *   preds    = arg-max of each map as (x, y) in heat-map pixels, zero where the maximum is <= 0, moved a quarter
 *              pixel towards the higher neighbour when post_processing != 0            -> preds_dev (n,J,2)
 *   maxvals  = the maxima                                                              -> maxvals_dev (n,J)
 * flip_pairs_host: npairs x 2 joint indices that swap under mirroring (COCO: datasets/COCO.py:113), each in
 * [0, nof_joints) -- anything else fails with code 7 and nothing launched; any number of pairs up to the table of
 * HRN_MAX_JOINTS joints.  Pairs that share a joint compose in order, as flip_back's in-place swaps do.  The inverse
 * affine of get_final_preds (transform_preds, cv2) stays with the caller. */
int hrn_forward_flip_tta(hrn_handle h, const void *images_dev, int n, const int32_t *flip_pairs_host, int npairs,
                         int post_processing, float *heatmaps_dev, float *preds_dev, float *maxvals_dev, void *stream);

/* ---- scoring an evaluation batch: Gaussian targets, loss and PCK (testing/Test.py:141-157, training/COCO.py `_val`) ----
 * The two numbers Test.py prints per batch, `loss_fn(output, target, target_weight)` and `ds.evaluate_accuracy(output, target)`,
 * from heat-maps that stay on the device.
 *
 * Targets (datasets/COCO.py:460-515, `_generate_target`; heatmap_type 'gaussian'), per person and joint, from joints in CROP
 * pixels (float64, after affine_transform: COCO.py:298-300 = postproc.joints_to_crop) and their visibility, with
 * h = height / 4, w = width / 4, t = 3 * sigma:
 *   mu = int(joint / 4 + 0.5) in float64, truncated towards zero (feat_stride = image_size / heatmap_size = 4);
 *   weight = visibility, set to 0 when mu_x - t >= w or mu_y - t >= h or mu_x + t + 1 < 0 or mu_y + t + 1 < 0;
 *   when weight > 0.5 the cells (x, y) of the map with |x - mu_x| <= t and |y - mu_y| <= t receive
 *   g[(x - mu_x)^2 + (y - mu_y)^2], everything else is 0; target_weight = weight * joints_weight[j] (float32) when given.
 *   A QUIRK KEPT: the test is `br < 0`, not `<= 0` -- a joint with mu = -(t + 1) on an axis keeps its weight although its
 *   window misses the map: an all-zero target that enters the loss with full weight.
 *   The table is this library's: g[d2] = float32(exp(-double(d2) / (2 sigma^2))), d2 = 0 .. 2 t^2, evaluated in float64 on the
 *   host and rounded once (kept in the handle per sigma).  The reference evaluates numpy's float32 SIMD exp, which is not
 *   correctly rounded and differs between numpy builds (1 ulp at sigma 2, up to 3 ulp at sigma 3 where this was written), so
 *   the pin against it is "same support, values within a measured number of ulps", not bit equality.
 * hrn_target_centers (no handle, host only): mu_out (n,J,2) int32 (x, y); draw_out (n,J) the weight before joints_weight;
 *   target_weight_out (n,J); each may be NULL.  height / width: the crop resolution.  Errors: hrn_last_error(NULL).
 * hrn_generate_targets: the (n,J,h,w) fp32 target maps on the device (for inspection, and for tests of the analytic mode cell
 *   by cell) and target_weight_host (n,J) (may be NULL). */
int hrn_target_centers(const double *joints, const float *vis, const float *joints_weight /* J or NULL */, int n, int J,
                       int height, int width, double sigma, int32_t *mu_out, float *draw_out, float *target_weight_out);
int hrn_generate_targets(hrn_handle h, const double *joints_host, const float *vis_host, const float *joints_weight_host,
                         int n, double sigma, float *targets_dev, float *target_weight_host, void *stream);
/* hrn_score_heatmaps: one pass over heatmaps_dev (n,J,h,w) fp32 (what hrn_forward / hrn_forward_flip_tta write), then one
 * small kernel.  Every field of hrn_score_out is a DEVICE pointer the caller provides:
 *   map_loss (n,J) fp64   L[i][j] = 0.5 / (h*w) * sum_p (double(o) * w - double(t) * w)^2, w = target_weight[i][j], every term
 *                         and the sum in fp64, in an order fixed by (h, w): the same bits for a map in any batch, at any
 *                         position, in both target modes
 *   loss_mse fp64         mean(L) = JointsMSELoss(use_target_weight=True) (losses/loss.py:20-54)
 *   loss_ohkm fp64        mean over persons of the mean of the ohkm_topk largest L[i][:] = JointsOHKMMSELoss
 *                         (losses/loss.py:6-16, 73-92, with the module-level ohkm its forward means); NaN when ohkm_topk <= 0
 *   preds, target_preds (n,J,2) fp32   get_max_preds (misc/utils.py:125-151): (x, y) of the first maximum (a NaN is a maximum,
 *                         as torch.max has it), (0, 0) where the maximum is not > 0
 *   maxvals (n,J) fp32    the maxima of the output maps
 *   dists (J,n), acc (J), avg_acc fp32, cnt int32   calc_dists / dist_acc / evaluate_pck_accuracy (misc/utils.py:185-244) in
 *                         float32 with the reference's operations: norm = (h / 10, w / 10) -- x is divided by h / 10 and y by
 *                         w / 10, as written there --, dist = sqrt(dx*dx + dy*dy) of the normalised differences (no fused
 *                         multiply-add) when target_x > 1 and target_y > 1, else -1; acc[j] = count(d < pck_thr) /
 *                         count(d != -1) or -1; avg_acc = mean of the acc[j] >= 0 (0 when there is none), cnt their number
 * Target source, exactly one of:
 *   analytic  joints_host (n,J,2) float64 + vis_host (n,J) [+ joints_weight_host (J)] + sigma: t is the Gaussian above, looked
 *             up in the table; nothing of target size is read or written.  target_preds = mu clamped to the map where the
 *             window is drawn and meets the map, else (0, 0) -- the arg-max of that target map.
 *   maps      targets_dev (n,J,h,w) fp32 + target_weight_host (n,J) as the dataset returns them (sigma is not read): any
 *             tensor of that shape, e.g. another engine's heat-maps; its arg-max is taken in the same pass.
 * Stream-ordered like hrn_forward (no synchronise inside), any n >= 0 (not bounded by max_batch; n = 0 gives NaN losses and
 * cnt 0); the staging and the table live in the handle: nothing is allocated after the first call of a size class.
 * Fails (code 7, nothing launched) on: a plan-only handle, n < 0, both or neither target source, maps that are not 16-byte
 * aligned, sigma <= 0 or 3 * sigma not an integer (this library's restriction; the reference's configurations use 1, 2, 3), a
 * joint that is not finite or whose joint / 4 + 0.5 does not fit an int32 (the reference's int() raises there), ohkm_topk > J,
 * pck_thr not finite, a NULL field of hrn_score_out (the per-person arrays may be NULL when n is 0). */
typedef struct {
    double *loss_mse, *loss_ohkm;
    float *avg_acc;
    int32_t *cnt;
    float *acc, *dists;
    double *map_loss;
    float *preds, *target_preds, *maxvals;
} hrn_score_out;
int hrn_score_heatmaps(hrn_handle h, const float *heatmaps_dev, int n, const float *targets_dev, const double *joints_host,
                       const float *vis_host, const float *joints_weight_host, double sigma, const float *target_weight_host,
                       float pck_thr, int ohkm_topk, const hrn_score_out *out_dev, void *stream);

/* Sub-pixel joint decoding (opt-in; hrn_forward keeps the integer arg-max of SimpleHRNet.py:297-308).  Each mode works on
 * one raw heat-map H (h x w fp32, as the head writes it) and its integer arg-max (px, py) -- the first maximum of the
 * unsmoothed map -- and moves it by an offset (ox, oy) in cells:
 *   HRN_REFINE_NONE     no offset: bit-identical to hrn_forward.
 *   HRN_REFINE_QUARTER  get_final_preds's rule (misc/utils.py:154-175; hrn_forward_flip_tta's post_processing): when
 *                       1 < px < w-1 and 1 < py < h-1, ox = sign(H[py][px+1] - H[py][px-1]) * 0.25, oy likewise.
 *   HRN_REFINE_DARK     distribution-aware decoding (DARK, Zhang et al., CVPR 2020), when 2 <= px <= w-3 and 2 <= py <= h-3:
 *                       B = H blurred by the separable 11-tap Gaussian g[k] = exp(-k^2/8) / sum, k = -5..5 (sigma 2,
 *                       cv2.getGaussianKernel(11, 0)), H = 0 outside the map; L = ln(max(B, 1e-10)); central differences
 *                       dx = (L(1,0) - L(-1,0))/2, dxx = (L(2,0) - 2L(0,0) + L(-2,0))/4, dy / dyy likewise,
 *                       dxy = (L(1,1) - L(1,-1) - L(-1,1) + L(-1,-1))/4; offset = -Hess^-1 (dx, dy), applied only when the
 *                       Hessian is negative definite (dxx < 0, det > 0), each component clamped to [-1, 1].  DarkPose's
 *                       max(H)/max(B) rescaling is left out: a positive factor does not change the derivatives of L.
 *                       Evaluated in fp64.  (The definiteness test and the clamp are this library's: on near-flat maps an
 *                       unguarded Newton step can be arbitrarily large.)
 * Joints: y = (py + oy) / h * (y2 - y1) + y1, x likewise, in fp64 as hrn_forward; the confidence stays the raw maximum. */
enum { HRN_REFINE_NONE = 0, HRN_REFINE_QUARTER = 1, HRN_REFINE_DARK = 2 };
/* hrn_forward with a refine mode: the same arguments, pts_dev required unless refine is HRN_REFINE_NONE (which IS
 * hrn_forward).  The head then writes heat-maps -- to heatmaps_dev when given, otherwise to a scratch buffer of max_batch
 * crops the handle allocates on its first refined call without heatmaps_dev -- and the decode reads them; same launch count. */
int hrn_forward_refined(hrn_handle h, const void *images_dev, int n, const void *boxes_dev, int box_dtype, int refine,
                        float *pts_dev, float *heatmaps_dev, void *stream);
/* The offset alone, in heat-map space (DARK on hrn_forward_flip_tta's averaged maps; synthetic maps in tests):
 *   heatmaps_dev  (n,J,h,w) fp32 of this handle's shape
 *   coords_dev    (n,J,2) (x, y), integer-valued on entry (e.g. hrn_forward_flip_tta with post_processing = 0), refined
 *                 in place; an entry outside [0, w-1] x [0, h-1] is left as it is.  HRN_REFINE_NONE changes nothing. */
int hrn_refine_coords(hrn_handle h, const float *heatmaps_dev, int n, int refine, float *coords_dev, void *stream);

/* Greedy IoU non-maximum suppression -- the reference's only native component:
 * `void _nms(int *keep_out, int *num_out, const float *boxes_host, int boxes_num, int boxes_dim, float thresh,
 * int device_id)` (misc/nms/gpu_nms.hpp; kernel misc/nms/nms_kernel.cu:33-77, caller misc/nms/gpu_nms.pyx:19-34).
 * Same contract: boxes sorted by score descending, rows [x1,y1,x2,y2,score,...], IoU with the +1 pixel convention,
 * a box is dropped when its IoU with an earlier kept box is > thresh; keep_out receives the kept row indices in
 * order, *num_out their count.  Needs no handle.  Returns 0 or an error code (hrn_nms_last_error()). */
/* SYNCHRONOUS like the reference's _nms (host boxes in, host indices out: two blocking copies on the default stream around
 * the kernels) -- it is the one entry point of this ABI that is not stream-ordered.  At most 65536 boxes (the n x n/64
 * suppression mask is the scratch that grows quadratically: 512 MiB there); the caller's current device is restored.
 * Scratch is kept per device between calls (the reference allocates and frees per call); hrn_nms_release(device_id) frees
 * it (device_id < 0: on every device). */
int hrn_nms(int32_t *keep_out, int32_t *num_out, const float *boxes_host, int boxes_num, int boxes_dim,
            float nms_overlap_thresh, int device_id);
int hrn_nms_release(int device_id);
const char *hrn_nms_last_error(void);

/* ---- pose post-processing on the host (O(people^2 * joints) on a handful of skeletons: host code in the reference,
 * host code here; numpy's float64 / float32 arithmetic and summation order reproduced) ------------------------------
 * OKS non-maximum suppression, misc/nms/nms.py:97-122 (`oks_nms`) and :138-180 (`soft_oks_nms`; at most 20 kept, gaussian
 * rescoring), called per image by datasets/COCO.py:371-374.  kpts: n x J x (x, y, score) float64 (`keypoints.flatten()`),
 * order: the indices by descending score (`scores.argsort()[::-1]`, done by the caller with numpy as the reference does),
 * sigmas: J values or NULL for COCO's 17, in_vis_thre: NaN for None.  keep_out (n entries) receives the kept indices. */
int hrn_oks_nms(int32_t *keep_out, int32_t *num_out, const double *kpts, const double *areas, const int32_t *order, int n, int J,
                double thresh, const double *sigmas, double in_vis_thre);
int hrn_soft_oks_nms(int32_t *keep_out, int32_t *num_out, const double *kpts, const double *areas, const double *scores_sorted,
                     const int32_t *order, int n, int J, double thresh, const double *sigmas, double in_vis_thre);
/* Tracker, misc/utils.py:372-384 (`compute_similarity_matrices`: box IoU :318-334 and OKS :341-369 of every current
 * skeleton against every previous one).  boxes: n x (x1, y1, x2, y2) as float64 (exact for the int32 boxes of the
 * multi-person path), poses: n x J x (y, x, confidence) float32 as predict() returns them; outputs na x nb float32. */
int hrn_pose_similarity(const double *boxes_a, const float *poses_a, int na, const double *boxes_b, const float *poses_b, int nb, int J,
                        float *sim_bbox, float *sim_pose);
/* The optimal assignment `munkres.Munkres().compute(cost)` returns (misc/utils.py:406-407): minimum total cost, every
 * row matched when rows <= cols, otherwise every column; row_to_col[r] = column or -1. */
int hrn_assignment(const double *cost, int rows, int cols, int32_t *row_to_col);

/* Debug tap -- test infrastructure hook for the per-stage parity tests (tests/test_bf16_pin.py), never needed in production.
 * The reference's counterpart is a forward hook on a sub-module (`module.register_forward_hook`, torch.nn.Module): the value
 * of an intermediate of HRNet.forward (models_/hrnet.py:157-189).  A tap is a tensor some launch of the pass writes to HBM:
 *   "stem"                       conv1 + bn1 + ReLU (hrnet.py:158-160)
 *   "<state_dict prefix>"        every convolution, e.g. "layer1.0.conv3", "stage3.1.branches.2.0.conv2",
 *                                "stage4.0.fuse_layers.3.0.2.0", "transition2.2.0.0": its output after the folded BatchNorm,
 *                                the residual and the ReLU, as stored (bf16 engine: the stored bf16 values, widened exactly)
 *   "<stage>.fuse.<i>"           the i-th output of a StageModule (hrnet.py:60-69), e.g. "stage3.2.fuse.0"
 * hrn_forward_tap runs ONE micro-batch (1 <= n <= max_batch) and copies crops crop0, crop0 + crop_step, ... (ncrops of them)
 * of the named tensor to dst_dev as (ncrops, C, H, W) fp32 right after the launch that completes it; heatmaps_dev
 * (n,J,h,w) may be NULL.  A tensor
 * the plan keeps on-chip at this batch size (conv1 of a fused BasicBlock; the projection shortcut of layer1.0) has no tap:
 * the call fails and says so. */
typedef struct {
    char name[96];
    int32_t c, h, w;
    int32_t conv_index;   /* index for hrn_get_conv_info, or -1 (stem / fuse outputs) */
} hrn_tap_info;
int hrn_tap_count(hrn_handle h);
int hrn_get_tap_info(hrn_handle h, int index, hrn_tap_info *out);
int hrn_forward_tap(hrn_handle h, const void *images_dev, int n, const char *tap_name, int crop0, int ncrops, int crop_step,
                    float *dst_dev, float *heatmaps_dev, void *stream);

/* Introspection used by tests, bench.py and the roofline accounting. */
int hrn_conv_count(hrn_handle h);
int hrn_get_conv_info(hrn_handle h, int index, hrn_conv_info *out);
double hrn_flops_per_crop(hrn_handle h);            /* 2*MAC, convolutions only              */
int64_t hrn_workspace_bytes(hrn_handle h);
/* Block maps / descriptor arrays built and uploaded since the handle was created.  They depend on the micro-batch size
 * only; the handle keeps the four most recent sizes, so a call pattern that alternates a few sizes (every predict() whose
 * n is not a multiple of max_batch: SimpleHRNet.py:285-294 runs a short last chunk) stops rebuilding after its first
 * pass over each size -- the test of that property reads this counter. */
int64_t hrn_map_rebuilds(hrn_handle h);
/* The number of entries of the static launch list (grouped launches count once).  A small call may issue more kernels: a
 * stride-2 slab group with too few tiles runs its convolutions on the generic kernel (one or more launches), a debug tap adds one. */
int hrn_launches_per_pass(hrn_handle h);
/* 1 when the handle runs the stem (conv1 + bn1 + ReLU + conv2 + bn2 + ReLU, models_/hrnet.py:158-163) as ONE kernel that
 * keeps conv1's output in LDS (bf16 HRNet handles whose crop width fits; bit-identical to the two launches, which remain
 * the path of hrn_forward_tap("stem") and of HRN_DISABLE_STEM_FUSE=1); hrn_launches_per_pass counts it as one launch. */
int hrn_stem_fused(hrn_handle h);
/* 1 when convolution `index` (hrn_get_conv_info numbering; algo 3 = the 96-cout form of the BasicBlock kernel) enumerates REAL
 * pixels only: its M tiles are runs of h * w * n pixels in (image, row, column) order instead of runs of flat rows of the padded
 * layout, so no matrix instruction is spent on the pad column / pad row (9 % of the 24x18 grid, 17 % of 12x9).  Same input layout,
 * same arithmetic per output pixel: bit-identical to the flat enumeration (HRN_DISABLE_COMPACT=1). */
int hrn_conv_compact(hrn_handle h, int index);
/* The HRN_* environment switches (same-box A/B runs, bit-identity tests) this handle saw when it was
 * created, as "NAME=value;..." -- always "" in production: the library ignores every HRN_* variable unless the process opts in
 * with HRN_DEBUG_ENV=1 (the test suite, tools/ab.sh).  Then they are read at hrn_create only, never during a call. */
const char *hrn_switches(hrn_handle h);
/* Debug: the number of elements at pad / guard positions of the activation workspace that are not zero (synchronises the
 * device; -1 on error or on a plan-only handle).  The layout's invariant -- every 3x3 convolution's zero padding is the pad
 * column / pad row shared by neighbouring rows and images, written as zeros or never touched by every kernel -- says 0 after
 * any sequence of calls; the GPU tests check it after every path of the engine has run. */
int64_t hrn_debug_pad_violations(hrn_handle h);
/* Block map of the `group`-th grouped BasicBlock launch for a call of n crops, as the host would upload it (works on
 * plan-only handles: the CPU tests check that every (conv, cout tile, M tile) is covered exactly once).  Per block six
 * int32: descriptor, cout tile, M tiles walked, first M tile, pixels per M tile, flags (1 = fused BasicBlock, 2 =
 * small tiles).  members[d] = convolution index of descriptor d (+ 2^30: the fused form, which also computes
 * the block's conv2).  Returns the number of blocks (may exceed capacity), -1 for a bad group / n. */
int hrn_plan_block_map(hrn_handle h, int group, int n, int reverse, int32_t *blocks, int capacity, int32_t *members,
                       int member_capacity);
/* Likewise for the `group`-th grouped launch of the generic kernel: per block three int32 (descriptor, cout tile, M tile;
 * M tiles past the end are alignment padding and return at once), members[d] = convolution index, *pixels_per_tile =
 * 64 * (fragments per wave chosen for n). */
int hrn_plan_direct_map(hrn_handle h, int group, int n, int32_t *blocks, int capacity, int32_t *members, int member_capacity,
                        int32_t *pixels_per_tile);
/* Likewise for the `group`-th launch of the stride-2 slab kernel (conv_s2.hip): per block three int32 (problem, tiles walked,
 * first tile; a tile = `rows` output rows of one image, numbered image-major); per part five int32 (problem, convolution
 * index, 48-cout tile of it, output rows per tile, tiles per image); *active = 1 when a call of n crops takes this kernel
 * (0: too few tiles, the same convolutions run on the generic kernel).  Returns blocks | (parts << 20), -1 for a bad group / n.
 * group = -1: the fused stem kernel's map (hrn_stem_fused; stem_fused.hip): conv2 with ONE output row per tile, two parts of 32
 * couts, at most one block per CU, every block an equal run of tiles. */
int hrn_plan_s2_map(hrn_handle h, int group, int n, int32_t *blocks, int capacity, int32_t *parts, int part_capacity,
                    int32_t *active);
/* The head / decode split of a call of n crops (works on plan-only handles): returns the number of slabs a heat-map is cut
 * into, *slab_px = pixels per slab (1024, or 256 for a call of a few crops); -1 for a bad handle / n. */
int hrn_plan_head_slabs(hrn_handle h, int n, int32_t *slab_px);
/* Where a grouped launch sits in a pass and how its blocks loop (works on plan-only handles).  kind 0: the `index`-th grouped
 * BasicBlock launch (hrn_plan_block_map numbering); kind 1: the `index`-th launch of the layer1 chain kernel.  out[0] = position
 * in the launch list, out[1] = 1 when a pass walks this launch's tensors backwards (every odd position; pass it to
 * hrn_plan_block_map as `reverse`); kind 1 also: out[2] = waves of the launch of a call of n crops (persistent blocks x waves per
 * block), out[3] = 16-pixel fragments they share by a grid-stride loop, out[4] = the kernel form (0: conv3 + the next conv1,
 * 1: with the projection shortcut, 2: with the 3x3 in front, 3: that on a layer's last block).  `out` holds five int32.
 * Returns 0, -1 for a bad kind / index / n. */
int hrn_plan_launch_walk(hrn_handle h, int kind, int index, int n, int32_t *out);
/* per-kernel HIP-event timing of one pass (dominant-kernel roofline in bench.py):
 * runs one micro-batch of n crops and returns, for conv i, its device time in ms. */
int hrn_profile_pass(hrn_handle h, const void *images_dev, int n, float *conv_ms, int conv_ms_len,
                     float *other_ms /* [4]: stem, fuse, head, decode */, void *stream);
const char *hrn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HRNET_MI355_H */
