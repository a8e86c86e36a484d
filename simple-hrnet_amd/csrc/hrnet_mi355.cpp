// Host runtime of the MI355X-native HRNet hot path: graph compiler (static launch list for a given
// width c / resolution), BatchNorm folding + MFMA-fragment weight packing, workspace planner and the
// C ABI declared in include/hrnet_mi355.h.  Graph follows models_/hrnet.py:157-189 (HRNet.forward),
// :55-71 (StageModule.forward) and models_/modules.py:20-40,56-72 of the reference.
#include "../../include/hrnet_mi355.h"

#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "assoc_math.h"
#include "tracks_math.h"
#include "letterbox_math.h"
#include "pose_nms_math.h"
#include "detector_nms_math.h"
#include "draw_labels_math.h"
#include "heat_math.h"
#include "mosaic_math.h"
#include "keypoint_eval_math.h"
#include "kernels.h"
#include "rotate_math.h"
#include "temporal_math.h"
#include "track_geometry.h"
#include "yuv_fwd.h"

namespace {
#include "ctx_types.h"
}  // namespace

namespace {
// hrn_env() (kernels.h) + a record of what was found: hrn_create copies it into the handle (hrn_switches)
thread_local std::string g_env_seen;
const char *env_sw(const char *name) {
    const char *v = hrn_env(name);
    if (v) {
        const std::string item = std::string(name) + "=" + v + ";";
        if (g_env_seen.find(item) == std::string::npos) g_env_seen += item;
    }
    return v;
}
// the three ways a switch is read (ctx_switches.inc), each looking its variable up once
bool sw_set(const char *name) { return env_sw(name) != nullptr; }
int sw_int(const char *name, int dflt) {
    const char *v = env_sw(name);
    return v ? atoi(v) : dflt;
}
double sw_real(const char *name, double dflt) {
    const char *v = env_sw(name);
    return v ? atof(v) : dflt;
}
bool sw_zero(const char *name) {   // set, and reads as 0: what turns off a switch that is on by default
    const char *v = env_sw(name);
    return v && atoi(v) == 0;
}
}  // namespace

struct hrn_ctx {
    std::string switches;   // the HRN_* variables this handle saw when it was created ("NAME=value;...")
    int c, joints, H, W, dtype, max_batch, device;
    int model = 0;  // 0 = HRNet (c = width), 1 = PoseResNet (c = ResNet size), SimpleHRNet.py:109-112
    int head_c = 0; // channels of the tensor final_layer reads
    int pool_in_t = -1, pool_out_t = -1;
    bool plan_only;
    int esize;
    std::string err;
    // the 16-bit MFMA path: bf16 and fp16 handles share every plan, layout and kernel; only the element format differs
    bool is16() const { return dtype == HRN_BF16 || dtype == HRN_F16; }

    std::vector<Tensor> tensors;
    std::vector<Buffer> buffers;
    std::vector<ConvOp> convs;
    std::vector<FuseOp> fuses;
    std::vector<Conv3Group> groups;
    std::vector<DirectGroup> dgroups;
    std::vector<S2Group> s2groups;
    S2Problem *s2probs_dev = nullptr;   // (the problems of `s2groups`, then of `stemf`)
    struct Chain {
        int conv3, conv1, ds;  // conv3 of Bottleneck b, conv1 of Bottleneck b+1 (-1: none, the layer's last block), projection shortcut folded in (or -1)
        int conv2 = -1;        // round 5: the 3x3 conv of Bottleneck b computed in front of conv3 (or -1: it has its own launch)
    };
    std::vector<Chain> chains;
    std::vector<TapPoint> taps;
    Conv3Problem *probs_dev = nullptr;
    std::vector<Op> ops;
    int stem_out_t = -1, head_in_t = -1;
    int64_t stem_w_off = 0, stem_b_off = 0, stem_wp_off = 0, head_w_off = 0, head_b_off = 0, head_wp_off = 0;

    int64_t blob_bytes = 0;
    char *blob = nullptr;  // device (or host when plan_only)
    bool weights_loaded = false;

#include "ctx_switches.inc"
    bool conv_xl(const ConvOp &cv) const {
        return direct_xlds && direct_wlds && is16() && cv.k == 3 && cv.stride == 2 && cv.cin % 32 == 0 && !cv.up && cv.res_t < 0 && cv.nr == 6 &&
               cv.kchunks >= 4;
    }
    std::vector<Conv3Problem> probs_host;
    bool stem_fuse = false;       // planned (bf16 HRNet whose geometry fits: stem_fused_fits)
    int stem_conv2_op = -1;       // ops[] index of conv2's own launch (skipped by a pass that ran the fused kernel)
    S2Group stemf;                // the fused kernel's problem (conv2 with one output row per tile) and block maps
    int head_slabs = 1, head_slab_px = 1024;
    static constexpr int kHeadSlabPxSmall = 256;
    int head_slabs_small = 1;
    // the head / decode split of a pass of nb crops: 1024-pixel slabs unless that leaves most of the chip idle
    int head_px_for(int nb) const { return (long)nb * head_slabs >= 192 ? head_slab_px : kHeadSlabPxSmall; }
    int head_slabs_for(int nb) const { return (long)nb * head_slabs >= 192 ? head_slabs : head_slabs_small; }
    float *part_val = nullptr;
    int *part_idx = nullptr;
    uint64_t map_clock = 0;    // LRU stamp of the block-map slots
    int64_t map_builds = 0;     // block maps built + uploaded since creation (hrn_map_rebuilds)
    float *scratch_hm = nullptr;  // max_batch heat-maps of the handle's own: flip-TTA's mirrored pass, a refined decode the caller gave no maps
    float *scratch_heatmaps() {   // allocated on first use; nullptr (and err) if that fails
        if (!scratch_hm && !hip_ok(hipMalloc((void **)&scratch_hm, (size_t)max_batch * joints * (H / 4) * (W / 4) * sizeof(float)),
                                   "hipMalloc(scratch heat-maps)"))
            scratch_hm = nullptr;
        return scratch_hm;
    }
    int64_t workspace_bytes = 0;

#include "ctx_plan.inc"
#include "ctx_memory.inc"
#include "ctx_weights.inc"
#include "ctx_run.inc"
#include "ctx_scratch.inc"
};

// ====================================================================================================
namespace {
using CallScope = hrn_ctx::CallScope;
using CallFrame = hrn_ctx::CallFrame;
using PreFrame = hrn_ctx::PreFrame;
using PinnedImage = hrn_ctx::PinnedImage;

// The refusals of an entry whose text is "<entry>: <fault>", in the newer entries' order: the arguments (`fault`, or nullptr: they
// need no device, so a plan-only handle judges them too), then the handle; true + err: the entry returns 7.
bool refused(hrn_ctx *h, const char *entry, const char *fault) {
    if (!fault) return h->refuse_plan_only();
    h->err = std::string(entry) + ": " + fault;
    return true;
}

// The loop of every forward entry: the device, then (n > 0) the scratch heat-maps if asked for, one CallScope on the pass guard and
// pass(off, nb) for each micro-batch of at most max_batch crops (false: the entry returns 8).
template <class Pass>
int each_micro_batch(hrn_ctx *h, int n, bool scratch, hipStream_t s, const Pass &pass) {
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    if (n == 0) return 0;
    if (scratch && !h->scratch_heatmaps()) return 6;
    CallScope scope(h, &h->pass, s);
    if (!scope.entered) return 6;
    for (int off = 0; off < n; off += h->max_batch)
        if (!pass(off, std::min(n - off, h->max_batch))) return 8;
    return scope.leave() ? 0 : 6;
}

bool valid_refine(hrn_ctx *h, int refine) {
    if (refine == HRN_REFINE_NONE || refine == HRN_REFINE_QUARTER || refine == HRN_REFINE_DARK) return true;
    h->err = "refine must be HRN_REFINE_NONE, HRN_REFINE_QUARTER or HRN_REFINE_DARK";
    return false;
}

// what is wrong with a BGR frame somebody is cut from, or nullptr
const char *bgr_frame_fault(const hrn_frame &f) { return !f.data || f.height <= 0 || f.width <= 0 ? "is null or has no size" : nullptr; }

// The refusals of the four multi-frame pre-path entries, in their order: the arguments first (they need no device, so a
// plan-only handle judges them too), then the handle; true + err.  `pointers`: everything the entry requires when n > 0 is there.
template <class Frame>
bool frame_table_fault(hrn_handle h, const char *entry, int variant, int n, int nframes, int det_stride, bool pointers, const int32_t *fidx,
                       const Frame *frames, const char *(*frame_fault)(const Frame &)) {
    const std::string name = entry;
    std::string why;
    if (variant != HRN_CROP_PAD && variant != HRN_CROP_CLAMP) why = "variant must be HRN_CROP_PAD or HRN_CROP_CLAMP";
    else if (n < 0 || nframes < 0 || det_stride < 4 || (n > 0 && (nframes < 1 || !pointers))) why = "bad frames / detections / n";
    else if (n > 0 && !fidx && nframes != 1) why = name + ": without frame_index there must be one frame";
    for (int i = 0; why.empty() && i < n; ++i) {
        const long f = fidx ? (long)fidx[i] : 0;
        if (f < 0 || f >= nframes)
            why = name + ": frame_index " + std::to_string(f) + " of person " + std::to_string(i) + " is outside [0, " + std::to_string(nframes) + ")";
        else if (const char *fault = frame_fault(frames[f]))
            why = name + ": frame " + std::to_string(f) + ", which person " + std::to_string(i) + " is cut from, " + fault;
    }
    if (why.empty()) return h->refuse_plan_only();
    h->err = why;
    return true;
}

// hrn_forward (HRN_REFINE_NONE) and hrn_forward_refined: one pass per micro-batch, its OP_DECODE launching decode_kernel<refine>
// (decode.hip).  A sub-pixel mode has the head write heat-maps -- the caller's, or the handle's scratch -- for the decode to read.
int forward(hrn_ctx *h, const void *images, int n, const void *boxes, int box_dtype, int refine, float *pts, float *heatmaps,
            hipStream_t s) {
    if (!h) return 1;
    if (!valid_refine(h, refine)) return 7;
    if (!h->check_forward_args(images, n, boxes, pts, heatmaps)) return 7;
    if (refine != HRN_REFINE_NONE && !pts) {
        h->err = "hrn_forward_refined: a refine mode needs pts (it refines the joint coordinates)";
        return 7;
    }
    const bool scratch = refine != HRN_REFINE_NONE && !heatmaps;
    return each_micro_batch(h, n, scratch, s, [&](int off, int nb) {
        const float *img = (const float *)images + (size_t)off * 3 * h->H * h->W;
        const void *bx = boxes ? (const char *)boxes + (size_t)off * 16 : nullptr;
        float *p = pts ? pts + (size_t)off * h->joints * 3 : nullptr;
        float *hp = heatmaps ? heatmaps + (size_t)off * h->joints * (h->H / 4) * (h->W / 4) : scratch ? h->scratch_hm : nullptr;
        return h->run_pass(img, nb, bx, box_dtype, p, hp, s, nullptr, 0, nullptr, refine);
    });
}
}  // namespace

extern "C" {

const char *hrn_version(void) { return "hrnet_mi355 0.1 (gfx950)"; }

int hrn_create(hrn_handle *out, int c, int nof_joints, int height, int width, int dtype, int max_batch,
               int device_id) {
    return hrn_create_model(out, HRN_MODEL_HRNET, c, nof_joints, height, width, dtype, max_batch, device_id);
}

int hrn_create_model(hrn_handle *out, int model, int c, int nof_joints, int height, int width, int dtype, int max_batch,
                     int device_id) {
    if (!out) return 1;
    *out = nullptr;
    if (model != HRN_MODEL_HRNET && model != HRN_MODEL_POSERESNET) {
        g_create_error = "model must be HRN_MODEL_HRNET or HRN_MODEL_POSERESNET";
        return 2;
    }
    if (model == HRN_MODEL_POSERESNET && c != 50 && c != 101 && c != 152) {
        g_create_error = "PoseResNet: c is the ResNet size, 50 / 101 / 152 (the reference's 18 / 34 cannot run: modules.py:50)";
        return 2;
    }
    if (model == HRN_MODEL_HRNET && (c <= 0 || (c % 32 != 0 && c % 48 != 0))) {
        g_create_error = "c must be a positive multiple of 32 or of 48 (HRNet-W32 / W48 / W64 ...): the kernels tile output channels by 32 / 48 / 64";
        return 2;
    }
    if (height <= 0 || width <= 0 || height % 32 || width % 32) {
        g_create_error = "resolution must be a positive multiple of 32 in both dimensions";
        return 2;
    }
    static_assert(HRN_MAX_JOINTS == kMaxJoints, "the header's bound is the kernels' bound");
    if (nof_joints <= 0 || nof_joints > HRN_MAX_JOINTS) {
        g_create_error = "nof_joints must be in [1, HRN_MAX_JOINTS = " + std::to_string(HRN_MAX_JOINTS) + "]";
        return 2;
    }
    if (dtype != HRN_F32 && dtype != HRN_BF16 && dtype != HRN_F16) {
        g_create_error = "dtype must be HRN_F32, HRN_BF16 or HRN_F16";
        return 2;
    }
    if (max_batch <= 0) {
        g_create_error = "max_batch must be positive";
        return 2;
    }
    g_env_seen.clear();
    std::unique_ptr<hrn_ctx> h(new hrn_ctx());
    h->switches = g_env_seen;
    h->model = model;
    h->c = c, h->joints = nof_joints, h->H = height, h->W = width, h->dtype = dtype, h->max_batch = max_batch;
    h->device = device_id, h->plan_only = device_id < 0;
    h->esize = h->is16() ? 2 : 4;
    if (!h->plan_only) {
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || device_id >= ndev) {
            g_create_error = "no such HIP device " + std::to_string(device_id) + " (" +
                             (e != hipSuccess ? hipGetErrorString(e) : "device count " + std::to_string(ndev)) + ")";
            return 3;
        }
    }
    h->build_plan();
    h->index_taps();
    // every conv launcher covers cout in tiles of 16*nr channels: a width that leaves a remainder would silently skip
    // channels (c = 80: 16 of branch 0's 80).  Multiples of 32 and of 48 never do.
    for (const ConvOp &cv : h->convs)
        if (cv.nr <= 0 || cv.cout % (16 * cv.nr) != 0) {
            g_create_error = "unsupported width: convolution '" + cv.conv + "' has " + std::to_string(cv.cout) +
                             " output channels, not a multiple of its " + std::to_string(16 * cv.nr) +
                             "-channel tile (use a width that is a multiple of 32 or of 48)";
            return 2;
        }
    if (!h->allocate()) {
        g_create_error = h->err.empty() ? "allocation failed" : h->err;
        h->free_all();
        return 4;
    }
    *out = h.release();
    return 0;
}

void hrn_destroy(hrn_handle h) {
    if (!h) return;
    h->free_all();
    delete h;
}

const char *hrn_last_error(hrn_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int hrn_load_weights(hrn_handle h, const hrn_tensor_desc *descs, int n) {
    if (!h || !descs) return 1;
    return h->load_weights(descs, n) ? 0 : 5;
}

int64_t hrn_weight_blob_bytes(hrn_handle h) { return h ? h->blob_bytes : 0; }
void *hrn_weight_blob_ptr(hrn_handle h) { return h ? h->blob : nullptr; }
int hrn_adopt_weights(hrn_handle h) {
    if (!h) return 1;
    h->weights_loaded = true;
    return 0;
}

int hrn_weight_blob_read(hrn_handle h, int64_t offset, void *dst, int64_t nbytes) {
    if (!h || !dst || offset < 0 || nbytes < 0 || offset + nbytes > h->blob_bytes) return 1;
    if (h->plan_only) {
        memcpy(dst, h->blob + offset, (size_t)nbytes);
        return 0;
    }
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    return h->hip_ok(hipMemcpy(dst, h->blob + offset, (size_t)nbytes, hipMemcpyDeviceToHost), "hipMemcpy") ? 0 : 6;
}

int hrn_forward(hrn_handle h, const void *images_dev, int n, const void *boxes_dev, int box_dtype, float *pts_dev,
                float *heatmaps_dev, void *stream) {
    return forward(h, images_dev, n, boxes_dev, box_dtype, HRN_REFINE_NONE, pts_dev, heatmaps_dev, (hipStream_t)stream);
}

// Flip test-time augmentation + the evaluation decode (testing/Test.py:132-140, training/COCO.py:206-230,
// misc/utils.py:9-29, 125-175): two passes per micro-batch (the second reads the crops mirrored in the stem), then one
// kernel averages, finds the maxima and applies the quarter-pixel refinement.
int hrn_forward_flip_tta(hrn_handle h, const void *images_dev, int n, const int32_t *flip_pairs_host, int npairs,
                         int post_processing, float *heatmaps_dev, float *preds_dev, float *maxvals_dev, void *stream) {
    if (!h) return 1;
    if (!h->check_forward_args(images_dev, n, nullptr, nullptr, heatmaps_dev, /*outputs_optional=*/true)) return 7;
    if (!heatmaps_dev || !preds_dev || !maxvals_dev || npairs < 0 || (npairs > 0 && !flip_pairs_host)) {
        h->err = "heatmaps, preds and maxvals are required outputs; flip_pairs must be npairs x 2";
        return 7;
    }
    TtaArgs a;
    for (int j = 0; j < kMaxJoints; ++j) a.pair[j] = j;
    for (int k = 0; k < npairs; ++k) {
        const int p0 = flip_pairs_host[2 * k], p1 = flip_pairs_host[2 * k + 1];
        if (p0 < 0 || p1 < 0 || p0 >= h->joints || p1 >= h->joints) {
            h->err = "flip pair out of range";
            return 7;
        }
        // flip_back (misc/utils.py:24-27) swaps the two maps IN PLACE, pair after pair: compose the swaps in that order
        // (equal to "p0 <-> p1" only while no joint occurs in two pairs)
        std::swap(a.pair[p0], a.pair[p1]);
    }
    a.joints = h->joints, a.h = h->H / 4, a.w = h->W / 4, a.post_processing = post_processing;
    hipStream_t s = (hipStream_t)stream;
    return each_micro_batch(h, n, /*scratch=*/true, s, [&](int off, int nb) {   // the scratch takes the mirrored pass
        const float *img = (const float *)images_dev + (size_t)off * 3 * h->H * h->W;
        float *out = heatmaps_dev + (size_t)off * h->joints * a.h * a.w;
        if (!h->run_pass(img, nb, nullptr, 0, nullptr, out, s, nullptr, 0) ||
            !h->run_pass(img, nb, nullptr, 0, nullptr, h->scratch_hm, s, nullptr, 1))
            return false;
        a.hm = out, a.hm_flipped = h->scratch_hm, a.n = nb;
        a.preds = preds_dev + (size_t)off * h->joints * 2, a.maxvals = maxvals_dev + (size_t)off * h->joints;
        return h->hip_ok(launch_tta_decode(a, s), "flip-TTA decode launch");
    });
}

int hrn_forward_refined(hrn_handle h, const void *images_dev, int n, const void *boxes_dev, int box_dtype, int refine,
                        float *pts_dev, float *heatmaps_dev, void *stream) {
    return forward(h, images_dev, n, boxes_dev, box_dtype, refine, pts_dev, heatmaps_dev, (hipStream_t)stream);
}

int hrn_refine_coords(hrn_handle h, const float *heatmaps_dev, int n, int refine, float *coords_dev, void *stream) {
    if (!h) return 1;
    if (!valid_refine(h, refine)) return 7;
    if (h->refuse_plan_only()) return 7;
    if (n < 0 || (n > 0 && (!heatmaps_dev || !coords_dev))) {
        h->err = "hrn_refine_coords: bad heatmaps / coords / n";
        return 7;
    }
    if (n == 0 || refine == HRN_REFINE_NONE) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    DecodeArgs a{};
    a.heatmaps = heatmaps_dev, a.coords = coords_dev;
    a.n = n, a.joints = h->joints, a.h = h->H / 4, a.w = h->W / 4, a.mode = refine;
    CallScope scope(h, &h->pass, (hipStream_t)stream);
    if (!scope.entered) return 6;
    if (!h->hip_ok(launch_refine_coords(a, (hipStream_t)stream), "refine launch")) return 8;
    return scope.leave() ? 0 : 6;
}

namespace {
// track_geometry.h's crop_geometry_one (the box arithmetic, one text for the host and the record kernel of track.hip) with the
// host entries' refusals: false + err when the reference would wrap around or divide by zero
bool crop_geometry_one(const float *d, int i, int frame_h, int frame_w, int H, int W, int variant, CropParams &cp, int32_t *box,
                       std::string &err) {
    long pad_hw[2];
    const int status = hrn::crop_geometry_one(d, frame_h, frame_w, H, W, variant, cp, box, pad_hw);
    if (status == CROP_OK) return true;
    err = "detection " + std::to_string(i) +
          (status == CROP_DEGENERATE ? " is degenerate" : status == CROP_OUTSIDE ? " starts outside the frame" : " is degenerate after clamping");
    return false;
}

thread_local std::string g_geometry_error;

// (y0, CY, CUB, CUG, CVG, CVR) in 20-bit fixed point; false on an unknown matrix or range
bool yuv_coefficients(int matrix, int range, int32_t out[6]) {
    if ((matrix != HRN_YUV_BT601 && matrix != HRN_YUV_BT709) || (range != HRN_YUV_LIMITED && range != HRN_YUV_FULL)) return false;
    if (matrix == HRN_YUV_BT601 && range == HRN_YUV_LIMITED) {   // OpenCV's published constants (color_yuv: ITUR_BT_601_*), verbatim
        const int32_t cv[6] = {16, 1220542, 2116026, -409993, -852492, 1673527};
        memcpy(out, cv, sizeof(cv));
        return true;
    }
    const double kr = matrix == HRN_YUV_BT601 ? 0.299 : 0.2126, kb = matrix == HRN_YUV_BT601 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
    const double sy = range == HRN_YUV_LIMITED ? 255.0 / 219.0 : 1.0, sc = range == HRN_YUV_LIMITED ? 255.0 / 224.0 : 1.0;
    const double x[5] = {sy, 2.0 * (1.0 - kb) * sc, -2.0 * (1.0 - kb) * kb / kg * sc, -2.0 * (1.0 - kr) * kr / kg * sc, 2.0 * (1.0 - kr) * sc};
    out[0] = range == HRN_YUV_LIMITED ? 16 : 0;
    for (int k = 0; k < 5; ++k) out[1 + k] = (int32_t)std::floor(x[k] * 1048576.0 + 0.5);
    return true;
}

// what is wrong with a YUV frame somebody reads, or nullptr
// the 4:2:0 layouts by name: every place that treats one differently from another asks one of these
inline bool pix_is_yuv(int format) {
    return format == HRN_PIX_NV12 || format == HRN_PIX_I420 || format == HRN_PIX_NV21 || format == HRN_PIX_P010 || format == HRN_PIX_I010;
}
inline bool pix_is_planar(int format) { return format == HRN_PIX_I420 || format == HRN_PIX_I010; }   // U and V planes of their own
inline bool pix_is_10bit(int format) { return format == HRN_PIX_P010 || format == HRN_PIX_I010; }    // 16-bit words

// the pitch and plane checks of a YUV frame, behind its format and size checks: planes of 8-bit samples or of 16-bit words
const char *yuv_plane_fault(const hrn_yuv_frame &f) {
    const bool planar = pix_is_planar(f.format), wide = pix_is_10bit(f.format);
    if (f.pitch_y < (wide ? 2L : 1L) * f.width) return wide ? "has pitch_y below twice its width" : "has pitch_y below its width";
    // a chroma row: width bytes (NV12 / NV21: width / 2 pairs; I010: width / 2 words), width / 2 (I420) or 2 * width (P010)
    const long need_c = f.format == HRN_PIX_P010 ? 2L * f.width : f.format == HRN_PIX_I420 ? f.width / 2 : f.width;
    if (f.pitch_c < need_c)
        return f.format == HRN_PIX_P010   ? "has pitch_c below twice its width"
               : f.format == HRN_PIX_I420 ? "has pitch_c below half its width"
                                          : "has pitch_c below its width";
    if (!f.y || !f.u || (planar && !f.v)) return "has a null plane";
    if (wide && (((size_t)f.y | (size_t)f.u | (planar ? (size_t)f.v : 0) | (size_t)f.pitch_y | (size_t)f.pitch_c) & 1))
        return "has an odd plane address or pitch on a 10-bit frame";
    return nullptr;
}

const char *yuv_frame_fault(const hrn_yuv_frame &f) {
    if (!pix_is_yuv(f.format))
        return "has an unknown format (HRN_PIX_NV12, HRN_PIX_I420, HRN_PIX_NV21, HRN_PIX_P010 or HRN_PIX_I010)";
    if (f.matrix != HRN_YUV_BT601 && f.matrix != HRN_YUV_BT709) return "has an unknown matrix (HRN_YUV_BT601 or HRN_YUV_BT709)";
    if (f.range != HRN_YUV_LIMITED && f.range != HRN_YUV_FULL) return "has an unknown range (HRN_YUV_LIMITED or HRN_YUV_FULL)";
    if (f.height <= 0 || f.width <= 0 || (f.height & 1) || (f.width & 1)) return "has an odd or non-positive width or height";
    return yuv_plane_fault(f);
}

YuvSource yuv_source(const hrn_yuv_frame &f) {   // of a frame yuv_frame_fault has passed
    YuvSource ys{};
    ys.y = f.y, ys.u = f.u, ys.v = pix_is_planar(f.format) ? f.v : nullptr;
    ys.pitch_y = f.pitch_y, ys.pitch_c = f.pitch_c, ys.format = f.format;
    int32_t c[6];
    (void)yuv_coefficients(f.matrix, f.range, c);
    for (int k = 0; k < 6; ++k) ys.coef[k] = c[k];
    return ys;
}

// the one body of hrn_preprocess_frame and hrn_preprocess_frames, behind their argument checks: person i is cut from
// frames[fidx ? fidx[i] : 0]; everything that can be refused is refused before anything is queued
// (yframes: the people are cut from YUV frames instead -- the same records, staging and vertical pass, a YuvSource beside each)
int preprocess_people(hrn_handle h, const hrn_frame *frames, const hrn_yuv_frame *yframes, const int32_t *fidx, const float *dets_host,
                      int det_stride, int n, int variant, float *images_dev, int32_t *boxes_host, int32_t *boxes_dev, hipStream_t s) {
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    const int H = h->H, W = h->W;
    // crop parameters (each with its frame's pointer and size: the frame table travels inside them) + boxes are written
    // straight into a pinned image the async uploads below read after this call has returned; kPreRing images in rotation,
    // each reused only once the upload that read it last has completed
    const size_t cp_bytes = ((size_t)n * sizeof(CropParams) + 63) / 64 * 64, box_bytes = (size_t)n * 16;
    const size_t need = cp_bytes + box_bytes + (yframes ? (size_t)n * sizeof(YuvSource) : 0);
    const PinnedImage img = h->image(need);
    if (!img) return 6;
    CropParams *cps = img.as<CropParams>();
    int32_t *boxes = img.as<int32_t>(cp_bytes);
    YuvSource *srcs = img.as<YuvSource>(cp_bytes + box_bytes);
    size_t tmp_bytes = 0;
    int max_h_pad = 0;
    for (int i = 0; i < n; ++i) {
        const int fi = fidx ? fidx[i] : 0;
        const int frame_h = yframes ? yframes[fi].height : frames[fi].height, frame_w = yframes ? yframes[fi].width : frames[fi].width;
        CropParams &cp = cps[i];
        if (!crop_geometry_one(dets_host + (size_t)i * det_stride, i, frame_h, frame_w, H, W, variant, cp, boxes + (size_t)i * 4, h->err))
            return 7;
        cp.frame = yframes ? nullptr : frames[fi].data, cp.frame_w = frame_w, cp.frame_h = frame_h;
        if (yframes) srcs[i] = yuv_source(yframes[fi]);
        cp.tmp_off = (long long)tmp_bytes;
        tmp_bytes += ((size_t)cp.h_pad * W * 3 + 255) / 256 * 256;
        if (cp.h_pad > max_h_pad) max_h_pad = cp.h_pad;
    }
    PreFrame frame(h, tmp_bytes, n, yframes != nullptr, s);
    CropParams *params = frame.dev<CropParams>(h->pre_params);
    YuvSource *yuv = yframes ? frame.dev<YuvSource>(h->pre_yuv) : nullptr;
    if (!frame.upload(img, {{yuv, srcs, (size_t)n * sizeof(YuvSource), "hipMemcpyAsync(YUV sources)"},
                            {params, cps, (size_t)n * sizeof(CropParams), "hipMemcpyAsync(crop params)"},
                            {boxes_dev, boxes, (size_t)n * 16, "hipMemcpyAsync(boxes)"}}))
        return 6;
    if (boxes_host) memcpy(boxes_host, boxes, (size_t)n * 16);
    const hipError_t e = yframes ? launch_prepath_yuv(params, yuv, n, max_h_pad, frame.dev<unsigned char>(), images_dev, H, W, s)
                                 : launch_prepath(params, n, max_h_pad, frame.dev<unsigned char>(), images_dev, H, W, s);
    if (!h->hip_ok(e, "pre-path launch")) return 8;
    return frame.leave() ? 0 : 6;
}
}  // namespace

int hrn_crop_geometry(const float *dets, int det_stride, int n, const int32_t *frame_hw, int per_person_hw, int height, int width,
                      int variant, int32_t *boxes_out, int32_t *slice_out) {
    g_geometry_error.clear();
    if (variant != HRN_CROP_PAD && variant != HRN_CROP_CLAMP) {
        g_geometry_error = "variant must be HRN_CROP_PAD or HRN_CROP_CLAMP";
        return 7;
    }
    if (n < 0 || det_stride < 4 || height <= 0 || width <= 0 || (n > 0 && (!dets || !frame_hw))) {
        g_geometry_error = "bad frame / detections / n";
        return 7;
    }
    for (int i = 0; i < n; ++i) {
        const int32_t *hw = frame_hw + (per_person_hw ? (size_t)i * 2 : 0);
        if (hw[0] <= 0 || hw[1] <= 0) {
            g_geometry_error = "bad frame / detections / n";
            return 7;
        }
        CropParams cp{};
        int32_t box[4];
        if (!crop_geometry_one(dets + (size_t)i * det_stride, i, hw[0], hw[1], height, width, variant, cp, box, g_geometry_error)) return 7;
        if (boxes_out) memcpy(boxes_out + (size_t)i * 4, box, sizeof(box));
        if (slice_out) {
            const int32_t sl[8] = {cp.x1, cp.y1, cp.w_crop, cp.h_crop, cp.pad_top, cp.pad_left, cp.h_pad, cp.w_pad};
            memcpy(slice_out + (size_t)i * 8, sl, sizeof(sl));
        }
    }
    return 0;
}

const char *hrn_crop_geometry_last_error(void) { return g_geometry_error.c_str(); }

int hrn_preprocess_frame(hrn_handle h, const uint8_t *frame_dev, int frame_h, int frame_w, const float *dets_host,
                         int det_stride, int n, int variant, float *images_dev, int32_t *boxes_host, int32_t *boxes_dev,
                         void *stream) {
    if (!h) return 1;
    if (h->refuse_plan_only()) return 7;
    if (variant != HRN_CROP_PAD && variant != HRN_CROP_CLAMP) {
        h->err = "variant must be HRN_CROP_PAD or HRN_CROP_CLAMP";
        return 7;
    }
    if (n < 0 || det_stride < 4 || frame_h <= 0 || frame_w <= 0 || (n > 0 && (!frame_dev || !dets_host || !images_dev))) {
        h->err = "bad frame / detections / n";
        return 7;
    }
    if (n == 0) return 0;
    const hrn_frame one = {frame_dev, frame_h, frame_w};   // a one-frame table: the same kernels, the same bits
    return preprocess_people(h, &one, nullptr, nullptr, dets_host, det_stride, n, variant, images_dev, boxes_host, boxes_dev,
                             (hipStream_t)stream);
}

// SimpleHRNet.py:383-412 over a whole stack, or :236-278 over many frames.  The arguments are judged first (they need no
// device, so a plan-only handle judges them too), then the handle, then the boxes; nothing is queued before all have passed.
int hrn_preprocess_frames(hrn_handle h, const hrn_frame *frames_host, int nframes, const float *dets_host, int det_stride,
                          const int32_t *frame_index_host, int n, int variant, float *images_dev, int32_t *boxes_host,
                          int32_t *boxes_dev, void *stream) {
    if (!h) return 1;
    if (frame_table_fault(h, "hrn_preprocess_frames", variant, n, nframes, det_stride,
                          frames_host && dets_host && images_dev, frame_index_host, frames_host, bgr_frame_fault))
        return 7;
    if (n == 0) return 0;
    return preprocess_people(h, frames_host, nullptr, frame_index_host, dets_host, det_stride, n, variant, images_dev, boxes_host,
                             boxes_dev, (hipStream_t)stream);
}

int hrn_yuv_coefficients(int matrix, int range, int32_t out[6]) {
    if (!out) return 7;
    return yuv_coefficients(matrix, range, out) ? 0 : 7;
}

int hrn_yuv_to_bgr(hrn_handle h, const hrn_yuv_frame *frame_host, uint8_t *bgr_dev, void *stream) {
    if (!h) return 1;
    if (!frame_host || !bgr_dev) {
        h->err = "hrn_yuv_to_bgr: null frame or output";
        return 7;
    }
    if (const char *fault = yuv_frame_fault(*frame_host)) {
        h->err = std::string("hrn_yuv_to_bgr: the frame ") + fault;
        return 7;
    }
    if (h->refuse_plan_only()) return 7;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    if (!h->hip_ok(launch_yuv_to_bgr(yuv_source(*frame_host), frame_host->height, frame_host->width, bgr_dev, (hipStream_t)stream),
                   "yuv_to_bgr launch"))
        return 8;
    return 0;
}

// hrn_preprocess_frames over YUV frames: its checks and texts, then the frames' own, then the handle, then the boxes
int hrn_preprocess_frames_yuv(hrn_handle h, const hrn_yuv_frame *frames_host, int nframes, const float *dets_host, int det_stride,
                              const int32_t *frame_index_host, int n, int variant, float *images_dev, int32_t *boxes_host,
                              int32_t *boxes_dev, void *stream) {
    if (!h) return 1;
    if (frame_table_fault(h, "hrn_preprocess_frames_yuv", variant, n, nframes, det_stride,
                          frames_host && dets_host && images_dev, frame_index_host, frames_host, yuv_frame_fault))
        return 7;
    if (n == 0) return 0;
    return preprocess_people(h, nullptr, frames_host, frame_index_host, dets_host, det_stride, n, variant, images_dev, boxes_host,
                             boxes_dev, (hipStream_t)stream);
}

// ---- the tracking link: boxes from joints, and the crop pre-path from detections on the device --------------------------------
namespace {
thread_local std::string g_pose_boxes_error;

// what is wrong with the arguments of hrn_pose_boxes / hrn_boxes_from_poses, into `why` (false: nothing); needs no device
bool pose_box_fault(const void *pts, int n, int J, const int32_t *frame_hw, int per_person_hw, int min_joints, double scale,
                    double min_side, const void *dets, std::string &why) {
    why.clear();
    if (n < 0) why = "n is negative";
    else if (J < 1 || J > HRN_MAX_JOINTS) why = "J must be in [1, " + std::to_string(HRN_MAX_JOINTS) + "]";
    else if (min_joints < 1) why = "min_joints must be at least 1";
    else if (!std::isfinite(scale) || !(scale > 0)) why = "scale must be finite and positive";
    else if (!std::isfinite(min_side) || min_side < 0) why = "min_side must be finite and not negative";
    else if (n > 0 && (!pts || !frame_hw || !dets)) why = "null joints / frame sizes / output";
    for (int i = 0; why.empty() && i < (per_person_hw ? n : std::min(n, 1)); ++i)
        if (frame_hw[2 * (size_t)i] <= 0 || frame_hw[2 * (size_t)i + 1] <= 0)
            why = "the frame of person " + std::to_string(i) + " has a non-positive side";
    return !why.empty();
}

// the one body of hrn_preprocess_frames_dev and hrn_preprocess_frames_yuv_dev, behind their argument checks
int preprocess_people_dev(hrn_handle h, const hrn_frame *frames, const hrn_yuv_frame *yframes, int nframes, const int32_t *fidx,
                          const float *dets_dev, int det_stride, int n, int variant, float *images_dev, int32_t *boxes_dev,
                          int32_t *status_dev, hipStream_t s) {
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    const int H = h->H, W = h->W;
    const auto entry = [&](int f) {
        TrackFrame t{};
        if (yframes) {
            if (!yuv_frame_fault(yframes[f])) t.height = yframes[f].height, t.width = yframes[f].width, t.yuv = yuv_source(yframes[f]);
        } else {
            t.bgr = frames[f].data, t.height = frames[f].height, t.width = frames[f].width;
        }
        return t;
    };
    // the host sizes grid and scratch without knowing the boxes: every person gets the rows a box inside the largest frame
    // referred to can need -- and at least H, the rows of the all-padding crop of a refused person
    long rows = H;
    for (int i = 0; i < n; ++i) {
        const int f = fidx ? fidx[i] : 0;
        const int frame_h = yframes ? yframes[f].height : frames[f].height, frame_w = yframes ? yframes[f].width : frames[f].width;
        rows = std::max(rows, crop_hcap(frame_h, frame_w, H, W));
    }
    const size_t slot = ((size_t)rows * W * 3 + 255) / 256 * 256;
    // (fidx) the frame table and everybody's entry of it
    const size_t table_bytes = fidx ? (size_t)nframes * sizeof(TrackFrame) : 0, need = fidx ? table_bytes + (size_t)n * sizeof(int32_t) : 0;
    PreFrame frame(h, (size_t)n * slot, n, yframes != nullptr, s);
    // (the table's guard is left behind the launch that reads it)
    CallFrame table(h, s, {{&h->trk_table, need, hrn_ctx::twice(need, 4096), "hipMalloc(tracking table)"}});
    CropParams *params = frame.dev<CropParams>(h->pre_params);
    YuvSource *yuv = frame.dev<YuvSource>(h->pre_yuv);
    CropRecordArgs a{};
    a.dets = dets_dev, a.det_stride = det_stride, a.n = n, a.H = H, a.W = W, a.variant = variant, a.yuv = yframes ? 1 : 0;
    a.slot_bytes = (long long)slot;
    a.crops = params, a.srcs = yuv, a.boxes = boxes_dev, a.status = status_dev;
    const char *dev = table.table<char>(need, "hipMemcpyAsync(tracking table)", [&](char *pin) {
        std::vector<char> used((size_t)nframes, 0);
        for (int i = 0; i < n; ++i) used[fidx[i]] = 1;
        for (int f = 0; f < nframes; ++f) ((TrackFrame *)pin)[f] = used[f] ? entry(f) : TrackFrame{};
        memcpy(pin + table_bytes, fidx, (size_t)n * sizeof(int32_t));
    });
    if (!frame.ok() || !table.ok()) return 6;
    if (dev) a.frames = (const TrackFrame *)dev, a.frame_index = (const int *)(dev + table_bytes);
    else a.frame0 = entry(0);
    if (!h->hip_ok(launch_crop_records(a, s), "crop records launch")) return 8;
    if (!table.leave()) return 6;
    const hipError_t e = yframes ? launch_prepath_yuv(params, yuv, n, (int)rows, frame.dev<unsigned char>(), images_dev, H, W, s)
                                 : launch_prepath(params, n, (int)rows, frame.dev<unsigned char>(), images_dev, H, W, s);
    if (!h->hip_ok(e, "pre-path launch")) return 8;
    return frame.leave() ? 0 : 6;
}
}  // namespace

int hrn_pose_boxes(const float *pts, int n, int J, const int32_t *frame_hw, int per_person_hw, float threshold, int min_joints,
                   double scale, double min_side, float *dets_out) {
    if (pose_box_fault(pts, n, J, frame_hw, per_person_hw, min_joints, scale, min_side, dets_out, g_pose_boxes_error)) return 7;
    for (int i = 0; i < n; ++i) {
        const int32_t *hw = frame_hw + (per_person_hw ? (size_t)i * 2 : 0);
        pose_box_one(pts + (size_t)i * J * 3, J, hw[0], hw[1], threshold, min_joints, scale, min_side, dets_out + (size_t)i * 5);
    }
    return 0;
}

const char *hrn_pose_boxes_last_error(void) { return g_pose_boxes_error.c_str(); }

int hrn_boxes_from_poses(hrn_handle h, const float *pts_dev, int n, int J, const int32_t *frame_hw_host, int per_person_hw,
                         float threshold, int min_joints, double scale, double min_side, float *dets_dev, void *stream) {
    if (!h) return 1;
    std::string fault;
    const bool bad = pose_box_fault(pts_dev, n, J, frame_hw_host, per_person_hw, min_joints, scale, min_side, dets_dev, fault);
    if (refused(h, "hrn_boxes_from_poses", bad ? fault.c_str() : nullptr)) return 7;
    if (n == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;
    PoseBoxArgs a{};
    a.pts = pts_dev, a.n = n, a.J = J, a.threshold = threshold, a.min_joints = min_joints, a.scale = scale, a.min_side = min_side;
    a.dets = dets_dev;
    const size_t need = per_person_hw ? (size_t)n * 2 * sizeof(int32_t) : 0;   // a frame size per person: a table through the pinned ring
    CallFrame frame(h, s, {{&h->trk_table, need, hrn_ctx::twice(need, 4096), "hipMalloc(tracking table)"}});
    a.frame_hw = frame.table<int>(frame_hw_host, (size_t)n * 2, "hipMemcpyAsync(tracking table)");
    if (!frame.ok()) return 6;
    if (!a.frame_hw) a.frame_h = frame_hw_host[0], a.frame_w = frame_hw_host[1];
    if (!h->hip_ok(launch_pose_boxes(a, s), "pose boxes launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// hrn_preprocess_frames with the detections on the device: its argument checks and texts (minus the per-detection ones, which
// become status_dev), then the handle
int hrn_preprocess_frames_dev(hrn_handle h, const hrn_frame *frames_host, int nframes, const float *dets_dev, int det_stride,
                              const int32_t *frame_index_host, int n, int variant, float *images_dev, int32_t *boxes_dev,
                              int32_t *status_dev, void *stream) {
    if (!h) return 1;
    if (frame_table_fault(h, "hrn_preprocess_frames_dev", variant, n, nframes, det_stride,
                          frames_host && dets_dev && images_dev && boxes_dev && status_dev, frame_index_host, frames_host, bgr_frame_fault))
        return 7;
    if (n == 0) return 0;
    return preprocess_people_dev(h, frames_host, nullptr, nframes, frame_index_host, dets_dev, det_stride, n, variant, images_dev,
                                 boxes_dev, status_dev, (hipStream_t)stream);
}

int hrn_preprocess_frames_yuv_dev(hrn_handle h, const hrn_yuv_frame *frames_host, int nframes, const float *dets_dev, int det_stride,
                                  const int32_t *frame_index_host, int n, int variant, float *images_dev, int32_t *boxes_dev,
                                  int32_t *status_dev, void *stream) {
    if (!h) return 1;
    if (frame_table_fault(h, "hrn_preprocess_frames_yuv_dev", variant, n, nframes, det_stride,
                          frames_host && dets_dev && images_dev && boxes_dev && status_dev, frame_index_host, frames_host, yuv_frame_fault))
        return 7;
    if (n == 0) return 0;
    return preprocess_people_dev(h, nullptr, frames_host, nframes, frame_index_host, dets_dev, det_stride, n, variant, images_dev,
                                 boxes_dev, status_dev, (hipStream_t)stream);
}

int hrn_yuv_from_bgr(int matrix, int range, const uint8_t *bgr, int n, uint8_t *yuv_out) {
    if ((matrix != HRN_YUV_BT601 && matrix != HRN_YUV_BT709) || (range != HRN_YUV_LIMITED && range != HRN_YUV_FULL)) return 7;
    if (n < 0 || (n > 0 && (!bgr || !yuv_out))) return 7;
    const double kr = matrix == HRN_YUV_BT601 ? 0.299 : 0.2126, kb = matrix == HRN_YUV_BT601 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
    const double y0 = range == HRN_YUV_LIMITED ? 16.0 : 0.0, sy = range == HRN_YUV_LIMITED ? 219.0 / 255.0 : 1.0,
                 sc = range == HRN_YUV_LIMITED ? 224.0 / 255.0 : 1.0;
    const auto clip8 = [](double v) { return (uint8_t)std::min(255.0, std::max(0.0, std::nearbyint(v))); };
    for (int i = 0; i < n; ++i) {
        const double b = bgr[3 * i], g = bgr[3 * i + 1], r = bgr[3 * i + 2];
        const double luma = kr * r + kg * g + kb * b;
        yuv_out[3 * i] = clip8(y0 + sy * luma);
        yuv_out[3 * i + 1] = clip8(128.0 + sc * (b - luma) / (2.0 * (1.0 - kb)));
        yuv_out[3 * i + 2] = clip8(128.0 + sc * (r - luma) / (2.0 * (1.0 - kr)));
    }
    return 0;
}

namespace {
// what is wrong with a canvas somebody is drawn on, or nullptr
const char *canvas_fault(const hrn_canvas &c) {
    if (!c.y && !c.u && !c.v) return "is null";
    if (c.format != HRN_PIX_BGR && c.format != HRN_PIX_NV12 && c.format != HRN_PIX_I420)
        return "has an unknown format (HRN_PIX_BGR, HRN_PIX_NV12 or HRN_PIX_I420)";
    if (c.height <= 0 || c.width <= 0) return "has a non-positive width or height";
    if (c.height > 8192 || c.width > 8192) return "has a side above 8192";
    if (c.format == HRN_PIX_BGR) {
        if ((long)c.pitch_y < 3L * c.width) return "has a pitch below three times its width";
        return c.y ? nullptr : "is null";
    }
    if ((c.height & 1) || (c.width & 1)) return "has an odd width or height";
    if (c.pitch_y < c.width) return "has pitch_y below its width";
    if (c.pitch_c < (c.format == HRN_PIX_NV12 ? c.width : c.width / 2))
        return c.format == HRN_PIX_NV12 ? "has pitch_c below its width" : "has pitch_c below half its width";
    if (!c.y || !c.u || (c.format == HRN_PIX_I420 && !c.v)) return "has a null plane";
    return nullptr;
}
inline unsigned pack_colour(const uint8_t *c) { return (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16); }
inline size_t align16(size_t v) { return (v + 15) / 16 * 16; }

extern "C++" {   // (a std::string result and a member template, inside this file's extern "C")
// What is wrong with the canvases the n people of a call refer to, or "": a frame index out of range, a referenced canvas that
// canvas_fault refuses, BGR and YUV canvases in one call, two referenced canvases that start at the same address.  (One writer
// per byte needs canvases that do not overlap; overlapping views of one buffer cannot be told from here: the header forbids them.)
std::string canvas_table_fault(const hrn_canvas *canvases, int nframes, int n, const int32_t *frame_index) {
    int kind = -1;   // 0: BGR canvases, 1: YUV
    for (int i = 0; i < n; ++i) {
        const long f = frame_index ? (long)frame_index[i] : 0;
        if (f < 0 || f >= nframes)
            return "frame_index " + std::to_string(f) + " of person " + std::to_string(i) + " is outside [0, " + std::to_string(nframes) + ")";
        if (const char *fault = canvas_fault(canvases[f]))
            return "canvas " + std::to_string(f) + ", which person " + std::to_string(i) + " is drawn on, " + fault;
        const int k = canvases[f].format == HRN_PIX_BGR ? 0 : 1;
        if (kind >= 0 && k != kind)
            return "canvas " + std::to_string(f) + ", which person " + std::to_string(i) +
                   " is drawn on, mixes formats: the canvases of a call are all BGR or all YUV";
        kind = k;
    }
    std::map<const uint8_t *, int> first_at;
    for (int i = 0; i < n; ++i) {
        const int f = frame_index ? frame_index[i] : 0;
        const auto seen = first_at.emplace(canvases[f].y, f);
        if (!seen.second && seen.first->second != f)
            return "canvases " + std::to_string(seen.first->second) + " and " + std::to_string(f) +
                   " name the same buffer: the canvases of a call must not overlap";
    }
    return "";
}

// The head of a drawing call's table, the same for hrn_draw_poses and hrn_draw_labels_dev: the canvases somebody refers to, in
// table order, each with its tiles and its people; the people grouped by canvas in call order; everybody's canvas.  The entry's
// own pieces follow from `end`.
struct CanvasTable {
    std::vector<int> slot, count;   // per canvas of the call: its DrawFrame or -1, its people
    int used = 0;                   // DrawFrames
    size_t off_order = 0, off_pframe = 0, end = 0;
    CanvasTable(int nframes, int n, const int32_t *frame_index) : slot(nframes, -1), count(nframes, 0) {
        for (int i = 0; i < n; ++i) ++count[frame_index ? frame_index[i] : 0];
        for (int f = 0; f < nframes; ++f)
            if (count[f]) slot[f] = used++;
        off_order = align16((size_t)used * sizeof(DrawFrame)), off_pframe = off_order + align16((size_t)n * 4);
        end = off_pframe + align16((size_t)n * 4);
    }
    // fills the three pieces at `pin`; size_of(canvas) goes into DrawFrame::radius; returns the tiles of the launch
    template <class Size>
    int fill(char *pin, const hrn_canvas *canvases, int n, const int32_t *frame_index, const Size &size_of) const {
        DrawFrame *frames = (DrawFrame *)pin;
        int *order = (int *)(pin + off_order), *pframe = (int *)(pin + off_pframe);
        int tiles = 0, people = 0;
        for (int f = 0; f < (int)slot.size(); ++f) {
            if (slot[f] < 0) continue;
            const hrn_canvas &c = canvases[f];
            DrawFrame &d = frames[slot[f]];
            d.p0 = c.y, d.p1 = c.format == HRN_PIX_BGR ? nullptr : c.u, d.p2 = c.format == HRN_PIX_I420 ? c.v : nullptr;
            d.height = c.height, d.width = c.width, d.pitch0 = c.pitch_y, d.pitch1 = c.format == HRN_PIX_BGR ? 0 : c.pitch_c;
            d.format = c.format;
            d.radius = size_of(c);
            d.tile_start = tiles, d.tiles_x = (c.width + kDrawTile - 1) / kDrawTile;
            tiles += d.tiles_x * ((c.height + kDrawTile - 1) / kDrawTile);                      // (at most 256 x 256 per canvas)
            d.person_start = people, d.person_count = 0;
            people += count[f];
        }
        for (int i = 0; i < n; ++i) {
            DrawFrame &d = frames[slot[frame_index ? frame_index[i] : 0]];
            order[d.person_start + d.person_count++] = i;
            pframe[i] = (int)(&d - frames);
        }
        return tiles;
    }
};
}  // extern "C++"
}  // namespace

namespace {
// misc/visualization.py:71-192 for every person of every frame, the one body of hrn_draw_poses (person_index_dev == nullptr) and
// hrn_draw_poses_ids_dev (ids_on_device): the arguments are judged first (they need no device), then the handle; one table
// upload and two launches follow (three with the ids on the device)
int draw_poses(const char *entry, hrn_handle h, const hrn_canvas *canvases_host, int nframes, const float *pts_dev, int n, int J,
               const int32_t *frame_index_host, const int32_t *skeleton_host, int K, const uint8_t *point_colors_host, int Cp,
               const uint8_t *bone_colors_host, int Cb, const int32_t *person_index_host, const int32_t *person_index_dev,
               bool ids_on_device, int radius, int thickness, float threshold, void *stream) {
    if (!h) return 1;
    const auto fail = [&](const std::string &what) {
        h->err = std::string(entry) + ": " + what;
        return 7;
    };
    if (ids_on_device && n > 0 && !person_index_dev) return fail("null person_index_dev");
    if (n < 0) return fail("n is negative");
    if (J < 1 || J > HRN_MAX_JOINTS) return fail("J must be in [1, " + std::to_string(HRN_MAX_JOINTS) + "]");
    if (K < 0 || K > kDrawMaxBones) return fail("K must be in [0, " + std::to_string(kDrawMaxBones) + "]");
    if (Cp < 1 || Cb < 1) return fail("Cp and Cb must be at least 1");
    if (thickness < 1 || thickness > 16) return fail("thickness must be in [1, 16]");
    if (radius < 0 || radius > 64) return fail("radius must be in [0, 64]");
    if (!canvases_host || nframes < 1 || !point_colors_host || !bone_colors_host || (K > 0 && !skeleton_host) || (n > 0 && !pts_dev))
        return fail("null canvases / joints / skeleton / colours");
    if (!frame_index_host && nframes != 1) return fail("without frame_index there must be one frame");
    for (int k = 0; k < 2 * K; ++k)
        if (skeleton_host[k] < 0 || skeleton_host[k] >= J)
            return fail("skeleton index " + std::to_string(skeleton_host[k]) + " of bone " + std::to_string(k / 2) + " is outside [0, " +
                        std::to_string(J) + ")");
    const std::string fault = canvas_table_fault(canvases_host, nframes, n, frame_index_host);
    if (!fault.empty()) return fail(fault);
    if (h->refuse_plan_only()) return 7;
    if (n == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;

    // the canvases somebody refers to, in table order, and their people in call order (CanvasTable); then the entry's own pieces
    const CanvasTable ct(nframes, n, frame_index_host);
    const int used = ct.used;
    const size_t off_order = ct.off_order, off_pframe = ct.off_pframe, off_bone = ct.end, off_point = off_bone + align16((size_t)n * 4),
                 off_skel = off_point + align16((size_t)Cp * 4), off_palette = off_skel + align16((size_t)std::max(K, 1) * 4),
                 table_bytes = off_palette + (ids_on_device ? align16((size_t)Cb * 4) : 0);   // (host ids: the table ends at off_palette)
    const PinnedImage img = h->image(table_bytes);
    if (!img) return 6;
    char *pin = img.ptr;
    unsigned *bone = (unsigned *)(pin + off_bone), *point = (unsigned *)(pin + off_point), *skel = (unsigned *)(pin + off_skel);
    const int tiles = ct.fill(pin, canvases_host, n, frame_index_host, [&](const hrn_canvas &c) {
        return radius > 0 ? radius : std::max(1, std::min(c.height, c.width) / 160);   // (at most 8192 / 160 = 51)
    });
    for (int i = 0; i < n; ++i) {
        const long id = person_index_host ? (long)person_index_host[i] : (long)i;
        bone[i] = ids_on_device ? 0u : pack_colour(bone_colors_host + 3 * (size_t)(((id % Cb) + Cb) % Cb));   // Python's modulo
    }
    if (ids_on_device)   // the palette travels with the table; a launch behind the copy fills bone[] from the ids on the device
        for (int k = 0; k < Cb; ++k) ((unsigned *)(pin + off_palette))[k] = pack_colour(bone_colors_host + 3 * (size_t)k);
    for (int k = 0; k < Cp; ++k) point[k] = pack_colour(point_colors_host + 3 * (size_t)k);
    for (int k = 0; k < K; ++k) skel[k] = (unsigned)skeleton_host[2 * k] | ((unsigned)skeleton_host[2 * k + 1] << 16);

    const size_t off_live = align16((size_t)n * J * sizeof(short2)), off_box = off_live + align16((size_t)n * (kMaxJoints / 32) * 4),
                 rec_bytes = off_box + (size_t)n * sizeof(int4);
    CallFrame frame(h, s, {{&h->draw_table, table_bytes, hrn_ctx::twice(table_bytes, 4096), "hipMalloc(draw table)"},
                           {&h->draw_records, rec_bytes, hrn_ctx::twice(rec_bytes, 4096), "hipMalloc(draw records)"}});
    char *table = frame.upload(img, table_bytes, "hipMemcpyAsync(draw table)"), *records = frame.dev(h->draw_records);
    if (!table) return 6;
    if (ids_on_device && !h->hip_ok(launch_bone_ids(person_index_dev, n, (const unsigned *)(table + off_palette), Cb,
                                                    (unsigned *)(table + off_bone), s), "bone colour launch"))
        return 8;
    DrawArgs a{};
    a.pts = pts_dev, a.n = n, a.J = J, a.K = K, a.Cp = Cp, a.nframes = used, a.total_tiles = tiles, a.thickness = thickness;
    a.threshold = threshold;
    a.frames = (const DrawFrame *)table, a.order = (const int *)(table + off_order);
    a.person_frame = (const int *)(table + off_pframe), a.bone_colour = (const unsigned *)(table + off_bone);
    a.point_colour = (const unsigned *)(table + off_point), a.skeleton = (const unsigned *)(table + off_skel);
    a.xy = (short2 *)records, a.live = (unsigned *)(records + off_live), a.box = (int4 *)(records + off_box);
    if (!h->hip_ok(launch_draw(a, s), "draw launch")) return 8;
    return frame.leave() ? 0 : 6;
}
}  // namespace

int hrn_draw_poses(hrn_handle h, const hrn_canvas *canvases_host, int nframes, const float *pts_dev, int n, int J,
                   const int32_t *frame_index_host, const int32_t *skeleton_host, int K, const uint8_t *point_colors_host, int Cp,
                   const uint8_t *bone_colors_host, int Cb, const int32_t *person_index_host, int radius, int thickness,
                   float threshold, void *stream) {
    return draw_poses("hrn_draw_poses", h, canvases_host, nframes, pts_dev, n, J, frame_index_host, skeleton_host, K, point_colors_host,
                      Cp, bone_colors_host, Cb, person_index_host, nullptr, false, radius, thickness, threshold, stream);
}

int hrn_draw_poses_ids_dev(hrn_handle h, const hrn_canvas *canvases_host, int nframes, const float *pts_dev, int n, int J,
                           const int32_t *frame_index_host, const int32_t *skeleton_host, int K, const uint8_t *point_colors_host,
                           int Cp, const uint8_t *bone_colors_host, int Cb, const int32_t *person_index_dev, int radius,
                           int thickness, float threshold, void *stream) {
    return draw_poses("hrn_draw_poses_ids_dev", h, canvases_host, nframes, pts_dev, n, J, frame_index_host, skeleton_host, K,
                      point_colors_host, Cp, bone_colors_host, Cb, nullptr, person_index_dev, true, radius, thickness, threshold, stream);
}

// ---- person labels: the box, the id and the score of every person drawn beside it (draw_labels_math.h, draw.hip) ----------------
static thread_local std::string g_label_error;

int hrn_label_layout(const int32_t *box, int has_id, int32_t id, int has_score, float score, int scale, int thickness,
                     hrn_label_record *record_out) {
    static_assert(sizeof(hrn_label_record) == sizeof(LabelRecord), "hrn_label_record is LabelRecord");
    g_label_error.clear();
    if (!box || !record_out) g_label_error = "null box / record";
    else if (scale < 1 || scale > kLabelMaxScale) g_label_error = "scale must be in [1, " + std::to_string(kLabelMaxScale) + "]";
    else if (thickness < 0 || thickness > kLabelMaxThickness)
        g_label_error = "thickness must be in [0, " + std::to_string(kLabelMaxThickness) + "]";
    if (!g_label_error.empty()) return 7;
    const LabelRecord r = label_layout(box, has_id != 0, id, has_score != 0, score, scale, thickness);
    memcpy(record_out, &r, sizeof(r));
    return 0;
}

// 0: not covered, 1: the person's colour (plate or outline), 2: the person's text colour (ink); 7 on a bad record
int hrn_label_covers(const hrn_label_record *record, int px, int py) {
    g_label_error.clear();
    if (!record) g_label_error = "null record";
    else if (record->drawn && (record->scale < 1 || record->scale > kLabelMaxScale || record->thickness < 0 ||
                               record->thickness > kLabelMaxThickness || record->ncells < 0 || record->ncells > kLabelMaxCells))
        g_label_error = "the record is not one hrn_label_layout wrote";
    if (!g_label_error.empty()) return 7;
    LabelRecord r;
    memcpy(&r, record, sizeof(r));
    return label_covers(r, px, py);
}

const char *hrn_label_last_error(void) { return g_label_error.c_str(); }

// the arguments are judged first (they need no device), then the handle; one table upload and two launches follow
int hrn_draw_labels_dev(hrn_handle h, const hrn_canvas *canvases_host, int nframes, const int32_t *boxes_dev, const int32_t *ids_dev,
                        const float *scores_dev, int score_stride, int n, const int32_t *frame_index_host, const uint8_t *colors_host,
                        const uint8_t *text_colors_host, int Cb, int scale, int thickness, void *stream) {
    if (!h) return 1;
    const auto fail = [&](const std::string &what) {
        h->err = "hrn_draw_labels_dev: " + what;
        return 7;
    };
    if (n < 0) return fail("n is negative");
    if (Cb < 1) return fail("Cb must be at least 1");
    if (scale < 0 || scale > kLabelMaxScale) return fail("scale must be in [0, " + std::to_string(kLabelMaxScale) + "]");
    if (thickness < 0 || thickness > kLabelMaxThickness) return fail("thickness must be in [0, " + std::to_string(kLabelMaxThickness) + "]");
    if (scores_dev && score_stride < 1) return fail("score_stride must be at least 1");
    if (!canvases_host || nframes < 1 || !colors_host || !text_colors_host || (n > 0 && !boxes_dev)) return fail("null canvases / boxes / colours");
    if (!frame_index_host && nframes != 1) return fail("without frame_index there must be one frame");
    const std::string fault = canvas_table_fault(canvases_host, nframes, n, frame_index_host);
    if (!fault.empty()) return fail(fault);
    if (h->refuse_plan_only()) return 7;
    if (n == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;

    const CanvasTable ct(nframes, n, frame_index_host);
    const size_t off_colour = ct.end, off_text = off_colour + align16((size_t)Cb * 4), table_bytes = off_text + align16((size_t)Cb * 4);
    const PinnedImage img = h->image(table_bytes);
    if (!img) return 6;
    const int tiles = ct.fill(img.ptr, canvases_host, n, frame_index_host, [&](const hrn_canvas &c) {
        return scale > 0 ? scale : std::min(kLabelMaxScale, std::max(1, std::min(c.height, c.width) / 360));   // (the glyph scale)
    });
    for (int k = 0; k < Cb; ++k) {
        img.as<unsigned>(off_colour)[k] = pack_colour(colors_host + 3 * (size_t)k);
        img.as<unsigned>(off_text)[k] = pack_colour(text_colors_host + 3 * (size_t)k);
    }
    const size_t off_reach = (size_t)n * sizeof(LabelRecord), rec_bytes = off_reach + (size_t)n * sizeof(int4);
    CallFrame frame(h, s, {{&h->draw_table, table_bytes, hrn_ctx::twice(table_bytes, 4096), "hipMalloc(draw table)"},
                           {&h->draw_records, rec_bytes, hrn_ctx::twice(rec_bytes, 4096), "hipMalloc(draw records)"}});
    char *table = frame.upload(img, table_bytes, "hipMemcpyAsync(draw table)"), *records = frame.dev(h->draw_records);
    if (!table) return 6;
    LabelArgs a{};
    a.boxes = boxes_dev, a.ids = ids_dev, a.scores = scores_dev, a.score_stride = score_stride, a.n = n, a.Cb = Cb;
    a.nframes = ct.used, a.total_tiles = tiles, a.thickness = thickness;
    a.frames = (const DrawFrame *)table, a.order = (const int *)(table + ct.off_order), a.person_frame = (const int *)(table + ct.off_pframe);
    a.colour = (const unsigned *)(table + off_colour), a.text_colour = (const unsigned *)(table + off_text);
    a.records = (LabelRecord *)records, a.reach = (int4 *)(records + off_reach);
    if (!h->hip_ok(launch_draw_labels(a, s), "label launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// ---- heat-map overlays: the maximum over the chosen joints, coloured and blended into the frame (heat_math.h, heat.hip) -----------
static thread_local std::string g_heat_error;

namespace {
extern "C++" {
// what is wrong with the arguments the three heat-map entries share, or "" (canvases: hrn_draw_poses' checks, when there are any)
std::string heat_fault(const hrn_canvas *canvases, int nframes, bool with_canvases, const void *maps, const void *boxes, int n, int J,
                       int hq, int wq, const int32_t *frame_index, const uint8_t *joint_mask, float lo, float hi, const uint8_t *lut,
                       int alpha, int alpha_mode, int cutoff) {
    if (n < 0) return "n is negative";
    if (J < 1 || J > HRN_MAX_JOINTS) return "J must be in [1, " + std::to_string(HRN_MAX_JOINTS) + "]";
    if (hq < 1 || hq > kHeatMaxSide || wq < 1 || wq > kHeatMaxSide) return "hq and wq must be in [1, " + std::to_string(kHeatMaxSide) + "]";
    if (!std::isfinite(lo) || !std::isfinite(hi)) return "lo and hi must be finite";
    if (!(hi > lo)) return "hi must be above lo";
    if (joint_mask) {
        bool any = false;
        for (int j = 0; j < J; ++j) any = any || joint_mask[j] != 0;
        if (!any) return "the joint mask selects no joint";
    }
    if (!with_canvases) return n > 0 && !maps ? "null heat-maps" : "";
    if (alpha < 0 || alpha > 255) return "alpha must be in [0, 255]";
    if (alpha_mode != HRN_HEAT_ALPHA_CONST && alpha_mode != HRN_HEAT_ALPHA_VALUE)
        return "alpha_mode must be HRN_HEAT_ALPHA_CONST or HRN_HEAT_ALPHA_VALUE";
    if (cutoff < 1 || cutoff > 255) return "cutoff must be in [1, 255]";
    if (!canvases || nframes < 1 || !lut || (n > 0 && (!maps || !boxes))) return "null canvases / heat-maps / boxes / colour table";
    if (!frame_index && nframes != 1) return "without frame_index there must be one frame";
    return canvas_table_fault(canvases, nframes, n, frame_index);
}
}  // extern "C++"
// one person's Q (hq, wq) from its (J, hq, wq) maps: the host's form of heat_reduce_kernel
void heat_quantise_person(const float *maps, int J, int cells, const uint8_t *joint_mask, float lo, float k, uint8_t *out) {
    for (int c = 0; c < cells; ++c) {
        float v = __builtin_nanf("");
        for (int j = 0; j < J; ++j)
            if (!joint_mask || joint_mask[j]) v = heat_max(v, maps[(size_t)j * cells + c]);
        out[c] = (uint8_t)heat_quantise(v, lo, k);
    }
}
}  // namespace

const char *hrn_heatmap_last_error(void) { return g_heat_error.c_str(); }

int hrn_heatmap_quantise(const float *maps, int n, int J, int hq, int wq, const uint8_t *joint_mask, float lo, float hi, uint8_t *out) {
    g_heat_error = heat_fault(nullptr, 0, false, maps, nullptr, n, J, hq, wq, nullptr, joint_mask, lo, hi, nullptr, 0, 0, 1);
    if (g_heat_error.empty() && n > 0 && !out) g_heat_error = "null output";
    if (!g_heat_error.empty()) return 7;
    const float k = 255.0f / (hi - lo);
    const int cells = hq * wq;
    for (int i = 0; i < n; ++i) heat_quantise_person(maps + (size_t)i * J * cells, J, cells, joint_mask, lo, k, out + (size_t)i * cells);
    return 0;
}

// the whole definition on the CPU: Q of everybody, then per canvas one full-frame V and the blend
int hrn_draw_heatmaps_host(const hrn_canvas *canvases_host, int nframes, const float *heatmaps_host, const int32_t *boxes_host, int n, int J,
                           int hq, int wq, const int32_t *frame_index_host, const uint8_t *joint_mask_host, float lo, float hi,
                           const uint8_t *lut_host, int alpha, int alpha_mode, int cutoff) {
    g_heat_error = heat_fault(canvases_host, nframes, true, heatmaps_host, boxes_host, n, J, hq, wq, frame_index_host, joint_mask_host, lo,
                              hi, lut_host, alpha, alpha_mode, cutoff);
    if (!g_heat_error.empty()) return 7;
    if (n == 0) return 0;
    const float k = 255.0f / (hi - lo);
    const int cells = hq * wq;
    std::vector<uint8_t> q((size_t)n * cells);
    for (int i = 0; i < n; ++i)
        heat_quantise_person(heatmaps_host + (size_t)i * J * cells, J, cells, joint_mask_host, lo, k, q.data() + (size_t)i * cells);
    std::vector<uint8_t> V;
    for (int f = 0; f < nframes; ++f) {
        std::vector<int> people;
        for (int i = 0; i < n; ++i)
            if ((frame_index_host ? frame_index_host[i] : 0) == f) people.push_back(i);
        if (people.empty()) continue;
        const hrn_canvas &c = canvases_host[f];
        const int H = c.height, W = c.width;
        V.assign((size_t)H * W, 0);
        for (int i : people) {
            const int32_t *b = boxes_host + 4 * (size_t)i;
            if (!heat_box_drawn(b[0], b[1], b[2], b[3])) continue;
            const int bw = b[2] - b[0], bh = b[3] - b[1];
            for (int py = std::max(b[1], 0); py < std::min(b[3], H); ++py) {
                const int uy = heat_coord(py - b[1], hq, bh);
                for (int px = std::max(b[0], 0); px < std::min(b[2], W); ++px) {
                    const int S = heat_sample(q.data() + (size_t)i * cells, hq, wq, heat_coord(px - b[0], wq, bw), uy);
                    uint8_t &v = V[(size_t)py * W + px];
                    if (S > v) v = (uint8_t)S;
                }
            }
        }
        const auto colour = [&](int v, int ch) { return (int)lut_host[3 * v + ch]; };
        if (c.format == HRN_PIX_BGR) {
            for (int py = 0; py < H; ++py)
                for (int px = 0; px < W; ++px) {
                    const int v = V[(size_t)py * W + px];
                    int a;
                    if (!heat_written(v, alpha, alpha_mode, cutoff, &a)) continue;
                    uint8_t *dst = c.y + (size_t)py * c.pitch_y + 3 * (size_t)px;
                    for (int ch = 0; ch < 3; ++ch) dst[ch] = (uint8_t)heat_blend(dst[ch], colour(v, ch), a);
                }
            continue;
        }
        for (int by = 0; by < H / 2; ++by)
            for (int bx = 0; bx < W / 2; ++bx) {
                int v4[4];
                bool any = false;
                for (int p = 0; p < 4; ++p) {
                    const int py = 2 * by + (p >> 1), px = 2 * bx + (p & 1);
                    v4[p] = V[(size_t)py * W + px];
                    int a;
                    if (!heat_written(v4[p], alpha, alpha_mode, cutoff, &a)) continue;
                    uint8_t *dst = c.y + (size_t)py * c.pitch_y + px;
                    *dst = (uint8_t)heat_blend(*dst, colour(v4[p], 0), a);
                    any = true;
                }
                if (!any) continue;
                const int vc = heat_block_value(v4[0], v4[1], v4[2], v4[3]), ac = heat_alpha(vc, alpha, alpha_mode);
                if (ac <= 0) continue;
                uint8_t *u = c.format == HRN_PIX_NV12 ? c.u + (size_t)by * c.pitch_c + 2 * bx : c.u + (size_t)by * c.pitch_c + bx;
                uint8_t *v = c.format == HRN_PIX_NV12 ? u + 1 : c.v + (size_t)by * c.pitch_c + bx;
                *u = (uint8_t)heat_blend(*u, colour(vc, 1), ac);
                *v = (uint8_t)heat_blend(*v, colour(vc, 2), ac);
            }
    }
    return 0;
}

// the arguments are judged first (they need no device), then the handle; one table upload and two launches follow
int hrn_draw_heatmaps_dev(hrn_handle h, const hrn_canvas *canvases_host, int nframes, const float *heatmaps_dev, const int32_t *boxes_dev,
                          int n, int J, int hq, int wq, const int32_t *frame_index_host, const uint8_t *joint_mask_host, float lo, float hi,
                          const uint8_t *lut_host, int alpha, int alpha_mode, int cutoff, void *stream) {
    if (!h) return 1;
    const std::string fault = heat_fault(canvases_host, nframes, true, heatmaps_dev, boxes_dev, n, J, hq, wq, frame_index_host,
                                         joint_mask_host, lo, hi, lut_host, alpha, alpha_mode, cutoff);
    if (!fault.empty()) {
        h->err = "hrn_draw_heatmaps_dev: " + fault;
        return 7;
    }
    if (h->refuse_plan_only()) return 7;
    if (n == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;

    const CanvasTable ct(nframes, n, frame_index_host);
    const size_t off_lut = ct.end, table_bytes = off_lut + 256 * 4;
    const PinnedImage img = h->image(table_bytes);
    if (!img) return 6;
    const int tiles = ct.fill(img.ptr, canvases_host, n, frame_index_host, [](const hrn_canvas &) { return 0; });
    for (int v = 0; v < 256; ++v) img.as<unsigned>(off_lut)[v] = pack_colour(lut_host + 3 * (size_t)v);
    const size_t q_bytes = (size_t)n * hq * wq;
    CallFrame frame(h, s, {{&h->draw_table, table_bytes, hrn_ctx::twice(table_bytes, 4096), "hipMalloc(draw table)"},
                           {&h->draw_records, q_bytes, hrn_ctx::twice(q_bytes, 4096), "hipMalloc(quantised heat-maps)"}});
    char *table = frame.upload(img, table_bytes, "hipMemcpyAsync(draw table)"), *records = frame.dev(h->draw_records);
    if (!table) return 6;
    HeatArgs a{};
    a.maps = heatmaps_dev, a.boxes = boxes_dev, a.n = n, a.J = J, a.hq = hq, a.wq = wq, a.nframes = ct.used, a.total_tiles = tiles;
    a.lo = lo, a.k = 255.0f / (hi - lo), a.alpha = alpha, a.mode = alpha_mode, a.cutoff = cutoff;
    static_assert(kMaxJoints <= 256, "a joint index fits a byte");
    for (int j = 0; j < J; ++j)
        if (!joint_mask_host || joint_mask_host[j]) a.joints[a.njoints++] = (unsigned char)j;
    a.frames = (const DrawFrame *)table, a.order = (const int *)(table + ct.off_order), a.lut = (const unsigned *)(table + off_lut);
    a.q = (unsigned char *)records;
    if (!h->hip_ok(launch_draw_heatmaps(a, s), "heat-map launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// ---- the face mosaic: a square around chosen joints, or a box, pixelated in place (mosaic_math.h, mosaic.hip) -------------------
static thread_local std::string g_mosaic_error;

namespace {
extern "C++" {
// what is wrong with the arguments the mosaic entries share, or "" (canvases: hrn_draw_poses' checks, when there are any)
std::string mosaic_fault(const hrn_canvas *canvases, int nframes, bool with_canvases, const void *pts, int n, int J, const int32_t *joints,
                         int K, const void *boxes, const int32_t *frame_index, int scale_num, int scale_den, int min_half, int cell) {
    if (n < 0) return "n is negative";
    if (pts && boxes) return "people come from pts or from boxes, not from both";
    if (n > 0 && !pts && !boxes) return "null pts and boxes: people come from one of them";
    if (!boxes && (n > 0 || pts || joints)) {
        if (J < 1 || J > HRN_MAX_JOINTS) return "J must be in [1, " + std::to_string(HRN_MAX_JOINTS) + "]";
        if (K < 1 || K > kMosaicMaxList) return "K must be in [1, " + std::to_string(kMosaicMaxList) + "]";
        if (!joints) return "null joint list";
        for (int k = 0; k < K; ++k)
            if (joints[k] < 0 || joints[k] >= J)
                return "joint index " + std::to_string(joints[k]) + " at position " + std::to_string(k) + " of the list is outside [0, " +
                       std::to_string(J) + ")";
    }
    if (scale_num < 1 || scale_num > kMosaicMaxScale || scale_den < 1 || scale_den > kMosaicMaxScale)
        return "scale_num and scale_den must be in [1, " + std::to_string(kMosaicMaxScale) + "]";
    if (min_half < 0 || min_half > kMosaicMaxHalf) return "min_half must be in [0, " + std::to_string(kMosaicMaxHalf) + "]";
    if (!with_canvases) return "";
    if (!mosaic_cell_valid(cell)) return "cell must be 0, 2, 4, 8, 16 or 32";
    if (!canvases || nframes < 1) return "null canvases";
    if (!frame_index && nframes != 1) return "without frame_index there must be one frame";
    return canvas_table_fault(canvases, nframes, n, frame_index);
}
}  // extern "C++"
// the joints of the list as a bit set (a repeated index marks its bit once more)
void mosaic_listed_bits(const int32_t *joints, int K, uint32_t *bits /* kMaxJoints / 32 */) {
    for (int w = 0; w < kMaxJoints / 32; ++w) bits[w] = 0;
    for (int k = 0; k < K; ++k) bits[joints[k] >> 5] |= 1u << (joints[k] & 31);
}
// person i's region on a canvas of H x W from whichever source the call has: the host's form of mosaic_build_kernel
int mosaic_person_region(const float *pts, int J, const uint32_t *bits, const int32_t *boxes, int i, float threshold, int scale_num,
                         int scale_den, int min_half, int H, int W, int *out) {
    if (boxes) return mosaic_region_of_box(boxes + 4 * (size_t)i, H, W, out);
    return mosaic_region_of_person(pts + (size_t)i * J * 3, J, bits, threshold, scale_num, scale_den, min_half, H, W, out);
}
}  // namespace

const char *hrn_mosaic_last_error(void) { return g_mosaic_error.c_str(); }

int hrn_mosaic_regions(const float *pts, int n, int J, const int32_t *joints, int K, const int32_t *boxes, const int32_t *canvas_hw,
                       float threshold, int scale_num, int scale_den, int min_half, int32_t *regions_out, int32_t *status_out) {
    g_mosaic_error = mosaic_fault(nullptr, 0, false, pts, n, J, joints, K, boxes, nullptr, scale_num, scale_den, min_half, 0);
    if (g_mosaic_error.empty() && n > 0 && (!canvas_hw || !regions_out || !status_out)) g_mosaic_error = "null canvas sizes / outputs";
    for (int i = 0; g_mosaic_error.empty() && i < n; ++i)
        if (canvas_hw[2 * i] < 1 || canvas_hw[2 * i] > 8192 || canvas_hw[2 * i + 1] < 1 || canvas_hw[2 * i + 1] > 8192)
            g_mosaic_error = "the canvas size of person " + std::to_string(i) + " is outside [1, 8192]";
    if (!g_mosaic_error.empty()) return 7;
    uint32_t bits[kMaxJoints / 32] = {};
    if (!boxes && n > 0) mosaic_listed_bits(joints, K, bits);
    for (int i = 0; i < n; ++i)
        status_out[i] = mosaic_person_region(pts, J, bits, boxes, i, threshold, scale_num, scale_den, min_half, canvas_hw[2 * i],
                                             canvas_hw[2 * i + 1], regions_out + 4 * (size_t)i);
    return 0;
}

// the whole definition on the CPU: everybody's region, then per canvas the marks of its cell grid and the means of the marked cells
int hrn_mosaic_host(const hrn_canvas *canvases_host, int nframes, const float *pts_host, int n, int J, const int32_t *joints_host, int K,
                    const int32_t *boxes_host, const int32_t *frame_index_host, float threshold, int scale_num, int scale_den,
                    int min_half, int cell, int32_t *status_out) {
    g_mosaic_error = mosaic_fault(canvases_host, nframes, true, pts_host, n, J, joints_host, K, boxes_host, frame_index_host, scale_num,
                                  scale_den, min_half, cell);
    if (!g_mosaic_error.empty()) return 7;
    if (n == 0) return 0;
    uint32_t bits[kMaxJoints / 32] = {};
    if (!boxes_host) mosaic_listed_bits(joints_host, K, bits);
    std::vector<int> region((size_t)4 * n);
    for (int i = 0; i < n; ++i) {
        const hrn_canvas &c = canvases_host[frame_index_host ? frame_index_host[i] : 0];
        const int st = mosaic_person_region(pts_host, J, bits, boxes_host, i, threshold, scale_num, scale_den, min_half, c.height, c.width,
                                            &region[4 * (size_t)i]);
        if (status_out) status_out[i] = st;
    }
    std::vector<uint8_t> marks;
    for (int f = 0; f < nframes; ++f) {
        const hrn_canvas &c = canvases_host[f];
        int s = 0, gw = 0, gh = 0;
        for (int i = 0; i < n; ++i) {
            if ((frame_index_host ? frame_index_host[i] : 0) != f) continue;
            if (!s) {   // (a canvas somebody refers to has been judged: its sides are positive)
                s = mosaic_cell_size(cell, c.height, c.width), gw = (c.width + s - 1) / s, gh = (c.height + s - 1) / s;
                marks.assign((size_t)gw * gh, 0);
            }
            const int *r = &region[4 * (size_t)i];
            if (r[2] <= r[0]) continue;
            for (int cy = r[1] / s; cy <= (r[3] - 1) / s; ++cy)
                for (int cx = r[0] / s; cx <= (r[2] - 1) / s; ++cx) marks[(size_t)cy * gw + cx] = 1;
        }
        if (!s) continue;
        const bool bgr = c.format == HRN_PIX_BGR;
        for (int cy = 0; cy < gh; ++cy)
            for (int cx = 0; cx < gw; ++cx) {
                if (!marks[(size_t)cy * gw + cx]) continue;
                const int x0 = cx * s, y0 = cy * s, w = std::min(s, c.width - x0), h = std::min(s, c.height - y0);
                const int count = mosaic_cell_count(x0, y0, s, c.height, c.width);
                // one channel of the cell: its first byte, the bytes between rows and between samples, its rows and columns
                const auto flatten = [](uint8_t *first, int pitch, int step, int rows, int cols, int cnt) {
                    int sum = 0;
                    for (int y = 0; y < rows; ++y)
                        for (int x = 0; x < cols; ++x) sum += first[(size_t)y * pitch + (size_t)x * step];
                    const uint8_t m = (uint8_t)mosaic_mean(sum, cnt);
                    for (int y = 0; y < rows; ++y)
                        for (int x = 0; x < cols; ++x) first[(size_t)y * pitch + (size_t)x * step] = m;
                };
                if (bgr) {
                    for (int ch = 0; ch < 3; ++ch) flatten(c.y + (size_t)y0 * c.pitch_y + 3 * (size_t)x0 + ch, c.pitch_y, 3, h, w, count);
                    continue;
                }
                flatten(c.y + (size_t)y0 * c.pitch_y + x0, c.pitch_y, 1, h, w, count);
                if (c.format == HRN_PIX_NV12) {
                    flatten(c.u + (size_t)(y0 / 2) * c.pitch_c + x0, c.pitch_c, 2, h / 2, w / 2, count / 4);
                    flatten(c.u + (size_t)(y0 / 2) * c.pitch_c + x0 + 1, c.pitch_c, 2, h / 2, w / 2, count / 4);
                } else {
                    flatten(c.u + (size_t)(y0 / 2) * c.pitch_c + x0 / 2, c.pitch_c, 1, h / 2, w / 2, count / 4);
                    flatten(c.v + (size_t)(y0 / 2) * c.pitch_c + x0 / 2, c.pitch_c, 1, h / 2, w / 2, count / 4);
                }
            }
    }
    return 0;
}

// the arguments are judged first (they need no device), then the handle; one table upload and two launches follow
int hrn_mosaic_dev(hrn_handle h, const hrn_canvas *canvases_host, int nframes, const float *pts_dev, int n, int J,
                   const int32_t *joints_host, int K, const int32_t *boxes_dev, const int32_t *frame_index_host, float threshold,
                   int scale_num, int scale_den, int min_half, int cell, int32_t *status_dev, void *stream) {
    if (!h) return 1;
    const std::string fault = mosaic_fault(canvases_host, nframes, true, pts_dev, n, J, joints_host, K, boxes_dev, frame_index_host,
                                           scale_num, scale_den, min_half, cell);
    if (!fault.empty()) {
        h->err = "hrn_mosaic_dev: " + fault;
        return 7;
    }
    if (h->refuse_plan_only()) return 7;
    if (n == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;

    const CanvasTable ct(nframes, n, frame_index_host);
    const size_t off_listed = ct.end, table_bytes = off_listed + (kMaxJoints / 32) * 4;
    const PinnedImage img = h->image(table_bytes);
    if (!img) return 6;
    const int tiles = ct.fill(img.ptr, canvases_host, n, frame_index_host,
                              [&](const hrn_canvas &c) { return mosaic_cell_size(cell, c.height, c.width); });
    if (boxes_dev) memset(img.as<unsigned>(off_listed), 0, (kMaxJoints / 32) * 4);
    else mosaic_listed_bits(joints_host, K, img.as<unsigned>(off_listed));
    const size_t rec_bytes = (size_t)n * sizeof(int4);
    CallFrame frame(h, s, {{&h->draw_table, table_bytes, hrn_ctx::twice(table_bytes, 4096), "hipMalloc(draw table)"},
                           {&h->draw_records, rec_bytes, hrn_ctx::twice(rec_bytes, 4096), "hipMalloc(mosaic regions)"}});
    char *table = frame.upload(img, table_bytes, "hipMemcpyAsync(draw table)"), *records = frame.dev(h->draw_records);
    if (!table) return 6;
    MosaicArgs a{};
    a.pts = pts_dev, a.boxes = boxes_dev, a.n = n, a.J = J, a.nframes = ct.used, a.total_tiles = tiles, a.threshold = threshold;
    a.scale_num = scale_num, a.scale_den = scale_den, a.min_half = min_half;
    a.frames = (const DrawFrame *)table, a.order = (const int *)(table + ct.off_order), a.person_frame = (const int *)(table + ct.off_pframe);
    a.listed = (const unsigned *)(table + off_listed), a.status = status_dev, a.region = (int4 *)records;
    if (!h->hip_ok(launch_mosaic(a, s), "mosaic launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// find_person_id_associations and the demo's next_id update for P problems in one launch (assoc.hip); the arguments are judged
// first (assoc_math.h's assoc_fault, as in the host form: they need no device), then the handle
int hrn_associate_people_dev(hrn_handle h, int P, const int32_t *cur_start_host, const int32_t *prev_start_host, int J,
                             int32_t *boxes_dev, float *pts_dev, const int32_t *prev_boxes_dev, const float *prev_pts_dev,
                             const int32_t *prev_ids_dev, int32_t *next_id_dev, double pose_alpha, double similarity_threshold,
                             double smoothing_alpha, int32_t *ids_dev, int32_t *match_dev, int32_t *status_dev, void *stream) {
    if (!h) return 1;
    if (refused(h, "hrn_associate_people_dev",
                assoc_fault(P, cur_start_host, prev_start_host, J, boxes_dev, pts_dev, prev_boxes_dev, prev_pts_dev, prev_ids_dev, next_id_dev,
                            pose_alpha, similarity_threshold, smoothing_alpha, ids_dev, match_dev, status_dev)))
        return 7;
    if (P == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;
    // the problems, each with its piece of the scratch behind the table
    const size_t table_bytes = P > 1 ? ((size_t)P * sizeof(AssocProblem) + 255) / 256 * 256 : 0;
    std::vector<AssocProblem> probs((size_t)P);
    size_t need = table_bytes;
    for (int p = 0; p < P; ++p) {
        AssocProblem &q = probs[p];
        q.cur0 = cur_start_host[p], q.n = cur_start_host[p + 1] - q.cur0;
        q.prev0 = prev_start_host[p], q.m = prev_start_host[p + 1] - q.prev0;
        q.scratch = (long long)need;
        need += ((size_t)q.n * q.m * 12 + 15) / 16 * 16;
    }
    CallFrame frame(h, s, {{&h->assoc_buf, need, hrn_ctx::twice(need, 65536), "hipMalloc(association scratch)"}});
    AssocArgs a{};
    a.P = P, a.J = J, a.no_assign = h->assoc_no_assign ? 1 : 0;
    if (P > 1) a.table = frame.table(probs.data(), (size_t)P, "hipMemcpyAsync(association table)");
    else a.one = probs[0];
    if (!frame.ok()) return 6;
    a.boxes = boxes_dev, a.pts = pts_dev, a.prev_boxes = prev_boxes_dev, a.prev_pts = prev_pts_dev, a.prev_ids = prev_ids_dev;
    a.next_id = next_id_dev, a.pose_alpha = pose_alpha, a.similarity_threshold = similarity_threshold, a.smoothing_alpha = smoothing_alpha;
    a.ids = ids_dev, a.match = match_dev, a.status = status_dev, a.scratch = frame.dev();
    if (!h->hip_ok(launch_assoc(a, s), "association launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// one update of P per-stream track tables in one launch (tracks.hip); the arguments are judged first (tracks_math.h's track_fault,
// as in the host form: they need no device), then the handle.  The scratch per stream: 12 * n * C bytes of costs and similarities
// (at most 768 KiB) and, with coast, the compared state of the C slots (16 * C + 12 * C * J bytes, at most 772 KiB).
int hrn_track_people_dev(hrn_handle h, int P, const int32_t *cur_start_host, int C, int J, int32_t *boxes_dev, float *pts_dev,
                         int32_t *slot_id_dev, int32_t *slot_lost_dev, int32_t *slot_hits_dev, int32_t *slot_row_dev,
                         int32_t *slot_boxes_dev, float *slot_pts_dev, float *slot_vel_dev, int32_t *next_id_dev, double pose_alpha,
                         double similarity_threshold, double smoothing_alpha, int max_lost, int coast, double velocity_alpha,
                         int32_t *ids_dev, int32_t *match_row_dev, int32_t *slot_dev, int32_t *status_dev, void *stream) {
    if (!h) return 1;
    if (refused(h, "hrn_track_people_dev",
                track_fault(P, cur_start_host, C, J, boxes_dev, pts_dev, slot_id_dev, slot_lost_dev, slot_hits_dev, slot_row_dev, slot_boxes_dev,
                            slot_pts_dev, slot_vel_dev, next_id_dev, pose_alpha, similarity_threshold, smoothing_alpha, max_lost, coast,
                            velocity_alpha, ids_dev, match_row_dev, slot_dev, status_dev)))
        return 7;
    if (P == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;
    // the streams, each with its piece of the scratch behind the table
    const size_t table_bytes = P > 1 ? ((size_t)P * sizeof(TrackProblem) + 255) / 256 * 256 : 0;
    const size_t compared = coast ? (size_t)C * 16 + (size_t)C * J * 12 : 0;
    std::vector<TrackProblem> probs((size_t)P);
    size_t need = table_bytes;
    for (int p = 0; p < P; ++p) {
        TrackProblem &q = probs[p];
        q.cur0 = cur_start_host[p], q.n = cur_start_host[p + 1] - q.cur0;
        q.scratch = (long long)need;
        need += ((size_t)q.n * C * 12 + compared + 15) / 16 * 16;
    }
    CallFrame frame(h, s, {{&h->tracks_buf, need, hrn_ctx::twice(need, 65536), "hipMalloc(track table scratch)"}});
    TracksArgs a{};
    a.P = P, a.C = C, a.J = J, a.max_lost = max_lost, a.coast = coast;
    if (P > 1) a.table = frame.table(probs.data(), (size_t)P, "hipMemcpyAsync(track stream table)");
    else a.one = probs[0];
    if (!frame.ok()) return 6;
    a.boxes = boxes_dev, a.pts = pts_dev, a.slot_id = slot_id_dev, a.slot_lost = slot_lost_dev, a.slot_hits = slot_hits_dev;
    a.slot_row = slot_row_dev, a.slot_boxes = slot_boxes_dev, a.slot_pts = slot_pts_dev, a.slot_vel = slot_vel_dev, a.next_id = next_id_dev;
    a.pose_alpha = pose_alpha, a.similarity_threshold = similarity_threshold, a.smoothing_alpha = smoothing_alpha;
    a.velocity_alpha = velocity_alpha;
    a.ids = ids_dev, a.match_row = match_row_dev, a.slot = slot_dev, a.status = status_dev, a.scratch = frame.dev();
    if (!h->hip_ok(launch_tracks(a, s), "track table launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// rescoring and OKS NMS for P problems in one launch (pose_nms.hip); the arguments are judged first (pose_nms_math.h's
// pose_nms_fault, as in the host form: they need no device), then the handle.  Only a call with several problems touches the handle
// (its table), so only that call enters a guard.
int hrn_pose_nms_dev(hrn_handle h, int P, const int32_t *start_host, int J, int flags, void *kpts_dev, void *areas_dev,
                     const void *scores_dev, double thresh, double in_vis_thre, double rescore_thre, const double *sigmas_dev,
                     int32_t *keep_dev, int32_t *num_dev, double *scores_out_dev, int32_t *suppressor_dev, int32_t *status_dev,
                     void *stream) {
    if (!h) return 1;
    if (refused(h, "hrn_pose_nms_dev", pose_nms_fault(P, start_host, J, flags, kpts_dev, areas_dev, scores_dev, thresh, sigmas_dev, keep_dev,
                                                      num_dev, scores_out_dev, suppressor_dev, status_dev)))
        return 7;
    if (P == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;
    const size_t table_bytes = P > 1 ? (size_t)P * sizeof(PoseNmsProblem) : 0;
    CallFrame frame(h, s, {{&h->nms_table, table_bytes, hrn_ctx::twice(table_bytes, 4096), "hipMalloc(pose NMS table)"}});
    PoseNmsArgs a{};
    a.P = P, a.J = J, a.flags = flags;
    a.table = frame.table<PoseNmsProblem>((size_t)P, "hipMemcpyAsync(pose NMS table)", [&](PoseNmsProblem *t) {
        for (int p = 0; p < P; ++p) t[p].first = start_host[p], t[p].n = start_host[p + 1] - start_host[p];
    });
    if (!frame.ok()) return 6;
    if (!a.table) a.one.first = start_host[0], a.one.n = start_host[1] - start_host[0];
    a.kpts = kpts_dev, a.areas = areas_dev, a.scores = scores_dev, a.sigmas = sigmas_dev;
    a.thresh = thresh, a.in_vis_thre = in_vis_thre, a.rescore_thre = rescore_thre;
    a.keep = keep_dev, a.num = num_dev, a.scores_out = scores_out_dev, a.suppressor = suppressor_dev, a.status = status_dev;
    if (!h->hip_ok(launch_pose_nms(a, s), "pose NMS launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// detector NMS for B images in two launches (detector_nms.hip); the arguments are judged first (detector_nms_math.h's dnms_fault,
// as in the host form: they need no device), then the handle.  The handle keeps the scratch of the scoring launch: 32 bytes per
// row of pred, then two ints per block of 256 rows.
int hrn_detector_nms_dev(hrn_handle h, const void *pred_dev, int dtype, int B, int N, int C, int rule, int flags, float conf_thres,
                         float iou_thres, int max_candidates, int max_det, float *rows_dev, int32_t *index_dev, int32_t *counts_dev,
                         int32_t *status_dev, void *stream) {
    if (!h) return 1;
    if (refused(h, "hrn_detector_nms_dev", dnms_fault(pred_dev, dtype, B, N, C, rule, flags, conf_thres, iou_thres, max_candidates, max_det,
                                                      rows_dev, index_dev, counts_dev, status_dev)))
        return 7;
    if (B == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;
    DetectorNmsArgs a{};
    a.nchunks = (N + kDnmsChunk - 1) / kDnmsChunk;
    const size_t cand_bytes = ((size_t)B * N * sizeof(DnmsCand) + 255) / 256 * 256;
    const size_t info_bytes = ((size_t)B * a.nchunks * sizeof(int) + 255) / 256 * 256, need = cand_bytes + 2 * info_bytes;
    CallFrame frame(h, s, {{&h->dnms_buf, need, hrn_ctx::twice(need, 1 << 20), "hipMalloc(detector NMS scratch)"}});
    if (!frame.ok()) return 6;
    a.pred = pred_dev, a.dtype = dtype, a.B = B, a.N = N, a.C = C, a.rule = rule, a.flags = flags;
    a.max_candidates = max_candidates, a.max_det = max_det, a.conf_thres = conf_thres, a.iou_thres = iou_thres;
    a.cand = frame.dev<DnmsCand>(), a.chunk_info = frame.dev<int>(cand_bytes), a.chunk_off = frame.dev<int>(cand_bytes + info_bytes);
    a.rows = rows_dev, a.index = index_dev, a.counts = counts_dev, a.status = status_dev;
    if (!h->hip_ok(launch_detector_nms(a, s), "detector NMS launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// COCO keypoint AP / AR of an evaluation set (keypoint_eval.hip); the arguments are judged first (keypoint_eval_math.h's
// keypoint_eval_fault, as in the host form: they need no device), then the handle.  The handle keeps the image table and the
// set-wide order of the slots; the table goes through the pinned ring.
int hrn_keypoint_eval_dev(hrn_handle h, int P, const int32_t *dt_start_host, const int32_t *gt_start_host, int J,
                          const double *dt_kpts_dev, const double *dt_scores_dev, const double *gt_kpts_dev, const double *gt_area_dev,
                          const double *gt_bbox_dev, const int32_t *gt_iscrowd_dev, const double *sigmas_dev, double *stats_dev,
                          double *precision_dev, double *recall_dev, int32_t *slot_person_dev, double *slot_score_dev,
                          int32_t *dt_match_dev, uint8_t *dt_ignore_dev, int32_t *npig_dev, int32_t *status_dev, void *stream) {
    if (!h) return 1;
    if (refused(h, "hrn_keypoint_eval_dev",
                keypoint_eval_fault(P, dt_start_host, gt_start_host, J, dt_kpts_dev, dt_scores_dev, gt_kpts_dev, gt_area_dev, gt_bbox_dev,
                                    gt_iscrowd_dev, sigmas_dev, stats_dev, precision_dev, recall_dev, slot_person_dev, slot_score_dev,
                                    dt_match_dev, dt_ignore_dev, npig_dev, status_dev)))
        return 7;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;
    int S = 0;
    for (int p = 0; p < P; ++p) S += std::min(dt_start_host[p + 1] - dt_start_host[p], kEvalMaxDet);
    const size_t table_bytes = ((size_t)P * sizeof(EvalImage) + 255) / 256 * 256, need = table_bytes + (size_t)S * sizeof(int);
    CallFrame frame(h, s, {{&h->eval_buf, need, hrn_ctx::twice(need, 4096), "hipMalloc(keypoint evaluation scratch)"}});
    KeypointEvalArgs a{};
    a.P = P, a.J = J, a.S = S;
    a.images = frame.table<EvalImage>((size_t)P, "hipMemcpyAsync(keypoint evaluation table)",
                                      [&](EvalImage *t) { keypoint_eval_images(P, dt_start_host, gt_start_host, t); });
    if (!frame.ok()) return 6;
    if (a.images) a.set_order = frame.dev<int>(table_bytes);
    a.dt_kpts = dt_kpts_dev, a.dt_scores = dt_scores_dev, a.gt_kpts = gt_kpts_dev, a.gt_area = gt_area_dev, a.gt_bbox = gt_bbox_dev;
    a.gt_iscrowd = gt_iscrowd_dev, a.sigmas = sigmas_dev;
    a.stats = stats_dev, a.precision = precision_dev, a.recall = recall_dev, a.slot_person = slot_person_dev, a.slot_score = slot_score_dev;
    a.dt_match = dt_match_dev, a.dt_ignore = dt_ignore_dev, a.npig = npig_dev, a.status = status_dev;
    if (!h->hip_ok(launch_keypoint_eval(a, s), "keypoint evaluation launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// ---- the detector link: the letterboxed detector tensor, and the detector's boxes back in frame coordinates --------------------
namespace {
// the one body of hrn_letterbox_frames and hrn_letterbox_frames_yuv: everything is judged -- the arguments, every frame, every
// geometry, then the handle -- before the device is touched
int letterbox_frames(const char *entry, hrn_handle h, const hrn_frame *frames, const hrn_yuv_frame *yframes, int n, int rule, int out_h,
                     int out_w, const uint8_t *pad, int order, int form, void *out_dev, hrn_letterbox *geometry_host, hipStream_t s) {
    const std::string name = entry;
    std::string why;
    if (rule != HRN_LETTERBOX_MAX_SIDE && rule != HRN_LETTERBOX_MIN_RATIO) why = letterbox_fault_text(LB_BAD_RULE);
    else if (order != HRN_LB_RGB && order != HRN_LB_BGR) why = "order must be HRN_LB_RGB or HRN_LB_BGR";
    else if (form != HRN_LB_F32 && form != HRN_LB_F16 && form != HRN_LB_BF16 && form != HRN_LB_U8_HWC)
        why = "form must be HRN_LB_F32, HRN_LB_F16, HRN_LB_BF16 or HRN_LB_U8_HWC";
    else if (out_h < 1 || out_w < 1 || out_h > 16384 || out_w > 16384) why = "out_h and out_w must be in [1, 16384]";
    else if (rule == HRN_LETTERBOX_MAX_SIDE && out_h != out_w) why = letterbox_fault_text(LB_NOT_SQUARE);
    else if (n < 0 || n > 65535) why = "n must be in [0, 65535]";
    else if (!pad || (n > 0 && (!(frames || yframes) || !out_dev))) why = "null frames / pad / output";
    std::vector<LetterboxFrame> recs((size_t)(why.empty() ? n : 0));
    for (int i = 0; why.empty() && i < n; ++i) {
        const char *fault = yframes ? yuv_frame_fault(yframes[i]) : bgr_frame_fault(frames[i]);
        if (fault) {
            why = name + ": frame " + std::to_string(i) + " " + fault;
            break;
        }
        LetterboxFrame &r = recs[i];
        r = LetterboxFrame{};
        r.src_h = yframes ? yframes[i].height : frames[i].height, r.src_w = yframes ? yframes[i].width : frames[i].width;
        hrn_letterbox g;
        const int code = letterbox_geometry_one(rule, r.src_h, r.src_w, out_h, out_w, &g, nullptr);
        if (code != LB_OK) {
            why = name + ": frame " + std::to_string(i) + " (" + std::to_string(r.src_h) + " x " + std::to_string(r.src_w) + ") " +
                  letterbox_fault_text(code);
            break;
        }
        if (yframes) r.yuv = yuv_source(yframes[i]);
        else r.bgr = frames[i].data;
        r.new_h = g.new_h, r.new_w = g.new_w, r.top = g.top, r.left = g.left;
        r.mode = g.new_h == r.src_h && g.new_w == r.src_w           ? LB_MODE_COPY
                 : r.src_h == 2 * g.new_h && r.src_w == 2 * g.new_w ? LB_MODE_AREA
                                                                    : LB_MODE_LINEAR;
        r.scale_x = resize_scale(g.new_w, r.src_w), r.scale_y = resize_scale(g.new_h, r.src_h);
        if (geometry_host) geometry_host[i] = g;
    }
    if (!why.empty()) {
        h->err = why.compare(0, name.size(), name) == 0 ? why : name + ": " + why;
        return 7;
    }
    if (h->refuse_plan_only()) return 7;
    if (n == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    const size_t table_bytes = n > 1 ? (size_t)n * sizeof(LetterboxFrame) : 0;
    CallFrame frame(h, s, {{&h->lb_table, table_bytes, hrn_ctx::twice(table_bytes, 4096), "hipMalloc(letterbox table)"}});
    LetterboxArgs a{};
    a.n = n, a.out_h = out_h, a.out_w = out_w, a.form = form, a.order = order, a.yuv = yframes ? 1 : 0;
    for (int i = 0; yframes && i < n; ++i)   // a call of NV12 / I420 frames alone keeps the two-way kernel
        if (yframes[i].format != HRN_PIX_NV12 && yframes[i].format != HRN_PIX_I420) a.yuv = 2;
    a.pad[0] = pad[0], a.pad[1] = pad[1], a.pad[2] = pad[2];
    a.out = out_dev;
    a.table = frame.table(recs.data(), (size_t)n, "hipMemcpyAsync(letterbox table)");
    if (!frame.ok()) return 6;
    if (!a.table) a.one = recs[0];
    if (!h->hip_ok(launch_letterbox(a, s), "letterbox launch")) return 8;
    return frame.leave() ? 0 : 6;
}
}  // namespace

int hrn_letterbox_frames(hrn_handle h, const hrn_frame *frames_host, int n, int rule, int out_h, int out_w, const uint8_t *pad, int order,
                         int form, void *out_dev, hrn_letterbox *geometry_host, void *stream) {
    if (!h) return 1;
    return letterbox_frames("hrn_letterbox_frames", h, frames_host, nullptr, n, rule, out_h, out_w, pad, order, form, out_dev, geometry_host,
                            (hipStream_t)stream);
}

int hrn_letterbox_frames_yuv(hrn_handle h, const hrn_yuv_frame *frames_host, int n, int rule, int out_h, int out_w, const uint8_t *pad,
                             int order, int form, void *out_dev, hrn_letterbox *geometry_host, void *stream) {
    if (!h) return 1;
    return letterbox_frames("hrn_letterbox_frames_yuv", h, nullptr, frames_host, n, rule, out_h, out_w, pad, order, form, out_dev,
                            geometry_host, (hipStream_t)stream);
}

// hrn_detections_to_frame on the device (letterbox.hip): the arguments are judged first (letterbox_math.h's det_fault, as in the
// host form: they need no device), then the handle.  Only a call with several frames touches the handle (its table).
int hrn_detections_to_frame_dev(hrn_handle h, int rule, const float *dets_dev, int det_stride, const int32_t *start_host, int P,
                                const hrn_letterbox *geometry_host, const int32_t *frame_hw_host, int out_h, int out_w, int conf_col,
                                float conf_thres, int class_col, const int32_t *classes_host, int nclasses, int flags,
                                float *dets_out_dev, int32_t *counts_dev, int32_t *status_dev, void *stream) {
    if (!h) return 1;
    DetFilter q{};
    const char *fault = det_fault(rule, dets_dev, det_stride, start_host, P, geometry_host, frame_hw_host, out_h, out_w, conf_col, conf_thres,
                                  class_col, classes_host, nclasses, flags, dets_out_dev, counts_dev, status_dev, q);
    if (refused(h, "hrn_detections_to_frame_dev", fault ? fault : P > 65535 ? "at most 65535 frames" : nullptr)) return 7;
    if (P == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;
    const size_t table_bytes = P > 1 ? (size_t)P * sizeof(DetFrame) : 0;
    CallFrame frame(h, s, {{&h->det_table, table_bytes, hrn_ctx::twice(table_bytes, 4096), "hipMalloc(detection table)"}});
    const auto record = [&](int p) {
        return det_frame(rule, geometry_host[p], frame_hw_host[2 * (size_t)p], frame_hw_host[2 * (size_t)p + 1], out_h, out_w, start_host[p],
                         start_host[p + 1] - start_host[p]);
    };
    DetArgs a{};
    a.P = P, a.compact = (flags & kDetCompact) ? 1 : 0;
    a.dets = dets_dev, a.out = dets_out_dev, a.counts = counts_dev, a.status = status_dev;
    a.table = frame.table<DetFrame>((size_t)P, "hipMemcpyAsync(detection table)", [&](DetFrame *t) {
        for (int p = 0; p < P; ++p) t[p] = record(p);
    });
    if (!frame.ok()) return 6;
    if (!h->hip_ok(launch_detections_to_frame(a, a.table ? DetFrame{} : record(0), q, s), "detections launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// ---- frame rotation: cv2.rotate for BGR, NV12 and I420 frames, and people between the two orientations (rotate.hip) -----------
namespace {
// the planes of a frame as (height, width) in elements, element size and the pitch / plane pointers of either side
struct RotPlaneShape {
    int h, w, es;
    bool chroma, second;   // which pitch, and I420's V
};
int rotate_plane_shapes(const hrn_canvas &c, RotPlaneShape out[3]) {
    if (c.format == HRN_PIX_BGR) {
        out[0] = {c.height, c.width, 3, false, false};
        return 1;
    }
    const int sample = pix_is_10bit(c.format) ? 2 : 1;   // bytes of a Y, U or V sample
    out[0] = {c.height, c.width, sample, false, false};
    if (!pix_is_planar(c.format)) {   // NV12 / NV21 / P010 (the caller has named the format): one plane of chroma pairs
        out[1] = {c.height / 2, c.width / 2, 2 * sample, true, false};
        return 2;
    }
    out[1] = {c.height / 2, c.width / 2, sample, true, false};
    out[2] = {c.height / 2, c.width / 2, sample, true, true};
    return 3;
}
// what is wrong with one side of a frame of hrn_rotate_frames, or nullptr
const char *rotate_frame_fault(const hrn_canvas &c) {
    if (c.format != HRN_PIX_BGR && !pix_is_yuv(c.format))
        return "has an unknown format (HRN_PIX_BGR, HRN_PIX_NV12, HRN_PIX_I420, HRN_PIX_NV21, HRN_PIX_P010 or HRN_PIX_I010)";
    if (!c.y || (c.format != HRN_PIX_BGR && !c.u) || (pix_is_planar(c.format) && !c.v)) return "has a null plane";
    if (c.height <= 0 || c.width <= 0) return "has a non-positive width or height";
    if (c.format != HRN_PIX_BGR && ((c.height & 1) || (c.width & 1))) return "has an odd width or height";
    RotPlaneShape shapes[3];
    const int np = rotate_plane_shapes(c, shapes);
    for (int k = 0; k < np; ++k) {
        const long pitch = shapes[k].chroma ? c.pitch_c : c.pitch_y;
        if (pitch < (long)shapes[k].w * shapes[k].es) return shapes[k].chroma ? "has pitch_c below its chroma row's bytes" : "has pitch_y below its row's bytes";
        if (pitch * shapes[k].h >= (1L << 31)) return "has a plane with pitch * rows >= 2^31";
    }
    if (pix_is_10bit(c.format) &&
        (((size_t)c.y | (size_t)c.u | (pix_is_planar(c.format) ? (size_t)c.v : 0) | (size_t)c.pitch_y | (size_t)c.pitch_c) & 1))
        return "has an odd plane address or pitch on a 10-bit frame";
    return nullptr;
}
}  // namespace

int hrn_rotate_frames(hrn_handle h, const hrn_canvas *src_host, const hrn_canvas *dst_host, int nframes, const int32_t *codes_host,
                      void *stream) {
    if (!h) return 1;
    const auto fail = [&](const std::string &what) {
        h->err = "hrn_rotate_frames: " + what;
        return 7;
    };
    if (nframes < 0) return fail("nframes is negative");
    if (nframes > 0 && (!src_host || !dst_host || !codes_host)) return fail("null frame tables / codes");
    std::vector<RotPlane> planes;
    long tiles = 0;
    std::map<const uint8_t *, int> written;   // first plane of a destination -> its frame
    for (int k = 0; k < nframes; ++k) {
        const hrn_canvas &s = src_host[k], &d = dst_host[k];
        const std::string frame = "frame " + std::to_string(k);
        const int code = codes_host[k];
        if (code != HRN_ROTATE_90_CW && code != HRN_ROTATE_180 && code != HRN_ROTATE_90_CCW)
            return fail(frame + ": code " + std::to_string(code) + " is outside {0, 1, 2}");
        if (s.format != d.format) return fail(frame + ": source and destination differ in format");
        if (const char *fault = rotate_frame_fault(s)) return fail(frame + ": the source " + fault);
        if (const char *fault = rotate_frame_fault(d)) return fail(frame + ": the destination " + fault);
        const bool turn = code != HRN_ROTATE_180;
        if (d.height != (turn ? s.width : s.height) || d.width != (turn ? s.height : s.width))
            return fail(frame + ": the destination is " + std::to_string(d.height) + " x " + std::to_string(d.width) + ", the rotated size is " +
                        std::to_string(turn ? s.width : s.height) + " x " + std::to_string(turn ? s.height : s.width));
        if (!written.emplace(d.y, k).second)
            return fail("frames " + std::to_string(written[d.y]) + " and " + std::to_string(k) + " name the same destination");
        RotPlaneShape shapes[3];
        const int np = rotate_plane_shapes(s, shapes);
        for (int q = 0; q < np; ++q) {
            RotPlane p{};
            p.src = q == 0 ? s.y : shapes[q].second ? s.v : s.u, p.dst = q == 0 ? d.y : shapes[q].second ? d.v : d.u;
            p.hs = shapes[q].h, p.ws = shapes[q].w, p.es = shapes[q].es, p.code = code;
            p.spitch = shapes[q].chroma ? s.pitch_c : s.pitch_y, p.dpitch = shapes[q].chroma ? d.pitch_c : d.pitch_y;
            const int dst_w = turn ? p.hs : p.ws, dst_h = turn ? p.ws : p.hs;
            p.tile_start = (int)tiles, p.tiles_x = (dst_w + kRotTile - 1) / kRotTile;
            const int tile_rows = turn ? kRotTile : kRotRows180;
            tiles += (long)p.tiles_x * ((dst_h + tile_rows - 1) / tile_rows);
            if (tiles > 0x7fffffffL) return fail("the call has more than 2^31 - 1 tiles");
            planes.push_back(p);
        }
    }
    for (int k = 0; k < nframes; ++k) {   // in-place rotation is not offered: no source is a destination of the call
        const auto hit = written.find(src_host[k].y);
        if (hit != written.end())
            return fail("the source of frame " + std::to_string(k) + " is the destination of frame " + std::to_string(hit->second) +
                        ": in-place rotation is not offered");
    }
    if (h->refuse_plan_only()) return 7;
    if (nframes == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;
    const size_t table_bytes = nframes > 1 ? planes.size() * sizeof(RotPlane) : 0;
    CallFrame frame(h, s, {{&h->rot_table, table_bytes, hrn_ctx::twice(table_bytes, 4096), "hipMalloc(rotation table)"}});
    RotArgs a{};
    a.nplanes = (int)planes.size(), a.total_tiles = (int)tiles;
    a.table = frame.table(planes.data(), planes.size(), "hipMemcpyAsync(rotation table)");
    if (!frame.ok()) return 6;
    if (!a.table) std::copy(planes.begin(), planes.end(), a.one);
    if (!h->hip_ok(launch_rotate(a, s), "rotate launch")) return 8;
    return frame.leave() ? 0 : 6;
}

int hrn_rotate_people_dev(hrn_handle h, int n, int J, const int32_t *frame_hw_host, int per_person_hw, const int32_t *codes_host,
                          int per_person_code, const float *pts_dev, const int32_t *boxes_dev, float *pts_out_dev, int32_t *boxes_out_dev,
                          void *stream) {
    if (!h) return 1;
    if (refused(h, "hrn_rotate_people_dev", rotate_people_fault(n, J, frame_hw_host, per_person_hw, codes_host, per_person_code, pts_dev,
                                                                boxes_dev, pts_out_dev, boxes_out_dev)))
        return 7;
    if (n == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;
    const size_t hw_bytes = per_person_hw ? (size_t)n * 2 * sizeof(int32_t) : 0, code_bytes = per_person_code ? (size_t)n * sizeof(int32_t) : 0;
    const size_t need = hw_bytes + code_bytes;   // what the call has per person: a table through the pinned ring
    CallFrame frame(h, s, {{&h->rot_people, need, hrn_ctx::twice(need, 4096), "hipMalloc(rotated people table)"}});
    RotPeopleArgs a{};
    a.n = n, a.J = J, a.hs = frame_hw_host[0], a.ws = frame_hw_host[1], a.code = codes_host[0];
    a.pts = pts_dev, a.boxes = (const int *)boxes_dev, a.pts_out = pts_out_dev, a.boxes_out = (int *)boxes_out_dev;
    const char *dev = frame.table<char>(need, "hipMemcpyAsync(rotated people table)", [&](char *pin) {
        if (hw_bytes) memcpy(pin, frame_hw_host, hw_bytes);
        if (code_bytes) memcpy(pin + hw_bytes, codes_host, code_bytes);
    });
    if (!frame.ok()) return 6;
    if (hw_bytes) a.frame_hw = (const int *)dev;
    if (code_bytes) a.codes = (const int *)(dev + hw_bytes);
    if (!h->hip_ok(launch_rotate_people(a, s), "rotate people launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// ---- BGR frames back to 4:2:0 YCbCr frames (yuv_out.hip; the arithmetic: yuv_fwd.h, one text for these entries and the kernel) ----
int hrn_yuv_forward_coefficients(int matrix, int range, int32_t out[10]) {
    if (!out) return 7;
    return yuv_forward_table(matrix, range, out) ? 0 : 7;
}

int hrn_bgr_to_yuv_blocks(int matrix, int range, int depth, const uint8_t *bgr, int n, uint16_t *out) {
    int32_t c[kYuvFwdCoefs];
    if (!yuv_forward_table(matrix, range, c) || (depth != 8 && depth != 10)) return 7;
    if (n < 0 || (n > 0 && (!bgr || !out))) return 7;
    for (int i = 0; i < n; ++i) yuv_fwd_block(c, depth == 10, bgr + (size_t)i * 12, out + (size_t)i * 6);
    return 0;
}

// One launch for all frames, as hrn_rotate_frames: both sides of every frame are judged by its plane checks (rotate_frame_fault),
// the destination's matrix and range choose its table, the records go into the kernel arguments (one frame) or through the
// handle's guarded table and the pinned ring (more).
int hrn_bgr_to_yuv_frames(hrn_handle h, const hrn_canvas *src_host, const hrn_canvas *dst_host, int nframes, void *stream) {
    if (!h) return 1;
    const auto fail = [&](const std::string &what) {
        h->err = "hrn_bgr_to_yuv_frames: " + what;
        return 7;
    };
    if (nframes < 0) return fail("nframes is negative");
    if (nframes > 0 && (!src_host || !dst_host)) return fail("null frame tables");
    std::vector<YuvOutFrame> frames;
    long tiles = 0;
    std::map<const uint8_t *, int> written;   // first plane of a destination -> its frame
    for (int k = 0; k < nframes; ++k) {
        const hrn_canvas &s = src_host[k], &d = dst_host[k];
        const std::string frame = "frame " + std::to_string(k);
        if (s.format != HRN_PIX_BGR) return fail(frame + ": the source is not an HRN_PIX_BGR frame");
        if (!pix_is_yuv(d.format))
            return fail(frame + ": the destination has an unknown format (HRN_PIX_NV12, HRN_PIX_I420, HRN_PIX_NV21, HRN_PIX_P010 or HRN_PIX_I010)");
        YuvOutFrame f{};
        if (d.matrix != HRN_YUV_BT601 && d.matrix != HRN_YUV_BT709)
            return fail(frame + ": the destination has an unknown matrix (HRN_YUV_BT601 or HRN_YUV_BT709)");
        if (!yuv_forward_table(d.matrix, d.range, f.coef))
            return fail(frame + ": the destination has an unknown range (HRN_YUV_LIMITED or HRN_YUV_FULL)");
        if (const char *fault = rotate_frame_fault(s)) return fail(frame + ": the source " + fault);
        if ((s.height & 1) || (s.width & 1)) return fail(frame + ": the source has an odd width or height");
        if (s.height > 8192 || s.width > 8192) return fail(frame + ": the source has a side above 8192");
        if (const char *fault = rotate_frame_fault(d)) return fail(frame + ": the destination " + fault);
        if (d.height != s.height || d.width != s.width)
            return fail(frame + ": the destination is " + std::to_string(d.height) + " x " + std::to_string(d.width) + ", the source is " +
                        std::to_string(s.height) + " x " + std::to_string(s.width));
        if (!written.emplace(d.y, k).second)
            return fail("frames " + std::to_string(written[d.y]) + " and " + std::to_string(k) + " name the same destination");
        f.src = s.y, f.y = d.y, f.u = d.u, f.v = pix_is_planar(d.format) ? d.v : nullptr;
        f.height = s.height, f.width = s.width, f.spitch = s.pitch_y, f.pitch_y = d.pitch_y, f.pitch_c = d.pitch_c, f.format = d.format;
        f.tile_start = (int)tiles, f.tiles_x = (f.width + kYuvOutTileW - 1) / kYuvOutTileW;
        tiles += (long)f.tiles_x * ((f.height + kYuvOutTileH - 1) / kYuvOutTileH);   // (at most 32 x 1024 per frame)
        if (tiles > 0x7fffffffL) return fail("the call has more than 2^31 - 1 tiles");
        frames.push_back(f);
    }
    for (int k = 0; k < nframes; ++k) {   // a BGR buffer cannot hold its own YUV form: no source is a destination of the call
        const auto hit = written.find(src_host[k].y);
        if (hit != written.end())
            return fail("the source of frame " + std::to_string(k) + " is the destination of frame " + std::to_string(hit->second) +
                        ": in-place conversion is not offered");
    }
    if (h->refuse_plan_only()) return 7;
    if (nframes == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;
    const size_t table_bytes = nframes > 1 ? frames.size() * sizeof(YuvOutFrame) : 0;
    CallFrame frame(h, s, {{&h->yuvout_table, table_bytes, hrn_ctx::twice(table_bytes, 4096), "hipMalloc(BGR to YUV table)"}});
    YuvOutArgs a{};
    a.nframes = nframes, a.total_tiles = (int)tiles;
    a.table = frame.table(frames.data(), frames.size(), "hipMemcpyAsync(BGR to YUV table)");
    if (!frame.ok()) return 6;
    if (!a.table) a.one = frames[0];
    if (!h->hip_ok(launch_bgr_to_yuv(a, s), "bgr_to_yuv launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// the One-Euro filter and the motion lookahead of every joint of the call in one launch (temporal.hip); the arguments are judged
// first (temporal_math.h's temporal_fault, as in the host form: they need no device), then the handle.  Only a call with several
// problems touches the handle (the per-person segment table), so only that call enters a guard.
int hrn_filter_poses_dev(hrn_handle h, int P, const int32_t *cur_start_host, const int32_t *prev_start_host, int J, const float *pts_dev,
                         const int32_t *match_dev, const float *prev_state_dev, const int32_t *prev_age_dev, double dt, double min_cutoff,
                         double beta, double d_cutoff, float threshold, double lookahead, float *pts_out_dev, float *pred_out_dev,
                         float *state_dev, int32_t *age_dev, void *stream) {
    if (!h) return 1;
    if (refused(h, "hrn_filter_poses_dev", temporal_fault(P, cur_start_host, prev_start_host, J, pts_dev, match_dev, prev_state_dev, prev_age_dev,
                                                          dt, min_cutoff, beta, d_cutoff, lookahead, pts_out_dev, state_dev, age_dev)))
        return 7;
    const int n = P > 0 ? cur_start_host[P] - cur_start_host[0] : 0;
    if (n == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;
    const size_t table_bytes = P > 1 ? (size_t)n * sizeof(TemporalSegment) : 0;
    CallFrame frame(h, s, {{&h->tmp_table, table_bytes, hrn_ctx::twice(table_bytes, 4096), "hipMalloc(filter segment table)"}});
    TemporalArgs a{};
    a.J = J, a.first = cur_start_host[0], a.total = n * J;   // (n * J <= 2^31 - 1: temporal_fault)
    a.one.prev0 = prev_start_host[0], a.one.m = prev_start_host[1] - prev_start_host[0];
    a.table = frame.table<TemporalSegment>((size_t)n, "hipMemcpyAsync(filter segment table)", [&](TemporalSegment *t) {   // everybody's
        for (int p = 0; p < P; ++p)
            for (int i = cur_start_host[p]; i < cur_start_host[p + 1]; ++i)
                t[i - a.first] = TemporalSegment{prev_start_host[p], prev_start_host[p + 1] - prev_start_host[p]};
    });
    if (!frame.ok()) return 6;
    a.pts = pts_dev, a.match = (const int *)match_dev, a.prev_state = prev_state_dev, a.prev_age = (const int *)prev_age_dev;
    a.pts_out = pts_out_dev, a.pred_out = pred_out_dev, a.state = state_dev, a.age = (int *)age_dev;
    if (!h->hip_ok(launch_temporal(a, temporal_params(dt, min_cutoff, beta, d_cutoff, threshold, lookahead), s), "filter launch")) return 8;
    return frame.leave() ? 0 : 6;
}

int hrn_resize_frames(hrn_handle h, const uint8_t *frames_dev, int n, int frame_h, int frame_w, int interpolation,
                      float *images_dev, void *stream) {
    if (!h) return 1;
    if (h->refuse_plan_only()) return 7;
    if (interpolation != HRN_INTER_NEAREST && interpolation != HRN_INTER_LINEAR && interpolation != HRN_INTER_CUBIC) {
        h->err = "interpolation must be HRN_INTER_NEAREST (0), HRN_INTER_LINEAR (1) or HRN_INTER_CUBIC (2)";
        return 7;
    }
    if (n < 0 || frame_h <= 0 || frame_w <= 0 || (n > 0 && (!frames_dev || !images_dev))) {
        h->err = "bad frames / n";
        return 7;
    }
    if (n == 0) return 0;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hipStream_t s = (hipStream_t)stream;
    const int H = h->H, W = h->W;
    const size_t taps_bytes = (size_t)(W + H) * sizeof(ResizeTaps);   // the one tap table of the handle, rewritten by every call
    CallFrame frame(h, s, {{&h->rs_taps, taps_bytes, taps_bytes, "hipMalloc(resize taps)"}});
    if (!frame.ok()) return 6;
    if (!h->hip_ok(launch_resize_frames(frames_dev, n, frame_h, frame_w, interpolation, frame.dev<ResizeTaps>(), images_dev, H, W, s),
                   "resize launch"))
        return 8;
    return frame.leave() ? 0 : 6;
}

namespace {
// The inversion cv::warpAffine performs on a forward matrix (no WARP_INVERSE_MAP), statement for statement, each product and
// sum rounded on its own.  False when the matrix is not finite, singular, or its inverse is not finite.
bool invert_affine(const double *fwd, double *M) {
#pragma clang fp contract(off)
    for (int k = 0; k < 6; ++k) {
        if (!std::isfinite(fwd[k])) return false;
        M[k] = fwd[k];
    }
    double D = M[0] * M[4] - M[1] * M[3];
    if (D == 0) return false;   // (the reference would go on with D = 0 and sample one pixel everywhere)
    D = 1. / D;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11, M[1] *= -D;
    M[3] *= -D, M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5];
    const double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1, M[5] = b2;
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(M[k])) return false;
    return true;
}
}  // namespace

// datasets/COCO.py:290-304 / misc/utils.py:99-107.  Everything that can be refused is refused before anything is queued.
int hrn_warp_crops(hrn_handle h, const uint8_t *frames_dev, int nframes, int frame_h, int frame_w, const int32_t *frame_index_host,
                   const double *matrices_host, int n, float *images_dev, void *stream) {
    if (!h) return 1;
    if (h->refuse_plan_only()) return 7;
    if (n < 0 || nframes < 0 || frame_h <= 0 || frame_w <= 0 || (n > 0 && (nframes < 1 || !frames_dev || !matrices_host || !images_dev))) {
        h->err = "bad frames / matrices / n";
        return 7;
    }
    if (frame_h > 32766 || frame_w > 32766) {   // OpenCV saturates source coordinates to int16
        h->err = "hrn_warp_crops: a frame side above 32766 is not supported";
        return 7;
    }
    if (n == 0) return 0;
    if (!frame_index_host && nframes != n && nframes != 1) {
        h->err = "hrn_warp_crops: without frame_index there must be one frame per crop, or one frame";
        return 7;
    }
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    const int H = h->H, W = h->W;
    const size_t bytes = (size_t)n * sizeof(WarpParams);
    const PinnedImage img = h->image(bytes);
    if (!img) return 6;
    WarpParams *wp = img.as<WarpParams>();
    for (int i = 0; i < n; ++i) {
        const long f = frame_index_host ? (long)frame_index_host[i] : nframes == 1 ? 0 : i;
        if (f < 0 || f >= nframes) {
            h->err = "hrn_warp_crops: frame_index " + std::to_string(f) + " of crop " + std::to_string(i) + " is outside [0, " +
                     std::to_string(nframes) + ")";
            return 7;
        }
        WarpParams &p = wp[i];
        p.frame = (int)f, p.pad_ = 0;
        if (!invert_affine(matrices_host + (size_t)i * 6, p.m)) {
            h->err = "hrn_warp_crops: matrix " + std::to_string(i) + " is not finite or singular";
            return 7;
        }
        // the fixed point is 10 fractional bits in int32 in OpenCV: keep every source coordinate of the crop (an affine map
        // takes its extremes at the corners) within 2^20
        const double lim = 1048576.0;
        for (int c = 0; c < 4; ++c) {
            const double x = (c & 1) ? W - 1 : 0, y = (c & 2) ? H - 1 : 0;
            const double sx = p.m[0] * x + p.m[1] * y + p.m[2], sy = p.m[3] * x + p.m[4] * y + p.m[5];
            if (!(std::fabs(sx) <= lim) || !(std::fabs(sy) <= lim)) {
                h->err = "hrn_warp_crops: matrix " + std::to_string(i) + " maps the crop beyond 2^20 pixels from the frame's origin";
                return 7;
            }
        }
    }
    hipStream_t s = (hipStream_t)stream;
    CallFrame frame(h, s, {{&h->warp_params, bytes, std::max(n, 256) * sizeof(WarpParams), "hipMalloc(warp params)"}});
    const WarpParams *params = frame.upload<WarpParams>(img, bytes, "hipMemcpyAsync(warp params)");
    if (!params) return 6;
    if (!h->hip_ok(launch_warp_crops(frames_dev, frame_h, frame_w, params, n, images_dev, H, W, s), "warp launch")) return 8;
    return frame.leave() ? 0 : 6;
}

extern "C++" {
namespace {
// datasets/COCO.py:466-488, 512-513 for n persons: mu = int(joint / feat_stride + 0.5) (float64, truncated towards zero; the
// stride is image_size / heatmap_size = 4), ul = mu - t, br = mu + t + 1, weight = visibility, 0 when ul >= size or br < 0 on
// either axis (`br < 0`, not `<= 0`: a window that ends exactly at the map's edge keeps its weight and draws nothing).
// Any of the outputs may be NULL.  Returns "" or what is wrong with the arguments; nothing is written then.
std::string target_centers(const double *joints, const float *vis, const float *joints_weight, int n, int J, int height, int width,
                           double sigma, int32_t *mu_out, float *draw_out, float *target_weight_out, ScoreJoint *recs) {
    if (n < 0 || J <= 0 || (n > 0 && (!joints || !vis))) return "bad joints / visibility / n";
    if (height <= 0 || width <= 0 || height % 32 || width % 32) return "resolution must be a positive multiple of 32 in both dimensions";
    const double t_real = 3.0 * sigma;
    if (!(sigma > 0) || !std::isfinite(sigma) || t_real != std::floor(t_real) || t_real > 1024)
        return "sigma must be positive with 3 * sigma an integer (at most 1024)";
    const long long t = (long long)t_real, h = height / 4, w = width / 4;
    const double stride_x = (double)width / (double)w, stride_y = (double)height / (double)h;
    for (size_t k = 0; k < (size_t)n * J; ++k) {   // everything is checked before anything is written
        const double fx = joints[2 * k] / stride_x + 0.5, fy = joints[2 * k + 1] / stride_y + 0.5;
        if (!std::isfinite(joints[2 * k]) || !std::isfinite(joints[2 * k + 1]) || !(std::fabs(fx) < 2147483648.0) ||
            !(std::fabs(fy) < 2147483648.0))
            return "joint " + std::to_string(k % J) + " of person " + std::to_string(k / J) + " is not finite or does not fit an int32 in heat-map cells";
    }
    for (size_t k = 0; k < (size_t)n * J; ++k) {
        const long long mx = (long long)(joints[2 * k] / stride_x + 0.5), my = (long long)(joints[2 * k + 1] / stride_y + 0.5);
        const bool off = mx - t >= w || my - t >= h || mx + t + 1 < 0 || my + t + 1 < 0;
        const float v = off ? 0.f : vis[k];
        const bool draw = v > 0.5f && mx + t + 1 > 0 && my + t + 1 > 0;   // (the window meets the map)
        const float tw = joints_weight ? v * joints_weight[k % J] : v;
        if (mu_out) mu_out[2 * k] = (int32_t)mx, mu_out[2 * k + 1] = (int32_t)my;
        if (draw_out) draw_out[k] = v;
        if (target_weight_out) target_weight_out[k] = tw;
        if (recs) recs[k] = ScoreJoint{draw ? (int)mx : 0, draw ? (int)my : 0, tw, draw ? 1 : 0};
    }
    return "";
}

// what hrn_generate_targets and hrn_score_heatmaps share: the image their n * J records are written into, and the frame on
// score_joints that carries them to the device
PinnedImage score_image(hrn_ctx *h, int64_t count) { return h->image((size_t)std::max<int64_t>(count, 1) * sizeof(ScoreJoint)); }
struct ScoreFrame : CallFrame {
    const ScoreJoint *joints;   // on the device (nullptr and not ok(): the entry returns 6)
    ScoreFrame(hrn_ctx *h, const PinnedImage &img, int64_t count, hipStream_t s)
        : CallFrame(h, s, {{&h->score_joints, (size_t)count * sizeof(ScoreJoint), (size_t)std::max<int64_t>(count, 256 * 17) * sizeof(ScoreJoint),
                            "hipMalloc(score records)"}}),
          joints(upload<ScoreJoint>(img, (size_t)count * sizeof(ScoreJoint), "hipMemcpyAsync(score records)")) {}
};
}  // namespace
}  // extern "C++"

int hrn_target_centers(const double *joints, const float *vis, const float *joints_weight, int n, int J, int height, int width,
                       double sigma, int32_t *mu_out, float *draw_out, float *target_weight_out) {
    g_create_error = target_centers(joints, vis, joints_weight, n, J, height, width, sigma, mu_out, draw_out, target_weight_out, nullptr);
    if (!g_create_error.empty()) g_create_error = "hrn_target_centers: " + g_create_error;
    return g_create_error.empty() ? 0 : 7;
}

// datasets/COCO.py:460-515 for a batch.  Everything that can be refused is refused before anything is queued.
int hrn_generate_targets(hrn_handle h, const double *joints_host, const float *vis_host, const float *joints_weight_host, int n,
                         double sigma, float *targets_dev, float *target_weight_host, void *stream) {
    if (!h) return 1;
    if (h->refuse_plan_only()) return 7;
    if (n < 0 || (n > 0 && !targets_dev) || ((uintptr_t)targets_dev & 15)) {
        h->err = "hrn_generate_targets: bad targets / n (targets must be 16-byte aligned)";
        return 7;
    }
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    const int64_t count = (int64_t)n * h->joints;
    const PinnedImage img = score_image(h, count);
    if (!img) return 6;
    const std::string bad = target_centers(joints_host, vis_host, joints_weight_host, n, h->joints, h->H, h->W, sigma, nullptr, nullptr,
                                           target_weight_host, img.as<ScoreJoint>());
    if (!bad.empty()) {
        h->err = "hrn_generate_targets: " + bad;
        return 7;
    }
    if (n == 0) return 0;
    ScoreArgs a{};
    a.t = (int)(3.0 * sigma);
    a.table = h->score_table(a.t, sigma);
    if (!a.table) return 6;
    hipStream_t s = (hipStream_t)stream;
    ScoreFrame frame(h, img, count, s);
    if (!frame.ok()) return 6;
    a.joints = frame.joints, a.n = n, a.J = h->joints, a.h = h->H / 4, a.w = h->W / 4;
    if (!h->hip_ok(launch_targets(a, targets_dev, s), "targets launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// testing/Test.py:141-157: loss_fn(output, target, target_weight) and evaluate_pck_accuracy(output, target) of one batch.
int hrn_score_heatmaps(hrn_handle h, const float *heatmaps_dev, int n, const float *targets_dev, const double *joints_host,
                       const float *vis_host, const float *joints_weight_host, double sigma, const float *target_weight_host,
                       float pck_thr, int ohkm_topk, const hrn_score_out *out_dev, void *stream) {
    if (!h) return 1;
    if (h->refuse_plan_only()) return 7;
    if (n < 0 || (n > 0 && !heatmaps_dev)) {
        h->err = "hrn_score_heatmaps: bad heatmaps / n";
        return 7;
    }
    if (((uintptr_t)heatmaps_dev | (uintptr_t)targets_dev) & 15) {
        h->err = "hrn_score_heatmaps: heatmaps / targets must be 16-byte aligned (the maps are read with 16-byte loads)";
        return 7;
    }
    const bool maps = targets_dev != nullptr, analytic = joints_host != nullptr;
    if (maps == analytic) {
        h->err = "hrn_score_heatmaps: give either targets (with target_weight) or joints (with visibility), not both and not neither";
        return 7;
    }
    if (maps ? (!target_weight_host || vis_host || joints_weight_host) : (!vis_host || target_weight_host != nullptr)) {
        h->err = maps ? "hrn_score_heatmaps: target maps come with target_weight and without visibility / joints_weight"
                      : "hrn_score_heatmaps: joints come with visibility and without target_weight";
        return 7;
    }
    if (!std::isfinite(pck_thr)) {
        h->err = "hrn_score_heatmaps: pck_thr is not finite";
        return 7;
    }
    if (ohkm_topk > h->joints) {
        h->err = "hrn_score_heatmaps: ohkm_topk " + std::to_string(ohkm_topk) + " exceeds the " + std::to_string(h->joints) + " joints";
        return 7;
    }
    if (!out_dev || !out_dev->loss_mse || !out_dev->loss_ohkm || !out_dev->avg_acc || !out_dev->cnt || !out_dev->acc ||
        (n > 0 && (!out_dev->dists || !out_dev->map_loss || !out_dev->preds || !out_dev->target_preds || !out_dev->maxvals))) {
        h->err = "hrn_score_heatmaps: every field of hrn_score_out must point to device memory (the per-person ones unless n is 0)";
        return 7;
    }
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    const int64_t count = (int64_t)n * h->joints;
    const PinnedImage img = score_image(h, count);
    if (!img) return 6;
    ScoreJoint *recs = img.as<ScoreJoint>();
    ScoreArgs a{};
    if (analytic) {
        const std::string bad = target_centers(joints_host, vis_host, joints_weight_host, n, h->joints, h->H, h->W, sigma, nullptr, nullptr,
                                               nullptr, recs);
        if (!bad.empty()) {
            h->err = "hrn_score_heatmaps: " + bad;
            return 7;
        }
        a.t = (int)(3.0 * sigma);
        a.table = h->score_table(a.t, sigma);
        if (!a.table) return 6;
    } else {
        for (int64_t k = 0; k < count; ++k) recs[k] = ScoreJoint{0, 0, target_weight_host[k], 0};
    }
    hipStream_t s = (hipStream_t)stream;
    ScoreFrame frame(h, img, count, s);
    if (!frame.ok()) return 6;
    a.heatmaps = heatmaps_dev, a.targets = targets_dev, a.joints = frame.joints;
    a.n = n, a.J = h->joints, a.h = h->H / 4, a.w = h->W / 4;
    a.map_loss = out_dev->map_loss, a.preds = out_dev->preds, a.target_preds = out_dev->target_preds, a.maxvals = out_dev->maxvals;
    a.loss_mse = out_dev->loss_mse, a.loss_ohkm = out_dev->loss_ohkm, a.avg_acc = out_dev->avg_acc, a.acc = out_dev->acc;
    a.dists = out_dev->dists, a.cnt = out_dev->cnt, a.pck_thr = pck_thr, a.ohkm_topk = ohkm_topk;
    if (!h->hip_ok(launch_score(a, s), "score launch")) return 8;
    return frame.leave() ? 0 : 6;
}

// Debug tap: one micro-batch with the named tensor copied out right after the launch that completes it.
int hrn_tap_count(hrn_handle h) { return h ? (int)h->taps.size() : 0; }

int hrn_get_tap_info(hrn_handle h, int index, hrn_tap_info *out) {
    if (!h || !out || index < 0 || index >= (int)h->taps.size()) return 1;
    const TapPoint &tp = h->taps[index];
    const Tensor &t = h->tensors[tp.tensor];
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", tp.name.c_str());
    out->c = t.c, out->h = t.h, out->w = t.w, out->conv_index = tp.conv;
    return 0;
}

int hrn_forward_tap(hrn_handle h, const void *images_dev, int n, const char *tap_name, int crop0, int ncrops, int crop_step,
                    float *dst_dev, float *heatmaps_dev, void *stream) {
    if (!h) return 1;
    if (!h->check_forward_args(images_dev, n, nullptr, nullptr, nullptr, /*outputs_optional=*/true)) return 7;
    if (!tap_name || !dst_dev || n < 1 || n > h->max_batch || crop0 < 0 || ncrops < 1 || crop_step < 1 ||
        (int64_t)crop0 + (int64_t)(ncrops - 1) * crop_step >= n) {
        h->err = "hrn_forward_tap: needs a tap name, a destination, 1 <= n <= max_batch and crops crop0, crop0 + step, ... inside the call";
        return 7;
    }
    const TapPoint *tp = nullptr;
    for (const TapPoint &t : h->taps)
        if (t.name == tap_name) tp = &t;
    if (!tp) {
        h->err = std::string("hrn_forward_tap: no tensor named '") + tap_name + "' is written by this plan";
        return 7;
    }
    if (tp->conv >= 0 && h->fused_now(h->convs[tp->conv], n)) {
        h->err = std::string("hrn_forward_tap: '") + tap_name + "' stays in LDS at this batch size (fused BasicBlock pass); tap the block's conv2";
        return 7;
    }
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    const TapReq req{tp->op, tp->tensor, crop0, ncrops, crop_step, dst_dev};
    CallScope scope(h, &h->pass, (hipStream_t)stream);
    if (!scope.entered) return 6;
    if (!h->run_pass((const float *)images_dev, n, nullptr, 0, nullptr, heatmaps_dev, (hipStream_t)stream, nullptr, 0, &req)) return 8;
    return scope.leave() ? 0 : 6;
}

int hrn_conv_count(hrn_handle h) { return h ? (int)h->convs.size() : 0; }

int hrn_get_conv_info(hrn_handle h, int index, hrn_conv_info *out) {
    if (!h || !out || index < 0 || index >= (int)h->convs.size()) return 1;
    const ConvOp &cv = h->convs[index];
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", cv.conv.c_str());
    out->cin = cv.cin, out->cout = cv.cout, out->ksize = cv.k, out->stride = cv.stride, out->relu = cv.relu;
    out->has_residual = cv.res_t >= 0;
    out->in_h = h->tensors[cv.in_t].h, out->in_w = h->tensors[cv.in_t].w;
    out->out_h = h->tensors[cv.out_t].h, out->out_w = h->tensors[cv.out_t].w;
    out->kpad = cv.kpad, out->nr = cv.nr, out->algo = cv.fuse_with >= 0 || cv.fused_away ? 2 : cv.n96 ? 3 : cv.s2 ? 4 : cv.algo, out->ks = cv.ks;
    out->w_offset = cv.w_off, out->w_bytes = cv.w_bytes, out->b_offset = cv.b_off;
    out->flops = cv.flops;
    return 0;
}

double hrn_flops_per_crop(hrn_handle h) {
    if (!h) return 0;
    double f = 2.0 * 64 * (h->model == 1 ? 147 : 27) * (h->H / 2) * (double)(h->W / 2);   // conv1
    for (auto &cv : h->convs) f += cv.flops;
    f += 2.0 * h->joints * h->head_c * (h->H / 4) * (double)(h->W / 4);      // final_layer
    return f;
}

int64_t hrn_workspace_bytes(hrn_handle h) { return h ? h->workspace_bytes : 0; }
int64_t hrn_map_rebuilds(hrn_handle h) { return h ? h->map_builds : -1; }
int hrn_launches_per_pass(hrn_handle h) { return h ? (int)h->ops.size() - (h->stem_fuse ? 1 : 0) : 0; }
int hrn_stem_fused(hrn_handle h) { return h && h->stem_fuse ? 1 : 0; }
int hrn_conv_compact(hrn_handle h, int index) { return h && index >= 0 && index < (int)h->convs.size() && h->convs[index].compact ? 1 : 0; }
const char *hrn_switches(hrn_handle h) { return h ? h->switches.c_str() : ""; }

int64_t hrn_debug_pad_violations(hrn_handle h) {
    if (!h || h->plan_only) return -1;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return -1;
    unsigned long long *cnt = nullptr, host = 0;
    if (!h->hip_ok(hipMalloc((void **)&cnt, sizeof *cnt), "hipMalloc") || !h->hip_ok(hipMemset(cnt, 0, sizeof *cnt), "hipMemset")) return -1;
    bool ok = h->hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    for (const Buffer &b : h->buffers) {
        if (!ok) break;
        PadCheckArgs a;
        a.buf = b.dev, a.count = cnt, a.rows = (long)b.rows, a.lead_rows = (long)b.lead_rows;
        a.c = b.c, a.h = b.h, a.w = b.w, a.wp = b.w + 1, a.hpwp = (b.h + 1) * (b.w + 1), a.nmax = h->max_batch;
        ok = h->hip_ok(launch_pad_check(h->dtype, a, nullptr), "pad check launch");
    }
    ok = ok && h->hip_ok(hipMemcpy(&host, cnt, sizeof host, hipMemcpyDeviceToHost), "hipMemcpy");
    (void)hipFree(cnt);
    return ok ? (int64_t)host : -1;
}

int hrn_plan_block_map(hrn_handle h, int group, int n, int reverse, int32_t *blocks, int capacity, int32_t *members, int member_capacity) {
    if (!h || n <= 0 || n > h->max_batch) return -1;
    if (group < 0 || group >= (int)h->groups.size()) return -1;
    const Conv3Group &g = h->groups[group];
    std::vector<int2> map;
    std::vector<int> px;
    const int nblocks = h->group_blocks(g, n, &map, reverse != 0, false, &px);
    for (int i = 0; i < nblocks && i < capacity; ++i) {
        const int x = map[i].x, y = map[i].y;
        int32_t *o = blocks + (size_t)i * 6;
        o[0] = x & 0xff, o[1] = (x >> 8) & 0xff, o[2] = x >> 16, o[3] = y & 0x1fffffff, o[4] = px[i],
        o[5] = ((y >> 29) & 1) | (((y >> 30) & 1) << 1);
    }
    int nm = 0;  // descriptor -> convolution: the plain ones first, then the fused forms (conv1's index + 2^30)
    for (size_t k = 0; k < g.conv_idx.size(); ++k, ++nm)
        if (nm < member_capacity) members[nm] = g.conv_idx[k];
    for (size_t k = 0; k < g.conv_idx.size(); ++k)
        if (g.fused_prob[k] >= 0) {
            if (g.fused_prob[k] < member_capacity) members[g.fused_prob[k]] = g.conv_idx[k] | (1 << 30);
            ++nm;
        }
    return nblocks;
}

int hrn_plan_direct_map(hrn_handle h, int group, int n, int32_t *blocks, int capacity, int32_t *members, int member_capacity,
                        int32_t *pixels_per_tile) {
    if (!h || n <= 0 || n > h->max_batch) return -1;
    if (group < 0 || group >= (int)h->dgroups.size()) return -1;
    const DirectGroup &g = h->dgroups[group];
    const int mr = h->direct_mr(g, n);
    std::vector<int2> map;
    const int nblocks = h->direct_group_blocks(g, n, &map, mr);
    for (int i = 0; i < nblocks && i < capacity; ++i)
        blocks[(size_t)i * 3] = map[i].x & 0xff, blocks[(size_t)i * 3 + 1] = map[i].x >> 8, blocks[(size_t)i * 3 + 2] = map[i].y;
    for (size_t k = 0; k < g.conv_idx.size() && (int)k < member_capacity; ++k) members[k] = g.conv_idx[k];
    if (pixels_per_tile) *pixels_per_tile = 64 * mr;
    return nblocks;
}

int hrn_plan_s2_map(hrn_handle h, int group, int n, int32_t *blocks, int capacity, int32_t *parts, int part_capacity, int32_t *active) {
    if (!h || n <= 0 || n > h->max_batch) return -1;
    // group -1: the fused stem's problem (conv2 with one output row per tile), when the handle runs it (hrn_stem_fused)
    if (group == -1 && !h->stem_fuse) return -1;
    if (group < -1 || group >= (int)h->s2groups.size()) return -1;
    const S2Group &g = group == -1 ? h->stemf : h->s2groups[group];
    std::vector<int2> map;
    const int nblocks = h->s2_blocks(g, n, &map);
    for (int i = 0; i < nblocks && i < capacity; ++i)
        blocks[(size_t)i * 3] = map[i].x & 0xff, blocks[(size_t)i * 3 + 1] = map[i].x >> 8, blocks[(size_t)i * 3 + 2] = map[i].y;
    int np = 0;  // per part: problem, convolution, 48-cout tile, rows per tile, tiles per image
    for (size_t k = 0; k < g.probs.size(); ++k)
        for (auto &pt : g.probs[k].parts) {
            if (np < part_capacity) {
                int32_t *o = parts + (size_t)np * 5;
                o[0] = (int32_t)k, o[1] = pt.first, o[2] = pt.second, o[3] = g.probs[k].rows, o[4] = g.probs[k].tiles_per_image;
            }
            ++np;
        }
    if (active) *active = h->s2_active(g, n) ? 1 : 0;
    return nblocks | (np << 20);
}

int hrn_plan_head_slabs(hrn_handle h, int n, int32_t *slab_px) {
    if (!h || n <= 0 || n > h->max_batch) return -1;
    if (slab_px) *slab_px = h->head_px_for(n);
    return h->head_slabs_for(n);
}

int hrn_plan_launch_walk(hrn_handle h, int kind, int index, int n, int32_t *out) {
    if (!h || !out || n <= 0 || n > h->max_batch || index < 0) return -1;
    if (kind != 0 && kind != 1) return -1;
    if (index >= (int)(kind == 0 ? h->groups.size() : h->chains.size())) return -1;
    int pos = -1;
    for (size_t oi = 0; oi < h->ops.size(); ++oi)
        if (h->ops[oi].kind == (kind == 0 ? OP_CONV3_GROUP : OP_CHAIN) && h->ops[oi].idx == index) pos = (int)oi;
    if (pos < 0) return -1;
    out[0] = pos, out[1] = h->walks_back(pos) ? 1 : 0, out[2] = out[3] = out[4] = 0;
    if (kind == 1) {
        const auto &ch = h->chains[index];
        out[4] = ch.conv2 >= 0 ? (ch.conv1 >= 0 ? 2 : 3) : ch.ds >= 0 ? 1 : 0;   // (launch_bottleneck_chain_t)
        const int m = n * h->tensors[h->convs[ch.conv3].out_t].hpwp;
        out[2] = chain_waves(ch.ds >= 0, ch.conv2 >= 0) * chain_grid(m, ch.ds >= 0, ch.conv2 >= 0, h->chain_blocks);
        out[3] = (m + 15) / 16;
    }
    return 0;
}

int hrn_profile_pass(hrn_handle h, const void *images_dev, int n, float *conv_ms, int conv_ms_len, float *other_ms,
                     void *stream) {
    if (!h) return 1;
    if (n > h->max_batch) n = h->max_batch;
    // profiling computes heat-map partials only (no pts): boxes are not needed
    if (!h->check_forward_args(images_dev, n, nullptr, nullptr, nullptr, /*outputs_optional=*/true)) return 7;
    if (!h->hip_ok(hipSetDevice(h->device), "hipSetDevice")) return 6;
    hrn_ctx::Timing tm;
    tm.ev.resize(h->ops.size() + 1);
    for (auto &e : tm.ev)
        if (!h->hip_ok(hipEventCreate(&e), "hipEventCreate")) return 6;
    CallScope scope(h, &h->pass, (hipStream_t)stream);
    bool ok = scope.entered && h->run_pass((const float *)images_dev, n, nullptr, 0, nullptr, nullptr, (hipStream_t)stream, &tm) && scope.leave();
    ok = ok && h->hip_ok(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
    if (ok) {
        if (other_ms) other_ms[0] = other_ms[1] = other_ms[2] = other_ms[3] = 0.f;
        for (int i = 0; i < conv_ms_len; ++i) conv_ms[i] = 0.f;
        for (size_t oi = 0; oi < h->ops.size(); ++oi) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, tm.ev[oi], tm.ev[oi + 1]);
            const Op &op = h->ops[oi];
            if (op.kind == OP_CONV) {
                if (conv_ms && op.idx < conv_ms_len) conv_ms[op.idx] = ms;
            } else if (op.kind == OP_CONV3_GROUP) {  // one launch, several convs: split by FLOPs
                const Conv3Group &g = h->groups[op.idx];
                double tot = 0;  // (a fused BasicBlock's launch carries its conv2 as well, and conv2's launch skips it)
                for (int ci : g.conv_idx) {
                    const ConvOp &cv = h->convs[ci];
                    if (h->skipped(cv, n)) continue;
                    tot += cv.flops + (h->fused_now(cv, n) ? h->convs[cv.fuse_with].flops : 0.0);
                }
                for (int ci : g.conv_idx) {
                    const ConvOp &cv = h->convs[ci];
                    if (h->skipped(cv, n)) continue;
                    if (conv_ms && ci < conv_ms_len) conv_ms[ci] = (float)(ms * cv.flops / tot);
                    const int c2 = h->fused_now(cv, n) ? cv.fuse_with : -1;
                    if (conv_ms && c2 >= 0 && c2 < conv_ms_len) conv_ms[c2] = (float)(ms * h->convs[c2].flops / tot);
                }
            } else if (op.kind == OP_CONV_GROUP) {  // likewise; these are latency / bandwidth bound: split by block count
                const DirectGroup &g = h->dgroups[op.idx];
                double tot = 0;
                std::vector<double> wgt;
                for (int ci : g.conv_idx) {
                    const ConvOp &cv = h->convs[ci];
                    wgt.push_back((double)h->grid_of(cv).hpwp * (cv.cout / (16 * g.nr)) * cv.kchunks);
                    tot += wgt.back();
                }
                for (size_t k = 0; k < g.conv_idx.size(); ++k)
                    if (conv_ms && g.conv_idx[k] < conv_ms_len) conv_ms[g.conv_idx[k]] = (float)(ms * wgt[k] / tot);
            } else if (op.kind == OP_S2_GROUP) {  // one launch (or its generic fallback): split by FLOPs
                const S2Group &g = h->s2groups[op.idx];
                double tot = 0;
                for (int ci : g.conv_idx) tot += h->convs[ci].flops;
                for (int ci : g.conv_idx)
                    if (conv_ms && ci < conv_ms_len) conv_ms[ci] = (float)(ms * h->convs[ci].flops / tot);
            } else if (op.kind == OP_CHAIN) {  // 1x1 convs of equal FLOPs (+ the 3x3 in front of them): split by FLOPs
                const hrn_ctx::Chain &ch = h->chains[op.idx];
                double tot = 0;
                for (int ci : {ch.conv3, ch.conv1, ch.ds, ch.conv2})
                    if (ci >= 0) tot += h->convs[ci].flops;
                for (int ci : {ch.conv3, ch.conv1, ch.ds, ch.conv2})
                    if (conv_ms && ci >= 0 && ci < conv_ms_len) conv_ms[ci] = (float)(ms * h->convs[ci].flops / tot);
            } else if (other_ms) {
                const int slot = (op.kind == OP_STEM || op.kind == OP_STEM7 || op.kind == OP_MAXPOOL) ? 0 : op.kind == OP_FUSE ? 1 : op.kind == OP_HEAD ? 2 : 3;
                other_ms[slot] += ms;
            }
        }
    }
    for (auto &e : tm.ev) (void)hipEventDestroy(e);
    return ok ? 0 : 8;
}

}  // extern "C"
