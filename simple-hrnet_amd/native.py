"""Host-side mirror of the reference's model seam, backed by the C ABI (include/hrnet_mi355.h).

``NativeHRNet`` is assignable to ``SimpleHRNet.model`` -- the reference invokes it as
``self.model(images)`` under ``torch.no_grad()`` and consumes ``.detach().cpu().numpy()``
(SimpleHRNet.py:284-296, 419-431), exactly as it does for its own TensorRT swap
(SimpleHRNet.py:143-147) -- and additionally offers the fused ``predict_crops`` (model call +
arg-max decode on the GPU, replacing SimpleHRNet.py:281-308 / 416-443).

PyTorch is used only as the container for device memory and for the current HIP stream.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .frames import (NUMPY_DTYPES, PIX_FORMATS, YUV_MATRICES, YUV_RANGES, Frames, YuvFrame, _bgr_rows, _check_frame, _frame_kind, as_tensor,  # noqa: F401
                     device_tensor, frame_stack, host_array, host_bytes, rotation_code_from_degrees, rotation_codes)
from .palettes import bgr_to_yuv_colors, embedded_palette, find_palette, heat_colormap  # noqa: F401

DTYPES = {"fp32": 0, "f32": 0, "float32": 0, torch.float32: 0, "bf16": 1, "bfloat16": 1, torch.bfloat16: 1,
          "fp16": 2, "f16": 2, "float16": 2, "half": 2, torch.float16: 2}
DTYPE_NAMES = {0: "fp32", 1: "bf16", 2: "fp16"}
# sub-pixel joint decoding (include/hrnet_mi355.h: HRN_REFINE_*): None = the integer arg-max of SimpleHRNet.py:297-308
REFINE_MODES = {None: 0, "quarter": 1, "dark": 2}


def refine_code(refine) -> int:
    """HRN_REFINE_* of a ``refine`` argument: None, "quarter" or "dark"; anything else raises ValueError"""
    if not (refine is None or isinstance(refine, str)) or refine not in REFINE_MODES:
        raise ValueError("refine must be None, 'quarter' or 'dark', got %r" % (refine,))
    return REFINE_MODES[refine]


def crop_code(variant) -> int:
    """HRN_CROP_* of a ``variant`` argument: "pad" or "clamp"; anything else raises ValueError"""
    if variant not in ("pad", "clamp"):
        raise ValueError("variant must be 'pad' or 'clamp'")
    return 0 if variant == "pad" else 1


DRAW_TILE = 32   # csrc/kernels.h: kDrawTile -- the rasteriser of draw_poses works on 32 x 32 tiles (tests place shapes across the borders)


_PALETTE_CACHE: Dict[Tuple[str, int], np.ndarray] = {}   # (tests empty it here, so the cache stays in this module)


def palette(name: str, samples: int = 16) -> np.ndarray:
    """The colours ``draw_points`` / ``draw_skeleton`` derive from a matplotlib palette name (``misc/visualization.py:91-98``) as a
    (C, 3) uint8 array of (B, G, R) rows: a listed palette's own colours, else ``samples`` colours sampled over [0, 1].  Evaluated
    with matplotlib where it can be imported; without it the four palettes of the demo programs (``tab20``, ``Set2``,
    ``gist_rainbow`` at 10 samples, ``jet`` at 8) come from stored tables and any other name raises ValueError."""
    key = (str(name), int(samples))
    if key not in _PALETTE_CACHE:
        _PALETTE_CACHE[key] = find_palette(*key)
    return _PALETTE_CACHE[key].copy()


HEAT_ALPHA_MODES = {"const": 0, "value": 1}   # include/hrnet_mi355.h: HRN_HEAT_ALPHA_CONST / _VALUE


def heat_arguments(J: int, joints, colormap, alpha, alpha_mode, vmin, vmax, cutoff):
    """the scalar arguments of ``draw_heatmaps`` (here and in ``postproc``) as the C ABI takes them: (joint mask (J,) uint8 or None,
    BGR table (256, 3) uint8, alpha 0..255, mode code, lo, hi, cutoff 1..255); ValueError on what the library would not be asked"""
    mask = None
    if joints is not None:
        if isinstance(joints, str) or any(isinstance(j, str) for j in joints):
            raise ValueError("joints must be joint indices: this package knows no joint names (take them from the reference's joints_dict())")
        idx = np.asarray(joints, dtype=np.int64).reshape(-1)
        if len(idx) < 1 or idx.min() < 0 or idx.max() >= J:
            raise ValueError("joints must be a non-empty list of indices in [0, %d)" % J)
        mask = np.zeros((J,), np.uint8)
        mask[idx] = 1
    if isinstance(colormap, str):
        lut = heat_colormap(colormap)
    else:
        lut = np.asarray(colormap)
        if lut.shape != (256, 3) or lut.dtype != np.uint8:
            raise ValueError("colormap must be a name (heat_colormap) or a (256, 3) uint8 array of (B, G, R) rows")
        lut = np.ascontiguousarray(lut)
    if alpha_mode not in HEAT_ALPHA_MODES:
        raise ValueError("alpha_mode must be 'const' or 'value', got %r" % (alpha_mode,))

    def byte(x, what, low):
        v = int(round(255 * float(x))) if isinstance(x, (float, np.floating)) else int(x)
        if not low <= v <= 255:
            raise ValueError("%s must be in [%s, 1.0] as a float or [%d, 255] as an integer, got %r" % (what, "1/255" if low else "0.0", low, x))
        return v

    return mask, lut, byte(alpha, "alpha", 0), HEAT_ALPHA_MODES[alpha_mode], float(vmin), float(vmax), byte(cutoff, "cutoff", 1)


COCO_HEAD_JOINTS = (0, 1, 2, 3, 4)   # nose, eyes and ears in the reference's joints_dict()["coco"] (misc/visualization.py): ``mosaic(joints=...)``


def mosaic_arguments(J: Optional[int], joints, scale, min_half, cell):
    """the scalar arguments of ``mosaic`` (here and in ``postproc``) as the C ABI takes them: (joint list (K,) int32 or None for
    boxes, scale_num, scale_den, min_half, cell); ValueError on what the library would not be asked.  ``J`` None: the people come
    from boxes and ``joints`` must not be given"""
    idx = None
    if J is None:
        if joints is not None:
            raise ValueError("joints choose among the joints of pts: with boxes there are none")
    elif joints is None:
        idx = np.arange(J, dtype=np.int32)
    else:
        if isinstance(joints, str) or any(isinstance(j, str) for j in joints):
            raise ValueError("joints must be joint indices: this package knows no joint names (take them from the reference's joints_dict())")
        idx = np.ascontiguousarray(np.asarray(joints, dtype=np.int64).reshape(-1))
        if len(idx) < 1 or len(idx) > 256 or idx.min() < 0 or idx.max() >= J:
            raise ValueError("joints must be a list of 1 to 256 indices in [0, %d)" % J)
        idx = idx.astype(np.int32)
    try:
        num, den = (int(v) for v in scale)
    except (TypeError, ValueError):
        raise ValueError("scale must be a pair of integers (numerator, denominator), each in [1, 64], got %r" % (scale,)) from None
    if (num, den) != tuple(scale):
        raise ValueError("scale must be a pair of integers (numerator, denominator), each in [1, 64], got %r" % (scale,))
    return idx, num, den, 0 if min_half is None else int(min_half), 0 if cell is None else int(cell)


def _colors(spec, samples) -> np.ndarray:
    """a palette name, or ready (C, 3) uint8 BGR colours"""
    if isinstance(spec, str):
        return palette(spec, samples)
    c = np.asarray(spec)
    if c.ndim != 2 or c.shape[1] != 3 or len(c) < 1 or c.dtype != np.uint8:
        raise ValueError("colours must be a palette name or a (C, 3) uint8 array of (B, G, R) rows")
    return np.ascontiguousarray(c)


def _device_index(device) -> int:
    if isinstance(device, int):
        return device
    d = torch.device(device)
    if d.type != "cuda":
        raise ValueError("Wrong device name.")  # same message as SimpleHRNet.py:139
    return d.index if d.index is not None else torch.cuda.current_device()


def group_frames(counts, limit: int, people_per_pass: Optional[int] = None):
    """The frame-grouping rule of ``predict_frames`` and ``predict_clip``: which people share a pass.

    ``counts``: people per frame, in order (any iterable; it is read lazily, one frame ahead of the group being formed);
    ``limit``: the engine's ``max_batch``; ``people_per_pass``: at most that many people per group (default ``limit``; more than
    ``limit`` is refused with ValueError, as is anything below 1).  Yields groups, each a list of ``(frame, lo, hi)``: people
    ``lo:hi`` of frame ``frame`` -- in frame order, every person exactly once, every frame in at least one group:

    * consecutive frames are packed greedily while their people fit; a frame is never split to fill a group up;
    * a frame without people joins the group being formed as ``(frame, 0, 0)`` (its empty result keeps its place in the order);
    * a frame with more people than fit one pass closes the group being formed and goes out alone, in as many groups of its
      own as it needs (``(f, 0, P), (f, P, 2P), ...``); the frame after it starts a fresh group."""
    per_pass = limit if people_per_pass is None else people_per_pass
    if isinstance(per_pass, bool) or int(per_pass) != per_pass or per_pass < 1:
        raise ValueError("people_per_pass must be a positive integer, got %r" % (people_per_pass,))
    if per_pass > limit:
        raise ValueError("people_per_pass=%d exceeds max_batch=%d" % (per_pass, limit))
    per_pass = int(per_pass)
    group, held = [], 0
    for f, c in enumerate(counts):
        c = int(c)
        if c < 0:
            raise ValueError("frame %d has a negative number of people" % f)
        if c > per_pass:
            if group:
                yield group
            for lo in range(0, c, per_pass):
                yield [(f, lo, min(c, lo + per_pass))]
            group, held = [], 0
            continue
        if held + c > per_pass:
            yield group
            group, held = [], 0
        group.append((f, 0, c))
        held += c
    if group:
        yield group


def _detections(detections, trim: bool = True) -> np.ndarray:
    """one frame's detections as a contiguous (P, 4) float32 array (None: nobody; ``trim=False``: (P, >=4)); ValueError otherwise"""
    if detections is None:
        return np.zeros((0, 4), np.float32)
    d = host_array(detections, np.float32)
    if d.ndim != 2 or (len(d) and d.shape[1] < 4):
        raise ValueError("detections must be (P, >=4)")
    return np.ascontiguousarray(d[:, :4] if trim else d) if len(d) else np.zeros((0, 4), np.float32)


def _warp_arguments(nframes: int, size_wh, centers, scales, rotations, frame_index, pixel_std, matrices):
    """the host-side arguments of ``hrn_warp_crops``: ``(matrices (n, 6) float64, frame_index (n,) int32)``, checked -- every
    argument error is a ValueError here, before the library is called"""
    from . import postproc

    if matrices is not None:
        if centers is not None or scales is not None or rotations is not None:
            raise ValueError("give either centers / scales (/ rotations) or matrices, not both")
        m = np.asarray(matrices, dtype=np.float64)
        if m.ndim < 2 or m.size != m.shape[0] * 6 or tuple(m.shape[1:]) not in ((2, 3), (6,)):
            raise ValueError("matrices must be (n, 2, 3) or (n, 6)")
        m = np.ascontiguousarray(m.reshape(-1, 6))
    else:
        if centers is None or scales is None:
            raise ValueError("centers and scales (or matrices) are needed")
        c = np.asarray(centers)
        n = len(c)
        sc = np.asarray(scales)
        rot = np.zeros(n) if rotations is None else np.asarray(rotations)
        if c.shape != (n, 2) or sc.shape not in ((n, 2), (n,)) or rot.shape != (n,):
            raise ValueError("centers must be (n, 2), scales (n, 2) or (n,), rotations (n,): got %s, %s, %s" % (c.shape, sc.shape, rot.shape))
        m = np.empty((n, 6), np.float64)
        for i in range(n):
            m[i] = postproc.affine_matrix(c[i], sc[i], pixel_std, rot[i], size_wh).reshape(6)
    n = len(m)
    if not np.isfinite(m).all():
        raise ValueError("a matrix is not finite")
    if n and ((m[:, 0] * m[:, 4] - m[:, 1] * m[:, 3]) == 0).any():
        raise ValueError("a matrix is singular")
    if frame_index is None:
        if nframes not in (1, n):
            raise ValueError("without frame_index there must be one frame per crop, or one frame: %d frames, %d crops" % (nframes, n))
        fi = np.zeros(n, np.int32) if nframes == 1 else np.arange(n, dtype=np.int32)
    else:
        fi = np.asarray(frame_index)
        if fi.shape != (n,) or fi.dtype.kind not in "iu":
            raise ValueError("frame_index must be %d integers" % n)
        if n and (fi.min() < 0 or fi.max() >= nframes):
            raise ValueError("frame_index outside [0, %d)" % nframes)
        fi = np.ascontiguousarray(fi, dtype=np.int32)
    return m, fi


class UploadPipeline:
    """Two device buffers ("slots") filled in turn on a copy stream while the stream that was current at construction (the
    compute stream) works on the other one: the plumbing of ``predict_stream`` and ``predict_clip``.  Per item the caller
    takes ``buffer(slot, ...)``, copies inside ``with filling(slot)``, and on the compute stream calls ``ready(slot)`` before
    the work that reads the slot and ``release(slot)`` after it."""

    def __init__(self, device):
        self.device = device
        self.compute = torch.cuda.current_stream(device)
        self.copy = torch.cuda.Stream(device)
        self.slots = [None, None]
        self.landed = [torch.cuda.Event(), torch.cuda.Event()]
        self.consumed = [None, None]
        self.copy.wait_stream(self.compute)   # the first upload must not overtake the compute stream either (see buffer)

    def buffer(self, slot: int, dtype, shape, at_least: Optional[int] = None) -> torch.Tensor:
        """the slot's device buffer as long as it has ``dtype`` and ``at_least`` elements (default: those of ``shape``), else a
        new one of ``shape`` in its place"""
        have = self.slots[slot]
        if have is None or have.dtype != dtype or have.numel() < (math.prod(shape) if at_least is None else at_least):
            # a new block comes from the caching allocator on the COMPUTE stream and may be recycled memory that kernels already
            # queued there still read: the upload into it must not overtake them
            self.slots[slot] = torch.empty(shape, dtype=dtype, device=self.device)
            self.slots[slot].record_stream(self.copy)
            self.copy.wait_stream(self.compute)
        return self.slots[slot]

    @contextlib.contextmanager
    def filling(self, slot: int):
        """the scope of the copies into the slot: on the copy stream, after the work that read the slot last; what is copied has
        landed when the scope ends"""
        with torch.cuda.stream(self.copy):
            if self.consumed[slot] is not None:
                self.copy.wait_event(self.consumed[slot])
            yield
            self.landed[slot].record(self.copy)

    def ready(self, slot: int):
        """the compute stream goes on when the copies into the slot have landed"""
        self.compute.wait_event(self.landed[slot])

    def release(self, slot: int):
        """the work queued on the compute stream so far is the last that reads the slot"""
        self.consumed[slot] = torch.cuda.Event()
        self.consumed[slot].record(self.compute)


class NativeHRNet:
    """HRNet-W{c} pose network compiled to hand-written gfx950 kernels.

    Parameters mirror ``HRNet(c, nof_joints)`` (models_/hrnet.py:75) plus what a static engine
    needs up front: input ``resolution`` (h, w), arithmetic ``dtype`` ('bf16' MFMA with fp32
    accumulate, 'fp16' -- the same plan and kernels with fp16 storage: 11 significant bits instead of 8 --,
    or 'fp32' exact-fp32 MFMA), and ``max_batch`` = crops per internal pass.
    ``device=-1`` builds a plan-only handle (graph + weight packing on the host, no GPU): it cannot
    run -- there is no CPU compute path.
    """

    def __init__(self, c: int = 48, nof_joints: int = 17, resolution: Tuple[int, int] = (384, 288),
                 dtype: Union[str, torch.dtype] = "bf16", max_batch: int = 32, device=0, model_name: str = "HRNet"):
        if dtype not in DTYPES:
            raise ValueError("dtype must be 'bf16', 'fp16' or 'fp32'")
        if model_name in ("HRNet", "hrnet"):            # SimpleHRNet.py:109-112
            model = 0
        elif model_name in ("PoseResNet", "poseresnet", "ResNet", "resnet"):
            model = 1                                  # c = ResNet size (50 / 101 / 152)
        else:
            raise ValueError("Wrong model name.")
        self.model_name = "HRNet" if model == 0 else "PoseResNet"
        self.c, self.nof_joints = int(c), int(nof_joints)
        self.resolution = (int(resolution[0]), int(resolution[1]))
        self.dtype = DTYPE_NAMES[DTYPES[dtype]]
        self.max_batch = int(max_batch)
        self.device_index = -1 if (isinstance(device, int) and device < 0) else _device_index(device)
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        rc = self._lib.hrn_create_model(ctypes.byref(self._h), model, self.c, self.nof_joints, self.resolution[0],
                                        self.resolution[1], DTYPES[dtype], self.max_batch, self.device_index)
        if rc != 0:
            msg = self._lib.hrn_last_error(None).decode()
            self._h = ctypes.c_void_p()
            raise (ValueError if rc == 2 else RuntimeError)("hrn_create failed: " + msg)
        self._keep = None
        # rotate_frames' lean path: the two hrn_canvas entries and the three codes of a one-frame call (read by the call before it returns)
        self._rot_pair = (_lib.CanvasC * 2)()
        self._rot_codes = np.arange(3, dtype=np.int32)
        self._rot_code_ptr = [self._rot_codes.ctypes.data + 4 * k for k in range(3)]

    # -- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.hrn_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self._lib.hrn_last_error(self._h).decode()))

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device_index).cuda_stream

    def _launch(self, name: str, *args):
        """the one way into a GPU entry of the library: ``name(handle, *args, current stream)`` on the engine's device;
        RuntimeError with the library's message when it refuses"""
        with torch.cuda.device(self.device_index):
            rc = getattr(self._lib, name)(self._h, *args, self._stream())
        self._check(rc, name)

    # -- nn.Module look-alikes the reference calls on self.model (SimpleHRNet.py:141-142) --------
    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    @property
    def torch_device(self) -> torch.device:
        return torch.device("cuda", self.device_index)

    # -- weights --------------------------------------------------------------------------------
    def load_state_dict(self, state_dict: Dict) -> "NativeHRNet":
        """Accepts what ``torch.load(checkpoint)`` yields: a raw ``state_dict`` or ``{'model': ...}``
        (SimpleHRNet.py:117-121); values may be torch tensors or numpy arrays."""
        if "model" in state_dict and not hasattr(state_dict["model"], "shape"):
            state_dict = state_dict["model"]
        keep, descs = [], []
        for k, v in state_dict.items():
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().numpy()
            a = np.asarray(v)
            if a.dtype == np.int64:
                code = 1
            else:
                a = np.ascontiguousarray(a, dtype=np.float32)
                code = 0
            if a.ndim > 4:
                raise ValueError("state_dict entry %s has %d dims" % (k, a.ndim))
            keep.append(a)
            dims = (ctypes.c_int64 * 4)(*(list(a.shape) + [0] * (4 - a.ndim)))
            descs.append(_lib.TensorDesc(k.encode(), a.ctypes.data_as(ctypes.c_void_p), a.ndim, dims, code))
        arr = (_lib.TensorDesc * len(descs))(*descs)
        rc = self._lib.hrn_load_weights(self._h, arr, len(descs))
        if rc != 0:
            raise KeyError("hrn_load_weights: " + self._lib.hrn_last_error(self._h).decode())
        return self

    def load_checkpoint(self, path: str) -> "NativeHRNet":
        return self.load_state_dict(torch.load(path, map_location="cpu"))

    # -- multi-GPU weight distribution (RCCL broadcast of the packed blob) -------------------------
    def weight_blob_bytes(self) -> int:
        return int(self._lib.hrn_weight_blob_bytes(self._h))

    def weight_blob_tensor(self) -> torch.Tensor:
        """uint8 CUDA tensor aliasing the packed-weight blob (zero-copy, for torch.distributed)."""

        class _Raw:
            pass

        raw = _Raw()
        raw.__cuda_array_interface__ = {"shape": (self.weight_blob_bytes(),), "typestr": "|u1",
                                        "data": (int(self._lib.hrn_weight_blob_ptr(self._h)), False), "version": 2}
        raw._owner = self
        with torch.cuda.device(self.device_index):
            return torch.as_tensor(raw, device=self.torch_device)

    def adopt_weights(self):
        rc = self._lib.hrn_adopt_weights(self._h)
        self._check(rc, "hrn_adopt_weights")

    def read_blob(self, offset: int, nbytes: int) -> np.ndarray:
        out = np.empty(nbytes, dtype=np.uint8)
        rc = self._lib.hrn_weight_blob_read(self._h, offset, out.ctypes.data_as(ctypes.c_void_p), nbytes)
        self._check(rc, "hrn_weight_blob_read")
        return out

    # -- the hot path ---------------------------------------------------------------------------
    def _images_ptr(self, images: torch.Tensor) -> torch.Tensor:
        if not isinstance(images, torch.Tensor):
            raise TypeError("images must be a torch.Tensor (n,3,H,W)")
        h, w = self.resolution
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, h, w):
            raise ValueError("images must have shape (n,3,%d,%d), got %s" % (h, w, tuple(images.shape)))
        if images.device.type != "cuda":
            images = images.to(self.torch_device, non_blocking=True)
        elif images.device.index != self.device_index:
            raise ValueError("images live on %s, engine on cuda:%d" % (images.device, self.device_index))
        return images.to(torch.float32).contiguous()

    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        """``self.model(images)``: (n,3,H,W) fp32 -> heat-maps (n,J,H/4,W/4) fp32 on the same GPU."""
        x = self._images_ptr(images)
        n = x.shape[0]
        h, w = self.resolution
        out = torch.empty((n, self.nof_joints, h // 4, w // 4), dtype=torch.float32, device=x.device)
        if n:
            self._launch("hrn_forward", x.data_ptr(), n, None, 0, None, out.data_ptr())
        return out

    forward = __call__

    def predict_crops(self, images: torch.Tensor, boxes, return_heatmaps: bool = False, refine: Optional[str] = None):
        """Model call + decode (SimpleHRNet.py:281-308): returns ``pts`` (n,J,3) fp32 CUDA tensor of
        ``(y, x, confidence)``; with ``return_heatmaps`` also the (n,J,H/4,W/4) heat-maps.
        ``boxes``: (n,4) ``[x1,y1,x2,y2]`` int32 (multi-person path) or float32 (single-person).
        ``refine``: None = the integer arg-max; ``"quarter"`` = a quarter cell towards the higher neighbour
        (get_final_preds); ``"dark"`` = DARK's sub-pixel decoding (include/hrnet_mi355.h: hrn_forward_refined)."""
        mode = refine_code(refine)
        x = self._images_ptr(images)
        n = x.shape[0]
        b = as_tensor(boxes)
        if tuple(b.shape) != (n, 4):
            raise ValueError("boxes must have shape (%d,4), got %s" % (n, tuple(b.shape)))
        if b.dtype in (torch.int32, torch.int64, torch.int16, torch.uint8):
            b, box_dtype = b.to(torch.int32), 0
        else:
            b, box_dtype = b.to(torch.float32), 1
        b = b.to(x.device).contiguous()
        h, w = self.resolution
        pts = torch.empty((n, self.nof_joints, 3), dtype=torch.float32, device=x.device)
        hm = torch.empty((n, self.nof_joints, h // 4, w // 4), dtype=torch.float32,
                         device=x.device) if return_heatmaps else None
        if n:   # (mode 0 = HRN_REFINE_NONE: hrn_forward_refined is hrn_forward)
            self._launch("hrn_forward_refined", x.data_ptr(), n, b.data_ptr(), box_dtype, mode, pts.data_ptr(),
                         hm.data_ptr() if hm is not None else None)
        return (hm, pts) if return_heatmaps else pts

    def predict_stream(self, batches, return_heatmaps: bool = False, refine: Optional[str] = None):
        """Model call + decode for a sequence of HOST-resident batches with the uploads hidden behind the compute:
        batch k+1 crosses PCIe on a copy stream (two device staging buffers) while batch k runs on the current stream.
        ``batches``: iterable of ``(images, boxes (n,4))`` with ``n <= max_batch``; ``images`` is a HOST tensor (pinned memory for
        a truly asynchronous copy), either ``(n,3,H,W) float32`` -- the normalised crops the reference builds on the CPU
        (``SimpleHRNet.py:213-232``) -- or ``(n,H,W,3) uint8`` BGR crops already at the network's resolution (what ``cv2.resize``
        leaves before ``cvtColor`` / ``ToTensor`` / ``Normalize``): a quarter of the bytes over PCIe (85 MB instead of 340 MB per
        256 crops of 384x288), the colour flip and the normalisation then run on the GPU (``hrn_resize_frames`` at identity size:
        the reference transform's float32 arithmetic).  Yields, per batch, what ``predict_crops`` returns (results of batch k
        are ready on the current stream; read them after a synchronize or through ``.cpu()``).  ``refine``: as in ``predict_crops``."""
        refine_code(refine)
        dev = self.torch_device
        h, w = self.resolution
        pipe = UploadPipeline(dev)   # its slots: fp32 NCHW or uint8 NHWC staging, by what the caller sends
        norm = [None, None]   # uint8 form: the normalised fp32 crops of each slot

        def upload(slot, item):
            images, boxes = item
            if not isinstance(images, torch.Tensor) or images.device.type != "cpu":
                raise TypeError("predict_stream takes host tensors; device-resident crops go to predict_crops")
            n = images.shape[0]
            if n > self.max_batch:
                raise ValueError("a batch of %d crops exceeds max_batch=%d" % (n, self.max_batch))
            u8 = images.dtype == torch.uint8
            if u8 and tuple(images.shape[1:]) != (h, w, 3):
                raise ValueError("uint8 crops must be (n, %d, %d, 3) BGR at the network's resolution" % (h, w))
            if not u8 and tuple(images.shape[1:]) != (3, h, w):   # (copy_ would broadcast or fail obscurely)
                raise ValueError("float crops must be (n, 3, %d, %d) at the network's resolution" % (h, w))
            stage = pipe.buffer(slot, torch.uint8, (self.max_batch, h, w, 3)) if u8 else \
                pipe.buffer(slot, torch.float32, (self.max_batch, 3, h, w))
            with pipe.filling(slot):                             # the pass that read this buffer has finished
                stage[:n].copy_(images if u8 else images.to(torch.float32), non_blocking=True)
            return n, boxes, u8

        it = iter(batches)
        nxt = next(it, None)
        pending = upload(0, nxt) if nxt is not None else None
        k = 0
        while pending is not None:
            slot = k & 1
            n, boxes, u8 = pending
            nxt = next(it, None)
            pending = upload(slot ^ 1, nxt) if nxt is not None else None   # goes out while this batch computes
            pipe.ready(slot)
            if u8:   # identity size: colour flip + ToTensor + Normalize on the GPU, into ONE fp32 buffer per slot (340 MB at 256 crops)
                if norm[slot] is None:
                    norm[slot] = torch.empty((self.max_batch, 3, h, w), dtype=torch.float32, device=dev)
                x = self.resize_frames(pipe.slots[slot][:n], 0, out=norm[slot])
            else:
                x = pipe.slots[slot][:n]
            out = self.predict_crops(x, boxes, return_heatmaps=return_heatmaps, refine=refine)
            pipe.release(slot)
            yield out
            k += 1

    # -- introspection --------------------------------------------------------------------------
    def predict_flip_tta(self, images: torch.Tensor, flip_pairs, post_processing: Union[bool, str] = True):
        """Flip test-time augmentation + evaluation decode (``testing/Test.py:132-140``, ``misc/utils.py:9-29, 125-175``):
        returns ``(heatmaps (n,J,h,w) averaged over the crop and its mirror image, preds (n,J,2) = (x, y) in heat-map
        pixels with the quarter-pixel refinement, maxvals (n,J,1))`` -- what ``get_final_preds`` works on before its
        inverse affine.  ``post_processing="dark"``: no quarter-pixel step; DARK's offset on the averaged maps instead
        (``refine_coords``), as DarkPose decodes its flip-averaged maps."""
        dark = isinstance(post_processing, str)
        if dark and post_processing != "dark":
            raise ValueError("post_processing must be True, False or 'dark', got %r" % (post_processing,))
        x = self._images_ptr(images)
        n = x.shape[0]
        fp = np.ascontiguousarray(np.asarray(flip_pairs, dtype=np.int32).reshape(-1, 2))
        h, w = self.resolution
        hm = torch.empty((n, self.nof_joints, h // 4, w // 4), dtype=torch.float32, device=x.device)
        preds = torch.empty((n, self.nof_joints, 2), dtype=torch.float32, device=x.device)
        maxvals = torch.empty((n, self.nof_joints, 1), dtype=torch.float32, device=x.device)
        if n:
            self._launch("hrn_forward_flip_tta", x.data_ptr(), n, fp.ctypes.data, len(fp), 1 if post_processing and not dark else 0,
                         hm.data_ptr(), preds.data_ptr(), maxvals.data_ptr())
            if dark:
                self._launch("hrn_refine_coords", hm.data_ptr(), n, REFINE_MODES["dark"], preds.data_ptr())
        return hm, preds, maxvals

    def refine_coords(self, heatmaps, coords, mode: Optional[str]) -> torch.Tensor:
        """The sub-pixel offset alone, in heat-map space: ``heatmaps`` (n,J,H/4,W/4) and integer-valued ``coords`` (n,J,2) =
        (x, y) in cells (e.g. ``predict_flip_tta(..., post_processing=False)``'s preds) -> the refined coordinates as a new
        (n,J,2) float32 tensor on this engine's GPU (include/hrnet_mi355.h: hrn_refine_coords).  ``mode``: "quarter", "dark"
        or None (a copy)."""
        code = refine_code(mode)
        h, w = self.resolution
        dev = self.torch_device
        hm = torch.as_tensor(heatmaps).to(dev, torch.float32).contiguous()
        out = torch.as_tensor(coords).to(dev, torch.float32).clone().contiguous()
        n = int(hm.shape[0]) if hm.dim() == 4 else -1
        if tuple(hm.shape) != (n, self.nof_joints, h // 4, w // 4) or tuple(out.shape) != (n, self.nof_joints, 2):
            raise ValueError("heatmaps must be (n,%d,%d,%d) and coords (n,%d,2), got %s and %s"
                             % (self.nof_joints, h // 4, w // 4, self.nof_joints, tuple(hm.shape), tuple(out.shape)))
        if n and code:
            self._launch("hrn_refine_coords", hm.data_ptr(), n, code, out.data_ptr())
        return out

    def preprocess_frame(self, frame: torch.Tensor, detections, variant: str = "pad") -> Tuple[torch.Tensor, np.ndarray, torch.Tensor]:
        """The crop pre-path of ``SimpleHRNet.predict`` for one frame (``SimpleHRNet.py:236-278``) on the GPU.

        ``frame``: (Hf, Wf, 3) uint8 BGR (the cv2 frame; host tensors / arrays are uploaded once), or a ``YuvFrame`` (any of its
        formats, 8- or 10-bit: the crops equal, bit for bit, those of the frame ``yuv_to_bgr`` makes of it);
        ``detections``: (P, >=4) float array-like, columns 0..3 = x1, y1, x2, y2 as the detector returns them.
        ``variant``: ``"pad"`` = the single-image path (aspect ratio corrected by zero padding), ``"clamp"`` = the batch
        path's enlarge-and-clamp (``SimpleHRNet.py:383-412``; call once per image of the stack).
        Returns ``(images (P,3,H,W) float32 on the GPU, boxes (P,4) int32 numpy, boxes on the GPU)`` -- bit-identical
        to the reference's ``ToPILImage -> Resize -> ToTensor -> Normalize`` of the RGB crops."""
        crop = crop_code(variant)
        if isinstance(frame, YuvFrame):   # the same call over a one-frame table of hrn_preprocess_frames_yuv
            frames = Frames([frame.to(self.torch_device, non_blocking=True)], True)
            dets = _detections(detections)
            return self._preprocess_table(frames.table(), 1, dets, np.zeros(len(dets), np.int32), variant)
        frame = as_tensor(frame)
        if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
            raise ValueError("frame must be (H, W, 3) uint8 BGR")
        frame = frame.to(self.torch_device, non_blocking=True).contiguous()
        dets = _detections(detections, trim=False)   # the rows go to the library as they are, with their stride
        p = len(dets)
        h, w = self.resolution
        images = torch.empty((p, 3, h, w), dtype=torch.float32, device=self.torch_device)
        boxes = np.empty((p, 4), dtype=np.int32)
        boxes_dev = torch.empty((p, 4), dtype=torch.int32, device=self.torch_device)
        if p:
            self._launch("hrn_preprocess_frame", frame.data_ptr(), int(frame.shape[0]), int(frame.shape[1]), dets.ctypes.data,
                         int(dets.shape[1]), p, crop, images.data_ptr(), boxes.ctypes.data, boxes_dev.data_ptr())
        return images, boxes, boxes_dev

    def yuv_to_bgr(self, frame: YuvFrame) -> torch.Tensor:
        """A whole ``YuvFrame`` as an (H, W, 3) uint8 BGR tensor on the engine's GPU (``hrn_yuv_to_bgr``): the bridge to a consumer
        that needs BGR, such as the detector -- a host frame still crosses PCIe once, at 1.5 bytes per pixel (3 for the 10-bit
        formats, whose result is 8-bit BGR too).  The arithmetic is the crop pre-path's (include/hrnet_mi355.h),
        cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420)'s form."""
        if not isinstance(frame, YuvFrame):
            raise TypeError("yuv_to_bgr takes a YuvFrame")
        frame = frame.to(self.torch_device, non_blocking=True)
        out = torch.empty((frame.height, frame.width, 3), dtype=torch.uint8, device=self.torch_device)
        entry = _lib.YuvFrameC()
        frame._fill(entry)
        self._launch("hrn_yuv_to_bgr", ctypes.byref(entry), out.data_ptr())
        return out

    def draw_poses(self, frames, pts, skeleton, frame_index=None, person_ids=None, points_palette="tab20", points_samples: int = 16,
                   skeleton_palette="Set2", skeleton_samples: int = 8, confidence_threshold: float = 0.5, radius: Optional[int] = None,
                   thickness: int = 2):
        """The overlay of the reference's demo programs on the GPU (``hrn_draw_poses``): for every person the bones of ``skeleton``
        and then the joints, later people over earlier ones -- the loop around ``draw_points_and_skeleton``
        (``scripts/live-demo.py:135-138``, ``misc/visualization.py:71-192``) in two launches, whatever the number of frames and
        people, and without the frame leaving the device.  The shapes are the integer definition of include/hrnet_mi355.h (discs,
        capsules), which looks like cv2's circles and lines; pixel equality with cv2 is not claimed.

        ``frames``: one (H, W, 3) uint8 BGR tensor or array (rows may be strided: a view into a larger frame), a ``YuvFrame``, or a
        list of either kind (entries nobody is drawn on may be None).  Frames on the engine's GPU are drawn IN PLACE and returned;
        host frames are uploaded and the device copy is returned.  Only covered pixels are written.
        ``pts``: (J, 3) or (n, J, 3) (y, x, confidence) as ``predict*`` returns them, on the device or the host;
        ``skeleton``: (K, 2) joint index pairs (``joints_dict()[set]["skeleton"]`` of the reference);
        ``frame_index``: n frame numbers when there are several frames; ``person_ids``: the ``person_index`` of each person
        (bone colour ``person_ids[i] % len(palette)``; default i) -- a tensor on the engine's GPU (the ids of
        ``associate_people`` / ``PersonTracker.update``) stays there: ``hrn_draw_poses_ids_dev`` looks the colours up on the
        device, with no host read; anything else is read on the host as before;
        palettes: a matplotlib name (``palette``) or ready (C, 3) uint8 BGR colours -- converted with ``bgr_to_yuv_colors`` for
        ``YuvFrame``s, which then share one matrix and range;
        ``radius``: of a joint's disc (default: the reference's ``max(1, min(H, W) // 160)`` per frame); ``thickness``: of a bone."""
        single = not isinstance(frames, (list, tuple))
        items = [frames] if single else list(frames)
        if not items:
            raise ValueError("draw_poses needs at least one frame")
        dev = self.torch_device
        canvases = Frames.canvases(items, dev)
        table = canvases.table(kind=_lib.CanvasC)
        pts = as_tensor(pts, np.float32)
        if pts.dim() == 2:
            pts = pts.unsqueeze(0)
        if pts.dim() != 3 or pts.shape[2] != 3 or pts.shape[1] < 1:
            raise ValueError("pts must be (J, 3) or (n, J, 3) (y, x, confidence)")
        pts = device_tensor(pts, dev, torch.float32)
        n, joints = int(pts.shape[0]), int(pts.shape[1])
        skel = np.ascontiguousarray(np.asarray(skeleton, dtype=np.int32).reshape(-1, 2))
        fi = None
        if frame_index is not None:
            fi = np.ascontiguousarray(np.asarray(frame_index, dtype=np.int32).reshape(-1))
            if len(fi) != n:
                raise ValueError("frame_index must have one entry per person: %d for %d people" % (len(fi), n))
        elif len(items) != 1:
            raise ValueError("several frames need frame_index: which frame each person is drawn on")
        ids = ids_dev = None
        if isinstance(person_ids, torch.Tensor) and person_ids.is_cuda:
            if person_ids.device != dev or person_ids.dtype != torch.int32:
                raise ValueError("person_ids on a GPU must be an int32 tensor on the engine's device %s (the ids of associate_people / "
                                 "PersonTracker.update), got %s on %s" % (dev, person_ids.dtype, person_ids.device))
            ids_dev = person_ids.reshape(-1).contiguous()
            if len(ids_dev) != n:
                raise ValueError("person_ids must have one entry per person: %d for %d people" % (len(ids_dev), n))
        elif person_ids is not None:
            ids = np.ascontiguousarray(np.asarray(person_ids, dtype=np.int32).reshape(-1))
            if len(ids) != n:
                raise ValueError("person_ids must have one entry per person: %d for %d people" % (len(ids), n))
        pc, bc = _colors(points_palette, points_samples), _colors(skeleton_palette, skeleton_samples)
        if canvases.yuv:
            spaces = {(f.matrix, f.range) for f in canvases if f is not None}
            if len(spaces) != 1:
                raise ValueError("the YuvFrames of one draw_poses call share one matrix and range (the colours are converted once)")
            (matrix, range_), = spaces
            pc, bc = bgr_to_yuv_colors(pc, matrix, range_), bgr_to_yuv_colors(bc, matrix, range_)
        index = (None if ids is None else ids.ctypes.data) if ids_dev is None else ids_dev.data_ptr()
        self._launch("hrn_draw_poses" if ids_dev is None else "hrn_draw_poses_ids_dev", table, len(items), pts.data_ptr(), n, joints,
                     None if fi is None else fi.ctypes.data, skel.ctypes.data if len(skel) else None, len(skel), pc.ctypes.data, len(pc),
                     bc.ctypes.data, len(bc), index, 0 if radius is None else int(radius), int(thickness), float(confidence_threshold))
        return canvases[0] if single else list(canvases)

    def draw_labels(self, frames, boxes, person_ids=None, scores=None, frame_index=None, palette="Set2", samples: int = 8,  # noqa: A002
                    text_colors=None, scale: Optional[int] = None, thickness: int = 2):
        """Every person's box, id and score drawn beside it, on the GPU (``hrn_draw_labels_dev``): the outline of ``boxes[i]``, and
        above its top-left corner (inside it where there is no room above) a plate in the person's colour with the decimal digits
        of ``person_ids[i]`` and of the score as a percentage -- formed, laid out and rasterised on the device in two launches,
        with no host read: ids, boxes and scores are used where ``PersonTracker.update`` / ``predict_frame`` left them.  The
        shapes are the integer definition of include/hrnet_mi355.h (5 x 7 dot-matrix digits); equality with cv2.putText is not
        claimed.  Call it after ``draw_poses``: later drawing lies on top.

        ``frames``: as in ``draw_poses`` -- a BGR tensor or array (rows may be strided), a ``YuvFrame``, or a list of either kind
        with None for frames nobody is on; frames on the engine's GPU are drawn IN PLACE and returned, host frames are uploaded.
        ``boxes``: (n, 4) or (4,) int32 (x1, y1, x2, y2); a person whose box is (0, 0, 0, 0) or degenerate is not drawn.
        ``person_ids``: n int32 or None (no id is printed, colour index i; a negative id prints nothing); ``scores``: n float32 or
        None, possibly a strided view such as ``dets[:, 4]``; tensors on the engine's GPU stay there, anything else is uploaded.
        ``frame_index``: n frame numbers when there are several frames.  ``palette``: the people's colours, a matplotlib name or
        (C, 3) uint8 BGR (``person_ids[i] % C``, as the bones of ``draw_poses``); ``text_colors``: (C, 3) uint8 BGR, default black
        or white per colour by its luma ``(114 B + 587 G + 299 R) / 1000 >= 128``; both are converted with ``bgr_to_yuv_colors``
        for ``YuvFrame``s.  ``scale``: pixels per glyph dot, 1..16 (default ``max(1, min(H, W) // 360)`` per frame, at most 16);
        ``thickness``: of the outline, 0..16 (0: none)."""
        single = not isinstance(frames, (list, tuple))
        items = [frames] if single else list(frames)
        if not items:
            raise ValueError("draw_labels needs at least one frame")
        dev = self.torch_device
        canvases = Frames.canvases(items, dev)
        table = canvases.table(kind=_lib.CanvasC)
        if not isinstance(boxes, torch.Tensor):
            boxes = np.asarray(boxes)
        if (boxes.is_floating_point() or boxes.dtype == torch.bool) if isinstance(boxes, torch.Tensor) else boxes.dtype.kind not in "iu":
            raise ValueError("boxes must be integers (the int32 boxes predict_frame / PersonTracker.update return)")
        boxes = as_tensor(boxes, np.int32)
        if boxes.dim() == 1:
            boxes = boxes.unsqueeze(0)
        if boxes.dim() != 2 or boxes.shape[1] != 4:
            raise ValueError("boxes must be (4,) or (n, 4) (x1, y1, x2, y2)")
        boxes = device_tensor(boxes, dev, torch.int32)
        n = int(boxes.shape[0])

        def per_person(x, dtype, what):
            x = as_tensor(x, NUMPY_DTYPES[dtype]).reshape(-1)
            if len(x) != n:
                raise ValueError("%s must have one entry per person: %d for %d people" % (what, len(x), n))
            return x.to(dev, dtype=dtype, non_blocking=True)

        ids = None if person_ids is None else per_person(person_ids, torch.int32, "person_ids").contiguous()
        stride = 1
        if scores is not None:
            scores = per_person(scores, torch.float32, "scores")     # a view such as dets[:, 4] is read where it lies
            if n > 1 and scores.stride(0) < 1:
                scores = scores.contiguous()
            stride = int(scores.stride(0)) if n > 1 else 1
        fi = None
        if frame_index is not None:
            fi = np.ascontiguousarray(np.asarray(frame_index, dtype=np.int32).reshape(-1))
            if len(fi) != n:
                raise ValueError("frame_index must have one entry per person: %d for %d people" % (len(fi), n))
        elif len(items) != 1:
            raise ValueError("several frames need frame_index: which frame each person is drawn on")
        colours = _colors(palette, samples)
        if text_colors is None:   # black on a light colour, white on a dark one: by the BGR luma, before any YUV conversion
            wide = colours.astype(np.int64)
            luma = (114 * wide[:, 0] + 587 * wide[:, 1] + 299 * wide[:, 2]) // 1000
            text = np.where((luma >= 128)[:, None], np.uint8(0), np.uint8(255)).repeat(3, 1).astype(np.uint8)
        else:
            text = _colors(text_colors, 0)
            if len(text) != len(colours):
                raise ValueError("text_colors must have one colour per palette entry: %d for %d" % (len(text), len(colours)))
        text = np.ascontiguousarray(text)
        if canvases.yuv:
            spaces = {(f.matrix, f.range) for f in canvases if f is not None}
            if len(spaces) != 1:
                raise ValueError("the YuvFrames of one draw_labels call share one matrix and range (the colours are converted once)")
            (matrix, range_), = spaces
            colours, text = bgr_to_yuv_colors(colours, matrix, range_), bgr_to_yuv_colors(text, matrix, range_)
        self._launch("hrn_draw_labels_dev", table, len(items), boxes.data_ptr() if n else None, None if ids is None else ids.data_ptr(),
                     None if scores is None else scores.data_ptr(), stride, n, None if fi is None else fi.ctypes.data,
                     colours.ctypes.data, text.ctypes.data, len(colours), 0 if scale is None else int(scale), int(thickness))
        return canvases[0] if single else list(canvases)

    def draw_heatmaps(self, frames, heatmaps, boxes, frame_index=None, joints=None, colormap="jet", alpha=0.6, alpha_mode: str = "value",
                      vmin: float = 0.0, vmax: float = 1.0, cutoff=0.1, matrix: Optional[str] = None, range: Optional[str] = None):  # noqa: A002
        """What the network sees, on the frame, on the GPU (``hrn_draw_heatmaps_dev``): for every person the maximum of its
        heat-maps over ``joints``, stretched over the person's box as the decode places it (a peak lies under the disc
        ``draw_poses`` draws for it), coloured through ``colormap`` and blended into the frame; where boxes overlap the larger
        value shows.  Two launches whatever the number of frames and people; maps, boxes and frames are used where
        ``predict_frame(..., return_heatmaps=True)`` / ``track_frame`` left them.  The arithmetic is the integer definition of
        include/hrnet_mi355.h; equality with cv2.resize / applyColorMap / addWeighted is not claimed.  Call it before
        ``draw_poses``: later drawing lies on top.

        ``frames``: as in ``draw_poses`` -- a BGR tensor or array (rows may be strided), a ``YuvFrame`` (``"nv12"`` / ``"i420"``), or
        a list of either kind with None for frames nobody is on; frames on the engine's GPU are drawn IN PLACE and returned, host
        frames are uploaded.  ``heatmaps``: (n, J, h, w) or (J, h, w) float32; ``boxes``: (n, 4) or (4,) integer (x1, y1, x2, y2), a
        tensor on the device or the numpy boxes ``predict_frame`` returns; a degenerate box is skipped.  ``frame_index``: n frame
        numbers when there are several frames.  ``joints``: the indices that take part (default all; this package knows no joint
        names).  ``colormap``: a ``heat_colormap`` name or a (256, 3) uint8 BGR table -- converted with ``bgr_to_yuv_colors`` for
        ``YuvFrame``s, by the frames' own matrix and range unless ``matrix`` / ``range`` name another.  ``vmin`` / ``vmax``: the
        map values shown as 0 and 255.  ``alpha``, ``cutoff``: floats are mapped to 0..255 by ``round(255 x)``, integers are taken
        as they are; ``alpha_mode``: ``"const"`` blends every shown pixel with ``alpha``, ``"value"`` with ``alpha`` times its value;
        a pixel below ``cutoff`` is left alone.  For flip-TTA, pass ``predict_flip_tta``'s averaged maps."""
        single = not isinstance(frames, (list, tuple))
        items = [frames] if single else list(frames)
        if not items:
            raise ValueError("draw_heatmaps needs at least one frame")
        dev = self.torch_device
        canvases = Frames.canvases(items, dev)
        table = canvases.table(kind=_lib.CanvasC)
        maps = as_tensor(heatmaps, np.float32)
        if maps.dim() == 3:
            maps = maps.unsqueeze(0)
        if maps.dim() != 4 or min(maps.shape[1:]) < 1:
            raise ValueError("heatmaps must be (J, h, w) or (n, J, h, w)")
        maps = device_tensor(maps, dev, torch.float32)
        n, J, hq, wq = (int(v) for v in maps.shape)
        if not isinstance(boxes, torch.Tensor):
            boxes = np.asarray(boxes)
        if (boxes.is_floating_point() or boxes.dtype == torch.bool) if isinstance(boxes, torch.Tensor) else boxes.dtype.kind not in "iu":
            raise ValueError("boxes must be integers (the int32 boxes predict_frame / PersonTracker.update return)")
        boxes = as_tensor(boxes, np.int32)
        if boxes.dim() == 1:
            boxes = boxes.unsqueeze(0)
        if boxes.dim() != 2 or boxes.shape[1] != 4 or int(boxes.shape[0]) != n:
            raise ValueError("boxes must be (n, 4) (x1, y1, x2, y2), one row per person: %s for %d people" % (tuple(boxes.shape), n))
        boxes = device_tensor(boxes, dev, torch.int32)
        fi = None
        if frame_index is not None:
            fi = np.ascontiguousarray(np.asarray(frame_index, dtype=np.int32).reshape(-1))
            if len(fi) != n:
                raise ValueError("frame_index must have one entry per person: %d for %d people" % (len(fi), n))
        elif len(items) != 1:
            raise ValueError("several frames need frame_index: which frame each person is drawn on")
        mask, lut, a, mode, lo, hi, cut = heat_arguments(J, joints, colormap, alpha, alpha_mode, vmin, vmax, cutoff)
        if canvases.yuv:
            spaces = {(matrix or f.matrix, range or f.range) for f in canvases if f is not None}
            if len(spaces) != 1:
                raise ValueError("the YuvFrames of one draw_heatmaps call share one matrix and range (the table is converted once)")
            (matrix_, range_), = spaces
            lut = bgr_to_yuv_colors(lut, matrix_, range_)
        self._launch("hrn_draw_heatmaps_dev", table, len(items), maps.data_ptr() if n else None, boxes.data_ptr() if n else None, n, J, hq, wq,
                     None if fi is None else fi.ctypes.data, None if mask is None else mask.ctypes.data, lo, hi, lut.ctypes.data, a, mode, cut)
        return canvases[0] if single else list(canvases)

    def mosaic(self, frames, pts=None, boxes=None, joints=None, frame_index=None, confidence_threshold: float = 0.5, scale=(1, 1),
               min_half: Optional[int] = None, cell: Optional[int] = None, return_status: bool = False):
        """Hide people on the frame, on the GPU (``hrn_mosaic_dev``): a square around the chosen joints of every person -- for faces
        ``joints=COCO_HEAD_JOINTS`` -- or the given ``boxes`` is pixelated IN PLACE: every cell of the frame's ``cell`` x ``cell``
        grid that the square touches takes the mean of its own pixels, per channel.  Two launches whatever the number of frames
        and people; joints, boxes and frames are used where ``predict_frame`` / ``track_frame`` left them.  The arithmetic is the
        integer definition of include/hrnet_mi355.h; equality with cv2.blur or a resize down and up is not claimed.  The result
        depends on the set of touched cells alone -- not on the order of the people or on overlaps -- and a second identical call
        changes nothing.  A mosaic with small cells is NOT irreversible anonymisation: choose ``cell`` for the footage, and mind
        that a face the network does not find is not hidden.  Call it BEFORE ``draw_heatmaps`` / ``draw_poses`` / ``draw_labels``:
        later drawing lies on top.

        ``frames``: as in ``draw_poses`` -- a BGR tensor or array (rows may be strided), a ``YuvFrame`` (``"nv12"`` / ``"i420"``), or
        a list of either kind with None for frames nobody is on; frames on the engine's GPU are changed IN PLACE and returned, host
        frames are uploaded and the device copy is returned.  Exactly one of ``pts``: (n, J, 3) or (J, 3) (y, x, confidence), and
        ``boxes``: (n, 4) or (4,) integer (x1, y1, x2, y2); a degenerate box hides nothing.  ``joints``: the indices the square
        is put around (default all: the whole person); a joint counts when its confidence is above ``confidence_threshold``.
        ``frame_index``: n frame numbers when there are several frames.  ``scale``: (numerator, denominator), each 1..64: the
        square's half side is the extent of the chosen joints times ``scale``, rounded up (1 / 1: twice the ear-to-ear width of a
        frontal face).  ``min_half``: the least half side, 1..4096 (default: a sixteenth of the extent of all the person's joints,
        rounded up, so that a face in profile is not a dot).  ``cell``: 2, 4, 8, 16 or 32 (default per frame: 8 at 720p, 16 at
        1080p, 32 at 2160p).  ``return_status``: also return an (n,) int32 tensor on the device -- 0 hidden, 1 no region (no
        chosen joint counts, or a degenerate box), 2 the region lies outside the frame."""
        single = not isinstance(frames, (list, tuple))
        items = [frames] if single else list(frames)
        if not items:
            raise ValueError("mosaic needs at least one frame")
        if (pts is None) == (boxes is None):
            raise ValueError("mosaic takes pts or boxes: exactly one of them")
        dev = self.torch_device
        canvases = Frames.canvases(items, dev)
        table = canvases.table(kind=_lib.CanvasC)
        J = None
        if pts is not None:
            pts = as_tensor(pts, np.float32)
            if pts.dim() == 2:
                pts = pts.unsqueeze(0)
            if pts.dim() != 3 or pts.shape[2] != 3 or pts.shape[1] < 1:
                raise ValueError("pts must be (J, 3) or (n, J, 3) (y, x, confidence)")
            pts = device_tensor(pts, dev, torch.float32)
            n, J = int(pts.shape[0]), int(pts.shape[1])
        else:
            if not isinstance(boxes, torch.Tensor):
                boxes = np.asarray(boxes)
            if (boxes.is_floating_point() or boxes.dtype == torch.bool) if isinstance(boxes, torch.Tensor) else boxes.dtype.kind not in "iu":
                raise ValueError("boxes must be integers (the int32 boxes predict_frame / PersonTracker.update return)")
            boxes = as_tensor(boxes, np.int32)
            if boxes.dim() == 1:
                boxes = boxes.unsqueeze(0)
            if boxes.dim() != 2 or boxes.shape[1] != 4:
                raise ValueError("boxes must be (4,) or (n, 4) (x1, y1, x2, y2)")
            boxes = device_tensor(boxes, dev, torch.int32)
            n = int(boxes.shape[0])
        fi = None
        if frame_index is not None:
            fi = np.ascontiguousarray(np.asarray(frame_index, dtype=np.int32).reshape(-1))
            if len(fi) != n:
                raise ValueError("frame_index must have one entry per person: %d for %d people" % (len(fi), n))
        elif len(items) != 1:
            raise ValueError("several frames need frame_index: which frame each person is on")
        idx, num, den, half, size = mosaic_arguments(J, joints, scale, min_half, cell)
        status = torch.empty((n,), dtype=torch.int32, device=dev) if return_status else None
        self._launch("hrn_mosaic_dev", table, len(items), pts.data_ptr() if J is not None and n else None, n, J or 0,
                     None if idx is None else idx.ctypes.data, 0 if idx is None else len(idx), boxes.data_ptr() if J is None and n else None,
                     None if fi is None else fi.ctypes.data, float(confidence_threshold), num, den, half, size,
                     status.data_ptr() if return_status and n else None)
        out = canvases[0] if single else list(canvases)
        return (out, status) if return_status else out

    def resize_frames(self, frames, interpolation: int = 2, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The single-person pre-path (``multiperson=False``, ``SimpleHRNet.py:213-222`` / ``:355-366``) on the GPU:
        ``cv2.resize(frame, (W, H), interpolation)`` + BGR -> RGB + ToTensor + Normalize for every frame.

        ``frames``: (Hf, Wf, 3) or (n, Hf, Wf, 3) uint8 BGR (host arrays are uploaded once); ``interpolation``: the
        ``cv2.INTER_*`` value -- 0 nearest, 1 linear, 2 cubic (the reference's default).  Returns (n, 3, H, W) float32 on the GPU
        (written into the first n entries of ``out`` when given: ``predict_stream`` keeps one such buffer per staging slot).
        Follows OpenCV's published generic 8-bit path; equality with a particular cv2 build is not pinned (include/hrnet_mi355.h)."""
        if interpolation not in (0, 1, 2):
            raise ValueError("interpolation must be cv2.INTER_NEAREST (0), cv2.INTER_LINEAR (1) or cv2.INTER_CUBIC (2)")
        frames = frame_stack(frames, crops=False).to(self.torch_device, non_blocking=True).contiguous()
        n, h, w = int(frames.shape[0]), *self.resolution
        if out is not None:
            if out.dtype != torch.float32 or out.device != self.torch_device or not out.is_contiguous() or \
                    out.dim() != 4 or out.shape[0] < n or tuple(out.shape[1:]) != (3, h, w):
                raise ValueError("out must be a contiguous (>= %d, 3, %d, %d) float32 tensor on %s" % (n, h, w, self.torch_device))
            images = out[:n]
        else:
            images = torch.empty((n, 3, h, w), dtype=torch.float32, device=self.torch_device)
        if n:
            self._launch("hrn_resize_frames", frames.data_ptr(), n, int(frames.shape[1]), int(frames.shape[2]), int(interpolation),
                         images.data_ptr())
        return images

    def warp_crops(self, frames, centers=None, scales=None, rotations=None, frame_index=None, pixel_std=200, matrices=None) -> torch.Tensor:
        """The evaluation pre-path (``datasets/COCO.py:290-304``, ``misc/utils.py:99-107``) on the GPU: per person
        ``cv2.warpAffine(image, get_affine_transform(center, scale, pixel_std, rot, (W, H)), (W, H), flags=cv2.INTER_LINEAR)``
        + ToTensor + Normalize.

        ``frames``: (Hf, Wf, 3) or (F, Hf, Wf, 3) uint8 BGR (host arrays are uploaded once); ``centers`` (n, 2) / ``scales``
        (n, 2) or (n,) as the dataset provides them (``postproc.box_to_center_scale``), ``rotations`` (n,) in degrees -- or
        explicit forward 2x3 ``matrices`` (n, 2, 3), frame -> crop.  ``frame_index`` (n,): the frame of each crop; None = crop i
        reads frame i (F == n) or the one frame (F == 1).  Returns (n, 3, H, W) float32 on the GPU, for any n.
        Follows warpAffine's 8-bit integer path (include/hrnet_mi355.h); equality with a particular cv2 build is not pinned."""
        frames = frame_stack(frames)
        h, w = self.resolution
        m, fi = _warp_arguments(int(frames.shape[0]), (w, h), centers, scales, rotations, frame_index, pixel_std, matrices)
        frames = frames.to(self.torch_device, non_blocking=True).contiguous()
        n = len(m)
        images = torch.empty((n, 3, h, w), dtype=torch.float32, device=self.torch_device)
        if n:
            self._launch("hrn_warp_crops", frames.data_ptr(), int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2]),
                         fi.ctypes.data, m.ctypes.data, n, images.data_ptr())
        return images

    def decode_eval(self, images: torch.Tensor, flip_pairs, flip: bool = True, post_processing: Union[bool, str] = True):
        """heat-maps + evaluation decode of a crop batch: ``predict_flip_tta`` (``flip``), or one plain pass followed by the same
        decode -- get_max_preds (coordinates zeroed where the maximum is not positive), then the quarter-pixel or DARK offset.
        Returns ``(heatmaps, preds (n,J,2) = (x, y) in heat-map pixels, maxvals (n,J,1))``."""
        if flip:
            return self.predict_flip_tta(images, flip_pairs, post_processing=post_processing)
        if isinstance(post_processing, str) and post_processing != "dark":
            raise ValueError("post_processing must be True, False or 'dark', got %r" % (post_processing,))
        h, w = self.resolution
        n = int(images.shape[0])
        cells = torch.tensor([[0, 0, w // 4, h // 4]] * n, dtype=torch.float32).reshape(n, 4)   # pts come out in heat-map cells
        hm, pts = self.predict_crops(images, cells, return_heatmaps=True)
        maxvals = pts[:, :, 2:3].contiguous()
        preds = torch.where(maxvals > 0, pts[:, :, [1, 0]], torch.zeros_like(maxvals))
        if post_processing:
            preds = self.refine_coords(hm, preds, "dark" if post_processing == "dark" else "quarter")
        return hm, preds, maxvals

    def predict_eval(self, frames, centers, scales, flip_pairs, frame_index=None, flip: bool = True,
                     post_processing: Union[bool, str] = True, pixel_std=200):
        """One batch of ``Test._test`` (``testing/Test.py:124-140``) + ``get_final_preds`` from uint8 images:
        ``warp_crops`` -> ``predict_flip_tta`` (``flip=False``: one plain pass and the same decode) -> ``postproc.final_preds``.
        ``frames`` / ``centers`` / ``scales`` / ``frame_index`` as in ``warp_crops`` (no rotation at test time);
        ``post_processing`` as in ``predict_flip_tta``.  Returns ``(preds (n,J,2) float32 numpy = (x, y) in image pixels,
        maxvals (n,J,1) on the GPU, heatmaps (n,J,H/4,W/4) on the GPU)``."""
        from . import postproc

        images = self.warp_crops(frames, centers, scales, frame_index=frame_index, pixel_std=pixel_std)
        hm, preds, maxvals = self.decode_eval(images, flip_pairs, flip=flip, post_processing=post_processing)
        h, w = self.resolution
        return postproc.final_preds(preds, np.asarray(centers), np.asarray(scales), pixel_std, (w // 4, h // 4)), maxvals, hm

    # -- scoring an evaluation batch (testing/Test.py:141-157) ---------------------------------------
    def _joint_arguments(self, joints, visibility, joints_weight):
        """host arguments of the analytic target source: ``(joints (n,J,2) float64, visibility (n,J) float32, joints_weight (J,)
        float32 or None)``; ``visibility`` may be (n,J) or the dataset's (n,J,k), whose column 0 is read (``COCO.py:467``)"""
        J = self.nof_joints
        jt = host_array(joints, np.float64)
        if jt.ndim != 3 or jt.shape[1] != J or jt.shape[2] < 2:
            raise ValueError("joints must be (n, %d, 2), got %s" % (J, jt.shape))
        jt = np.ascontiguousarray(jt[:, :, :2])
        vis = host_array(visibility, np.float32)
        if vis.ndim == 3:
            vis = vis[:, :, 0]
        if vis.shape != jt.shape[:2]:
            raise ValueError("visibility must be (n, %d) or (n, %d, k), got %s" % (J, J, vis.shape))
        vis = np.ascontiguousarray(vis)
        jw = None
        if joints_weight is not None:
            jw = np.ascontiguousarray(np.asarray(joints_weight, dtype=np.float32).reshape(-1))
            if jw.shape != (J,):
                raise ValueError("joints_weight must hold %d values" % J)
        return jt, vis, jw

    def generate_targets(self, joints, visibility, sigma=2, joints_weight=None):
        """``_generate_target`` (``datasets/COCO.py:460-515``) for a batch, on the GPU: ``joints`` (n,J,2) in crop pixels (float64,
        ``postproc.joints_to_crop``), ``visibility`` (n,J) or (n,J,k).  Returns ``(targets (n,J,H/4,W/4) float32 on the GPU,
        target_weight (n,J,1) float32 numpy)``.  The Gaussian table is the library's (include/hrnet_mi355.h)."""
        jt, vis, jw = self._joint_arguments(joints, visibility, joints_weight)
        n, (h, w) = len(jt), self.resolution
        targets = torch.empty((n, self.nof_joints, h // 4, w // 4), dtype=torch.float32, device=self.torch_device)
        tw = np.empty((n, self.nof_joints, 1), np.float32)
        self._launch("hrn_generate_targets", jt.ctypes.data, vis.ctypes.data, None if jw is None else jw.ctypes.data, n, float(sigma),
                     targets.data_ptr(), tw.ctypes.data)
        return targets, tw

    def score_heatmaps(self, heatmaps, joints=None, visibility=None, targets=None, target_weight=None, sigma=2, joints_weight=None,
                       thr: float = 0.5, topk: int = 0) -> Dict:
        """Loss and PCK of a batch of heat-maps against its ground truth (``testing/Test.py:141-157``), on the GPU.

        Target source: ``joints`` (n,J,2) in crop pixels + ``visibility`` [+ ``joints_weight``] + ``sigma`` -- the Gaussian targets
        are evaluated inside the kernel, nothing of target size exists -- or ``targets`` (n,J,h,w) + ``target_weight`` (n,J[,1])
        as the dataset returns them (any tensor of that shape: another engine's heat-maps with weights of one).
        Returns a dict of tensors on the GPU (stream-ordered, nothing is synchronised):
        ``loss`` = ``JointsMSELoss``, ``loss_ohkm`` = ``JointsOHKMMSELoss(topk)`` (NaN for ``topk=0``), both float64 scalars;
        ``accs`` (J,), ``avg_acc`` (), ``cnt`` () int32, ``joints_preds`` / ``joints_target`` (n,J,2) = the five values of
        ``evaluate_pck_accuracy(output, target, thr=thr)``; ``dists`` (J,n), ``maxvals`` (n,J,1), ``map_loss`` (n,J) float64."""
        h, w = self.resolution
        J, dev = self.nof_joints, self.torch_device
        hm = torch.as_tensor(heatmaps).to(dev, torch.float32).contiguous()
        n = int(hm.shape[0]) if hm.dim() == 4 else -1
        if tuple(hm.shape) != (n, J, h // 4, w // 4):
            raise ValueError("heatmaps must be (n,%d,%d,%d), got %s" % (J, h // 4, w // 4, tuple(hm.shape)))
        if (joints is None) == (targets is None):
            raise ValueError("give either joints and visibility, or targets and target_weight")
        jt = vis = jw = tg = tw = None
        if joints is not None:
            if visibility is None or target_weight is not None:
                raise ValueError("joints come with visibility and without target_weight")
            jt, vis, jw = self._joint_arguments(joints, visibility, joints_weight)
            if len(jt) != n:
                raise ValueError("%d heat-maps but %d persons" % (n, len(jt)))
        else:
            if target_weight is None or visibility is not None or joints_weight is not None:
                raise ValueError("targets come with target_weight and without visibility / joints_weight")
            tg = torch.as_tensor(targets).to(dev, torch.float32).contiguous()
            tw = np.ascontiguousarray(host_array(target_weight, np.float32).reshape(-1))
            if tuple(tg.shape) != tuple(hm.shape) or tw.size != n * J:
                raise ValueError("targets must have the heat-maps' shape and target_weight n*J entries")
        f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
        t = {"loss_mse": torch.empty((), **f64), "loss_ohkm": torch.empty((), **f64), "avg_acc": torch.empty((), **f32),
             "cnt": torch.empty((), dtype=torch.int32, device=dev), "acc": torch.empty((J,), **f32), "dists": torch.empty((J, n), **f32),
             "map_loss": torch.empty((n, J), **f64), "preds": torch.empty((n, J, 2), **f32), "target_preds": torch.empty((n, J, 2), **f32),
             "maxvals": torch.empty((n, J, 1), **f32)}
        out = _lib.ScoreOut(**{k: v.data_ptr() for k, v in t.items()})

        def ptr(a):
            return None if a is None else a.ctypes.data

        self._launch("hrn_score_heatmaps", hm.data_ptr(), n, None if tg is None else tg.data_ptr(), ptr(jt), ptr(vis), ptr(jw),
                     float(sigma), ptr(tw), float(thr), int(topk), ctypes.byref(out))
        return {"loss": t["loss_mse"], "loss_ohkm": t["loss_ohkm"], "accs": t["acc"], "avg_acc": t["avg_acc"], "cnt": t["cnt"],
                "joints_preds": t["preds"], "joints_target": t["target_preds"], "dists": t["dists"], "maxvals": t["maxvals"],
                "map_loss": t["map_loss"]}

    def score_eval(self, frames, centers, scales, flip_pairs, gt_joints, gt_visibility, frame_index=None, flip: bool = True,
                   post_processing: Union[bool, str] = True, pixel_std=200, sigma=2, joints_weight=None, thr: float = 0.5, topk: int = 0):
        """``predict_eval`` plus the score of its heat-maps against the ground truth: one batch of ``Test._test``
        (``testing/Test.py:124-157``) from uint8 images and the annotations.  ``gt_joints`` (n,J,2) in IMAGE pixels and
        ``gt_visibility`` (n,J) or (n,J,k) as the dataset holds them; the joints are taken to crop pixels by the matrices the crops
        are cut with (``postproc.joints_to_crop``).  Returns ``(predict_eval's tuple, score_heatmaps' dict)``."""
        from . import postproc

        h, w = self.resolution
        c, s = np.asarray(centers), np.asarray(scales)
        m = np.stack([postproc.affine_matrix(c[i], s[i], pixel_std, 0, (w, h)) for i in range(len(c))]) if len(c) else np.zeros((0, 2, 3))
        crop_joints = postproc.joints_to_crop(gt_joints, gt_visibility, m)
        self._joint_arguments(crop_joints, gt_visibility, joints_weight)   # argument errors before the network runs
        out = self.predict_eval(frames, centers, scales, flip_pairs, frame_index=frame_index, flip=flip, post_processing=post_processing,
                                pixel_std=pixel_std)
        score = self.score_heatmaps(out[2], joints=crop_joints, visibility=gt_visibility, sigma=sigma, joints_weight=joints_weight,
                                    thr=thr, topk=topk)
        return out, score

    def predict_frame(self, frame, detections, return_heatmaps: bool = False, variant: str = "pad", refine: Optional[str] = None):
        """pre-path + model + decode for one frame: what ``SimpleHRNet._predict_single`` does after the detector.
        Returns ``(boxes (P,4) int32 numpy, pts (P,J,3) on the GPU[, heatmaps])``.  ``refine``: as in ``predict_crops``."""
        refine_code(refine)
        images, boxes, boxes_dev = self.preprocess_frame(frame, detections, variant)
        out = self.predict_crops(images, boxes_dev, return_heatmaps=return_heatmaps, refine=refine)
        if return_heatmaps:
            return boxes, out[1], out[0]
        return boxes, out

    # -- the tracking link: between two detector runs the next frame's crops are cut from the previous frame's joints ------------
    def boxes_from_poses(self, pts, frame_hw, threshold: float = 0.5, min_joints: int = 3, scale: float = 1.25,
                         min_side: float = 0.0) -> torch.Tensor:
        """``postproc.pose_boxes`` on the GPU (``hrn_boxes_from_poses``: one launch, one wave per person, no synchronisation):
        ``pts`` (n, J, 3) float32 ``(y, x, confidence)`` where the decode left them (any J up to 256; a host array is uploaded),
        ``frame_hw`` = (height, width) for everybody or (n, 2), on the host.  Returns (n, 5) float32 detection rows
        ``(x1, y1, x2, y2, score)`` on the GPU, bit for bit ``pose_boxes``'s; five zeros where fewer than ``min_joints`` joints
        have ``confidence > threshold``."""
        from .postproc import _frame_sizes

        pts = as_tensor(pts, np.float32)
        if pts.dim() != 3 or pts.shape[2] != 3:
            raise ValueError("pts must be (n, J, 3), got %s" % (tuple(pts.shape),))
        pts = device_tensor(pts, self.torch_device, torch.float32)
        n, J = int(pts.shape[0]), int(pts.shape[1])
        hw, per_person = _frame_sizes(frame_hw, n)
        dets = torch.empty((n, 5), dtype=torch.float32, device=self.torch_device)
        self._launch("hrn_boxes_from_poses", pts.data_ptr(), n, J, hw.ctypes.data, per_person, ctypes.c_float(threshold),
                     int(min_joints), ctypes.c_double(scale), ctypes.c_double(min_side), dets.data_ptr())
        return dets

    def _tracked_frames(self, frames, frame_index, n: int):
        """``frames`` / ``frame_index`` of ``preprocess_frames_dev`` / ``track_frame`` as (``Frames`` on the device, int32 index or None)"""
        frames = self._device_frames(frames, one=True)
        if frame_index is None:
            if len(frames) != 1:
                raise ValueError("%d frames need a frame_index (one entry per person)" % len(frames))
            return frames, None
        index = np.ascontiguousarray(host_array(frame_index, np.int32).reshape(-1))
        if len(index) != n:
            raise ValueError("frame_index has %d entries for %d people" % (len(index), n))
        if len(index) and (index.min() < 0 or index.max() >= len(frames)):
            raise ValueError("frame_index must lie in [0, %d)" % len(frames))
        if any(frames[f] is None for f in set(index.tolist())):
            raise ValueError("a frame somebody is cut from is None")
        return frames, index

    def _preprocess_dev(self, frames: Frames, dets_dev: torch.Tensor, index, variant: str):
        """``hrn_preprocess_frames_dev`` / ``_yuv_dev`` over device frames (the ``Frames`` ``_tracked_frames`` made)"""
        crop = crop_code(variant)
        if dets_dev.dim() != 2 or dets_dev.shape[1] < 4:
            raise ValueError("detections must be (P, >=4)")
        dets_dev = device_tensor(dets_dev, self.torch_device, torch.float32)
        n = int(dets_dev.shape[0])
        h, w = self.resolution
        dev = self.torch_device
        images = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
        boxes_dev = torch.empty((n, 4), dtype=torch.int32, device=dev)
        status_dev = torch.empty((n,), dtype=torch.int32, device=dev)
        if n:
            self._launch("hrn_preprocess_frames%s_dev" % ("_yuv" if frames.yuv else ""), frames.table(), len(frames), dets_dev.data_ptr(),
                         int(dets_dev.shape[1]), None if index is None else index.ctypes.data, n, crop, images.data_ptr(),
                         boxes_dev.data_ptr(), status_dev.data_ptr())
        return images, boxes_dev, status_dev

    def preprocess_frames_dev(self, frames, dets_dev, frame_index=None, variant: str = "pad"):
        """The crop pre-path with the detections ON THE GPU (``hrn_preprocess_frames_dev``): ``preprocess_frames`` without a host
        read of the boxes, for detections a kernel made -- ``boxes_from_poses``, or a detector that leaves its rows on the device.

        ``frames``: one frame ((Hf, Wf, 3) uint8 BGR or a ``YuvFrame``), or a stack / sequence of frames as in
        ``preprocess_frames`` together with ``frame_index`` (one frame number per person, on the host: who belongs to which
        frame is known without reading the device); ``dets_dev``: (P, >=4) float32, columns 0..3 = x1, y1, x2, y2 (a host array is
        uploaded).  Returns ``(images (P, 3, H, W) float32, boxes (P, 4) int32, status (P,) int32)``, all on the GPU, nothing
        synchronised.  ``status`` 0: images and boxes are ``preprocess_frames``'s, bit for bit.  Otherwise the person's box is
        zero and its crop all padding (1 degenerate, 2 starts outside the frame, 3 degenerate after clamping, 4 padded crop too
        tall for the scratch, 5 a coordinate not finite or beyond 2^30: include/hrnet_mi355.h).  The scratch is sized for the
        tallest crop a box inside the frame can need: about 2.2 MB per person at 1080p / 384x288, kept by the engine."""
        dets_dev = as_tensor(dets_dev, np.float32)
        frames, index = self._tracked_frames(frames, frame_index, int(dets_dev.shape[0]))
        return self._preprocess_dev(frames, dets_dev, index, variant)

    def track_frame(self, frame, prev_pts, frame_index=None, variant: str = "pad", refine: Optional[str] = None,
                    return_heatmaps: bool = False, **box_args):
        """One frame of a video loop WITHOUT the detector: the people are cut from ``frame`` where their joints were in the
        previous frame -- ``boxes_from_poses(prev_pts)`` -> ``preprocess_frames_dev`` -> ``predict_crops``, device tensors in and
        out, stream-ordered, no synchronisation.  ``prev_pts``: (P, J, 3) as ``predict_frame`` / ``track_frame`` returned them;
        ``box_args``: ``threshold``, ``min_joints``, ``scale``, ``min_side`` of ``boxes_from_poses``.  Given a list of frames plus
        ``frame_index`` it is the clip form: the people of many streams in one call.
        Returns ``(boxes (P, 4) int32, pts (P, J, 3), status (P,) int32[, heatmaps])`` on the GPU.  A person whose ``status`` is
        not 0 (too few live joints, or all of them on one side of the frame) went through the pass as an all-padding crop: its
        ``pts`` mean nothing -- drop it, or run the detector again.  Equal, bit for bit, to downloading ``prev_pts``,
        ``postproc.pose_boxes`` and ``predict_frame`` with those host detections."""
        refine_code(refine)
        n = int(prev_pts.shape[0])
        frames, index = self._tracked_frames(frame, frame_index, n)
        sizes = frames.sizes()
        dets = self.boxes_from_poses(prev_pts, sizes[0] if index is None else sizes[index].reshape(n, 2), **box_args)
        images, boxes_dev, status_dev = self._preprocess_dev(frames, dets, index, variant)
        out = self.predict_crops(images, boxes_dev, return_heatmaps=return_heatmaps, refine=refine)
        if return_heatmaps:
            return boxes_dev, out[1], status_dev, out[0]
        return boxes_dev, out, status_dev

    # -- the detector link: the letterboxed detector tensor, and the detector's boxes back in frame coordinates --------------------
    LETTERBOX_FORMS = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.uint8: 3}   # include/hrnet_mi355.h: HRN_LB_*

    def detector_input(self, frames, size, style: str = "yolov3", dtype=torch.float32, order: str = "rgb", pad=None):
        """What the reference's detector wrappers do to a frame BEFORE their network, on the GPU (``hrn_letterbox_frames``: one
        launch for all frames, no scratch): ``letterbox`` (cv2.resize(INTER_LINEAR) + cv2.copyMakeBorder), BGR -> RGB, ``ToTensor``.

        ``frames``: one frame ((Hf, Wf, 3) uint8 BGR or a ``YuvFrame``), or a stack / sequence of frames of any sizes as in
        ``preprocess_frames`` (host frames are uploaded); ``size``: the detector's input side, or (height, width) for
        ``style="yolov5"``; ``style``: ``"yolov3"`` = ``letterbox(mode='square')`` with border 128 (the wrapper's 127.5 as cv2
        saturates it), ``"yolov5"`` = ``letterbox(auto=False, scaleFill=False)`` with border 114; ``pad``: one value or three, in
        output channel order; ``order``: ``"rgb"`` (what both wrappers feed their network) or ``"bgr"``; ``dtype``: float32 / float16 /
        bfloat16 give (n, 3, out_h, out_w) with values ``v / 255``, uint8 gives (n, out_h, out_w, 3).
        Returns ``(tensor on the GPU, geometry)``; ``geometry`` (``postproc.LetterboxGeometry``) is what ``detections_to_frame``
        takes.  Nothing is synchronised.  The resize is OpenCV's published 8-bit arithmetic, not pinned against a cv2 build
        (include/hrnet_mi355.h); a YUV frame gives, bit for bit, the tensor of its ``yuv_to_bgr`` conversion."""
        from .postproc import LETTERBOX_PAD, LETTERBOX_RULES, LetterboxGeometry, _letterbox_size

        out_h, out_w = _letterbox_size(size, style)
        if dtype not in self.LETTERBOX_FORMS:
            raise ValueError("dtype must be torch.float32, float16, bfloat16 or uint8, got %r" % (dtype,))
        if order not in ("rgb", "bgr"):
            raise ValueError("order must be 'rgb' or 'bgr', got %r" % (order,))
        fill = np.asarray(LETTERBOX_PAD[style] if pad is None else pad)
        if fill.size not in (1, 3) or (fill < 0).any() or (fill > 255).any() or (fill != np.round(fill)).any():
            raise ValueError("pad must be one or three integers in [0, 255], got %r" % (pad,))
        fill = np.ascontiguousarray(np.broadcast_to(fill.reshape(-1), (3,)).astype(np.uint8))
        frames = self._device_frames(frames, one=True)
        if not frames or any(f is None for f in frames):
            raise ValueError("detector_input needs at least one frame, and none of them None")
        n = len(frames)
        shape = (n, out_h, out_w, 3) if dtype == torch.uint8 else (n, 3, out_h, out_w)
        out = torch.empty(shape, dtype=dtype, device=self.torch_device)
        geometry = (_lib.Letterbox * n)()
        self._launch("hrn_letterbox_frames" + ("_yuv" if frames.yuv else ""), frames.table(), n, LETTERBOX_RULES[style], out_h, out_w,
                     fill.ctypes.data, 0 if order == "rgb" else 1, self.LETTERBOX_FORMS[dtype], out.data_ptr(), ctypes.addressof(geometry))
        return out, LetterboxGeometry(style, (out_h, out_w), frames.sizes(), geometry)

    def detections_to_frame(self, dets, geometry, counts=None, conf_thres=None, classes=None, compact: bool = True, conf_col: int = 4,
                            class_col: int = -1):
        """``postproc.detections_to_frame`` on the GPU (``hrn_detections_to_frame_dev``: one launch, one block per frame, no host
        read): what the reference's detector wrappers do AFTER their network and its NMS -- confidence and class filter, then the
        boxes back from letterbox to frame coordinates.  ``dets`` (n, >=5) float32 on the GPU (a host array is uploaded), the rows
        of frame p are ``counts[p]`` consecutive ones (host-known: the shapes of the detector's per-image tensors); the other
        arguments as in ``postproc.detections_to_frame``.  Returns ``(rows (n, stride), counts (P,) int32, status (n,) int32)`` on
        the GPU, bit for bit the host form's.  A row that is not kept is all zeros, which ``preprocess_frames_dev`` reports as
        status 1; ``rows[:, :4]`` can go there as it is."""
        from .postproc import detection_arguments

        dets = as_tensor(dets, np.float32)
        start, thres, col, ids, flags = detection_arguments(tuple(dets.shape), geometry, counts, conf_thres, classes, class_col, compact)
        dev = self.torch_device
        dets = device_tensor(dets, dev, torch.float32)
        n, P = int(dets.shape[0]), len(geometry)
        out = torch.empty_like(dets)
        kept = torch.empty((P,), dtype=torch.int32, device=dev)
        status = torch.empty((n,), dtype=torch.int32, device=dev)
        self._launch("hrn_detections_to_frame_dev", geometry.rule, dets.data_ptr(), int(dets.shape[1]), start.ctypes.data, P,
                     ctypes.addressof(geometry.table), geometry.frame_hw.ctypes.data, geometry.size[0], geometry.size[1], int(conf_col),
                     ctypes.c_float(thres), col, ids.ctypes.data, len(ids), flags, out.data_ptr(), kept.data_ptr(), status.data_ptr())
        return out, kept, status

    def detector_nms(self, pred, rule, conf_thres, iou_thres, max_det: int = 300, max_candidates: int = 4096, agnostic: bool = False):
        """``postproc.detector_nms`` on the GPU (``hrn_detector_nms_dev``: a scoring launch over the head's output and one block per
        image, no host read): the detector's own non-maximum suppression, the step between the detector network and
        ``detections_to_frame``.  ``pred`` (B, N, 5 + C) float32 or float16, the raw output of a YOLO head (rows ``cx, cy, w, h,
        obj, cls...``); a tensor on the engine's GPU is used where it lies, a host array is uploaded; the other arguments as in
        ``postproc.detector_nms``.  Returns ``(rows (B, max_det, 6 | 7) float32, counts (B,) int32, index (B, max_det) int32,
        status (B,) int32)`` on the GPU, bit for bit the host form's; ``rows.reshape(-1, F)`` with ``max_det`` rows per image can go
        to ``detections_to_frame`` as it is, whose confidence filter drops the zero rows (a positive ``conf_thres``).  Nothing is
        synchronised."""
        from .postproc import detector_nms_arguments

        pred = as_tensor(pred)
        if pred.dtype not in (torch.float16, torch.float32):
            pred = pred.to(torch.float32)
        dev = self.torch_device
        pred = device_tensor(pred, dev, pred.dtype)
        name = {torch.float32: "float32", torch.float16: "float16"}.get(pred.dtype, str(pred.dtype))
        B, N, C, dtype, code, flags, F = detector_nms_arguments(tuple(pred.shape), name, rule, max_det, max_candidates, agnostic)
        max_det, max_candidates = int(max_det), int(max_candidates)
        shape = (B, max(max_det, 0))
        rows = torch.empty(shape + (F,), dtype=torch.float32, device=dev)
        index = torch.empty(shape, dtype=torch.int32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        ptr = lambda t: None if t.numel() == 0 else t.data_ptr()   # noqa: E731 -- (an empty tensor has no address)
        self._launch("hrn_detector_nms_dev", ptr(pred), dtype, B, N, C, code, flags, float(conf_thres), float(iou_thres), max_candidates,
                     max_det, ptr(rows), ptr(index), ptr(counts), ptr(status))
        return rows, counts, index, status

    # -- frame rotation: a video stored sideways, upright without leaving the device -----------------------------------------------
    def rotate_frames(self, frames, rotation_code, out=None):
        """``cv2.rotate(frame, rotation_code)`` on the GPU (``hrn_rotate_frames``: ONE launch for all frames, no scratch) -- the
        first step of the reference's frame loops for a video with a rotation tag (``scripts/live-demo.py:102-103``).  A pure
        permutation of pixels: bit for bit ``np.rot90`` per plane (include/hrnet_mi355.h has the rule).

        ``frames``: one (H, W, 3) uint8 BGR frame, an (F, H, W, 3) stack, a sequence of frames of any sizes, or ``YuvFrame``(s);
        host frames are uploaded once, None entries pass through.  ``rotation_code``: 0 (90 degrees clockwise), 1 (180), 2 (90
        counter-clockwise) -- ``cv2.ROTATE_*``'s values, see ``rotation_code_from_degrees`` -- for every frame, or one per frame;
        None returns the resident frames unrotated.  Returns the rotated frames on the GPU in the shape they came in: a frame, a
        stack (its frames then turn alike: all by 180 degrees or none), or a list; a ``YuvFrame`` comes back as a ``YuvFrame``
        with swapped sides, its own format (8- or 10-bit), matrix and range, and no pitch padding.
        ``out``: destinations on the engine's GPU to write into instead (the same shape of argument; pitched BGR views and pitched
        ``YuvFrame``s are allowed; bytes of a row beyond its pixels keep their value); they are returned.  A destination may not
        be a source: in-place rotation is not offered.  Nothing is synchronised."""
        dev = self.torch_device
        if out is None and type(rotation_code) is int and 0 <= rotation_code <= 2:
            turned = self._rotate_one(frames, rotation_code, dev)
            if turned is not None:
                return turned
        single = isinstance(frames, YuvFrame) or (isinstance(frames, (torch.Tensor, np.ndarray)) and frames.ndim == 3)
        stack = not single and isinstance(frames, (torch.Tensor, np.ndarray)) and frames.ndim == 4
        if stack:   # uploaded here, in one copy: what comes back unrotated is this tensor
            frames = as_tensor(frames).to(dev, non_blocking=True).contiguous()
        src = Frames.resident(frames, dev, one=True, rows=True)
        if rotation_code is None:
            return src[0] if single else frames if stack else list(src)
        codes = rotation_codes(rotation_code, len(src))
        whole = None   # a stack's destination, as one tensor
        if out is None:
            if stack:
                if len({int(c) == 1 for c in codes}) > 1:
                    raise ValueError("the frames of a stack come back as a stack: they all turn by 180 degrees, or none does")
                h, w = (int(d) for d in src[0].shape[:2]) if len(src) else (0, 0)
                h, w = (h, w) if len(codes) and codes[0] == 1 else (w, h)
                whole = torch.empty((len(src), h, w, 3), dtype=torch.uint8, device=dev)
                dst = Frames([whole[k] for k in range(len(src))], False)
            else:
                dst = src.rotated(codes, dev)
        else:
            if stack and isinstance(out, torch.Tensor) and out.dim() == 4:
                whole, out = out, [out[k] for k in range(int(out.shape[0]))]
            items = [out] if single else list(out)
            if len(items) != len(src):
                raise ValueError("out has %d frames for %d" % (len(items), len(src)))
            for k, f in enumerate(items):
                if f is not None and (not isinstance(f, (torch.Tensor, YuvFrame)) or f.device != dev):
                    raise ValueError("out[%d] must lie on the engine's device %s: it is written where it is" % (k, dev))
            dst = Frames.canvases(items, dev)
            if dst.yuv != src.yuv and any(f is not None for f in src):
                raise ValueError("out must hold frames of the kind of `frames`: BGR tensors or YuvFrames")
        live = [k for k, f in enumerate(src) if f is not None]
        if any(dst[k] is None for k in live):
            raise ValueError("out has no destination for a frame that is there")
        if live:
            s_table = Frames([src[k] for k in live], src.yuv).table(kind=_lib.CanvasC)
            d_table = Frames([dst[k] for k in live], src.yuv).table(kind=_lib.CanvasC)
            picked = np.ascontiguousarray(codes[live])
            self._launch("hrn_rotate_frames", s_table, d_table, len(live), picked.ctypes.data)
        if single:
            return dst[0]
        return whole if whole is not None else [dst[k] if src[k] is not None else None for k in range(len(src))]

    def _rotate_one(self, frame, code: int, dev):
        """the lean path of ``rotate_frames`` -- ONE frame that lies on the engine's GPU, one code, a fresh destination: the call a
        video loop makes per frame, which is launch-bound, so the host side is what it costs.  None: not that case."""
        src, dst = self._rot_pair[0], self._rot_pair[1]
        if isinstance(frame, torch.Tensor):
            if frame.dim() != 3 or frame.device != dev or frame.dtype != torch.uint8 or frame.shape[2] != 3 or not _bgr_rows(frame):
                return None
            h, w = int(frame.shape[0]), int(frame.shape[1])
            if h < 1 or w < 1:
                return None
            rh, rw = (h, w) if code == 1 else (w, h)
            out = torch.empty((rh, rw, 3), dtype=torch.uint8, device=dev)
            src.y, src.height, src.width, src.pitch_y, src.format = frame.data_ptr(), h, w, max(int(frame.stride(0)), 3 * w), 0
            dst.y, dst.height, dst.width, dst.pitch_y, dst.format = out.data_ptr(), rh, rw, 3 * rw, 0
        elif isinstance(frame, YuvFrame) and frame.device == dev:
            rh, rw = (frame.height, frame.width) if code == 1 else (frame.width, frame.height)
            out = YuvFrame._trusted(torch.empty((rh * rw * 3 // 2 * frame.sample_bytes,), dtype=torch.uint8, device=dev), rh, rw, frame)
            frame._fill(src)
            out._fill(dst)
        else:
            return None
        if torch.cuda.current_device() != self.device_index:
            self._launch("hrn_rotate_frames", ctypes.byref(src), ctypes.byref(dst), 1, self._rot_code_ptr[code])
        else:   # already on the engine's device: no device context to enter and leave (the library selects its device itself)
            self._check(self._lib.hrn_rotate_frames(self._h, ctypes.byref(src), ctypes.byref(dst), 1, self._rot_code_ptr[code], self._stream()),
                        "hrn_rotate_frames")
        return out

    def rotate_people(self, pts=None, boxes=None, frame_hw=None, rotation_code=None):
        """``postproc.rotate_people`` on the GPU (``hrn_rotate_people_dev``: one launch, one thread per joint and per box, no host
        read): joints and boxes computed on one orientation of a frame, in the coordinates of the other.  ``pts`` (n, J, 3)
        float32 ``(y, x, confidence)`` and / or ``boxes`` (n, 4) int32 ``(x1, y1, x2, y2)`` where the engine left them (a host
        array is uploaded); ``frame_hw``: (height, width) of the SOURCE frame for everybody, or (n, 2); ``rotation_code``: one code
        or n.  Returns the rotated tensor on the GPU -- ``(pts, boxes)`` when both were given -- bit for bit the host form's.  The
        way back is code ``2 - c`` with the rotated frame's size."""
        from .postproc import rotate_people_arguments

        dev = self.torch_device
        if pts is not None:
            pts = as_tensor(pts, np.float32)
            if pts.dim() != 3 or pts.shape[2] != 3:
                raise ValueError("pts must be (n, J, 3), got %s" % (tuple(pts.shape),))
            pts = device_tensor(pts, dev, torch.float32)
        if boxes is not None:
            boxes = as_tensor(boxes, np.int32)
            if boxes.dim() != 2 or boxes.shape[1] != 4:
                raise ValueError("boxes must be (n, 4), got %s" % (tuple(boxes.shape),))
            boxes = device_tensor(boxes, dev, torch.int32)
        n, J, hw, per_hw, codes, per_code = rotate_people_arguments(None if pts is None else tuple(pts.shape),
                                                                     None if boxes is None else tuple(boxes.shape), frame_hw, rotation_code)
        pts_out = None if pts is None else torch.empty_like(pts)
        boxes_out = None if boxes is None else torch.empty_like(boxes)
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        if n > 0:   # (nobody: an empty tensor has no address to hand over, and nothing would be launched)
            self._launch("hrn_rotate_people_dev", n, J, hw.ctypes.data, per_hw, codes.ctypes.data, per_code, ptr(pts), ptr(boxes), ptr(pts_out),
                         ptr(boxes_out))
        return pts_out if boxes is None else boxes_out if pts is None else (pts_out, boxes_out)

    # -- the annotated frame back to the encoder's layout ----------------------------------------------------------------------------
    def bgr_to_yuv(self, frames, format: str = "nv12", matrix: str = "bt601", range: str = "limited",  # noqa: A002
                   chroma_order: str = "uv", out=None):
        """BGR frames as 4:2:0 ``YuvFrame``s on the GPU (``hrn_bgr_to_yuv_frames``: ONE launch for all frames, no scratch) -- the
        way back from the frame the overlays draw on to what an encoder, a recorder or ``ffmpeg -f rawvideo -pix_fmt
        nv12|nv21|yuv420p|p010le|yuv420p10le`` consumes.  The arithmetic is the integer definition of include/hrnet_mi355.h: the
        exact forward coefficients at 20 bits, one chroma sample per 2x2 block from the block's mean; the 10-bit formats from the
        same 8-bit pixels with one rounding.  Equality with ``cv2.cvtColor(COLOR_BGR2YUV_I420)`` is not pinned.

        ``frames``: one (H, W, 3) uint8 BGR frame, an (F, H, W, 3) stack or a sequence of frames of any (even) sizes; host frames
        are uploaded once.  ``format``: ``"nv12"``, ``"i420"``, ``"p010"`` or ``"i010"``; ``chroma_order="vu"`` on nv12 gives NV21;
        ``matrix`` / ``range`` as in ``YuvFrame``.  Returns packed ``YuvFrame``(s) on the engine's GPU with those arguments: one for
        a frame, a list for a stack or a sequence.
        ``out``: ``YuvFrame`` destinations on the engine's GPU to write into instead (one, or one per frame; pitched ones are
        allowed, their padding keeps its bytes); format, matrix, range and chroma order are then THEIRS, and they are returned.
        Nothing is synchronised."""
        # what the arguments alone tell is told before anything is uploaded
        if not isinstance(frames, (torch.Tensor, np.ndarray, YuvFrame)):
            frames = list(frames)
        single = isinstance(frames, (torch.Tensor, np.ndarray)) and frames.ndim == 3
        if isinstance(frames, YuvFrame) or (not single and any(f is None or isinstance(f, YuvFrame) for f in frames)):
            raise ValueError("bgr_to_yuv takes BGR frames, none of them None, not YuvFrames")
        shapes = [tuple(f.shape) if hasattr(f, "shape") else np.shape(f) for f in ([frames] if single else frames)]
        for k, shape in enumerate(shapes):
            if len(shape) != 3 or shape[2] != 3:
                raise ValueError("frame %d must be (H, W, 3) uint8 BGR" % k)
            if shape[0] <= 0 or shape[1] <= 0 or shape[0] % 2 or shape[1] % 2:
                raise ValueError("frame %d: a 4:2:0 frame has an even, positive height and width, got %d x %d" % (k, shape[0], shape[1]))
        if out is None:
            YuvFrame.empty(2, 2, format, matrix, range, chroma_order)   # (its ValueError; judged even when there is no frame)
        else:
            dst = [out] if isinstance(out, YuvFrame) else list(out)
            if len(dst) != len(shapes):
                raise ValueError("out has %d frames for %d" % (len(dst), len(shapes)))
            for k, (d, shape) in enumerate(zip(dst, shapes)):
                if not isinstance(d, YuvFrame):
                    raise ValueError("out[%d] must be a YuvFrame" % k)
                if (d.height, d.width) != shape[:2]:
                    raise ValueError("out[%d] is %d x %d, frame %d is %d x %d" % (k, d.height, d.width, k, shape[0], shape[1]))
        dev = self.torch_device
        src = Frames.resident(frames, dev, one=True, rows=True)
        if out is None:
            dst = [YuvFrame.empty(h, w, format, matrix, range, chroma_order, dev) for h, w, _ in shapes]
        elif any(d.device != dev for d in dst):
            raise ValueError("out must lie on the engine's device %s: it is written where it is" % (dev,))
        if len(src):
            self._launch("hrn_bgr_to_yuv_frames", src.table(kind=_lib.CanvasC), Frames(dst, True).table(kind=_lib.CanvasC), len(src))
        return dst[0] if single else dst

    # -- person ids between two frames: who of the previous frame is who of this one ------------------------------------------------
    def associate_people(self, boxes, pts, prev_boxes, prev_pts, prev_ids, next_id, pose_alpha: float = 0.5,
                         similarity_threshold: float = 0.5, smoothing_alpha: float = 0.0, counts=None, prev_counts=None):
        """``postproc.associate_people`` on the GPU (``hrn_associate_people_dev``: one launch, one block per problem, no host
        read): ``find_person_id_associations`` of the reference's demo loop and its ``next_id`` update, for one video or the
        streams of a camera wall (``counts`` / ``prev_counts``: people per stream, on the host).

        ``boxes`` (n, 4) int32 and ``pts`` (n, J, 3) float32 as ``predict_frame`` / ``track_frame`` return them, ``prev_boxes``,
        ``prev_pts``, ``prev_ids`` (m,) int32 of the previous frame, ``next_id`` one int or (P,) int32.  Tensors of the right type
        on the engine's GPU are used where they lie -- ``boxes`` and ``pts`` are then smoothed IN PLACE and ``next_id`` is
        updated in place; host arrays are uploaded.  Returns ``(boxes, pts, ids, match, next_id, status)`` on the GPU, bit for
        bit the host form's: ``match`` the accepted previous person (counted inside its problem) or -1, ``status`` per problem
        (bit 0: a non-finite similarity, e.g. of two zero boxes, was counted as 0 and not accepted).  At most 256 people per
        problem and side."""
        from .postproc import _next_ids, _segments

        dev = self.torch_device
        boxes, prev_boxes = device_tensor(boxes, dev, torch.int32, (-1, 4)), device_tensor(prev_boxes, dev, torch.int32, (-1, 4))
        n, m = int(boxes.shape[0]), int(prev_boxes.shape[0])
        pts, prev_pts = as_tensor(pts, np.float32), as_tensor(prev_pts, np.float32)
        widths = {int(v.shape[1]) for v in (pts, prev_pts) if v.dim() == 3 and v.shape[0]}
        if len(widths) > 1:
            raise ValueError("the two sets of skeletons have different joint counts")
        joints = widths.pop() if widths else 1
        pts, prev_pts = device_tensor(pts, dev, torch.float32, (-1, joints, 3)), device_tensor(prev_pts, dev, torch.float32, (-1, joints, 3))
        prev_ids = device_tensor(prev_ids, dev, torch.int32, (-1,))
        if int(pts.shape[0]) != n or int(prev_pts.shape[0]) != m or int(prev_ids.shape[0]) != m:
            raise ValueError("pts must be (n, J, 3) beside (n, 4) boxes with one J on both sides, and prev_ids one per previous "
                             "person: got %s, %s, %s, %s, %s" % tuple(tuple(v.shape) for v in (boxes, pts, prev_boxes, prev_pts, prev_ids)))
        cur, prev = _segments(counts, n, "counts"), _segments(prev_counts, m, "prev_counts")
        if len(cur) != len(prev):
            raise ValueError("counts and prev_counts name %d and %d problems" % (len(cur) - 1, len(prev) - 1))
        problems = len(cur) - 1
        if isinstance(next_id, torch.Tensor) and next_id.is_cuda:   # used where it lies: never read on the host
            if next_id.device != dev or next_id.dtype != torch.int32 or next_id.numel() != problems or not next_id.is_contiguous():
                raise ValueError("next_id on a GPU must be a contiguous int32 tensor of %d value(s) on %s, got %s %s on %s"
                                 % (problems, dev, next_id.dtype, tuple(next_id.shape), next_id.device))
            nxt = next_id.reshape(-1)
        else:
            nxt = torch.from_numpy(_next_ids(next_id.numpy() if isinstance(next_id, torch.Tensor) else next_id, problems))
            nxt = nxt.to(dev, non_blocking=True)
        ids = torch.empty((n,), dtype=torch.int32, device=dev)
        match = torch.empty((n,), dtype=torch.int32, device=dev)
        status = torch.zeros((problems,), dtype=torch.int32, device=dev)
        self._launch("hrn_associate_people_dev", problems, cur.ctypes.data, prev.ctypes.data, joints, boxes.data_ptr(), pts.data_ptr(),
                     prev_boxes.data_ptr(), prev_pts.data_ptr(), prev_ids.data_ptr(), nxt.data_ptr(), float(pose_alpha),
                     float(similarity_threshold), float(smoothing_alpha), ids.data_ptr(), match.data_ptr(), status.data_ptr())
        return boxes, pts, ids, match, nxt, status

    # -- person ids through occlusions: the track table ---------------------------------------------------------------------------
    def new_track_table(self, streams: int = 1, capacity: int = 256, joints: Optional[int] = None) -> dict:
        """``postproc.new_track_table`` on the engine's GPU: a fresh table for ``track_people`` (``joints`` None: the engine's)"""
        from .postproc import new_track_table

        host = new_track_table(streams, capacity, self.nof_joints if joints is None else joints)
        return {name: torch.from_numpy(a).to(self.torch_device, non_blocking=True) for name, a in host.items()}

    def track_people(self, boxes, pts, table, pose_alpha: float = 0.5, similarity_threshold: float = 0.5, smoothing_alpha: float = 0.0,
                     max_lost: int = 0, coast: bool = False, velocity_alpha: float = 0.5, counts=None):
        """``postproc.track_people`` on the GPU (``hrn_track_people_dev``: one launch, one block per stream, no host read): one
        update of a track table that lives in device memory -- ids that survive gaps of up to ``max_lost`` updates, lost people
        compared where their velocity expects them with ``coast``, the library's zero rows numbered -1.

        ``boxes`` (n, 4) int32 and ``pts`` (n, J, 3) float32 as ``predict_frame`` / ``track_frame`` return them; tensors of the
        right type on the engine's GPU are used where they lie and smoothed IN PLACE, host arrays are uploaded.  ``table``: what
        ``new_track_table`` returned -- contiguous tensors on the engine's GPU, updated in place (``next_id`` included).
        ``counts``: rows per stream, on the host.  Returns ``(boxes, pts, ids, match_row, slot, status)`` on the GPU, bit for bit
        the host form's."""
        from .postproc import TRACK_FIELDS, _segments, track_table_shape

        dev = self.torch_device
        streams, capacity, joints = track_table_shape(table, lambda t: t.shape)
        for name, _, dtype, _ in TRACK_FIELDS + (("next_id", (), np.int32, 0),):
            t = table[name]
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != (torch.int32 if dtype is np.int32 else torch.float32) \
                    or not t.is_contiguous():
                raise ValueError("%s of the track table must be a contiguous %s tensor on %s" % (name, np.dtype(dtype).name, dev))
        boxes = device_tensor(boxes, dev, torch.int32, (-1, 4))
        n = int(boxes.shape[0])
        pts = device_tensor(as_tensor(pts, np.float32), dev, torch.float32, (-1, joints, 3))
        if int(pts.shape[0]) != n:
            raise ValueError("pts must be (n, %d, 3) beside (n, 4) boxes: got %s, %s" % (joints, tuple(boxes.shape), tuple(pts.shape)))
        cur = _segments(counts, n, "counts")
        if len(cur) - 1 != streams:
            raise ValueError("counts names %d streams, the table holds %d" % (len(cur) - 1, streams))
        ids, match_row, slot = (torch.empty((n,), dtype=torch.int32, device=dev) for _ in range(3))
        status = torch.zeros((streams,), dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t.numel() else None   # noqa: E731 -- (an empty tensor has no address to hand over)
        self._launch("hrn_track_people_dev", streams, cur.ctypes.data, capacity, joints, ptr(boxes), ptr(pts),
                     *[table[name].data_ptr() for name, *_ in TRACK_FIELDS], table["next_id"].data_ptr(), float(pose_alpha),
                     float(similarity_threshold), float(smoothing_alpha), int(max_lost), int(coast), float(velocity_alpha), ptr(ids),
                     ptr(match_row), ptr(slot), status.data_ptr())
        return boxes, pts, ids, match_row, slot, status

    # -- joints over time: One-Euro smoothing and the prediction of the next frame's joints -----------------------------------------
    def filter_poses(self, pts, state=None, match=None, counts=None, prev_counts=None, dt: float = 1 / 30, min_cutoff: float = 1.0,
                     beta: float = 0.007, d_cutoff: float = 1.0, threshold: float = 0.5, lookahead: Optional[float] = None):
        """``postproc.filter_poses`` on the GPU (``hrn_filter_poses_dev``: one launch, one thread per (person, joint), no host
        read): the One-Euro filter of every joint and the predicted joints ``raw position + filtered velocity * lookahead``,
        for one video or the streams of a camera wall (``counts`` / ``prev_counts``: people per stream, on the host).

        ``pts`` (n, J, 3) float32 as ``predict_frame`` / ``track_frame`` / ``associate_people`` return them, ``state`` the pair the
        previous call returned (None on the first frame), ``match`` (n,) int32 as ``associate_people`` wrote it (None: nobody is
        known).  Tensors of the right type on the engine's GPU are used where they lie; host arrays are uploaded.  The arguments
        are left as they are.  Returns ``(pts_out, pred, (values, age))`` on the GPU, bit for bit the host form's; ``pred`` is what
        ``track_frame`` wants as ``prev_pts``.  The prediction starts from the RAW position on purpose: the filtered position lags on
        steady motion -- the filter's known trade, tuned by ``beta`` -- while raw + velocity converges to zero error."""
        from .postproc import filter_arguments

        dev = self.torch_device
        pts = as_tensor(pts, np.float32)
        if pts.numel() == 0 and pts.dim() != 3:
            pts = pts.reshape(0, int(state[0].shape[1]) if state is not None and len(state[0].shape) == 3 else 1, 3)
        pts = device_tensor(pts, dev, torch.float32)
        if state is not None:
            state = device_tensor(state[0], dev, torch.float32), device_tensor(state[1], dev, torch.int32)
        if match is not None:
            match = device_tensor(match, dev, torch.int32, (-1,))
        n, m, joints, cur, prev, numbers = filter_arguments(tuple(pts.shape), None if state is None else (tuple(state[0].shape), tuple(state[1].shape)),
                                                            None if match is None else int(match.shape[0]), counts, prev_counts, dt, min_cutoff,
                                                            beta, d_cutoff, threshold, lookahead)
        pts_out, pred = torch.empty_like(pts), torch.empty_like(pts)
        values = torch.empty((n, joints, 6), dtype=torch.float32, device=dev)
        age = torch.empty((n, joints), dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()   # noqa: E731 -- (an empty tensor has no address)
        self._launch("hrn_filter_poses_dev", len(cur) - 1, cur.ctypes.data, prev.ctypes.data, joints, ptr(pts), ptr(match),
                     ptr(state and state[0]), ptr(state and state[1]), *numbers, ptr(pts_out), ptr(pred), ptr(values), ptr(age))
        return pts_out, pred, (values, age)

    # -- pose NMS: duplicate skeletons removed per image or stream, without leaving the device --------------------------------------
    def _pose_nms_launch(self, engine: bool, kpts, areas, scores, seg: np.ndarray, thresh, in_vis_thre, rescore_thre, soft, sigmas,
                         suppress):
        """``hrn_pose_nms_dev`` on device tensors of the right type (``scores`` may be None in the engine layout; ``sigmas`` a host
        array or None); returns the dict of output tensors"""
        from .postproc import _nan_if_none, pose_nms_flags

        dev = self.torch_device
        n, problems, joints = int(areas.shape[0]), len(seg) - 1, int(kpts.shape[1])
        sg = None
        if sigmas is not None:
            sg = torch.as_tensor(np.ascontiguousarray(sigmas, dtype=np.float64).reshape(-1))
            if sg.numel() != joints:
                raise ValueError("sigmas must have one value per joint")
            sg = sg.to(dev, non_blocking=True)
        keep = torch.empty((n,), dtype=torch.int32, device=dev)
        num = torch.empty((problems,), dtype=torch.int32, device=dev)
        scores_out = torch.empty((n,), dtype=torch.float64, device=dev)
        suppressor = torch.empty((n,), dtype=torch.int32, device=dev)
        status = torch.empty((problems,), dtype=torch.int32, device=dev)
        self._launch("hrn_pose_nms_dev", problems, seg.ctypes.data, joints, pose_nms_flags(engine, soft, suppress), kpts.data_ptr(),
                     areas.data_ptr(), None if scores is None else scores.data_ptr(), float(thresh), _nan_if_none(in_vis_thre),
                     _nan_if_none(rescore_thre), None if sg is None else sg.data_ptr(), keep.data_ptr(), num.data_ptr(),
                     scores_out.data_ptr(), suppressor.data_ptr(), status.data_ptr())
        return dict(keep=keep, num=num, scores=scores_out, suppressor=suppressor, status=status)

    def pose_nms(self, pts, boxes, det_scores=None, counts=None, thresh: float = 0.9, in_vis_thre=None, rescore_thre=None,
                 soft: bool = False, sigmas=None, suppress: bool = False):
        """``postproc.pose_nms`` (engine layout) on the GPU (``hrn_pose_nms_dev``: one launch, one block per problem, no host
        read): which of the skeletons of a frame are duplicates of a better one -- OKS NMS as the reference's evaluation runs it
        (``misc/nms/nms.py:97-177``), hard or ``soft``, for one video or the streams of a camera wall (``counts``: people per
        stream, on the host).

        ``pts`` (n, J, 3) float32 ``(y, x, confidence)`` and ``boxes`` (n, 4) int32 as ``predict_frame`` / ``track_frame`` return
        them, ``det_scores`` (n,) float32 or None (everybody 1.0).  Tensors of the right type on the engine's GPU are used where
        they lie; host arrays are uploaded.  ``rescore_thre``: order by the mean confidence of the joints above it times the
        score (None: by the score as given); ``in_vis_thre``: only the candidate's joints above it enter an OKS.  The order is
        descending and stable.  ``suppress=True`` zeroes the confidences and the box of everybody who is not kept, IN PLACE:
        ``draw_poses`` then skips them and the next ``track_frame`` reports them lost (all-padding crop) -- nothing is compacted
        and no ids are touched.
        Returns a dict of device tensors, bit for bit the host form's: ``keep`` (n,) int32 -- per problem the kept people in
        selection order, counted from the problem's first person, then -1; ``num`` (P,); ``scores`` (n,) float64 after rescoring;
        ``suppressor`` (n,) -- -1 kept, else who removed it (soft: -2 at the cap of 20); ``status`` (P,) -- bit 0 a NaN score was
        ordered last, bit 1 a non-finite OKS counted as 0; and the ``pts`` / ``boxes`` tensors the call worked on.  At most 256
        people per problem.  A latency link: one block per problem, one OKS row per kept person."""
        from .postproc import _segments

        dev = self.torch_device
        boxes = device_tensor(boxes, dev, torch.int32, (-1, 4))
        n = int(boxes.shape[0])
        joints = int(pts.shape[1]) if len(pts.shape) == 3 else (17 if sigmas is None else len(sigmas))
        pts = device_tensor(pts, dev, torch.float32, (-1, joints, 3))
        det = None if det_scores is None else device_tensor(det_scores, dev, torch.float32, (-1,))
        if int(pts.shape[0]) != n or (det is not None and int(det.shape[0]) != n):
            raise ValueError("pts must be (n, J, 3) beside (n, 4) boxes and n det_scores, got %s, %s, %s"
                             % (tuple(pts.shape), tuple(boxes.shape), None if det is None else tuple(det.shape)))
        out = self._pose_nms_launch(True, pts, boxes, det, _segments(counts, n, "counts"), thresh, in_vis_thre, rescore_thre, soft,
                                    sigmas, suppress)
        out["pts"], out["boxes"] = pts, boxes
        return out

    def _pose_nms_coco(self, kpts: np.ndarray, areas: np.ndarray, scores: np.ndarray, counts, thresh, in_vis_thre, rescore_thre, soft,
                       sigmas):
        """host arrays in the COCO layout through the device: one upload each, one launch, one download each; numpy results"""
        from .postproc import _segments

        dev = self.torch_device
        up = [torch.from_numpy(v).to(dev, non_blocking=True) for v in (kpts, areas, scores)]
        out = self._pose_nms_launch(False, up[0], up[1], up[2], _segments(counts, len(areas), "counts"), thresh, in_vis_thre,
                                    rescore_thre, soft, sigmas, False)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def nms_eval(self, preds, maxvals, areas, box_scores, image_index, oks_thre: float = 0.9, in_vis_thre: float = 0.2,
                 soft: bool = False, sigmas=None):
        """The rescoring and OKS NMS of ``evaluate_overall_accuracy`` (``datasets/COCO.py:353-382``) for a whole evaluation set in
        ONE launch, one block per image: ``preds`` (N, J, 2) image coordinates ``(x, y)`` and ``maxvals`` (N, J) or (N, J, 1) as
        ``predict_eval`` / ``get_final_preds`` give them, ``areas`` and ``box_scores`` (N,) of the detections, ``image_index`` (N,)
        integers naming each person's image (any order).  People are grouped by image on the host (a stable sort: inside an image
        they keep the caller's order); every score becomes the mean confidence of the joints above ``in_vis_thre`` times the box
        score, then ``oks_nms`` or (``soft``) ``soft_oks_nms`` runs per image with ``oks_thre`` and no visibility mask, as the
        reference calls them.
        Returns ``(scores, kept)``: ``scores`` (N,) float64, the rescored scores in the caller's order; ``kept`` a dict, image ->
        the indices into the caller's arrays that survive, best first, images in order of first appearance -- the structure the
        reference builds as ``oks_nmsed_kpts``.  Where nothing is kept everybody is returned (``COCO.py:379-380``).  At most 256
        people per image."""
        from .postproc import nms_eval

        return nms_eval(preds, maxvals, areas, box_scores, image_index, oks_thre, in_vis_thre, soft, sigmas, solve=self._pose_nms_coco)

    # -- COCO keypoint AP / AR: the number an evaluation reports, without leaving the device ------------------------------------------
    def keypoint_eval(self, dt_kpts, dt_scores, dt_image, gt_kpts, gt_area, gt_bbox, gt_iscrowd, gt_image, sigmas=None):
        """``postproc.keypoint_eval`` on the GPU (``hrn_keypoint_eval_dev``: four stream-ordered launches, no host read, no
        atomics): OKS matching of the detections to the ground truth per image, precision / recall over the set and the ten AP /
        AR statistics, as DEFINED in ``csrc/keypoint_eval_math.h`` (what ``COCOeval(gt, dt, 'keypoints')`` does with one category
        and ``maxDets = 20``; parity with pycocotools is not pinned).

        Arguments as ``postproc.keypoint_eval``; ``dt_image`` / ``gt_image`` are read on the host (both sides are grouped by image
        id there: a stable sort, ids ascending, the union of both sides' ids), everything else is a float64 / int32 tensor on the
        engine's GPU -- used where it lies when the side already is in image order, gathered on the device otherwise -- or a host
        array, which is uploaded.  Returns the dict of ``postproc.keypoint_eval`` as device tensors, bit for bit the host form's,
        plus ``images`` (P,) int64 on the host.  At most 256 detections and 256 people per image."""
        from .postproc import EVAL_AREAS, EVAL_RECS, EVAL_THRS, keypoint_eval_groups, keypoint_eval_joints

        dev = self.torch_device
        images, dt_order, gt_order, dt_start, gt_start, slots = keypoint_eval_groups(dt_image, gt_image)
        total, people, problems = int(dt_start[-1]), int(gt_start[-1]), len(images)
        joints = keypoint_eval_joints(tuple(dt_kpts.shape) if hasattr(dt_kpts, "shape") else np.shape(dt_kpts),
                                      tuple(gt_kpts.shape) if hasattr(gt_kpts, "shape") else np.shape(gt_kpts), sigmas)
        sg = None
        if sigmas is not None:
            sg = torch.as_tensor(np.ascontiguousarray(sigmas, dtype=np.float64).reshape(-1))
            if sg.numel() != joints:
                raise ValueError("sigmas must have one value per joint")
            sg = sg.to(dev, non_blocking=True)
        orders = [None if o is None else torch.from_numpy(o).to(dev, non_blocking=True) for o in (dt_order, gt_order)]

        def side(x, dtype, shape, order):
            x = device_tensor(x, dev, dtype, shape)
            return x if order is None else x[order.long()].contiguous()

        dk, ds = side(dt_kpts, torch.float64, (total, joints, 3), orders[0]), side(dt_scores, torch.float64, (total,), orders[0])
        gk, ga = side(gt_kpts, torch.float64, (people, joints, 3), orders[1]), side(gt_area, torch.float64, (people,), orders[1])
        gb, gc = side(gt_bbox, torch.float64, (people, 4), orders[1]), side(gt_iscrowd, torch.int32, (people,), orders[1])
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)   # noqa: E731
        out = dict(stats=new((10,), torch.float64), precision=new((EVAL_AREAS, EVAL_THRS, EVAL_RECS), torch.float64),
                   recall=new((EVAL_AREAS, EVAL_THRS), torch.float64), slot_person=new((slots,), torch.int32),
                   slot_score=new((slots,), torch.float64), dt_match=new((EVAL_AREAS, EVAL_THRS, slots), torch.int32),
                   dt_ignore=new((EVAL_AREAS, EVAL_THRS, slots), torch.uint8), npig=new((problems, EVAL_AREAS), torch.int32),
                   status=new((problems,), torch.int32))
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()   # noqa: E731 -- (an empty tensor has no address)
        self._launch("hrn_keypoint_eval_dev", problems, dt_start.ctypes.data, gt_start.ctypes.data, joints, ptr(dk), ptr(ds), ptr(gk),
                     ptr(ga), ptr(gb), ptr(gc), ptr(sg), *[ptr(v) for v in out.values()])
        if orders[0] is not None:
            out["slot_person"] = orders[0][out["slot_person"].long()]
        if orders[1] is not None:
            m = out["dt_match"]
            out["dt_match"] = torch.where(m >= 0, orders[1][m.clamp(min=0).long()], torch.full_like(m, -1))
        out["images"] = images
        return out

    def evaluate_overall_accuracy(self, preds, maxvals, areas, box_scores, image_index, gt_kpts, gt_area, gt_bbox, gt_iscrowd, gt_image,
                                  oks_thre: float = 0.9, in_vis_thre: float = 0.2, soft: bool = False, sigmas=None):
        """``evaluate_overall_accuracy`` of the reference's COCO dataset after the last batch (``datasets/COCO.py:353-388``) from
        arrays: ``nms_eval`` (rescoring and OKS NMS per image), the float32 rounding of the result file
        (``COCO.py:551-564``), then ``keypoint_eval`` against the ground truth -- both on the GPU.  ``preds`` .. ``image_index`` as
        ``nms_eval`` takes them, ``gt_*`` as ``keypoint_eval``.  Returns the reference's value: ``(OrderedDict of 'AP', 'Ap .5',
        'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)', AP)``."""
        from .postproc import evaluate_overall_accuracy

        return evaluate_overall_accuracy(preds, maxvals, areas, box_scores, image_index, gt_kpts, gt_area, gt_bbox, gt_iscrowd, gt_image,
                                         oks_thre, in_vis_thre, soft, sigmas, nms=self.nms_eval, evaluate=self.keypoint_eval)

    # -- clip mode: the people of many frames in one pre-path launch and one pass (throughput, not latency) ------------------
    def _device_frames(self, frames, one: bool = False) -> Frames:
        """``frames`` of ``preprocess_frames`` on the engine's GPU (``Frames.resident``); ``one``: a single frame is accepted too"""
        return Frames.resident(frames, self.torch_device, one)

    @staticmethod
    def _frame_table(frames):
        """the frame table of a list of device frames (``Frames.table``)"""
        return Frames(frames).table()

    def _preprocess_table(self, table, nframes: int, dets: np.ndarray, frame_index: np.ndarray, variant: str):
        """``hrn_preprocess_frames`` over a ready frame table (``_lib.Frame`` array whose device memory the caller keeps alive), or
        ``hrn_preprocess_frames_yuv`` over a ``_lib.YuvFrameC`` array: ``dets`` (n, 4) float32, ``frame_index`` (n,) int32.
        Returns ``(images, boxes numpy, boxes on the device)``."""
        crop = crop_code(variant)
        # the table is all this signature carries of the frames (tests call it with tables of their own): its element type is their kind
        yuv = isinstance(table, ctypes.Array) and table._type_ is _lib.YuvFrameC
        n = len(dets)
        h, w = self.resolution
        images = torch.empty((n, 3, h, w), dtype=torch.float32, device=self.torch_device)
        boxes = np.empty((n, 4), dtype=np.int32)
        boxes_dev = torch.empty((n, 4), dtype=torch.int32, device=self.torch_device)
        if n:
            self._launch("hrn_preprocess_frames" + ("_yuv" if yuv else ""), table, nframes, dets.ctypes.data, 4,
                         frame_index.ctypes.data, n, crop, images.data_ptr(), boxes.ctypes.data, boxes_dev.data_ptr())
        return images, boxes, boxes_dev

    def _frame_arguments(self, frames, detections, variant):
        crop_code(variant)
        frames = self._device_frames(frames)
        dets = [_detections(d) for d in detections]
        if len(dets) != len(frames):
            raise ValueError("%d frames but %d detection arrays" % (len(frames), len(dets)))
        for k, (f, d) in enumerate(zip(frames, dets)):
            if f is None and len(d):
                raise ValueError("frame %d is None but has %d detections" % (k, len(d)))
        return frames, dets

    def preprocess_frames(self, frames, detections, variant: str = "pad"):
        """The crop pre-path for the people of MANY frames in one call (``hrn_preprocess_frames``): one pair of launches, and the
        crops are written once, into the one batch the model reads -- no ``preprocess_frame`` per frame, no ``torch.cat``.

        ``frames``: (F, Hf, Wf, 3) uint8 BGR tensor or array, or a sequence of (Hf_k, Wf_k, 3) frames of differing sizes (host
        frames are uploaded once; a frame without people may be None), or a sequence of ``YuvFrame``s of any sizes, formats,
        matrices and ranges (all frames of a call are of one kind: a mixture raises ValueError); ``detections``: F arrays
        (P_k, >=4), empty arrays and None allowed; ``variant`` as in ``preprocess_frame``.
        Returns ``(images (sum P, 3, H, W) float32 on the GPU, boxes (sum P, 4) int32 numpy, boxes on the GPU, counts [P_k])``, the
        people in frame order -- bit-identical to the concatenated ``preprocess_frame`` outputs of the frames."""
        frames, dets = self._frame_arguments(frames, detections, variant)
        counts = [len(d) for d in dets]
        all_dets = np.ascontiguousarray(np.concatenate(dets, 0)) if dets else np.zeros((0, 4), np.float32)
        frame_index = np.repeat(np.arange(len(counts), dtype=np.int32), counts).astype(np.int32)
        images, boxes, boxes_dev = self._preprocess_table(frames.table(), len(frames), all_dets, frame_index, variant)
        return images, boxes, boxes_dev, counts

    def _run_group(self, table, nframes, dets, group, variant, return_heatmaps, refine):
        """pre-path + pass + decode of one group of ``group_frames``: ``[(frame, lo, hi, boxes, pts, heatmaps or None)]``"""
        parts = [dets[f][lo:hi] for f, lo, hi in group]
        sizes = [hi - lo for _, lo, hi in group]
        all_dets = np.ascontiguousarray(np.concatenate(parts, 0))
        frame_index = np.repeat(np.asarray([f for f, _, _ in group], np.int32), sizes).astype(np.int32)
        images, boxes, boxes_dev = self._preprocess_table(table, nframes, all_dets, frame_index, variant)
        out = self.predict_crops(images, boxes_dev, return_heatmaps=return_heatmaps, refine=refine)
        hm, pts = out if return_heatmaps else (None, out)
        res, at = [], 0
        for (f, lo, hi), n in zip(group, sizes):
            res.append((f, lo, hi, boxes[at:at + n], pts[at:at + n], None if hm is None else hm[at:at + n]))
            at += n
        return res

    @staticmethod
    def _frame_result(pieces, return_heatmaps):
        """one frame's ``(boxes, pts[, heatmaps])`` from the pieces of its passes (one piece: views, nothing is copied)"""
        if len(pieces) == 1:
            boxes, pts, hm = pieces[0]
        else:
            boxes = np.concatenate([p[0] for p in pieces], 0)
            pts = torch.cat([p[1] for p in pieces], 0)
            hm = torch.cat([p[2] for p in pieces], 0) if return_heatmaps else None
        return (boxes, pts, hm) if return_heatmaps else (boxes, pts)

    def predict_frames(self, frames, detections, return_heatmaps: bool = False, variant: str = "pad", refine: Optional[str] = None):
        """``preprocess_frames`` + ``predict_crops`` for a set of resident (or small) frames: the THROUGHPUT form of ``predict_frame``
        -- the people of consecutive frames share a pass (``group_frames``: greedily while they fit ``max_batch``; a frame with more
        people than ``max_batch`` runs in several passes).  Nothing about one frame's latency improves: ``predict_frame`` stays the
        call of a live loop.  ``frames`` / ``detections`` / ``variant`` as in ``preprocess_frames``, ``refine`` as in ``predict_crops``.
        Returns one ``(boxes (P_k,4) int32 numpy, pts (P_k,J,3) on the GPU[, heatmaps])`` per frame, ``pts`` / ``heatmaps`` views of
        their pass's outputs; a frame without people gives (0,4), (0,J,3) and (0,J,H/4,W/4)."""
        refine_code(refine)
        frames, dets = self._frame_arguments(frames, detections, variant)
        table = frames.table()
        pieces = [[] for _ in frames]
        for group in group_frames([len(d) for d in dets], self.max_batch):
            if any(hi > lo for _, lo, hi in group):
                for f, lo, hi, bx, pts, hm in self._run_group(table, len(frames), dets, group, variant, return_heatmaps, refine):
                    if hi > lo:
                        pieces[f].append((bx, pts, hm))
        return [self._frame_result(p, return_heatmaps) if p else self._empty_result(return_heatmaps) for p in pieces]

    def _empty_result(self, return_heatmaps):
        h, w = self.resolution
        dev = self.torch_device
        out = (np.zeros((0, 4), np.int32), torch.zeros((0, self.nof_joints, 3), dtype=torch.float32, device=dev))
        return out + (torch.zeros((0, self.nof_joints, h // 4, w // 4), dtype=torch.float32, device=dev),) if return_heatmaps else out

    def predict_clip(self, items, people_per_pass: Optional[int] = None, return_heatmaps: bool = False, variant: str = "pad",
                     refine: Optional[str] = None):
        """The throughput loop over a video file or a wall of cameras, modelled on ``predict_stream``: HOST frames in, joints out,
        with the uploads hidden behind the compute.  Not a latency path -- a frame's result comes when its group has run.

        ``items``: iterable of ``(frame, detections)``; ``frame`` a HOST (Hf, Wf, 3) uint8 BGR tensor or array (pinned memory for a
        truly asynchronous copy), of any size from item to item, or a host ``YuvFrame`` (half the upload bytes; all frames of a
        clip are of one kind, a mixture raises ValueError); a frame without people may be None; ``detections`` (P, >=4), empty
        or None.  Device-resident frames are refused (TypeError): they go to ``predict_frames``.
        Frames are read ahead into groups of at most ``people_per_pass`` people (default and upper bound ``max_batch``;
        ``group_frames``).  A group's frames are uploaded on a copy stream into one of two device arenas (grown on demand, frames at
        256-byte offsets; the frame table points into the arena) while the group before it runs pre-path, pass and decode on the
        current stream.  A frame with more people than one pass crosses once per pass.
        Yields per frame, in order, what ``predict_frames`` returns per frame; results are ready on the current stream (read them
        after a synchronize or through ``.cpu()``)."""
        refine_code(refine)
        crop_code(variant)
        per_pass = self.max_batch if people_per_pass is None else people_per_pass
        pipe = UploadPipeline(self.torch_device)   # its slots: byte arenas, grown on demand
        held = {}            # frame number -> (host frame or None, detections) of the frames read ahead and not yet run
        kinds = set()        # {True}: a clip of YuvFrames, {False}: of BGR frames

        def counts():        # feeds group_frames, which reads one frame ahead of the group it forms
            for k, item in enumerate(items):
                frame, d = item
                if isinstance(frame, (torch.Tensor, YuvFrame)) and frame.device.type != "cpu":
                    raise TypeError("predict_clip takes host frames; device-resident frames go to predict_frames")
                d = _detections(d)
                if frame is not None:
                    kinds.add(isinstance(frame, YuvFrame))
                    if len(kinds) > 1:
                        raise ValueError("the frames of one clip are all YuvFrames or all BGR frames, not a mixture")
                    if not isinstance(frame, YuvFrame):
                        frame = as_tensor(frame)
                        _check_frame(frame, k)
                        frame = frame.contiguous()
                elif len(d):
                    raise ValueError("frame %d is None but has %d detections" % (k, len(d)))
                held[k] = (frame, d)
                yield len(d)

        def upload(slot, group):
            """the frames of `group` that somebody is cut from -> the slot's arena on the copy stream; returns the group's table"""
            first = group[0][0]
            frames = Frames([None] * (group[-1][0] - first + 1), kinds == {True})
            offs, need = {}, 0   # frame, counted from `first` -> where its bytes start in the arena
            for f, lo, hi in group:
                if hi > lo and f - first not in offs:
                    frames[f - first] = held[f][0]
                    offs[f - first] = need
                    need += (host_bytes(held[f][0]).numel() + 255) // 256 * 256   # (a 10-bit frame needs an even address, whatever lies before it)
            arena = pipe.buffer(slot, torch.uint8, (need + need // 4,), at_least=need) if need else None
            with pipe.filling(slot):                             # the pre-path that read this arena has finished
                for f, off in offs.items():
                    flat = host_bytes(frames[f])
                    arena[off:off + flat.numel()].copy_(flat, non_blocking=True)
            return frames.table({f: arena.data_ptr() + off for f, off in offs.items()}), first, len(frames), bool(offs)

        groups = group_frames(counts(), self.max_batch, per_pass)
        nxt = next(groups, None)
        pending = upload(0, nxt) if nxt is not None else None
        k, pieces = 0, {}
        while nxt is not None:
            slot, group, (table, first, nfr, busy) = k & 1, nxt, pending
            nxt = next(groups, None)
            pending = upload(slot ^ 1, nxt) if nxt is not None else None   # goes out while this group computes
            if busy:
                pipe.ready(slot)
                local = [(f - first, lo, hi) for f, lo, hi in group]
                dets = {f - first: held[f][1] for f, _, _ in group}
                for f, lo, hi, bx, pts, hm in self._run_group(table, nfr, dets, local, variant, return_heatmaps, refine):
                    if hi > lo:
                        pieces.setdefault(f + first, []).append((bx, pts, hm))
                pipe.release(slot)
            last = group[-1][0]
            for f in sorted({g[0] for g in group}):
                # a frame above one pass spans several groups: it is complete with the group that holds its last people
                if f == last and nxt is not None and nxt[0][0] == f:
                    continue
                p = pieces.pop(f, None)
                del held[f]
                yield self._frame_result(p, return_heatmaps) if p else self._empty_result(return_heatmaps)
            k += 1

    def tap_infos(self) -> List[_lib.TapInfo]:
        """the tensors ``forward_tap`` can read: name, (c, h, w), index of the convolution that writes it (or -1)"""
        out = []
        for i in range(self._lib.hrn_tap_count(self._h)):
            ti = _lib.TapInfo()
            rc = self._lib.hrn_get_tap_info(self._h, i, ctypes.byref(ti))
            self._check(rc, "hrn_get_tap_info")
            out.append(ti)
        return out

    def forward_tap(self, images: torch.Tensor, name: str, crop0: int = 0, ncrops: Optional[int] = None,
                    return_heatmaps: bool = False, crop_step: int = 1):
        """Debug tap (the engine's forward hook): ONE micro-batch over ``images`` (n <= max_batch) with the named
        intermediate tensor of crops ``crop0, crop0 + crop_step, ...`` (``ncrops`` of them) copied out as (ncrops, C, H, W) fp32 -- for the bf16
        engine the stored bf16 values, widened exactly.  Names: ``tap_infos()`` / include/hrnet_mi355.h."""
        x = self._images_ptr(images)
        n = x.shape[0]
        if ncrops is None:
            ncrops = (n - crop0 + crop_step - 1) // crop_step
        info = {t.name.decode(): t for t in self.tap_infos()}.get(name)
        if info is None:
            raise KeyError("no tensor named %r is written by this plan" % name)
        dst = torch.empty((ncrops, info.c, info.h, info.w), dtype=torch.float32, device=x.device)
        h, w = self.resolution
        hm = torch.empty((n, self.nof_joints, h // 4, w // 4), dtype=torch.float32, device=x.device) if return_heatmaps else None
        self._launch("hrn_forward_tap", x.data_ptr(), n, name.encode(), int(crop0), int(ncrops), int(crop_step), dst.data_ptr(),
                     hm.data_ptr() if hm is not None else None)
        return (dst, hm) if return_heatmaps else dst

    def conv_infos(self) -> List[_lib.ConvInfo]:
        out = []
        for i in range(self._lib.hrn_conv_count(self._h)):
            ci = _lib.ConvInfo()
            rc = self._lib.hrn_get_conv_info(self._h, i, ctypes.byref(ci))
            self._check(rc, "hrn_get_conv_info")
            out.append(ci)
        return out

    def flops_per_crop(self) -> float:
        return float(self._lib.hrn_flops_per_crop(self._h))

    def workspace_bytes(self) -> int:
        return int(self._lib.hrn_workspace_bytes(self._h))

    def map_rebuilds(self) -> int:
        """block maps / descriptor arrays built and uploaded so far (they depend on the micro-batch size only)"""
        return int(self._lib.hrn_map_rebuilds(self._h))

    def launches_per_pass(self) -> int:
        return int(self._lib.hrn_launches_per_pass(self._h))

    def conv_compact(self, index: int) -> bool:
        """convolution `index` (conv_infos numbering) runs the 96-cout form over real pixels only (csrc/conv3x3_n96.inc, CP)"""
        return bool(self._lib.hrn_conv_compact(self._h, index))

    def stem_fused(self) -> bool:
        """conv1 + conv2 of the stem run as one kernel (csrc/stem_fused.hip)"""
        return bool(self._lib.hrn_stem_fused(self._h))

    def pad_violations(self) -> int:
        """debug: non-zero elements at pad / guard positions of the activation workspace (0 = the layout's invariant holds)"""
        return int(self._lib.hrn_debug_pad_violations(self._h))

    def switches(self) -> str:
        """the HRN_* environment switches this engine saw when it was created (always "" unless the process opted in with HRN_DEBUG_ENV=1)"""
        return self._lib.hrn_switches(self._h).decode()

    def profile_pass(self, images: torch.Tensor):
        """HIP-event time of every kernel of ONE internal pass over ``images[:max_batch]``.
        Returns (conv_ms[list], other_ms{stem,fuse,head,decode})."""
        x = self._images_ptr(images)
        n = min(x.shape[0], self.max_batch)
        nconv = self._lib.hrn_conv_count(self._h)
        conv_ms = (ctypes.c_float * nconv)()
        other = (ctypes.c_float * 4)()
        self._launch("hrn_profile_pass", x.data_ptr(), n, conv_ms, nconv, other)
        return list(conv_ms), dict(zip(("stem", "fuse", "head", "decode"), list(other)))


class MultiDeviceHRNet:
    """One process, several GPUs -- what ``torch.nn.DataParallel(model, device_ids)`` gives a user of the reference
    with ONE call (``SimpleHRNet.py:123-135``), without its per-forward parameter broadcast and heat-map gather:

    * one ``NativeHRNet`` handle per listed device (a device may be listed twice: two handles, two streams -- "lanes" of one
      GPU: each lane runs half the batch, and the launches of one fill the drain / tail of the other's, +4 % on a
      256-crop W48 batch, same joints);
    * weights are folded + packed once (first handle) and copied blob-to-blob to the others;
    * ``predict_crops`` / ``__call__`` / ``predict_frame`` split the packed crop batch (or the frame's detections) into
      contiguous index ranges (``dist.shard_range``), run every range on its device from its own host thread (the C ABI
      releases the GIL) on a per-handle side stream, and gather the small results on the first device.

    Same method surface as ``NativeHRNet`` for what ``SimpleHRNet`` uses.  Multi-process jobs (one rank per GPU,
    ``dist.ShardedHRNet``) remain the way to scale a serving loop; this class is the drop-in for the reference's
    single-process ``device='cuda'`` / ``'cuda:1,2'``."""

    def __init__(self, devices: Sequence[int], c: int = 48, nof_joints: int = 17, resolution: Tuple[int, int] = (384, 288),
                 dtype="bf16", max_batch: int = 32, model_name: str = "HRNet"):
        from concurrent.futures import ThreadPoolExecutor

        if len(devices) < 1:
            raise ValueError("at least one device")
        self.devices = [int(d) for d in devices]
        self.nets = [NativeHRNet(c, nof_joints, resolution, dtype, max_batch=max_batch, device=d, model_name=model_name)
                     for d in self.devices]
        self.streams = [torch.cuda.Stream(torch.device("cuda", d)) for d in self.devices]
        self.pool = ThreadPoolExecutor(max_workers=len(self.devices), thread_name_prefix="hrn-dev")
        first = self.nets[0]
        self.c, self.nof_joints, self.resolution = first.c, first.nof_joints, first.resolution
        self.dtype, self.max_batch, self.model_name = first.dtype, first.max_batch, first.model_name
        self.device_index = first.device_index

    @property
    def torch_device(self) -> torch.device:
        return self.nets[0].torch_device

    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def close(self):
        for n in getattr(self, "nets", []):
            n.close()
        pool = getattr(self, "pool", None)
        if pool is not None:
            pool.shutdown(wait=True)
            self.pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights: fold + pack once, then blob -> blob (device to device; peer copy across GPUs) -----------------------
    def load_state_dict(self, state_dict: Dict) -> "MultiDeviceHRNet":
        self.nets[0].load_state_dict(state_dict)
        src = self.nets[0].weight_blob_tensor()
        for net in self.nets[1:]:
            net.weight_blob_tensor().copy_(src)
            torch.cuda.synchronize(net.torch_device)
            net.adopt_weights()
        torch.cuda.synchronize(self.torch_device)
        return self

    def load_checkpoint(self, path: str) -> "MultiDeviceHRNet":
        return self.load_state_dict(torch.load(path, map_location="cpu"))

    def adopt_from(self, src: "NativeHRNet") -> "MultiDeviceHRNet":
        """weights from an engine that already holds them (loaded, or received over RCCL): blob -> blob, no re-packing"""
        blob = src.weight_blob_tensor()
        for net in self.nets:
            net.weight_blob_tensor().copy_(blob)
            torch.cuda.synchronize(net.torch_device)
            net.adopt_weights()
        return self

    # -- sharded execution ---------------------------------------------------------------------------------------------
    def _ranges(self, n: int) -> List[Tuple[int, int]]:
        from .dist import shard_range

        return [shard_range(n, len(self.nets), k) for k in range(len(self.nets))]

    def _run(self, n: int, work):
        """work(k, net, lo, hi) -> tuple of tensors on net's device (None and host arrays pass through); runs every non-empty
        range on its own thread and stream, orders it after the caller's stream on every device involved, returns the per-range
        results moved to the first device (in range order)."""
        first = self.torch_device
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(first))   # inputs produced on the caller's stream of the first device

        def job(k, lo, hi):
            net, stream = self.nets[k], self.streams[k]
            with torch.cuda.device(net.device_index), torch.cuda.stream(stream):
                stream.wait_event(ready)
                out = work(k, net, lo, hi)
                out = tuple(t if t is None or not isinstance(t, torch.Tensor) else t.to(first, non_blocking=True) for t in out)
                done = torch.cuda.Event()
                done.record(stream)
                return out, done

        futs = [(self.pool.submit(job, k, lo, hi)) for k, (lo, hi) in enumerate(self._ranges(n)) if hi > lo]
        outs = []
        mine = torch.cuda.current_stream(first)
        for f in futs:
            out, done = f.result()
            mine.wait_event(done)
            for t in out:   # produced under a side stream's allocator pool, consumed on the caller's stream
                if isinstance(t, torch.Tensor) and t.is_cuda:
                    t.record_stream(mine)
            outs.append(out)
        return outs

    def resize_frames(self, frames, interpolation: int = 2) -> torch.Tensor:
        """single-person pre-path (``NativeHRNet.resize_frames``) on the first device; ``predict_crops`` shards the result"""
        return self.nets[0].resize_frames(frames, interpolation)

    def predict_crops(self, images: torch.Tensor, boxes, return_heatmaps: bool = False, refine: Optional[str] = None):
        refine_code(refine)
        kw = {} if refine is None else {"refine": refine}   # None: every engine is called as without the option
        n = int(images.shape[0])
        b = as_tensor(boxes)
        if n == 0:
            return self.nets[0].predict_crops(images, b, return_heatmaps=return_heatmaps, **kw)

        def work(k, net, lo, hi):
            x = images[lo:hi].to(net.torch_device, non_blocking=True)
            out = net.predict_crops(x, b[lo:hi], return_heatmaps=return_heatmaps, **kw)
            return out if return_heatmaps else (out,)

        outs = self._run(n, work)
        if return_heatmaps:
            return torch.cat([o[0] for o in outs], 0), torch.cat([o[1] for o in outs], 0)
        return torch.cat([o[0] for o in outs], 0)

    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        n = int(images.shape[0])
        if n == 0:
            return self.nets[0](images)
        outs = self._run(n, lambda k, net, lo, hi: (net(images[lo:hi].to(net.torch_device, non_blocking=True)),))
        return torch.cat([o[0] for o in outs], 0)

    forward = __call__

    def _frame_shards(self, frame, detections, call):
        """``call(net, frame, dets)`` -> a tuple of numpy arrays and device tensors for the people of one frame: on the first
        engine when there is nobody, else every engine on its range of the detections (the frame goes to each once); the pieces
        joined in range order, the tensors on the first device"""
        dets = _detections(detections)
        if len(dets) == 0:
            return call(self.nets[0], frame, dets)
        frame = as_tensor(frame)
        outs = self._run(len(dets), lambda k, net, lo, hi: call(net, frame, dets[lo:hi]))
        return tuple(np.concatenate(p, 0) if isinstance(p[0], np.ndarray) else torch.cat(p, 0) for p in zip(*outs))

    def preprocess_frame(self, frame, detections, variant: str = "pad"):
        """crops of one frame, produced on the devices that will run them and gathered on the first one"""
        return self._frame_shards(frame, detections, lambda net, frame, dets: net.preprocess_frame(frame, dets, variant))

    def warp_crops(self, frames, centers=None, scales=None, rotations=None, frame_index=None, pixel_std=200, matrices=None) -> torch.Tensor:
        """``NativeHRNet.warp_crops`` with the crops split into index ranges: every device gets the frames once, cuts its range, and
        the batch is gathered on the first one"""
        frames = frame_stack(frames)
        h, w = self.resolution
        m, fi = _warp_arguments(int(frames.shape[0]), (w, h), centers, scales, rotations, frame_index, pixel_std, matrices)
        if len(m) == 0:
            return self.nets[0].warp_crops(frames, matrices=m, frame_index=fi)
        outs = self._run(len(m), lambda k, net, lo, hi: (net.warp_crops(frames, matrices=m[lo:hi], frame_index=fi[lo:hi]),))
        return torch.cat([o[0] for o in outs], 0)

    def predict_eval(self, frames, centers, scales, flip_pairs, frame_index=None, flip: bool = True,
                     post_processing: Union[bool, str] = True, pixel_std=200):
        """``NativeHRNet.predict_eval`` by the same split: each device warps, runs and decodes its range of people"""
        from . import postproc

        frames = frame_stack(frames)
        h, w = self.resolution
        m, fi = _warp_arguments(int(frames.shape[0]), (w, h), centers, scales, None, frame_index, pixel_std, None)
        if len(m) == 0:
            return self.nets[0].predict_eval(frames, centers, scales, flip_pairs, frame_index, flip, post_processing, pixel_std)

        def work(k, net, lo, hi):
            images = net.warp_crops(frames, matrices=m[lo:hi], frame_index=fi[lo:hi])
            return net.decode_eval(images, flip_pairs, flip=flip, post_processing=post_processing)

        outs = self._run(len(m), work)
        hm, preds, maxvals = (torch.cat([o[j] for o in outs], 0) for j in range(3))
        return postproc.final_preds(preds, np.asarray(centers), np.asarray(scales), pixel_std, (w // 4, h // 4)), maxvals, hm

    def predict_frame(self, frame, detections, return_heatmaps: bool = False, variant: str = "pad", refine: Optional[str] = None):
        refine_code(refine)
        kw = {} if refine is None else {"refine": refine}
        return self._frame_shards(frame, detections, lambda net, frame, dets: net.predict_frame(
            frame, dets, return_heatmaps=return_heatmaps, variant=variant, **kw))
