"""What a caller's "frames" are, and how they become device memory plus a frame table of the C ABI (include/hrnet_mi355.h).

A frame is an (Hf, Wf, 3) uint8 BGR tensor or array, or a ``YuvFrame`` (NV12 / NV21 / I420, 10-bit P010 / I010); the frames of a call are one frame, an
(F, Hf, Wf, 3) stack, or a sequence of frames of any sizes with None for a frame nobody is cut from -- all of one kind.
``Frames`` is that list together with its kind, its sizes and its ``hrn_frame`` / ``hrn_yuv_frame`` / ``hrn_canvas`` table.
The coercions every caller's tensor-or-array-like goes through (``as_tensor``, ``host_array``, ``device_tensor``) live here too.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib

PIX_FORMATS = {"nv12": 1, "i420": 2}          # include/hrnet_mi355.h: HRN_PIX_*: the 8-bit formats, which every entry takes
PIX_FORMATS_10BIT = {"p010": 5, "i010": 6}     # HRN_PIX_P010 / _I010: planes of 16-bit little-endian words; input side and bgr_to_yuv
PIX_NV21 = 4                                   # HRN_PIX_NV21: an "nv12" frame with chroma_order="vu"; input side and bgr_to_yuv (3 is unassigned)
PIX_10BIT = tuple(PIX_FORMATS_10BIT)
PIX_PLANAR = ("i420", "i010")                  # U and V planes of their own, rows of pitch / 2 bytes
YUV_MATRICES = {"bt601": 0, "bt709": 1}        # HRN_YUV_BT601 / _BT709
YUV_RANGES = {"limited": 0, "full": 1}         # HRN_YUV_LIMITED / _FULL


NUMPY_DTYPES = {torch.int32: np.int32, torch.float32: np.float32}   # what device_tensor converts an array-like to on the host


def as_tensor(x, dtype=None) -> torch.Tensor:
    """a tensor as it is (host or device); anything else as a host tensor over its contiguous array (of ``dtype``, when given)"""
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=dtype))


def host_array(x, dtype) -> np.ndarray:
    """a tensor (host or device: it is read back) or array-like as a host array of ``dtype``"""
    return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=dtype)


def device_tensor(x, device, dtype, shape=None) -> torch.Tensor:
    """a tensor or array-like as a contiguous ``dtype`` tensor on ``device``, of ``shape`` when given.  A tensor that already
    is all that is used where it lies -- what is written into the result is written into ``x``; anything else is converted
    (an array-like on the host when ``dtype`` is in ``NUMPY_DTYPES``, else on the device) or uploaded (once, asynchronously)."""
    x = as_tensor(x, NUMPY_DTYPES.get(dtype)).to(device, dtype=dtype, non_blocking=True)
    return (x if shape is None else x.reshape(shape)).contiguous()


class YuvFrame:
    """One 4:2:0 video frame as a decoder or ``ffmpeg -pix_fmt nv12|nv21|yuv420p|p010le|yuv420p10le`` delivers it, accepted
    wherever a BGR frame is (``preprocess_frame(s)``, ``predict_frame(s)``, ``predict_clip``, ``track_frame``, ``detector_input``,
    ``rotate_frames``) and by ``NativeHRNet.yuv_to_bgr``; ``draw_poses`` / ``draw_labels`` take ``"nv12"`` and ``"i420"`` only.
    ``NativeHRNet.bgr_to_yuv`` goes the other way: it returns BGR frames as ``YuvFrame``s of any of the five layouts (and writes
    into a caller's, through ``out=``) -- the annotated frame in the layout an encoder consumes.

    ``data``: uint8 tensor or array of any shape, host or device, in the rawvideo layout: ``height`` rows of ``pitch`` bytes of Y,
    then the chroma -- ``"nv12"``: ``height / 2`` rows of ``pitch`` bytes of interleaved U, V; ``"i420"``:
    ``height / 2`` rows of ``pitch / 2`` bytes of U, then the same of V.  NV21 (ffmpeg ``nv21``, Android cameras) is ``"nv12"``
    with ``chroma_order="vu"``: the pairs are V, U.  (The format string ``"nv21"`` itself stays refused, as it always was.)  The 10-bit formats have the same layouts in 16-bit
    little-endian words, ``pitch`` still in BYTES: ``"p010"`` is nv12's, the sample in the top 10 bits of a word; ``"i010"``
    (yuv420p10le) is i420's, the sample in the low 10 bits; the other six bits are ignored.  For these ``data`` may also be a numpy
    ``uint16`` array or a torch ``int16`` / ``uint16`` tensor, which is taken as its bytes.  ``pitch`` defaults to ``width``
    (``2 * width`` for the 10-bit formats); bytes of a row beyond its samples are never read into a result.  ``matrix``:
    ``"bt601"`` or ``"bt709"``; ``range``: ``"limited"`` (16..235, x 4 for 10 bits) or ``"full"``.
    ``draw_poses`` / ``draw_labels`` refuse a ``"vu"`` frame as they refuse the 10-bit formats.
    ValueError on an odd or non-positive size, a ``chroma_order`` other than ``"uv"`` / ``"vu"`` (``"vu"``: nv12 only), a pitch below the row's bytes, an odd pitch for i420, p010 and i010 (i010: not a
    multiple of 4 -- its chroma rows are ``pitch / 2`` bytes of words), a buffer shorter than ``nbytes``, or an unknown format,
    matrix or range."""

    def __init__(self, data, height: int, width: int, format: str = "nv12", matrix: str = "bt601", range: str = "limited",  # noqa: A002
                 pitch: Optional[int] = None, chroma_order: str = "uv"):
        if format not in PIX_FORMATS and format not in PIX_FORMATS_10BIT:
            raise ValueError("format must be one of %s, got %r" % (", ".join(repr(k) for k in list(PIX_FORMATS) + list(PIX_FORMATS_10BIT)), format))
        if chroma_order not in ("uv", "vu") or (chroma_order == "vu" and format != "nv12"):
            raise ValueError("chroma_order must be 'uv', or 'vu' on an 'nv12' frame (NV21), got %r on %r" % (chroma_order, format))
        if matrix not in YUV_MATRICES:
            raise ValueError("matrix must be 'bt601' or 'bt709', got %r" % (matrix,))
        if range not in YUV_RANGES:
            raise ValueError("range must be 'limited' or 'full', got %r" % (range,))
        height, width = int(height), int(width)
        if height <= 0 or width <= 0 or height % 2 or width % 2:
            raise ValueError("a 4:2:0 frame has an even, positive height and width, got %d x %d" % (height, width))
        wide = format in PIX_10BIT
        row = 2 * width if wide else width
        pitch = row if pitch is None else int(pitch)
        if pitch < row:
            raise ValueError("pitch %d is below %s %d" % (pitch, "twice the width" if wide else "the width", width))
        if format == "i420" and pitch % 2:
            raise ValueError("an i420 frame has an even pitch (its chroma rows are pitch / 2 bytes), got %d" % pitch)
        if wide and pitch % (4 if format == "i010" else 2):
            raise ValueError("a %s frame has a pitch that is a multiple of %d (its rows are 16-bit words%s), got %d"
                             % (format, 4 if format == "i010" else 2, ", its chroma rows pitch / 2 bytes" if format == "i010" else "", pitch))
        if wide and isinstance(data, np.ndarray) and data.dtype == np.uint16:
            data = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        data = as_tensor(data)
        if wide and data.dtype in (torch.int16, torch.uint16):
            data = data.contiguous().view(-1).view(torch.uint8)
        if data.dtype != torch.uint8:
            raise ValueError("data must be uint8" + (" (or 16-bit words, for a 10-bit format)" if wide else ""))
        self.height, self.width, self.pitch = height, width, pitch
        self.format, self.matrix, self.range, self.chroma_order = format, matrix, range, chroma_order
        data = data.contiguous().view(-1)
        if data.numel() < self.nbytes:
            raise ValueError("a %d x %d %s frame of pitch %d has %d bytes, the buffer has %d"
                             % (height, width, format, pitch, self.nbytes, data.numel()))
        self.data = data[:self.nbytes]

    @classmethod
    def _trusted(cls, data: torch.Tensor, height: int, width: int, like: "YuvFrame") -> "YuvFrame":
        """a packed frame (pitch == a row's bytes) of ``like``'s format, matrix and range over the flat uint8 tensor ``data`` of
        exactly its bytes, without the constructor's checks: ``rotate_frames``' fresh destination, whose arguments are its own"""
        f = cls.__new__(cls)
        f.height, f.width, f.pitch = height, width, width * like.sample_bytes
        f.format, f.matrix, f.range, f.chroma_order = like.format, like.matrix, like.range, like.chroma_order
        f.data = data
        return f

    @classmethod
    def empty(cls, height: int, width: int, format: str = "nv12", matrix: str = "bt601", range: str = "limited",  # noqa: A002
              chroma_order: str = "uv", device=None) -> "YuvFrame":
        """a packed frame over fresh, uninitialised bytes on ``device``: ``bgr_to_yuv``'s destination; the constructor's checks"""
        nbytes = max(int(height), 0) * max(int(width), 0) * 3 // 2 * (2 if format in PIX_10BIT else 1)
        return cls(torch.empty((nbytes,), dtype=torch.uint8, device=device), height, width, format, matrix, range, chroma_order=chroma_order)

    @property
    def sample_bytes(self) -> int:
        """bytes of one Y, U or V sample: 2 for the 10-bit formats"""
        return 2 if self.format in PIX_10BIT else 1

    @property
    def nbytes(self) -> int:
        return self.pitch * self.height * 3 // 2

    @property
    def device(self):
        return self.data.device

    def to(self, device, non_blocking: bool = False) -> "YuvFrame":
        """the same frame with its bytes on ``device`` (itself when they already are)"""
        data = self.data.to(device, non_blocking=non_blocking)
        return self if data is self.data else YuvFrame(data, self.height, self.width, self.format, self.matrix, self.range, self.pitch,
                                                       self.chroma_order)

    def _fill(self, entry: "_lib.YuvFrameC", base: Optional[int] = None):
        """``entry`` = the ``hrn_yuv_frame`` of this frame, its bytes at device address ``base`` (default: where ``data`` is)"""
        base = self.data.data_ptr() if base is None else base
        luma = self.pitch * self.height
        entry.y, entry.u = base, base + luma
        planar = self.format in PIX_PLANAR
        entry.v = base + luma + (self.pitch // 2) * (self.height // 2) if planar else None
        entry.height, entry.width, entry.pitch_y = self.height, self.width, self.pitch
        entry.pitch_c = self.pitch // 2 if planar else self.pitch
        code = PIX_NV21 if self.chroma_order == "vu" else PIX_FORMATS.get(self.format) or PIX_FORMATS_10BIT[self.format]
        entry.format, entry.matrix, entry.range = code, YUV_MATRICES[self.matrix], YUV_RANGES[self.range]


ROTATE_CODES = {"90cw": 0, "180": 1, "90ccw": 2}   # HRN_ROTATE_*: the values of cv2.ROTATE_90_CLOCKWISE / _180 / _90_COUNTERCLOCKWISE


def rotation_code_from_degrees(deg) -> Optional[int]:
    """The rotation tag of a video (degrees clockwise, what ffprobe reports) as the ``cv2.rotate`` code that turns its stored
    frames upright -- the mapping of the reference's ``check_video_rotation`` (misc/visualization.py:271-293) without ffmpeg:
    90 -> 0 (``ROTATE_90_CLOCKWISE``), 180 -> 1, 270 -> 2; None or 0 -> None (nothing to rotate); anything else: ValueError."""
    if deg is None:
        return None
    if isinstance(deg, (bool, str)) or deg != int(deg) or int(deg) not in (0, 90, 180, 270):
        raise ValueError("a rotation tag is 0, 90, 180 or 270 degrees, got %r" % (deg,))
    return {0: None, 90: 0, 180: 1, 270: 2}[int(deg)]


def rotation_codes(rotation_code, n: int) -> np.ndarray:
    """``rotation_code`` of ``rotate_frames`` / ``rotate_people`` -- one code or n of them -- as n int32; ValueError otherwise"""
    if type(rotation_code) is int and 0 <= rotation_code <= 2:   # (the usual call, without numpy's conversions)
        return np.full((n,), rotation_code, np.int32)
    codes = np.asarray(rotation_code)
    if codes.dtype.kind not in "iu" or codes.ndim > 1 or (codes.ndim == 1 and len(codes) != n):
        raise ValueError("rotation_code must be one integer code or one per item (%d), got %r" % (n, rotation_code))
    codes = np.ascontiguousarray(np.broadcast_to(codes, (n,)), dtype=np.int32)
    if ((codes < 0) | (codes > 2)).any():
        raise ValueError("a rotation code is 0 (90 clockwise), 1 (180) or 2 (90 counter-clockwise), got %r" % (rotation_code,))
    return codes


def _frame_kind(frames) -> bool:
    """True when the (non-None) frames are ``YuvFrame``s, False when none is; a mixture raises ValueError"""
    kinds = {isinstance(f, YuvFrame) for f in frames if f is not None}
    if len(kinds) > 1:
        raise ValueError("the frames of one call are all YuvFrames or all BGR frames, not a mixture")
    return kinds == {True}


def _check_frame(frame, k: int):
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3 or min(frame.shape[:2]) < 1:
        raise ValueError("frame %d must be (H, W, 3) uint8 BGR" % k)


def _bgr_rows(t: torch.Tensor) -> bool:
    """an (H, W, 3) tensor the overlay can be drawn into where it lies: packed pixels, rows any pitch >= 3 W apart"""
    return t.stride(2) == 1 and t.stride(1) == 3 and (t.shape[0] == 1 or t.stride(0) >= 3 * t.shape[1])


def frame_stack(frames, crops: bool = True) -> torch.Tensor:
    """``frames`` of ``warp_crops`` (``crops``) or ``resize_frames`` as an (F, Hf, Wf, 3) uint8 tensor (host or device, as
    given); ValueError otherwise.  Only ``warp_crops`` refuses an empty stack and sides outside [1, 32766]."""
    frames = as_tensor(frames)
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or (crops and frames.shape[0] < 1):
        raise ValueError("frames must be (Hf, Wf, 3) or (F, Hf, Wf, 3) uint8 BGR")
    if crops and (max(int(frames.shape[1]), int(frames.shape[2])) > 32766 or min(int(frames.shape[1]), int(frames.shape[2])) < 1):
        raise ValueError("frame sides must be in [1, 32766]")
    return frames


def host_bytes(frame) -> torch.Tensor:
    """the bytes of a host frame of ``predict_clip`` as a flat uint8 tensor: what is uploaded (a ``YuvFrame``: 1.5 bytes per pixel)"""
    return frame.data if isinstance(frame, YuvFrame) else frame.view(-1)


class Frames(list):
    """The frames of one call: a list of (Hf, Wf, 3) uint8 tensors or of ``YuvFrame``s (``yuv``), None where a frame nobody is
    cut from is left out."""

    def __init__(self, frames=(), yuv: Optional[bool] = None):
        super().__init__(frames)
        self.yuv = _frame_kind(self) if yuv is None else yuv

    @classmethod
    def resident(cls, frames, device, one: bool = False, rows: bool = False) -> "Frames":
        """``frames`` of ``preprocess_frames`` as contiguous frames on ``device``; a 4-D stack crosses PCIe in one copy and is
        then indexed, a sequence frame by frame (once each).  A sequence of ``YuvFrame``s stays ``YuvFrame``s, now on the
        device; one that mixes the two kinds raises ValueError.  ``one``: a single frame is taken as a sequence of one.
        ``rows``: a BGR frame of packed pixels whose rows are strided (a view into a larger buffer) stays as it is -- for
        ``rotate_frames``, whose ``hrn_canvas`` table carries a pitch."""
        if one and (isinstance(frames, YuvFrame) or (isinstance(frames, (torch.Tensor, np.ndarray)) and frames.ndim == 3)):
            frames = [frames]
        if isinstance(frames, np.ndarray) and frames.ndim == 4:
            frames = as_tensor(frames)
        if isinstance(frames, torch.Tensor):
            if frames.dim() != 4:
                raise ValueError("frames must be (F, Hf, Wf, 3) uint8 BGR or a sequence of (Hf, Wf, 3) frames")
            stack = frames.to(device, non_blocking=True).contiguous()
            out = [stack[k] for k in range(int(stack.shape[0]))]
        else:
            frames = list(frames)
            if _frame_kind(frames):
                return cls([None if f is None else f.to(device, non_blocking=True) for f in frames], True)
            out = [None if f is None else as_tensor(f).to(device, non_blocking=True) for f in frames]
            out = [f if f is None or (rows and f.dim() == 3 and _bgr_rows(f)) else f.contiguous() for f in out]
        for k, f in enumerate(out):
            if f is not None:
                _check_frame(f, k)
        return cls(out, False)

    @classmethod
    def canvases(cls, frames, device) -> "Frames":
        """the frames of ``draw_poses``: a frame on ``device`` stays where it is (it is drawn in place: ValueError when its
        pixels are not packed), a host frame is uploaded; the rows of a BGR frame may be strided"""
        yuv = _frame_kind(frames)
        out = []
        for k, f in enumerate(frames):
            if f is None or yuv:
                out.append(None if f is None else f.to(device, non_blocking=True))
                continue
            if not isinstance(f, torch.Tensor):
                f = torch.from_numpy(f) if isinstance(f, np.ndarray) and all(s > 0 for s in f.strides) else as_tensor(f)
            _check_frame(f, k)
            if f.device != device:
                f = f.to(device, non_blocking=True)
                if not _bgr_rows(f):
                    f = f.contiguous()
            elif not _bgr_rows(f):
                raise ValueError("frame %d cannot be drawn in place: its pixels must be packed (B, G, R) bytes in rows" % k)
            out.append(f)
        return cls(out, yuv)

    def rotated(self, codes, device) -> "Frames":
        """fresh destinations for ``rotate_frames``: per frame an (H', W', 3) tensor, or a ``YuvFrame`` of the rotated size with the
        frame's format, matrix and range and no pitch padding (2 bytes per sample for the 10-bit formats); None stays None"""
        out = []
        for f, code in zip(self, codes):
            if f is None:
                out.append(None)
                continue
            h, w = (f.height, f.width) if self.yuv else (int(f.shape[0]), int(f.shape[1]))
            h, w = (h, w) if code == 1 else (w, h)
            if self.yuv:
                out.append(YuvFrame(torch.empty((h * w * 3 // 2 * f.sample_bytes,), dtype=torch.uint8, device=device), h, w, f.format,
                                    f.matrix, f.range, chroma_order=f.chroma_order))
            else:
                out.append(torch.empty((h, w, 3), dtype=torch.uint8, device=device))
        return Frames(out, self.yuv)

    def sizes(self) -> np.ndarray:
        """(F, 2) int32 ``(height, width)`` per frame; zeros for None"""
        return np.asarray([(0, 0) if f is None else ((f.height, f.width) if self.yuv else tuple(f.shape[:2])) for f in self],
                          np.int32).reshape(-1, 2)

    def table(self, bases=None, kind=None):
        """the ``hrn_frame`` table of the frames (None: a null entry), the ``hrn_yuv_frame`` table when they are ``YuvFrame``s, or
        a table of another ``kind`` (``_lib.CanvasC``: only there may a BGR frame have strided rows).  ``bases``: frame number ->
        the device address its bytes were copied to (host frames in an arena); default: where each frame lies."""
        kind = kind or (_lib.YuvFrameC if self.yuv else _lib.Frame)
        table = (kind * max(len(self), 1))()
        for k, f in enumerate(self):
            if f is None:
                continue
            entry = table[k]
            base = None if bases is None else bases[k]
            if self.yuv:
                f._fill(entry, base)
                continue
            if base is None:
                base = f.data_ptr()
            entry.height, entry.width = int(f.shape[0]), int(f.shape[1])
            if kind is _lib.Frame:
                entry.data = base
            else:   # a canvas: the pixels of a BGR frame in `y`, its rows `pitch_y` bytes apart
                entry.y = base
                entry.pitch_y = max(int(f.stride(0)), 3 * int(f.shape[1]))
                entry.format = 0
        return table
