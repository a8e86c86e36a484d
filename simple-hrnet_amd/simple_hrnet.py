"""``SimpleHRNet`` with the reference's constructor and ``predict()`` contract (``SimpleHRNet.py:21-172, 174-496``) on
top of the MI355X library -- what a user of the reference instantiates after switching.

Same argument names and meaning, same return structure (numpy arrays: heat-maps float32, boxes int32 / float32, joints
``(y, x, confidence)`` float32; lists per image for stacks), same error for a wrong model name or image rank.  What is
different, and why:

* the person detector is injected (``detector=``: an object with ``predict_single(image)`` / ``predict(images)``
  returning ``(P, >=4)`` rows ``x1, y1, x2, y2, ...`` or ``None``) -- the reference's YOLOv3 wrapper depends on an
  un-vendored third-party submodule (``models_/detectors/yolo``) and YOLOv5 on ``torch.hub`` (network);
* ``multiperson=False``: frames of another size than the model resolution are resized on the GPU the way
  ``cv2.resize(frame, (W, H), interpolation)`` does it (``:213-218``; ``interpolation`` = ``cv2.INTER_NEAREST`` 0 /
  ``INTER_LINEAR`` 1 / ``INTER_CUBIC`` 2, default cubic as in the reference, anything else raises) -- OpenCV's published generic
  8-bit arithmetic, NOT pinned against a cv2 build (cv2 is absent here; ``include/hrnet_mi355.h``: ``hrn_resize_frames``);
* ``dtype`` picks the arithmetic mode of the engine (``"fp32"`` = parity mode, ``"bf16"`` = MFMA bf16, ``"fp16"`` = the same
  MFMA path with fp16 storage -- the counterpart of the reference's half-precision TensorRT export, ``--half``);
* ``refine`` (opt-in, default None = the reference's integer arg-max): ``"quarter"`` moves every joint a quarter heat-map cell
  towards the higher neighbour (the reference's ``get_final_preds`` step), ``"dark"`` decodes it to sub-cell precision with
  DARK (``include/hrnet_mi355.h``: ``HRN_REFINE_*``); every ``predict()`` path applies it;
* ``redetect_every`` (opt-in, default 1 = the detector runs on every call, as in the reference): with K > 1 the single-image
  multi-person path runs the detector on every K-th ``predict()`` call only -- and on a call that follows one that returned
  nobody -- and otherwise cuts the people from the new frame where their joints were in the previous one
  (``NativeHRNet.track_frame``, on the GPU; ``track_args`` = its ``threshold`` / ``min_joints`` / ``scale`` / ``min_side``).  People
  who cannot be followed (too few confident joints, or all of them beyond the frame) are dropped from the returned arrays;
* ``device_detector`` (opt-in, instead of ``detector``): a detector that takes and returns DEVICE tensors -- an object with
  ``predict_tensor(x)`` (``x``: the letterboxed (n, 3, size, size) float32 RGB batch ``NativeHRNet.detector_input`` made; returns,
  per image, a device tensor of its NMS-ed rows ``x1, y1, x2, y2, confidence, ...`` in LETTERBOX coordinates, or None) and the
  attributes ``size``, ``style`` (``"yolov3"`` / ``"yolov5"``), ``conf_thres`` and ``classes`` (either may be None).  The letterbox,
  the filters and the way back to frame coordinates run on the GPU (``detector_input`` -> ``predict_tensor`` ->
  ``detections_to_frame`` -> ``preprocess_frames_dev``); only the number of people per image is read back.  A box the host path
  would refuse with an error (degenerate, outside the frame) goes through as an all-padding crop instead.
  A detector object that has ``predict_raw(x)`` and no ``predict_tensor`` returns the RAW (n, N, 5 + C) output of its YOLO head
  (rows ``cx, cy, w, h, obj, cls...``, float32 or float16, on the device) and leaves the NMS to the GPU as well
  (``detector_input`` -> ``predict_raw`` -> ``NativeHRNet.detector_nms`` -> ``detections_to_frame`` -> ...): the rule is its
  ``style``, the IoU threshold its attribute ``nms_thres`` (required), and ``max_det`` (300), ``max_candidates`` (4096) and
  ``agnostic`` (False) are read when present.  On this path ``conf_thres`` must be set and positive (ValueError otherwise): the
  rows beyond an image's count are zeros, and a zero row must never become a person;
* devices: ``'cuda:N'`` is that GPU.  ``'cuda'`` (all GPUs) and ``'cuda:1,2'`` (the listed ones) are, in a plain Python
  process, ONE engine per listed GPU driven from this process (``native.MultiDeviceHRNet``: the crop batch of a
  ``predict()`` call is split by index range, one host thread per GPU) -- what ``DataParallel`` gives the reference with
  one call (``SimpleHRNet.py:123-135``); under ``torch.distributed.run`` (``LOCAL_RANK`` set) the same strings name the
  job's GPUs and each process takes the one of its rank (``resolve_device``), to be combined with ``dist.ShardedHRNet``.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from .native import MultiDeviceHRNet, NativeHRNet, refine_code

_MEAN = (0.485, 0.456, 0.406)   # SimpleHRNet.py:171
_STD = (0.229, 0.224, 0.225)


def _raw_detector_arguments(dd) -> dict:
    """the NMS arguments of a ``device_detector`` that has ``predict_raw`` and no ``predict_tensor``, as keywords of
    ``NativeHRNet.detector_nms``; ValueError when the object cannot be driven that way"""
    if not hasattr(dd, "predict_raw"):
        raise ValueError("device_detector needs predict_tensor(x) or predict_raw(x)")
    conf = getattr(dd, "conf_thres", None)
    if conf is None or not float(conf) > 0.0:
        raise ValueError("a device_detector with predict_raw needs a positive conf_thres (a zero row must never become a person), "
                         "got %r" % (conf,))
    if getattr(dd, "nms_thres", None) is None:
        raise ValueError("a device_detector with predict_raw needs nms_thres (the IoU threshold of its NMS)")
    return dict(iou_thres=float(dd.nms_thres), max_det=int(getattr(dd, "max_det", 300)),
                max_candidates=int(getattr(dd, "max_candidates", 4096)), agnostic=bool(getattr(dd, "agnostic", False)))


# (local-rank variable, task-count variables of the same launcher): srun / mpirun export their local rank even for a one-task
# job, so the variable only means "one GPU per process" when the job has more than one task
_LAUNCHERS = (("SLURM_LOCALID", ("SLURM_NTASKS", "SLURM_NPROCS")),
              ("OMPI_COMM_WORLD_LOCAL_RANK", ("OMPI_COMM_WORLD_SIZE",)),
              ("MV2_COMM_WORLD_LOCAL_RANK", ("MV2_COMM_WORLD_SIZE",)),
              ("MPI_LOCALRANKID", ("PMI_SIZE",)))


def _launcher_local_rank() -> Optional[int]:
    """the GPU slot a multi-process launcher gave this process, or None for a plain process.  ``torch.distributed.run`` sets
    LOCAL_RANK (taken as it is: torchrun does not restrict the visible devices).  srun / mpirun set their own variables and
    no LOCAL_RANK -- under any of them a process drives ONE GPU (a rank that built an engine on every visible GPU would
    oversubscribe the node) -- but only when the job really has several tasks, and the rank is folded onto the
    devices this task can SEE: under ``srun --gpus-per-task=1`` / gpu-bind every task sees a single GPU at index 0 while
    SLURM_LOCALID runs 0..7."""
    ndev = max(1, torch.cuda.device_count())
    if "LOCAL_RANK" in os.environ:
        # (taken as it is: whether it names a visible device is checked where it is USED as the device index -- _check_local_rank;
        # an explicit 'cuda:i[,j]' list maps it with a modulo instead)
        return int(os.environ["LOCAL_RANK"])
    for key, sizes in _LAUNCHERS:
        if key in os.environ:
            counts = [int(os.environ[k]) for k in sizes if os.environ.get(k, "").isdigit()]
            if not counts and os.environ.get("WORLD_SIZE", "").isdigit():
                counts = [int(os.environ["WORLD_SIZE"])]
            # one GPU per process unless the job is EXPLICITLY a single task (a launcher that exports a local rank
            # but no task count used to fall through and let every task build engines on all visible GPUs)
            if not counts or max(counts) > 1:
                return int(os.environ[key]) % ndev
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and "RANK" in os.environ:   # a launcher without a local-rank variable
        return int(os.environ["RANK"]) % ndev
    return None


def _check_local_rank(lr: int) -> int:
    """ torchrun does not restrict the visible devices: a local rank used DIRECTLY as the device index (device
    None / 'cuda' / torch.device('cuda')) beyond them is a launch error, said here rather than as an invalid-device failure deep
    inside the engine.  Explicit lists ('cuda:0', 'cuda:0,0', one visible GPU per rank) never come through here."""
    ndev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if lr < 0 or (ndev and lr >= ndev):
        raise ValueError("LOCAL_RANK=%d but this process sees %d GPU(s): launch at most one rank per visible GPU" % (lr, ndev))
    return lr


def resolve_device(device, local_rank: Optional[int] = None) -> torch.device:
    """The reference's device argument (``SimpleHRNet.py:123-139``) mapped onto one-process-per-GPU: ``'cuda:3'`` is that
    GPU; ``'cuda'`` (all GPUs through DataParallel there) and ``'cuda:1,2'`` (the listed ones) name the set this job runs
    on, of which THIS process takes the entry of its ``LOCAL_RANK`` (0 when not launched by ``torch.distributed.run``).
    Anything that is not CUDA raises, as the reference does for a wrong name -- there is no CPU path here."""
    if local_rank is None:
        local_rank = _launcher_local_rank() or 0
    if device is None:
        return torch.device("cuda", _check_local_rank(local_rank))
    if isinstance(device, torch.device):
        if device.type != "cuda":
            raise ValueError("the MI355X engine has no CPU path (device=%s)" % device)
        return torch.device("cuda", _check_local_rank(local_rank) if device.index is None else device.index)
    name = str(device)
    if name == "cuda":
        return torch.device("cuda", _check_local_rank(local_rank))
    if name.startswith("cuda:"):
        try:
            ids = [int(x) for x in name[5:].split(",")]
        except ValueError:
            raise ValueError("Wrong device name.") from None           # SimpleHRNet.py:139
        if ids and all(i >= 0 for i in ids):
            return torch.device("cuda", ids[local_rank % len(ids)])
    raise ValueError("Wrong device name." if name.startswith("cuda") else "the MI355X engine has no CPU path (device=%s)" % name)


def resolve_devices(device) -> list:
    """GPU indices THIS process drives for the reference's ``device`` argument.  Launched by ``torch.distributed.run``
    or another multi-process launcher (``LOCAL_RANK`` / ``SLURM_LOCALID`` / ``OMPI_COMM_WORLD_LOCAL_RANK`` / ``RANK`` +
    ``WORLD_SIZE``): exactly one, ``resolve_device``'s.  A plain process: ``'cuda'`` = every visible GPU,
    ``'cuda:1,2'`` = those (an index may repeat), ``'cuda:3'`` / ``torch.device('cuda', 3)`` = that one, ``None`` = GPU 0."""
    if _launcher_local_rank() is not None:
        return [resolve_device(device).index]
    if device is None:
        return [0]
    if isinstance(device, torch.device):
        if device.type == "cuda" and device.index is None:
            return list(range(max(1, torch.cuda.device_count())))   # (no visible GPU: index 0, and the engine says so when created)
        return [resolve_device(device).index]
    name = str(device)
    if name == "cuda":
        return list(range(max(1, torch.cuda.device_count())))
    if name.startswith("cuda:") and "," in name:
        resolve_device(name)   # validates (raises the reference's error for a malformed list)
        return [int(x) for x in name[5:].split(",")]
    return [resolve_device(device, 0).index]


class SimpleHRNet:
    def __init__(self, c, nof_joints, checkpoint_path, model_name="HRNet", resolution=(384, 288), interpolation=None,
                 multiperson=True, return_heatmaps=False, return_bounding_boxes=False, max_batch_size=32,
                 yolo_version="v3", yolo_model_def=None, yolo_class_path=None, yolo_weights_path=None, device=None,
                 enable_tensorrt=False, *, detector=None, dtype="fp32", refine=None, redetect_every=1, track_args=None,
                 device_detector=None):
        refine_code(refine)   # (raises ValueError before any engine is built)
        self.refine = refine
        if int(redetect_every) != redetect_every or redetect_every < 1:
            raise ValueError("redetect_every must be a positive integer, got %r" % (redetect_every,))
        self.redetect_every, self.track_args = int(redetect_every), dict(track_args or {})
        self._calls, self._last_pts = 0, None   # single-image multi-person calls so far; the joints the next call tracks from
        self.c, self.nof_joints, self.checkpoint_path = c, nof_joints, checkpoint_path
        self.model_name, self.resolution = model_name, tuple(resolution)
        self.interpolation = 2 if interpolation is None else int(interpolation)   # cv2.INTER_CUBIC (SimpleHRNet.py:27)
        if self.interpolation not in (0, 1, 2):
            raise ValueError("interpolation: only cv2.INTER_NEAREST (0), cv2.INTER_LINEAR (1) and cv2.INTER_CUBIC (2) are built")
        self.multiperson, self.return_heatmaps = multiperson, return_heatmaps
        self.return_bounding_boxes, self.max_batch_size = return_bounding_boxes, max_batch_size
        if model_name not in ("HRNet", "hrnet", "PoseResNet", "poseresnet", "ResNet", "resnet"):
            raise ValueError("Wrong model name.")                                   # SimpleHRNet.py:114
        if enable_tensorrt:
            raise ValueError("TensorRT is an NVIDIA engine; this class IS the native engine on MI355X")
        self.devices = resolve_devices(device)
        if self.redetect_every > 1 and len(self.devices) > 1:
            raise ValueError("redetect_every > 1 runs on one GPU (tracking is not sharded over devices)")
        self.device = torch.device("cuda", self.devices[0])      # where results are gathered / single-GPU work runs
        if detector is not None and device_detector is not None:
            raise ValueError("pass detector= or device_detector=, not both")
        if device_detector is not None and len(self.devices) > 1:
            raise ValueError("device_detector= runs on one GPU (the detector link is not sharded over devices)")
        if multiperson and detector is None and device_detector is None:
            raise ValueError("multiperson=True needs detector= (the reference's YOLO wrappers are un-vendored third-party code)")
        self.detector, self.device_detector = detector, device_detector
        if device_detector is not None and not hasattr(device_detector, "predict_tensor"):
            _raw_detector_arguments(device_detector)   # (raises ValueError before any engine is built)
        if len(self.devices) == 1:
            self.model = NativeHRNet(c, nof_joints, self.resolution, dtype, max_batch=max_batch_size, device=self.device,
                                     model_name=model_name)
        else:   # SimpleHRNet.py:126-135: DataParallel over the listed GPUs
            self.model = MultiDeviceHRNet(self.devices, c, nof_joints, self.resolution, dtype, max_batch=max_batch_size,
                                          model_name=model_name)
        if isinstance(checkpoint_path, dict):
            self.model.load_state_dict(checkpoint_path)
        else:
            self.model.load_checkpoint(checkpoint_path)                              # torch.load, raw or {'model': ...}

    # ------------------------------------------------------------------------------------------ SimpleHRNet.py:174-210
    def predict(self, image):
        rank = np.ndim(image)
        if rank == 3:       # one BGR frame
            return self._one_frame(image)
        if rank == 4:       # a stack of frames
            return self._frame_stack(image)
        raise ValueError("Wrong image format.")

    def _result(self, heatmaps, boxes, pts):                                       # :333-343 / :486-496
        wanted = ((self.return_heatmaps, heatmaps), (self.return_bounding_boxes, boxes), (True, pts))
        out = [value for keep, value in wanted if keep]
        return out[0] if len(out) == 1 else out

    def _normalise(self, images_bgr: np.ndarray) -> torch.Tensor:
        """single-person transform (SimpleHRNet.py:213-222 / :355-366): cv2.resize to the model resolution when the frame
        has another size (on the GPU, ``NativeHRNet.resize_frames``), BGR -> RGB, ToTensor, Normalize"""
        if tuple(images_bgr.shape[-3:-1]) != self.resolution:
            return self.model.resize_frames(images_bgr, self.interpolation)
        x = torch.from_numpy(np.ascontiguousarray(images_bgr[..., ::-1])).to(self.device)
        # tensor divisors: torch turns a division by a python scalar into a multiplication by its reciprocal on the GPU,
        # which is not the float32 division ToTensor performs
        x = x.reshape((-1,) + x.shape[-3:]).permute(0, 3, 1, 2).to(torch.float32)
        x = x / torch.full((1, 1, 1, 1), 255.0, dtype=torch.float32, device=self.device)
        mean = torch.tensor(_MEAN, dtype=torch.float32, device=self.device).view(1, 3, 1, 1)
        std = torch.tensor(_STD, dtype=torch.float32, device=self.device).view(1, 3, 1, 1)
        return ((x - mean) / std).contiguous()

    def _refine_kw(self):
        """the engine's ``refine`` argument; None: the engine is called exactly as without the option"""
        return {} if self.refine is None else {"refine": self.refine}

    def _hm_shape(self, n):
        return (n, self.nof_joints, self.resolution[0] // 4, self.resolution[1] // 4)

    # ------------------------------------------------------------------------------------------ SimpleHRNet.py:212-343
    def _one_frame(self, image):
        if not self.multiperson:
            images = self._normalise(image)
            boxes = np.asarray([[0, 0, image.shape[1], image.shape[0]]], dtype=np.float32)
            hm, pts = self.model.predict_crops(images, boxes, return_heatmaps=True, **self._refine_kw())
            return self._result(hm.cpu().numpy(), boxes, pts.cpu().numpy())
        if self.redetect_every > 1:
            return self._one_frame_tracked(image)
        if self.device_detector is not None:
            out = self._one_frame_detected_dev(image)
            return self._nobody() if out is None else self._result(None if out[2] is None else out[2].cpu().numpy(), out[0], out[1].cpu().numpy())
        found = self.detector.predict_single(image)
        if found is None or len(found) == 0:
            return self._nobody()
        dets = np.asarray(found.cpu() if isinstance(found, torch.Tensor) else found, np.float32)[:, :4]
        out = self.model.predict_frame(image, dets, return_heatmaps=self.return_heatmaps, **self._refine_kw())
        boxes, pts = out[0], out[1].cpu().numpy()
        hm = out[2].cpu().numpy() if self.return_heatmaps else None
        return self._result(hm, boxes, pts)

    def _device_detections(self, frames):
        """the detector link on the GPU for device frames (one (Hf, Wf, 3) tensor or a stack): ``detector_input`` ->
        ``predict_tensor`` (or ``predict_raw`` -> ``detector_nms``) -> ``detections_to_frame``.  Returns ``(rows, found, kept)``: the compacted rows in frame coordinates
        on the device (None when the detector found nothing anywhere), per image whether the detector returned rows at all, and
        the number of rows kept per image -- the one thing read back."""
        dd = self.device_detector
        nms = None if hasattr(dd, "predict_tensor") else _raw_detector_arguments(dd)
        x, geometry = self.model.detector_input(frames, dd.size, dd.style)
        if nms is not None:   # the raw head output: its NMS on the GPU; max_det rows per image, the zero rows fall to the filter below
            raw = dd.predict_raw(x)
            if len(raw.shape) != 3 or int(raw.shape[0]) != len(geometry):
                raise ValueError("predict_raw returned %s for %d images" % (tuple(raw.shape), len(geometry)))
            kept_rows = self.model.detector_nms(raw, dd.style, dd.conf_thres, **nms)[0]
            found, counts = [True] * len(geometry), [int(kept_rows.shape[1])] * len(geometry)
            dets = kept_rows.reshape(-1, int(kept_rows.shape[2]))
        else:
            per_image = list(dd.predict_tensor(x))
            if len(per_image) != len(geometry):
                raise ValueError("predict_tensor returned %d results for %d images" % (len(per_image), len(geometry)))
            found = [t is not None for t in per_image]
            counts = [int(t.shape[0]) if t is not None else 0 for t in per_image]
            if not any(counts):
                return None, found, [0] * len(counts)
            dets = torch.cat([t.to(self.device, torch.float32) for t in per_image if t is not None and len(t)], 0)
        rows, kept, _ = self.model.detections_to_frame(dets, geometry, counts=counts, conf_thres=getattr(dd, "conf_thres", None),
                                                       classes=getattr(dd, "classes", None), compact=True)
        kept = kept.cpu().numpy().tolist()
        if len(counts) > 1:   # the kept rows lead each image's segment: gather them (the index is host arithmetic on the counts)
            starts = np.concatenate([[0], np.cumsum(counts)])
            index = np.concatenate([np.arange(s, s + k) for s, k in zip(starts, kept)]).astype(np.int64)
            rows = rows[torch.from_numpy(index).to(self.device)]
        else:
            rows = rows[:kept[0]]
        return rows, found, kept

    def _one_frame_detected_dev(self, image):
        """the single-image multi-person path behind ``device_detector``: ``(boxes int32 numpy, pts on the GPU, heat-maps on the
        GPU or None)``, or None when nobody is kept"""
        frame = torch.from_numpy(np.ascontiguousarray(image)).to(self.device)
        rows, _, kept = self._device_detections(frame)
        if rows is None or kept[0] == 0:
            return None
        images, boxes_dev, _ = self.model.preprocess_frames_dev(frame, rows[:, :4], variant="pad")
        out = self.model.predict_crops(images, boxes_dev, return_heatmaps=self.return_heatmaps, **self._refine_kw())
        hm, pts = out if self.return_heatmaps else (None, out)
        return boxes_dev.cpu().numpy(), pts, hm

    def _nobody(self):                                                              # :331
        return self._result(np.zeros(self._hm_shape(0), np.float32), np.empty((0, 4), np.int32), np.empty((0, 0, 3), dtype=np.float32))

    def _one_frame_tracked(self, image):
        """``redetect_every`` = K > 1: the detector on calls 0, K, 2K, ... and after a call that returned nobody; every other call
        follows the previous call's people on the GPU.  The joints stay on the device between calls; what is downloaded is what
        the contract returns."""
        call, self._calls = self._calls, self._calls + 1
        if call % self.redetect_every == 0 or self._last_pts is None:
            self._last_pts = None
            if self.device_detector is not None:
                out = self._one_frame_detected_dev(image)
                if out is None:
                    return self._nobody()
                self._last_pts = out[1]
                return self._result(None if out[2] is None else out[2].cpu().numpy(), out[0], out[1].cpu().numpy())
            found = self.detector.predict_single(image)
            if found is None or len(found) == 0:
                return self._nobody()
            dets = np.asarray(found.cpu() if isinstance(found, torch.Tensor) else found, np.float32)[:, :4]
            out = self.model.predict_frame(image, dets, return_heatmaps=self.return_heatmaps, **self._refine_kw())
            self._last_pts = out[1]
            return self._result(out[2].cpu().numpy() if self.return_heatmaps else None, out[0], out[1].cpu().numpy())
        out = self.model.track_frame(image, self._last_pts, return_heatmaps=self.return_heatmaps, **self._refine_kw(), **self.track_args)
        alive = out[2] == 0                                  # people who could not be followed are dropped
        self._last_pts = out[1][alive]
        boxes, pts = out[0][alive].cpu().numpy(), self._last_pts.cpu().numpy()
        if len(pts) == 0:
            self._last_pts = None
            return self._nobody()
        return self._result(out[3][alive].cpu().numpy() if self.return_heatmaps else None, boxes, pts)

    # ------------------------------------------------------------------------------------------ SimpleHRNet.py:345-496
    def _frame_stack(self, images):
        if not self.multiperson:
            x = self._normalise(images)
            boxes = np.repeat(np.asarray([[0, 0, images.shape[2], images.shape[1]]], dtype=np.float32), len(images), axis=0)
            hm, pts = self.model.predict_crops(x, boxes, return_heatmaps=True, **self._refine_kw())
            return self._result(hm.cpu().numpy(), boxes, np.expand_dims(pts.cpu().numpy(), axis=1))   # :475
        if self.device_detector is not None:
            return self._frame_stack_detected_dev(images)
        per_frame = self.detector.predict(images)
        counts = [None if found is None else len(found) for found in per_frame]
        dets = [None if not n else np.asarray(found.cpu() if isinstance(found, torch.Tensor) else found, np.float32)[:, :4]
                for found, n in zip(per_frame, counts)]
        if not any(counts):                                                          # :477-484
            pts = [np.zeros((0, self.nof_joints, 3), dtype=np.float32) for _ in per_frame]
            return self._result(np.zeros(self._hm_shape(0), np.float32), np.asarray([], dtype=np.int32), pts)
        if hasattr(self.model, "preprocess_frames"):
            # :383-412 for the whole stack in one call: the stack crosses PCIe once, one pair of launches cuts everybody, and the
            # crops are written once, where the model reads them (no call per image, no torch.cat of :409-412)
            crops, boxes, _, _ = self.model.preprocess_frames(images, dets, "clamp")
        else:   # an engine without the multi-frame entry (native.MultiDeviceHRNet shards one frame's people): image by image
            parts = [self.model.preprocess_frame(images[index], d, "clamp") for index, d in enumerate(dets) if d is not None]
            crops, boxes = torch.cat([p[0] for p in parts], 0), np.concatenate([p[1] for p in parts], 0)
        out = self.model.predict_crops(crops, boxes, return_heatmaps=self.return_heatmaps, **self._refine_kw())
        hm, pts = (out[0].cpu().numpy(), out[1].cpu().numpy()) if self.return_heatmaps else (None, out.cpu().numpy())
        return self._per_frame(counts, hm, boxes, pts)

    def _frame_stack_detected_dev(self, images):
        """the stack path behind ``device_detector``: the stack crosses PCIe once; everybody is cut by one pre-path call"""
        stack = torch.from_numpy(np.ascontiguousarray(images)).to(self.device)
        rows, found, kept = self._device_detections(stack)
        if rows is None or not any(kept):                                            # :477-484
            pts = [np.zeros((0, self.nof_joints, 3), dtype=np.float32) for _ in found]
            return self._result(np.zeros(self._hm_shape(0), np.float32), np.asarray([], dtype=np.int32), pts)
        frame_index = np.repeat(np.arange(len(kept), dtype=np.int32), kept)
        crops, boxes_dev, _ = self.model.preprocess_frames_dev(stack, rows[:, :4], frame_index=frame_index, variant="clamp")
        out = self.model.predict_crops(crops, boxes_dev, return_heatmaps=self.return_heatmaps, **self._refine_kw())
        hm, pts = (out[0].cpu().numpy(), out[1].cpu().numpy()) if self.return_heatmaps else (None, out.cpu().numpy())
        counts = [k if f else None for f, k in zip(found, kept)]
        return self._per_frame(counts, hm, boxes_dev.cpu().numpy(), pts)

    def _per_frame(self, counts, hm, boxes, pts):
        pts_b, hm_b, boxes_b, index = [], [], [], 0                                  # :445-472: re-add the batch axis
        for n in counts:
            if n is not None:
                pts_b.append(pts[index:index + n])
                if hm is not None:
                    hm_b.append(hm[index:index + n])
                boxes_b.append(boxes[index:index + n])
                index += n
            else:
                pts_b.append(np.zeros((0, self.nof_joints, 3), dtype=np.float32))
                hm_b.append(np.zeros(self._hm_shape(0), dtype=np.float32))
                boxes_b.append(np.zeros((0, 4), dtype=np.float32))
        return self._result(hm_b, boxes_b, pts_b)
