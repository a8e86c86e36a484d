"""simple-hrnet_amd -- MI355X-native (gfx950 / CDNA4) HRNet pose-inference hot path.

Drop-in for the model call + heat-map decode behind ``SimpleHRNet.predict()`` of
stefanopini/simple-HRNet (SimpleHRNet.py:281-308), plus its crop pre-path, flip-TTA evaluation decode, PoseResNet
and box NMS: hand-written HIP kernels behind the C ABI in
``include/hrnet_mi355.h``; this package is the thin ctypes / torch-tensor shim around it.

The directory name contains a hyphen (the name the project mandates), so import it with
``importlib.import_module("simple-hrnet_amd")`` or through the ``simple_hrnet_amd`` alias module
at the repository root.
"""
from . import _lib  # noqa: F401
from . import synth  # noqa: F401
from .native import COCO_HEAD_JOINTS, NativeHRNet, YuvFrame, bgr_to_yuv_colors, heat_colormap, palette, rotation_code_from_degrees  # noqa: F401
from .nms import gpu_nms  # noqa: F401
from . import postproc  # noqa: F401
from .postproc import filter_poses, find_person_id_associations, oks_nms, rotate_people, soft_oks_nms  # noqa: F401
from .simple_hrnet import SimpleHRNet  # noqa: F401
from .tracker import PersonTracker  # noqa: F401
from .synth import synth_boxes, synth_crops, synth_state_dict  # noqa: F401

__all__ = ["NativeHRNet", "YuvFrame", "palette", "heat_colormap", "COCO_HEAD_JOINTS", "bgr_to_yuv_colors", "SimpleHRNet", "PersonTracker", "gpu_nms", "oks_nms", "soft_oks_nms", "find_person_id_associations", "filter_poses", "rotate_people", "rotation_code_from_degrees", "postproc", "synth", "synth_state_dict", "synth_crops", "synth_boxes"]
