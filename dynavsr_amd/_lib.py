"""ctypes binding of libdynavsr_hip.so (the C ABI declared in include/dynavsr_hip.h).

There is deliberately NO fallback: if the library is missing or a call fails, a RuntimeError
carrying dvsr_last_error() is raised.  The product path never routes through torch CPU ops or
the oracle.
"""
import ctypes
import functools
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_longlong, c_size_t, c_void_p

import torch

_runtime = {"configured": False, "hw_queues": None, "effective": None}


def configure_runtime(hw_queues=6):
    """Process-wide runtime settings the execution plans want, applied EXPLICITLY (never at import).

    ROCm maps HIP streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default), and streams that share a queue run
    behind each other.  The plans put their weight gradients on a side stream; with the default, as soon as another
    component of the process holds streams (an initialised RCCL communicator does) that side stream shares a queue and
    the inner MAML step measures 10.0 instead of 8.2 ms.  Two more queues are enough.  The runtime reads
    the variable when HIP is initialised (the first device call), so this must run before that: `create_model`,
    `bench.py` and the tools call it first thing.  A value the user exported is never overridden.  Returns
    {"hw_queues": the value in force, "effective": False when HIP was already initialised and the value came too late}."""
    if not _runtime["configured"]:
        user = os.environ.get("GPU_MAX_HW_QUEUES")
        late = torch.cuda.is_initialized()
        if user is None and not late:
            os.environ["GPU_MAX_HW_QUEUES"] = str(int(hw_queues))
        _runtime.update(configured=True, hw_queues=os.environ.get("GPU_MAX_HW_QUEUES"),
                        effective=(user is not None) or not late)
    return {"hw_queues": _runtime["hw_queues"], "effective": _runtime["effective"]}


def runtime_report(device=None):
    """What the process actually got: the hardware-queue setting, whether it came in time, and the MEASURED answer to the
    question it exists for -- does the plans' weight-gradient side stream run beside the current stream of `device`
    (dvsr_side_stream_overlaps: 1 / 0 / -1 unknown)?  bench.py records it in its line."""
    r = configure_runtime()
    overlaps = None
    if torch.cuda.is_available():
        with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
            overlaps = int(lib().dvsr_side_stream_overlaps(stream()))
    return {"hw_queues": r["hw_queues"], "effective": r["effective"], "side_stream_overlaps": overlaps}


_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libdynavsr_hip.so")
_lib = None

ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2


class Conv2dDesc(Structure):
    _fields_ = [("x0", c_void_p), ("x1", c_void_p), ("w", c_void_p), ("bias", c_void_p),
                ("res", c_void_p), ("y", c_void_p),
                ("N", c_int), ("c0", c_int), ("c1", c_int), ("H", c_int), ("W", c_int),
                ("Cout", c_int), ("ks", c_int), ("stride", c_int), ("pad", c_int), ("act", c_int),
                ("pixel_shuffle", c_int), ("x1_bdiv", c_int),
                ("x0_bstride", c_longlong), ("x1_bstride", c_longlong),
                ("pre", c_void_p), ("pre_bdiv", c_int)]


class EdvrConfig(Structure):
    _fields_ = [(k, c_int) for k in ("nf", "nframes", "groups", "front_RBs", "back_RBs", "scale",
                                     "center", "bf16_mfma")]


class FrameDesc(Structure):
    """dvsr_frame_desc: a frame at any address and pitch (include/dynavsr_hip.h)."""
    _fields_ = [("format", c_int), ("h", c_int), ("w", c_int), ("row_stride", c_longlong), ("plane_stride", c_longlong),
                ("pixel_stride", c_int)]


FRAME_F32_CHW, FRAME_U8_HWC_RGB, FRAME_U8_HWC_BGR, FRAME_U8_Y = 0, 1, 2, 3
FRAME_U16_Y_MSB, FRAME_U16_Y_10, FRAME_U16_Y_12 = 4, 5, 6          # (U8_Y and these: dvsr_frame_luma_sad and dvsr_frame_score)
FRAME_U16_HWC_RGB, FRAME_U16_HWC_BGR = 16, 17                      # rgb48le / bgr48le (pixel stride 6 or 8 bytes), depth 16
FRAME_U8_CHW_RGB, FRAME_U8_CHW_GBR = 18, 19                        # planar bytes: torchvision's decoded image / gbrp
FRAME_U16_CHW_RGB, FRAME_U16_CHW_GBR = 20, 21                      # planar words, the level in the low bits: frame_depth()
FRAME_PAD_REFLECT, FRAME_PAD_REPLICATE = 0, 1


def frame_depth(fmt, depth):
    """DVSR_FRAME_DEPTH: a 16-bit-word format of dvsr_frame_desc with the bits of a level, 10, 12 or 16 (stored as 0)."""
    return fmt | ((depth & 15) << 8)


class YuvDesc(Structure):
    """dvsr_yuv_desc: a YCbCr 4:2:0 / 4:2:2 / 4:4:4 frame, every plane at any address and pitch (include/dynavsr_hip.h)."""
    _fields_ = [("format", c_int), ("h", c_int), ("w", c_int), ("matrix", c_int), ("range", c_int),
                ("plane", c_void_p * 3), ("row_stride", c_longlong * 3)]


YUV_NV12, YUV_I420 = 0, 1
YUV_CHROMA_420, YUV_CHROMA_422, YUV_CHROMA_444 = 0, 1, 2          # format = form | chroma << 4, of both descriptors
# the same field with a chroma siting other than "left" (DESIGN 3.2x): a pair of sub-sampling and siting
YUV_CHROMA_420_CENTER, YUV_CHROMA_420_TOPLEFT, YUV_CHROMA_422_CENTER = 4, 5, 6


def yuv_format(form, chroma):
    """DVSR_YUV_FORMAT: the semi-planar (0) or planar (1) form of a descriptor with a chroma sub-sampling."""
    return form | (chroma << 4)


YUV_BT601, YUV_BT709 = 0, 1
YUV_BT2020NC = 9                                                  # H.273's MatrixCoefficients code
YUV_LIMITED, YUV_FULL = 0, 1


class Yuv16Desc(Structure):
    """dvsr_yuv16_desc: a 10- / 12-bit YCbCr 4:2:0 / 4:2:2 / 4:4:4 frame in 16-bit words, every plane at any even address and pitch."""
    _fields_ = [("format", c_int), ("depth", c_int), ("h", c_int), ("w", c_int), ("matrix", c_int), ("range", c_int),
                ("plane", c_void_p * 3), ("row_stride", c_longlong * 3)]


YUV16_SEMI_MSB, YUV16_PLANAR_LSB = 0, 1


class ResizeAxis(Structure):
    """dvsr_resize_axis: the table of one axis of dvsr_frame_resize, in device memory (include/dynavsr_hip.h)."""
    _fields_ = [("first", c_void_p), ("weights", c_void_p), ("taps", c_int)]


class StitchAxis(Structure):
    """dvsr_stitch_axis: the table of one axis of dvsr_frame_stitch, in device memory (include/dynavsr_hip.h)."""
    _fields_ = [("first", c_void_p), ("weights", c_void_p), ("origins", c_void_p), ("cover", c_int)]


FLIP_W, FLIP_H = 1, 2                                             # dvsr_frame_flip's flags
TASK_TRANSPOSE = 4                                                # beside them in a dvsr_task_frame's flags


class TaskFrame(Structure):
    """dvsr_task_frame: one frame of one task of dvsr_task_degrade / dvsr_task_gather, 32 bytes (include/dynavsr_hip.h)."""
    _fields_ = [("src", c_void_p), ("row_stride", c_longlong), ("plane_stride", c_longlong), ("kernel", c_int), ("flags", c_int)]


class ScoreArgs(Structure):
    """dvsr_score_args: what dvsr_frame_score compares and where (include/dynavsr_hip.h)."""
    _fields_ = [("channel", c_int), ("crop_border", c_int), ("depth", c_int), ("lo", c_float), ("hi", c_float)]


SCORE_RGB, SCORE_Y = 0, 1


class EstimatorConfig(Structure):
    _fields_ = [(k, c_int) for k in ("kind", "nf", "in_nc", "scale", "nframes")]


def _declare(lib):
    P, I, F, LL = c_void_p, c_int, c_float, c_longlong
    sig = {
        "dvsr_last_error": (c_char_p, []),
        "dvsr_version": (I, []),
        "dvsr_mdcn_forward": (I, [P] * 6 + [I] * 13 + [P]),
        "dvsr_mdcn_forward_fast_workspace_bytes": (c_size_t, [I, I, I]),
        "dvsr_mdcn_forward_fast": (I, [P] * 6 + [I] * 7 + [P, c_size_t, P]),
        "dvsr_mdcn_pack_forward": (I, [P] * 5 + [I] * 13 + [P]),
        "dvsr_mdcn_pack_forward_fast": (I, [P] * 5 + [I] * 7 + [P, c_size_t, P]),
        "dvsr_conv2d_forward": (I, [POINTER(Conv2dDesc), P]),
        "dvsr_upsample_bilinear_forward": (I, [P, P, LL, I, I, I, F, P]),
        "dvsr_upsample_bilinear_backward": (I, [P, P, LL, I, I, I, F, I, P]),
        "dvsr_pool3s2_forward": (I, [P, P, P, LL, I, I, P]),
        "dvsr_pool3s2_backward": (I, [P, P, P, P, LL, I, I, P]),
        "dvsr_tsa_gate_forward": (I, [P] * 5 + [I, I, I, LL, P]),
        "dvsr_tsa_gate_backward": (I, [P] * 8 + [I, I, I, LL, P]),
        "dvsr_tsa_blend_forward": (I, [P] * 4 + [LL, P]),
        "dvsr_tsa_blend_backward": (I, [P] * 5 + [LL, P]),
        "dvsr_edvr_plan_create": (I, [POINTER(EdvrConfig), I, I, I, POINTER(c_void_p)]),
        "dvsr_edvr_plan_create_grouped": (I, [POINTER(EdvrConfig), I, I, I, I, POINTER(c_void_p)]),
        "dvsr_edvr_plan_create_ex": (I, [POINTER(EdvrConfig), I, I, I, I, I, POINTER(c_void_p)]),
        "dvsr_edvr_plan_destroy": (None, [P]),
        "dvsr_edvr_num_params": (I, [P]),
        "dvsr_edvr_num_launches": (I, [P]),
        "dvsr_edvr_workspace_bytes": (c_size_t, [P, I]),
        "dvsr_edvr_forward": (I, [P, POINTER(c_void_p), P, P, P, c_size_t, P]),
        "dvsr_edvr_forward_packed": (I, [P, POINTER(c_void_p), P, P, P, c_size_t, P]),
        "dvsr_edvr_backward": (I, [P, POINTER(c_void_p), P, P, POINTER(c_void_p), P, P, c_size_t, P]),
        "dvsr_edvr_num_backward_launches": (I, [P]),
        "dvsr_estimator_plan_create": (I, [POINTER(EstimatorConfig), I, I, I, POINTER(c_void_p)]),
        "dvsr_estimator_plan_create_grouped": (I, [POINTER(EstimatorConfig), I, I, I, I, POINTER(c_void_p)]),
        "dvsr_estimator_plan_create_ex": (I, [POINTER(EstimatorConfig), I, I, I, I, I, POINTER(c_void_p)]),
        "dvsr_estimator_plan_destroy": (None, [P]),
        "dvsr_estimator_num_params": (I, [P]),
        "dvsr_estimator_num_launches": (I, [P, I]),
        "dvsr_estimator_workspace_bytes": (c_size_t, [P, I]),
        "dvsr_estimator_forward": (I, [P, POINTER(c_void_p), P, P, P, c_size_t, P]),
        "dvsr_estimator_backward": (I, [P, POINTER(c_void_p), P, P, POINTER(c_void_p), P, c_size_t, P]),
        "dvsr_conv2d_backward_workspace_bytes": (c_size_t, [POINTER(Conv2dDesc)]),
        "dvsr_conv2d_backward": (I, [POINTER(Conv2dDesc), P, P, P, P, P, P, c_size_t, P]),
        "dvsr_mdcn_backward_workspace_bytes": (c_size_t, [I] * 10),
        "dvsr_mdcn_backward": (I, [P] * 10 + [I] * 12 + [P, c_size_t, P]),
        "dvsr_adam_step": (I, [POINTER(c_void_p)] * 4 + [POINTER(LL), I, F, F, F, F, F, I, P]),
        "dvsr_sgd_step": (I, [POINTER(c_void_p)] * 2 + [POINTER(LL), I, F, F, P]),
        "dvsr_replicate_tensors": (I, [POINTER(c_void_p)] * 2 + [POINTER(LL), I, I, P]),
        "dvsr_degrade_apply": (I, [P, P, P, I, I, I, I, I, I, I, I, I, P]),
        "dvsr_frame_degrade": (I, [P, POINTER(FrameDesc), P, I, I, P, LL, LL, I, P]),
        "dvsr_task_degrade": (I, [P, P, I, I, I, I, I, P, I, I, I, P, I, P]),
        "dvsr_task_gather": (I, [P, P, I, I, I, I, I, P, P]),
        "dvsr_frame_metrics_workspace_bytes": (c_size_t, [I, I, I]),
        "dvsr_frame_metrics": (I, [P, P, I, I, I, F, F, P, P, P, c_size_t, P]),
        "dvsr_charbonnier_workspace_bytes": (c_size_t, []),
        "dvsr_charbonnier_forward": (I, [P, P, P, LL, F, P, c_size_t, P]),
        "dvsr_conv2d_packed_workspace_bytes": (c_size_t, [POINTER(Conv2dDesc)]),
        "dvsr_conv2d_forward_packed": (I, [POINTER(Conv2dDesc), P, c_size_t, P]),
        "dvsr_conv2d_dgrad_packed": (I, [POINTER(Conv2dDesc), P, P, P, c_size_t, P]),
        "dvsr_conv2d_packed_geometry": (I, [POINTER(Conv2dDesc), POINTER(ctypes.c_int * 4)]),
        "dvsr_conv2d_wgrad_geometry": (I, [POINTER(Conv2dDesc), I, I, POINTER(ctypes.c_int * 8)]),
        "dvsr_conv2d_wgrad_workspace_bytes": (c_size_t, [POINTER(Conv2dDesc), I]),
        "dvsr_conv2d_wgrad_bf16": (I, [POINTER(Conv2dDesc), P, P, P, P, c_size_t, P]),
        "dvsr_conv2d_wgrad_split3": (I, [POINTER(Conv2dDesc), P, P, P, P, c_size_t, P]),
        "dvsr_flow_warp_forward": (I, [P, P, P, I, I, I, I, LL, P]),
        "dvsr_flow_warp_backward": (I, [P, P, P, P, P, I, I, I, I, LL, P]),
        "dvsr_avgpool2_forward": (I, [P, P, LL, I, I, P]),
        "dvsr_avgpool2_backward": (I, [P, P, LL, I, I, I, P]),
        "dvsr_resize_bilinear_ac_forward": (I, [P, P, LL, I, I, I, I, F, LL, P]),
        "dvsr_resize_bilinear_ac_backward": (I, [P, P, LL, I, I, I, I, F, LL, P]),
        "dvsr_upsample_bicubic_ac_forward": (I, [P, P, LL, I, I, I, P]),
        "dvsr_upsample_bicubic_ac_backward": (I, [P, P, LL, I, I, I, P]),
        "dvsr_channel_affine": (I, [P, P, P, P, I, I, LL, LL, LL, I, P]),
        "dvsr_batchnorm_workspace_bytes": (c_size_t, [I]),
        "dvsr_batchnorm_forward": (I, [P] * 8 + [I, I, LL, I, F, F, I, P, c_size_t, P]),
        "dvsr_batchnorm_backward": (I, [P] * 9 + [I, I, LL, I, I, P, c_size_t, P]),
        "dvsr_temporal_gather3_forward": (I, [P, P, I, I, I, LL, I, P]),
        "dvsr_temporal_gather3_backward": (I, [P, P, I, I, I, LL, I, P]),
        "dvsr_dynamic_filter_forward": (I, [P, P, P, P, I, I, I, I, I, P]),
        "dvsr_dynamic_filter_backward": (I, [P, P, P, P, P, P, I, I, I, I, I, P]),
        "dvsr_conv3x3_small_cout": (I, [P, P, P, P, P, I, I, I, I, I, I, P]),
        "dvsr_conv1x1_dual": (I, [P, P, P, P, P, P, P, I, I, I, I, I, P]),
        "dvsr_patch_gather_forward": (I, [P, P, POINTER(c_int), POINTER(c_int), I, I, I, I, I, I, P]),
        "dvsr_patch_gather_backward": (I, [P, P, POINTER(c_int), POINTER(c_int), I, I, I, I, I, I, P]),
        "dvsr_l1_tail_forward": (I, [P, P, P, F, P, LL, P, c_size_t, P]),
        "dvsr_l1_tail_backward": (I, [P, P, P, F, P, LL, P]),
        "dvsr_charbonnier_backward": (I, [P, P, P, P, LL, F, P]),
        "dvsr_charbonnier_forward_grouped": (I, [P, P, P, LL, I, F, P, c_size_t, P]),
        "dvsr_charbonnier_backward_grouped": (I, [P, P, P, P, LL, I, F, P]),
        "dvsr_l1_tail_forward_grouped": (I, [P, P, P, F, P, LL, I, P, c_size_t, P]),
        "dvsr_l1_tail_backward_grouped": (I, [P, P, P, F, P, LL, I, P]),
        "dvsr_charbonnier_region_forward": (I, [P, P, P, I, LL, I, I, I, I, F, P, c_size_t, P]),
        "dvsr_charbonnier_region_backward": (I, [P, P, P, P, I, LL, I, I, I, I, F, P]),
        "dvsr_l1_tail_region_forward": (I, [P, P, P, F, P, I, LL, I, I, I, I, P, c_size_t, P]),
        "dvsr_l1_tail_region_backward": (I, [P, P, P, F, P, I, LL, I, I, I, I, P]),
        "dvsr_edvr_op_info": (I, [P, I, c_char_p, I, c_char_p, I, POINTER(ctypes.c_double),
                                  POINTER(ctypes.c_double)]),
        "dvsr_edvr_forward_timed": (I, [P, POINTER(c_void_p), P, P, P, c_size_t, P, POINTER(c_float)]),
        "dvsr_debug_mfma_peak": (LL, [P, I, I, I, I, P]),
        "dvsr_debug_mfma_shadow": (I, [P, P, I, I, I, I, I, P]),
        "dvsr_edvr_tensor_info": (I, [P, c_char_p, POINTER(LL), POINTER(LL)]),
        "dvsr_edvr_plan_work": (I, [P, POINTER(ctypes.c_double * 9)]),
        "dvsr_edvr_plan_work_nograd": (I, [P, POINTER(ctypes.c_double * 9)]),
        "dvsr_edvr_op_launch_count": (I, [P, I, I]),
        "dvsr_side_stream_overlaps": (I, [P]),
        "dvsr_edvr_op_output": (I, [P, I, I, POINTER(c_int), POINTER(LL), POINTER(LL)]),
        "dvsr_estimator_plan_work": (I, [P, POINTER(ctypes.c_double * 9)]),
        "dvsr_edvr_stream_create": (I, [POINTER(EdvrConfig), I, I, I, POINTER(c_void_p)]),
        "dvsr_edvr_stream_destroy": (None, [P]),
        "dvsr_edvr_stream_num_params": (I, [P]),
        "dvsr_edvr_stream_num_launches": (I, [P, I]),
        "dvsr_edvr_stream_cache_bytes": (c_size_t, [P]),
        "dvsr_edvr_stream_workspace_bytes": (c_size_t, [P]),
        "dvsr_edvr_stream_extract": (I, [P, POINTER(c_void_p), P, I, P, c_size_t, P, c_size_t, I, P]),
        "dvsr_edvr_stream_fuse": (I, [P, POINTER(c_void_p), POINTER(c_int), P, c_size_t, P, P, c_size_t, I, P]),
        "dvsr_frame_ingest": (I, [P, POINTER(FrameDesc), P, I, I, I, P]),
        "dvsr_frame_emit": (I, [P, I, I, P, POINTER(FrameDesc), F, F, P]),
        "dvsr_edvr_stream_extract_frame": (I, [P, POINTER(c_void_p), P, POINTER(FrameDesc), I, I, P, c_size_t, P, c_size_t, I,
                                               P]),
        "dvsr_frame_ingest_yuv": (I, [POINTER(YuvDesc), P, I, I, I, P]),
        "dvsr_frame_emit_yuv": (I, [P, I, I, POINTER(YuvDesc), F, F, P]),
        "dvsr_edvr_stream_extract_frame_yuv": (I, [P, POINTER(c_void_p), POINTER(YuvDesc), I, I, P, c_size_t, P, c_size_t, I, P]),
        "dvsr_frame_luma_sad": (I, [P, P, POINTER(FrameDesc), LL, I, P, P]),
        "dvsr_frame_ingest_yuv16": (I, [POINTER(Yuv16Desc), P, I, I, I, P]),
        "dvsr_frame_emit_yuv16": (I, [P, I, I, POINTER(Yuv16Desc), F, F, P]),
        "dvsr_edvr_stream_extract_frame_yuv16": (I, [P, POINTER(c_void_p), POINTER(Yuv16Desc), I, I, P, c_size_t, P, c_size_t, I,
                                                     P]),
        "dvsr_frame_resize_taps": (I, [I, I]),
        "dvsr_frame_resize_table": (I, [I, I, I, P, P]),
        "dvsr_frame_resize": (I, [P, I, I, I, I, P, I, I, I, I, POINTER(ResizeAxis), POINTER(ResizeAxis), P]),
        "dvsr_frame_imresize_taps": (I, [I, I, I, I, POINTER(c_int)]),
        "dvsr_frame_imresize_table": (I, [I, I, I, I, I, P, P]),
        "dvsr_frame_imresize": (I, [P, POINTER(FrameDesc), I, I, I, I, I, P, LL, LL, I, I, POINTER(ResizeAxis), POINTER(ResizeAxis),
                                    I, P]),
        "dvsr_frame_flip": (I, [P, P, LL, I, I, I, P]),
        "dvsr_frame_flip_mean": (I, [P, P, P, P, P, LL, I, I, P]),
        "dvsr_frame_stitch_origins": (I, [I, I, I, POINTER(c_int), I]),
        "dvsr_frame_stitch_cover": (I, [I, I, I]),
        "dvsr_frame_stitch_table": (I, [I, I, I, I, I, P, P]),
        "dvsr_frame_stitch": (I, [P, I, I, I, I, I, P, I, I, POINTER(StitchAxis), POINTER(StitchAxis), POINTER(c_int),
                                  POINTER(c_int), P]),
        "dvsr_edvr_stream_max_image_bytes": (ctypes.c_ulonglong, [P]),
        "dvsr_frame_score_workspace_bytes": (c_size_t, [I, I, I]),
        "dvsr_frame_score": (I, [P, POINTER(FrameDesc), P, POINTER(FrameDesc), POINTER(ScoreArgs), P, P, c_size_t, P]),
        "dvsr_switch_count": (I, []),
        "dvsr_switch_info": (I, [I, POINTER(c_char_p), POINTER(c_int), POINTER(c_int), POINTER(c_char_p)]),
        "dvsr_switch_parse": (I, [I, c_char_p, POINTER(c_int)]),
        "dvsr_switch_value": (I, [I, POINTER(c_int)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return sig


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                "libdynavsr_hip.so is missing (%s). Build it with `python -m dynavsr_amd.build` "
                "(hipcc --offload-arch=gfx950); there is no fallback path." % SO_PATH)
        # DVSR_HIP_LIB: load another build of the same library (tools/ use it for the trace build)
        _lib = ctypes.CDLL(os.environ.get("DVSR_HIP_LIB", SO_PATH))
        _lib._signatures = _declare(_lib)
    return _lib


SW_BUILD, SW_PROCESS, SW_CALL, SW_DEBUG = 0, 1, 2, 3             # DVSR_SW_*: when the library reads a switch


@functools.lru_cache(maxsize=None)
def switches():
    """The library's table of DVSR_* environment switches (csrc/switches.h), in its order: [(name, scope, default, doc)].
    A switch's index in this list is its index in dvsr_switch_parse / dvsr_switch_value.  No device needed."""
    rows = []
    for i in range(lib().dvsr_switch_count()):
        name, doc, scope, dflt = c_char_p(), c_char_p(), c_int(), c_int()
        check(lib().dvsr_switch_info(i, ctypes.byref(name), ctypes.byref(scope), ctypes.byref(dflt), ctypes.byref(doc)), "dvsr_switch_info")
        rows.append((name.value.decode(), scope.value, dflt.value, doc.value.decode()))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def switch_names(scope):
    """The names of one scope: SW_BUILD makes the engine's plan-cache key, SW_PROCESS its warn-on-change list."""
    return tuple(name for name, s, _dflt, _doc in switches() if s == scope)


def switch_value(name):
    """What the library takes the switch for now, under its scope (dvsr_switch_value)."""
    v = c_int()
    check(lib().dvsr_switch_value([r[0] for r in switches()].index(name), ctypes.byref(v)), "dvsr_switch_value")
    return v.value


def check(rc, what=""):
    if rc != 0:
        msg = lib().dvsr_last_error().decode("utf-8", "replace")
        raise RuntimeError("libdynavsr_hip %s failed (rc=%d): %s" % (what, rc, msg))


def ptr(t):
    """Device pointer of a tensor that must already be fp32, contiguous and on a HIP device."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libdynavsr_hip needs a tensor on the GPU, got device %s" % t.device)
    if t.dtype != torch.float32:
        raise RuntimeError("libdynavsr_hip computes in fp32, got %s" % t.dtype)
    if not t.is_contiguous():
        raise RuntimeError("libdynavsr_hip needs contiguous tensors")  # deform_conv_cuda.cpp:493-494
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream
