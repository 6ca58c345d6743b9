"""Frames in and out of the video path (csrc/frame_io.hip: dvsr_frame_ingest / dvsr_frame_emit).

A decoder delivers 8-bit interleaved RGB or BGR (cv2 order) frames [H,W,3|4] of any size; the networks compute on fp32
planar [3,Hp,Wp] in [0,1] whose sides are multiples of 4 (EDVR) or 16 (TOFlow), and an encoder or PNG writer wants 8-bit
interleaved back.  The reference does both on the host (`img.astype(np.float32) / 255.`, BGR -> RGB: data/util.py:82,
:109; util.tensor2img on the fp32 frame copied back); here the bytes travel and the conversion runs on the device:

    padded_size(h, w, multiple)   -> (Hp, Wp)
    ingest(frame, ...)            -> fp32 [3,Hp,Wp] on the GPU: v / 255, RGB order, padded at the bottom and right from the
                                     frame itself ('reflect' = torch.nn.functional.pad(.., mode='reflect'), or 'replicate')
    emit(sr, h, w, layout)        -> the top-left h x w crop of fp32 [3,Hs,Ws] as uint8 [h,w,3] (util.tensor2img's bits)
                                     or fp32 [3,h,w]

`layout` is 'chw' (fp32 planar), 'hwc_rgb' or 'hwc_bgr' (uint8 interleaved); None means 'chw' for a float tensor and
'hwc_rgb' for a uint8 one.  adapt.super_resolve_frames uses these (and engine.StreamPlan.extract_frame, which ingests
straight into the frame cache); they are also the building blocks for feeding padded clips to the adaptation loops by hand.
"""
import ctypes

import torch

from . import _lib as L

LAYOUTS = ('chw', 'hwc_rgb', 'hwc_bgr')
_FORMAT = {'chw': L.FRAME_F32_CHW, 'hwc_rgb': L.FRAME_U8_HWC_RGB, 'hwc_bgr': L.FRAME_U8_HWC_BGR}
_PAD = {'reflect': L.FRAME_PAD_REFLECT, 'replicate': L.FRAME_PAD_REPLICATE}


def padded_size(h, w, multiple):
    """The smallest (Hp, Wp) >= (h, w) whose sides are multiples of `multiple`."""
    h, w, m = int(h), int(w), int(multiple)
    if h < 1 or w < 1 or m < 1:
        raise ValueError("padded_size: h=%d, w=%d, multiple=%d must be positive" % (h, w, m))
    return -(-h // m) * m, -(-w // m) * m


def resolve_layout(frame, layout=None):
    """Checks one frame tensor against `layout` (None: by dtype) and returns (layout, h, w).  No GPU call."""
    if not torch.is_tensor(frame):
        raise ValueError("a frame must be a tensor, got %s" % type(frame).__name__)
    if layout is None:
        layout = 'hwc_rgb' if frame.dtype == torch.uint8 else 'chw'
    if layout not in LAYOUTS:
        raise ValueError("unknown frame layout %r (one of %s)" % (layout, ', '.join(LAYOUTS)))
    if frame.dtype == torch.uint8:
        if layout == 'chw':
            raise ValueError("a uint8 frame is interleaved ('hwc_rgb' / 'hwc_bgr'), not 'chw'")
        if frame.dim() != 3 or frame.shape[2] not in (3, 4):
            raise ValueError("a uint8 frame must be [H,W,3] or [H,W,4], got %s" % (tuple(frame.shape),))
        h, w = int(frame.shape[0]), int(frame.shape[1])
    elif frame.is_floating_point():
        if layout != 'chw':
            raise ValueError("a float frame is planar ('chw'), not %r" % layout)
        if frame.dim() != 3 or frame.shape[0] != 3:
            raise ValueError("a float frame must be [3,H,W], got %s" % (tuple(frame.shape),))
        h, w = int(frame.shape[1]), int(frame.shape[2])
    else:
        raise ValueError("a frame must be uint8 or floating point, got %s" % frame.dtype)
    if h < 1 or w < 1:
        raise ValueError("empty frame %s" % (tuple(frame.shape),))
    return layout, h, w


def check_pad(h, w, Hp, Wp, pad_mode):
    if pad_mode not in _PAD:
        raise ValueError("unknown pad mode %r ('reflect' or 'replicate')" % (pad_mode,))
    if pad_mode == 'reflect' and (Hp - h >= h or Wp - w >= w):
        raise ValueError("a reflect pad of %d x %d is not smaller than the frame %d x %d (use 'replicate')"
                         % (Hp - h, Wp - w, h, w))


def describe(frame, layout):
    """(frame', dvsr_frame_desc) of a tensor that resolve_layout accepted.  A view that the descriptor can express -- any
    offset, any row pitch, a fourth byte per pixel -- is passed by stride; anything else is copied first."""
    if layout == 'chw':
        if frame.dtype != torch.float32:
            frame = frame.float()
        _, h, w = frame.shape
        st = frame.stride()
        if not (st[2] == 1 and st[1] >= w and st[0] >= (h - 1) * st[1] + w):
            frame = frame.contiguous()
            st = frame.stride()
        return frame, L.FrameDesc(_FORMAT[layout], h, w, st[1], st[0], 1)
    h, w, _ = frame.shape
    st = frame.stride()
    if not (st[2] == 1 and st[1] in (3, 4) and st[0] >= w * st[1]):
        frame = frame[:, :, :3].contiguous()
        st = frame.stride()
    return frame, L.FrameDesc(_FORMAT[layout], h, w, st[0], 0, st[1])


def _planar_ok(t):
    return t.is_contiguous() and t.shape[-1] % 4 == 0 and t.data_ptr() % 16 == 0


def ingest(frame, layout=None, multiple=4, pad_mode='reflect', out=None):
    """One frame -> fp32 [3,Hp,Wp] on the GPU, (Hp, Wp) = padded_size(h, w, multiple).

    frame: uint8 [H,W,3|4] ('hwc_rgb' / 'hwc_bgr'; a fourth byte is ignored) or float [3,H,W] ('chw'), on the CPU or the
    GPU; a CPU frame is copied to the device as it is -- 8-bit frames travel as bytes.  out: an fp32 contiguous [3,Hp,Wp]
    GPU tensor to fill (Wp a multiple of 4).  When Wp is not a multiple of 4 (multiple = 1, 2) the result is a
    [3,Hp,Wp] view of a buffer whose rows are."""
    layout, h, w = resolve_layout(frame, layout)
    Hp, Wp = padded_size(h, w, multiple)
    Wb = -(-Wp // 4) * 4
    check_pad(h, w, Hp, Wb, pad_mode)
    if out is not None:
        if not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (3, Hp, Wp) and Wb == Wp):
            raise ValueError("ingest: out must be an fp32 [3,%d,%d] tensor with a width that is a multiple of 4" % (Hp, Wp))
        if not out.is_cuda:
            raise RuntimeError("ingest: out must be on the GPU (libdynavsr_hip); there is no CPU path")
        if not _planar_ok(out):
            raise ValueError("ingest: out must be contiguous and 16-byte aligned")
    dev = out.device if out is not None else (frame.device if frame.is_cuda else torch.device('cuda', torch.cuda.current_device()))
    if not frame.is_cuda:
        frame = frame.to(dev, non_blocking=True)
    frame, desc = describe(frame, layout)
    with torch.cuda.device(dev):
        buf = out if out is not None else torch.empty((3, Hp, Wb), dtype=torch.float32, device=dev)
        L.check(L.lib().dvsr_frame_ingest(frame.data_ptr(), ctypes.byref(desc), buf.data_ptr(), Hp, Wb, _PAD[pad_mode],
                                          L.stream()), "dvsr_frame_ingest")
    return buf if Wb == Wp else buf[:, :, :Wp]


def emit(sr, h, w, layout, min_max=(0, 1), out=None):
    """The top-left h x w crop of sr (fp32 [3,Hs,Ws] or [1,3,Hs,Ws] on the GPU) as uint8 [h,w,3] ('hwc_rgb' / 'hwc_bgr':
    clamp to min_max, rescale, x 255, round half to even -- util.tensor2img's image, and dvsr_frame_metrics') or as fp32
    [3,h,w] ('chw').  out: the tensor to write (any offset and row pitch; what lies outside the crop is not touched).
    A source whose rows are not 16-byte aligned (Ws not a multiple of 4) is copied into one that is, first."""
    if layout not in LAYOUTS:
        raise ValueError("unknown frame layout %r (one of %s)" % (layout, ', '.join(LAYOUTS)))
    if sr.dim() == 4 and sr.shape[0] == 1:
        sr = sr[0]
    if sr.dim() != 3 or sr.shape[0] != 3:
        raise ValueError("emit expects [3,Hs,Ws] or [1,3,Hs,Ws], got %s" % (tuple(sr.shape),))
    Hs, Ws = int(sr.shape[1]), int(sr.shape[2])
    h, w = int(h), int(w)
    if not (1 <= h <= Hs and 1 <= w <= Ws):
        raise ValueError("emit: crop %d x %d outside the frame %d x %d" % (h, w, Hs, Ws))
    if not sr.is_cuda:
        raise RuntimeError("emit runs on the GPU (libdynavsr_hip); there is no CPU path")
    if sr.dtype != torch.float32:
        sr = sr.float()
    if not _planar_ok(sr):
        sr = torch.nn.functional.pad(sr, (0, -Ws % 4)).contiguous()
        Ws = int(sr.shape[2])
    with torch.cuda.device(sr.device):
        if out is None:
            out = (torch.empty((3, h, w), dtype=torch.float32, device=sr.device) if layout == 'chw' else
                   torch.empty((h, w, 3), dtype=torch.uint8, device=sr.device))
        else:
            want = (torch.float32, (3, h, w)) if layout == 'chw' else (torch.uint8, (h, w, 3))
            if out.dtype != want[0] or tuple(out.shape) != want[1] or out.device != sr.device:
                raise ValueError("emit: out must be %s %s on %s" % (want[0], list(want[1]), sr.device))
        dst, desc = describe(out, layout)
        if dst is not out:
            raise ValueError("emit: out must have contiguous pixels and non-overlapping rows")
        L.check(L.lib().dvsr_frame_emit(sr.data_ptr(), Hs, Ws, out.data_ptr(), ctypes.byref(desc), float(min_max[0]),
                                        float(min_max[1]), L.stream()), "dvsr_frame_emit")
    return out
