"""Frames in and out of the video path (csrc/frame_io.hip: dvsr_frame_ingest / dvsr_frame_emit; csrc/frame_yuv.hip:
dvsr_frame_ingest_yuv / dvsr_frame_emit_yuv and their _yuv16 counterparts).

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
'hwc_rgb' for a uint8 one.  video.super_resolve_frames uses these (and engine.StreamPlan.extract_frame, which ingests
straight into the frame cache); they are also the building blocks for feeding padded clips to the adaptation loops by hand.

What a video decoder delivers (ffmpeg rawvideo pipes, PyAV) and an encoder takes is 8-bit YCbCr 4:2:0: the layouts 'nv12'
and 'i420' (yuv420p), never inferred.  Such a frame is PACKED -- one uint8 tensor [H + H/2, W], H and W even: the Y plane
followed by the interleaved CbCr rows (NV12, any row pitch) or by the Cb and the Cr plane (I420, contiguous) -- or a tuple
of PLANES on one device: (y [H,W], uv [Hc,Wc,2]) for NV12, (y, u [Hc,Wc], v [Hc,Wc]) for I420, Hc x Wc = ceil(H/2) x
ceil(W/2), every plane at any offset and row pitch (passed by stride) and H, W of either parity.  `matrix` ('bt601' |
'bt709' | 'bt2020nc') and `yuv_range` ('limited' | 'full') name the conversion; the defaults are the reference's ycbcr2rgb / rgb2ycbcr
(data/util.py:234-299).  ingest gives the un-rounded fp32 RGB, emit goes from fp32 RGB to 4:2:0 bytes in one launch; the
arithmetic is written out in csrc/frame_yuv.hip and DESIGN 3.2k.

High-bit-depth video (HEVC Main10, AV1, VP9 profile 2) decodes to 16-bit little-endian words that hold 10 or 12 bits: the
layouts 'p010' / 'p012' (semi-planar like NV12, the level in the TOP bits of the word) and 'i420p10' / 'i420p12'
(yuv420p10le / yuv420p12le: planar like I420, the level in the LOW bits), never inferred either.  Frames come packed or as
planes exactly as above, as torch.uint16 or torch.int16 tensors (the same bits; numpy and PyAV hand over uint16); the bits of a
word that carry no level are ignored on the way in and written as 0, and emit returns torch.uint16.  The same matrices, ranges,
siting and filters apply with H.273's level scale at that depth, nothing is rounded to 8 bits on the way, and an 8-bit or RGB
source may leave with 10 bits (the same kernels of csrc/frame_yuv.hip on 16-bit samples).

Footage that is not 4:2:0 (the chroma axis of the same kernel pair), never inferred either.  4:2:2 -- ProRes, DNxHR,
XAVC intermediates, capture cards -- has chroma planes Hc x Wc = H x ceil(W/2): 'i422' (yuv422p) and 'nv16', 'i422p10' /
'i422p12' (yuv422p10le / 12le, the level in the low bits) and 'p210' / 'p212' (the level in the top bits); a packed frame is
[2H, W] with W even and any H, the planar form contiguous, the semi-planar one at any pitch.  4:4:4 -- screen recordings, Hi444 /
RExt, animation masters -- has full-size chroma planes: 'i444' (yuv444p), 'i444p10' / 'i444p12' (yuv444p10le / 12le); a packed
frame is [3H, W] at any size and pitch.  Plane tuples are as above with those plane sizes.  Matrices, ranges, level scales and
word conventions are those of the 4:2:0 layout of the same sample kind; 4:2:2 keeps the horizontal chroma filters and has no
vertical one, 4:4:4 has none.  YUV_LAYOUTS / YUV16_LAYOUTS name the 4:2:0 layouts, YUV422_LAYOUTS / YUV444_LAYOUTS these,
ALL_YUV_LAYOUTS all of them.  Not provided: semi-planar 4:4:4 (nv24 / p410), packed 4:2:2 (YUY2 / UYVY / v210), 4:1:1 / 4:4:0,
16-bit YCbCr.

Where the chroma samples sit, and BT.2020, never inferred: `siting` is 'left' (MPEG-2 / H.264, y4m 420mpeg2: on
luma column 2k, midway between rows 2j and 2j+1; the default and what every call without it means), 'center' (JPEG / MPEG-1 /
MJPEG, yuvj420p, y4m 420jpeg: midway both ways) or 'topleft' (HEVC / AV1 UHD and HDR10, chroma_sample_location=topleft: on
column 2k and row 2j).  One siting serves input and output, as `matrix` does.  4:2:2 has no vertical position, so its 'topleft'
is 'left'; for 4:4:4 and every layout that is not YCbCr the name is checked and has no effect.  matrix='bt2020nc' is BT.2020
non-constant luminance (Kr = 0.2627, Kb = 0.0593; H.273 MatrixCoefficients 9), what nearly every 'p010' stream carries.  Not
provided: constant-luminance BT.2020 and ICtCp, transfer functions (PQ / HLG: the network sees the transfer-coded R'G'B' as it
does for SDR), a siting per direction, bottom and interlaced sitings, 420paldv.

RGB above 8 bits and planar integer RGB (RGB_LAYOUTS; csrc/frame_rgb.hip through dvsr_frame_ingest / dvsr_frame_emit),
never inferred from dtype or shape either -- what 16-bit PNG / TIFF / DPX, torchvision's decoders and an FFV1 archive hold:
    'hwc_rgb16' / 'hwc_bgr16'                  uint16 / int16 [H,W,3|4]: rgb48le / bgr48le, with a fourth word rgba64le / bgra64le
                                               (ignored on the way in; an emitted frame has three).  Depth 16.
    'chw_rgb8' / 'chw_gbr8'                    uint8 [3,H,W]: torchvision's decoded image; ffmpeg gbrp (planes G, B, R)
    'chw_rgb10' / 'chw_rgb12' / 'chw_rgb16',   uint16 / int16 [3,H,W]: a 16-bit PNG as torch decodes it; gbrp10le / gbrp12le /
    'chw_gbr10' / 'chw_gbr12' / 'chw_gbr16'    gbrp16le.  The level is in the LOW d bits; higher bits are ignored in, 0 out.
ingest: value = float32(level) / float32(2^d - 1), an IEEE division (depth 8: the v / 255 of 'hwc_rgb', the same bits); emit: the
8-bit quantiser with 255 replaced by 2^d - 1 (clamp to min_max, rescale, x (2^d - 1), round half to even), as torch.uint8 /
torch.uint16 of the layout's shape; emit(ingest(x)) == x.  Interleaved views (any offset, any row pitch, a pixel stride of 3 or 4
words) and planar views (any offset, any row pitch, any plane stride that keeps the planes from overlapping) are passed by stride;
anything else is copied once.  luma_sad takes the top 8 bits of each level; score compares the d-bit levels (channel 'rgb' alone
above 8 bits; a float side is then quantised at that depth); degrade and imresize go through ingest(.., multiple=1) like the
YCbCr layouts.  Not provided: separately allocated planes, rgb24-in-int32 / x2rgb10 / r210 packed words, big-endian words,
float16 / float32 interleaved, an alpha plane or alpha out.

Scene cuts (csrc/frame_cut.hip: dvsr_frame_luma_sad), for any of the layouts above:

    luma_sad(frames, layout)             -> int64 [T-1]: sum over the frame of |Y8_t - Y8_(t-1)|, exact, in one pass on the device
    scene_scores(sad, h, w)              -> float64 [T]: min(mafd_t, |mafd_t - mafd_(t-1)|), mafd = 100 SAD / (255 h w); host code
    detect_cuts(frames, layout, threshold) -> the frames whose score reaches the threshold: the `cuts` of super_resolve_frames

A target output size (csrc/frame_resize.hip: dvsr_frame_resize):

    resize_table(n_in, n_out)            -> (first int32 [n_out], weights fp32 [n_out, taps]) on the CPU: one axis of the resampler
    resize(sr, h, w, (oh, ow))           -> the top-left h x w crop of sr resampled to fp32 [3,oh,ow] on the GPU, one launch
    emit(sr, h, w, layout, size=(oh, ow)) = emit(resize(sr, h, w, (oh, ow)), oh, ow, layout)

The resampler is separable antialiased bicubic, torch.nn.functional.interpolate(.., mode='bicubic', antialias=True,
align_corners=False); per axis n_in / n_out <= 4 and n_out / n_in <= 2.

The flip-test x4 self-ensemble (csrc/frame_flip.hip: dvsr_frame_flip / dvsr_frame_flip_mean):

    flip(x, flags)                       -> fp32 [..., H, W] mirrored in W (flags & 1) and / or H (flags & 2), one launch
    flip_mean(y0, yw, yh, yhw)           -> (((y0 + yw.flip(-1)) + yh.flip(-2)) + yhw.flip((-2, -1))) * 0.25, one launch

Frames in overlapping tiles (csrc/frame_stitch.hip: dvsr_frame_stitch_origins / _cover / _table / dvsr_frame_stitch):

    tile_view(frame, layout, y, x, th, tw) -> the tile's strided view (plane views for YCbCr) that ingest / extract_frame take
    stitch_table(n, tile, overlap, scale) -> (origins [tiles] in SR pixels, first int32 [s n], weights fp32 [s n, K]): one axis
    stitch(tiles, ny, nx, rows, cols)    -> fp32 [..., H, W] from [ny * nx, ..., Ht, Wt]: the seams cross-faded, one launch

PSNR / SSIM against ground truth, RGB or Y (csrc/frame_score.hip: dvsr_frame_score), for any two of the layouts:

    score(a, b, layout_a, layout_b, channel='rgb' | 'y', crop_border=k) -> float64 [mse, ssim] on the device, no host sync
    psnr(mse, peak=255)                  -> 20 log10(peak / sqrt(mse)) on the host, inf at 0

A ground-truth frame degraded as it arrives (csrc/degrade.hip: dvsr_frame_degrade):

    degraded_size(h, w, K, scale)        -> (Hc, Wc, h_lr, w_lr): the crop to a multiple of the scale and the LR size; host code
    degrade(frame, degradation, layout)  -> fp32 [3,h_lr,w_lr] on the GPU: Degradation.apply(.., quantise) of the frame's Hc x Wc
                                            crop, from the frame's own bytes, one launch

MATLAB's imresize(img, scale, 'bicubic') (csrc/frame_imresize.hip: dvsr_frame_imresize_taps / _table / dvsr_frame_imresize;
DESIGN 3.2u) -- the BI degradation imresize(hr, 1 / s) and the "Bicubic" baseline imresize(lr, s); scale is one of 1/2, 1/3,
1/4, 2, 3, 4:

    imresize_size(h, w, scale)           -> (oh, ow) = (ceil(h scale), ceil(w scale)); host code
    imresize_table(n_in, scale)          -> (first int32 [n_out], weights fp32 [n_out, taps]) on the CPU: one axis, folded
    imresize(frame, scale, layout)       -> fp32 [3,oh,ow] on the GPU from the frame's own bytes, one launch
    Imresize(s)                          -> names BI where a degradation is expected: degrade(frame, Imresize(4)) =
                                            imresize(frame, 1/4, quantise=True, modcrop=4)
"""
import ctypes
import numbers

import torch

from . import _lib as L

LAYOUTS = ('chw', 'hwc_rgb', 'hwc_bgr')
_BYTES, _WORDS = (torch.uint8,), (torch.uint16, torch.int16)
# YCbCr layout -> (semi-planar, depth, the format of its descriptor, the format of its Y plane for luma_sad, its dtypes, its
# chroma sub-sampling)
_YUV = {'nv12': (True, 8, L.YUV_NV12, L.FRAME_U8_Y, _BYTES), 'i420': (False, 8, L.YUV_I420, L.FRAME_U8_Y, _BYTES),
        'p010': (True, 10, L.YUV16_SEMI_MSB, L.FRAME_U16_Y_MSB, _WORDS), 'p012': (True, 12, L.YUV16_SEMI_MSB, L.FRAME_U16_Y_MSB, _WORDS),
        'i420p10': (False, 10, L.YUV16_PLANAR_LSB, L.FRAME_U16_Y_10, _WORDS),
        'i420p12': (False, 12, L.YUV16_PLANAR_LSB, L.FRAME_U16_Y_12, _WORDS)}
_YUV = {k: v + (L.YUV_CHROMA_420,) for k, v in _YUV.items()}
YUV_LAYOUTS = tuple(k for k, v in _YUV.items() if v[1] == 8)
YUV16_LAYOUTS = tuple(k for k, v in _YUV.items() if v[1] > 8)
# 4:2:2 and 4:4:4: the 4:2:0 layout of the same sample kind with the chroma field of the format set (4:4:4: planar alone)
for _name, _like, _chroma in (('i422', 'i420', L.YUV_CHROMA_422), ('nv16', 'nv12', L.YUV_CHROMA_422),
                              ('i422p10', 'i420p10', L.YUV_CHROMA_422), ('i422p12', 'i420p12', L.YUV_CHROMA_422),
                              ('p210', 'p010', L.YUV_CHROMA_422), ('p212', 'p012', L.YUV_CHROMA_422),
                              ('i444', 'i420', L.YUV_CHROMA_444), ('i444p10', 'i420p10', L.YUV_CHROMA_444),
                              ('i444p12', 'i420p12', L.YUV_CHROMA_444)):
    _v = _YUV[_like]
    _YUV[_name] = _v[:2] + (L.yuv_format(_v[2], _chroma),) + _v[3:5] + (_chroma,)
YUV422_LAYOUTS = tuple(k for k, v in _YUV.items() if v[5] == L.YUV_CHROMA_422)
YUV444_LAYOUTS = tuple(k for k, v in _YUV.items() if v[5] == L.YUV_CHROMA_444)
ALL_YUV_LAYOUTS = YUV_LAYOUTS + YUV16_LAYOUTS + YUV422_LAYOUTS + YUV444_LAYOUTS
# sub-sampling -> the shape of a packed frame, as the messages write it
_PACKED = {L.YUV_CHROMA_420: '[H*3/2, W]', L.YUV_CHROMA_422: '[2H, W]', L.YUV_CHROMA_444: '[3H, W]'}
_YUV_MATRIX = {'bt601': L.YUV_BT601, 'bt709': L.YUV_BT709, 'bt2020nc': L.YUV_BT2020NC}
# where the chroma samples sit, never inferred: siting -> sub-sampling -> the chroma field of a descriptor's format.
# 4:2:2 has no vertical position, so its 'topleft' is 'left'; 4:4:4 has no siting.
YUV_SITINGS = ('left', 'center', 'topleft')
_YUV_SITING = {'left': {}, 'center': {L.YUV_CHROMA_420: L.YUV_CHROMA_420_CENTER, L.YUV_CHROMA_422: L.YUV_CHROMA_422_CENTER},
               'topleft': {L.YUV_CHROMA_420: L.YUV_CHROMA_420_TOPLEFT}}
_YUV_RANGE = {'limited': L.YUV_LIMITED, 'full': L.YUV_FULL}
_FORMAT = {'chw': L.FRAME_F32_CHW, 'hwc_rgb': L.FRAME_U8_HWC_RGB, 'hwc_bgr': L.FRAME_U8_HWC_BGR}
# integer RGB beyond 8-bit interleaved, never inferred -> (planar, depth, the format of its descriptor, its dtypes)
_RGB = {'hwc_rgb16': (False, 16, L.FRAME_U16_HWC_RGB, _WORDS), 'hwc_bgr16': (False, 16, L.FRAME_U16_HWC_BGR, _WORDS),
        'chw_rgb8': (True, 8, L.FRAME_U8_CHW_RGB, _BYTES), 'chw_gbr8': (True, 8, L.FRAME_U8_CHW_GBR, _BYTES)}
for _d in (10, 12, 16):
    _RGB['chw_rgb%d' % _d] = (True, _d, L.frame_depth(L.FRAME_U16_CHW_RGB, _d), _WORDS)
    _RGB['chw_gbr%d' % _d] = (True, _d, L.frame_depth(L.FRAME_U16_CHW_GBR, _d), _WORDS)
RGB_LAYOUTS = tuple(_RGB)
_FORMAT.update((k, v[2]) for k, v in _RGB.items())
_PAD = {'reflect': L.FRAME_PAD_REFLECT, 'replicate': L.FRAME_PAD_REPLICATE}


def padded_size(h, w, multiple):
    """The smallest (Hp, Wp) >= (h, w) whose sides are multiples of `multiple`."""
    h, w, m = int(h), int(w), int(multiple)
    if h < 1 or w < 1 or m < 1:
        raise ValueError("padded_size: h=%d, w=%d, multiple=%d must be positive" % (h, w, m))
    return -(-h // m) * m, -(-w // m) * m


def is_yuv(layout):
    """`layout` is one of the YCbCr layouts, of any sub-sampling and depth."""
    return layout in ALL_YUV_LAYOUTS


def resolve_layout(frame, layout=None):
    """Checks one frame against `layout` (None: by dtype; the YCbCr layouts are never inferred) and returns
    (layout, h, w).  No GPU call."""
    if is_yuv(layout):
        return (layout,) + yuv_planes(frame, layout)[1:]
    if not torch.is_tensor(frame):
        raise ValueError("a frame must be a tensor, got %s" % type(frame).__name__)
    if layout is None:
        layout = 'hwc_rgb' if frame.dtype == torch.uint8 else 'chw'
    if layout in _RGB:
        planar, _, _, dtypes = _RGB[layout]
        kind = 'uint8' if dtypes is _BYTES else 'uint16 / int16'
        if frame.dtype not in dtypes or frame.dim() != 3 or (frame.shape[0] != 3 if planar else frame.shape[2] not in (3, 4)):
            raise ValueError("a %s frame must be %s %s, got %s %s" % (layout, kind, '[3,H,W]' if planar else '[H,W,3] or [H,W,4]',
                                                                      frame.dtype, tuple(frame.shape)))
        h, w = (int(frame.shape[1]), int(frame.shape[2])) if planar else (int(frame.shape[0]), int(frame.shape[1]))
        if h < 1 or w < 1:
            raise ValueError("empty frame %s" % (tuple(frame.shape),))
        return layout, h, w
    if layout not in LAYOUTS:
        raise ValueError("unknown frame layout %r (one of %s)" % (layout, ', '.join(LAYOUTS + RGB_LAYOUTS + ALL_YUV_LAYOUTS)))
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
    if layout in _RGB:
        return _describe_rgb(frame, layout)
    h, w, _ = frame.shape
    st = frame.stride()
    if not (st[2] == 1 and st[1] in (3, 4) and st[0] >= w * st[1]):
        frame = frame[:, :, :3].contiguous()
        st = frame.stride()
    return frame, L.FrameDesc(_FORMAT[layout], h, w, st[0], 0, st[1])


def _describe_rgb(frame, layout):
    """describe() for the layouts of RGB_LAYOUTS: strides in BYTES, as for the 16-bit Y planes.  Interleaved words: any
    sample-aligned offset and row pitch, a pixel stride of 3 or 4 words.  Planar: any sample-aligned offset, any row pitch, any
    plane stride that keeps the planes from overlapping.  Anything else is copied once."""
    planar, _, fmt, _ = _RGB[layout]
    es, st = frame.element_size(), frame.stride()
    if planar:
        _, h, w = frame.shape
        row = max(int(st[1]), w)
        if not ((st[2] == 1 or w == 1) and (st[1] >= w or h == 1) and st[0] >= (h - 1) * row + w and frame.data_ptr() % es == 0):
            frame = frame.clone(memory_format=torch.contiguous_format)
            st, row = frame.stride(), w
        return frame, L.FrameDesc(fmt, h, w, row * es, int(st[0]) * es, es)
    h, w, _ = frame.shape
    if not (st[2] == 1 and st[1] in (3, 4) and (st[0] >= w * st[1] or h == 1) and frame.data_ptr() % es == 0):
        frame = frame[:, :, :3].clone(memory_format=torch.contiguous_format)
        st = frame.stride()
    return frame, L.FrameDesc(fmt, h, w, max(int(st[0]), w * int(st[1])) * es, 0, int(st[1]) * es)


def check_yuv_names(matrix, yuv_range, siting='left'):
    if matrix not in _YUV_MATRIX:
        raise ValueError("unknown YCbCr matrix %r ('bt601', 'bt709' or 'bt2020nc', BT.2020 non-constant luminance)" % (matrix,))
    if yuv_range not in _YUV_RANGE:
        raise ValueError("unknown YCbCr range %r ('limited' or 'full')" % (yuv_range,))
    if not isinstance(siting, str) or siting not in _YUV_SITING:
        raise ValueError("unknown chroma siting %r ('left', 'center' or 'topleft')" % (siting,))


def chroma_size(layout, h, w):
    """(Hc, Wc) of a chroma plane of an h x w frame: ceil(h/2) x ceil(w/2) (4:2:0), h x ceil(w/2) (4:2:2), h x w (4:4:4)."""
    chroma = _YUV[layout][5]
    return ((h + 1) // 2 if chroma == L.YUV_CHROMA_420 else h), (w if chroma == L.YUV_CHROMA_444 else (w + 1) // 2)


def packed_rows(layout, h):
    """The rows of a packed frame of luma height h: h*3/2 (4:2:0), 2h (4:2:2), 3h (4:4:4)."""
    return {L.YUV_CHROMA_420: h * 3 // 2, L.YUV_CHROMA_422: 2 * h, L.YUV_CHROMA_444: 3 * h}[_YUV[layout][5]]


def packed_needs(layout, h, w):
    """What a packed frame of `layout` asks of h x w and does not get: 'an even size' (4:2:0), 'an even width' (4:2:2), or None
    (4:4:4 packs at any size)."""
    chroma = _YUV[layout][5]
    if chroma == L.YUV_CHROMA_420:
        return 'an even size' if h % 2 or w % 2 else None
    return 'an even width' if chroma == L.YUV_CHROMA_422 and w % 2 else None


def yuv_planes(frame, layout):
    """(planes, h, w) of a YCbCr frame -- a packed tensor ([H*3/2, W] for 4:2:0, [2H, W] for 4:2:2, [3H, W] for 4:4:4) or a tuple
    of plane tensors, uint8 for the 8-bit layouts, uint16 or int16 for the 10- / 12-bit ones: the planes as views (y, uv) /
    (y, u, v), nothing copied.  ValueError for anything else.  No GPU call."""
    if not is_yuv(layout):
        raise ValueError("unknown YCbCr layout %r (one of %s)" % (layout, ', '.join(ALL_YUV_LAYOUTS)))
    semi, depth, _, _, dtypes, chroma = _YUV[layout]
    n, kind = (2 if semi else 3), ('uint8' if depth == 8 else 'uint16 / int16')
    if torch.is_tensor(frame):
        if frame.dtype not in dtypes or frame.dim() != 2:
            raise ValueError("a packed %s frame must be %s %s, got %s %s" % (layout, kind, _PACKED[chroma], frame.dtype,
                                                                             tuple(frame.shape)))
        rows, w = int(frame.shape[0]), int(frame.shape[1])
        if chroma == L.YUV_CHROMA_420:
            h = rows * 2 // 3
            if rows < 3 or rows % 3 or h % 2 or w < 2 or w % 2:
                raise ValueError("a packed %s frame is [H*3/2, W] with H and W even, got %s (pass planes for odd sizes)"
                                 % (layout, tuple(frame.shape)))
        elif chroma == L.YUV_CHROMA_422:
            h = rows // 2
            if rows < 2 or rows % 2 or w < 2 or w % 2:
                raise ValueError("a packed %s frame is [2H, W] with W even, got %s (pass planes for an odd width)"
                                 % (layout, tuple(frame.shape)))
        else:
            h = rows // 3
            if rows < 3 or rows % 3 or w < 1:
                raise ValueError("a packed %s frame is [3H, W], got %s" % (layout, tuple(frame.shape)))
            return (frame[:h], frame[h:2 * h], frame[2 * h:]), h, w         # (three planes of full rows: any pitch)
        hc, wc = chroma_size(layout, h, w)
        if semi:
            return (frame[:h], frame[h:].unflatten(1, (wc, 2))), h, w
        if not frame.is_contiguous():
            raise ValueError("a packed %s frame must be contiguous (its chroma rows are half as long); pass planes" % layout)
        flat, n_c = frame.view(-1), hc * wc
        return (frame[:h], flat[h * w:h * w + n_c].view(hc, wc), flat[h * w + n_c:].view(hc, wc)), h, w
    if not isinstance(frame, (tuple, list)) or len(frame) != n or not all(torch.is_tensor(p) for p in frame):
        raise ValueError("a %s frame is a packed %s tensor or %d plane tensors, got %s" % (
            layout, kind, n, type(frame).__name__ if not isinstance(frame, (tuple, list)) else "%d items" % len(frame)))
    planes = tuple(frame)
    y = planes[0]
    if any(p.dtype not in dtypes for p in planes) or any(p.device != y.device for p in planes):
        raise ValueError("the planes of a %s frame must be %s tensors on one device" % (layout, kind))
    if y.dim() != 2 or y.shape[0] < 1 or y.shape[1] < 1:
        raise ValueError("the Y plane must be [H,W], got %s" % (tuple(y.shape),))
    h, w = int(y.shape[0]), int(y.shape[1])
    want = chroma_size(layout, h, w) + ((2,) if semi else ())
    for p in planes[1:]:
        if tuple(p.shape) != want:
            raise ValueError("a chroma plane of a %d x %d %s frame must be %s, got %s" % (h, w, layout, list(want), tuple(p.shape)))
    return planes, h, w


def describe_yuv(planes, layout, h, w, matrix='bt601', yuv_range='limited', copy=True, siting='left'):
    """(planes', dvsr_yuv_desc) of what yuv_planes returned (a dvsr_yuv16_desc for the 10- / 12-bit layouts; the layout's chroma
    sub-sampling and `siting` are in the descriptor's format).  A plane that the
    descriptor can express -- any offset, any row pitch -- is passed by stride; any other is copied first (copy = False:
    ValueError, for a destination)."""
    check_yuv_names(matrix, yuv_range, siting)
    (_, depth, fmt, _, _, chroma), rest = _YUV[layout], (h, w, _YUV_MATRIX[matrix], _YUV_RANGE[yuv_range])
    fmt = L.yuv_format(fmt & 15, _YUV_SITING[siting].get(chroma, chroma))
    desc = L.Yuv16Desc(fmt, depth, *rest) if depth > 8 else L.YuvDesc(fmt, *rest)
    kept = []
    for i, p in enumerate(planes):
        es = p.element_size()                                           # 1, or 2 for 16-bit words
        row = p.shape[1] * (p.shape[2] if p.dim() == 3 else 1)          # samples of a row
        st = p.stride()
        inner = st[1:] == ((2, 1) if p.dim() == 3 else (1,)) or row == 1
        if not (inner and (st[0] >= row or p.shape[0] == 1) and p.data_ptr() % es == 0):
            if not copy:
                raise ValueError("plane %d must have contiguous rows that do not overlap" % i)
            p = p.clone(memory_format=torch.contiguous_format)
            st = p.stride()
        kept.append(p)
        desc.plane[i] = p.data_ptr()
        desc.row_stride[i] = max(int(st[0]), row) * es                  # bytes
    return tuple(kept), desc


def _yuv_entry(layout, name):
    """The C entry point `name` ('frame_ingest' / 'frame_emit' / 'edvr_stream_extract_frame') of a YCbCr layout."""
    name = "dvsr_%s_%s" % (name, 'yuv16' if _YUV[layout][1] > 8 else 'yuv')
    return getattr(L.lib(), name), name


def to_device(frame, device):
    """A frame (tensor or tuple of planes) on `device`; a CPU frame is copied as it is -- 8-bit frames travel as bytes, 10- and
    12-bit ones as 16-bit words."""
    if torch.is_tensor(frame):
        return frame if frame.is_cuda else frame.to(device, non_blocking=True)
    return tuple(to_device(p, device) for p in frame)


def _planar_ok(t):
    return t.is_contiguous() and t.shape[-1] % 4 == 0 and t.data_ptr() % 16 == 0


def ingest(frame, layout=None, multiple=4, pad_mode='reflect', out=None, matrix='bt601', yuv_range='limited', siting='left'):
    """One frame -> fp32 [3,Hp,Wp] on the GPU, (Hp, Wp) = padded_size(h, w, multiple).

    frame: uint8 [H,W,3|4] ('hwc_rgb' / 'hwc_bgr'; a fourth byte is ignored) or float [3,H,W] ('chw'), on the CPU or the
    GPU; a CPU frame is copied to the device as it is -- 8-bit frames travel as bytes.  out: an fp32 contiguous [3,Hp,Wp]
    GPU tensor to fill (Wp a multiple of 4).  When Wp is not a multiple of 4 (multiple = 1, 2) the result is a
    [3,Hp,Wp] view of a buffer whose rows are.
    'nv12' / 'i420': frame is a packed uint8 [H*3/2, W] tensor or a tuple of planes (module docstring), converted with
    `matrix` / `yuv_range` to un-rounded RGB in [0,1] -- one launch, like the other layouts.  'p010' / 'p012' / 'i420p10' /
    'i420p12': the same for uint16 / int16 words of 10 or 12 bits.  The 4:2:2 and 4:4:4 layouts (module docstring): the same,
    packed [2H, W] / [3H, W] or as planes.  `siting` ('left' | 'center' | 'topleft', module docstring) names where the chroma
    samples of a 4:2:0 / 4:2:2 frame sit; it is checked and has no effect for every other layout.
    RGB_LAYOUTS (module docstring): uint16 / int16 [H,W,3|4] words or uint8 / uint16 / int16 [3,H,W] planes, level / (2^d - 1)."""
    check_yuv_names(matrix, yuv_range, siting)
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
    first = frame if torch.is_tensor(frame) else frame[0]
    dev = out.device if out is not None else (first.device if first.is_cuda else torch.device('cuda', torch.cuda.current_device()))
    frame = to_device(frame, dev)
    yuv = is_yuv(layout)
    if yuv:
        planes, desc = describe_yuv(yuv_planes(frame, layout)[0], layout, h, w, matrix, yuv_range, siting=siting)
    else:
        frame, desc = describe(frame, layout)
    with torch.cuda.device(dev):
        buf = out if out is not None else torch.empty((3, Hp, Wb), dtype=torch.float32, device=dev)
        if yuv:
            fn, name = _yuv_entry(layout, 'frame_ingest')
            L.check(fn(ctypes.byref(desc), buf.data_ptr(), Hp, Wb, _PAD[pad_mode], L.stream()), name)
        else:
            L.check(L.lib().dvsr_frame_ingest(frame.data_ptr(), ctypes.byref(desc), buf.data_ptr(), Hp, Wb, _PAD[pad_mode],
                                              L.stream()), "dvsr_frame_ingest")
    return buf if Wb == Wp else buf[:, :, :Wp]


DEGRADE_MAX_K, DEGRADE_MAX_SCALE = 33, 4      # the limits of dvsr_degrade_apply / dvsr_frame_degrade (csrc/degrade.hip)


def degraded_size(h, w, K, scale):
    """(Hc, Wc, h_lr, w_lr) of an h x w frame degraded with a shifted kernel of edge K at stride `scale`: the frame is cropped
    to Hc x Wc = (h - h % scale) x (w - w % scale), the reference's modcrop (data/util.py:302), reflection-padded by K // 2 and
    correlated at that stride, so h_lr = (Hc + 2 (K // 2) - K) // scale + 1 and w_lr likewise -- Hc / scale for an odd K, one more
    for an even one.  ValueError for what dvsr_frame_degrade refuses: K outside [1, 33], scale outside [1, 4], a frame with no
    multiple of the scale inside, a pad K // 2 that is not smaller than the crop.  Host code."""
    h, w, K, scale = int(h), int(w), int(K), int(scale)
    if not (1 <= K <= DEGRADE_MAX_K and 1 <= scale <= DEGRADE_MAX_SCALE):
        raise ValueError("degraded_size: kernel edge %d (1 .. %d) / scale %d (1 .. %d)" % (K, DEGRADE_MAX_K, scale, DEGRADE_MAX_SCALE))
    Hc, Wc = h - h % scale, w - w % scale
    if Hc < 1 or Wc < 1:
        raise ValueError("degraded_size: a %d x %d frame has no multiple of scale %d inside" % (h, w, scale))
    pad = K // 2
    if pad >= Hc or pad >= Wc:
        raise ValueError("degraded_size: the reflection pad %d of a %d x %d kernel is not smaller than the %d x %d crop of a "
                         "%d x %d frame" % (pad, K, K, Hc, Wc, h, w))
    return Hc, Wc, (Hc + 2 * pad - K) // scale + 1, (Wc + 2 * pad - K) // scale + 1


def degradation_edge(degradation, kernel_index=0, who="degrade"):
    """(K, scale) of a data.random_kernel_generator.Degradation for kernel `kernel_index` of its set (0 for a single [K0,K0]
    kernel): the edge of the shifted kernel and the stride.  ValueError for an index outside the set.  Host code."""
    kernel = degradation.kernel
    n = 1 if kernel.ndim == 2 else int(kernel.shape[0])
    if isinstance(kernel_index, bool) or not isinstance(kernel_index, numbers.Integral) or not 0 <= kernel_index < n:
        raise ValueError("%s: kernel_index=%r outside the degradation's %d kernel%s" % (who, kernel_index, n, "" if n == 1 else "s"))
    return degradation.shifted_edge(int(kernel_index)), int(degradation.scale)


def degrade(frame, degradation, layout=None, *, kernel_index=0, quantise=True, out=None, matrix='bt601', yuv_range='limited',
            siting='left'):
    """One ground-truth frame -> its LR frame, fp32 [3,h_lr,w_lr] on the GPU ((Hc, Wc, h_lr, w_lr) = degraded_size(h, w, K,
    degradation.scale)): Degradation.apply(ingest(frame, multiple=1)[:, :Hc, :Wc].contiguous()[None], quantise)[0] bit for bit,
    in one launch that reads the frame as it is (dvsr_frame_degrade) -- no fp32 copy of the HR frame, no crop.

    frame: anything ingest() takes, on the CPU or the GPU (a CPU frame is copied to the device as it is: 8-bit frames travel as
    bytes).  degradation: a data.random_kernel_generator.Degradation; its shifted kernel (cached per device) is the kernel and
    its `scale` the stride; `kernel_index` picks one of a [T,K0,K0] set.  A data.old_kernel_generator.Degradation is taken the
    same way (its kernel as it is: no shift).  An Imresize(s) is BI instead of a blur: imresize(frame, 1 / s, layout,
    quantise=quantise, modcrop=s), fp32 [3, Hc / s, Wc / s].  quantise: the 8-bit round trip of vsrbase.py:185,
    mul(255).clamp(0, 255).round().div(255), in the same launch -- what an LR video stored as 8-bit images holds.
    RGB / BGR bytes and float planar frames go to the kernel directly, views by stride (nothing is copied); every YCbCr layout
    goes through ingest(.., multiple=1) first -- one extra fp32 HR frame -- and gives the bits of that float frame.
    out: the fp32 [3,h_lr,w_lr] GPU tensor to fill, possibly a view with contiguous columns and rows and planes that do not
    overlap.  Arguments are checked before the first GPU call (ValueError)."""
    check_yuv_names(matrix, yuv_range, siting)
    if isinstance(degradation, Imresize):
        if isinstance(kernel_index, bool) or not isinstance(kernel_index, numbers.Integral) or kernel_index != 0:
            raise ValueError("degrade: kernel_index=%r of an Imresize, which has no kernel set" % (kernel_index,))
        return imresize(frame, (1, degradation.scale), layout, antialiasing=degradation.antialiasing, quantise=quantise,
                        modcrop=degradation.scale, out=out, matrix=matrix, yuv_range=yuv_range, siting=siting)
    layout, h, w = resolve_layout(frame, layout)
    K, scale = degradation_edge(degradation, kernel_index)
    Hc, Wc, hl, wl = degraded_size(h, w, K, scale)
    if out is not None:
        if not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (3, hl, wl)):
            raise ValueError("degrade: out must be an fp32 [3,%d,%d] tensor" % (hl, wl))
        st = out.stride()
        if not ((st[2] == 1 or wl == 1) and (st[1] >= wl or hl == 1) and st[0] >= (hl - 1) * st[1] + wl):
            raise ValueError("degrade: out must have contiguous columns and rows and planes that do not overlap")
        if not out.is_cuda:
            raise RuntimeError("degrade: out must be on the GPU (libdynavsr_hip); there is no CPU path")
    first = frame if torch.is_tensor(frame) else frame[0]
    dev = out.device if out is not None else (first.device if first.is_cuda else torch.device('cuda', torch.cuda.current_device()))
    frame = to_device(frame, dev)
    with torch.cuda.device(dev):
        if is_yuv(layout) or layout in _RGB:
            # (multiple=1 pads nothing but the buffer's rows to 4 floats, which are never read here)
            frame, layout = ingest(frame, layout, 1, 'replicate', matrix=matrix, yuv_range=yuv_range, siting=siting), 'chw'
        frame, desc = describe(frame, layout)
        kernel = degradation._shifted_on(dev)[int(kernel_index)]
        if tuple(kernel.shape) != (K, K):
            raise RuntimeError("degrade: the shifted kernel is %s, shifted_edge() says %d" % (tuple(kernel.shape), K))
        if out is None:
            out = torch.empty((3, hl, wl), dtype=torch.float32, device=dev)
        st = out.stride()
        L.check(L.lib().dvsr_frame_degrade(frame.data_ptr(), ctypes.byref(desc), kernel.data_ptr(), K, scale, out.data_ptr(),
                                           max(int(st[1]), wl), int(st[0]), 1 if quantise else 0, L.stream()),
                "dvsr_frame_degrade")
    return out


IMRESIZE_SCALES = ((1, 2), (1, 3), (1, 4), (2, 1), (3, 1), (4, 1))     # num / den: what dvsr_frame_imresize takes


def imresize_ratio(scale, who="imresize"):
    """(num, den) of a scale: a number within 1e-9 of 1/2, 1/3, 1/4, 2, 3 or 4, or such a pair itself.  ValueError otherwise."""
    if isinstance(scale, (tuple, list)):
        if tuple(scale) in IMRESIZE_SCALES:
            return int(scale[0]), int(scale[1])
    elif isinstance(scale, numbers.Real) and not isinstance(scale, bool):
        for num, den in IMRESIZE_SCALES:
            if abs(float(scale) - num / den) <= 1e-9:
                return num, den
    raise ValueError("%s: scale=%r is not one of 1/2, 1/3, 1/4, 2, 3, 4" % (who, scale))


def imresize_size(h, w, scale):
    """(oh, ow) of MATLAB's imresize of an h x w image: ceil(h scale), ceil(w scale) in integers.  Host code."""
    num, den = imresize_ratio(scale, "imresize_size")
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("imresize_size: h=%d, w=%d must be positive" % (h, w))
    return -(-h * num // den), -(-w * num // den)


def imresize_table(n_in, scale, antialiasing=True):
    """One axis of MATLAB's bicubic imresize, n_in -> ceil(n_in scale) samples: (first int32 [n_out], weights fp32 [n_out, taps])
    CPU tensors from dvsr_frame_imresize_taps / _table -- output i is sum_t weights[i, t] * x[first[i] + t]: the reference's
    calculate_weights_indices evaluated in double, the taps beyond either edge folded back onto the image (MATLAB's symmetric
    copy) and added to the taps they land on; taps = the longest window of the axis, shorter rows zero-padded.  No GPU call."""
    num, den = imresize_ratio(scale, "imresize_table")
    n_in = int(n_in)
    if n_in < 1:
        raise ValueError("imresize_table: n_in=%d must be positive" % n_in)
    n_out = ctypes.c_int()
    taps = L.lib().dvsr_frame_imresize_taps(n_in, num, den, 1 if antialiasing else 0, ctypes.byref(n_out))
    if taps < 1:
        raise ValueError("imresize_table: " + L.lib().dvsr_last_error().decode("utf-8", "replace"))
    first = torch.empty((n_out.value,), dtype=torch.int32)
    weights = torch.empty((n_out.value, taps), dtype=torch.float32)
    L.check(L.lib().dvsr_frame_imresize_table(n_in, num, den, 1 if antialiasing else 0, taps, first.data_ptr(),
                                              weights.data_ptr()), "dvsr_frame_imresize_table")
    return first, weights


_imresize_tables = {}    # (n_in, (num, den), antialiasing, device) -> the table on the device + its dvsr_resize_axis


def _imresize_axis(n_in, ratio, antialiasing, device):
    key = (int(n_in), ratio, bool(antialiasing), str(device))
    hit = _imresize_tables.get(key)
    if hit is None:
        first, weights = imresize_table(n_in, ratio, antialiasing)
        first, weights = first.to(device), weights.to(device)       # (blocking copies: usable from any stream afterwards)
        hit = _imresize_tables[key] = (first, weights, L.ResizeAxis(first.data_ptr(), weights.data_ptr(), int(weights.shape[1])))
    return hit[2]


def imresize(frame, scale, layout=None, *, antialiasing=True, quantise=False, modcrop=None, out=None, matrix='bt601',
             yuv_range='limited', siting='left'):
    """MATLAB's imresize(frame, scale, 'bicubic') -- the reference's data.util.imresize -- of one frame: fp32 [3,oh,ow] on the
    GPU, (oh, ow) = imresize_size(h, w, scale), in one launch that reads the frame as it is (dvsr_frame_imresize).

    frame: anything ingest() takes, on the CPU or the GPU (a CPU frame is copied to the device as it is).  scale: 1/2, 1/3, 1/4
    (with `antialiasing` the kernel is widened by 1 / scale: BI) or 2, 3, 4.  modcrop=m: only the top-left (h - h % m) x
    (w - w % m) of the frame is read, the reference's modcrop, at no cost.  quantise: the 8-bit round trip
    mul(255).clamp(0, 255).round().div(255) in the same launch (round half to even).  RGB / BGR bytes and float planar frames go
    to the kernel directly, views by stride; every YCbCr layout goes through ingest(.., multiple=1) first.  out: the fp32
    [3,oh,ow] GPU tensor to fill, possibly a view with contiguous columns and rows and planes that do not overlap.
    Arguments are checked before the first GPU call (ValueError)."""
    check_yuv_names(matrix, yuv_range, siting)
    ratio = imresize_ratio(scale)
    layout, h, w = resolve_layout(frame, layout)
    if modcrop is not None:
        if isinstance(modcrop, bool) or not isinstance(modcrop, numbers.Integral) or modcrop < 1:
            raise ValueError("imresize: modcrop=%r must be a positive int" % (modcrop,))
        h, w = h - h % modcrop, w - w % modcrop
        if h < 1 or w < 1:
            raise ValueError("imresize: the frame has no multiple of modcrop=%d inside" % modcrop)
    oh, ow = imresize_size(h, w, ratio)
    if out is not None:
        if not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (3, oh, ow)):
            raise ValueError("imresize: out must be an fp32 [3,%d,%d] tensor" % (oh, ow))
        st = out.stride()
        if not ((st[2] == 1 or ow == 1) and (st[1] >= ow or oh == 1) and st[0] >= (oh - 1) * st[1] + ow):
            raise ValueError("imresize: out must have contiguous columns and rows and planes that do not overlap")
        if not out.is_cuda:
            raise RuntimeError("imresize: out must be on the GPU (libdynavsr_hip); there is no CPU path")
    first = frame if torch.is_tensor(frame) else frame[0]
    dev = out.device if out is not None else (first.device if first.is_cuda else torch.device('cuda', torch.cuda.current_device()))
    frame = to_device(frame, dev)
    with torch.cuda.device(dev):
        if is_yuv(layout) or layout in _RGB:
            frame, layout = ingest(frame, layout, 1, 'replicate', matrix=matrix, yuv_range=yuv_range, siting=siting), 'chw'
        frame, desc = describe(frame, layout)
        rows, cols = _imresize_axis(h, ratio, antialiasing, dev), _imresize_axis(w, ratio, antialiasing, dev)
        if out is None:
            out = torch.empty((3, oh, ow), dtype=torch.float32, device=dev)
        st = out.stride()
        L.check(L.lib().dvsr_frame_imresize(frame.data_ptr(), ctypes.byref(desc), h, w, ratio[0], ratio[1], 1 if antialiasing else 0,
                                            out.data_ptr(), max(int(st[1]), ow), max(int(st[0]), (oh - 1) * max(int(st[1]), ow) + ow),
                                            oh, ow, ctypes.byref(rows), ctypes.byref(cols), 1 if quantise else 0, L.stream()),
                "dvsr_frame_imresize")
    return out


class Imresize:
    """BI -- MATLAB's imresize(img, 1 / scale, 'bicubic') -- where degrade(), video.degrade_frames and the evaluate_degraded
    functions expect a degradation: `scale` is the integer down-scale factor (2, 3 or 4), `antialiasing` the reference's."""

    def __init__(self, scale, antialiasing=True):
        if isinstance(scale, bool) or not isinstance(scale, numbers.Integral) or (1, int(scale)) not in IMRESIZE_SCALES:
            raise ValueError("Imresize: scale=%r is not 2, 3 or 4" % (scale,))
        self.scale = int(scale)
        self.antialiasing = bool(antialiasing)

    def __repr__(self):
        return "Imresize(%d, antialiasing=%r)" % (self.scale, self.antialiasing)

    def lr_size(self, h, w):
        """(Hc, Wc, h_lr, w_lr) of an h x w frame: the crop to a multiple of the scale and Hc / scale x Wc / scale."""
        s = self.scale
        Hc, Wc = int(h) - int(h) % s, int(w) - int(w) % s
        if Hc < 1 or Wc < 1:
            raise ValueError("Imresize: a %d x %d frame has no multiple of scale %d inside" % (h, w, s))
        return Hc, Wc, Hc // s, Wc // s


def check_size(size, what="size"):
    """(oh, ow) of a target size: a pair of positive ints, ValueError otherwise.  No GPU call."""
    if isinstance(size, (str, bytes)) or not isinstance(size, (tuple, list, torch.Size)) or len(size) != 2 or \
            any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in size) or size[0] < 1 or size[1] < 1:
        raise ValueError("%s=%r must be a pair of positive ints (oh, ow)" % (what, size))
    return int(size[0]), int(size[1])


def check_resize(h, w, size, what="size"):
    """(oh, ow) of a target size that the resampler takes from h x w (per axis n_in / n_out <= 4 and n_out / n_in <= 2),
    ValueError otherwise.  No GPU call."""
    oh, ow = check_size(size, what)
    for n_in, n_out in ((int(h), oh), (int(w), ow)):
        if n_in < 1 or n_in > 4 * n_out or n_out > 2 * n_in:
            raise ValueError("%s=%r: %d -> %d is outside the accepted ratios (n_in / n_out <= 4, n_out / n_in <= 2) of %d x %d"
                             % (what, tuple(size), n_in, n_out, h, w))
    return oh, ow


def resize_table(n_in, n_out):
    """One axis of the resampler, n_in -> n_out samples: (first int32 [n_out], weights fp32 [n_out, taps]) CPU tensors from
    dvsr_frame_resize_taps / dvsr_frame_resize_table -- output i is sum_t weights[i, t] * x[first[i] + t]; rows shorter than
    taps are zero-padded.  No GPU call."""
    n_in, n_out = int(n_in), int(n_out)
    taps = L.lib().dvsr_frame_resize_taps(n_in, n_out)
    if taps < 1:
        raise ValueError("resize_table: " + L.lib().dvsr_last_error().decode("utf-8", "replace"))
    first = torch.empty((n_out,), dtype=torch.int32)
    weights = torch.empty((n_out, taps), dtype=torch.float32)
    L.check(L.lib().dvsr_frame_resize_table(n_in, n_out, taps, first.data_ptr(), weights.data_ptr()), "dvsr_frame_resize_table")
    return first, weights


_resize_tables = {}      # (n_in, n_out, device) -> (first, weights) on the device + the dvsr_resize_axis that points at them


def _resize_axis(n_in, n_out, device):
    key = (int(n_in), int(n_out), str(device))
    hit = _resize_tables.get(key)
    if hit is None:
        first, weights = resize_table(n_in, n_out)
        first, weights = first.to(device), weights.to(device)       # (blocking copies: usable from any stream afterwards)
        hit = _resize_tables[key] = (first, weights, L.ResizeAxis(first.data_ptr(), weights.data_ptr(), int(weights.shape[1])))
    return hit[2]


def resize_buffer(size, device):
    """The fp32 [3, oh, Wb] buffer that resize() fills, Wb = ow rounded up to a multiple of 4 (its `out`)."""
    oh, ow = check_size(size)
    return torch.empty((3, oh, -(-ow // 4) * 4), dtype=torch.float32, device=device)


def resize(sr, h, w, size, out=None):
    """The top-left h x w crop of sr (fp32 [3,Hs,Ws] or [1,3,Hs,Ws] on the GPU) resampled to size = (oh, ow): fp32
    [3,oh,ow], a view of a contiguous [3,oh,Wb] buffer whose rows are a multiple of 4 floats (columns ow .. Wb-1 are 0) --
    what emit() takes without a copy.  Separable antialiased bicubic, torch.nn.functional.interpolate(crop, size,
    mode='bicubic', antialias=True, align_corners=False) at fp32 rounding; what lies outside the crop is never read.
    out: that buffer (resize_buffer), to fill.  One launch (dvsr_frame_resize); the tables of an axis are built once per
    (n_in, n_out, device) and kept on the device."""
    buf, ow = _resize(sr, h, w, size, out)
    return buf if buf.shape[2] == ow else buf[:, :, :ow]


def _resize(sr, h, w, size, out=None):
    """resize(): (the whole [3,oh,Wb] buffer, ow)."""
    if sr.dim() == 4 and sr.shape[0] == 1:
        sr = sr[0]
    if sr.dim() != 3 or sr.shape[0] != 3:
        raise ValueError("resize expects [3,Hs,Ws] or [1,3,Hs,Ws], got %s" % (tuple(sr.shape),))
    Hs, Ws = int(sr.shape[1]), int(sr.shape[2])
    h, w = int(h), int(w)
    if not (1 <= h <= Hs and 1 <= w <= Ws):
        raise ValueError("resize: crop %d x %d outside the frame %d x %d" % (h, w, Hs, Ws))
    oh, ow = check_resize(h, w, size)
    Wb = -(-ow // 4) * 4
    if out is not None:
        if not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (3, oh, Wb)):
            raise ValueError("resize: out must be an fp32 [3,%d,%d] tensor" % (oh, Wb))
        if out.device != sr.device:
            raise ValueError("resize: out must be on %s" % sr.device)
        if not _planar_ok(out):
            raise ValueError("resize: out must be contiguous and 16-byte aligned")
    if not sr.is_cuda:
        raise RuntimeError("resize runs on the GPU (libdynavsr_hip); there is no CPU path")
    if sr.dtype != torch.float32:
        sr = sr.float()
    if not _planar_ok(sr):
        sr = torch.nn.functional.pad(sr, (0, -Ws % 4)).contiguous()
        Ws = int(sr.shape[2])
    with torch.cuda.device(sr.device):
        rows, cols = _resize_axis(h, oh, sr.device), _resize_axis(w, ow, sr.device)
        buf = out if out is not None else resize_buffer((oh, ow), sr.device)
        L.check(L.lib().dvsr_frame_resize(sr.data_ptr(), Hs, Ws, h, w, buf.data_ptr(), oh, Wb, oh, ow, ctypes.byref(rows),
                                          ctypes.byref(cols), L.stream()), "dvsr_frame_resize")
    return buf, ow


def _flip_operand(x, what):
    """The checks of flip() / flip_mean() on one tensor; no GPU call."""
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() < 2:
        raise ValueError("%s must be an fp32 [..., H, W] tensor, got %s" % (
            what, "%s %s" % (x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x).__name__))
    if x.numel() < 1 or x.shape[-1] % 4:
        raise ValueError("%s: %s must be non-empty with a width that is a multiple of 4" % (what, tuple(x.shape)))
    if not x.is_contiguous() or x.data_ptr() % 16:
        raise ValueError("%s must be contiguous and 16-byte aligned" % what)


def _flip_out(out, like, what):
    if out is None:
        return
    if not (torch.is_tensor(out) and out.dtype == torch.float32 and out.shape == like.shape and out.device == like.device):
        raise ValueError("%s: out must be an fp32 %s tensor on %s" % (what, list(like.shape), like.device))
    if not out.is_contiguous() or out.data_ptr() % 16:
        raise ValueError("%s: out must be contiguous and 16-byte aligned" % what)


def flip(x, flags, out=None):
    """x (fp32 [..., H, W] on the GPU, contiguous, 16-byte aligned, W a multiple of 4) mirrored in W (flags & 1), in H
    (flags & 2), in both (3) or copied (0): torch.flip(x, (-1,)) / (-2,) / (-2, -1), one launch with 16-byte accesses only
    (dvsr_frame_flip).  out: the tensor to fill, of x's shape -- never x itself.  Arguments are checked before the GPU call
    (ValueError)."""
    if isinstance(flags, bool) or not isinstance(flags, numbers.Integral) or not 0 <= flags <= 3:
        raise ValueError("flip: flags=%r (0, or FLIP_W = 1 | FLIP_H = 2)" % (flags,))
    _flip_operand(x, "flip: x")
    _flip_out(out, x, "flip")
    if out is not None and out.data_ptr() == x.data_ptr():
        raise ValueError("flip: out is x (flipping in place is not provided)")
    if not x.is_cuda:
        raise RuntimeError("flip runs on the GPU (libdynavsr_hip); there is no CPU path")
    H, W = int(x.shape[-2]), int(x.shape[-1])
    with torch.cuda.device(x.device):
        if out is None:
            out = torch.empty_like(x)
        L.check(L.lib().dvsr_frame_flip(x.data_ptr(), out.data_ptr(), x.numel() // (H * W), H, W, int(flags), L.stream()),
                "dvsr_frame_flip")
    return out


def flip_mean(y0, yw, yh, yhw, out=None):
    """The mean of the flip-test x4 self-ensemble: y0, yw, yh, yhw are the network's outputs on a clip as it is, mirrored in W,
    in H and in both (fp32 [..., H, W] on one GPU, one shape, contiguous, 16-byte aligned, W a multiple of 4) ->
    (((y0 + yw.flip(-1)) + yh.flip(-2)) + yhw.flip((-2, -1))) * 0.25, the additions in this order: the reference's
    flipx4_forward (utils/util.py:232-254) bit for bit, in one launch that reads each input once (dvsr_frame_flip_mean).
    out: the tensor to fill -- none of the inputs.  Arguments are checked before the GPU call (ValueError)."""
    ys = (y0, yw, yh, yhw)
    for i, y in enumerate(ys):
        _flip_operand(y, "flip_mean: input %d" % i)
        if y.shape != y0.shape or y.device != y0.device:
            raise ValueError("flip_mean: input %d is %s on %s, input 0 is %s on %s" % (i, tuple(y.shape), y.device, tuple(y0.shape),
                                                                                     y0.device))
    _flip_out(out, y0, "flip_mean")
    if out is not None and any(out.data_ptr() == y.data_ptr() for y in ys):
        raise ValueError("flip_mean: out is one of the inputs (averaging in place is not provided)")
    if not y0.is_cuda:
        raise RuntimeError("flip_mean runs on the GPU (libdynavsr_hip); there is no CPU path")
    H, W = int(y0.shape[-2]), int(y0.shape[-1])
    with torch.cuda.device(y0.device):
        if out is None:
            out = torch.empty_like(y0)
        L.check(L.lib().dvsr_frame_flip_mean(y0.data_ptr(), yw.data_ptr(), yh.data_ptr(), yhw.data_ptr(), out.data_ptr(),
                                             y0.numel() // (H * W), H, W, L.stream()), "dvsr_frame_flip_mean")
    return out


def tile_view(frame, layout, y, x, th, tw):
    """The tile [y : min(y + th, h), x : min(x + tw, w)] of a frame that resolve_layout accepts, as a strided view -- or, for a
    YCbCr layout, as the tuple of plane views (packed frames included) -- that ingest / StreamPlan.extract_frame take: nothing
    is copied.  y and x must be even where the layout sub-samples that axis (a tile then starts on a chroma sample; the
    multiples of 4 of video.tile_origins are).  No GPU call."""
    layout, h, w = resolve_layout(frame, layout)
    y, x, th, tw = int(y), int(x), int(th), int(tw)
    if not (0 <= y < h and 0 <= x < w and th >= 1 and tw >= 1):
        raise ValueError("tile_view: a tile of %d x %d at (%d, %d) lies outside the %d x %d frame" % (th, tw, y, x, h, w))
    y1, x1 = min(y + th, h), min(x + tw, w)
    if layout == 'chw' or (layout in _RGB and _RGB[layout][0]):
        return frame[:, y:y1, x:x1]
    if not is_yuv(layout):
        return frame[y:y1, x:x1]
    chroma = _YUV[layout][5]
    sy, sx = (2 if chroma == L.YUV_CHROMA_420 else 1), (1 if chroma == L.YUV_CHROMA_444 else 2)
    if y % sy or x % sx:
        raise ValueError("tile_view: a %s tile must start on a chroma sample, got (%d, %d)" % (layout, y, x))
    planes = yuv_planes(frame, layout)[0]
    cy0, cy1, cx0, cx1 = y // sy, -(-y1 // sy), x // sx, -(-x1 // sx)
    return (planes[0][y:y1, x:x1],) + tuple(p[cy0:cy1, cx0:cx1] for p in planes[1:])


def stitch_table(n, tile, overlap, scale):
    """One axis of the tile grid and its blend weights: (origins int32 [tiles] in SR pixels, first int32 [scale * n], weights fp32
    [scale * n, K]) CPU tensors from dvsr_frame_stitch_origins / _cover / _table -- n the padded length in LR pixels, tile and
    overlap as video.tile_origins takes them; SR position r is sum_a weights[r, a] * tile(first[r] + a) at r - origins[first[r]
    + a]; rows with fewer covering tiles than K are zero-padded.  No GPU call."""
    n, tile, overlap, scale = int(n), int(tile), int(overlap), int(scale)
    lib = L.lib()
    count = lib.dvsr_frame_stitch_origins(n, tile, overlap, None, 0)
    if count < 1:
        raise ValueError("stitch_table: " + lib.dvsr_last_error().decode("utf-8", "replace"))
    if not 1 <= scale <= 16:
        raise ValueError("stitch_table: scale=%d outside [1, 16]" % scale)
    arr = (ctypes.c_int * count)()
    lib.dvsr_frame_stitch_origins(n, tile, overlap, arr, count)
    cover = lib.dvsr_frame_stitch_cover(n, tile, overlap)
    origins = torch.tensor([scale * o for o in arr], dtype=torch.int32)
    first = torch.empty((scale * n,), dtype=torch.int32)
    weights = torch.empty((scale * n, cover), dtype=torch.float32)
    L.check(lib.dvsr_frame_stitch_table(n, tile, overlap, scale, cover, first.data_ptr(), weights.data_ptr()),
            "dvsr_frame_stitch_table")
    return origins, first, weights


_stitch_axes = {}      # (device, the table's bytes) -> the table on the device + the dvsr_stitch_axis that points at it


def _stitch_axis(table, device):
    origins, first, weights = table
    if not (all(torch.is_tensor(t) for t in table) and origins.dtype == torch.int32 and first.dtype == torch.int32 and
            weights.dtype == torch.float32 and origins.dim() == 1 and first.dim() == 1 and weights.dim() == 2 and
            origins.numel() >= 1 and weights.shape[0] == first.shape[0] and 1 <= weights.shape[1] <= 3):
        raise ValueError("stitch: an axis is stitch_table's (origins int32 [tiles], first int32 [N], weights fp32 [N, K <= 3])")
    host = tuple(t.cpu().contiguous() for t in table)
    key = (str(device),) + tuple(t.numpy().tobytes() for t in host)
    hit = _stitch_axes.get(key)
    if hit is None:
        dev = tuple(t.to(device) for t in host)                     # (blocking copies: usable from any stream afterwards)
        hit = _stitch_axes[key] = (dev, L.StitchAxis(dev[1].data_ptr(), dev[2].data_ptr(), dev[0].data_ptr(), int(weights.shape[1])),
                                   (ctypes.c_int * origins.numel())(*host[0].tolist()))
    return hit


def stitch(tiles, ny, nx, rows, cols, out=None):
    """SR tiles -> the SR frame, the seams blended (dvsr_frame_stitch, one launch with 16-byte accesses only).

    tiles: fp32 [ny * nx, ..., Ht, Wt] on the GPU, contiguous, 16-byte aligned, tile (iy, ix) at index iy * nx + ix; rows, cols:
    stitch_table's result for the two axes (their tables are copied to the device once per content and kept).  Returns fp32
    [..., H, W], H = len(rows' first), W = len(cols' first):
        out[..., r, c] = sum_a sum_b (wy[r, a] * wx[c, b]) * tiles[(first_y[r] + a) * nx + first_x[c] + b][..., r - O_y, c - O_x]
    a outer, b inner, in fp32, never contracted, the accumulator starting as the first term; a zero weight is neither read nor
    added.  out: the tensor to fill -- it must not overlap tiles.  Arguments are checked before the GPU call (ValueError)."""
    ny, nx = int(ny), int(nx)
    if not torch.is_tensor(tiles) or tiles.dtype != torch.float32 or tiles.dim() < 3:
        raise ValueError("stitch: tiles must be an fp32 [ny * nx, ..., Ht, Wt] tensor, got %s" % (
            "%s %s" % (tiles.dtype, tuple(tiles.shape)) if torch.is_tensor(tiles) else type(tiles).__name__))
    if ny < 1 or nx < 1 or tiles.shape[0] != ny * nx or tiles.numel() < 1:
        raise ValueError("stitch: %s is not %d x %d tiles" % (tuple(tiles.shape), ny, nx))
    Ht, Wt = int(tiles.shape[-2]), int(tiles.shape[-1])
    if not tiles.is_contiguous() or tiles.data_ptr() % 16:
        raise ValueError("stitch: tiles must be contiguous and 16-byte aligned")
    for name, table, tl, cnt in (("rows", rows, Ht, ny), ("cols", cols, Wt, nx)):
        if not isinstance(table, (tuple, list)) or len(table) != 3:
            raise ValueError("stitch: %s must be stitch_table's (origins, first, weights)" % name)
    H, W = int(rows[1].shape[0]), int(cols[1].shape[0])
    shape = tuple(tiles.shape[1:-2]) + (H, W)
    planes = tiles.numel() // (ny * nx * Ht * Wt)
    if Ht % 4 or Wt % 4 or H % 4 or W % 4 or Ht > H or Wt > W or H > 65535 or planes > 65535:
        raise ValueError("stitch: tiles of %d x %d into %d x %d (multiples of 4, a tile no larger than the frame, at most 65535 "
                         "rows and planes)" % (Ht, Wt, H, W))
    for name, table, tl, cnt, N in (("rows", rows, Ht, ny, H), ("cols", cols, Wt, nx, W)):
        o = [int(v) for v in table[0].tolist()]
        ok = len(o) == cnt and o[0] == 0 and o[-1] == N - tl and all(v % 4 == 0 for v in o) and \
            all(0 < b - a <= tl for a, b in zip(o[:-1], o[1:]))
        if not ok:
            raise ValueError("stitch: the origins %s of %s do not tile %d with %d tiles of %d" % (o, name, N, cnt, tl))
    if out is not None:
        if not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == shape and out.device == tiles.device):
            raise ValueError("stitch: out must be an fp32 %s tensor on %s" % (list(shape), tiles.device))
        if not out.is_contiguous() or out.data_ptr() % 16:
            raise ValueError("stitch: out must be contiguous and 16-byte aligned")
        a0, b0 = tiles.data_ptr(), out.data_ptr()
        if a0 < b0 + out.numel() * 4 and b0 < a0 + tiles.numel() * 4:
            raise ValueError("stitch: out overlaps tiles (stitching in place is not provided)")
    if not tiles.is_cuda:
        raise RuntimeError("stitch runs on the GPU (libdynavsr_hip); there is no CPU path")
    with torch.cuda.device(tiles.device):
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=tiles.device)
        _stitch_run(tiles, ny, nx, _stitch_axis(rows, tiles.device), _stitch_axis(cols, tiles.device), out)
    return out


def _stitch_run(tiles, ny, nx, rows, cols, out):
    """stitch() behind its checks, on the current device and stream; rows, cols: what _stitch_axis returned (adapt.
    super_resolve_frames prepares them once per video)."""
    Ht, Wt, H, W = int(tiles.shape[-2]), int(tiles.shape[-1]), int(out.shape[-2]), int(out.shape[-1])
    L.check(L.lib().dvsr_frame_stitch(tiles.data_ptr(), ny, nx, tiles.numel() // (ny * nx * Ht * Wt), Ht, Wt, out.data_ptr(), H, W,
                                      ctypes.byref(rows[1]), ctypes.byref(cols[1]), rows[2], cols[2], L.stream()),
            "dvsr_frame_stitch")


def emit(sr, h, w, layout, min_max=(0, 1), out=None, matrix='bt601', yuv_range='limited', size=None, siting='left'):
    """The top-left h x w crop of sr (fp32 [3,Hs,Ws] or [1,3,Hs,Ws] on the GPU) as uint8 [h,w,3] ('hwc_rgb' / 'hwc_bgr':
    clamp to min_max, rescale, x 255, round half to even -- util.tensor2img's image, and dvsr_frame_metrics') or as fp32
    [3,h,w] ('chw').  out: the tensor to write (any offset and row pitch; what lies outside the crop is not touched).
    A source whose rows are not 16-byte aligned (Ws not a multiple of 4) is copied into one that is, first.
    'nv12' / 'i420': the crop as YCbCr 4:2:0 bytes (`matrix`, `yuv_range`, `siting` -- where the chroma samples are to sit,
    module docstring; chroma filtered inside the crop alone).  With h and
    w even and no `out` the result is a packed uint8 [h*3/2, w] tensor; otherwise `out` is a packed tensor of that shape or a
    tuple of planes (module docstring; needed for an odd h or w) and is returned; bytes outside the planes' rows are not
    touched.  'p010' / 'p012' / 'i420p10' / 'i420p12': the same as 10- / 12-bit words, a packed torch.uint16 [h*3/2, w] tensor
    (`out`: uint16 or int16); the bits of a word that carry no level are written as 0.
    The 4:2:2 layouts: packed [2h, w], which needs an even w alone; the 4:4:4 layouts: packed [3h, w] at any size.
    RGB_LAYOUTS: the crop as torch.uint16 [h,w,3] words ('hwc_rgb16' / 'hwc_bgr16') or as torch.uint8 / torch.uint16 [3,h,w] planes
    of d-bit levels ('chw_*'): clamp to min_max, rescale, x (2^d - 1), round half to even; `out`: such a tensor (int16 too), any
    offset, row pitch and plane stride.
    size = (oh, ow): the crop is first resampled to oh x ow (resize(): one more launch into a buffer of its own), and
    everything above holds for the oh x ow image -- emit(resize(sr, h, w, size), oh, ow, layout, ...), bit for bit."""
    if layout not in LAYOUTS + RGB_LAYOUTS and not is_yuv(layout):
        raise ValueError("unknown frame layout %r (one of %s)" % (layout, ', '.join(LAYOUTS + RGB_LAYOUTS + ALL_YUV_LAYOUTS)))
    check_yuv_names(matrix, yuv_range, siting)
    if size is not None:
        oh, ow = check_resize(h, w, size)
        if is_yuv(layout) and out is None and packed_needs(layout, oh, ow):
            raise ValueError("emit: a packed %s frame needs %s, got %d x %d: pass `out` as planes"
                             % (layout, packed_needs(layout, oh, ow), oh, ow))
        # (the whole buffer goes on: its rows are 16-byte aligned, those of resize()'s view are not when ow % 4)
        return emit(_resize(sr, h, w, (oh, ow))[0], oh, ow, layout, min_max, out, matrix, yuv_range, siting=siting)
    if sr.dim() == 4 and sr.shape[0] == 1:
        sr = sr[0]
    if sr.dim() != 3 or sr.shape[0] != 3:
        raise ValueError("emit expects [3,Hs,Ws] or [1,3,Hs,Ws], got %s" % (tuple(sr.shape),))
    Hs, Ws = int(sr.shape[1]), int(sr.shape[2])
    h, w = int(h), int(w)
    if not (1 <= h <= Hs and 1 <= w <= Ws):
        raise ValueError("emit: crop %d x %d outside the frame %d x %d" % (h, w, Hs, Ws))
    if is_yuv(layout):
        if out is None and packed_needs(layout, h, w):
            raise ValueError("emit: a packed %s frame needs %s, got %d x %d: pass `out` as planes"
                             % (layout, packed_needs(layout, h, w), h, w))
        if out is not None:
            planes, ho, wo = yuv_planes(out, layout)
            if (ho, wo) != (h, w):
                raise ValueError("emit: out is a %d x %d frame, the crop is %d x %d" % (ho, wo, h, w))
            if planes[0].device != sr.device:
                raise ValueError("emit: out must be on %s" % sr.device)
    if layout in _RGB:
        planar, _, _, dtypes = _RGB[layout]
        shape = (3, h, w) if planar else (h, w, 3)
        if not float(min_max[1]) > float(min_max[0]):
            raise ValueError("emit: min_max=%r needs hi > lo" % (min_max,))
        if out is not None:
            if not torch.is_tensor(out) or out.dtype not in dtypes or tuple(out.shape) != shape or out.device != sr.device:
                raise ValueError("emit: out must be %s %s on %s" % (' / '.join(str(d) for d in dtypes), list(shape), sr.device))
            if describe(out, layout)[0] is not out or (not planar and out.stride(1) != 3):
                raise ValueError("emit: out must have contiguous samples, a pixel stride of 3 words (an emitted frame has no "
                                 "fourth word) and rows and planes that do not overlap")
    if not sr.is_cuda:
        raise RuntimeError("emit runs on the GPU (libdynavsr_hip); there is no CPU path")
    if sr.dtype != torch.float32:
        sr = sr.float()
    if not _planar_ok(sr):
        sr = torch.nn.functional.pad(sr, (0, -Ws % 4)).contiguous()
        Ws = int(sr.shape[2])
    if is_yuv(layout):
        with torch.cuda.device(sr.device):
            if out is None:
                out = torch.empty((packed_rows(layout, h), w), dtype=_YUV[layout][4][0], device=sr.device)
                planes = yuv_planes(out, layout)[0]
            _, desc = describe_yuv(planes, layout, h, w, matrix, yuv_range, copy=False, siting=siting)
            fn, name = _yuv_entry(layout, 'frame_emit')
            L.check(fn(sr.data_ptr(), Hs, Ws, ctypes.byref(desc), float(min_max[0]), float(min_max[1]), L.stream()), name)
        return out
    with torch.cuda.device(sr.device):
        if layout in _RGB:
            if out is None:
                out = torch.empty(shape, dtype=dtypes[0], device=sr.device)
        elif out is None:
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


def _luma_part(frame, layout):
    """The tensor of a frame that carries its luma: the Y plane of a 4:2:0 frame (a view), the frame itself otherwise."""
    if is_yuv(layout):
        return yuv_planes(frame, layout)[0][0]
    return frame if layout != 'chw' or frame.dtype == torch.float32 else frame.float()


def _describe_luma(x, layout):
    """(x', the fields of its dvsr_frame_desc) of what _luma_part returned; a view that the descriptor cannot express is
    copied first."""
    if is_yuv(layout):
        h, w = x.shape
        es = x.element_size()
        st = x.stride()
        if not ((st[1] == 1 or w == 1) and (st[0] >= w or h == 1) and x.data_ptr() % es == 0):
            x = x.clone(memory_format=torch.contiguous_format)
            st = x.stride()
        return x, (_YUV[layout][3], h, w, max(int(st[0]), w) * es, 0, es)
    x, d = describe(x, layout)
    return x, (d.format, d.h, d.w, d.row_stride, d.plane_stride, d.pixel_stride)


def _luma_sad_launch(a, b, fields, frame_stride, pairs, sad):
    desc = L.FrameDesc(*fields)
    L.check(L.lib().dvsr_frame_luma_sad(a.data_ptr(), b.data_ptr(), ctypes.byref(desc), int(frame_stride), int(pairs),
                                        sad.data_ptr(), L.stream()), "dvsr_frame_luma_sad")


def luma_sad(frames, layout=None):
    """SAD_t = sum over the h x w frame of |Y8_t(p) - Y8_(t-1)(p)| for t = 1 .. T - 1, as an int64 CPU tensor [T - 1].

    `frames` is what video.super_resolve_frames accepts: a [T,...] tensor or a list of frames of one kind and size, on the CPU
    or the GPU, in any `layout` (None: by dtype).  Y8, the luma of a pixel, is an 8-bit integer: the Y-plane byte of an
    'nv12' / 'i420' frame as it is (`matrix` and `yuv_range` play no part), the top 8 bits of the level of a 10- / 12-bit
    Y-plane word (so that scores and thresholds mean what they mean for 8-bit video), (77 R + 150 G + 29 B + 128) >> 8 of an
    8-bit RGB / BGR pixel or of the top 8 bits of the levels of a pixel of RGB_LAYOUTS, and the same formula on the 8-bit
    values emit() would write (clamp to [0,1], x 255, round half to
    even) of a float frame.  The sums are exact.
    A video tensor on the GPU is one launch over all pairs; a list takes one launch per pair.  CPU frames travel as bytes
    (the Y plane alone of a 4:2:0 frame) through two staging buffers on the device, so a long video is never resident as a
    whole.  One device-to-host copy at the end carries the sums."""
    T = len(frames)
    if T < 1:
        raise ValueError("luma_sad: no frames")
    lay, h, w = resolve_layout(frames[0], layout)
    first = _luma_part(frames[0], lay)
    dev = first.device if first.is_cuda else torch.device('cuda', torch.cuda.current_device())
    if T == 1:
        return torch.zeros((0,), dtype=torch.int64)
    with torch.cuda.device(dev):
        sad = torch.empty((T - 1,), dtype=torch.int64, device=dev)
        if torch.is_tensor(frames) and frames.is_cuda:
            video = frames if lay != 'chw' or frames.dtype == torch.float32 else frames.float()
            for attempt in (0, 1):
                p0, p1 = _luma_part(video[0], lay), _luma_part(video[1], lay)
                (x0, d0), (x1, d1) = _describe_luma(p0, lay), _describe_luma(p1, lay)
                step = x1.data_ptr() - x0.data_ptr()
                if x0.data_ptr() == p0.data_ptr() and x1.data_ptr() == p1.data_ptr() and d0 == d1 and \
                        step == video.stride(0) * video.element_size():
                    break
                if attempt:
                    raise RuntimeError("luma_sad: a contiguous video must be expressible by stride")
                video = video.contiguous()                 # (a view the descriptor cannot express)
            # (the frame stride in the descriptor's units: floats for 'chw', bytes for everything else)
            _luma_sad_launch(x0, x1, d0, video.stride(0) * (1 if lay == 'chw' else video.element_size()), T - 1, sad)
            return sad.cpu()
        stage, prev, kind = [None, None], None, None
        for t in range(T):
            ht, wt = resolve_layout(frames[t], lay)[1:]
            if (ht, wt) != (h, w):
                raise ValueError("luma_sad: frame %d is %d x %d, frame 0 is %d x %d" % (t, ht, wt, h, w))
            x = _luma_part(frames[t], lay)
            if kind is None:
                kind = (x.dtype, tuple(x.shape))
            if (x.dtype, tuple(x.shape)) != kind:
                raise ValueError("luma_sad: frame %d is %s, frame 0 is %s" % (t, (x.dtype, tuple(x.shape)), kind))
            if x.device != dev:
                if stage[t % 2] is None:
                    stage[t % 2] = torch.empty(x.shape, dtype=x.dtype, device=dev)
                stage[t % 2].copy_(x, non_blocking=True)    # (behind the launch that last read this buffer, on one stream)
                x = stage[t % 2]
            cur = _describe_luma(x, lay)
            if prev is not None:
                a, b = prev, cur
                if a[1] != b[1]:                            # two views of different pitch: one descriptor serves copies
                    a, b = _describe_luma(a[0].contiguous(), lay), _describe_luma(b[0].contiguous(), lay)
                _luma_sad_launch(a[0], b[0], a[1], 0, 1, sad[t - 1:])
            prev = cur
        return sad.cpu()


_SCORE_CHANNEL = {'rgb': L.SCORE_RGB, 'y': L.SCORE_Y}
SCORE_MAX_SIDE = 32768


def layout_depth(layout):
    """The bits of a sample of `layout`: 10 or 12 for the 16-bit YCbCr layouts, 8, 10, 12 or 16 for those of RGB_LAYOUTS, 8 for
    everything else (a float frame is scored as the 8-bit image emit() would write, or under channel='rgb' as the image of the
    other side's depth)."""
    if layout in _RGB:
        return _RGB[layout][1]
    return _YUV[layout][1] if is_yuv(layout) else 8


def check_score(side_a, side_b, channel='rgb', crop_border=0, min_max=(0, 1), who="score"):
    """The checks of score() on two sides given as (layout, h, w), the layouts resolved: ValueError for everything
    dvsr_frame_score refuses.  Returns (lo, hi, depth).  No GPU call."""
    (la, ha, wa), (lb, hb, wb) = side_a, side_b
    if channel not in _SCORE_CHANNEL:
        raise ValueError("%s: channel=%r ('rgb' or 'y')" % (who, channel))
    if isinstance(crop_border, bool) or not isinstance(crop_border, numbers.Integral) or crop_border < 0:
        raise ValueError("%s: crop_border=%r must be an int >= 0" % (who, crop_border))
    try:
        lo, hi = (float(v) for v in min_max)
    except (TypeError, ValueError):
        raise ValueError("%s: min_max=%r must be a pair (lo, hi)" % (who, min_max))
    if not hi > lo:
        raise ValueError("%s: min_max=%r needs hi > lo" % (who, min_max))
    if (ha, wa) != (hb, wb):
        raise ValueError("%s: frame a is %d x %d, frame b is %d x %d" % (who, ha, wa, hb, wb))
    if ha > SCORE_MAX_SIDE or wa > SCORE_MAX_SIDE:
        raise ValueError("%s: frames of %d x %d (at most %d a side)" % (who, ha, wa, SCORE_MAX_SIDE))
    if ha - 2 * crop_border < 1 or wa - 2 * crop_border < 1:
        raise ValueError("%s: crop_border=%d leaves nothing of %d x %d" % (who, crop_border, ha, wa))
    for lay in (la, lb):
        if channel == 'rgb' and is_yuv(lay):
            raise ValueError("%s: channel='rgb' on the Y plane of a %s frame (use channel='y')" % (who, lay))
        if channel == 'y' and lay in _RGB and layout_depth(lay) > 8:
            raise ValueError("%s: channel='y' on a %d-bit RGB frame (%s): the reference defines no Y from RGB at that depth "
                             "(use channel='rgb')" % (who, layout_depth(lay), lay))
    da, db = layout_depth(la), layout_depth(lb)
    if channel == 'rgb':                               # an fp32 side is quantised at the other side's depth
        da, db = (db if la == 'chw' else da), (da if lb == 'chw' else db)
    if da != db:
        raise ValueError("%s: %s has %d-bit samples, %s has %d-bit samples: scoring at mixed bit depths is not provided"
                         % (who, la, da, lb, db))
    return lo, hi, da


def _check_score_out(out, who="score"):
    if out is None:
        return
    if not (torch.is_tensor(out) and out.dtype == torch.float64 and tuple(out.shape) == (2,) and out.is_contiguous()):
        raise ValueError("%s: out must be a contiguous float64 [2] tensor" % who)
    if not out.is_cuda:
        raise ValueError("%s: out must be on the GPU" % who)


def score(a, b, layout_a=None, layout_b=None, *, channel='rgb', crop_border=0, min_max=(0, 1), out=None):
    """[mse, ssim] of frame `a` against frame `b` as a float64 [2] tensor on the device (or written into `out`), without a
    host synchronisation: what the reference's evaluation scripts compute per frame -- tensor2img, optionally
    bgr2ycbcr(only_y=True) (channel='y', the Vid4 protocol), util.crop_border(crop_border), calculate_psnr's mean squared
    difference and calculate_ssim -- for two frames in the formats they come in (csrc/frame_score.hip: dvsr_frame_score, one
    tile launch and one finalize launch on the current stream).

    a, b: frames in any layout ingest / luma_sad take, each with its own (`layout_a`, `layout_b`; None: by dtype, the 4:2:0
    layouts are never inferred), on the CPU or the GPU, of one size; views are passed by stride, CPU frames go to the device as
    bytes (the Y plane alone of a 4:2:0 frame).  Samples: channel='rgb' compares the three 8-bit values of a pixel -- the bytes
    of a uint8 frame in RGB order, emit()'s quantisation (clamp to `min_max`, rescale, x 255, round half to even) of a float
    frame; channel='y' compares one: Y8 = (65.481 R + 128.553 G + 24.966 B) / 255 + 16 of those, rounded half to even
    (evaluated exactly in integers), the byte of the Y plane of an 'nv12' / 'i420' frame (packed or planes), or the 10- / 12-bit
    level of the Y plane of a 16-bit layout.  Both frames must have samples of one depth.  mse is the exact integer sum of
    squared differences over the crop divided once; ssim uses L = 255 (or 2^d - 1) and is NaN when the crop has no valid region
    (a side <= 10).  psnr(mse) converts on the host.  ValueError before the first GPU call for every bad argument.
    RGB_LAYOUTS: channel='rgb' compares the d-bit levels in RGB order (L = 2^d - 1; a float frame on the other side is quantised
    at that depth), channel='y' is defined at 8 bits alone ('chw_rgb8' / 'chw_gbr8'), and both sides hold one depth."""
    la, ha, wa = resolve_layout(a, layout_a)
    lb, hb, wb = resolve_layout(b, layout_b)
    lo, hi, depth = check_score((la, ha, wa), (lb, hb, wb), channel, crop_border, min_max)
    _check_score_out(out)
    pa, pb = _luma_part(a, la), _luma_part(b, lb)
    dev = out.device if out is not None else next((p.device for p in (pa, pb) if p.is_cuda),
                                                   torch.device('cuda', torch.cuda.current_device()))
    for p in (pa, pb):
        if p.is_cuda and p.device != dev:
            raise ValueError("score: the frames and out must be on one device, got %s and %s" % (p.device, dev))
    with torch.cuda.device(dev):
        (xa, fa), (xb, fb) = _describe_luma(to_device(pa, dev), la), _describe_luma(to_device(pb, dev), lb)
        if out is None:
            out = torch.empty((2,), dtype=torch.float64, device=dev)
        k = int(crop_border)
        nbytes = L.lib().dvsr_frame_score_workspace_bytes(3 if channel == 'rgb' else 1, ha - 2 * k, wa - 2 * k)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        da, db = L.FrameDesc(*fa), L.FrameDesc(*fb)
        args = L.ScoreArgs(_SCORE_CHANNEL[channel], k, depth, lo, hi)
        L.check(L.lib().dvsr_frame_score(xa.data_ptr(), ctypes.byref(da), xb.data_ptr(), ctypes.byref(db), ctypes.byref(args),
                                         out.data_ptr(), ws.data_ptr(), nbytes, L.stream()), "dvsr_frame_score")
    return out


def psnr(mse, peak=255):
    """20 log10(peak / sqrt(mse)) of a mean squared difference (a number, or a one-element tensor: that is a device-to-host
    copy), inf at 0 like the reference's calculate_psnr.  peak: 255, or 2^d - 1 for d-bit samples."""
    import math
    mse = float(mse)
    return float('inf') if mse == 0 else 20 * math.log10(float(peak) / math.sqrt(mse))


def scene_scores(sad, h, w):
    """The scene-change score of every frame, float64 [T], from luma_sad's [T - 1] sums -- pure host code.
    mafd_t = 100 * SAD_t / (255 h w) for t = 1 .. T - 1 (the mean absolute luma difference in percent of full scale),
    mafd_0 = 0, and score_t = min(mafd_t, |mafd_t - mafd_(t-1)|): the form of the score of ffmpeg's scene-change filter.
    The min with the CHANGE of the difference keeps sustained fast motion from reading as a cut."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("scene_scores: h=%d, w=%d must be positive" % (h, w))
    sad = torch.as_tensor(sad).to(torch.float64).reshape(-1)
    mafd = torch.cat([torch.zeros(1, dtype=torch.float64), 100.0 * sad / (255.0 * h * w)])
    prev = torch.cat([torch.zeros(1, dtype=torch.float64), mafd[:-1]])
    return torch.minimum(mafd, (mafd - prev).abs())


def detect_cuts(frames, layout=None, threshold=10.0):
    """The hard cuts of a video: the list of t with scene_scores(luma_sad(frames, layout))[t] >= threshold, frame t being
    the first of a new scene -- the `cuts` of video.super_resolve_frames.  The default threshold is a policy default that
    callers override; it has not been tuned on real footage.  Fades and dissolves are not found."""
    threshold = float(threshold)
    if not threshold > 0:
        raise ValueError("detect_cuts: threshold=%r must be positive" % (threshold,))
    if len(frames) < 1:
        raise ValueError("detect_cuts: no frames")
    _, h, w = resolve_layout(frames[0], layout)
    scores = scene_scores(luma_sad(frames, layout), h, w)
    return [t for t in range(1, len(scores)) if float(scores[t]) >= threshold]
