"""The YCbCr 4:2:2 and 4:4:4 arithmetic of csrc/frame_yuv.hip restated in fp64 numpy: the yardstick of
test_yuv_chroma_host.py and test_gpu_yuv_chroma.py.  A helper, not a conftest.  The matrix step, the level scales, the rounding
and the storage of a level in a 16-bit word are tests/yuv_ref.py's and tests/yuv16_ref.py's; only the chroma resampling and the
packing of the two sub-samplings are defined here.

    4:2:2   chroma planes h x ceil(w/2); chroma sample (y, k) on luma row y, column 2k
            up:   Ch(y, x) = C[y][x/2] (x even) | (C[y][k] + C[y][min(k+1, Wc-1)]) / 2, k = (x-1)/2 (x odd); no vertical step
            down: taps [1,2,1]/4 on columns 2k-1, 2k, 2k+1 of row y, indices clamped; no vertical mean
    4:4:4   chroma planes h x w; a pixel's chroma is its own sample both ways

Everything works on LEVELS and returns the values BEFORE rounding, as the two helpers it is built on do."""
import numpy as np

import yuv16_ref
import yuv_ref
from yuv16_ref import from_words, to_levels, to_words
from yuv_ref import to_bytes

# layout -> (sub-sampling, semi-planar, depth, storage of a level in a 16-bit word)
LAYOUTS = {'i422': ('422', False, 8, None), 'nv16': ('422', True, 8, None),
           'i422p10': ('422', False, 10, 'lsb'), 'i422p12': ('422', False, 12, 'lsb'),
           'p210': ('422', True, 10, 'msb'), 'p212': ('422', True, 12, 'msb'),
           'i444': ('444', False, 8, None), 'i444p10': ('444', False, 10, 'lsb'), 'i444p12': ('444', False, 12, 'lsb')}


def chroma_size(layout, h, w):
    return (h, (w + 1) // 2) if LAYOUTS[layout][0] == '422' else (h, w)


def upsample422(c, h, w):
    """A 4:2:2 chroma plane [h,Wc] (levels) on the luma grid [h,w]: [1,1]/2 between two chroma columns for an odd x, the right
    edge clamped; rows as they are."""
    c = np.asarray(c, np.float64)
    Wc = c.shape[1]
    assert c.shape == (h, (w + 1) // 2)
    x = np.arange(w)
    ka = x // 2
    kb = np.where(x % 2 == 1, np.minimum(ka + 1, Wc - 1), ka)
    return (c[:, ka] + c[:, kb]) / 2


def downsample422(c):
    """A chroma signal on the luma grid [h,w] -> [h,Wc]: taps [1,2,1]/4 on columns 2k-1, 2k, 2k+1 of every row, indices clamped
    to the plane."""
    c = np.asarray(c, np.float64)
    w = c.shape[1]
    k = 2 * np.arange((w + 1) // 2)
    return (c[:, np.maximum(k - 1, 0)] + 2 * c[:, k] + c[:, np.minimum(k + 1, w - 1)]) / 4


def upsample(c, h, w, layout):
    if LAYOUTS[layout][0] == '422':
        return upsample422(c, h, w)
    c = np.asarray(c, np.float64)
    assert c.shape == (h, w)
    return c


def downsample(c, layout):
    return downsample422(c) if LAYOUTS[layout][0] == '422' else np.asarray(c, np.float64)


def _to_rgb(y, cb, cr, depth, matrix, yuv_range):
    if depth == 8:
        return yuv_ref.ycbcr_to_rgb(y, cb, cr, matrix, yuv_range)
    return yuv16_ref.ycbcr_to_rgb(y, cb, cr, depth, matrix, yuv_range)


def _to_ycbcr(rgb, depth, matrix, yuv_range):
    if depth == 8:
        return yuv_ref.rgb_to_ycbcr(rgb, matrix, yuv_range)
    return yuv16_ref.rgb_to_ycbcr(rgb, depth, matrix, yuv_range)


def ingest(y, cb, cr, Hp, Wp, layout, mode='reflect', matrix='bt601', yuv_range='limited'):
    """Integer level planes y [h,w], cb / cr [Hc,Wc] -> fp64 RGB [3,Hp,Wp]: converted at the frame's size, then padded at the
    bottom and right as torch.nn.functional.pad does ('reflect' | 'replicate')."""
    h, w = y.shape
    rgb = _to_rgb(y, upsample(cb, h, w, layout), upsample(cr, h, w, layout), LAYOUTS[layout][2], matrix, yuv_range)
    return np.pad(rgb, ((0, 0), (0, Hp - h), (0, Wp - w)), mode='reflect' if mode == 'reflect' else 'edge')


def emit(sr, h, w, layout, lo=0.0, hi=1.0, matrix='bt601', yuv_range='limited'):
    """fp32 / fp64 RGB [3,Hs,Ws] -> the top-left h x w crop as (Y [h,w], Cb [Hc,Wc], Cr [Hc,Wc]) levels BEFORE rounding."""
    v = np.asarray(sr, np.float64)[:, :h, :w]
    t = (np.clip(v, lo, hi) - lo) / (hi - lo)
    y, cb, cr = _to_ycbcr(t, LAYOUTS[layout][2], matrix, yuv_range)
    return y, downsample(cb, layout), downsample(cr, layout)


def round_levels(levels, layout):
    """Round half to even, clamp to 0 .. 2^d - 1 (uint8 at 8 bits, uint16 above)."""
    depth = LAYOUTS[layout][2]
    return to_bytes(levels) if depth == 8 else to_levels(levels, depth)


def tie_distance(levels, layout):
    depth = LAYOUTS[layout][2]
    return yuv_ref.tie_distance(levels) if depth == 8 else yuv16_ref.tie_distance(levels, depth)


def samples_of(levels, layout, garbage=None):
    """Integer levels -> the samples of the layout: bytes, or the 16-bit words of its storage (`garbage` fills the bits that
    carry no level)."""
    _, _, depth, storage = LAYOUTS[layout]
    return np.asarray(levels).astype(np.uint8) if depth == 8 else to_words(levels, storage, depth, garbage)


def levels_of(samples, layout):
    """(levels, the bits that carry no level) of the layout's samples."""
    _, _, depth, storage = LAYOUTS[layout]
    if depth == 8:
        return np.asarray(samples), np.zeros_like(samples)
    return from_words(samples, storage, depth)


def pack(y, cb, cr, layout):
    """Sample planes -> the packed frame of a rawvideo pipe: [2h, w] (4:2:2, w even) or [3h, w] (4:4:4)."""
    chroma, semi = LAYOUTS[layout][:2]
    h, w = y.shape
    if chroma == '444':
        return np.concatenate([y, cb, cr])
    assert w % 2 == 0
    if semi:
        return np.concatenate([y, np.stack([cb, cr], -1).reshape(h, w)])
    return np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)]).reshape(2 * h, w)


def unpack(frame, layout):
    """The inverse of pack: (y, cb, cr) planes."""
    chroma, semi = LAYOUTS[layout][:2]
    rows, w = frame.shape
    if chroma == '444':
        h = rows // 3
        return frame[:h], frame[h:2 * h], frame[2 * h:]
    h = rows // 2
    y = frame[:h]
    if semi:
        uv = frame[h:].reshape(h, w // 2, 2)
        return y, uv[:, :, 0], uv[:, :, 1]
    c = frame[h:].reshape(2, h, w // 2)
    return y, c[0], c[1]
