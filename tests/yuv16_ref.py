"""The YCbCr 4:2:0 arithmetic of csrc/frame_yuv.hip restated in fp64 numpy at a depth d: the yardstick of
test_yuv16_host.py and test_gpu_yuv16.py.  A helper, not a conftest.  The up-sampling, down-sampling, padding and packing are
tests/yuv_ref.py's; only the level scale and the storage of a level in a 16-bit word are defined here.

    level scale, s = 2^(d-8)   limited: y0 = 16 s, ys = 219 s, cs = 224 s, chroma mid 128 s
                               full:    y0 = 0, ys = cs = 2^d - 1, chroma mid 2^(d-1)          (H.273; d = 8 is yuv_ref's)
    storage 'msb' (P010 / P012)                word = level << (16 - d); the low 16 - d bits are ignored on the way in
            'lsb' (yuv420p10le / yuv420p12le)  word = level; the high 16 - d bits are ignored on the way in

Everything works on LEVELS (fp64 or integers) and returns the values BEFORE rounding, as yuv_ref does."""
import numpy as np

import yuv_ref
from yuv_ref import MATRICES

LAYOUTS = {'p010': ('msb', 10), 'p012': ('msb', 12), 'i420p10': ('lsb', 10), 'i420p12': ('lsb', 12)}


def level_scale(depth, yuv_range):
    """(y0, ys, cs, chroma mid) in levels."""
    s = float(2 ** (depth - 8))
    if yuv_range == 'limited':
        return 16.0 * s, 219.0 * s, 224.0 * s, 128.0 * s
    assert yuv_range == 'full'
    top = float(2 ** depth - 1)
    return 0.0, top, top, float(2 ** (depth - 1))


def ycbcr_to_rgb(y, cb, cr, depth, matrix='bt601', yuv_range='limited', clamp=True):
    """Levels (any shape, chroma already on the luma grid) -> fp64 RGB in [0,1], stacked on a new first axis."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    y0, ys, cs, cm = level_scale(depth, yuv_range)
    yn = (np.asarray(y, np.float64) - y0) / ys
    cb = (np.asarray(cb, np.float64) - cm) / cs
    cr = (np.asarray(cr, np.float64) - cm) / cs
    rgb = np.stack([yn + 2 * (1 - kr) * cr,
                    yn - (2 * kb * (1 - kb) / kg) * cb - (2 * kr * (1 - kr) / kg) * cr,
                    yn + 2 * (1 - kb) * cb])
    return np.clip(rgb, 0.0, 1.0) if clamp else rgb


def rgb_to_ycbcr(rgb, depth, matrix='bt601', yuv_range='limited'):
    """fp64 RGB [3,...] in [0,1] -> (Y, Cb, Cr) levels before rounding."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    y0, ys, cs, cm = level_scale(depth, yuv_range)
    r, g, b = (np.asarray(c, np.float64) for c in rgb)
    y = kr * r + kg * g + kb * b
    return y0 + ys * y, cm + cs * (b - y) / (2 * (1 - kb)), cm + cs * (r - y) / (2 * (1 - kr))


def to_levels(levels, depth):
    """Round half to even, clamp to 0 .. 2^d - 1."""
    return np.clip(np.rint(levels), 0, 2 ** depth - 1).astype(np.uint16)


def tie_distance(levels, depth):
    """How far a pre-rounding value is from the nearest tie x.5 (values that the clamp decides are far from any)."""
    v = np.asarray(levels, np.float64)
    d = np.abs(v - np.floor(v) - 0.5)
    return np.where((v < -0.5) | (v > 2 ** depth - 0.5), 0.5, d)


def ingest(y, cb, cr, Hp, Wp, depth, mode='reflect', matrix='bt601', yuv_range='limited'):
    """Integer level planes y [h,w], cb / cr [Hc,Wc] -> fp64 RGB [3,Hp,Wp]: converted at the frame's size, then padded at the
    bottom and right as torch.nn.functional.pad does ('reflect' | 'replicate')."""
    h, w = y.shape
    rgb = ycbcr_to_rgb(y, yuv_ref.upsample(cb, h, w), yuv_ref.upsample(cr, h, w), depth, matrix, yuv_range)
    return np.pad(rgb, ((0, 0), (0, Hp - h), (0, Wp - w)), mode='reflect' if mode == 'reflect' else 'edge')


def emit(sr, h, w, depth, lo=0.0, hi=1.0, matrix='bt601', yuv_range='limited'):
    """fp32 / fp64 RGB [3,Hs,Ws] -> the top-left h x w crop as (Y [h,w], Cb [Hc,Wc], Cr [Hc,Wc]) levels BEFORE rounding."""
    v = np.asarray(sr, np.float64)[:, :h, :w]
    t = (np.clip(v, lo, hi) - lo) / (hi - lo)
    y, cb, cr = rgb_to_ycbcr(t, depth, matrix, yuv_range)
    return y, yuv_ref.downsample(cb), yuv_ref.downsample(cr)


def to_words(levels, storage, depth, garbage=None):
    """Integer levels -> the uint16 words of a storage; `garbage` (any integers of the same shape) fills the bits that carry no
    level, 0 otherwise."""
    lev = np.asarray(levels).astype(np.uint32)
    assert int(lev.max(initial=0)) < 2 ** depth
    g = np.zeros_like(lev) if garbage is None else np.asarray(garbage).astype(np.uint32)
    free = 16 - depth
    if storage == 'msb':
        return ((lev << free) | (g & (2 ** free - 1))).astype(np.uint16)
    assert storage == 'lsb'
    return (lev | ((g & (2 ** free - 1)) << depth)).astype(np.uint16)


def from_words(words, storage, depth):
    """uint16 words -> (levels, the bits that carry no level) as uint16 arrays."""
    v = np.asarray(words).astype(np.uint32) & 0xffff
    free = 16 - depth
    if storage == 'msb':
        return (v >> free).astype(np.uint16), (v & (2 ** free - 1)).astype(np.uint16)
    assert storage == 'lsb'
    return (v & (2 ** depth - 1)).astype(np.uint16), (v >> depth).astype(np.uint16)


def pack(y, cb, cr, layout):
    """uint16 word planes of an even-sized frame -> the packed [h*3/2, w] frame of a rawvideo pipe."""
    return yuv_ref.pack(y, cb, cr, 'nv12' if LAYOUTS[layout][0] == 'msb' else 'i420')


def unpack(frame, layout):
    """The inverse of pack: (y, cb, cr) word planes."""
    return yuv_ref.unpack(frame, 'nv12' if LAYOUTS[layout][0] == 'msb' else 'i420')
