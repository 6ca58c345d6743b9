"""The chroma sitings and the BT.2020 NCL matrix of csrc/frame_yuv.hip restated in fp64 numpy: the yardstick of
test_yuv_siting_host.py and test_gpu_yuv_siting.py.  A helper, not a conftest.  The matrix step of 'bt601' / 'bt709', the level
scales, the rounding, the storage of a level in a 16-bit word and the packing are tests/yuv_ref.py's, tests/yuv16_ref.py's and
tests/yuv_chroma_ref.py's; only the resampling per siting and the 'bt2020nc' coefficients are defined here.

Chroma sample (j, k) sits at luma position (4:2:2: y is the luma row itself; 4:4:4: on its pixel)
                x          y
    left        2k         2j + 1/2
    center      2k + 1/2   2j + 1/2
    topleft     2k         2j

The resampling is stated twice, independently:
  (a) upsample_taps / downsample_taps: the tap formulas with clamped indices, as the kernels and the documents write them
  (b) upsample_interp / downsample_filter: interp_at(c, positions, at), plain linear interpolation of samples that sit at
      `positions` with the edge values held beyond the first and last one; and a triangle ([1,2,1]/4, co-sited) or box ([1,1]/2,
      midway) filter centred on the same positions, taps beyond the plane folded onto its edge
test_yuv_siting_host.py holds (a) == (b); ingest / emit use (a).

Everything works on LEVELS and returns the values BEFORE rounding, as the helpers it is built on do."""
import numpy as np

import yuv16_ref
import yuv_chroma_ref
import yuv_ref
from yuv16_ref import from_words, to_levels, to_words
from yuv_ref import to_bytes

SITINGS = ('left', 'center', 'topleft')
KR_KB_BT2020 = (0.2627, 0.0593)                 # H.273 MatrixCoefficients 9, BT.2020 non-constant luminance
MATRICES = dict(yuv_ref.MATRICES, bt2020nc=KR_KB_BT2020)

# layout -> (sub-sampling, semi-planar, depth, storage of a level in a 16-bit word)
LAYOUTS = {'nv12': ('420', True, 8, None), 'i420': ('420', False, 8, None),
           'p010': ('420', True, 10, 'msb'), 'p012': ('420', True, 12, 'msb'),
           'i420p10': ('420', False, 10, 'lsb'), 'i420p12': ('420', False, 12, 'lsb')}
LAYOUTS.update(yuv_chroma_ref.LAYOUTS)


def chroma_size(layout, h, w):
    sub = LAYOUTS[layout][0]
    return ((h + 1) // 2 if sub == '420' else h), (w if sub == '444' else (w + 1) // 2)


def axes(sub, siting):
    """(the kind of the x axis, of the y axis) of a sub-sampling under a siting: 'co' -- chroma sample k on luma index 2k --,
    'mid' -- on 2k + 1/2 -- or None, an axis that is not sub-sampled."""
    assert siting in SITINGS
    x = None if sub == '444' else ('mid' if siting == 'center' else 'co')
    y = None if sub != '420' else ('co' if siting == 'topleft' else 'mid')
    return x, y


def positions(n, kind):
    """The luma coordinates of the n chroma samples of an axis."""
    return 2.0 * np.arange(n) + (0.5 if kind == 'mid' else 0.0)


# ---- (a) the tap formulas
def _up_taps_axis(c, n, kind):
    """Axis 0 of c ([Nc, ...] levels) on the n luma indices of that axis."""
    if kind is None:
        assert c.shape[0] == n
        return c
    nc = c.shape[0]
    assert nc == (n + 1) // 2
    s = np.arange(n)
    k, odd = s // 2, s % 2 == 1
    if kind == 'co':              # C[k] (even) | (C[k] + C[min(k+1, Nc-1)]) / 2 (odd)
        return (c[k] + c[np.where(odd, np.minimum(k + 1, nc - 1), k)]) / 2
    # midway: 0.75 C[k] + 0.25 C[max(k-1, 0)] (even) | 0.75 C[k] + 0.25 C[min(k+1, Nc-1)] (odd)
    return 0.75 * c[k] + 0.25 * c[np.where(odd, np.minimum(k + 1, nc - 1), np.maximum(k - 1, 0))]


def upsample_taps(c, h, w, sub, siting):
    c = np.asarray(c, np.float64)
    kx, ky = axes(sub, siting)
    hx = _up_taps_axis(c.T, w, kx).T                       # the horizontal step H(j, x), per chroma row
    return _up_taps_axis(hx, h, ky)


def _down_taps_axis(c, kind):
    """Axis 0 of c ([n, ...] on the luma grid) -> the ceil(n/2) chroma samples of that axis."""
    if kind is None:
        return c
    n = c.shape[0]
    k = 2 * np.arange((n + 1) // 2)
    if kind == 'co':              # [1,2,1]/4 on 2k-1, 2k, 2k+1
        return (c[np.maximum(k - 1, 0)] + 2 * c[k] + c[np.minimum(k + 1, n - 1)]) / 4
    return (c[k] + c[np.minimum(k + 1, n - 1)]) / 2        # the mean of 2k and min(2k+1, n-1)


def downsample_taps(c, sub, siting):
    c = np.asarray(c, np.float64)
    kx, ky = axes(sub, siting)
    return _down_taps_axis(_down_taps_axis(c.T, kx).T, ky)


# ---- (b) the same from the positions alone
def interp_at(c, pos, at):
    """Axis 0 of c, whose samples sit at the increasing coordinates `pos`, linearly interpolated at the coordinates `at`; the
    first / last sample is held beyond either end."""
    c, pos, at = np.asarray(c, np.float64), np.asarray(pos, np.float64), np.asarray(at, np.float64)
    if len(pos) == 1:
        return np.repeat(c, len(at), axis=0)
    i = np.clip(np.searchsorted(pos, at, side='right') - 1, 0, len(pos) - 2)
    t = np.clip((at - pos[i]) / (pos[i + 1] - pos[i]), 0.0, 1.0)
    t = t.reshape((-1,) + (1,) * (c.ndim - 1))
    return (1 - t) * c[i] + t * c[i + 1]


def upsample_interp(c, h, w, sub, siting):
    c = np.asarray(c, np.float64)
    kx, ky = axes(sub, siting)
    if kx is not None:
        c = interp_at(c.T, positions(c.shape[1], kx), np.arange(w)).T
    if ky is not None:
        c = interp_at(c, positions(c.shape[0], ky), np.arange(h))
    return c


def filter_matrix(n, kind):
    """[ceil(n/2), n]: row k holds the weights of the filter centred on chroma sample k's position -- a triangle of half-width
    2 (co-sited: 1/4, 1/2, 1/4) or a box of width 2 (midway: 1/2, 1/2) at the integer luma indices, those beyond the axis added
    to its edge."""
    pos = positions((n + 1) // 2, kind)
    m = np.zeros((len(pos), n))
    for k, p in enumerate(pos):
        for s in range(int(np.floor(p)) - 2, int(np.ceil(p)) + 3):
            d = abs(s - p)
            wgt = max(0.0, 1.0 - d / 2) / 2 if kind == 'co' else (0.5 if d < 1 else 0.0)
            m[k, min(max(s, 0), n - 1)] += wgt
    assert np.allclose(m.sum(1), 1.0)
    return m


def downsample_filter(c, sub, siting):
    c = np.asarray(c, np.float64)
    kx, ky = axes(sub, siting)
    if kx is not None:
        c = c @ filter_matrix(c.shape[1], kx).T
    if ky is not None:
        c = filter_matrix(c.shape[0], ky) @ c
    return c


# ---- the conversion
def upsample(c, h, w, layout, siting='left'):
    return upsample_taps(c, h, w, LAYOUTS[layout][0], siting)


def downsample(c, layout, siting='left'):
    return downsample_taps(c, LAYOUTS[layout][0], siting)


def ycbcr_to_rgb(y, cb, cr, depth, matrix='bt601', yuv_range='limited', clamp=True):
    """Levels (chroma already on the luma grid) -> fp64 RGB in [0,1].  'bt601' / 'bt709': yuv_ref's / yuv16_ref's own lines."""
    if matrix in yuv_ref.MATRICES:
        if depth == 8:
            return yuv_ref.ycbcr_to_rgb(y, cb, cr, matrix, yuv_range, clamp)
        return yuv16_ref.ycbcr_to_rgb(y, cb, cr, depth, matrix, yuv_range, clamp)
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    y0, ys, cs, cm = yuv16_ref.level_scale(depth, yuv_range)
    yn = (np.asarray(y, np.float64) - y0) / ys
    cb = (np.asarray(cb, np.float64) - cm) / cs
    cr = (np.asarray(cr, np.float64) - cm) / cs
    rgb = np.stack([yn + 2 * (1 - kr) * cr,
                    yn - (2 * kb * (1 - kb) / kg) * cb - (2 * kr * (1 - kr) / kg) * cr,
                    yn + 2 * (1 - kb) * cb])
    return np.clip(rgb, 0.0, 1.0) if clamp else rgb


def rgb_to_ycbcr(rgb, depth, matrix='bt601', yuv_range='limited'):
    """fp64 RGB [3,...] in [0,1] -> (Y, Cb, Cr) levels before rounding."""
    if matrix in yuv_ref.MATRICES:
        return yuv_ref.rgb_to_ycbcr(rgb, matrix, yuv_range) if depth == 8 else yuv16_ref.rgb_to_ycbcr(rgb, depth, matrix, yuv_range)
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    y0, ys, cs, cm = yuv16_ref.level_scale(depth, yuv_range)
    r, g, b = (np.asarray(c, np.float64) for c in rgb)
    y = kr * r + kg * g + kb * b
    return y0 + ys * y, cm + cs * (b - y) / (2 * (1 - kb)), cm + cs * (r - y) / (2 * (1 - kr))


def to_rgb(y, cb, cr, layout, matrix='bt601', yuv_range='limited', siting='left'):
    """Integer level planes y [h,w], cb / cr [Hc,Wc] -> fp64 RGB [3,h,w]."""
    h, w = y.shape
    return ycbcr_to_rgb(y, upsample(cb, h, w, layout, siting), upsample(cr, h, w, layout, siting), LAYOUTS[layout][2], matrix,
                        yuv_range)


def ingest(y, cb, cr, Hp, Wp, layout, mode='reflect', matrix='bt601', yuv_range='limited', siting='left'):
    """... -> fp64 RGB [3,Hp,Wp]: converted at the frame's size, then padded at the bottom and right as
    torch.nn.functional.pad does ('reflect' | 'replicate')."""
    h, w = y.shape
    rgb = to_rgb(y, cb, cr, layout, matrix, yuv_range, siting)
    return np.pad(rgb, ((0, 0), (0, Hp - h), (0, Wp - w)), mode='reflect' if mode == 'reflect' else 'edge')


def emit(sr, h, w, layout, lo=0.0, hi=1.0, matrix='bt601', yuv_range='limited', siting='left'):
    """fp32 / fp64 RGB [3,Hs,Ws] -> the top-left h x w crop as (Y [h,w], Cb [Hc,Wc], Cr [Hc,Wc]) levels BEFORE rounding."""
    v = np.asarray(sr, np.float64)[:, :h, :w]
    t = (np.clip(v, lo, hi) - lo) / (hi - lo)
    y, cb, cr = rgb_to_ycbcr(t, LAYOUTS[layout][2], matrix, yuv_range)
    return y, downsample(cb, layout, siting), downsample(cr, layout, siting)


# ---- levels, samples, packed frames: the helpers' own, for every layout
def round_levels(levels, layout):
    depth = LAYOUTS[layout][2]
    return to_bytes(levels) if depth == 8 else to_levels(levels, depth)


def tie_distance(levels, layout):
    depth = LAYOUTS[layout][2]
    return yuv_ref.tie_distance(levels) if depth == 8 else yuv16_ref.tie_distance(levels, depth)


def samples_of(levels, layout, garbage=None):
    _, _, depth, storage = LAYOUTS[layout]
    return np.asarray(levels).astype(np.uint8) if depth == 8 else to_words(levels, storage, depth, garbage)


def levels_of(samples, layout):
    _, _, depth, storage = LAYOUTS[layout]
    if depth == 8:
        return np.asarray(samples), np.zeros_like(samples)
    return from_words(samples, storage, depth)


def pack(y, cb, cr, layout):
    sub, semi = LAYOUTS[layout][:2]
    return yuv_ref.pack(y, cb, cr, 'nv12' if semi else 'i420') if sub == '420' else yuv_chroma_ref.pack(y, cb, cr, layout)


def unpack(frame, layout):
    sub, semi = LAYOUTS[layout][:2]
    return yuv_ref.unpack(frame, 'nv12' if semi else 'i420') if sub == '420' else yuv_chroma_ref.unpack(frame, layout)
