"""The YCbCr 4:2:0 arithmetic of csrc/frame_yuv.hip restated in fp64 numpy: the yardstick of test_yuv_host.py and
test_gpu_yuv.py.  A helper, not a conftest.

    matrix  bt601: Kr = 0.299, Kb = 0.114;  bt709: Kr = 0.2126, Kb = 0.0722;  Kg = 1 - Kr - Kb
    range   limited: y0 = 16, ys = 219, cs = 224;  full: y0 = 0, ys = 255, cs = 255
    siting  chroma sample (j, k) on luma column 2k, midway between luma rows 2j and 2j+1; planes ceil(h/2) x ceil(w/2)

Everything here works on LEVELS (0 .. 255 as fp64) on the 8-bit side and returns the values BEFORE rounding, so that a test
can tell a byte that the arithmetic decides from one that sits on a tie."""
import numpy as np

MATRICES = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}
RANGES = {'limited': (16.0, 219.0, 224.0), 'full': (0.0, 255.0, 255.0)}


def ycbcr_to_rgb(y, cb, cr, matrix='bt601', yuv_range='limited', clamp=True):
    """Levels (any shape, chroma already on the luma grid) -> fp64 RGB in [0,1], stacked on a new first axis."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    y0, ys, cs = RANGES[yuv_range]
    yn = (np.asarray(y, np.float64) - y0) / ys
    cb = (np.asarray(cb, np.float64) - 128.0) / cs
    cr = (np.asarray(cr, np.float64) - 128.0) / cs
    rgb = np.stack([yn + 2 * (1 - kr) * cr,
                    yn - (2 * kb * (1 - kb) / kg) * cb - (2 * kr * (1 - kr) / kg) * cr,
                    yn + 2 * (1 - kb) * cb])
    return np.clip(rgb, 0.0, 1.0) if clamp else rgb


def rgb_to_ycbcr(rgb, matrix='bt601', yuv_range='limited'):
    """fp64 RGB [3,...] in [0,1] -> (Y, Cb, Cr) levels before rounding, each of the pixel's shape."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    y0, ys, cs = RANGES[yuv_range]
    r, g, b = (np.asarray(c, np.float64) for c in rgb)
    y = kr * r + kg * g + kb * b
    return y0 + ys * y, 128.0 + cs * (b - y) / (2 * (1 - kb)), 128.0 + cs * (r - y) / (2 * (1 - kr))


def to_bytes(levels):
    """Round half to even, clamp to 0 .. 255."""
    return np.clip(np.rint(levels), 0, 255).astype(np.uint8)


def tie_distance(levels):
    """How far a pre-rounding value is from the nearest tie x.5 (values that the clamp decides are far from any)."""
    v = np.asarray(levels, np.float64)
    d = np.abs(v - np.floor(v) - 0.5)
    return np.where((v < -0.5) | (v > 255.5), 0.5, d)


def upsample(c, h, w):
    """A chroma plane [Hc,Wc] (levels) on the luma grid [h,w]: [1,1]/2 between two chroma columns for an odd x, 0.75 / 0.25
    between the two nearest chroma rows, edges clamped."""
    c = np.asarray(c, np.float64)
    Hc, Wc = c.shape
    assert (Hc, Wc) == ((h + 1) // 2, (w + 1) // 2)
    x = np.arange(w)
    ka = x // 2
    kb = np.where(x % 2 == 1, np.minimum(ka + 1, Wc - 1), ka)
    ch = (c[:, ka] + c[:, kb]) / 2                            # [Hc, w]
    y = np.arange(h)
    j = y // 2
    jn = np.where(y % 2 == 1, np.minimum(j + 1, Hc - 1), np.maximum(j - 1, 0))
    return 0.75 * ch[j] + 0.25 * ch[jn]


def downsample(c):
    """A chroma signal on the luma grid [h,w] -> [Hc,Wc]: taps [1,2,1]/4 on columns 2k-1, 2k, 2k+1, the mean of rows 2j and
    min(2j+1, h-1), indices clamped to the plane."""
    c = np.asarray(c, np.float64)
    h, w = c.shape
    k = 2 * np.arange((w + 1) // 2)
    f = (c[:, np.maximum(k - 1, 0)] + 2 * c[:, k] + c[:, np.minimum(k + 1, w - 1)]) / 4
    j = 2 * np.arange((h + 1) // 2)
    return (f[j] + f[np.minimum(j + 1, h - 1)]) / 2


def ingest(y, cb, cr, Hp, Wp, mode='reflect', matrix='bt601', yuv_range='limited'):
    """uint8 planes y [h,w], cb / cr [Hc,Wc] -> fp64 RGB [3,Hp,Wp]: converted at the frame's size, then padded at the bottom
    and right as torch.nn.functional.pad does ('reflect' | 'replicate')."""
    h, w = y.shape
    rgb = ycbcr_to_rgb(y, upsample(cb, h, w), upsample(cr, h, w), matrix, yuv_range)
    return np.pad(rgb, ((0, 0), (0, Hp - h), (0, Wp - w)), mode='reflect' if mode == 'reflect' else 'edge')


def emit(sr, h, w, lo=0.0, hi=1.0, matrix='bt601', yuv_range='limited'):
    """fp32 / fp64 RGB [3,Hs,Ws] -> the top-left h x w crop as (Y [h,w], Cb [Hc,Wc], Cr [Hc,Wc]) levels BEFORE rounding."""
    v = np.asarray(sr, np.float64)[:, :h, :w]
    t = (np.clip(v, lo, hi) - lo) / (hi - lo)
    y, cb, cr = rgb_to_ycbcr(t, matrix, yuv_range)
    return y, downsample(cb), downsample(cr)


def pack(y, cb, cr, layout):
    """uint8 planes of an even-sized frame -> the packed [h*3/2, w] frame of a rawvideo pipe."""
    h, w = y.shape
    assert h % 2 == 0 and w % 2 == 0
    if layout == 'nv12':
        return np.concatenate([y, np.stack([cb, cr], -1).reshape(h // 2, w)])
    return np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)]).reshape(h * 3 // 2, w)


def unpack(frame, layout):
    """The inverse of pack: (y, cb, cr) planes."""
    rows, w = frame.shape
    h = rows * 2 // 3
    y = frame[:h]
    if layout == 'nv12':
        uv = frame[h:].reshape(h // 2, w // 2, 2)
        return y, uv[:, :, 0], uv[:, :, 1]
    c = frame[h:].reshape(2, h // 2, w // 2)
    return y, c[0], c[1]
