"""numpy restatement of the integer RGB layouts beyond 8-bit interleaved (csrc/frame_rgb.hip): fp32 restatements of
the two formulas -- value = float32(level) / float32(top) on the way in, level = rint(t * float32(top)) with
t = (min(max(v, lo), hi) - lo) / (hi - lo) on the way out, top = 2^d - 1 -- with np.pad for the padding, and the integer luma of
the scene-cut sums.  The tests that use it (test_rgb_host.py, test_gpu_rgb.py) never read the reference checkout."""
import numpy as np

# layout -> (planar, depth, the channel of each stored word of a pixel / of each stored plane, as an index into R, G, B)
LAYOUTS = {'hwc_rgb16': (False, 16, (0, 1, 2)), 'hwc_bgr16': (False, 16, (2, 1, 0)),
           'chw_rgb8': (True, 8, (0, 1, 2)), 'chw_gbr8': (True, 8, (1, 2, 0))}
for _d in (10, 12, 16):
    LAYOUTS['chw_rgb%d' % _d] = (True, _d, (0, 1, 2))
    LAYOUTS['chw_gbr%d' % _d] = (True, _d, (1, 2, 0))
NAMES = tuple(LAYOUTS)


def dtype(layout):
    return np.uint8 if LAYOUTS[layout][1] == 8 else np.uint16


def top(layout):
    return (1 << LAYOUTS[layout][1]) - 1


def shape(layout, h, w, ps=3):
    return (3, h, w) if LAYOUTS[layout][0] else (h, w, ps)


def levels(frame, layout):
    """int64 [3,h,w] levels of a frame in R, G, B order: word & top (a fourth word of an interleaved pixel is dropped)."""
    planar, _, order = LAYOUTS[layout]
    v = (np.asarray(frame).astype(np.int64) & 0xffff) & top(layout)
    stored = v if planar else v[:, :, :3].transpose(2, 0, 1)
    out = np.empty_like(stored)
    for k, c in enumerate(order):
        out[c] = stored[k]
    return out


def from_levels(lev, layout, junk=None, ps=3):
    """The frame of `layout` that holds the int [3,h,w] R, G, B levels; junk: int [3,h,w] values for the bits of a word above the
    level (planar 10 / 12 bits); ps = 4: a fourth word of 0x1234 per pixel."""
    planar, d, order = LAYOUTS[layout]
    lev = np.asarray(lev).astype(np.int64)
    stored = np.stack([lev[c] for c in order])
    if junk is not None:
        stored = stored | ((np.asarray(junk).astype(np.int64) & ((1 << (16 - d)) - 1)) << d)
    if planar:
        return stored.astype(dtype(layout))
    out = np.full(lev.shape[1:] + (ps,), 0x1234, dtype=np.int64)
    out[:, :, :3] = stored.transpose(1, 2, 0)
    return out.astype(dtype(layout))


def ingest(frame, layout, Hp, Wp, mode='reflect'):
    """fp32 [3,Hp,Wp]: float32(level) / float32(top), padded at the bottom and right ('reflect' | 'replicate')."""
    lev = levels(frame, layout)
    x = lev.astype(np.float32) / np.float32(top(layout))
    h, w = x.shape[1:]
    return np.pad(x, ((0, 0), (0, Hp - h), (0, Wp - w)), mode='reflect' if mode == 'reflect' else 'edge')


def quant(x, top_, lo=0.0, hi=1.0):
    """int64 levels of a float array: quant.h's quant_levels in fp32, round half to even."""
    lo, hi = np.float32(lo), np.float32(hi)
    v = np.asarray(x, dtype=np.float32)
    t = (np.minimum(np.maximum(v, lo), hi) - lo) / (hi - lo)
    return np.rint(t * np.float32(top_)).astype(np.int64)


def emit(x, h, w, layout, lo=0.0, hi=1.0):
    """The top-left h x w crop of fp32 [3,H,W] as a frame of `layout` (three words per pixel)."""
    return from_levels(quant(np.asarray(x)[:, :h, :w], top(layout), lo, hi), layout)


def luma8(frame, layout):
    """int64 [h,w]: (77 R + 150 G + 29 B + 128) >> 8 on the top 8 bits of each level."""
    r, g, b = levels(frame, layout) >> (LAYOUTS[layout][1] - 8)
    return (77 * r + 150 * g + 29 * b + 128) >> 8


def luma_sad(video, layout):
    """[T-1] exact sums of |Y8_t - Y8_(t-1)|."""
    y = [luma8(f, layout) for f in video]
    return [int(np.abs(b - a).sum()) for a, b in zip(y[:-1], y[1:])]
