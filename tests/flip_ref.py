"""The flip-test x4 self-ensemble in numpy (csrc/frame_flip.hip): the definitions of dvsr_frame_flip and
dvsr_frame_flip_mean, the shapes the tests run and their data."""
import numpy as np

FLIP_W, FLIP_H = 1, 2

# (planes, H, W): one float4 mirrored onto itself; the smallest with every axis > 1; an odd H and an odd number of float4s
# (the middle row and the middle chunk map to themselves); a row longer than one wave's 256 floats; the 5-D clip (B N 3 = 15)
SHAPES = [(1, 1, 4), (3, 2, 8), (3, 5, 12), (2, 3, 260), (15, 7, 20)]


def flip(x, flags):
    """dst[..., y, x] = src[..., fy(y), fx(x)], fx(x) = W-1-x if flags & 1, fy(y) = H-1-y if flags & 2."""
    if flags & FLIP_W:
        x = x[..., ::-1]
    if flags & FLIP_H:
        x = x[..., ::-1, :]
    return np.ascontiguousarray(x)


def flip_mean(y0, yw, yh, yhw):
    """(((y0 + flipW(yw)) + flipH(yh)) + flipHW(yhw)) * 0.25 in fp32, the additions in this order (utils/util.py:232-254)."""
    y0, yw, yh, yhw = (np.asarray(y, dtype=np.float32) for y in (y0, yw, yh, yhw))
    with np.errstate(invalid='ignore', over='ignore'):
        s = (y0 + flip(yw, FLIP_W)).astype(np.float32)
        s = (s + flip(yh, FLIP_H)).astype(np.float32)
        s = (s + flip(yhw, FLIP_W | FLIP_H)).astype(np.float32)
        return (s * np.float32(0.25)).astype(np.float32)


def data(shape, seed):
    """fp32 normal data (negative values included) with a NaN in the first element and an inf in the last: the two corners,
    which every flip moves."""
    x = np.random.RandomState(seed).standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    flat[0], flat[-1] = np.nan, np.inf
    return x


def special_places(shape, flags):
    """(flat index of the NaN, flat index of the inf) of flip(data(shape, .), flags)."""
    planes, H, W = shape

    def moved(p, y, x):
        return (p * H + (H - 1 - y if flags & FLIP_H else y)) * W + (W - 1 - x if flags & FLIP_W else x)
    return moved(0, 0, 0), moved(planes - 1, H - 1, W - 1)
