"""numpy restatement of the host side of frame scoring (csrc/frame_score.hip, frames.score, adapt.score_summary): the Y8 integer
rule, the samples of a frame in every format, crop, the exact sum of squared differences, the float64 SSIM with L in its
separable form (what the kernel evaluates) and in the reference's 2-D-window form, and the per-scene summary.  The tests that
use it (test_score_host.py, test_gpu_score.py) never read the reference checkout."""
import math

import numpy as np


def y8(r, g, b):
    """rgb2ycbcr(only_y=True) of 8-bit R, G, B, (65.481 R + 128.553 G + 24.966 B) / 255 + 16 rounded half to even, in integers."""
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    num = 65481 * r + 128553 * g + 24966 * b + 16 * 255000
    q, rem = num // 255000, num % 255000
    return q + ((rem > 127500) | ((rem == 127500) & (q % 2 == 1)))


def is_tie(r, g, b):
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    return (65481 * r + 128553 * g + 24966 * b) % 255000 == 127500


def tie_triples():
    """The [n,3] uint8 array of every (R, G, B) whose Y level is an exact tie."""
    v = np.arange(256, dtype=np.int64)
    gb = 128553 * v[:, None] + 24966 * v[None, :]
    out = []
    for r in range(256):
        g, b = np.nonzero((65481 * r + gb) % 255000 == 127500)
        out += [(r, int(gi), int(bi)) for gi, bi in zip(g, b)]
    return np.array(out, dtype=np.uint8)


def quant_u8(x, min_max=(0, 1)):
    """util.tensor2img's 8-bit values of a float array, in fp32 like torch / numpy / quant.h."""
    lo, hi = np.float32(min_max[0]), np.float32(min_max[1])
    a = (np.clip(np.asarray(x, dtype=np.float32), lo, hi) - lo) / (hi - lo)
    return (a * np.float32(255.0)).round().astype(np.int64)


def samples(frame, kind, channel, min_max=(0, 1), depth=8):
    """int64 [H,W,C] samples (C = 3 for 'rgb', 1 for 'y') of a numpy frame: kind 'hwc_rgb' / 'hwc_bgr' (uint8 [H,W,3|4]), 'chw'
    (float [3,H,W]), 'y' (uint8 [H,W]), 'y_msb' / 'y_lsb' (uint16 [H,W] holding `depth` bits at the top / the bottom)."""
    if kind in ('hwc_rgb', 'hwc_bgr', 'chw'):
        rgb = quant_u8(frame, min_max).transpose(1, 2, 0) if kind == 'chw' else np.asarray(frame)[:, :, :3].astype(np.int64)
        if kind == 'hwc_bgr':
            rgb = rgb[:, :, ::-1]
        return rgb if channel == 'rgb' else y8(rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2])[:, :, None]
    assert channel == 'y', "a Y plane has no RGB samples"
    w = np.asarray(frame).astype(np.int64) & 0xffff
    if kind == 'y':
        return w[:, :, None]
    return (w >> (16 - depth) if kind == 'y_msb' else w & ((1 << depth) - 1))[:, :, None]


def crop(x, k):
    """util.crop_border for one image."""
    return x if k == 0 else x[k:-k, k:-k]


def sse(a, b):
    """The exact integer sum of squared differences of two int64 sample arrays."""
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def taps():
    i = np.arange(11, dtype=np.float64) - 5.0
    k = np.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    return k / k.sum()


def _separable(x, g):
    h, w = x.shape[:2]
    hp = np.zeros((h, w - 10) + x.shape[2:], dtype=np.float64)
    for t in range(11):
        hp += g[t] * x[:, t:t + w - 10]
    out = np.zeros((h - 10, w - 10) + x.shape[2:], dtype=np.float64)
    for t in range(11):
        out += g[t] * hp[t:t + h - 10]
    return out


def _window(x, g):
    win = np.outer(g, g)
    h, w = x.shape[:2]
    out = np.zeros((h - 10, w - 10) + x.shape[2:], dtype=np.float64)
    for dy in range(11):
        for dx in range(11):
            out += win[dy, dx] * x[dy:dy + h - 10, dx:dx + w - 10]
    return out


def ssim(a, b, L=255, separable=True):
    """The mean SSIM of two [H,W,C] sample arrays over channels and the valid region; NaN without one."""
    if a.shape[0] <= 10 or a.shape[1] <= 10:
        return float('nan')
    f = _separable if separable else _window
    g = taps()
    c1, c2 = (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L)
    x, y = a.astype(np.float64), b.astype(np.float64)
    mu1, mu2 = f(x, g), f(y, g)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = f(x * x, g) - mu1_sq, f(y * y, g) - mu2_sq, f(x * y, g) - mu12
    m = ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))
    return float(m.mean())


def score(a, b, k=0, depth=8, separable=True):
    """(sse, samples, mse, ssim) of two [H,W,C] sample arrays after a crop of k."""
    a, b = crop(a, k), crop(b, k)
    s = sse(a, b)
    return s, a.size, s / a.size, ssim(a, b, (1 << depth) - 1, separable)


def psnr(mse, peak=255):
    return float('inf') if mse == 0 else 20 * math.log10(peak / math.sqrt(mse))


def summary(rows, nframes, cuts=None, peak=255):
    """The per-scene report of adapt.score_summary from rows [(mse, ssim), ...], restated with explicit loops."""
    rows = [(float(m), float(s)) for m, s in rows]
    edges = [0] + list(cuts or []) + [len(rows)]
    border = nframes // 2
    scenes = []
    for a, b in zip(edges[:-1], edges[1:]):
        acc = {'psnr': [0.0, 0], 'psnr_center': [0.0, 0], 'psnr_border': [0.0, 0],
               'ssim': [0.0, 0], 'ssim_center': [0.0, 0], 'ssim_border': [0.0, 0]}
        for i in range(b - a):
            m, s = rows[a + i]
            part = '_center' if border <= i < (b - a) - border else '_border'
            for name, v in (('psnr', psnr(m, peak)), ('ssim', s)):
                for key in (name, name + part):
                    acc[key][0] += v
                    acc[key][1] += 1
        sc = {'first': a, 'frames': b - a, 'center_frames': acc['psnr_center'][1], 'border_frames': acc['psnr_border'][1]}
        for key, (tot, n) in acc.items():
            sc[key] = tot / n if n else (float('nan') if key.endswith('_center') else 0.0)
        scenes.append(sc)
    keys = ('psnr', 'psnr_center', 'psnr_border', 'ssim', 'ssim_center', 'ssim_border')
    return {'scenes': scenes, 'mean': {k: sum(s[k] for s in scenes) / len(scenes) for k in keys}}
