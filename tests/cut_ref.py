"""A numpy restatement of the scene-cut arithmetic (csrc/frame_cut.hip, dynavsr_amd/frames.py), for the tests: the 8-bit luma
of every layout, the sum of absolute luma differences of consecutive frames, and the scores.  No test imports the product's
own arithmetic through this module."""
import numpy as np


def luma_rgb(r, g, b):
    """Y8 = (77 R + 150 G + 29 B + 128) >> 8 on integer arrays."""
    r, g, b = (np.asarray(c).astype(np.int64) for c in (r, g, b))
    return (77 * r + 150 * g + 29 * b + 128) >> 8


def quant(v):
    """quant_u8(v, 0, 1): clamp, x 255, round half to even, all in fp32."""
    v = np.clip(np.asarray(v, dtype=np.float32), np.float32(0), np.float32(1))
    return np.rint(v * np.float32(255)).astype(np.int64)


def luma(frame, layout):
    """int64 [h, w] luma of one frame: uint8 [h,w,3|4] ('hwc_rgb' / 'hwc_bgr'), float [3,h,w] ('chw'), or the Y plane
    [h,w] of a 4:2:0 frame ('nv12' / 'i420')."""
    frame = np.asarray(frame)
    if layout in ('nv12', 'i420'):
        return frame.astype(np.int64)
    if layout == 'chw':
        return luma_rgb(quant(frame[0]), quant(frame[1]), quant(frame[2]))
    c = (0, 1, 2) if layout == 'hwc_rgb' else (2, 1, 0)
    return luma_rgb(frame[..., c[0]], frame[..., c[1]], frame[..., c[2]])


def luma_sad(frames, layout):
    """int64 [T - 1]: sum |Y8_t - Y8_(t-1)| over the frame."""
    ys = [luma(f, layout) for f in frames]
    return np.array([int(np.abs(ys[t] - ys[t - 1]).sum()) for t in range(1, len(ys))], dtype=np.int64)


def scene_scores(sad, h, w):
    """float64 [T]: mafd_t = 100 SAD_t / (255 h w), mafd_0 = 0, score_t = min(mafd_t, |mafd_t - mafd_(t-1)|)."""
    mafd = np.concatenate([[0.0], 100.0 * np.asarray(sad, dtype=np.float64) / (255.0 * h * w)])
    prev = np.concatenate([[0.0], mafd[:-1]])
    return np.minimum(mafd, np.abs(mafd - prev))


def detect_cuts(sad, h, w, threshold):
    s = scene_scores(sad, h, w)
    return [t for t in range(1, len(s)) if s[t] >= threshold]


def scene_video(seed=0, h=24, w=40, lengths=(5, 4, 5)):
    """A seeded uint8 RGB video [T,h,w,3] of len(lengths) scenes with hard cuts between them.  Every scene is one smooth
    field (a few low-frequency waves around its own mean level) translated by a pixel per frame."""
    rng = np.random.RandomState(seed)
    levels = (40.0, 215.0, 60.0, 230.0, 20.0)
    yy, xx = np.mgrid[0:h, 0:w + 16].astype(np.float64)
    out = []
    for s, n in enumerate(lengths):
        chans = []
        for c in range(3):
            ph = rng.uniform(0, 2 * np.pi, 3)
            f = levels[s % len(levels)] + 8.0 * (np.sin(2 * np.pi * xx / 37.0 + ph[0]) + np.sin(2 * np.pi * yy / 29.0 + ph[1]) +
                                                 np.sin(2 * np.pi * (xx + yy) / 53.0 + ph[2]))
            chans.append(f)
        field = np.clip(np.rint(np.stack(chans, -1)), 0, 255).astype(np.uint8)
        for k in range(n):
            out.append(field[:, k:k + w])
    return np.ascontiguousarray(np.stack(out))


def rgb_to_nv12(video):
    """The packed NV12 [T, h*3/2, w] of a uint8 RGB video (h, w even) whose Y plane is luma_rgb of the pixels; the chroma is
    mid-grey (it plays no part in cut detection)."""
    T, h, w, _ = video.shape
    y = luma_rgb(video[..., 0], video[..., 1], video[..., 2]).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([y, np.full((T, h // 2, w), 128, np.uint8)], axis=1))
