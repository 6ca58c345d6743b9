"""Frame-window indexing of the reference's test datasets (codes/data/util.py:114 `index_generation`, used by
video_test_dataset_int.py:219 and demo.py:66), restated from its docstring contract.

A window of N frames is centred on frame `crt_i` of a sequence of `max_n` frames.  Positions inside the sequence are
taken as they are; a position that falls off either end is replaced according to `padding` (crt_i = 0, N = 5):

    replicate   [0, 0, 0, 1, 2]   the border frame, repeated
    reflection  [2, 1, 0, 1, 2]   mirrored about the border frame
    new_info    [4, 3, 0, 1, 2]   frames from beyond the window's far end: every entry is a different frame
    circle      [3, 4, 0, 1, 2]   shifted by N (a missing position p takes p + N at the start, p - N at the end)

Also here, with the reference's signatures: the YCbCr conversions (rgb2ycbcr, bgr2ycbcr, ycbcr2rgb) and MATLAB's imresize
(modcrop, imresize, imresize_np; the arithmetic of the latter two runs on the GPU).
"""

PADDING_MODES = ('replicate', 'reflection', 'new_info', 'circle')


def index_generation(crt_i, max_n, N, padding='reflection'):
    """-> the N frame indices of the window centred on `crt_i` in a sequence of `max_n` frames (list of int)."""
    if padding not in PADDING_MODES:
        raise ValueError('Wrong padding mode %r (one of %s)' % (padding, ' | '.join(PADDING_MODES)))
    last, half = max_n - 1, N // 2
    lo, hi = crt_i - half, crt_i + half
    before = {'replicate': lambda p: 0, 'reflection': lambda p: -p, 'new_info': lambda p: hi - p,
              'circle': lambda p: p + N}[padding]
    after = {'replicate': lambda p: last, 'reflection': lambda p: 2 * last - p, 'new_info': lambda p: lo - (p - last),
             'circle': lambda p: p - N}[padding]
    return [before(p) if p < 0 else (after(p) if p > last else p) for p in range(lo, hi + 1)]


# ---- YCbCr (BT.601, limited range: MATLAB's rgb2ycbcr / ycbcr2rgb), as the reference's data/util.py offers them ------------------
# An image is [..., 3] in the named channel order: uint8 in [0, 255] (the result is rounded half to even and cast back) or float
# in [0, 1] (the result is in [0, 1], in the input's dtype).  Unlike the reference's, these never scale the caller's array in
# place.  The arithmetic runs in numpy's promotion of (image dtype, float64) in the order written here, which is the order
# whose results tests/golden/ycbcr_reference.npz and score_reference.npz record.
_Y_FROM_RGB = (65.481, 128.553, 24.966)
_YCBCR_FROM_RGB = ((65.481, -37.797, 112.0), (128.553, -74.203, -93.786), (24.966, 112.0, -18.214))
_RGB_FROM_YCBCR = ((0.00456621, 0.00456621, 0.00456621), (0, -0.00153632, 0.00791071), (0.00625893, -0.00318811, 0))


def _colour_levels(img):
    """(the image on the 0 .. 255 scale -- a new array unless it is uint8 --, it is uint8, its dtype)"""
    import numpy as np
    img = np.asarray(img)
    is_u8 = img.dtype == np.uint8
    return (img if is_u8 else img * 255.), is_u8, img.dtype


def _colour_result(levels, is_u8, dtype):
    return (levels.round() if is_u8 else levels / 255.).astype(dtype)


def rgb2ycbcr(img, only_y=True):
    """RGB [..., 3] -> Y [...] (only_y) or YCbCr [..., 3]: Y = (65.481 R + 128.553 G + 24.966 B) / 255 + 16 on the 0 .. 255 scale."""
    import numpy as np
    x, is_u8, dtype = _colour_levels(img)
    if only_y:
        levels = np.dot(x, list(_Y_FROM_RGB)) / 255.0 + 16.0
    else:
        levels = np.matmul(x, [list(r) for r in _YCBCR_FROM_RGB]) / 255.0 + [16, 128, 128]
    return _colour_result(levels, is_u8, dtype)


def bgr2ycbcr(img, only_y=True):
    """rgb2ycbcr for an image in BGR order (cv2's)."""
    import numpy as np
    x, is_u8, dtype = _colour_levels(img)
    if only_y:
        levels = np.dot(x, list(_Y_FROM_RGB[::-1])) / 255.0 + 16.0
    else:
        levels = np.matmul(x, [list(r) for r in _YCBCR_FROM_RGB[::-1]]) / 255.0 + [16, 128, 128]
    return _colour_result(levels, is_u8, dtype)


def ycbcr2rgb(img):
    """YCbCr [..., 3] -> RGB [..., 3], the inverse of rgb2ycbcr(only_y=False) with MATLAB's rounded coefficients."""
    import numpy as np
    x, is_u8, dtype = _colour_levels(img)
    levels = np.matmul(x, [list(r) for r in _RGB_FROM_YCBCR]) * 255.0 + [-222.921, 135.576, -276.836]
    return _colour_result(levels, is_u8, dtype)


# ---- MATLAB's imresize, as the reference's data/util.py offers it (:302-524) ---------------------------------------------------
# The arithmetic runs on the GPU (dynavsr_amd.frames.imresize, csrc/frame_imresize.hip): as with Degradation.apply there is no
# CPU arithmetic path, and a CPU input is copied to the current device and the result back.
def modcrop(img_in, scale):
    """img_in: numpy, HWC or HW -> a copy of its top-left (H - H % scale) x (W - W % scale)."""
    import numpy as np
    img = np.copy(img_in)
    if img.ndim not in (2, 3):
        raise ValueError('Wrong img ndim: [{:d}].'.format(img.ndim))
    H, W = img.shape[:2]
    return np.copy(img[:H - H % scale, :W - W % scale])


def imresize(img, scale, antialiasing=True):
    """MATLAB's imresize(img, scale, 'bicubic').  img: a [3,H,W] tensor (RGB or BGR alike) in [0,1]; scale: 1/2, 1/3, 1/4, 2, 3 or 4
    within 1e-9 (ValueError otherwise).  -> fp32 [3, ceil(H scale), ceil(W scale)], not rounded, on the device img lives on."""
    import torch
    from dynavsr_amd import frames
    ratio = frames.imresize_ratio(scale, "imresize")
    if not torch.is_tensor(img) or img.dim() != 3 or img.shape[0] != 3 or not img.is_floating_point():
        raise ValueError("imresize: img must be a float [3,H,W] tensor, got %s" % (
            "%s %s" % (img.dtype, tuple(img.shape)) if torch.is_tensor(img) else type(img).__name__))
    out = frames.imresize(img, ratio, 'chw', antialiasing=antialiasing)
    return out if img.is_cuda else out.cpu()


def imresize_np(img, scale, antialiasing=True):
    """imresize for a numpy image [H,W,3] in [0,1] (any channel order) -> float32 [ceil(H scale), ceil(W scale), 3]."""
    import numpy as np
    import torch
    from dynavsr_amd import frames
    ratio = frames.imresize_ratio(scale, "imresize_np")
    img = np.asarray(img)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype.kind != 'f':
        raise ValueError("imresize_np: img must be a float [H,W,3] array, got %s %s" % (img.dtype, img.shape))
    chw = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1), dtype=np.float32))
    return np.ascontiguousarray(frames.imresize(chw, ratio, 'chw', antialiasing=antialiasing).cpu().numpy().transpose(1, 2, 0))
