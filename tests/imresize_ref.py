"""A float64 restatement of the definition behind dvsr_frame_imresize (include/dynavsr_hip.h), for the tests:
MATLAB's bicubic imresize per axis -- calculate_weights_indices of the reference evaluated in double -- with the taps beyond
either edge folded back onto the image by the periodic symmetric rule and added to the taps they land on.  No torch, no library:
plain Python floats in the order the header writes, so that the fp32 rounding of a weight is the library's."""
import math

import numpy as np

SCALES = ((1, 2), (1, 3), (1, 4), (2, 1), (3, 1), (4, 1))      # num / den


def cubic(x):
    ax = abs(x)
    ax2 = ax * ax
    ax3 = ax2 * ax
    if ax <= 1.0:
        return 1.5 * ax3 - 2.5 * ax2 + 1.0
    if ax <= 2.0:
        return -0.5 * ax3 + 2.5 * ax2 - 4.0 * ax + 2.0
    return 0.0


def n_out(n_in, num, den):
    return -(-n_in * num // den)


def fold(j, n_in):
    """MATLAB's symmetric copy, continued periodically: -k -> k - 1, n_in - 1 + k -> n_in - k."""
    m = j % (2 * n_in)
    return m if m < n_in else 2 * n_in - 1 - m


def axis_rows(n_in, num, den, antialiasing=True):
    """[(first, [w_0 .. w_len-1] in double)] per output: the folded window."""
    scale = num / den
    wide = num < den and antialiasing
    kw = 4.0 / scale if wide else 4.0
    P = math.ceil(kw) + 2
    rows = []
    for i in range(n_out(n_in, num, den)):
        u = (i + 1) / scale + 0.5 * (1.0 - 1.0 / scale)
        left = math.floor(u - kw / 2.0)
        k, total = [], 0.0
        for t in range(P):
            d = u - (left + t)
            v = scale * cubic(d * scale) if wide else cubic(d)
            k.append(v)
            total += v
        k = [v / total for v in k]
        j = [fold(left + t - 1, n_in) for t in range(P)]
        hit = [jt for jt, v in zip(j, k) if v != 0.0]
        lo, hi = min(hit), max(hit)
        w = [0.0] * (hi - lo + 1)
        for jt, v in zip(j, k):
            if v != 0.0:
                w[jt - lo] += v
        rows.append((lo, w))
    return rows


def axis_table(n_in, num, den, antialiasing=True):
    """(first int32 [n_out], weights fp32 [n_out, taps]), taps the longest window: what dvsr_frame_imresize_table fills."""
    rows = axis_rows(n_in, num, den, antialiasing)
    taps = max(len(w) for _, w in rows)
    first = np.array([f for f, _ in rows], dtype=np.int32)
    weights = np.zeros((len(rows), taps), dtype=np.float32)
    for i, (_, w) in enumerate(rows):
        weights[i, :len(w)] = np.asarray(w, dtype=np.float64).astype(np.float32)
    return first, weights


def axis_matrix(n_in, num, den, antialiasing=True):
    """The fp32 table as a dense float64 [n_out, n_in] matrix."""
    first, weights = axis_table(n_in, num, den, antialiasing)
    m = np.zeros((first.shape[0], n_in), dtype=np.float64)
    for i, f in enumerate(first):
        for t in range(weights.shape[1]):
            if weights[i, t] != 0.0:
                m[i, f + t] += float(weights[i, t])
    return m


def imresize(img, num, den, antialiasing=True):
    """img [C,H,W] (any float dtype; taken as float64) -> float64 [C, n_out(H), n_out(W)]: the fp32 tables applied in float64."""
    img = np.asarray(img, dtype=np.float64)
    mr, mc = axis_matrix(img.shape[1], num, den, antialiasing), axis_matrix(img.shape[2], num, den, antialiasing)
    return np.einsum('oh,chw,pw->cop', mr, img, mc)


def fold_reference(weights, indices, sym_len_s, n_in):
    """The reference's calculate_weights_indices output -- weights [n_out, P'] and 0-based indices into its symmetric-padded
    copy, which starts sym_len_s samples before the image -- folded onto the image: a dense float64 [n_out, n_in] matrix."""
    m = np.zeros((weights.shape[0], n_in), dtype=np.float64)
    for i in range(weights.shape[0]):
        for t in range(weights.shape[1]):
            m[i, fold(int(indices[i, t]) - int(sym_len_s), n_in)] += float(weights[i, t])
    return m


def quantise(y):
    """The library's one quantiser on float64 values: levels 0 .. 255."""
    return np.rint(np.clip(255.0 * y, 0.0, 255.0))
