"""The resampler of csrc/frame_resize.hip restated in fp64 numpy: the yardstick of test_resize_host.py and
test_gpu_resize.py.  A helper, not a conftest.

Separable antialiased bicubic: Keys' kernel with a = -0.5, half-pixel centres, the support widened by the down-scale ratio --
torch.nn.functional.interpolate(x, size, mode='bicubic', antialias=True, align_corners=False).  Per axis, n_in -> n_out:

    scale = n_in / n_out;  support = 2 scale and inv = 1 / scale if scale >= 1, else 2 and 1
    output i:  c = scale (i + 0.5),  first = max(0, int(c - support + 0.5)),  end = min(n_in, int(c + support + 0.5))
    w_j = k((j - c + 0.5) inv) for j in [first, end), divided by their sum
    k(x) = ((a+2)|x| - (a+3)) x^2 + 1 for |x| < 1,  a (((|x| - 5)|x| + 8)|x| - 4) for 1 <= |x| < 2,  0 otherwise

The window is cut at the edge of the image and renormalised.  Quantised outputs are compared through LEVELS before rounding,
as in yuv_ref.py, so that a test can tell a value that the arithmetic decides from one that sits on a tie."""
import numpy as np

A = -0.5


def keys(x):
    x = np.abs(np.asarray(x, np.float64))
    near = ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    far = A * (((x - 5.0) * x + 8.0) * x - 4.0)
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def axis_table(n_in, n_out):
    """(first int [n_out], weights fp64 [n_out, taps]) of one axis; rows shorter than taps are zero-padded."""
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    rows = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        first = max(0, int(c - support + 0.5))
        end = min(n_in, int(c + support + 0.5))
        k = keys((np.arange(first, end) - c + 0.5) * inv)
        rows.append((first, k / k.sum()))
    taps = max(len(k) for _, k in rows)
    first = np.array([f for f, _ in rows], np.int64)
    weights = np.zeros((n_out, taps), np.float64)
    for i, (_, k) in enumerate(rows):
        weights[i, :len(k)] = k
    return first, weights


def axis_matrix(n_in, n_out):
    """The axis as a dense fp64 [n_out, n_in] matrix."""
    first, weights = axis_table(n_in, n_out)
    m = np.zeros((n_out, n_in), np.float64)
    for i in range(n_out):
        n = min(weights.shape[1], n_in - first[i])
        m[i, first[i]:first[i] + n] = weights[i, :n]
    return m


def resize(x, size):
    """fp64 [..., h, w] -> [..., oh, ow]: columns first, then rows."""
    x = np.asarray(x, np.float64)
    oh, ow = size
    y = x @ axis_matrix(x.shape[-1], ow).T
    return np.swapaxes(np.swapaxes(y, -1, -2) @ axis_matrix(x.shape[-2], oh).T, -1, -2)


def bound(n_in_out_pairs):
    """The fp32 bar of a case: 3 (n + 1) 2^-24, n the larger tap count of its axes -- two passes, each with weights rounded to
    fp32 and a sum of n products, the second on values of up to sum |w| ~ 1.25 times the input."""
    n = max(axis_table(a, b)[1].shape[1] for a, b in n_in_out_pairs)
    return 3.0 * (n + 1) * 2.0 ** -24, n


def levels_u8(v, lo=0.0, hi=1.0):
    """fp64 values -> 8-bit levels BEFORE rounding (clamp to [lo,hi], rescale, x 255)."""
    return (np.clip(np.asarray(v, np.float64), lo, hi) - lo) / (hi - lo) * 255.0


def to_bytes(levels):
    """Round half to even, clamp to 0 .. 255."""
    return np.clip(np.rint(levels), 0, 255).astype(np.uint8)


def tie_distance(levels, top=255.0):
    """How far a pre-rounding level is from the nearest tie x.5 (levels that the clamp decides are far from any)."""
    v = np.asarray(levels, np.float64)
    d = np.abs(v - np.floor(v) - 0.5)
    return np.where((v < -0.5) | (v > top + 0.5), 0.5, d)


# (crop h x w, buffer Hs x Ws, target oh x ow) of the GPU tests: both axes at a non-integer ratio with ow % 4 != 0 | one axis
# only | the other axis only | ratio 4 | ratio 4 from a crop | up-scaling x 2 and x 1.4 | equal sizes | more than one
# workgroup tile (64 columns, at most 32 rows) each way
CASES = [((37, 53), (40, 56), (21, 30)), ((40, 56), (40, 56), (40, 31)), ((33, 47), (36, 48), (9, 47)),
         ((64, 96), (64, 96), (16, 24)), ((61, 93), (64, 96), (16, 24)), ((12, 20), (12, 20), (24, 40)),
         ((12, 20), (12, 20), (17, 29)), ((20, 20), (20, 20), (20, 20)), ((148, 212), (152, 216), (83, 119))]
