"""Frame-window indexing of the reference's test datasets (codes/data/util.py:114 `index_generation`, used by
video_test_dataset_int.py:219 and demo.py:66), restated from its docstring contract.

A window of N frames is centred on frame `crt_i` of a sequence of `max_n` frames.  Positions inside the sequence are
taken as they are; a position that falls off either end is replaced according to `padding` (crt_i = 0, N = 5):

    replicate   [0, 0, 0, 1, 2]   the border frame, repeated
    reflection  [2, 1, 0, 1, 2]   mirrored about the border frame
    new_info    [4, 3, 0, 1, 2]   frames from beyond the window's far end: every entry is a different frame
    circle      [3, 4, 0, 1, 2]   shifted by N (a missing position p takes p + N at the start, p - N at the end)
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
