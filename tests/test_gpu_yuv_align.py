"""GPU: every alignment class of the 4:2:0 sample groups (csrc/frame_yuv.hip: groups of 1 / 2 / 4 samples at any legal address,
moved in naturally aligned pieces), for all six layouts of dynavsr_amd/frames.py.

Every plane is a view inside a sentinel-filled buffer whose base is 8-byte aligned, at each byte offset o in range(0, 8, B)
(B = bytes per sample), with a row pitch one sample longer than the row: consecutive rows walk through the alignment classes of
the 4-sample group (mod 4 bytes for 8-bit samples, mod 8 bytes for 16-bit words).  6 x 10 and 7 x 9 frames, padded to 8 x 12,
hold an interior block, a ragged block, padded rows and columns and an odd last chroma row and column.  The yardstick is the
same call on contiguous copies of the same planes: bit equality, no tolerance; and not a byte outside the planes' rows changes."""
import numpy as np
import pytest
import torch

from dynavsr_amd import frames

pytestmark = pytest.mark.gpu

LAYOUTS = {'nv12': (8, 0), 'i420': (8, 0), 'p010': (10, 6), 'p012': (12, 4), 'i420p10': (10, 0), 'i420p12': (12, 0)}  # depth, shift
SEMI = ('nv12', 'p010', 'p012')
SIZES = [(6, 10), (7, 9)]
PADDED = (8, 12)
GUARD = 8                     # sentinel bytes ahead of the first row (a multiple of 8: the offset o stays the view's alignment)


def plane_shapes(h, w, layout):
    hc, wc = (h + 1) // 2, (w + 1) // 2
    return [(h, w), (hc, wc, 2)] if layout in SEMI else [(h, w), (hc, wc), (hc, wc)]


def offset_view(shape, dtype, o):
    """(buffer, view): a plane of `shape` at byte offset GUARD + o of a sentinel-filled uint8 buffer, its rows one sample more
    than a row apart."""
    es = torch.empty((), dtype=dtype).element_size()
    assert o % es == 0
    row = shape[1] * (shape[2] if len(shape) == 3 else 1)
    pitch = row + 1
    n = GUARD + o + shape[0] * pitch * es + GUARD
    buf = torch.full((n + n % 2,), 0x5A, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 8 == 0
    view = buf.view(dtype).as_strided(shape, (pitch,) + ((2, 1) if len(shape) == 3 else (1,)), (GUARD + o) // es)
    assert view.data_ptr() == buf.data_ptr() + GUARD + o
    return buf, view


def offset_planes(h, w, layout, o):
    dtype = torch.uint8 if LAYOUTS[layout][0] == 8 else torch.int16
    pairs = [offset_view(s, dtype, o) for s in plane_shapes(h, w, layout)]
    return [b for b, _ in pairs], tuple(v for _, v in pairs)


def untouched_outside(bufs, planes):
    """Every sentinel between rows, before the first row and after the last row is still there."""
    for buf, p in zip(bufs, planes):
        rest, es = buf.clone(), p.element_size()
        rest.view(p.dtype).as_strided(p.shape, p.stride(), (p.data_ptr() - buf.data_ptr()) // es).fill_(0x5A5A if es == 2 else 0x5A)
        if not bool((rest == 0x5A).all()):
            return False
    return True


_CASES = {}


def case(h, w, layout):
    """Per (size, layout), computed once and never modified: seeded random word planes on the device (contiguous), their
    ingest, a seeded fp32 image and its emit into contiguous planes."""
    key = (h, w, layout)
    if key not in _CASES:
        depth, shift = LAYOUTS[layout]
        r = np.random.RandomState(1000 * h + 10 * w + depth + shift)
        words = [r.randint(0, 2 ** depth, s) << shift for s in plane_shapes(h, w, layout)]
        src = tuple(torch.from_numpy(v.astype(np.uint8) if depth == 8 else v.astype(np.uint16).view(np.int16)).cuda() for v in words)
        assert all(p.is_contiguous() for p in src)
        rgb = frames.ingest(src, layout, 4, 'reflect')
        assert rgb.shape == (3,) + PADDED
        sr = torch.from_numpy(r.uniform(-0.2, 1.2, (3,) + PADDED).astype(np.float32)).cuda()
        dst = tuple(torch.zeros_like(p) for p in src)
        assert frames.emit(sr, h, w, layout, out=dst) is dst
        _CASES[key] = dict(src=src, rgb=rgb, sr=sr, dst=dst)
    return _CASES[key]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_every_alignment_class(size, layout):
    h, w = size
    c = case(h, w, layout)
    B = 1 if LAYOUTS[layout][0] == 8 else 2
    for o in range(0, 8, B):
        bufs, planes = offset_planes(h, w, layout, o)
        assert all(p.data_ptr() % 8 == o for p in planes)
        for p, s in zip(planes, c['src']):
            p.copy_(s)
        assert untouched_outside(bufs, planes), o                                # (the test's own views are what they claim)
        kept = frames.describe_yuv(planes, layout, h, w)[0]
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(kept, planes))   # passed by stride, not copied
        got = frames.ingest(planes, layout, 4, 'reflect')
        assert torch.equal(got, c['rgb']), (o, "ingest")
        assert untouched_outside(bufs, planes), (o, "ingest wrote to its source")
        for p in planes:
            p.fill_(0x5A5A if B == 2 else 0x5A)
        assert frames.emit(c['sr'], h, w, layout, out=planes) is planes
        for i, (p, d) in enumerate(zip(planes, c['dst'])):
            assert torch.equal(p, d), (o, "emit", i)
        assert untouched_outside(bufs, planes), (o, "emit")
