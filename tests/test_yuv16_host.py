"""CPU: the host side of the 10- / 12-bit YCbCr 4:2:0 frame path -- the fp64 restatement at a depth (tests/yuv16_ref.py) against
the 8-bit one (tests/yuv_ref.py) and H.273's anchor points, the layout rules of dynavsr_amd/frames.py for 'p010' / 'p012' /
'i420p10' / 'i420p12', and the argument checks of the three C entry points and of dvsr_frame_luma_sad's 16-bit formats, which
return DVSR_ERR_INVALID before any launch -- so they run without a GPU, with pointers that are never dereferenced."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import yuv16_ref
import yuv_ref
from dynavsr_amd import adapt, frames

INVALID = -1
A16 = 0x10000           # a 16-byte aligned address that nothing reads
PAIRS = list(itertools.product(('bt601', 'bt709'), ('limited', 'full')))
LAYOUTS16 = ('p010', 'p012', 'i420p10', 'i420p12')


@pytest.fixture(scope="module")
def lib():
    from dynavsr_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        from dynavsr_amd import build
        build.build()
    return _lib


# ---- the restatement
@pytest.mark.parametrize("matrix,yuv_range", PAIRS)
def test_depth_8_is_the_8_bit_restatement_to_the_last_bit(matrix, yuv_range):
    r = np.random.RandomState(8)
    assert yuv16_ref.level_scale(8, yuv_range) == yuv_ref.RANGES[yuv_range] + (128.0,)
    y, cb, cr = (r.randint(0, 256, (7, 9)), r.randint(0, 256, (4, 5)), r.randint(0, 256, (4, 5)))
    for mode in ('reflect', 'replicate'):
        a = yuv16_ref.ingest(y, cb, cr, 8, 12, 8, mode, matrix, yuv_range)
        b = yuv_ref.ingest(y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8), 8, 12, mode, matrix, yuv_range)
        assert a.dtype == np.float64 and np.array_equal(a, b)
    sr = r.uniform(-0.2, 1.2, (3, 8, 16))
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0)):
        for a, b in zip(yuv16_ref.emit(sr, 7, 13, 8, lo, hi, matrix, yuv_range), yuv_ref.emit(sr, 7, 13, lo, hi, matrix, yuv_range)):
            assert np.array_equal(a, b)
            assert np.array_equal(yuv16_ref.to_levels(a, 8), yuv_ref.to_bytes(b))
            assert np.array_equal(yuv16_ref.tie_distance(a, 8), yuv_ref.tie_distance(b))
    t = r.uniform(0, 255, (3, 50))
    assert np.array_equal(yuv16_ref.ycbcr_to_rgb(*t, 8, matrix, yuv_range, clamp=False), yuv_ref.ycbcr_to_rgb(*t, matrix, yuv_range, clamp=False))


def test_h273_anchor_points():
    grey = dict(atol=1e-15)
    assert np.allclose(yuv16_ref.ycbcr_to_rgb(64, 512, 512, 10, 'bt709', 'limited'), 0.0, **grey)        # 10-bit limited black
    assert np.allclose(yuv16_ref.ycbcr_to_rgb(940, 512, 512, 10, 'bt709', 'limited'), 1.0, **grey)       # ... white
    assert np.allclose(yuv16_ref.ycbcr_to_rgb(502, 512, 512, 10, 'bt601', 'limited'), 0.5, **grey)       # Cb = Cr = 512: grey
    assert np.allclose(yuv16_ref.ycbcr_to_rgb(4095, 2048, 2048, 12, 'bt601', 'full'), 1.0, **grey)       # 12-bit full white
    assert np.allclose(yuv16_ref.ycbcr_to_rgb(0, 2048, 2048, 12, 'bt601', 'full'), 0.0, **grey)
    assert yuv16_ref.level_scale(10, 'limited') == (64.0, 876.0, 896.0, 512.0)
    assert yuv16_ref.level_scale(12, 'limited') == (256.0, 3504.0, 3584.0, 2048.0)
    assert yuv16_ref.level_scale(10, 'full') == (0.0, 1023.0, 1023.0, 512.0)
    for depth, (matrix, yuv_range) in itertools.product((10, 12), PAIRS):
        y0, ys, cs, cm = yuv16_ref.level_scale(depth, yuv_range)
        kr, kb = yuv_ref.MATRICES[matrix]
        y, cb, cr = yuv16_ref.rgb_to_ycbcr(np.array([1.0, 0.0, 0.0]), depth, matrix, yuv_range)         # red: Cr at the top
        assert abs(y - (y0 + ys * kr)) < 1e-9 and abs(cr - (cm + cs / 2)) < 1e-9
        y, cb, cr = yuv16_ref.rgb_to_ycbcr(np.array([0.0, 0.0, 1.0]), depth, matrix, yuv_range)         # blue: Cb at the top
        assert abs(y - (y0 + ys * kb)) < 1e-9 and abs(cb - (cm + cs / 2)) < 1e-9
        r = np.random.RandomState(depth).uniform(0, 1, (3, 50))
        back = yuv16_ref.ycbcr_to_rgb(*yuv16_ref.rgb_to_ycbcr(r, depth, matrix, yuv_range), depth, matrix, yuv_range, clamp=False)
        assert np.abs(back - r).max() < 1e-12
        top = 2 ** depth - 1
        assert yuv16_ref.ycbcr_to_rgb(top, top, top, depth, matrix, yuv_range).max() == 1.0              # clamped, not wrapped
        assert yuv16_ref.to_levels(np.array([-3.0, 0.5, 1.5, 2.5, top + 0.49, top + 7.0]), depth).tolist() == \
            [0, 0, 2, 2, top, top]                                                                       # half to even, clamp


def test_words_of_the_two_storages():
    lev = np.array([0, 1, 513, 1023])
    assert yuv16_ref.to_words(lev, 'msb', 10).tolist() == [0, 64, 513 << 6, 1023 << 6]
    assert yuv16_ref.to_words(lev, 'lsb', 10).tolist() == [0, 1, 513, 1023]
    assert yuv16_ref.to_words(np.array([4095]), 'msb', 12).tolist() == [0xfff0]
    junk = np.array([0xffff, 0x1234, 7, 0x8001])
    for storage, depth in (('msb', 10), ('msb', 12), ('lsb', 10), ('lsb', 12)):
        lev = np.random.RandomState(depth).randint(0, 2 ** depth, 4)
        w = yuv16_ref.to_words(lev, storage, depth, junk)
        assert w.dtype == np.uint16
        got, rest = yuv16_ref.from_words(w, storage, depth)
        assert np.array_equal(got, lev) and np.array_equal(rest, junk & (2 ** (16 - depth) - 1))
        assert not np.array_equal(w, yuv16_ref.to_words(lev, storage, depth))                            # the junk is in the word
    y, cb, cr = (np.arange(24, dtype=np.uint16).reshape(4, 6) * 40, np.arange(6, dtype=np.uint16).reshape(2, 3),
                 np.arange(6, 12, dtype=np.uint16).reshape(2, 3))
    for layout in LAYOUTS16:
        packed = yuv16_ref.pack(y, cb, cr, layout)
        assert packed.shape == (6, 6) and packed.dtype == np.uint16
        assert all(np.array_equal(a, b) for a, b in zip(yuv16_ref.unpack(packed, layout), (y, cb, cr)))


# ---- layout rules
def test_16_bit_layouts_are_never_inferred_and_come_packed_or_as_planes():
    assert frames.YUV16_LAYOUTS == LAYOUTS16 and frames.YUV_LAYOUTS == ('nv12', 'i420')
    packed = torch.zeros(9, 8, dtype=torch.uint16)                              # 6 x 8
    with pytest.raises(ValueError):
        frames.resolve_layout(packed)                                           # a 2-D uint16 tensor with layout None
    with pytest.raises(ValueError):
        frames.ingest(packed)
    for layout in LAYOUTS16:
        semi = layout in ('p010', 'p012')
        for fr in (packed, packed.view(torch.int16)):                           # int16: the same bits
            assert frames.resolve_layout(fr, layout) == (layout, 6, 8)
            planes, h, w = frames.yuv_planes(fr, layout)
            assert (h, w) == (6, 8) and planes[0].shape == (6, 8) and planes[0].data_ptr() == fr.data_ptr()
            assert [tuple(p.shape) for p in planes[1:]] == ([(3, 4, 2)] if semi else [(3, 4), (3, 4)])
            assert planes[1].data_ptr() == fr.data_ptr() + 2 * 48
            if not semi:
                assert planes[2].data_ptr() == fr.data_ptr() + 2 * 60
        for bad in (torch.zeros(9, 7, dtype=torch.uint16),                      # odd width: planes only
                    torch.zeros(8, 8, dtype=torch.uint16),                      # rows not 3/2 of an even height
                    torch.zeros(9, 8, dtype=torch.uint8),                       # 8-bit samples in a 16-bit layout
                    torch.zeros(9, 8, dtype=torch.int32), torch.zeros(9, 8),
                    torch.zeros(9, 8, 1, dtype=torch.uint16), None, layout,
                    (packed,), (packed[:6],), (packed[:6],) * 4):
            with pytest.raises(ValueError):
                frames.resolve_layout(bad, layout)
            with pytest.raises(ValueError):
                frames.ingest(bad, layout)                                      # ... said before any GPU call
    for layout in ('nv12', 'i420'):                                             # and uint16 is no 8-bit frame
        with pytest.raises(ValueError, match="uint8"):
            frames.resolve_layout(packed, layout)
    # a pitched packed frame: semi-planar by stride, planar refused
    wide = torch.zeros(9, 12, dtype=torch.uint16)[:, 2:10]
    planes, _, _ = frames.yuv_planes(wide, 'p010')
    assert planes[1].stride() == (12, 2, 1) and planes[1].data_ptr() == wide.data_ptr() + 2 * 6 * 12
    with pytest.raises(ValueError, match="contiguous"):
        frames.yuv_planes(wide, 'i420p10')
    # planes: odd sizes in this form only
    y, uv, u, v = (torch.zeros(7, 9, dtype=torch.uint16), torch.zeros(4, 5, 2, dtype=torch.uint16),
                   torch.zeros(4, 5, dtype=torch.uint16), torch.zeros(4, 5, dtype=torch.int16))
    assert frames.resolve_layout((y, uv), 'p012') == ('p012', 7, 9)
    assert frames.resolve_layout([y, u, v], 'i420p12') == ('i420p12', 7, 9)
    for bad, layout in (((y, u, v), 'p010'), ((y, uv), 'i420p10'), ((y, u), 'p010'), ((y, uv[:3]), 'p010'),
                        ((y, u, v[:, :4]), 'i420p10'), ((y, u.float(), v), 'i420p10'), ((y[0], u, v), 'i420p10'),
                        ((y, u.view(torch.uint8)[:, :5], v), 'i420p10'), ((y, uv), 'p016'), ((y, uv), None), ((y, uv), 'nv12')):
        with pytest.raises(ValueError):
            frames.resolve_layout(bad, layout)


def test_describe_passes_pitched_and_offset_planes_by_stride():
    buf = torch.zeros(4096, dtype=torch.uint16)
    y = buf.as_strided((7, 9), (13, 1), 1)
    uv = buf.as_strided((4, 5, 2), (15, 2, 1), 201)
    u = buf.as_strided((4, 5), (7, 1), 301)
    v = buf.as_strided((4, 5), (9, 1), 403).view(torch.int16)
    planes, d = frames.describe_yuv((y, uv), 'p010', 7, 9)
    assert type(d).__name__ == 'Yuv16Desc'
    assert [p.data_ptr() for p in planes] == [y.data_ptr(), uv.data_ptr()] and y.data_ptr() == buf.data_ptr() + 2
    assert (d.format, d.depth, d.h, d.w, d.matrix, d.range) == (0, 10, 7, 9, 0, 0)
    assert (d.plane[0], d.plane[1], d.plane[2]) == (y.data_ptr(), uv.data_ptr(), None)
    assert tuple(d.row_stride)[:2] == (26, 30)                                  # bytes
    assert frames.describe_yuv((y, uv), 'p012', 7, 9)[1].depth == 12
    planes, d = frames.describe_yuv((y, u, v), 'i420p12', 7, 9, 'bt709', 'full')
    assert (d.format, d.depth, d.matrix, d.range) == (1, 12, 1, 1)
    assert tuple(d.plane) == (y.data_ptr(), u.data_ptr(), v.data_ptr()) and tuple(d.row_stride) == (26, 14, 18)
    assert frames.describe_yuv((y, u, v), 'i420p10', 7, 9)[1].depth == 10
    skip = buf.as_strided((4, 5), (20, 2), 0)                                   # a column stride no descriptor expresses: copied
    planes, d = frames.describe_yuv((y, skip, v), 'i420p10', 7, 9)
    assert planes[1].is_contiguous() and planes[1].dtype == torch.uint16 and d.row_stride[1] == 10
    assert planes[2].data_ptr() == v.data_ptr()
    with pytest.raises(ValueError, match="plane 1"):
        frames.describe_yuv((y, skip, v), 'i420p10', 7, 9, copy=False)          # ... and refused as a destination
    for kw in (dict(matrix='bt2020'), dict(yuv_range='tv')):
        with pytest.raises(ValueError):
            frames.describe_yuv((y, uv), 'p010', 7, 9, **kw)
    d8 = frames.describe_yuv((torch.zeros(6, 8, dtype=torch.uint8), torch.zeros(3, 4, 2, dtype=torch.uint8)), 'nv12', 6, 8)[1]
    assert type(d8).__name__ == 'YuvDesc' and tuple(d8.row_stride)[:2] == (8, 8)


def test_argument_checks_come_before_the_gpu():
    packed = torch.zeros(9, 8, dtype=torch.uint16)
    with pytest.raises(ValueError, match="matrix"):
        frames.ingest(packed, 'p010', matrix='bt2020')
    with pytest.raises(ValueError, match="range"):
        frames.ingest(packed, 'i420p10', yuv_range='pc')
    with pytest.raises(ValueError, match="pad mode"):
        frames.ingest(packed, 'p012', pad_mode='circular')
    with pytest.raises(ValueError, match="reflect"):
        frames.ingest(packed, 'p010', multiple=16)              # 10 rows of padding out of a 6-row frame
    with pytest.raises(ValueError, match="out must be"):
        frames.ingest(packed, 'p010', out=torch.zeros(3, 8, 12))
    sr = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError, match="layout"):
        frames.emit(sr, 8, 8, 'p016')
    with pytest.raises(ValueError, match="crop"):
        frames.emit(sr, 9, 8, 'p010')
    for h, w in ((7, 8), (8, 7), (7, 7)):                       # an odd crop needs planes
        with pytest.raises(ValueError, match="planes"):
            frames.emit(sr, h, w, 'p010')
        with pytest.raises(ValueError):
            frames.emit(sr, h, w, 'i420p12', out=torch.zeros(12, 8, dtype=torch.uint16))
    with pytest.raises(ValueError, match="out is a"):
        frames.emit(sr, 8, 8, 'p010', out=torch.zeros(9, 8, dtype=torch.uint16))
    with pytest.raises(ValueError, match="uint16"):
        frames.emit(sr, 8, 8, 'p010', out=torch.zeros(12, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="matrix"):
        frames.emit(sr, 8, 8, 'i420p10', matrix='rec709')
    with pytest.raises(RuntimeError, match="GPU"):               # a valid call gets as far as the device check
        frames.emit(sr, 8, 8, 'p010')
    with pytest.raises(RuntimeError, match="GPU"):
        frames.emit(sr, 8, 8, 'i420p10', out=torch.zeros(12, 8, dtype=torch.int16))
    with pytest.raises(RuntimeError, match="GPU"):
        frames.emit(sr, 7, 7, 'i420p12', out=(torch.zeros(7, 7, dtype=torch.uint16), torch.zeros(4, 4, dtype=torch.uint16),
                                              torch.zeros(4, 4, dtype=torch.uint16)))
    with pytest.raises(ValueError):
        frames.detect_cuts(torch.zeros(3, 9, 8, dtype=torch.uint16), 'i420p10', threshold=0)


class _Mean(torch.nn.Module):
    nframes = 3

    def forward(self, x):
        return x.mean(1)


def _first(gen):
    return next(iter(gen))


@pytest.mark.parametrize("edvr", [False, True])
def test_super_resolve_frames_checks_16_bit_arguments_first(edvr):
    if edvr:
        from dynavsr_amd.models.archs.EDVR_arch import EDVR
        net = EDVR()                                    # on the CPU: a valid call gets as far as the device check
        opt = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
    else:
        net = _Mean()
        opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    packed = torch.zeros(7, 27, 22, dtype=torch.uint16)                         # 18 x 22
    y, uv = torch.zeros(13, 15, dtype=torch.uint16), torch.zeros(7, 8, 2, dtype=torch.uint16)
    u8 = torch.zeros(7, 18, 22, 3, dtype=torch.uint8)
    bad = [
        dict(frames=packed),                                                    # never inferred
        dict(frames=packed, layout='p016'),
        dict(frames=packed, layout='nv12'),                                     # 16-bit words are no 8-bit frame
        dict(frames=packed, layout='hwc_rgb'),
        dict(frames=packed.view(torch.uint8), layout='p010'),
        dict(frames=u8, layout='p010'),
        dict(frames=packed, layout='p010', matrix='bt2020'),
        dict(frames=packed, layout='i420p10', yuv_range='tv'),
        dict(frames=packed, layout='p010', out='p016'),
        dict(frames=packed, layout='p010', pad_mode='circular'),
        dict(frames=packed[:, :26], layout='p012'),                             # 26 rows are not 3/2 of an even height
        dict(frames=packed[:, :, :21], layout='i420p12'),
        dict(frames=packed[:, :, :20], layout='i420p10'),                       # packed planar must be contiguous
        dict(frames=[(y, uv)] * 3 + [(y, uv[:6])] + [(y, uv)] * 3, layout='p010'),
        dict(frames=[(y, uv)] * 3 + [(y.view(torch.int16), uv)] + [(y, uv)] * 3, layout='p010'),   # frames of two kinds
        dict(frames=[(y, uv)] * 7, layout='i420p10'),
        dict(frames=[(y, uv)] * 7),
        dict(frames=u8, out='p010', matrix='bt2020'),
        dict(frames=packed, layout='p010', cuts='yes'),
    ]
    if not edvr:
        bad.append(dict(frames=[(y, uv)] * 7, layout='p010'))                   # scale 1: a packed 13 x 15 output cannot be
        bad.append(dict(frames=u8[:, :17], out='i420p10'))
    for kw in bad:
        fr = kw.pop('frames')
        with pytest.raises(ValueError):
            _first(adapt.super_resolve_frames(opt, net, fr, **kw))
    if edvr:
        for fr, kw in ((packed, dict(layout='p010')), (packed.view(torch.int16), dict(layout='i420p12', out='float', matrix='bt709')),
                       ([(y, uv)] * 7, dict(layout='p012', out='hwc_rgb')), ([(y, uv)] * 7, dict(layout='p010')),
                       (u8, dict(out='p010')), (torch.zeros(7, 3, 18, 22), dict(out='i420p12')),
                       (torch.zeros(7, 27, 22, dtype=torch.uint8), dict(layout='nv12', out='p010'))):
            with pytest.raises(RuntimeError, match="MI355X"):
                _first(adapt.super_resolve_frames(opt, net, fr, **kw))


# ---- the C entry points, without a device
def _desc(lib, fmt=0, depth=10, h=6, w=8, matrix=0, rng=0, planes=(A16 + 2, A16 + 202, A16 + 402), rows=None):
    if rows is None:
        wc = (w + 1) // 2
        rows = (2 * w, 4 * wc, 0) if fmt == 0 else (2 * w, 2 * wc, 2 * wc)
    d = lib.Yuv16Desc(fmt, depth, h, w, matrix, rng)
    for i in range(3):
        d.plane[i] = planes[i]
        d.row_stride[i] = rows[i]
    return d


DESC_CASES = [
    (dict(fmt=2), b"format"), (dict(fmt=-1), b"format"),
    (dict(depth=8), b"depth"), (dict(depth=16), b"depth"), (dict(depth=11), b"depth"), (dict(depth=0), b"depth"),
    (dict(matrix=2), b"matrix"), (dict(matrix=-1), b"matrix"),
    (dict(rng=2), b"range"), (dict(rng=-1), b"range"),
    (dict(planes=(None, A16, A16)), b"null plane 0"),
    (dict(planes=(A16, None, A16)), b"null plane 1"),
    (dict(fmt=1, planes=(A16, A16, None)), b"null plane 2"),
    (dict(planes=(A16 + 1, A16, A16)), b"odd address of plane 0"),
    (dict(planes=(A16, A16 + 3, A16)), b"odd address of plane 1"),
    (dict(fmt=1, planes=(A16, A16, A16 + 5)), b"odd address of plane 2"),
    (dict(rows=(14, 16, 0)), b"row stride"),
    (dict(rows=(16, 14, 0)), b"row stride"),               # semi-planar: a chroma row is 4 * Wc bytes
    (dict(w=7, rows=(14, 14, 0)), b"row stride"),          # ... = 16 for an odd width of 7
    (dict(fmt=1, rows=(16, 6, 8)), b"row stride"),
    (dict(fmt=1, rows=(16, 8, 6)), b"row stride"),
    (dict(rows=(17, 16, 0)), b"odd row stride"),
    (dict(rows=(16, 19, 0)), b"odd row stride"),
    (dict(fmt=1, rows=(16, 8, 9)), b"odd row stride"),
    (dict(h=0), b"frame size"), (dict(w=0), b"frame size"),
]


def test_frame_ingest_yuv16_bad_arguments_without_gpu(lib):
    l = lib.lib()

    def ingest(dst=A16, Hp=8, Wp=8, pad=0, null_desc=False, **kw):
        d = _desc(lib, **kw)
        return l.dvsr_frame_ingest_yuv16(None if null_desc else ctypes.byref(d), dst, Hp, Wp, pad, None)

    cases = DESC_CASES + [
        (dict(null_desc=True), b"null"),
        (dict(dst=None), b"null"),
        (dict(h=9), b"frame size"), (dict(w=9, rows=(18, 20, 0)), b"frame size"),      # larger than the target
        (dict(pad=2), b"pad mode"), (dict(pad=-1), b"pad mode"),
        (dict(h=4), b"reflect"), (dict(w=4), b"reflect"),                              # pad 4 >= 4
        (dict(dst=A16 + 4), b"misaligned"),
        (dict(Wp=10), b"multiple of 4"),
    ]
    for kw, word in cases:
        assert ingest(**kw) == INVALID, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())
    for depth in (10, 12):                                          # semi-planar ignores plane[2]: passes every check ...
        d = _desc(lib, fmt=0, depth=depth, planes=(A16 + 2, A16 + 6, None))
        assert l.dvsr_frame_ingest_yuv16(ctypes.byref(d), None, 8, 8, 0, None) == INVALID and b"null planar" in l.dvsr_last_error()


def test_frame_emit_yuv16_bad_arguments_without_gpu(lib):
    l = lib.lib()

    def emit(src=A16, Hs=8, Ws=8, lo=0.0, hi=1.0, null_desc=False, **kw):
        d = _desc(lib, **kw)
        return l.dvsr_frame_emit_yuv16(src, Hs, Ws, None if null_desc else ctypes.byref(d), lo, hi, None)

    cases = DESC_CASES + [
        (dict(null_desc=True), b"null"),
        (dict(src=None), b"null"),
        (dict(h=9), b"frame size"), (dict(w=12, rows=(24, 24, 0)), b"frame size"),
        (dict(src=A16 + 8), b"misaligned"),
        (dict(Ws=6), b"multiple of 4"),
        (dict(lo=1.0, hi=1.0), b"range ["), (dict(lo=1.0, hi=0.0), b"range ["),
    ]
    for kw, word in cases:
        assert emit(**kw) == INVALID, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())


def test_extract_frame_yuv16_bad_arguments_without_gpu(lib):
    l = lib.lib()
    h = ctypes.c_void_p()
    cfg = lib.EdvrConfig(64, 5, 8, 5, 10, 4, 2)
    assert l.dvsr_edvr_stream_create(cfg, 20, 24, 6, ctypes.byref(h)) == 0
    n = l.dvsr_edvr_stream_num_params(h)
    arr = (ctypes.c_void_p * n)(*([A16] * n))
    cb, wb = l.dvsr_edvr_stream_cache_bytes(h), l.dvsr_edvr_stream_workspace_bytes(h)

    def extract(pad=0, slot=0, cache=A16, cache_bytes=cb, ws=A16, ws_bytes=wb, null_desc=False, params=arr, **kw):
        kw.setdefault('h', 18)
        kw.setdefault('w', 22)
        d = _desc(lib, **kw)
        return l.dvsr_edvr_stream_extract_frame_yuv16(h, params, None if null_desc else ctypes.byref(d), pad, slot, cache,
                                                      cache_bytes, ws, ws_bytes, 0, None)

    cases = [
        (dict(null_desc=True), b"null"),
        (dict(params=None), b"null"),
        (dict(cache=None), b"null"),
        (dict(ws=None), b"null"),
        (dict(slot=6), b"slot"), (dict(slot=-1), b"slot"),
        (dict(cache_bytes=cb - 4), b"cache"),
        (dict(ws_bytes=wb - 4), b"workspace"),
        (dict(cache=A16 + 4), b"aligned"),
        (dict(fmt=9), b"format"), (dict(depth=8), b"depth"), (dict(matrix=3), b"matrix"), (dict(rng=3), b"range"),
        (dict(planes=(A16, None, None)), b"null plane 1"),
        (dict(fmt=1, planes=(A16, A16, None)), b"null plane 2"),
        (dict(planes=(A16 + 1, A16, A16)), b"odd address"),
        (dict(pad=3), b"pad mode"),
        (dict(h=21), b"frame size"), (dict(w=25, rows=(50, 52, 0)), b"frame size"),     # larger than the plan's 20 x 24
        (dict(h=0), b"frame size"),
        (dict(h=10), b"reflect"),                                                       # 10 rows of padding out of 10
        (dict(rows=(42, 44, 0)), b"row stride"), (dict(rows=(44, 42, 0)), b"row stride"),
        (dict(fmt=1, rows=(44, 22, 20)), b"row stride"),
        (dict(rows=(45, 44, 0)), b"odd row stride"),
    ]
    for kw, word in cases:
        assert extract(**kw) == INVALID, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())
    l.dvsr_edvr_stream_destroy(h)


def test_luma_sad_16_bit_formats_bad_arguments_without_gpu(lib):
    l = lib.lib()
    assert (lib.FRAME_U16_Y_MSB, lib.FRAME_U16_Y_10, lib.FRAME_U16_Y_12) == (4, 5, 6)

    def sad(fmt, h=8, w=8, row=16, ps=2, a=A16 + 2, b=A16 + 1026, fs=128, pairs=1, res=A16):
        d = lib.FrameDesc(fmt, h, w, row, 0, ps)
        return l.dvsr_frame_luma_sad(a, b, ctypes.byref(d), fs, pairs, res, None)

    for fmt in (4, 5, 6):
        cases = [
            (dict(ps=1), b"pixel stride"), (dict(ps=3), b"pixel stride"),
            (dict(a=A16 + 1), b"odd address"), (dict(b=A16 + 7), b"odd address"),
            (dict(row=14), b"row stride"),                                  # 8 words are 16 bytes
            (dict(row=17), b"odd row stride"),
            (dict(fs=129), b"frame stride"),
            (dict(a=None), b"null"), (dict(res=None), b"null"),
            (dict(h=0), b"frame size"), (dict(pairs=0), b"pairs"),
            (dict(res=A16 + 4), b"misaligned"),
        ]
        for kw, word in cases:
            assert sad(fmt, **kw) == INVALID, (fmt, kw)
            assert word in l.dvsr_last_error(), (fmt, kw, l.dvsr_last_error())
        # ingest and emit keep rejecting the single-plane formats
        d = lib.FrameDesc(fmt, 8, 8, 16, 0, 2)
        assert l.dvsr_frame_ingest(A16, ctypes.byref(d), A16, 8, 8, 0, None) == INVALID and b"format" in l.dvsr_last_error()
        assert l.dvsr_frame_emit(A16, 8, 8, A16, ctypes.byref(d), 0.0, 1.0, None) == INVALID and b"format" in l.dvsr_last_error()
    assert sad(7) == INVALID and b"format" in l.dvsr_last_error()
