"""CPU: the host side of the YCbCr 4:2:2 / 4:4:4 frame path -- the layout rules of dynavsr_amd/frames.py for the
nine new names, the descriptors they become, the argument checks of the C entry points for the new values of `format` (they
return DVSR_ERR_INVALID before any launch, so they run without a GPU, with pointers that are never dereferenced), the argument
checks of adapt.super_resolve_frames, and the fp64 restatement tests/yuv_chroma_ref.py tied to the 4:2:0 one."""
import ctypes
import os

import numpy as np
import pytest
import torch

import yuv16_ref
import yuv_chroma_ref as ref
import yuv_ref
from dynavsr_amd import adapt, frames

INVALID = -1
A16 = 0x10000           # a 16-byte aligned address that nothing reads
L422 = ['i422', 'nv16', 'i422p10', 'i422p12', 'p210', 'p212']
L444 = ['i444', 'i444p10', 'i444p12']
LAYOUTS = L422 + L444
# layout -> the value of `format` in its descriptor: form | chroma << 4
FORMAT = {'i422': 0x11, 'nv16': 0x10, 'i422p10': 0x11, 'i422p12': 0x11, 'p210': 0x10, 'p212': 0x10,
          'i444': 0x21, 'i444p10': 0x21, 'i444p12': 0x21}


@pytest.fixture(scope="module")
def lib():
    from dynavsr_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        from dynavsr_amd import build
        build.build()
    return _lib


def info(layout):
    chroma, semi, depth, _ = ref.LAYOUTS[layout]
    return chroma, semi, depth, (torch.uint8 if depth == 8 else torch.uint16)


def test_the_new_names_are_yuv_layouts_of_their_own_tuples():
    assert frames.YUV_LAYOUTS == ('nv12', 'i420') and frames.YUV16_LAYOUTS == ('p010', 'p012', 'i420p10', 'i420p12')
    assert sorted(frames.YUV422_LAYOUTS) == sorted(L422) and sorted(frames.YUV444_LAYOUTS) == sorted(L444)
    for layout in LAYOUTS:
        assert frames.is_yuv(layout) and frames.layout_depth(layout) == ref.LAYOUTS[layout][2]
    for name in ('nv24', 'p410', 'yuyv', 'uyvy', 'v210', 'yuv422p', 'yuv444p', 'i440', 'i411', 'gbrp', 'i444p16'):
        assert not frames.is_yuv(name)
        with pytest.raises(ValueError, match="layout"):
            frames.yuv_planes(torch.zeros(12, 8, dtype=torch.uint8), name)
    with pytest.raises(ValueError, match="i444p12"):                              # the "one of ..." texts name them
        frames.resolve_layout(torch.zeros(6, 8, 3, dtype=torch.uint8), 'nv24')
    with pytest.raises(ValueError, match="p212"):
        frames.emit(torch.zeros(3, 8, 8), 8, 8, 'yuv422p')


# ---- packed frames and plane tuples
@pytest.mark.parametrize("layout", LAYOUTS)
def test_packed_frames_resolve_to_plane_views(layout):
    chroma, semi, depth, dt = info(layout)
    es = 1 if depth == 8 else 2
    for h, w in ((6, 8), (7, 8)) + (((7, 9),) if chroma == '444' else ()):       # any H; any W for 4:4:4
        rows = 2 * h if chroma == '422' else 3 * h
        packed = torch.zeros(rows, w, dtype=dt)
        assert frames.resolve_layout(packed, layout) == (layout, h, w)
        planes, hh, ww = frames.yuv_planes(packed, layout)
        assert (hh, ww) == (h, w) and len(planes) == (2 if semi else 3)
        assert planes[0].shape == (h, w) and planes[0].data_ptr() == packed.data_ptr() and planes[0].stride() == (w, 1)
        base = packed.data_ptr() + h * w * es
        assert planes[1].data_ptr() == base
        if chroma == '444':
            assert [tuple(p.shape) for p in planes[1:]] == [(h, w)] * 2 and planes[2].data_ptr() == base + h * w * es
            assert all(p.stride() == (w, 1) for p in planes[1:])
        elif semi:
            assert tuple(planes[1].shape) == (h, w // 2, 2) and planes[1].stride() == (w, 2, 1)
        else:
            assert [tuple(p.shape) for p in planes[1:]] == [(h, w // 2)] * 2 and planes[2].data_ptr() == base + h * (w // 2) * es
            assert all(p.stride() == (w // 2, 1) for p in planes[1:])
        if depth > 8:                                                             # int16: the same bits
            assert frames.resolve_layout(packed.view(torch.int16), layout) == (layout, h, w)
        with pytest.raises(ValueError):
            frames.resolve_layout(packed)                                         # never inferred
        with pytest.raises(ValueError):
            frames.ingest(packed)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_plane_tuples_take_odd_sizes(layout):
    chroma, semi, depth, dt = info(layout)
    h, w = 7, 9
    hc, wc = (h, 5) if chroma == '422' else (h, w)
    y = torch.zeros(h, w, dtype=dt)
    c = torch.zeros((hc, wc, 2) if semi else (hc, wc), dtype=dt)
    good = (y, c) if semi else (y, c, c.clone())
    assert frames.resolve_layout(good, layout) == (layout, h, w)
    assert frames.resolve_layout(list(good), layout) == (layout, h, w)
    planes, hh, ww = frames.yuv_planes(good, layout)
    assert (hh, ww) == (h, w) and all(a.data_ptr() == b.data_ptr() for a, b in zip(planes, good))
    c420 = torch.zeros((4, 5, 2) if semi else (4, 5), dtype=dt)                   # the chroma plane of a 4:2:0 frame of 7 x 9
    other = torch.uint16 if depth == 8 else torch.uint8
    for bad in ((y, c420) if semi else (y, c420, c420),
                (y, c[:, :-1]) if semi else (y, c, c[:, :-1]),
                (y, c[:-1]) if semi else (y, c[:-1], c),
                (y,), (y, c, c, c), (y, c, c) if semi else (y, c),
                tuple(p.to(other) for p in good), tuple(p.float() for p in good), (y[0],) + good[1:]):
        with pytest.raises(ValueError):
            frames.resolve_layout(bad, layout)
        with pytest.raises(ValueError):
            frames.ingest(bad, layout)                                            # ... said before any GPU call


@pytest.mark.parametrize("layout", LAYOUTS)
def test_bad_packed_shapes_and_dtypes(layout):
    chroma, semi, depth, dt = info(layout)
    other = torch.uint16 if depth == 8 else torch.uint8
    n = 2 if chroma == '422' else 3
    bad = [torch.zeros(n * 6 + 1, 8, dtype=dt),                                    # rows not 2H / 3H
           torch.zeros(n * 6, 8, dtype=other),                                     # uint8 for a 16-bit layout and the reverse
           torch.zeros(n * 6, 8), torch.zeros(n * 6, 8, 1, dtype=dt), torch.zeros(n, 8, dtype=dt)[:0], None, layout]
    if chroma == '422':
        bad += [torch.zeros(12, 7, dtype=dt), torch.zeros(13, 8, dtype=dt)]       # odd W; an odd number of rows
    for b in bad:
        with pytest.raises(ValueError):
            frames.resolve_layout(b, layout)
        with pytest.raises(ValueError):
            frames.ingest(b, layout)
    if chroma == '422':
        with pytest.raises(ValueError, match="odd width"):
            frames.yuv_planes(torch.zeros(12, 7, dtype=dt), layout)


def test_pitched_packed_frames():
    wide = torch.zeros(12, 12, dtype=torch.uint8)[:, 2:10]                        # 6 x 8 nv16, rows 12 bytes apart
    planes, h, w = frames.yuv_planes(wide, 'nv16')
    assert (h, w) == (6, 8) and planes[0].stride() == (12, 1)
    assert planes[1].stride() == (12, 2, 1) and planes[1].data_ptr() == wide.data_ptr() + 6 * 12
    kept, d = frames.describe_yuv(planes, 'nv16', 6, 8)
    assert [p.data_ptr() for p in kept] == [p.data_ptr() for p in planes]          # passed by stride: nothing copied
    assert (d.plane[0], d.plane[1]) == (wide.data_ptr(), wide.data_ptr() + 72) and tuple(d.row_stride)[:2] == (12, 12)
    wide = torch.zeros(12, 11, dtype=torch.uint8)[:, 1:8]                         # 4 x 7 i444: odd width, odd pitch
    planes, h, w = frames.yuv_planes(wide, 'i444')
    assert (h, w) == (4, 7) and [p.data_ptr() - wide.data_ptr() for p in planes] == [0, 44, 88]
    kept, d = frames.describe_yuv(planes, 'i444', 4, 7)
    assert [p.data_ptr() for p in kept] == [p.data_ptr() for p in planes] and tuple(d.row_stride) == (11, 11, 11)
    wide16 = torch.zeros(12, 12, dtype=torch.uint16)[:, 2:10]                     # p210: strides in bytes
    planes, _, _ = frames.yuv_planes(wide16, 'p210')
    _, d = frames.describe_yuv(planes, 'p210', 6, 8)
    assert tuple(d.row_stride)[:2] == (24, 24) and d.plane[1] == wide16.data_ptr() + 6 * 24
    for layout, t in (('i422', torch.zeros(12, 12, dtype=torch.uint8)), ('i422p10', torch.zeros(12, 12, dtype=torch.uint16))):
        with pytest.raises(ValueError, match="contiguous"):
            frames.yuv_planes(t[:, 2:10], layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_describe_yuv_carries_the_chroma_field(layout):
    chroma, semi, depth, dt = info(layout)
    es = 1 if depth == 8 else 2
    h, w = 7, 9
    wc = 5 if chroma == '422' else 9
    buf = torch.zeros(4096, dtype=dt)
    y = buf.as_strided((h, w), (13, 1), 1)
    if semi:
        planes = (y, buf.as_strided((h, wc, 2), (15, 2, 1), 201))
        rows = (13, 15)
    else:
        planes = (y, buf.as_strided((h, wc), (11, 1), 301), buf.as_strided((h, wc), (wc, 1), 503))
        rows = (13, 11, wc)
    kept, d = frames.describe_yuv(planes, layout, h, w, 'bt709', 'full')
    assert [p.data_ptr() for p in kept] == [p.data_ptr() for p in planes]
    assert (d.format, d.h, d.w, d.matrix, d.range) == (FORMAT[layout], h, w, 1, 1)
    assert (d.format & 15, d.format >> 4) == (0 if semi else 1, 1 if chroma == '422' else 2)
    if depth > 8:
        assert d.depth == depth
    assert [d.plane[i] for i in range(len(planes))] == [p.data_ptr() for p in planes]
    assert tuple(d.row_stride)[:len(planes)] == tuple(r * es for r in rows)
    skip = buf.as_strided((h, wc, 2) if semi else (h, wc), (40, 4, 1) if semi else (40, 2), 0)   # no descriptor expresses it
    with pytest.raises(ValueError, match="plane 1"):
        frames.describe_yuv((y, skip) + planes[2:], layout, h, w, copy=False)
    with pytest.raises(ValueError):
        frames.describe_yuv(planes, layout, h, w, matrix='bt2020')


def test_emit_and_score_argument_checks_come_before_the_gpu():
    sr = torch.zeros(3, 8, 8)
    for layout in L422:
        dt = info(layout)[3]
        with pytest.raises(ValueError, match="even width"):
            frames.emit(sr, 8, 7, layout)
        with pytest.raises(ValueError, match="even width"):
            frames.emit(sr, 8, 8, layout, size=(6, 7))
        with pytest.raises(ValueError, match="out is a"):
            frames.emit(sr, 8, 8, layout, out=torch.zeros(12, 8, dtype=dt))
        with pytest.raises(RuntimeError, match="GPU"):                             # an odd height packs: as far as the device
            frames.emit(sr, 7, 8, layout)
    for layout in L444:
        dt = info(layout)[3]
        with pytest.raises(ValueError, match="out is a"):
            frames.emit(sr, 8, 8, layout, out=torch.zeros(21, 8, dtype=dt))
        with pytest.raises(RuntimeError, match="GPU"):                             # any size packs
            frames.emit(sr, 7, 7, layout)
    with pytest.raises(ValueError, match="crop"):
        frames.emit(sr, 9, 8, 'nv16')
    with pytest.raises(ValueError, match="matrix"):
        frames.emit(sr, 8, 8, 'i444', matrix='bt2020')
    # score: the Y plane, channel 'y' alone, one depth on both sides
    nv16, i444p10 = (torch.zeros(24, 16, dtype=torch.uint8), 'nv16', 12, 16), (torch.zeros(36, 16, dtype=torch.uint16), 'i444p10', 12, 16)
    for t, layout, h, w in (nv16, i444p10):
        assert frames.resolve_layout(t, layout) == (layout, h, w)
        with pytest.raises(ValueError, match="channel='y'"):
            frames.check_score((layout, h, w), ('hwc_rgb', h, w), 'rgb')
    assert frames.check_score(('nv16', 12, 16), ('hwc_rgb', 12, 16), 'y')[2] == 8
    assert frames.check_score(('i444p10', 12, 16), ('p010', 12, 16), 'y')[2] == 10
    with pytest.raises(ValueError, match="mixed bit depths"):
        frames.check_score(('i444p10', 12, 16), ('nv16', 12, 16), 'y')
    with pytest.raises(ValueError, match="mixed bit depths"):
        frames.score(i444p10[0], nv16[0], 'i444p10', 'nv16', channel='y')


# ---- the C entry points, without a device
def _desc(lib, layout, fmt=None, h=6, w=8, short=None, null=None):
    """The descriptor of `layout` at h x w with rows exactly as long as they must be; `short`: plane whose row stride is one
    sample less; `null`: plane without an address.  Returns (descriptor, the bytes a row of each plane needs)."""
    chroma, semi, depth, _ = ref.LAYOUTS[layout]
    es = 1 if depth == 8 else 2
    wc = (w + 1) // 2 if chroma == '422' else w
    need = [w * es, (2 * wc if semi else wc) * es, 0 if semi else wc * es]
    fmt = FORMAT[layout] if fmt is None else fmt
    d = lib.YuvDesc(fmt, h, w, 0, 0) if depth == 8 else lib.Yuv16Desc(fmt, depth, h, w, 0, 0)
    for i in range(3):
        d.plane[i] = None if i == null else A16 + 2 + 512 * i
        d.row_stride[i] = need[i] - (es if i == short else 0)
    return d, need


@pytest.mark.parametrize("layout", LAYOUTS)
def test_c_entry_points_take_the_new_formats_up_to_the_row_checks(lib, layout):
    l = lib.lib()
    chroma, semi, depth, _ = ref.LAYOUTS[layout]
    suffix = 'yuv' if depth == 8 else 'yuv16'
    ingest, emit = getattr(l, "dvsr_frame_ingest_" + suffix), getattr(l, "dvsr_frame_emit_" + suffix)
    for h, w in ((6, 8), (6, 7)):
        n = 2 if semi else 3
        for short in range(n):                                                     # one sample short: refused, with the length
            d, need = _desc(lib, layout, h=h, w=w, short=short)
            for rc in (ingest(ctypes.byref(d), A16, 8, 8, 0, None), emit(A16, 8, 8, ctypes.byref(d), 0.0, 1.0, None)):
                assert rc == INVALID
                msg = l.dvsr_last_error()
                assert b"row stride" in msg and b"of plane %d " % short in msg and b"row of %d bytes" % need[short] in msg, msg
        for null in range(n):
            d, _ = _desc(lib, layout, h=h, w=w, null=null)
            assert ingest(ctypes.byref(d), A16, 8, 8, 0, None) == INVALID and b"null plane %d" % null in l.dvsr_last_error()
        # rows exactly as long as needed pass the frame's checks: the next check of each function is the one that answers
        d, _ = _desc(lib, layout, h=h, w=w)
        assert ingest(ctypes.byref(d), A16, 8, 8, 2, None) == INVALID and b"pad mode" in l.dvsr_last_error()
        assert emit(A16, 8, 8, ctypes.byref(d), 1.0, 1.0, None) == INVALID and b"range [" in l.dvsr_last_error()
    d, _ = _desc(lib, layout, h=9)
    assert ingest(ctypes.byref(d), A16, 8, 8, 0, None) == INVALID and b"frame size" in l.dvsr_last_error()
    if depth > 8:
        d, _ = _desc(lib, layout)
        d.depth = 16
        assert ingest(ctypes.byref(d), A16, 8, 8, 0, None) == INVALID and b"depth" in l.dvsr_last_error()
        d, _ = _desc(lib, layout)
        d.plane[1] = A16 + 513
        assert ingest(ctypes.byref(d), A16, 8, 8, 0, None) == INVALID and b"odd address of plane 1" in l.dvsr_last_error()


@pytest.mark.parametrize("layout", ['nv16', 'p210'])
def test_c_entry_points_refuse_the_formats_that_are_not_provided(lib, layout):
    l = lib.lib()
    depth = ref.LAYOUTS[layout][2]
    suffix = 'yuv' if depth == 8 else 'yuv16'
    ingest, emit = getattr(l, "dvsr_frame_ingest_" + suffix), getattr(l, "dvsr_frame_emit_" + suffix)
    # semi-planar 4:4:4 | a third form | a fourth sub-sampling | the forms that were always refused | a negative value
    for fmt in (0x20, 0x12, 0x22, 0x30, 0x31, 2, 9, -1, -16, 0x110):
        d, _ = _desc(lib, layout, fmt=fmt)
        assert ingest(ctypes.byref(d), A16, 8, 8, 0, None) == INVALID, fmt
        assert b"format" in l.dvsr_last_error(), (fmt, l.dvsr_last_error())
        assert emit(A16, 8, 8, ctypes.byref(d), 0.0, 1.0, None) == INVALID, fmt
        assert b"format" in l.dvsr_last_error(), (fmt, l.dvsr_last_error())
    d, _ = _desc(lib, layout, fmt=0x20)
    ingest(ctypes.byref(d), A16, 8, 8, 0, None)
    assert b"4:4:4" in l.dvsr_last_error()


@pytest.mark.parametrize("layout", ['i422', 'i444p10'])
def test_extract_frame_takes_the_new_formats_up_to_the_row_checks(lib, layout):
    l = lib.lib()
    depth = ref.LAYOUTS[layout][2]
    fn = getattr(l, "dvsr_edvr_stream_extract_frame_" + ('yuv' if depth == 8 else 'yuv16'))
    h = ctypes.c_void_p()
    cfg = lib.EdvrConfig(64, 5, 8, 5, 10, 4, 2)
    assert l.dvsr_edvr_stream_create(cfg, 20, 24, 6, ctypes.byref(h)) == 0
    n = l.dvsr_edvr_stream_num_params(h)
    arr = (ctypes.c_void_p * n)(*([A16] * n))
    cb, wb = l.dvsr_edvr_stream_cache_bytes(h), l.dvsr_edvr_stream_workspace_bytes(h)

    def extract(d, pad=0):
        return fn(h, arr, ctypes.byref(d), pad, 0, A16, cb, A16, wb, 0, None)

    for short in range(3):
        d, need = _desc(lib, layout, h=18, w=22, short=short)
        assert extract(d) == INVALID
        assert b"row stride" in l.dvsr_last_error() and b"row of %d bytes" % need[short] in l.dvsr_last_error()
    d, _ = _desc(lib, layout, h=18, w=22)
    assert extract(d, pad=3) == INVALID and b"pad mode" in l.dvsr_last_error()
    d, _ = _desc(lib, layout, h=18, w=22, fmt=0x20)
    assert extract(d) == INVALID and b"format" in l.dvsr_last_error()
    d, _ = _desc(lib, layout, h=21, w=22)
    assert extract(d) == INVALID and b"frame size" in l.dvsr_last_error()
    l.dvsr_edvr_stream_destroy(h)


# ---- super_resolve_frames
class _Mean(torch.nn.Module):
    nframes = 3

    def forward(self, x):
        return x.mean(1)


def _first(gen):
    return next(iter(gen))


@pytest.mark.parametrize("edvr", [False, True])
def test_super_resolve_frames_checks_chroma_arguments_first(edvr):
    if edvr:
        from dynavsr_amd.models.archs.EDVR_arch import EDVR
        net = EDVR()                                    # on the CPU: a valid call gets as far as the device check
        opt = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
    else:
        net = _Mean()
        opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    nv16 = torch.zeros(7, 36, 22, dtype=torch.uint8)                            # 18 x 22
    i444 = torch.zeros(7, 54, 22, dtype=torch.uint8)
    p210 = torch.zeros(7, 36, 22, dtype=torch.uint16)
    y, u, uv = torch.zeros(13, 15, dtype=torch.uint16), torch.zeros(13, 15, dtype=torch.uint16), torch.zeros(13, 8, 2, dtype=torch.uint8)
    y8 = torch.zeros(13, 15, dtype=torch.uint8)
    u8 = torch.zeros(7, 18, 22, 3, dtype=torch.uint8)
    bad = [
        dict(frames=nv16),                                                      # never inferred
        dict(frames=nv16, layout='yuv422p'),
        dict(frames=nv16, layout='nv24'),
        dict(frames=nv16, layout='p210'),                                       # bytes under a 16-bit name
        dict(frames=p210, layout='nv16'),
        dict(frames=u8, layout='i444'),
        dict(frames=nv16, layout='nv16', matrix='bt2020'),
        dict(frames=i444, layout='i444', yuv_range='tv'),
        dict(frames=nv16, layout='nv16', out='nv24'),
        dict(frames=nv16, layout='nv16', out='yuv444p'),
        dict(frames=nv16, layout='i422', pad_mode='circular'),
        dict(frames=nv16[:, :35], layout='nv16'),                               # 35 rows are not 2H
        dict(frames=i444[:, :53], layout='i444'),                               # 53 rows are not 3H
        dict(frames=nv16[:, :, :21], layout='i422'),                            # odd W packed
        dict(frames=nv16[:, :, :20], layout='i422'),                            # packed I422 must be contiguous
        dict(frames=torch.zeros(7, 6, 22, dtype=torch.uint8), layout='nv16'),   # H < 4
        dict(frames=[(y8, uv)] * 3 + [(y8, uv[:12])] + [(y8, uv)] * 3, layout='nv16'),
        dict(frames=[(y8, uv)] * 3 + [nv16[0]] + [(y8, uv)] * 3, layout='nv16'),      # frames of two kinds
        dict(frames=[(y8, uv)] * 7, layout='i422'),
        dict(frames=[(y8, uv[:7])] * 7, layout='nv16'),                         # a 4:2:0-shaped chroma plane
        dict(frames=[(y, u, u)] * 7),                                           # planes are not inferred either
        dict(frames=[(y, u, u)] * 7, layout='i444'),                            # words under an 8-bit name
        dict(frames=u8, out='p210', matrix='bt2020'),
        dict(frames=u8, out='i422', out_size=(54, 65)),                         # a packed 4:2:2 output needs an even width
        dict(frames=nv16, layout='nv16', gt=u8, scores=torch.zeros(7, 2, dtype=torch.float64)),   # channel 'rgb' on a Y plane
    ]
    if not edvr:
        bad.append(dict(frames=[(y8, uv)] * 7, layout='nv16'))                  # scale 1: a packed 13 x 15 nv16 output cannot be
        bad.append(dict(frames=u8[:, :, :21], out='i422'))
    for kw in bad:
        fr = kw.pop('frames')
        with pytest.raises(ValueError):
            _first(adapt.super_resolve_frames(opt, net, fr, **kw))
    if edvr:
        good = [(nv16, dict(layout='nv16')), (nv16, dict(layout='i422', out='float', matrix='bt709', yuv_range='full')),
                (i444, dict(layout='i444')), (p210, dict(layout='p210')), (p210, dict(layout='i422p12', out='i444p10')),
                ([(y, u, u)] * 7, dict(layout='i444p10')),                      # 52 x 60 as packed 4:4:4: any size
                ([(y8, uv)] * 7, dict(layout='nv16')),                          # 52 x 60: an even width
                (u8, dict(out='p210')), (u8, dict(out='i422', out_size=(53, 66))),   # an odd height packs
                (u8, dict(out='i444', out_size=(53, 65))),
                (torch.zeros(7, 3, 18, 22), dict(out='i444p12'))]
        for fr, kw in good:
            with pytest.raises(RuntimeError, match="MI355X"):
                _first(adapt.super_resolve_frames(opt, net, fr, **kw))


# ---- the restatement, tied to the 4:2:0 one
def test_resampling_of_the_restatement():
    c = np.array([[10., 30.], [50., 70.], [20., 40.]])
    up = ref.upsample422(c, 3, 4)
    assert np.array_equal(up, [[10, 20, 30, 30], [50, 60, 70, 70], [20, 30, 40, 40]])       # x = 3 clamps to column 1; rows as they are
    assert np.array_equal(ref.upsample422(c, 3, 3), up[:, :3])                  # an odd width: the last column serves one pixel
    ramp = np.stack([np.arange(8.), 10 * np.arange(8.)])
    assert np.array_equal(ref.downsample422(ramp), [[0.25, 2, 4, 6], [2.5, 20, 40, 60]])     # the left tap of column 0 is clamped
    assert np.array_equal(ref.downsample422(ramp[:, :7]), [[0.25, 2, 4, 5.75], [2.5, 20, 40, 57.5]])   # ... and the right one
    flat = np.full((5, 7), 3.25)
    assert np.array_equal(ref.downsample422(flat), np.full((5, 4), 3.25))
    assert np.array_equal(ref.upsample422(np.full((5, 4), 3.25), 5, 7), flat)
    r = np.random.RandomState(0).uniform(0, 255, (5, 7))
    for layout in L444:                                                        # 4:4:4: the identity both ways
        assert ref.upsample(r, 5, 7, layout) is not None and np.array_equal(ref.upsample(r, 5, 7, layout), r)
        assert np.array_equal(ref.downsample(r, layout), r)
    for layout in L422:
        assert np.array_equal(ref.upsample(r[:, :4], 5, 7, layout), ref.upsample422(r[:, :4], 5, 7))
        assert np.array_equal(ref.downsample(r, layout), ref.downsample422(r))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pack_and_unpack_are_inverse_and_match_yuv_planes(layout):
    chroma, semi, depth, dt = info(layout)
    h, w = 5, 8
    hc, wc = ref.chroma_size(layout, h, w)
    r = np.random.RandomState(3)
    levels = [r.randint(0, 2 ** depth, s) for s in ((h, w), (hc, wc), (hc, wc))]
    samples = [ref.samples_of(p, layout) for p in levels]
    packed = ref.pack(*samples, layout)
    assert packed.shape == ((2 if chroma == '422' else 3) * h, w) and packed.dtype == (np.uint8 if depth == 8 else np.uint16)
    assert all(np.array_equal(a, b) for a, b in zip(ref.unpack(packed, layout), samples))
    planes = frames.yuv_planes(torch.from_numpy(packed), layout)[0]             # the library reads the same planes out of it
    got = [planes[0].numpy()] + ([planes[1][:, :, 0].numpy(), planes[1][:, :, 1].numpy()] if semi else [p.numpy() for p in planes[1:]])
    assert all(np.array_equal(a, b) for a, b in zip(got, samples))
    assert all(np.array_equal(ref.levels_of(s, layout)[0], p) for s, p in zip(samples, levels))


@pytest.mark.parametrize("layout,like", [('nv16', None), ('i422', None), ('p210', 'p010'), ('i422p12', 'i420p12')])
@pytest.mark.parametrize("matrix,yuv_range", [('bt601', 'limited'), ('bt709', 'full')])
def test_ingest_of_equal_chroma_rows_is_the_420_restatement(layout, like, matrix, yuv_range):
    """A 4:2:2 frame whose chroma rows are all equal against the 4:2:0 frame with those rows: the vertical 0.75 / 0.25 filter of
    equal rows is the row itself."""
    depth = ref.LAYOUTS[layout][2]
    h, w, Hp, Wp = 7, 9, 8, 12
    r = np.random.RandomState(depth)
    y = r.randint(0, 2 ** depth, (h, w))
    row_b, row_r = r.randint(0, 2 ** depth, (1, 5)), r.randint(0, 2 ** depth, (1, 5))
    for mode in ('reflect', 'replicate'):
        got = ref.ingest(y, np.repeat(row_b, h, 0), np.repeat(row_r, h, 0), Hp, Wp, layout, mode, matrix, yuv_range)
        if depth == 8:
            want = yuv_ref.ingest(y, np.repeat(row_b, 4, 0), np.repeat(row_r, 4, 0), Hp, Wp, mode, matrix, yuv_range)
        else:
            want = yuv16_ref.ingest(y, np.repeat(row_b, 4, 0), np.repeat(row_r, 4, 0), Hp, Wp, depth, mode, matrix, yuv_range)
        assert got.shape == (3, Hp, Wp) and float(np.abs(got - want).max()) <= 1e-12


@pytest.mark.parametrize("layout", LAYOUTS)
def test_emit_of_the_restatement_inverts_its_ingest_on_flat_chroma(layout):
    """Constant chroma survives both resamplings untouched, so emit(ingest(frame)) returns the frame's levels (in gamut)."""
    depth = ref.LAYOUTS[layout][2]
    h, w = 6, 9
    s = 2 ** (depth - 8)
    y = np.random.RandomState(1).randint(64 * s, 192 * s, (h, w))
    hc, wc = ref.chroma_size(layout, h, w)
    cb, cr = np.full((hc, wc), 120 * s), np.full((hc, wc), 135 * s)
    rgb = ref.ingest(y, cb, cr, h, w, layout)
    back = ref.emit(rgb, h, w, layout)
    assert [b.shape for b in back] == [(h, w), (hc, wc), (hc, wc)]
    for b, want in zip(back, (y, cb, cr)):
        assert float(np.abs(b - want).max()) < 1e-9
        assert np.array_equal(ref.round_levels(b, layout), want) and float(ref.tie_distance(b, layout).min()) > 0.49
