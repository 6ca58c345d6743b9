"""CPU: the host side of the YCbCr 4:2:0 frame path -- the fp64 restatement of its arithmetic (tests/yuv_ref.py) against what
the reference's own colour functions return (tests/golden/ycbcr_reference.npz, recorded by tools/gen_ycbcr_golden.py), the
layout rules of dynavsr_amd/frames.py, and the argument checks of the three C entry points, which return DVSR_ERR_INVALID before
any launch -- so they run without a GPU, with pointers that are never dereferenced."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import yuv_ref
from dynavsr_amd import adapt, frames

INVALID = -1
A16 = 0x10000           # a 16-byte aligned address that nothing reads
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ycbcr_reference.npz")
PAIRS = list(itertools.product(('bt601', 'bt709'), ('limited', 'full')))


@pytest.fixture(scope="module")
def lib():
    from dynavsr_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        from dynavsr_amd import build
        build.build()
    return _lib


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


# ---- the restatement (bt601, limited, chroma not resampled) against the reference's functions
def test_restatement_is_the_reference_ycbcr2rgb(golden):
    x, want = golden["ycbcr2rgb_f64_in"], golden["ycbcr2rgb_f64_out"]
    raw = yuv_ref.ycbcr_to_rgb(*(255.0 * x[:, :, c] for c in range(3)), clamp=False)
    ok = ((raw >= 0) & (raw <= 1)).all(0) & ((want >= 0) & (want <= 1)).all(-1)              # in-gamut pixels
    assert ok.mean() > 0.9
    got = np.moveaxis(yuv_ref.ycbcr_to_rgb(*(255.0 * x[:, :, c] for c in range(3))), 0, -1)
    err = float(np.abs(got - want)[ok].max())
    print("ycbcr2rgb float: max-abs %.2e on %d pixels" % (err, int(ok.sum())))
    assert err <= 1e-5                         # the reference's constants are truncated to 6 digits
    x, want = golden["ycbcr2rgb_u8_in"], golden["ycbcr2rgb_u8_out"]
    got = np.moveaxis(yuv_ref.ycbcr_to_rgb(*(x[:, :, c] for c in range(3))), 0, -1)
    differ = int((yuv_ref.to_bytes(255.0 * got) != want).sum())
    print("ycbcr2rgb uint8: %d of %d bytes differ" % (differ, want.size))
    assert differ == 0


@pytest.mark.parametrize("name", ["rgb2ycbcr", "bgr2ycbcr"])
def test_restatement_is_the_reference_rgb2ycbcr(golden, name):
    order = (0, 1, 2) if name == "rgb2ycbcr" else (2, 1, 0)
    x, want = golden[name + "_f64_in"], golden[name + "_f64_out"]
    got = np.stack(yuv_ref.rgb_to_ycbcr([x[:, :, c] for c in order]), -1)
    err = float(np.abs(got - 255.0 * want).max())
    print("%s float: max-abs %.2e levels" % (name, err))
    assert err <= 1e-3
    x, want = golden[name + "_u8_in"], golden[name + "_u8_out"]
    got = np.stack(yuv_ref.rgb_to_ycbcr([x[:, :, c] / 255.0 for c in order]), -1)
    differ = int((yuv_ref.to_bytes(got) != want).sum())
    print("%s uint8: %d of %d bytes differ" % (name, differ, want.size))
    assert differ == 0
    assert float(yuv_ref.tie_distance(got).min()) > 5e-4       # the fixture keeps its bytes away from ties (recorder: 1e-3)


# ---- anchors, from the constants
@pytest.mark.parametrize("matrix,yuv_range", PAIRS)
def test_anchor_cases(matrix, yuv_range):
    y0, ys, cs = yuv_ref.RANGES[yuv_range]
    kr, kb = yuv_ref.MATRICES[matrix]
    black, white = (16, 235) if yuv_range == 'limited' else (0, 255)
    assert (y0, y0 + ys) == (black, white)
    assert np.allclose(yuv_ref.ycbcr_to_rgb(white, 128, 128, matrix, yuv_range), 1.0, atol=1e-15)
    assert np.allclose(yuv_ref.ycbcr_to_rgb(black, 128, 128, matrix, yuv_range), 0.0, atol=1e-15)
    assert np.allclose(yuv_ref.ycbcr_to_rgb((black + white) / 2, 128, 128, matrix, yuv_range), 0.5, atol=1e-15)
    # the primaries: red has Cr at the top of the chroma range, blue has Cb there; luma is the matrix's weight
    for rgb, (wy, cb_top, cr_top) in (((1, 0, 0), (kr, False, True)), ((0, 0, 1), (kb, True, False)),
                                      ((0, 1, 0), (1 - kr - kb, False, False))):
        y, cb, cr = yuv_ref.rgb_to_ycbcr(np.array(rgb, np.float64), matrix, yuv_range)
        assert abs(y - (y0 + ys * wy)) < 1e-12
        assert (abs(cb - (128 + cs / 2)) < 1e-12) == cb_top and (abs(cr - (128 + cs / 2)) < 1e-12) == cr_top
        back = yuv_ref.ycbcr_to_rgb(y, cb, cr, matrix, yuv_range, clamp=False)           # ... and survive the round trip
        assert np.abs(back - np.array(rgb)).max() < 1e-12
    r = np.random.RandomState(1).uniform(0, 1, (3, 50))
    assert np.abs(yuv_ref.ycbcr_to_rgb(*yuv_ref.rgb_to_ycbcr(r, matrix, yuv_range), matrix, yuv_range, clamp=False) - r).max() < 1e-12
    # out of gamut: clamped, not wrapped
    assert yuv_ref.ycbcr_to_rgb(255, 255, 255, matrix, yuv_range).max() == 1.0
    assert yuv_ref.ycbcr_to_rgb(0, 0, 0, matrix, yuv_range)[[0, 2]].max() == 0.0


def test_resampling_of_the_restatement():
    c = np.array([[10., 30.], [50., 70.]])
    up = yuv_ref.upsample(c, 3, 4)                          # h = 3: the last chroma row serves one luma row
    assert np.array_equal(up[0], [10, 20, 30, 30])          # row 0: 0.75 C0 + 0.25 C(max(-1, 0)) = C0; x = 3 clamps to column 1
    assert np.array_equal(up[1], 0.75 * np.array([10, 20, 30, 30]) + 0.25 * np.array([50, 60, 70, 70]))
    assert np.array_equal(up[2], 0.75 * np.array([50, 60, 70, 70]) + 0.25 * np.array([10, 20, 30, 30]))
    flat = np.full((5, 7), 3.25)
    assert np.array_equal(yuv_ref.downsample(flat), np.full((3, 4), 3.25))
    assert np.array_equal(yuv_ref.upsample(np.full((3, 4), 3.25), 5, 7), flat)
    ramp = np.tile(np.arange(8.), (2, 1))
    assert np.array_equal(yuv_ref.downsample(ramp)[0], [0.25, 2, 4, 6])      # the left tap of column 0 is clamped
    y, cb, cr = (np.arange(24, dtype=np.uint8).reshape(4, 6), np.arange(6, dtype=np.uint8).reshape(2, 3),
                 np.arange(6, 12, dtype=np.uint8).reshape(2, 3))
    for layout in ('nv12', 'i420'):
        packed = yuv_ref.pack(y, cb, cr, layout)
        assert packed.shape == (6, 6) and all(np.array_equal(a, b) for a, b in zip(yuv_ref.unpack(packed, layout), (y, cb, cr)))


# ---- layout rules
def test_yuv_layouts_are_never_inferred_and_come_packed_or_as_planes():
    packed = torch.zeros(9, 8, dtype=torch.uint8)                               # 6 x 8
    with pytest.raises(ValueError):
        frames.resolve_layout(packed)                                           # a 2-D uint8 tensor with layout None
    with pytest.raises(ValueError):
        frames.ingest(packed)
    for layout in ('nv12', 'i420'):
        assert frames.resolve_layout(packed, layout) == (layout, 6, 8)
        planes, h, w = frames.yuv_planes(packed, layout)
        assert (h, w) == (6, 8) and planes[0].shape == (6, 8) and planes[0].data_ptr() == packed.data_ptr()
        assert [tuple(p.shape) for p in planes[1:]] == ([(3, 4, 2)] if layout == 'nv12' else [(3, 4), (3, 4)])
        assert planes[1].data_ptr() == packed.data_ptr() + 48
        if layout == 'i420':
            assert planes[2].data_ptr() == packed.data_ptr() + 60
        for bad in (torch.zeros(9, 7, dtype=torch.uint8),                       # odd width
                    torch.zeros(8, 8, dtype=torch.uint8),                       # rows not 3/2 of an even height
                    torch.zeros(3, 8, dtype=torch.uint8)[:0],
                    torch.zeros(9, 8), torch.zeros(9, 8, 1, dtype=torch.uint8), None, "nv12",
                    (packed,), (packed[:6],), (packed[:6], packed[:6], packed[:6], packed[:6])):
            with pytest.raises(ValueError):
                frames.resolve_layout(bad, layout)
            with pytest.raises(ValueError):
                frames.ingest(bad, layout)                                      # ... said before any GPU call
    # a pitched packed frame: NV12 by stride, I420 refused
    wide = torch.zeros(9, 12, dtype=torch.uint8)[:, 2:10]
    planes, _, _ = frames.yuv_planes(wide, 'nv12')
    assert planes[1].stride() == (12, 2, 1) and planes[1].data_ptr() == wide.data_ptr() + 6 * 12
    with pytest.raises(ValueError, match="contiguous"):
        frames.yuv_planes(wide, 'i420')
    # planes: odd sizes in this form only
    y, uv, u, v = (torch.zeros(7, 9, dtype=torch.uint8), torch.zeros(4, 5, 2, dtype=torch.uint8),
                   torch.zeros(4, 5, dtype=torch.uint8), torch.zeros(4, 5, dtype=torch.uint8))
    assert frames.resolve_layout((y, uv), 'nv12') == ('nv12', 7, 9)
    assert frames.resolve_layout([y, u, v], 'i420') == ('i420', 7, 9)
    for bad, layout in (((y, u, v), 'nv12'), ((y, uv), 'i420'), ((y, u), 'nv12'), ((y, uv[:3]), 'nv12'),
                        ((y, u, v[:, :4]), 'i420'), ((y, u.float(), v), 'i420'), ((y[0], u, v), 'i420'),
                        ((y, u, v), 'yuv'), ((y, uv), None), ((y, uv), 'hwc_rgb')):
        with pytest.raises(ValueError):
            frames.resolve_layout(bad, layout)


def test_describe_yuv_passes_pitched_and_offset_planes_by_stride():
    buf = torch.zeros(4096, dtype=torch.uint8)
    y = buf.as_strided((7, 9), (13, 1), 1)
    uv = buf.as_strided((4, 5, 2), (15, 2, 1), 201)
    u = buf.as_strided((4, 5), (7, 1), 301)
    v = buf.as_strided((4, 5), (9, 1), 403)
    planes, d = frames.describe_yuv((y, uv), 'nv12', 7, 9)
    assert [p.data_ptr() for p in planes] == [y.data_ptr(), uv.data_ptr()]
    assert (d.format, d.h, d.w, d.matrix, d.range) == (0, 7, 9, 0, 0)
    assert (d.plane[0], d.plane[1], d.plane[2]) == (y.data_ptr(), uv.data_ptr(), None)
    assert tuple(d.row_stride)[:2] == (13, 15)
    planes, d = frames.describe_yuv((y, u, v), 'i420', 7, 9, 'bt709', 'full')
    assert (d.format, d.matrix, d.range) == (1, 1, 1)
    assert tuple(d.plane) == (y.data_ptr(), u.data_ptr(), v.data_ptr()) and tuple(d.row_stride) == (13, 7, 9)
    skip = buf.as_strided((4, 5), (20, 2), 0)                                 # a column stride no descriptor expresses: copied
    planes, d = frames.describe_yuv((y, skip, v), 'i420', 7, 9)
    assert planes[1].is_contiguous() and d.row_stride[1] == 5 and planes[2].data_ptr() == v.data_ptr()
    with pytest.raises(ValueError, match="plane 1"):
        frames.describe_yuv((y, skip, v), 'i420', 7, 9, copy=False)             # ... and refused as a destination
    for kw in (dict(matrix='bt2020'), dict(yuv_range='tv')):
        with pytest.raises(ValueError):
            frames.describe_yuv((y, uv), 'nv12', 7, 9, **kw)


def test_argument_checks_come_before_the_gpu():
    packed = torch.zeros(9, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="matrix"):
        frames.ingest(packed, 'nv12', matrix='bt2020')
    with pytest.raises(ValueError, match="range"):
        frames.ingest(packed, 'i420', yuv_range='pc')
    with pytest.raises(ValueError, match="pad mode"):
        frames.ingest(packed, 'nv12', pad_mode='circular')
    with pytest.raises(ValueError, match="reflect"):
        frames.ingest(packed, 'nv12', multiple=16)              # 10 rows of padding out of a 6-row frame
    with pytest.raises(ValueError, match="out must be"):
        frames.ingest(packed, 'nv12', out=torch.zeros(3, 8, 12))
    sr = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError, match="layout"):
        frames.emit(sr, 8, 8, 'yuv420')
    with pytest.raises(ValueError, match="crop"):
        frames.emit(sr, 9, 8, 'nv12')
    for h, w in ((7, 8), (8, 7), (7, 7)):                       # an odd crop needs planes
        with pytest.raises(ValueError, match="planes"):
            frames.emit(sr, h, w, 'nv12')
        with pytest.raises(ValueError):
            frames.emit(sr, h, w, 'i420', out=torch.zeros(12, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out is a"):
        frames.emit(sr, 8, 8, 'nv12', out=torch.zeros(9, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="matrix"):
        frames.emit(sr, 8, 8, 'nv12', matrix='rec709')
    with pytest.raises(RuntimeError, match="GPU"):               # a valid call gets as far as the device check
        frames.emit(sr, 8, 8, 'nv12')
    with pytest.raises(RuntimeError, match="GPU"):
        frames.emit(sr, 7, 7, 'i420', out=(torch.zeros(7, 7, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8),
                                           torch.zeros(4, 4, dtype=torch.uint8)))


class _Mean(torch.nn.Module):
    nframes = 3

    def forward(self, x):
        return x.mean(1)


def _first(gen):
    return next(iter(gen))


@pytest.mark.parametrize("edvr", [False, True])
def test_super_resolve_frames_checks_yuv_arguments_first(edvr):
    if edvr:
        from dynavsr_amd.models.archs.EDVR_arch import EDVR
        net = EDVR()                                    # on the CPU: a valid call gets as far as the device check
        opt = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
    else:
        net = _Mean()
        opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    packed = torch.zeros(7, 27, 22, dtype=torch.uint8)                          # 18 x 22
    y, uv = torch.zeros(13, 15, dtype=torch.uint8), torch.zeros(7, 8, 2, dtype=torch.uint8)
    u8 = torch.zeros(7, 18, 22, 3, dtype=torch.uint8)
    bad = [
        dict(frames=packed),                                                    # never inferred
        dict(frames=packed, layout='yuv420p'),
        dict(frames=packed, layout='hwc_rgb'),
        dict(frames=u8, layout='nv12'),
        dict(frames=packed, layout='nv12', matrix='bt2020'),
        dict(frames=packed, layout='i420', yuv_range='tv'),
        dict(frames=packed, layout='nv12', out='yuv'),
        dict(frames=packed, layout='nv12', pad_mode='circular'),
        dict(frames=packed[:, :26], layout='nv12'),                             # 26 rows are not 3/2 of an even height
        dict(frames=packed[:, :, :21], layout='i420'),
        dict(frames=packed[:, :, :20], layout='i420'),                          # packed I420 must be contiguous
        dict(frames=torch.zeros(7, 3, 22, dtype=torch.uint8), layout='nv12'),   # H < 4
        dict(frames=[(y, uv)] * 3 + [(y, uv[:6])] + [(y, uv)] * 3, layout='nv12'),
        dict(frames=[(y, uv)] * 3 + [(y[:12], uv)] + [(y, uv)] * 3, layout='nv12'),   # frames of two sizes
        dict(frames=[(y, uv)] * 3 + [packed[0]] + [(y, uv)] * 3, layout='nv12'),      # ... of two kinds
        dict(frames=[(y, uv)] * 7, layout='i420'),
        dict(frames=[(y, uv)] * 7),                                             # planes are not inferred either
        dict(frames=u8, out='nv12', matrix='bt2020'),
    ]
    if not edvr:
        bad.append(dict(frames=[(y, uv)] * 7, layout='nv12'))                    # scale 1: a packed 13 x 15 output cannot be
        bad.append(dict(frames=u8[:, :17], out='i420'))
    for kw in bad:
        fr = kw.pop('frames')
        with pytest.raises(ValueError):
            _first(adapt.super_resolve_frames(opt, net, fr, **kw))
    if edvr:
        for fr, kw in ((packed, dict(layout='nv12')), (packed, dict(layout='i420', out='float', matrix='bt709', yuv_range='full')),
                       ([(y, uv)] * 7, dict(layout='nv12', out='hwc_rgb')), (u8, dict(out='nv12')),
                       (torch.zeros(7, 3, 18, 22), dict(out='i420'))):
            with pytest.raises(RuntimeError, match="MI355X"):
                _first(adapt.super_resolve_frames(opt, net, fr, **kw))


# ---- the C entry points, without a device
def _desc(lib, fmt=0, h=6, w=8, matrix=0, rng=0, planes=(A16 + 1, A16 + 101, A16 + 201), rows=None):
    if rows is None:
        wc = (w + 1) // 2
        rows = (w, 2 * wc, 0) if fmt == 0 else (w, wc, wc)
    d = lib.YuvDesc(fmt, h, w, matrix, rng)
    for i in range(3):
        d.plane[i] = planes[i]
        d.row_stride[i] = rows[i]
    return d


DESC_CASES = [
    (dict(fmt=2), b"format"), (dict(fmt=-1), b"format"),
    (dict(matrix=2), b"matrix"), (dict(matrix=-1), b"matrix"),
    (dict(rng=2), b"range"), (dict(rng=-1), b"range"),
    (dict(planes=(None, A16, A16)), b"null plane 0"),
    (dict(planes=(A16, None, A16)), b"null plane 1"),
    (dict(fmt=1, planes=(A16, A16, None)), b"null plane 2"),
    (dict(rows=(7, 8, 0)), b"row stride"),
    (dict(rows=(8, 7, 0)), b"row stride"),                 # NV12: a chroma row is 2 * Wc bytes
    (dict(w=7, rows=(7, 7, 0)), b"row stride"),            # ... = 8 for an odd width of 7
    (dict(fmt=1, rows=(8, 3, 4)), b"row stride"),
    (dict(fmt=1, rows=(8, 4, 3)), b"row stride"),
    (dict(h=0), b"frame size"), (dict(w=0), b"frame size"),
]


def test_frame_ingest_yuv_bad_arguments_without_gpu(lib):
    l = lib.lib()

    def ingest(dst=A16, Hp=8, Wp=8, pad=0, null_desc=False, **kw):
        d = _desc(lib, **kw)
        return l.dvsr_frame_ingest_yuv(None if null_desc else ctypes.byref(d), dst, Hp, Wp, pad, None)

    cases = DESC_CASES + [
        (dict(null_desc=True), b"null"),
        (dict(dst=None), b"null"),
        (dict(h=9), b"frame size"), (dict(w=9, rows=(9, 10, 0)), b"frame size"),       # larger than the target
        (dict(pad=2), b"pad mode"), (dict(pad=-1), b"pad mode"),
        (dict(h=4), b"reflect"), (dict(w=4), b"reflect"),                              # pad 4 >= 4
        (dict(dst=A16 + 4), b"misaligned"),
        (dict(Wp=10), b"multiple of 4"),
    ]
    for kw, word in cases:
        assert ingest(**kw) == INVALID, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())
    d = _desc(lib, fmt=0, planes=(A16 + 1, A16 + 3, None))          # NV12 ignores plane[2]: this one passes every check ...
    assert l.dvsr_frame_ingest_yuv(ctypes.byref(d), None, 8, 8, 0, None) == INVALID and b"null planar" in l.dvsr_last_error()


def test_frame_emit_yuv_bad_arguments_without_gpu(lib):
    l = lib.lib()

    def emit(src=A16, Hs=8, Ws=8, lo=0.0, hi=1.0, null_desc=False, **kw):
        d = _desc(lib, **kw)
        return l.dvsr_frame_emit_yuv(src, Hs, Ws, None if null_desc else ctypes.byref(d), lo, hi, None)

    cases = DESC_CASES + [
        (dict(null_desc=True), b"null"),
        (dict(src=None), b"null"),
        (dict(h=9), b"frame size"), (dict(w=12, rows=(12, 12, 0)), b"frame size"),
        (dict(src=A16 + 8), b"misaligned"),
        (dict(Ws=6), b"multiple of 4"),
        (dict(lo=1.0, hi=1.0), b"range ["), (dict(lo=1.0, hi=0.0), b"range ["),
    ]
    for kw, word in cases:
        assert emit(**kw) == INVALID, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())


def test_extract_frame_yuv_bad_arguments_without_gpu(lib):
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
        return l.dvsr_edvr_stream_extract_frame_yuv(h, params, None if null_desc else ctypes.byref(d), pad, slot, cache,
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
        (dict(fmt=9), b"format"), (dict(matrix=3), b"matrix"), (dict(rng=3), b"range"),
        (dict(planes=(A16, None, None)), b"null plane 1"),
        (dict(fmt=1, planes=(A16, A16, None)), b"null plane 2"),
        (dict(pad=3), b"pad mode"),
        (dict(h=21), b"frame size"), (dict(w=25, rows=(25, 26, 0)), b"frame size"),     # larger than the plan's 20 x 24
        (dict(h=0), b"frame size"),
        (dict(h=10), b"reflect"),                                                       # 10 rows of padding out of 10
        (dict(rows=(21, 22, 0)), b"row stride"), (dict(rows=(22, 21, 0)), b"row stride"),
        (dict(fmt=1, rows=(22, 11, 10)), b"row stride"),
    ]
    for kw, word in cases:
        assert extract(**kw) == INVALID, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())
    l.dvsr_edvr_stream_destroy(h)
