"""CPU: the host side of the frame path (dynavsr_amd/frames.py, the new arguments of adapt.super_resolve_frames, and the
argument checks of dvsr_frame_ingest / dvsr_frame_emit / dvsr_edvr_stream_extract_frame, which return DVSR_ERR_INVALID
before any launch -- so they can be exercised without a GPU, with pointers that are never dereferenced)."""
import ctypes

import pytest
import torch

from dynavsr_amd import adapt, frames

INVALID = -1
A16 = 0x10000           # a 16-byte aligned address that nothing reads


@pytest.fixture(scope="module")
def lib():
    import os
    from dynavsr_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        from dynavsr_amd import build
        build.build()
    return _lib


def test_padded_size():
    for m in (1, 4, 16):
        for h in range(4, 41):
            for w in range(4, 41):
                Hp, Wp = frames.padded_size(h, w, m)
                assert Hp % m == 0 and Wp % m == 0
                assert h <= Hp < h + m and w <= Wp < w + m
    assert frames.padded_size(480, 854, 4) == (480, 856)
    assert frames.padded_size(270, 480, 16) == (272, 480)
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        with pytest.raises(ValueError):
            frames.padded_size(*bad)


def test_layout_rules():
    u8 = torch.zeros(6, 8, 3, dtype=torch.uint8)
    u8x = torch.zeros(6, 8, 4, dtype=torch.uint8)
    f32 = torch.zeros(3, 6, 8)
    assert frames.resolve_layout(u8) == ('hwc_rgb', 6, 8)
    assert frames.resolve_layout(u8x, 'hwc_bgr') == ('hwc_bgr', 6, 8)
    assert frames.resolve_layout(f32) == ('chw', 6, 8)
    assert frames.resolve_layout(f32.double(), 'chw') == ('chw', 6, 8)
    for frame, layout in ((u8, 'chw'), (f32, 'hwc_rgb'), (f32, 'hwc_bgr'), (u8, 'rgb'), (f32, 'nchw'),
                          (torch.zeros(3, 6, 8, dtype=torch.uint8), None),       # planar uint8
                          (torch.zeros(6, 8, 2, dtype=torch.uint8), None),
                          (torch.zeros(6, 8, dtype=torch.uint8), None),
                          (torch.zeros(1, 6, 8, 3, dtype=torch.uint8), None),
                          (torch.zeros(6, 8, 3), None),                           # interleaved float
                          (torch.zeros(6, 8, 3, dtype=torch.int32), None),
                          (torch.zeros(0, 8, 3, dtype=torch.uint8), None)):
        with pytest.raises(ValueError):
            frames.resolve_layout(frame, layout)
        with pytest.raises(ValueError):                                           # ... and ingest says so before any GPU call
            frames.ingest(frame, layout)


def test_ingest_argument_checks_come_before_the_gpu():
    u8 = torch.zeros(6, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="pad mode"):
        frames.ingest(u8, pad_mode='circular')
    with pytest.raises(ValueError, match="reflect"):
        frames.ingest(u8, multiple=16)                 # 10 rows of padding out of a 6-row frame
    with pytest.raises(ValueError):
        frames.ingest(u8, multiple=0)
    with pytest.raises(ValueError, match="out must be"):
        frames.ingest(u8, out=torch.zeros(3, 8, 12))    # [3,8,8] is the padded size
    with pytest.raises(ValueError, match="layout"):
        frames.emit(torch.zeros(3, 8, 8), 8, 8, 'hwc')
    with pytest.raises(ValueError, match="crop"):
        frames.emit(torch.zeros(3, 8, 8), 9, 8, 'hwc_rgb')


def test_describe_passes_views_by_stride():
    base = torch.zeros(10, 12, 4, dtype=torch.uint8)
    view = base[1:7, 2:10, :3]                         # offset, pitched, a fourth byte per pixel
    t, d = frames.describe(view, 'hwc_bgr')
    assert t.data_ptr() == view.data_ptr()
    assert (d.format, d.h, d.w, d.row_stride, d.pixel_stride) == (2, 6, 8, 48, 4)
    fb = torch.zeros(3, 10, 12)
    fv = fb[:, 2:8, 1:9]
    t, d = frames.describe(fv, 'chw')
    assert t.data_ptr() == fv.data_ptr() and (d.format, d.h, d.w, d.row_stride, d.plane_stride) == (0, 6, 8, 12, 120)
    t, d = frames.describe(fb[:, :, ::2], 'chw')       # a column stride the descriptor cannot express: copied
    assert t.is_contiguous() and (d.row_stride, d.plane_stride) == (6, 60)
    t, d = frames.describe(base[:, ::2, :3], 'hwc_rgb')    # ... and a pixel stride of 8 bytes
    assert t.is_contiguous() and (d.row_stride, d.pixel_stride) == (18, 3)


class _Mean(torch.nn.Module):
    nframes = 3

    def forward(self, x):
        return x.mean(1)


def _first(gen):
    return next(iter(gen))


@pytest.mark.parametrize("edvr", [False, True])
def test_super_resolve_frames_checks_arguments_first(edvr):
    if edvr:
        from dynavsr_amd.models.archs.EDVR_arch import EDVR
        net = EDVR()                                    # on the CPU: a valid call gets as far as the device check
        opt = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
    else:
        net = _Mean()
        opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    u8 = torch.zeros(7, 18, 22, 3, dtype=torch.uint8)
    f32 = torch.zeros(7, 3, 18, 22)
    bad = [
        dict(frames=torch.zeros(7, 3, 18, 22, dtype=torch.uint8)),            # uint8 must be [H,W,3|4]
        dict(frames=torch.zeros(7, 18, 22, 2, dtype=torch.uint8)),
        dict(frames=torch.zeros(7, 18, 22, dtype=torch.uint8)),
        dict(frames=u8, layout='chw'),
        dict(frames=f32, layout='hwc_rgb'),
        dict(frames=u8, layout='yuv'),
        dict(frames=u8, out='uint8'),
        dict(frames=u8, pad_mode='circular'),
        dict(frames=u8, multiple=0),
        dict(frames=torch.zeros(7, 3, 22, 3, dtype=torch.uint8)),              # H < 4
        dict(frames=torch.zeros(7, 5, 6, 3, dtype=torch.uint8), multiple=16),  # reflect pad >= the dimension
        dict(frames=[u8[0], u8[1][:16]] + [u8[i] for i in range(2, 7)]),       # frames of two sizes
        dict(frames=[u8[0], f32[1]] + [u8[i] for i in range(2, 7)]),           # frames of two kinds
        dict(frames=[]),
    ]
    for kw in bad:
        fr = kw.pop('frames')
        with pytest.raises(ValueError):
            _first(adapt.super_resolve_frames(opt, net, fr, **kw))
    if edvr:
        for kw in (dict(), dict(out='float'), dict(layout='hwc_bgr', out='hwc_rgb', pad_mode='replicate', multiple=16)):
            with pytest.raises(RuntimeError, match="MI355X"):
                _first(adapt.super_resolve_frames(opt, net, u8, **kw))
        with pytest.raises(RuntimeError, match="MI355X"):                       # float frames of any size get there too now
            _first(adapt.super_resolve_frames(opt, net, f32))


def _desc(lib, fmt=1, h=6, w=8, row=None, plane=0, ps=3):
    if row is None:
        row = w * ps if fmt else w
    if fmt == 0 and plane == 0:
        plane = h * row
    return lib.FrameDesc(fmt, h, w, row, plane, ps)


def test_frame_ingest_bad_arguments_without_gpu(lib):
    l = lib.lib()

    def ingest(src=A16 + 1, d=None, dst=A16, Hp=8, Wp=8, pad=0, null_desc=False):
        d = d if d is not None else _desc(lib)
        return l.dvsr_frame_ingest(src, None if null_desc else ctypes.byref(d), dst, Hp, Wp, pad, None)

    cases = [
        (dict(src=None), b"null"),
        (dict(null_desc=True), b"null"),
        (dict(dst=None), b"null"),
        (dict(d=_desc(lib, fmt=3)), b"format"),
        (dict(d=_desc(lib, fmt=-1)), b"format"),
        (dict(pad=2), b"pad mode"),
        (dict(pad=-1), b"pad mode"),
        (dict(d=_desc(lib, h=0)), b"frame size"),
        (dict(d=_desc(lib, w=0)), b"frame size"),
        (dict(d=_desc(lib, h=9)), b"frame size"),          # larger than the target
        (dict(d=_desc(lib, w=9)), b"frame size"),
        (dict(d=_desc(lib, h=4), Hp=8), b"reflect"),       # pad 4 >= 4 rows
        (dict(d=_desc(lib, w=4), Wp=8), b"reflect"),
        (dict(d=_desc(lib, ps=2)), b"pixel stride"),
        (dict(d=_desc(lib, ps=5)), b"pixel stride"),
        (dict(d=_desc(lib, row=23)), b"row stride"),
        (dict(d=_desc(lib, ps=4, row=31)), b"row stride"),
        (dict(d=_desc(lib, fmt=0, row=7), src=A16), b"row stride"),
        (dict(d=_desc(lib, fmt=0, row=8, plane=47), src=A16), b"plane stride"),
        (dict(d=_desc(lib, fmt=0), src=A16 + 2), b"misaligned"),
        (dict(dst=A16 + 4), b"misaligned"),
        (dict(Wp=10), b"multiple of 4"),
    ]
    for kw, word in cases:
        assert ingest(**kw) == INVALID, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())


def test_frame_emit_bad_arguments_without_gpu(lib):
    l = lib.lib()

    def emit(src=A16, Hs=8, Ws=8, dst=A16 + 1, d=None, lo=0.0, hi=1.0, null_desc=False):
        d = d if d is not None else _desc(lib)
        return l.dvsr_frame_emit(src, Hs, Ws, dst, None if null_desc else ctypes.byref(d), lo, hi, None)

    cases = [
        (dict(src=None), b"null"),
        (dict(dst=None), b"null"),
        (dict(null_desc=True), b"null"),
        (dict(d=_desc(lib, fmt=5)), b"format"),
        (dict(d=_desc(lib, h=0)), b"frame size"),
        (dict(d=_desc(lib, h=9)), b"frame size"),
        (dict(d=_desc(lib, w=12)), b"frame size"),
        (dict(d=_desc(lib, ps=4, row=32)), b"pixel stride"),     # an emitted frame has 3 bytes per pixel
        (dict(d=_desc(lib, ps=1)), b"pixel stride"),
        (dict(d=_desc(lib, row=20)), b"row stride"),
        (dict(d=_desc(lib, fmt=0, row=6), dst=A16), b"row stride"),
        (dict(d=_desc(lib, fmt=0), dst=A16 + 1), b"misaligned"),
        (dict(src=A16 + 8), b"misaligned"),
        (dict(Ws=6), b"multiple of 4"),
        (dict(lo=1.0, hi=1.0), b"range"),
    ]
    for kw, word in cases:
        assert emit(**kw) == INVALID, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())


def test_extract_frame_bad_arguments_without_gpu(lib):
    l = lib.lib()
    h = ctypes.c_void_p()
    cfg = lib.EdvrConfig(64, 5, 8, 5, 10, 4, 2)
    assert l.dvsr_edvr_stream_create(cfg, 20, 24, 6, ctypes.byref(h)) == 0
    assert l.dvsr_edvr_stream_create(cfg, 18, 24, 6, ctypes.byref(ctypes.c_void_p())) == INVALID   # padding is the caller's
    n = l.dvsr_edvr_stream_num_params(h)
    arr = (ctypes.c_void_p * n)(*([A16] * n))
    cb, wb = l.dvsr_edvr_stream_cache_bytes(h), l.dvsr_edvr_stream_workspace_bytes(h)

    def extract(frame=A16 + 1, d=None, pad=0, slot=0, cache=A16, cache_bytes=cb, ws=A16, ws_bytes=wb, null_desc=False,
                params=arr):
        d = d if d is not None else _desc(lib, h=18, w=22)
        return l.dvsr_edvr_stream_extract_frame(h, params, frame, None if null_desc else ctypes.byref(d), pad, slot, cache,
                                                cache_bytes, ws, ws_bytes, 0, None)

    cases = [
        (dict(frame=None), b"null"),
        (dict(null_desc=True), b"null"),
        (dict(params=None), b"null"),
        (dict(cache=None), b"null"),
        (dict(ws=None), b"null"),
        (dict(slot=6), b"slot"),
        (dict(slot=-1), b"slot"),
        (dict(cache_bytes=cb - 4), b"cache"),
        (dict(ws_bytes=wb - 4), b"workspace"),
        (dict(cache=A16 + 4), b"aligned"),
        (dict(d=_desc(lib, fmt=9, h=18, w=22)), b"format"),
        (dict(pad=3), b"pad mode"),
        (dict(d=_desc(lib, h=21, w=22)), b"frame size"),          # larger than the plan's 20 x 24
        (dict(d=_desc(lib, h=18, w=25)), b"frame size"),
        (dict(d=_desc(lib, h=0, w=22)), b"frame size"),
        (dict(d=_desc(lib, h=10, w=22)), b"reflect"),             # 10 rows of padding out of 10
        (dict(d=_desc(lib, h=18, w=22, ps=6)), b"pixel stride"),
        (dict(d=_desc(lib, h=18, w=22, row=65)), b"row stride"),
        (dict(d=_desc(lib, fmt=0, h=18, w=22), frame=A16 + 1), b"misaligned"),
    ]
    for kw, word in cases:
        assert extract(**kw) == INVALID, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())
    l.dvsr_edvr_stream_destroy(h)
