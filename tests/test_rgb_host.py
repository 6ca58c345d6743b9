"""CPU: the host side of 16-bit RGB and planar integer RGB / GBR frames (dynavsr_amd/frames.py: RGB_LAYOUTS; the new values of
dvsr_frame_desc.format): layout resolution and every ValueError, describe() by stride, the restatement
tests/rgb_ref.py against itself, and the argument checks of the C entries, which return DVSR_ERR_INVALID before any launch -- so
they run without a GPU, with pointers that are never dereferenced."""
import ctypes

import numpy as np
import pytest
import torch

import rgb_ref
from dynavsr_amd import adapt, frames

INVALID = -1
A16 = 0x10000           # a 16-byte aligned address that nothing reads
U16, I16, U8 = torch.uint16, torch.int16, torch.uint8


@pytest.fixture(scope="module")
def lib():
    import os
    from dynavsr_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        from dynavsr_amd import build
        build.build()
    return _lib


def _zeros(layout, h=6, w=8, ps=3, dtype=None):
    dt = dtype or (U8 if rgb_ref.LAYOUTS[layout][1] == 8 else U16)
    return torch.zeros(rgb_ref.shape(layout, h, w, ps), dtype=dt)


def test_the_layout_table(lib):
    assert set(frames.RGB_LAYOUTS) == set(rgb_ref.NAMES) and len(frames.RGB_LAYOUTS) == 10
    for name in frames.RGB_LAYOUTS:
        assert frames.layout_depth(name) == rgb_ref.LAYOUTS[name][1] and not frames.is_yuv(name)
    assert lib.frame_depth(lib.FRAME_U16_CHW_GBR, 10) == lib.FRAME_U16_CHW_GBR | (10 << 8)
    assert lib.frame_depth(lib.FRAME_U16_CHW_RGB, 16) == lib.FRAME_U16_CHW_RGB            # 0 means 16
    # the seven old values keep their numbers
    assert (lib.FRAME_F32_CHW, lib.FRAME_U8_HWC_RGB, lib.FRAME_U8_HWC_BGR, lib.FRAME_U8_Y, lib.FRAME_U16_Y_MSB, lib.FRAME_U16_Y_10,
            lib.FRAME_U16_Y_12) == (0, 1, 2, 3, 4, 5, 6)
    assert frames.LAYOUTS == ('chw', 'hwc_rgb', 'hwc_bgr')


def test_layout_resolution():
    for name in frames.RGB_LAYOUTS:
        assert frames.resolve_layout(_zeros(name), name) == (name, 6, 8)
        if rgb_ref.LAYOUTS[name][1] > 8:
            assert frames.resolve_layout(_zeros(name, dtype=I16), name) == (name, 6, 8)        # int16: the same bits
    assert frames.resolve_layout(_zeros('hwc_bgr16', ps=4), 'hwc_bgr16') == ('hwc_bgr16', 6, 8)
    bad = [(_zeros('hwc_rgb16'), None),                                # never inferred from dtype or shape
           (_zeros('chw_rgb16'), None), (_zeros('chw_rgb8'), None),
           (_zeros('chw_rgb8'), 'chw'),                                # 'chw' stays the float layout
           (_zeros('hwc_rgb16', dtype=U8), 'hwc_rgb16'), (_zeros('hwc_rgb16'), 'hwc_rgb'),
           (_zeros('chw_rgb8', dtype=U16), 'chw_rgb8'), (_zeros('chw_gbr10', dtype=U8), 'chw_gbr10'),
           (_zeros('chw_rgb16', dtype=torch.int32), 'chw_rgb16'), (torch.zeros(3, 6, 8), 'chw_rgb16'),
           (_zeros('hwc_rgb16'), 'chw_rgb16'), (_zeros('chw_rgb16'), 'hwc_rgb16'),             # the other shape
           (_zeros('hwc_rgb16', ps=2), 'hwc_rgb16'), (_zeros('hwc_rgb16', ps=5), 'hwc_rgb16'),
           (torch.zeros(4, 6, 8, dtype=U16), 'chw_gbr16'), (torch.zeros(6, 8, dtype=U16), 'chw_rgb12'),
           (torch.zeros(3, 0, 8, dtype=U16), 'chw_rgb12'), (torch.zeros(6, 0, 3, dtype=U16), 'hwc_rgb16'),
           (_zeros('chw_rgb16'), 'chw_rgb14'), (_zeros('chw_rgb16'), 'gbrp16le'), (_zeros('hwc_rgb16'), 'hwc_rgb10')]
    for frame, layout in bad:
        with pytest.raises(ValueError):
            frames.resolve_layout(frame, layout)
        with pytest.raises(ValueError):                                # ... and ingest says so before any GPU call
            frames.ingest(frame, layout)
    with pytest.raises(ValueError, match="reflect"):
        frames.ingest(_zeros('chw_gbr10'), 'chw_gbr10', multiple=16)
    with pytest.raises(ValueError, match="pad mode"):
        frames.ingest(_zeros('hwc_rgb16'), 'hwc_rgb16', pad_mode='wrap')


def test_emit_argument_checks_come_before_the_gpu():
    sr = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError, match="layout"):
        frames.emit(sr, 8, 8, 'chw_rgb14')
    with pytest.raises(ValueError, match="crop"):
        frames.emit(sr, 9, 8, 'chw_rgb16')
    with pytest.raises(ValueError, match="hi > lo"):
        frames.emit(sr, 8, 8, 'hwc_rgb16', min_max=(1, 1))
    for layout, out in (('hwc_rgb16', torch.zeros(8, 8, 3, dtype=U8)), ('hwc_rgb16', torch.zeros(8, 8, 4, dtype=U16)),
                        ('hwc_bgr16', torch.zeros(8, 8, 4, dtype=U16)[:, :, :3]),          # an emitted frame has three words
                        ('hwc_rgb16', torch.zeros(3, 8, 8, dtype=U16)), ('chw_gbr10', torch.zeros(8, 8, 3, dtype=U16)),
                        ('chw_rgb8', torch.zeros(3, 8, 8, dtype=U16)), ('chw_rgb12', torch.zeros(3, 8, 7, dtype=U16)),
                        ('chw_rgb12', torch.zeros(3, 8, 16, dtype=U16)[:, :, ::2]),         # a column stride
                        ('chw_gbr16', torch.zeros(1, 8, 8, dtype=U16).expand(3, 8, 8))):    # planes that overlap
        with pytest.raises(ValueError, match="out must"):
            frames.emit(sr, 8, 8, layout, out=out)
    with pytest.raises(RuntimeError, match="GPU"):                      # a good call gets as far as the device check
        frames.emit(sr, 8, 8, 'chw_gbr10', out=torch.zeros(3, 8, 8, dtype=I16))


def test_describe_passes_views_by_stride(lib):
    base = torch.zeros(10, 12, 4, dtype=U16)
    view = base[1:7, 2:10, :3]                                          # offset, pitched, a fourth word per pixel
    t, d = frames.describe(view, 'hwc_bgr16')
    assert t.data_ptr() == view.data_ptr()
    assert (d.format, d.h, d.w, d.row_stride, d.pixel_stride) == (lib.FRAME_U16_HWC_BGR, 6, 8, 96, 8)
    flat = torch.zeros(400, dtype=I16)
    v3 = flat.as_strided((6, 8, 3), (25, 3, 1), 3)                      # an odd pitch in words: 50 bytes, 6 bytes in
    t, d = frames.describe(v3, 'hwc_rgb16')
    assert t.data_ptr() == v3.data_ptr() and (d.format, d.row_stride, d.pixel_stride) == (lib.FRAME_U16_HWC_RGB, 50, 6)
    t, d = frames.describe(base[:, ::2, :3], 'hwc_rgb16')              # a pixel stride of 8 words: copied once
    assert t.is_contiguous() and t.shape == (10, 6, 3) and (d.row_stride, d.pixel_stride) == (36, 6)
    t, d = frames.describe(base.permute(1, 0, 2)[:, :, :3], 'hwc_rgb16')
    assert t.is_contiguous() and (d.h, d.w, d.row_stride) == (12, 10, 60)
    # planar: any sample-aligned offset, any row pitch, any plane stride that keeps the planes apart
    flat = torch.zeros(1000, dtype=U16)
    pv = flat.as_strided((3, 6, 8), (77, 9, 1), 5)
    t, d = frames.describe(pv, 'chw_gbr10')
    assert t.data_ptr() == pv.data_ptr()
    assert (d.format, d.h, d.w, d.row_stride, d.plane_stride, d.pixel_stride) == (
        lib.frame_depth(lib.FRAME_U16_CHW_GBR, 10), 6, 8, 18, 154, 2)
    bytes_ = torch.zeros(1000, dtype=U8)
    bv = bytes_.as_strided((3, 6, 8), (61, 9, 1), 3)
    t, d = frames.describe(bv, 'chw_rgb8')
    assert t.data_ptr() == bv.data_ptr() and (d.format, d.row_stride, d.plane_stride, d.pixel_stride) == (lib.FRAME_U8_CHW_RGB, 9, 61, 1)
    whole = torch.zeros(3, 10, 12, dtype=U16)
    tv = whole[:, 2:8, 1:9]
    t, d = frames.describe(tv, 'chw_rgb16')
    assert t.data_ptr() == tv.data_ptr() and (d.format, d.row_stride, d.plane_stride) == (lib.FRAME_U16_CHW_RGB, 24, 240)
    assert frames.tile_view(whole, 'chw_rgb16', 2, 1, 6, 8).data_ptr() == tv.data_ptr()
    assert frames.tile_view(base, 'hwc_rgb16', 1, 2, 6, 8).shape == (6, 8, 4)
    for view in (whole[:, :, ::2], flat.as_strided((3, 6, 8), (40, 9, 1), 0), whole[0:1].expand(3, 10, 12)):
        t, d = frames.describe(view, 'chw_rgb12')                       # a column stride / planes that overlap: copied once
        assert t.is_contiguous() and t.data_ptr() != view.data_ptr() and d.plane_stride == d.h * d.row_stride
        assert torch.equal(t, view)


def test_score_and_cut_argument_checks():
    h, w = 24, 40
    sides = {name: (name, h, w) for name in frames.RGB_LAYOUTS + ('chw', 'hwc_rgb', 'nv12', 'p010')}
    ok = [('hwc_rgb16', 'chw_rgb16', 16), ('hwc_bgr16', 'chw_gbr16', 16), ('chw_gbr10', 'chw_rgb10', 10), ('chw_gbr10', 'chw', 10),
          ('chw', 'hwc_rgb16', 16), ('chw_rgb8', 'hwc_rgb', 8), ('chw_gbr8', 'chw', 8), ('chw_rgb12', 'chw_gbr12', 12)]
    for a, b, depth in ok:
        assert frames.check_score(sides[a], sides[b], 'rgb')[2] == depth
    assert frames.check_score(sides['chw_rgb8'], sides['nv12'], 'y')[2] == 8      # a planar 8-bit side pairs with any 8-bit side
    assert frames.check_score(sides['chw'], sides['chw'], 'rgb')[2] == 8
    for a, b in (('hwc_rgb16', 'chw_rgb12'), ('chw_rgb10', 'chw_rgb12'), ('hwc_rgb', 'hwc_rgb16'), ('chw_rgb8', 'chw_rgb16')):
        with pytest.raises(ValueError, match="mixed bit depths"):
            frames.check_score(sides[a], sides[b], 'rgb')
    for a, b in (('hwc_rgb16', 'hwc_rgb16'), ('chw_gbr10', 'chw'), ('chw_rgb12', 'chw_rgb12'), ('chw', 'chw_gbr16'),
                 ('chw_rgb10', 'p010')):
        with pytest.raises(ValueError, match="channel='y'"):
            frames.check_score(sides[a], sides[b], 'y')
    with pytest.raises(ValueError, match="mixed bit depths"):                     # the Y of a float frame is 8-bit
        frames.check_score(sides['chw'], sides['p010'], 'y')
    with pytest.raises(ValueError, match="channel='y'"):
        frames.score(_zeros('chw_rgb16', h, w), _zeros('chw_rgb16', h, w), 'chw_rgb16', 'chw_rgb16', channel='y')
    with pytest.raises(ValueError, match="mixed"):
        frames.score(_zeros('hwc_rgb16', h, w), _zeros('chw_rgb12', h, w), 'hwc_rgb16', 'chw_rgb12')
    with pytest.raises(ValueError):
        frames.luma_sad([_zeros('chw_rgb16', dtype=U8)], 'chw_rgb16')


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
    w16 = torch.zeros(7, 18, 22, 3, dtype=U16)
    p16 = torch.zeros(7, 3, 18, 22, dtype=I16)
    u8 = torch.zeros(7, 18, 22, 3, dtype=U8)
    bad = [
        dict(frames=w16), dict(frames=p16),                                      # never inferred
        dict(frames=w16, layout='chw_rgb16'), dict(frames=p16, layout='hwc_rgb16'),
        dict(frames=p16.to(U8), layout='chw_gbr12'), dict(frames=w16, layout='hwc_rgb'),
        dict(frames=w16, layout='hwc_rgb48'), dict(frames=u8, out='chw_rgb14'), dict(frames=u8, out='rgb48le'),
        dict(frames=w16, layout='hwc_rgb16', pad_mode='circular'),
        dict(frames=[w16[0], w16[1][:16]] + [w16[i] for i in range(2, 7)], layout='hwc_rgb16'),
        dict(frames=p16, layout='chw_gbr10', gt=p16, gt_layout='chw_gbr10', score='y',
             scores=torch.zeros(7, 2, dtype=torch.float64)),                     # no Y from RGB above 8 bits
        dict(frames=u8, out='chw_rgb16', gt=u8, scores=torch.zeros(7, 2, dtype=torch.float64)),   # mixed depths
    ]
    for kw in bad:
        fr = kw.pop('frames')
        with pytest.raises(ValueError):
            _first(adapt.super_resolve_frames(opt, net, fr, **kw))
    if edvr:
        for fr, kw in ((w16, dict(layout='hwc_rgb16')), (p16, dict(layout='chw_gbr10', out='hwc_bgr16')), (u8, dict(out='chw_gbr10')),
                       (p16.to(U8), dict(layout='chw_rgb8', out='float', pad_mode='replicate', multiple=16))):
            with pytest.raises(RuntimeError, match="MI355X"):
                _first(adapt.super_resolve_frames(opt, net, fr, **kw))


def test_the_restatement():
    r = np.random.RandomState(0)
    for name in rgb_ref.NAMES:
        planar, d, order = rgb_ref.LAYOUTS[name]
        assert frames.layout_depth(name) == d and frames.resolve_layout(_zeros(name, 5, 7), name) == (name, 5, 7)   # the library's table
        lev = r.randint(0, 1 << d, (3, 5, 7))
        frame = rgb_ref.from_levels(lev, name, junk=r.randint(0, 65536, (3, 5, 7)) if planar and 8 < d < 16 else None)
        assert frame.shape == rgb_ref.shape(name, 5, 7) and frame.dtype == rgb_ref.dtype(name)
        assert np.array_equal(rgb_ref.levels(frame, name), lev)                       # the junk above the level is ignored
        x = rgb_ref.ingest(frame, name, 8, 8, 'reflect')
        assert x.dtype == np.float32 and x.shape == (3, 8, 8) and x.max() <= 1.0
        assert np.array_equal(x[:, :5, :7], (lev / np.float64((1 << d) - 1)).astype(np.float32))   # correctly rounded
        assert np.array_equal(x[:, 5:, :7], x[:, [3, 2, 1], :7]) and np.array_equal(x[:, :, 7], x[:, :, 5])
        e = rgb_ref.ingest(frame, name, 8, 8, 'replicate')
        assert np.array_equal(e[:, 7, :7], e[:, 4, :7]) and np.array_equal(e[:, :, 7], e[:, :, 6])
        back = rgb_ref.emit(x, 5, 7, name)
        assert np.array_equal(rgb_ref.levels(back, name), lev) and int(back.max()) <= (1 << d) - 1   # high bits written as 0
    # BGR words and GBR planes are where they belong
    lev = np.arange(3)[:, None, None] * np.ones((3, 2, 2), dtype=np.int64) + 1       # R = 1, G = 2, B = 3
    assert rgb_ref.from_levels(lev, 'hwc_bgr16')[0, 0].tolist() == [3, 2, 1]
    assert rgb_ref.from_levels(lev, 'chw_gbr12')[:, 0, 0].tolist() == [2, 3, 1]
    assert rgb_ref.from_levels(lev, 'hwc_rgb16', ps=4)[0, 0].tolist() == [1, 2, 3, 0x1234]
    # round half to even, clamping, the (-1, 1) range
    top = 65535
    x = np.array([(0.5) / top, (1.5) / top, (2.5) / top, -0.3, 1.7, 1.0], dtype=np.float64)
    assert rgb_ref.quant(x.astype(np.float32), top).tolist()[3:] == [0, top, top]
    assert rgb_ref.quant(np.float32(0.0), 1023, -1.0, 1.0) == 512                    # 511.5 rounds to even
    assert rgb_ref.quant(np.array([0.5, 1.5, 2.5, 3.5], dtype=np.float32) / np.float32(4), 4).tolist() == [0, 2, 2, 4]
    # the luma of the cut detector: the 8-bit rule on the top 8 bits
    f16 = rgb_ref.from_levels(r.randint(0, 65536, (3, 4, 6)), 'chw_rgb16')
    r8, g8, b8 = (f16 >> 8).astype(np.int64)
    assert np.array_equal(rgb_ref.luma8(f16, 'chw_rgb16'), (77 * r8 + 150 * g8 + 29 * b8 + 128) >> 8)


def _desc(lib, fmt, h=6, w=8, row=None, plane=None, ps=None):
    planar, words = (fmt & 0xff) >= lib.FRAME_U8_CHW_RGB, (fmt & 0xff) not in (lib.FRAME_U8_CHW_RGB, lib.FRAME_U8_CHW_GBR)
    es = 2 if words else 1
    if ps is None:
        ps = es if planar else 6
    if row is None:
        row = w * ps
    if plane is None:
        plane = h * row if planar else 0
    return lib.FrameDesc(fmt, h, w, row, plane, ps)


def _rgb_cases(lib, emit):
    """(descriptor keywords, address offset, the word the message must hold) of every bad descriptor of the new formats."""
    H16, P8, P16 = lib.FRAME_U16_HWC_RGB, lib.FRAME_U8_CHW_GBR, lib.FRAME_U16_CHW_RGB
    cases = [
        (dict(fmt=lib.frame_depth(P16, 14)), 0, b"depth"), (dict(fmt=lib.frame_depth(P16, 8)), 0, b"depth"),
        (dict(fmt=lib.frame_depth(P16, 11)), 0, b"depth"), (dict(fmt=lib.frame_depth(H16, 10)), 0, b"depth"),
        (dict(fmt=lib.frame_depth(P8, 10)), 0, b"depth"), (dict(fmt=lib.FRAME_U16_CHW_GBR | 0x1000), 0, b"format"),
        (dict(fmt=22), 0, b"format"), (dict(fmt=15), 0, b"format"),
        (dict(fmt=H16), 1, b"odd"), (dict(fmt=H16, row=49), 0, b"odd"),
        (dict(fmt=lib.frame_depth(P16, 10)), 1, b"odd"), (dict(fmt=P16, row=17), 0, b"odd"), (dict(fmt=P16, plane=6 * 16 + 1), 0, b"odd"),
        (dict(fmt=H16, row=46), 0, b"row stride"), (dict(fmt=P16, row=14), 0, b"row stride"), (dict(fmt=P8, row=7), 0, b"row stride"),
        (dict(fmt=P16, row=18, plane=5 * 18 + 14), 0, b"plane stride"), (dict(fmt=P8, row=9, plane=5 * 9 + 7), 0, b"plane stride"),
        (dict(fmt=H16, ps=3), 0, b"pixel stride"), (dict(fmt=H16, ps=4), 0, b"pixel stride"), (dict(fmt=H16, ps=10), 0, b"pixel stride"),
        (dict(fmt=P16, ps=1), 0, b"pixel stride"), (dict(fmt=P8, ps=3), 0, b"pixel stride"), (dict(fmt=P16, ps=6), 0, b"pixel stride"),
        (dict(fmt=H16, h=0), 0, b"frame size"), (dict(fmt=P16, w=9), 0, b"frame size"),
    ]
    if emit:
        cases.append((dict(fmt=H16, ps=8, row=64), 0, b"pixel stride"))            # an emitted frame has three words per pixel
    return cases


def _good(lib):
    H16, B16 = lib.FRAME_U16_HWC_RGB, lib.FRAME_U16_HWC_BGR
    return [dict(fmt=H16), dict(fmt=B16, row=50), dict(fmt=lib.FRAME_U8_CHW_RGB), dict(fmt=lib.FRAME_U8_CHW_GBR, row=9, plane=5 * 9 + 8),
            dict(fmt=lib.FRAME_U16_CHW_RGB), dict(fmt=lib.frame_depth(lib.FRAME_U16_CHW_GBR, 10), row=18, plane=5 * 18 + 16),
            dict(fmt=lib.frame_depth(lib.FRAME_U16_CHW_RGB, 12)), dict(fmt=lib.frame_depth(lib.FRAME_U16_CHW_GBR, 16))]


def test_frame_ingest_refuses_bad_descriptors(lib):
    l = lib.lib()

    def ingest(d, src=A16, dst=A16, Hp=8, Wp=8, pad=0):
        return l.dvsr_frame_ingest(src, ctypes.byref(d), dst, Hp, Wp, pad, None)
    for kw, off, word in _rgb_cases(lib, False):
        assert ingest(_desc(lib, **kw), src=A16 + off) == INVALID, kw
        assert word in l.dvsr_last_error() and l.dvsr_last_error().startswith(b"frame_ingest:"), (kw, l.dvsr_last_error())
    # good descriptors pass the descriptor's own checks: the call is then refused for something else, named after them
    for kw in _good(lib) + [dict(fmt=lib.FRAME_U16_HWC_RGB, ps=8, row=64)]:
        assert ingest(_desc(lib, **kw), pad=2) == INVALID and b"pad mode" in l.dvsr_last_error(), kw
        assert ingest(_desc(lib, h=4, **kw)) == INVALID and b"reflect" in l.dvsr_last_error(), kw
        assert ingest(_desc(lib, **kw), dst=A16 + 4) == INVALID and b"misaligned" in l.dvsr_last_error(), kw
    # the seven old values pass the checks they passed
    for d in (lib.FrameDesc(0, 6, 8, 8, 48, 1), lib.FrameDesc(1, 6, 8, 24, 0, 3), lib.FrameDesc(2, 6, 8, 33, 0, 4)):
        assert ingest(d, src=A16 + (0 if d.format == 0 else 1), pad=2) == INVALID and b"pad mode" in l.dvsr_last_error()
    for fmt in (3, 4, 5, 6):
        assert ingest(lib.FrameDesc(fmt, 6, 8, 16, 0, 2)) == INVALID and b"format" in l.dvsr_last_error()


def test_frame_emit_refuses_bad_descriptors(lib):
    l = lib.lib()

    def emit(d, dst=A16, src=A16, Hs=8, Ws=8, lo=0.0, hi=1.0):
        return l.dvsr_frame_emit(src, Hs, Ws, dst, ctypes.byref(d), lo, hi, None)
    for kw, off, word in _rgb_cases(lib, True):
        assert emit(_desc(lib, **kw), dst=A16 + off) == INVALID, kw
        assert word in l.dvsr_last_error() and l.dvsr_last_error().startswith(b"frame_emit:"), (kw, l.dvsr_last_error())
    for kw in _good(lib):
        assert emit(_desc(lib, **kw), lo=1.0, hi=1.0) == INVALID and b"range" in l.dvsr_last_error(), kw
        assert emit(_desc(lib, **kw), src=A16 + 8) == INVALID and b"misaligned" in l.dvsr_last_error(), kw
    for d in (lib.FrameDesc(1, 6, 8, 24, 0, 3), lib.FrameDesc(2, 6, 8, 33, 0, 3)):
        assert emit(d, dst=A16 + 1, lo=1.0, hi=1.0) == INVALID and b"range" in l.dvsr_last_error()
    assert emit(lib.FrameDesc(0, 6, 8, 8, 48, 1), src=A16 + 8) == INVALID and b"misaligned" in l.dvsr_last_error()


def test_extract_frame_refuses_bad_descriptors(lib):
    l = lib.lib()
    h = ctypes.c_void_p()
    cfg = lib.EdvrConfig(64, 5, 8, 5, 10, 4, 2)
    assert l.dvsr_edvr_stream_create(cfg, 8, 8, 6, ctypes.byref(h)) == 0
    n = l.dvsr_edvr_stream_num_params(h)
    arr = (ctypes.c_void_p * n)(*([A16] * n))
    cb, wb = l.dvsr_edvr_stream_cache_bytes(h), l.dvsr_edvr_stream_workspace_bytes(h)

    def extract(d, frame=A16, pad=0):
        return l.dvsr_edvr_stream_extract_frame(h, arr, frame, ctypes.byref(d), pad, 0, A16, cb, A16, wb, 0, None)
    for kw, off, word in _rgb_cases(lib, False):
        assert extract(_desc(lib, **kw), frame=A16 + off) == INVALID, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())
    for kw in _good(lib):
        assert extract(_desc(lib, **kw), pad=3) == INVALID and b"pad mode" in l.dvsr_last_error(), kw
    l.dvsr_edvr_stream_destroy(h)


def test_luma_sad_and_score_refuse_bad_descriptors(lib):
    l = lib.lib()
    for kw, off, word in _rgb_cases(lib, False):
        if word == b"frame size" and kw.get('w') == 9:
            continue                                                    # (no target size here)
        d = _desc(lib, **kw)
        assert l.dvsr_frame_luma_sad(A16 + off, A16, ctypes.byref(d), 4096, 1, A16, None) == INVALID, kw
        assert word in l.dvsr_last_error() and l.dvsr_last_error().startswith(b"frame_luma_sad:"), (kw, l.dvsr_last_error())
    for kw in _good(lib):
        d = _desc(lib, **kw)
        assert l.dvsr_frame_luma_sad(A16, A16, ctypes.byref(d), 4096, 0, A16, None) == INVALID and b"pairs" in l.dvsr_last_error(), kw
    d = _desc(lib, lib.FRAME_U16_CHW_RGB)
    assert l.dvsr_frame_luma_sad(A16, A16, ctypes.byref(d), 4095, 2, A16, None) == INVALID and b"odd frame stride" in l.dvsr_last_error()
    # score: a 24 x 40 pair
    hh, ww = 24, 40
    need = l.dvsr_frame_score_workspace_bytes(3, hh, ww)

    def score(da, db, args, a=A16, b=A16):
        return l.dvsr_frame_score(a, ctypes.byref(da), b, ctypes.byref(db), ctypes.byref(args), A16, A16, need, None)
    RGB = lambda depth: lib.ScoreArgs(lib.SCORE_RGB, 0, depth, 0.0, 1.0)
    Y = lambda depth: lib.ScoreArgs(lib.SCORE_Y, 0, depth, 0.0, 1.0)
    w16 = _desc(lib, lib.FRAME_U16_HWC_RGB, hh, ww)
    p16, p10 = _desc(lib, lib.FRAME_U16_CHW_GBR, hh, ww), _desc(lib, lib.frame_depth(lib.FRAME_U16_CHW_GBR, 10), hh, ww)
    p8, u8 = _desc(lib, lib.FRAME_U8_CHW_RGB, hh, ww), lib.FrameDesc(lib.FRAME_U8_HWC_RGB, hh, ww, 3 * ww, 0, 3)
    f32 = lib.FrameDesc(lib.FRAME_F32_CHW, hh, ww, ww, hh * ww, 1)
    bad = [(w16, p16, RGB(8)), (w16, p16, RGB(12)), (w16, p10, RGB(16)), (w16, p10, RGB(10)), (p10, p10, RGB(12)),
           (w16, u8, RGB(16)), (w16, u8, RGB(8)), (p8, p16, RGB(8)), (p8, u8, RGB(16)),
           (w16, p16, Y(16)), (p10, p10, Y(10)), (p10, f32, Y(10)), (f32, f32, Y(10)),
           (w16, p16, RGB(9)), (w16, f32, lib.ScoreArgs(lib.SCORE_RGB, 0, 16, 1.0, 1.0))]
    for da, db, args in bad:
        assert score(da, db, args) == INVALID, (da.format, db.format, args.depth)
        assert l.dvsr_last_error().startswith(b"frame_score:")
    for kw, off, word in _rgb_cases(lib, False):
        if word == b"frame size" or 'row' in kw or 'plane' in kw:
            continue                                                    # (those sizes and strides belong to 6 x 8)
        d = _desc(lib, h=hh, w=ww, **kw)
        assert score(d, d, RGB(16), a=A16 + off) == INVALID, kw
        assert l.dvsr_last_error().startswith(b"frame_score:"), (kw, l.dvsr_last_error())
    # good pairs get past every check of the descriptors: the workspace is what is missing
    for da, db, args in ((w16, p16, RGB(16)), (p10, f32, RGB(10)), (p8, u8, RGB(8)), (p8, u8, Y(8)), (f32, f32, RGB(16))):
        assert l.dvsr_frame_score(A16, ctypes.byref(da), A16, ctypes.byref(db), ctypes.byref(args), A16, A16, need - 1, None) == -3


def test_degrade_and_imresize_keep_refusing(lib):
    l = lib.lib()
    for kw in _good(lib):
        d = _desc(lib, h=50, w=71, **{k: v for k, v in kw.items() if k == 'fmt'})
        assert l.dvsr_frame_degrade(A16, ctypes.byref(d), A16, 13, 2, A16, 36, 36 * 25, 1, None) == INVALID
        assert b"format" in l.dvsr_last_error(), kw
        ax = lib.ResizeAxis(A16, A16, 8)
        assert l.dvsr_frame_imresize(A16, ctypes.byref(d), 48, 68, 1, 4, 1, A16, 20, 240, 12, 17, ctypes.byref(ax), ctypes.byref(ax), 0,
                                     None) == INVALID
        assert b"format" in l.dvsr_last_error(), kw
