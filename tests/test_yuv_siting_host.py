"""CPU: chroma siting ('left' | 'center' | 'topleft') and the BT.2020 NCL matrix of the YCbCr frame path -- the fp64
restatement tests/yuv_siting_ref.py (its two statements of the resampling against each other, 'left' against the older
restatements, 'center' against torch's bilinear interpolation, the geometry on a ramp, the coefficients against H.273), the
names and the descriptors of dynavsr_amd/frames.py, the argument checks of the C entry points for the new values of `format` and
`matrix` (they return DVSR_ERR_INVALID before any launch, so they run without a GPU, with pointers that are never
dereferenced), and the argument checks of super_resolve_frames / adapt_frames."""
import ctypes
import os

import numpy as np
import pytest
import torch

import yuv16_ref
import yuv_chroma_ref
import yuv_ref
import yuv_siting_ref as ref
from dynavsr_amd import adapt, frames, video

INVALID = -1
A16 = 0x10000           # a 16-byte aligned address that nothing reads
SUBS = ('420', '422', '444')
NC = (1, 2, 3, 131)
# (layout, siting) -> the chroma field of `format`
FIELD = {('420', 'left'): 0, ('420', 'center'): 4, ('420', 'topleft'): 5, ('422', 'left'): 1, ('422', 'center'): 6,
         ('422', 'topleft'): 1, ('444', 'left'): 2, ('444', 'center'): 2, ('444', 'topleft'): 2}


@pytest.fixture(scope="module")
def lib():
    from dynavsr_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        from dynavsr_amd import build
        build.build()
    return _lib


def plane_sizes(sub, hc, wc):
    """The luma sizes (h, w) that have an hc x wc chroma plane."""
    hs = (hc,) if sub != '420' else tuple(h for h in (2 * hc - 1, 2 * hc))
    ws = (wc,) if sub == '444' else tuple(w for w in (2 * wc - 1, 2 * wc))
    return [(h, w) for h in hs for w in ws]


# ---- the restatement: its two statements, and the older restatements
@pytest.mark.parametrize("siting", ref.SITINGS)
@pytest.mark.parametrize("sub", SUBS)
def test_the_tap_formulas_are_linear_interpolation_at_the_sited_positions(sub, siting):
    r = np.random.RandomState(5)
    for hc in NC:
        for wc in NC:
            c = r.randint(0, 4096, (hc, wc)).astype(np.float64)
            for h, w in plane_sizes(sub, hc, wc):
                a, b = ref.upsample_taps(c, h, w, sub, siting), ref.upsample_interp(c, h, w, sub, siting)
                assert a.shape == b.shape == (h, w)
                assert np.array_equal(a, b), (hc, wc, h, w)                       # multiples of 1/16 of a level: exact
                assert np.array_equal(a * 16, np.rint(a * 16))
                big = r.uniform(-0.6, 0.6, (h, w))
                a, b = ref.downsample_taps(big, sub, siting), ref.downsample_filter(big, sub, siting)
                assert a.shape == b.shape == (hc, wc)
                assert float(np.abs(a - b).max()) <= 1e-15, (hc, wc, h, w)


def test_left_is_the_older_restatements():
    r = np.random.RandomState(6)
    for h, w in ((1, 1), (2, 2), (3, 5), (7, 9), (6, 10), (18, 262)):
        hc, wc = (h + 1) // 2, (w + 1) // 2
        c, big = r.randint(0, 256, (hc, wc)), r.uniform(0, 1, (h, w))
        assert np.array_equal(ref.upsample(c, h, w, 'i420'), yuv_ref.upsample(c, h, w))
        assert np.array_equal(ref.downsample(big, 'nv12'), yuv_ref.downsample(big))
        c2 = r.randint(0, 256, (h, wc))
        assert np.array_equal(ref.upsample(c2, h, w, 'nv16'), yuv_chroma_ref.upsample422(c2, h, w))
        assert np.array_equal(ref.upsample(c2, h, w, 'nv16', 'topleft'), yuv_chroma_ref.upsample422(c2, h, w))   # 4:2:2: the same x
        assert np.array_equal(ref.downsample(big, 'i422'), yuv_chroma_ref.downsample422(big))
        assert np.array_equal(ref.downsample(big, 'i422', 'topleft'), yuv_chroma_ref.downsample422(big))
        for siting in ref.SITINGS:                                               # 4:4:4: no siting
            assert np.array_equal(ref.upsample(big, h, w, 'i444', siting), big)
            assert np.array_equal(ref.downsample(big, 'i444', siting), big)
    h, w, Hp, Wp = 7, 9, 8, 12
    y, cb, cr = r.randint(0, 256, (h, w)), r.randint(0, 256, (4, 5)), r.randint(0, 256, (4, 5))
    sr = r.uniform(-0.2, 1.2, (3, Hp, Wp))
    for matrix, rng in (('bt601', 'limited'), ('bt709', 'full')):
        assert np.array_equal(ref.ingest(y, cb, cr, Hp, Wp, 'nv12', 'reflect', matrix, rng), yuv_ref.ingest(y, cb, cr, Hp, Wp, 'reflect', matrix, rng))
        assert np.array_equal(ref.ingest(4 * y, 4 * cb, 4 * cr, Hp, Wp, 'p010', 'replicate', matrix, rng),
                              yuv16_ref.ingest(4 * y, 4 * cb, 4 * cr, Hp, Wp, 10, 'replicate', matrix, rng))
        for a, b in zip(ref.emit(sr, h, w, 'i420', 0.0, 1.0, matrix, rng), yuv_ref.emit(sr, h, w, 0.0, 1.0, matrix, rng)):
            assert np.array_equal(a, b)
        for a, b in zip(ref.emit(sr, h, w, 'i420p12', -1.0, 1.0, matrix, rng), yuv16_ref.emit(sr, h, w, 12, -1.0, 1.0, matrix, rng)):
            assert np.array_equal(a, b)
        c2 = r.randint(0, 256, (h, 5))
        assert np.array_equal(ref.ingest(y, c2, c2, Hp, Wp, 'i422', 'reflect', matrix, rng),
                              yuv_chroma_ref.ingest(y, c2, c2, Hp, Wp, 'i422', 'reflect', matrix, rng))
        for a, b in zip(ref.emit(sr, h, w, 'p210', 0.0, 1.0, matrix, rng), yuv_chroma_ref.emit(sr, h, w, 'p210', 0.0, 1.0, matrix, rng)):
            assert np.array_equal(a, b)


def test_center_upsampling_is_torchs_bilinear_interpolation():
    r = np.random.RandomState(7)
    for hc in NC:
        for wc in NC:
            c = r.randint(0, 1024, (hc, wc)).astype(np.float64)
            want = torch.nn.functional.interpolate(torch.from_numpy(c)[None, None], scale_factor=2, mode='bilinear',
                                                   align_corners=False)[0, 0].numpy()
            for h, w in plane_sizes('420', hc, wc):
                assert np.array_equal(ref.upsample_taps(c, h, w, '420', 'center'), want[:h, :w]), (hc, wc, h, w)
            x = torch.nn.functional.interpolate(torch.from_numpy(c)[None], scale_factor=2, mode='linear', align_corners=False)[0].numpy()
            for _, w in plane_sizes('422', hc, wc):
                assert np.array_equal(ref.upsample_taps(c, hc, w, '422', 'center'), x[:, :w])


def test_the_geometry_on_a_ramp():
    """A plane linear in x and y survives down- then up-sampling away from the edges when both directions use one siting, and
    comes back shifted by half a luma pixel's worth where they differ."""
    h, w, ax, ay = 24, 28, 3.0, 5.0
    ramp = 100.0 + ax * np.arange(w)[None, :] + ay * np.arange(h)[:, None]
    inner = (slice(3, h - 3), slice(3, w - 3))
    # where a siting puts chroma sample (j, k), in units of half a luma pixel beyond (2j, 2k)
    off = {'left': (0, 1), 'center': (1, 1), 'topleft': (0, 0)}
    for down in ref.SITINGS:
        for up in ref.SITINGS:
            back = ref.upsample_taps(ref.downsample_taps(ramp, '420', down), h, w, '420', up)
            dx, dy = (off[down][0] - off[up][0]) / 2, (off[down][1] - off[up][1]) / 2
            assert float(np.abs(back - (ramp + ax * dx + ay * dy))[inner].max()) <= 1e-12, (down, up)
            assert (down == up) == (float(np.abs(back - ramp)[inner].max()) <= 1e-12)
    for down in ('left', 'center'):
        for up in ('left', 'center'):
            back = ref.upsample_taps(ref.downsample_taps(ramp, '422', down), h, w, '422', up)
            dx = (off[down][0] - off[up][0]) / 2
            assert float(np.abs(back - (ramp + ax * dx))[inner].max()) <= 1e-12, (down, up)


def test_small_worked_examples():
    c = np.array([[16., 32., 64.]])
    assert ref.upsample_taps(c, 1, 6, '422', 'center').tolist() == [[16., 20., 28., 40., 56., 64.]]
    assert ref.upsample_taps(c, 1, 5, '422', 'left').tolist() == [[16., 24., 32., 48., 64.]]
    c = np.array([[16.], [32.]])
    assert ref.upsample_taps(c, 4, 1, '420', 'topleft')[:, 0].tolist() == [16., 24., 32., 32.]
    assert ref.upsample_taps(c, 3, 1, '420', 'left')[:, 0].tolist() == [16., 20., 28.]
    big = np.array([[0., 8., 16., 24., 40.]])
    assert ref.downsample_taps(big, '422', 'center').tolist() == [[4., 20., 40.]]
    assert ref.downsample_taps(big, '422', 'left').tolist() == [[2., 16., 36.]]
    col = np.array([[0.], [8.], [16.]])
    assert ref.downsample_taps(col, '420', 'topleft')[:, 0].tolist() == [2., 14.]
    assert ref.downsample_taps(col, '420', 'center')[:, 0].tolist() == [4., 16.]


# ---- BT.2020 NCL
def test_bt2020_coefficients_are_h273s():
    kr, kb = ref.MATRICES['bt2020nc']
    assert (kr, kb) == (0.2627, 0.0593) and abs(1 - kr - kb - 0.6780) < 1e-12
    # BT.2020 table 4 writes the chroma quotients as 1.8814 and 1.4746
    assert abs(2 * (1 - kb) - 1.8814) < 1e-12 and abs(2 * (1 - kr) - 1.4746) < 1e-12
    for depth in (8, 10, 12):
        top, mid = 2 ** depth - 1, 2 ** (depth - 1)
        s = 2 ** (depth - 8)
        y, cb, cr = ref.rgb_to_ycbcr(np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]]).T, depth, 'bt2020nc', 'full')
        assert np.allclose(y, [kr * top, kb * top, top], atol=1e-9)
        assert np.allclose(cr, [mid + top / 2, mid - top * kb / (2 * (1 - kr)), mid], atol=1e-9)
        assert np.allclose(cb, [mid - top * kr / (2 * (1 - kb)), mid + top / 2, mid], atol=1e-9)
        y, cb, cr = ref.rgb_to_ycbcr(np.array([[0.0, 1.0, 0.0], [1.0, 1.0, 1.0]]).T, depth, 'bt2020nc', 'limited')
        assert np.allclose(y, [(16 + 219 * 0.6780) * s, 235 * s], atol=1e-9) and np.allclose(cb[1], 128 * s) and np.allclose(cr[1], 128 * s)


@pytest.mark.parametrize("yuv_range", ['limited', 'full'])
@pytest.mark.parametrize("matrix", ['bt601', 'bt709', 'bt2020nc'])
def test_rgb_round_trip_on_444_levels(matrix, yuv_range):
    rgb = np.random.RandomState(8).uniform(0, 1, (3, 9, 11))
    for depth in (8, 10, 12):
        back = ref.ycbcr_to_rgb(*ref.rgb_to_ycbcr(rgb, depth, matrix, yuv_range), depth, matrix, yuv_range, clamp=False)
        assert float(np.abs(back - rgb).max()) <= 1e-12


# ---- names and descriptors
def test_names():
    assert frames.YUV_SITINGS == ref.SITINGS
    for s in ref.SITINGS:
        frames.check_yuv_names('bt2020nc', 'full', s)
    frames.check_yuv_names('bt601', 'limited')                                       # two arguments, as before
    for bad in ('bottom', 'top', 'bottomleft', 'Left', 'mpeg2', 'jpeg', '', None, 0, 1):
        with pytest.raises(ValueError, match="siting"):
            frames.check_yuv_names('bt601', 'limited', bad)
    with pytest.raises(ValueError) as e:
        frames.check_yuv_names('bt2020', 'limited')
    msg = str(e.value)
    assert all(name in msg for name in ("'bt601'", "'bt709'", "'bt2020nc'")) and "non-constant" in msg
    for bad in ('bt2020', 'bt2020c', 'bt2020cl', 'bt2100', 'ictcp', 9, None):
        with pytest.raises(ValueError, match="matrix"):
            frames.check_yuv_names(bad, 'limited', 'left')


@pytest.mark.parametrize("layout", sorted(ref.LAYOUTS))
def test_describe_yuv_carries_the_siting_and_the_matrix(layout):
    sub, semi, depth, _ = ref.LAYOUTS[layout]
    dt = torch.uint8 if depth == 8 else torch.uint16
    h, w = 6, 8
    hc, wc = ref.chroma_size(layout, h, w)
    planes = (torch.zeros(h, w, dtype=dt),) + ((torch.zeros(hc, wc, 2, dtype=dt),) if semi else (torch.zeros(hc, wc, dtype=dt),) * 2)
    form = 0 if semi else 1
    for siting in ref.SITINGS:
        _, d = frames.describe_yuv(planes, layout, h, w, 'bt2020nc', 'full', True, siting)
        assert d.format == (FIELD[sub, siting] << 4 | form) and d.matrix == 9 and d.range == 1, (siting, hex(d.format))
        assert frames.describe_yuv(planes, layout, h, w, siting=siting)[1].format == d.format
    assert frames.describe_yuv(planes, layout, h, w, 'bt601', 'limited', True)[1].format == (FIELD[sub, 'left'] << 4 | form)
    assert frames.describe_yuv(planes, layout, h, w)[1].matrix == 0
    if sub == '420':
        assert frames.describe_yuv(planes, layout, h, w, siting='center')[1].format == 0x40 | form
        assert frames.describe_yuv(planes, layout, h, w, siting='topleft')[1].format == 0x50 | form
    if sub == '422':
        assert frames.describe_yuv(planes, layout, h, w, siting='center')[1].format == 0x60 | form
        assert frames.describe_yuv(planes, layout, h, w, siting='topleft')[1].format == 0x10 | form
    with pytest.raises(ValueError, match="siting"):
        frames.describe_yuv(planes, layout, h, w, siting='bottom')
    with pytest.raises(ValueError, match="matrix"):
        frames.describe_yuv(planes, layout, h, w, matrix='bt2020')


def test_every_function_takes_siting_and_checks_it_first():
    sr, nv12 = torch.zeros(3, 8, 8), torch.zeros(12, 8, dtype=torch.uint8)
    calls = [lambda **kw: frames.ingest(nv12, 'nv12', **kw), lambda **kw: frames.emit(sr, 8, 8, 'nv12', **kw),
             lambda **kw: frames.imresize(nv12, 2, 'nv12', **kw), lambda **kw: frames.degrade(nv12, frames.Imresize(2), 'nv12', **kw),
             lambda **kw: video.degrade_frames(nv12[None], frames.Imresize(2), layout='nv12', **kw),
             lambda **kw: frames.ingest(torch.zeros(8, 8, 3, dtype=torch.uint8), **kw),        # checked for every layout
             lambda **kw: frames.emit(sr, 8, 8, 'i444', **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="siting"):
            call(siting='bottom')
        with pytest.raises(ValueError, match="matrix"):
            call(matrix='bt2020')
        for kw in (dict(siting='center'), dict(siting='topleft', matrix='bt2020nc'), dict()):
            with pytest.raises(RuntimeError):                                   # as far as the device
                call(**kw)
    import inspect
    from dynavsr_amd import engine
    for f in (frames.ingest, frames.emit, frames.degrade, frames.imresize, frames.describe_yuv, engine.StreamPlan.extract_frame,
              video.super_resolve_frames, video.degrade_frames, video.evaluate_bicubic, adapt.adapt_frames):
        p = inspect.signature(f).parameters
        assert p['siting'].default == 'left', f
        names = list(p)
        if p['siting'].kind is not inspect.Parameter.KEYWORD_ONLY:                # appended: no positional call changes meaning
            assert names[-1] == 'siting', f


# ---- the C entry points, without a device
def _desc(lib, layout, field, matrix=0, h=6, w=8, short=None, form=None):
    sub, semi, depth, _ = ref.LAYOUTS[layout]
    es = 1 if depth == 8 else 2
    hc, wc = ref.chroma_size(layout, h, w)
    need = [w * es, (2 * wc if semi else wc) * es, 0 if semi else wc * es]
    fmt = field << 4 | ((0 if semi else 1) if form is None else form)
    d = lib.YuvDesc(fmt, h, w, matrix, 0) if depth == 8 else lib.Yuv16Desc(fmt, depth, h, w, matrix, 0)
    for i in range(3):
        d.plane[i] = A16 + 2 + 512 * i
        d.row_stride[i] = need[i] - (es if i == short else 0)
    return d, need


def _entries(lib, layout):
    l = lib.lib()
    suffix = 'yuv' if ref.LAYOUTS[layout][2] == 8 else 'yuv16'
    return l, getattr(l, "dvsr_frame_ingest_" + suffix), getattr(l, "dvsr_frame_emit_" + suffix)


CASES = [(lay, s) for lay in ('nv12', 'i420', 'p010', 'i420p12') for s in ('center', 'topleft')] + \
        [(lay, 'center') for lay in ('nv16', 'i422', 'p210', 'i422p10')]


@pytest.mark.parametrize("layout,siting", CASES)
def test_c_entry_points_take_the_sited_formats_and_bt2020_up_to_the_row_checks(lib, layout, siting):
    l, ingest, emit = _entries(lib, layout)
    sub, semi = ref.LAYOUTS[layout][:2]
    field = FIELD[sub, siting]
    assert field >= 4
    for matrix in (0, 1, 9):
        for h, w in ((6, 8), (5, 7)):
            for short in range(2 if semi else 3):                                  # one sample short: refused, with the length
                d, need = _desc(lib, layout, field, matrix, h, w, short)
                for rc in (ingest(ctypes.byref(d), A16, 8, 8, 0, None), emit(A16, 8, 8, ctypes.byref(d), 0.0, 1.0, None)):
                    assert rc == INVALID
                    msg = l.dvsr_last_error()
                    assert b"row stride" in msg and b"of plane %d " % short in msg and b"row of %d bytes" % need[short] in msg, msg
            # rows exactly as long as needed pass the frame's checks: the next check of each function is the one that answers
            d, _ = _desc(lib, layout, field, matrix, h, w)
            assert ingest(ctypes.byref(d), A16, 8, 8, 2, None) == INVALID and b"pad mode" in l.dvsr_last_error()
            assert emit(A16, 8, 8, ctypes.byref(d), 1.0, 1.0, None) == INVALID and b"range [" in l.dvsr_last_error()
    d, _ = _desc(lib, layout, field, 9, h=9)
    assert ingest(ctypes.byref(d), A16, 8, 8, 0, None) == INVALID and b"frame size" in l.dvsr_last_error()


@pytest.mark.parametrize("layout", ['nv12', 'i420', 'p010', 'i420p10', 'nv16', 'i444'])
def test_c_entry_points_refuse_what_is_not_a_format_or_a_matrix(lib, layout):
    l, ingest, emit = _entries(lib, layout)
    sub, semi = ref.LAYOUTS[layout][:2]
    # chroma fields 3 and 7 and above | a bit above bit 7 | a third form of a sited field (base 4) | the older refusals
    for fmt in (0x30, 0x31, 0x70, 0x71, 0x80, 0xf1, 0x140, 0x141, 0x44, 0x64, 0x54, 0x42, 0x20, 0x12, 0x22, 2, 9, -1, -16, 0x110):
        d, _ = _desc(lib, layout, FIELD[sub, 'left'])
        d.format = fmt
        for rc in (ingest(ctypes.byref(d), A16, 8, 8, 0, None), emit(A16, 8, 8, ctypes.byref(d), 0.0, 1.0, None)):
            assert rc == INVALID, hex(fmt)
            assert b"format" in l.dvsr_last_error(), (hex(fmt), l.dvsr_last_error())
    d, _ = _desc(lib, layout, 2, form=0)                                            # semi-planar 4:4:4
    ingest(ctypes.byref(d), A16, 8, 8, 0, None)
    assert b"4:4:4" in l.dvsr_last_error()
    for matrix in (2, 3, 4, 5, 6, 7, 8, 10, -1, 0x109):
        for field in sorted({FIELD[sub, s] for s in ref.SITINGS}):
            d, _ = _desc(lib, layout, field, matrix)
            for rc in (ingest(ctypes.byref(d), A16, 8, 8, 0, None), emit(A16, 8, 8, ctypes.byref(d), 0.0, 1.0, None)):
                assert rc == INVALID, matrix
                assert b"matrix" in l.dvsr_last_error(), (matrix, l.dvsr_last_error())


def test_extract_frame_takes_a_sited_frame_up_to_the_row_checks(lib):
    l = lib.lib()
    h = ctypes.c_void_p()
    cfg = lib.EdvrConfig(64, 5, 8, 5, 10, 4, 2)
    assert l.dvsr_edvr_stream_create(cfg, 20, 24, 6, ctypes.byref(h)) == 0
    n = l.dvsr_edvr_stream_num_params(h)
    arr = (ctypes.c_void_p * n)(*([A16] * n))
    cb, wb = l.dvsr_edvr_stream_cache_bytes(h), l.dvsr_edvr_stream_workspace_bytes(h)
    for layout, siting in (('i420', 'center'), ('p010', 'topleft'), ('nv16', 'center')):
        fn = getattr(l, "dvsr_edvr_stream_extract_frame_" + ('yuv' if ref.LAYOUTS[layout][2] == 8 else 'yuv16'))
        field = FIELD[ref.LAYOUTS[layout][0], siting]
        d, need = _desc(lib, layout, field, 9, 18, 22, short=1)
        assert fn(h, arr, ctypes.byref(d), 0, 0, A16, cb, A16, wb, 0, None) == INVALID
        assert b"row stride" in l.dvsr_last_error() and b"row of %d bytes" % need[1] in l.dvsr_last_error()
        d, _ = _desc(lib, layout, field, 9, 18, 22)
        assert fn(h, arr, ctypes.byref(d), 3, 0, A16, cb, A16, wb, 0, None) == INVALID and b"pad mode" in l.dvsr_last_error()
        d.format = 0x70
        assert fn(h, arr, ctypes.byref(d), 0, 0, A16, cb, A16, wb, 0, None) == INVALID and b"format" in l.dvsr_last_error()
    l.dvsr_edvr_stream_destroy(h)


# ---- the video functions
class _Mean(torch.nn.Module):
    nframes = 3

    def forward(self, x):
        return x.mean(1)


@pytest.mark.parametrize("edvr", [False, True])
def test_super_resolve_frames_checks_siting_before_the_device(edvr):
    if edvr:
        from dynavsr_amd.models.archs.EDVR_arch import EDVR
        net = EDVR()                                    # on the CPU: a valid call gets as far as the device check
        opt = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
    else:
        net = _Mean()
        opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    nv12 = torch.zeros(7, 27, 22, dtype=torch.uint8)                              # 18 x 22
    p010 = torch.zeros(7, 27, 22, dtype=torch.uint16)
    u8 = torch.zeros(7, 18, 22, 3, dtype=torch.uint8)
    for fr, kw in ((nv12, dict(layout='nv12', siting='bottom')), (p010, dict(layout='p010', siting='top', matrix='bt2020nc')),
                   (u8, dict(out='p010', siting='bottomleft')), (nv12, dict(layout='i420', siting=None)),
                   (p010, dict(layout='p010', matrix='bt2020', siting='topleft'))):
        with pytest.raises(ValueError, match="siting|matrix"):
            next(iter(video.super_resolve_frames(opt, net, fr, **kw)))
    for fr, kw in ((nv12, dict(layout='nv12', siting='center')), (p010, dict(layout='p010', siting='topleft', matrix='bt2020nc')),
                   (u8, dict(out='p010', siting='topleft', matrix='bt2020nc')), (nv12, dict(layout='i420', siting='left'))):
        with pytest.raises(RuntimeError, match="MI355X" if edvr else None):
            next(iter(video.super_resolve_frames(opt, net, fr, **kw)))
    with pytest.raises(ValueError, match="siting"):
        video.evaluate_bicubic(opt if edvr else dict(opt, scale=2), net, nv12, nv12, layout='nv12', score='y', siting='bottom')


def test_adapt_frames_checks_siting_before_the_device():
    from test_adapt_frames_host import _opt, _run
    opt = _opt()
    nv12 = torch.zeros(7, 48, 48, dtype=torch.uint8)                              # 32 x 48
    with pytest.raises(ValueError, match="siting"):
        _run(opt, nv12, layout='nv12', siting='bottom')
    with pytest.raises(ValueError, match="matrix"):
        _run(opt, nv12, layout='nv12', matrix='bt2020', siting='center')
    for kw in (dict(siting='center'), dict(siting='topleft', matrix='bt2020nc')):
        with pytest.raises(RuntimeError):                                           # no networks, no device: the first GPU call
            _run(opt, nv12, layout='nv12', **kw)
