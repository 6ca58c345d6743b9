"""CPU: the resampler's definition (tests/resize_ref.py) against torch's own op, the host half of csrc/frame_resize.hip
(dvsr_frame_resize_taps / _table, the argument checks of dvsr_frame_resize) against the definition, and the argument checks of
adapt.super_resolve_frames(..., out_size=) -- none of which needs a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_ref as ref

AXES = [(37, 21), (53, 30), (64, 16), (61, 16), (12, 24), (20, 29), (20, 20), (16, 4)]
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}


@pytest.fixture(scope="module")
def lib():
    from dynavsr_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        from dynavsr_amd import build
        build.build()
    return _lib


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[2]))
def test_reference_is_torch_bicubic_antialias(case):
    (h, w), _, size = case
    x = np.random.RandomState(h * 1000 + w).uniform(0, 1, (3, h, w))
    want = F.interpolate(torch.from_numpy(x)[None], size=size, mode='bicubic', antialias=True, align_corners=False)[0].numpy()
    err = float(np.abs(ref.resize(x, size) - want).max())
    print("%dx%d -> %dx%d: max-abs %.2e against torch fp64" % (h, w, size[0], size[1], err))
    assert err <= 1e-12


@pytest.mark.parametrize("axis", AXES, ids=lambda a: "%d-%d" % a)
def test_table_is_the_definition(lib, axis):
    from dynavsr_amd import frames
    n_in, n_out = axis
    first, weights = ref.axis_table(n_in, n_out)
    taps = lib.lib().dvsr_frame_resize_taps(n_in, n_out)
    assert taps == weights.shape[1]
    got_first, got = frames.resize_table(n_in, n_out)
    assert got_first.dtype == torch.int32 and got.dtype == torch.float32 and tuple(got.shape) == (n_out, taps)
    assert np.array_equal(got_first.numpy(), first)
    g = got.numpy().astype(np.float64)
    err = float(np.abs(g - weights).max())
    print("%d -> %d: %d taps, weights within %.2e of fp64" % (n_in, n_out, taps, err))
    assert err <= 2.0 ** -24
    assert float(np.abs(g.sum(1) - 1.0).max()) <= taps * 2.0 ** -24
    assert bool((g[weights == 0.0] == 0.0).all())                              # the zero-padding of short rows
    if n_in == n_out:
        for i in range(n_out):
            assert g[i, i - first[i]] == 1.0 and float(np.abs(g[i]).sum()) == 1.0


def test_table_rejects_ratios_outside_the_bounds(lib):
    from dynavsr_amd import frames
    l = lib.lib()
    assert l.dvsr_frame_resize_taps(64, 16) >= 1 and l.dvsr_frame_resize_taps(12, 24) >= 1
    for n_in, n_out in ((65, 16), (12, 25), (0, 4), (4, 0)):
        assert l.dvsr_frame_resize_taps(n_in, n_out) == -1
        with pytest.raises(ValueError):
            frames.resize_table(n_in, n_out)


def test_resize_validation_without_gpu(lib):
    """No device is needed to be told that an argument is wrong (the pattern of test_conv_desc_validation_without_gpu); the
    pointers are host memory that a launch would fault on -- none is started."""
    l = lib.lib()
    src, dst = torch.zeros(3 * 8 * 8), torch.zeros(3 * 8 * 8)
    first, weights = torch.zeros(8, dtype=torch.int32), torch.zeros(8 * 4)
    good = lib.ResizeAxis(first.data_ptr(), weights.data_ptr(), 4)

    def call(s=src.data_ptr(), Hs=8, Ws=8, h=8, w=8, d=dst.data_ptr(), Ho=8, Wo=8, oh=8, ow=8, rows=good, cols=good):
        return l.dvsr_frame_resize(s, Hs, Ws, h, w, d, Ho, Wo, oh, ow, ctypes.byref(rows) if rows is not None else None,
                                   ctypes.byref(cols) if cols is not None else None, None)
    for kw, word in (({'s': None}, b"null"), ({'d': None}, b"null"), ({'rows': None}, b"null"), ({'cols': None}, b"null"),
                     ({'rows': lib.ResizeAxis(None, weights.data_ptr(), 4)}, b"null"),
                     ({'Wo': 6, 'ow': 6}, b"multiple of 4"), ({'Ws': 6, 'w': 6}, b"multiple of 4"),
                     ({'oh': 1}, b"ratios"), ({'h': 2, 'w': 2}, b"ratios"), ({'oh': 9}, b"destination"),
                     ({'cols': lib.ResizeAxis(first.data_ptr(), weights.data_ptr(), 0)}, b"taps"),
                     ({'rows': lib.ResizeAxis(first.data_ptr(), weights.data_ptr(), 19)}, b"taps"),
                     ({'s': src.data_ptr() + 4}, b"misaligned")):
        assert call(**kw) == -1, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())


@pytest.mark.parametrize("out_size,out", [((0, 8), None), ((8,), None), ('1080p', None), ((8, 8.0), None), ((7, 32), None),
                                          ((32, 7), None), ((65, 32), None), ((32, 65), None), ((31, 32), 'nv12'),
                                          ((32, 31), 'nv12'), ((32, 31), 'p010')],
                         ids=lambda v: str(v).replace(' ', ''))
def test_out_size_is_checked_before_the_gpu(out_size, out):
    """An 8 x 8 video through a x4 network: SR frames of 32 x 32.  The network and the frames live on the CPU, so reaching
    the device would raise a RuntimeError ("runs on the MI355X only"), not a ValueError."""
    from dynavsr_amd import adapt
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    net = EDVR()
    u8 = torch.zeros((7, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="out_size"):
        next(adapt.super_resolve_frames(OPT, net, u8, out=out, out_size=out_size))
    flt = torch.zeros((7, 3, 8, 8))
    with pytest.raises(ValueError, match="out_size"):
        next(adapt.super_resolve_frames(OPT, net, flt, out=out, out_size=out_size))


def test_out_size_of_another_network_is_checked_too():
    from dynavsr_amd import adapt

    class Mean(torch.nn.Module):
        nframes = 3

        def forward(self, x):
            raise AssertionError("the network must not run")

    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    u8 = torch.zeros((5, 8, 12, 3), dtype=torch.uint8)
    for out_size, out in (((1, 12), None), ((8, 25), None), ((7, 12), 'i420'), ('8x12', None)):
        with pytest.raises(ValueError, match="out_size"):
            next(adapt.super_resolve_frames(opt, Mean(), u8, padding='replicate', out=out, out_size=out_size))
