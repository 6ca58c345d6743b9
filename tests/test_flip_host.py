"""CPU: the flip-test x4 self-ensemble's host side -- the numpy definitions (flip_ref.py) against torch's, the argument checks
of frames.flip / frames.flip_mean and of the `flip_test` keyword (all of them before any device call), and the two entry
points in header, library and ctypes table."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flip_ref as ref
from dynavsr_amd import adapt, frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = {0: None, 1: (-1,), 2: (-2,), 3: (-2, -1)}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_numpy_definitions_are_torchs(shape):
    xs = [ref.data(shape, 10 * sum(shape) + i) for i in range(4)]
    for flags in range(4):
        t = torch.from_numpy(xs[0])
        want = t if flags == 0 else torch.flip(t, DIMS[flags])
        got = ref.flip(xs[0], flags)
        assert np.array_equal(bits(got), bits(want.numpy()))
        nan_at, inf_at = ref.special_places(shape, flags)
        assert np.isnan(got.reshape(-1)[nan_at]) and np.isposinf(got.reshape(-1)[inf_at])
    a, b, c, d = (torch.from_numpy(x) for x in xs)
    want = ((((a + b.flip(-1)) + c.flip(-2)) + d.flip((-2, -1))) * 0.25).numpy()
    got = ref.flip_mean(*xs)
    assert got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(bits(got)[ok], bits(want)[ok])


def test_flip_mean_order_matters():
    """The four terms in another order round differently somewhere: the order is part of the definition."""
    xs = [np.random.RandomState(i).standard_normal((3, 8, 16)).astype(np.float32) for i in range(4)]
    other = (((ref.flip(xs[3], 3) + ref.flip(xs[2], 2)) + ref.flip(xs[1], 1)) + xs[0]) * np.float32(0.25)
    assert not np.array_equal(bits(ref.flip_mean(*xs)), bits(other))


@pytest.fixture
def no_device(monkeypatch):
    """Any call into the library or of a stream fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(frames.L, "lib", boom)
    monkeypatch.setattr(frames.L, "stream", boom)
    monkeypatch.setattr(torch.cuda, "current_stream", boom)


def test_flip_argument_errors(no_device):
    x = torch.zeros(3, 4, 8)
    assert x.data_ptr() % 16 == 0
    for flags in (-1, 4, 1.0, True, None, 'w'):
        with pytest.raises(ValueError):
            frames.flip(x, flags)
    bad = [x.double(), x.to(torch.uint8), torch.zeros(8), torch.zeros(3, 4, 6), torch.zeros(0, 4, 8), x[:, :, ::2],
           x.transpose(1, 2), torch.zeros(3 * 4 * 8 + 1)[1:].view(3, 4, 8), x.numpy(), None]
    for b in bad:
        with pytest.raises(ValueError):
            frames.flip(b, 1)
    for out in (x, x.view(3, 4, 8), torch.zeros(3, 4, 4), torch.zeros(3, 4, 8).double(), torch.zeros(3, 8, 8)[:, :4], 'out'):
        with pytest.raises(ValueError):
            frames.flip(x, 1, out=out)


def test_flip_mean_argument_errors(no_device):
    ys = [torch.zeros(1, 3, 4, 8) for _ in range(4)]
    for i in range(4):
        for b in (ys[i].double(), torch.zeros(1, 3, 4, 12), torch.zeros(1, 3, 4, 6), ys[i].transpose(2, 3), None,
                  torch.zeros(3 * 4 * 8 + 1)[1:].view(1, 3, 4, 8)):
            args = list(ys)
            args[i] = b
            with pytest.raises(ValueError):
                frames.flip_mean(*args)
    for out in ys + [torch.zeros(3, 4, 8), torch.zeros(1, 3, 4, 8).double(), torch.zeros(1, 3, 4, 16)[..., :8]]:
        with pytest.raises(ValueError):
            frames.flip_mean(*ys, out=out)


class Mean(torch.nn.Module):
    nframes = 3

    def forward(self, x):
        return x.mean(1)


@pytest.mark.parametrize("value", [1, 0, None, 'yes', 1.0])
def test_flip_test_must_be_a_bool(no_device, value):
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    video = torch.zeros(5, 3, 8, 8)
    for net in (Mean(), EDVR()):
        with pytest.raises(ValueError, match="flip_test"):
            next(adapt.super_resolve_frames(opt, net, video, flip_test=value))
    with pytest.raises(ValueError, match="flip_test"):
        next(adapt.super_resolve_video(opt, Mean(), [video[None]], flip_test=value))


def test_flip_test_of_another_network_needs_whole_float4s(no_device):
    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    with pytest.raises(ValueError, match="multiple of 4"):
        next(adapt.super_resolve_frames(opt, Mean(), torch.zeros(5, 3, 8, 10), flip_test=True))
    with pytest.raises(ValueError, match="multiple of 4"):
        next(adapt.super_resolve_frames(opt, Mean(), torch.zeros(5, 7, 9, 3, dtype=torch.uint8), flip_test=True))


# ---- header = exports = ctypes table (tests/test_cabi.py holds the whole set; here: the two are in it) ----
SYMBOLS = ("dvsr_frame_flip", "dvsr_frame_flip_mean")


@pytest.fixture(scope="module")
def lib():
    from dynavsr_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        from dynavsr_amd import build
        build.build()
    return _lib


def test_symbols_in_header_library_and_table(lib):
    src = open(os.path.join(ROOT, "include", "dynavsr_hip.h")).read()
    assert re.search(r"#define\s+DVSR_FLIP_W\s+1\b", src) and re.search(r"#define\s+DVSR_FLIP_H\s+2\b", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r" T (dvsr_[a-z0-9_]+)", out))
    sig = lib.lib()._signatures
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in exported, name
        assert name in sig and sig[name][0] is ctypes.c_int, name
    assert len(sig["dvsr_frame_flip"][1]) == 7 and len(sig["dvsr_frame_flip_mean"][1]) == 9
    assert (lib.FLIP_W, lib.FLIP_H) == (ref.FLIP_W, ref.FLIP_H) == (1, 2)


def test_rejections_need_no_device(lib):
    """Every bad argument is DVSR_ERR_INVALID before any launch: the checks run here, where there is no GPU."""
    l = lib.lib()
    a, b, c, d, e = 4096, 8192, 12288, 16384, 20480           # never dereferenced
    assert l.dvsr_frame_flip(None, b, 1, 1, 4, 0, None) == -1 and b"null" in l.dvsr_last_error()
    assert l.dvsr_frame_flip(a, None, 1, 1, 4, 0, None) == -1
    for planes, H, W in ((0, 1, 4), (1, 0, 4), (1, 1, 0), (-1, 1, 4), (1, 1, 6), (1, 1, 2)):
        assert l.dvsr_frame_flip(a, b, planes, H, W, 1, None) == -1, (planes, H, W)
        assert l.dvsr_frame_flip_mean(a, b, c, d, e, planes, H, W, None) == -1, (planes, H, W)
    for flags in (-1, 4, 7):
        assert l.dvsr_frame_flip(a, b, 1, 1, 4, flags, None) == -1 and b"flags" in l.dvsr_last_error()
    assert l.dvsr_frame_flip(a + 4, b, 1, 1, 4, 1, None) == -1 and b"misaligned" in l.dvsr_last_error()
    assert l.dvsr_frame_flip(a, b + 8, 1, 1, 4, 1, None) == -1 and b"misaligned" in l.dvsr_last_error()
    assert l.dvsr_frame_flip(a, a, 1, 1, 4, 1, None) == -1 and b"in place" in l.dvsr_last_error()
    ptrs = [a, b, c, d, e]
    for i in range(5):
        p = list(ptrs)
        p[i] = None
        assert l.dvsr_frame_flip_mean(*p, 1, 1, 4, None) == -1 and b"null" in l.dvsr_last_error()
        p[i] = ptrs[i] + 4
        assert l.dvsr_frame_flip_mean(*p, 1, 1, 4, None) == -1 and b"misaligned" in l.dvsr_last_error()
    for i in range(4):
        p = list(ptrs)
        p[4] = ptrs[i]
        assert l.dvsr_frame_flip_mean(*p, 1, 1, 4, None) == -1 and b"in place" in l.dvsr_last_error()
