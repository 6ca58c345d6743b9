"""CPU: the definition behind dvsr_frame_imresize -- MATLAB's bicubic imresize as a folded table -- against its
float64 restatement (tests/imresize_ref.py) and against what the reference's calculate_weights_indices / imresize recorded
(tests/golden/imresize_reference.npz, tools/gen_imresize_golden.py); every refusal ahead of a device; modcrop; and the old kernel
generator's host side against the reference's recorded kernels (tests/golden/old_kernel_reference.npz)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imresize_ref as R  # noqa: E402

from dynavsr_amd import _lib as L  # noqa: E402
from dynavsr_amd import frames, video  # noqa: E402
from dynavsr_amd.data import old_kernel_generator as old  # noqa: E402
from dynavsr_amd.data import util as dutil  # noqa: E402

CASES = ("q_37x50", "t_27x33", "h_24x40", "x4_9x13", "x2_12x10")
LONGEST = {(1, 2): 8, (1, 3): 11, (1, 4): 16, (2, 1): 4, (3, 1): 4, (4, 1): 4}       # antialiased; what the header promises
# tools/gen_imresize_golden.py printed, when it recorded the fixtures, the largest deviation of the reference's own fp32
# evaluation from the same rule in float64: 6.538e-08 for the folded weights of calculate_weights_indices, 2.267e-08 for the
# kernels of old_kernel_generator.  The bars are four times those.
WEIGHT_DEV, KERNEL_DEV = 6.538e-08, 2.267e-08


@pytest.fixture(scope="module")
def rec(golden):
    return golden("imresize_reference")


@pytest.fixture(scope="module")
def rec_old(golden):
    return golden("old_kernel_reference")


@pytest.mark.parametrize("num,den", R.SCALES)
@pytest.mark.parametrize("antialiasing", [True, False])
def test_table_is_the_restatement(num, den, antialiasing):
    for n_in in list(range(1, 41)) + [1080]:
        first, weights = frames.imresize_table(n_in, num / den, antialiasing)
        rf, rw = R.axis_table(n_in, num, den, antialiasing)
        assert first.dtype == torch.int32 and weights.dtype == torch.float32
        assert np.array_equal(first.numpy(), rf), (n_in, num, den)
        assert np.array_equal(weights.numpy(), rw), (n_in, num, den)          # equal in fp32, the zero padding included
        assert frames.imresize_size(n_in, n_in, num / den) == (R.n_out(n_in, num, den),) * 2 == (first.shape[0],) * 2


@pytest.mark.parametrize("num,den", R.SCALES)
@pytest.mark.parametrize("antialiasing", [True, False])
def test_windows_are_contiguous_and_bounded(num, den, antialiasing):
    lib = L.lib()
    worst = 0
    for n_in in list(range(1, 41)) + [1080]:
        n_out = ctypes.c_int()
        taps = lib.dvsr_frame_imresize_taps(n_in, num, den, int(antialiasing), ctypes.byref(n_out))
        first, weights = (t.numpy() for t in frames.imresize_table(n_in, (num, den), antialiasing))
        assert n_out.value == first.shape[0] and taps == weights.shape[1]
        longest, rule = 0, R.axis_rows(n_in, num, den, antialiasing)
        for i in range(n_out.value):
            nz = np.flatnonzero(weights[i])
            assert nz.size and nz[0] == 0, (n_in, i)                          # the window starts on its first tap ...
            assert 0 <= first[i] and first[i] + nz[-1] < n_in, (n_in, i)      # ... lies in the image ...
            longest = max(longest, int(nz[-1]) + 1)
            # ... and holds every folded tap of the rule: nothing lies outside [first, first + taps)
            f64, w64 = rule[i]
            assert f64 == first[i] and len(w64) <= taps
            assert abs(float(weights[i].astype(np.float64).sum()) - 1.0) < 1e-6
        assert longest == taps                                               # no longer than the entry says, and no shorter
        worst = max(worst, taps)
    if antialiasing:
        assert worst == LONGEST[(num, den)]
    assert worst <= 18


@pytest.mark.parametrize("name", CASES)
def test_table_against_the_recorded_weights(rec, name):
    num, den = (int(v) for v in rec[name + "_scale"])
    _, h, w = rec[name + "_in"].shape
    for axis, n_in in (("h", h), ("w", w)):
        wt, idx, sym = rec["%s_%s_weights" % (name, axis)], rec["%s_%s_indices" % (name, axis)], rec["%s_%s_sym" % (name, axis)]
        assert float(rec["%s_%s_dev" % (name, axis)]) <= WEIGHT_DEV
        assert wt.shape[0] == R.n_out(n_in, num, den) == rec[name + "_out"].shape[1 if axis == "h" else 2]
        ref = R.fold_reference(wt, idx, sym[0], n_in)
        first, weights = (t.numpy() for t in frames.imresize_table(n_in, num / den))
        mine = np.zeros_like(ref)
        for i in range(first.shape[0]):
            mine[i, first[i]:first[i] + weights.shape[1]] = weights[i][:n_in - first[i]]
        dev = float(np.abs(mine - ref).max())
        print("%s %s: |table - recorded, folded| max %.3e (bar %.3e)" % (name, axis, dev, 4 * WEIGHT_DEV))
        assert dev <= 4 * WEIGHT_DEV


@pytest.mark.parametrize("name", CASES)
def test_restatement_against_the_recorded_images(rec, name):
    num, den = (int(v) for v in rec[name + "_scale"])
    x = rec[name + "_in"].astype(np.float32) / np.float32(255.0)
    y = R.imresize(x, num, den)
    assert y.shape == rec[name + "_out"].shape
    dev = float(np.abs(y - rec[name + "_out"].astype(np.float64)).max())
    print("%s: |restatement - reference| max %.3e" % (name, dev))
    assert dev < 2e-6


def test_c_refusals():
    lib = L.lib()
    n_out = ctypes.c_int()
    for num, den in ((1, 1), (1, 5), (5, 1), (2, 3), (0, 1), (1, 0), (-1, 2), (2, 2)):
        assert lib.dvsr_frame_imresize_taps(8, num, den, 1, ctypes.byref(n_out)) == -2
    assert lib.dvsr_frame_imresize_taps(0, 1, 4, 1, ctypes.byref(n_out)) == -1
    assert lib.dvsr_frame_imresize_taps(1, 1, 4, 1, None) == 1                         # n_out may be null; any n_in >= 1
    first, weights = (ctypes.c_int * 16)(), (ctypes.c_float * (16 * 18))()
    assert lib.dvsr_frame_imresize_table(37, 1, 4, 1, 16, None, weights) == -1
    assert lib.dvsr_frame_imresize_table(37, 1, 4, 1, 16, first, None) == -1
    assert lib.dvsr_frame_imresize_table(37, 1, 4, 1, 15, first, weights) == -1          # shorter than the longest window
    assert lib.dvsr_frame_imresize_table(37, 1, 4, 1, 19, first, weights) == -1
    assert lib.dvsr_frame_imresize_table(37, 1, 5, 1, 16, first, weights) == -2
    assert lib.dvsr_frame_imresize_table(0, 1, 4, 1, 16, first, weights) == -1
    assert lib.dvsr_frame_imresize_table(37, 1, 4, 1, 18, first, weights) == 0

    # dvsr_frame_imresize: every refusal returns before a launch (the pointers are never followed: there is no device here)
    def call(src=0x1000, fmt=L.FRAME_U8_HWC_RGB, fh=40, fw=52, row=52 * 3, plane=0, px=3, h=37, w=50, num=1, den=4, dst=0x2000,
             drow=13, dplane=130, oh=10, ow=13, rows=(0x3000, 0x4000, 16), cols=(0x5000, 0x6000, 16), desc=True):
        d = L.FrameDesc(fmt, fh, fw, row, plane, px)
        r = L.ResizeAxis(*rows) if rows is not None else None
        c = L.ResizeAxis(*cols) if cols is not None else None
        return lib.dvsr_frame_imresize(src, ctypes.byref(d) if desc else None, h, w, num, den, 1, dst, drow, dplane, oh, ow,
                                       ctypes.byref(r) if r is not None else None, ctypes.byref(c) if c is not None else None, 1,
                                       None)
    for kw in (dict(src=None), dict(dst=None), dict(desc=False), dict(rows=None), dict(cols=None),
               dict(rows=(None, 0x4000, 16)), dict(cols=(0x5000, None, 16)),
               dict(fmt=7), dict(px=2), dict(px=5), dict(row=52 * 3 - 1),
               dict(h=41), dict(w=53), dict(h=0), dict(w=0),                               # a crop beyond the frame
               dict(oh=9), dict(ow=12), dict(oh=11),                                       # not the definition's
               dict(rows=(0x3000, 0x4000, 15)), dict(cols=(0x5000, 0x6000, 19)),           # taps outside [longest, 18]
               dict(drow=12), dict(dplane=129),                                            # a short row; planes that overlap
               dict(dst=0x2002), dict(rows=(0x3002, 0x4000, 16)), dict(cols=(0x5000, 0x6001, 16)),
               dict(fmt=L.FRAME_F32_CHW, row=52, plane=52 * 40, src=0x1002),               # a misaligned fp32 source
               dict(fmt=L.FRAME_F32_CHW, row=51, plane=52 * 40), dict(fmt=L.FRAME_F32_CHW, row=52, plane=52 * 39)):
        assert call(**kw) == -1, kw
    for kw in (dict(num=1, den=5), dict(num=3, den=2), dict(num=1, den=1)):
        assert call(**kw) == -2, kw
    assert b"scale" in lib.dvsr_last_error()


def test_python_refusals():
    for scale in (1, 0.2, 5, 0.25 + 1e-6, 1.5, "4", None, True, (1, 5)):
        with pytest.raises(ValueError):
            frames.imresize_ratio(scale)
        with pytest.raises(ValueError):
            frames.imresize_table(8, scale)
        with pytest.raises(ValueError):
            frames.imresize_size(8, 8, scale)
    assert frames.imresize_ratio(1 / 3 + 5e-10) == (1, 3) and frames.imresize_ratio(4) == (4, 1)
    assert frames.imresize_size(37, 50, 0.25) == (10, 13) and frames.imresize_size(11, 9, 3) == (33, 27)
    for bad in ((0, 8), (8, 0)):
        with pytest.raises(ValueError):
            frames.imresize_size(bad[0], bad[1], 2)
    with pytest.raises(ValueError):
        frames.imresize_table(0, 2)
    u8 = torch.zeros((8, 12, 3), dtype=torch.uint8)
    for kw in (dict(scale=1.5), dict(layout='chw'), dict(layout='nope'), dict(modcrop=0), dict(modcrop=2.0), dict(modcrop=16),
               dict(matrix='bt2020'), dict(yuv_range='tv'), dict(out=torch.zeros((3, 2, 3))), dict(out=torch.zeros((3, 2, 4))),
               dict(out=torch.zeros((3, 2, 3), dtype=torch.float64)), dict(out=torch.zeros((3, 3, 2)).transpose(1, 2))):
        kw = dict(dict(scale=0.25), **kw)
        scale = kw.pop('scale')
        with pytest.raises((ValueError, RuntimeError)) as e:
            frames.imresize(u8, scale, **kw)
        assert "libdynavsr_hip" in str(e.value) or isinstance(e.value, ValueError), kw    # (a CPU `out` of the right kind)
    with pytest.raises(ValueError):
        frames.imresize(torch.zeros((3, 8, 12), dtype=torch.int32), 2)
    for scale in (1, 5, 2.0, 0.25, "4", True):
        with pytest.raises(ValueError):
            frames.Imresize(scale)
    bi = frames.Imresize(4)
    assert (bi.scale, bi.antialiasing) == (4, True) and bi.lr_size(37, 50) == (36, 48, 9, 12)
    with pytest.raises(ValueError):
        bi.lr_size(3, 50)
    with pytest.raises(ValueError):
        frames.degrade(u8, bi, kernel_index=1)
    for f in (dutil.imresize, dutil.imresize_np):
        x = torch.zeros((3, 8, 8)) if f is dutil.imresize else np.zeros((8, 8, 3), dtype=np.float32)
        for scale in (1.5, 0.2, 1, 0.25 + 1e-6):
            with pytest.raises(ValueError):
                f(x, scale)
    with pytest.raises(ValueError):
        dutil.imresize(torch.zeros((8, 8, 3)), 0.25)
    with pytest.raises(ValueError):
        dutil.imresize_np(np.zeros((3, 8, 9), dtype=np.float32), 0.25)
    with pytest.raises(ValueError):
        dutil.imresize_np(np.zeros((8, 8, 3), dtype=np.uint8), 0.25)


def test_modcrop():
    r = np.random.RandomState(0)
    for shape in ((37, 50, 3), (37, 50), (36, 48, 3)):
        img = r.randint(0, 256, shape).astype(np.uint8)
        got = dutil.modcrop(img, 4)
        assert got.shape[:2] == (36, 48) and np.array_equal(got, img[:36, :48])
        assert not np.shares_memory(got, img) and got.flags['C_CONTIGUOUS'] and got.flags['OWNDATA']
    with pytest.raises(ValueError):
        dutil.modcrop(np.zeros((2, 3, 4, 5)), 2)


def test_evaluate_degraded_checks_the_scale_of_an_imresize():
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    net = EDVR()
    opt = {"scale": 4, "network_G": {"which_model_G": "EDVR", "nframes": 5}}
    hr = torch.zeros((5, 64, 96, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="is not opt"):
        video.evaluate_degraded(opt, net, hr, frames.Imresize(2))
    with pytest.raises(ValueError, match="gt"):
        video.evaluate_degraded(opt, net, hr, frames.Imresize(4), gt=hr)
    with pytest.raises(ValueError, match="no multiple"):
        video.degrade_frames(torch.zeros((5, 3, 96, 3), dtype=torch.uint8), frames.Imresize(4))
    with pytest.raises(ValueError):
        video.evaluate_bicubic({"scale": 1}, net, torch.zeros((5, 3, 16, 24)), torch.zeros((5, 3, 16, 24)))
    with pytest.raises(ValueError):
        video.evaluate_bicubic(opt, net, torch.zeros((5, 3, 16, 24)), torch.zeros((4, 3, 64, 96)))      # gt of another length
    with pytest.raises(ValueError):
        video.evaluate_bicubic(opt, net, torch.zeros((5, 3, 16, 24)), torch.zeros((5, 3, 64, 95)))      # gt of another size
    with pytest.raises(ValueError):
        video.evaluate_bicubic(opt, net, torch.zeros((5, 3, 16, 24)), None)


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("kind", [0.0, 0.7])
def test_old_generator_kernels(rec_old, scale, kind):
    for i in range(3):
        key = "s%d_t%.1f_%d" % (scale, kind, i)
        sx, sy, theta = (float(v) for v in rec_old[key + "_params"])
        assert float(rec_old[key + "_dev"]) <= KERNEL_DEV
        d = old.Degradation(21, scale, type=kind, theta=theta, sigma=[sx, sy])
        k = d.get_kernel()
        assert k.shape == (21, 21) and k.dtype == np.float64 and d.kernel is k
        dev = float(np.abs(k - rec_old[key + "_kernel"].astype(np.float64)).max())
        print("%s: |kernel - recorded| max %.3e (bar %.3e)" % (key, dev, 4 * KERNEL_DEV))
        assert dev <= 4 * KERNEL_DEV
        assert abs(k.sum() - 1.0) < 1e-12
        assert d.shifted_edge() == 21 == d.kernel_size and d.scale == scale
        assert np.array_equal(d.get_features(), k.reshape(-1))
        assert frames.degradation_edge(d) == (21, scale)
        assert frames.degraded_size(38, 54, d.shifted_edge(), scale) == (38 - 38 % scale, 54 - 54 % scale, 38 // scale, 54 // scale)
    for bad in (dict(kernel_size=21, scale_factor=3), dict(kernel_size=20, scale_factor=2), dict(kernel_size=23, scale_factor=2)):
        with pytest.raises(ValueError):
            old.Degradation(**bad)
    d = old.Degradation(21, 2)
    with pytest.raises(RuntimeError):
        d.apply(torch.zeros((3, 24, 32)))
