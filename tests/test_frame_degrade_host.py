"""CPU: the host side of degrading a ground-truth video on the device -- frames.degraded_size, Degradation.shifted_edge, the
argument checks of dvsr_frame_degrade (which return before any launch, so pointers that nothing reads will do), the ValueErrors
of video.degrade_frames / video.evaluate_degraded / adapt.evaluate_degraded ahead of their first GPU call, and the tie-band
condition of the quantised oracle test in tests/test_gpu_frame_degrade.py, which takes its inputs from here."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from dynavsr_amd import adapt, frames, video
from dynavsr_amd.data.random_kernel_generator import Degradation

INVALID, UNSUPPORTED = -1, -2
A16 = 0x10000           # a 16-byte aligned address that nothing reads
THETA, SIGMA = 0.4, [2.0, 0.8]
TIE_BAND = 2e-3         # in 8-bit levels: four times the 5e-4 that the 2e-6 bar of the unquantised comparison allows
# (h, w, scale, kernel_size) of the oracle comparisons: ragged against the tile with h % s and w % s != 0; 3 x 3 tiles; scale 3
ORACLE_CASES = [(50, 71, 4, 21), (144, 272, 4, 21), (47, 100, 3, 21)]


def degradation(ks, scale):
    return Degradation(ks, scale, theta=THETA, sigma=SIGMA)


def hr_u8(seed, h, w):
    """A uint8 [h,w,3] RGB frame on the CPU: smooth structure over the whole range plus noise, as footage has it."""
    r = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    img = np.stack([127.5 + 110.0 * np.sin(xx / (7.3 + c) + seed + c) * np.cos(yy / (5.1 + 2 * c) - c) for c in range(3)], -1)
    img = img + r.randint(-24, 25, size=img.shape)
    return torch.from_numpy(np.clip(np.rint(img), 0, 255).astype(np.uint8))


def oracle_lr(x, d):
    """The unquantised CPU oracle of degrading the uint8 frame x with d: float32 [3,h_lr,w_lr] (accumulated in float64)."""
    from oracle import degradation as od
    s = int(d.scale)
    h, w = x.shape[0] - x.shape[0] % s, x.shape[1] - x.shape[1] % s
    img = (x[:h, :w].permute(2, 0, 1).numpy().astype(np.float32) / np.float32(255))[None]
    return od.apply(img, d.kernel, s)[0]


def outside_tie_band(y):
    """Where 255 y of the unquantised oracle lies more than TIE_BAND from a half-integer: there a result within 2e-6 of y has y's
    8-bit level."""
    v = 255.0 * y.astype(np.float64)
    return np.abs(v - np.floor(v) - 0.5) > TIE_BAND


@pytest.fixture(scope="module")
def lib():
    from dynavsr_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        from dynavsr_amd import build
        build.build()
    return _lib


def test_degraded_size():
    assert frames.degraded_size(50, 71, 27, 4) == (48, 68, 12, 17)
    assert frames.degraded_size(47, 100, 25, 3) == (45, 99, 15, 33)
    assert frames.degraded_size(16, 16, 27, 4) == (16, 16, 4, 4)          # the smallest frame a pad of 13 allows ...
    assert frames.degraded_size(40, 40, 16, 2) == (40, 40, 21, 21)        # an even K: one more than Hc / scale
    assert frames.degraded_size(720, 1280, 27, 4) == (720, 1280, 180, 320)
    for bad in ((15, 40, 27, 4), (40, 15, 27, 4),                         # ... and a pad that is not smaller than the crop
                (13, 13, 27, 4), (3, 40, 1, 4), (40, 3, 1, 4),            # no multiple of the scale inside
                (40, 40, 35, 4), (40, 40, 0, 4), (40, 40, 27, 5), (40, 40, 27, 0)):
        with pytest.raises(ValueError):
            frames.degraded_size(*bad)


def test_shifted_kernel_edges():
    """The edges the GPU tests rely on: (4, 27), (2, 25) and (3, 25) take the phase-plane kernels -- ceil(K / scale) = 7, 13, 9 --
    and (4, 19) the generic one.  shifted_edge() is the arithmetic of kernel_shift without the spline."""
    for ks, scale, K in ((21, 4, 27), (21, 2, 25), (21, 3, 25), (13, 4, 19), (10, 2, 16)):
        d = degradation(ks, scale)
        assert d.shifted_edge() == K
        assert tuple(d._shifted_on("cpu").shape) == (1, K, K)
        assert frames.degradation_edge(d) == (K, scale)
    d = degradation(21, 4)
    d.set_kernel_directly(np.stack([degradation(21, 4).kernel, Degradation(21, 4, theta=1.0, sigma=[1.0, 3.0]).kernel]))
    assert [d.shifted_edge(j) for j in range(2)] == [27, 27] and tuple(d._shifted_on("cpu").shape) == (2, 27, 27)
    for bad in (2, -1, True, 0.0):
        with pytest.raises(ValueError):
            frames.degradation_edge(d, bad)


def _desc(lib, fmt=1, h=50, w=71, row=None, plane=0, ps=3):
    if row is None:
        row = w * ps if fmt else w
    if fmt == 0 and plane == 0:
        plane = h * row
    return lib.FrameDesc(fmt, h, w, row, plane, ps)


def test_frame_degrade_bad_arguments_without_gpu(lib):
    l = lib.lib()

    def degrade(src=A16 + 1, d=None, kernel=A16, K=27, scale=4, dst=A16, row=17, plane=12 * 17, null_desc=False):
        d = d if d is not None else _desc(lib)
        return l.dvsr_frame_degrade(src, None if null_desc else ctypes.byref(d), kernel, K, scale, dst, row, plane, 1, None)

    cases = [
        (dict(src=None), INVALID, b"null"),
        (dict(null_desc=True), INVALID, b"null"),
        (dict(kernel=None), INVALID, b"null"),
        (dict(dst=None), INVALID, b"null"),
        (dict(d=_desc(lib, fmt=3)), INVALID, b"format"),                  # a Y plane is no frame to degrade
        (dict(d=_desc(lib, fmt=-1)), INVALID, b"format"),
        (dict(d=_desc(lib, ps=2)), INVALID, b"pixel stride"),
        (dict(d=_desc(lib, ps=5)), INVALID, b"pixel stride"),
        (dict(d=_desc(lib, row=212)), INVALID, b"row stride"),
        (dict(d=_desc(lib, ps=4, row=283)), INVALID, b"row stride"),
        (dict(d=_desc(lib, fmt=0, row=70), src=A16), INVALID, b"row stride"),
        (dict(d=_desc(lib, fmt=0, plane=49 * 71 + 70), src=A16), INVALID, b"plane stride"),
        (dict(d=_desc(lib, h=0)), INVALID, b"frame size"),
        (dict(d=_desc(lib, h=3)), INVALID, b"no multiple"),                # Hc = 0
        (dict(d=_desc(lib, w=3)), INVALID, b"no multiple"),
        (dict(d=_desc(lib, h=15)), INVALID, b"reflection pad"),            # Hc = 12 <= 13
        (dict(d=_desc(lib, w=15)), INVALID, b"reflection pad"),
        (dict(K=35), UNSUPPORTED, b"kernel edge"),
        (dict(K=0), UNSUPPORTED, b"kernel edge"),
        (dict(scale=5), UNSUPPORTED, b"scale"),
        (dict(scale=0), UNSUPPORTED, b"scale"),
        (dict(row=16), INVALID, b"destination"),
        (dict(plane=11 * 17 + 16), INVALID, b"destination"),
        (dict(dst=A16 + 2), INVALID, b"misaligned"),
        (dict(kernel=A16 + 1), INVALID, b"misaligned"),
        (dict(d=_desc(lib, fmt=0), src=A16 + 2), INVALID, b"misaligned"),
    ]
    for kw, code, word in cases:
        assert degrade(**kw) == code, kw
        assert word in l.dvsr_last_error(), (kw, l.dvsr_last_error())


class _Mean(torch.nn.Module):
    nframes = 3
    scale = 4

    def forward(self, x):
        return x.mean(1)


def _adapt_opt():
    from dynavsr_amd.options import options as option
    opt = option.dict_to_nonedict(option.parse(os.path.join(
        ROOT, "dynavsr_amd", "options", "test", "EDVR", "EDVR_M_S4.yml"), is_train=False))
    opt["dist"] = False
    return opt


def _calls():
    """(name, f(hr, degradation, **kw)) for the three functions, on networks that live on the CPU: a call whose arguments
    pass gets as far as the first GPU call."""
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    net = EDVR()
    opt = {"scale": 4, "network_G": {"which_model_G": "EDVR", "nframes": 5}}
    aopt = _adapt_opt()
    return [("degrade_frames", lambda hr, d, **kw: video.degrade_frames(hr, d, **kw)),
            ("video.evaluate_degraded", lambda hr, d, **kw: video.evaluate_degraded(opt, net, hr, d, **kw)),
            ("adapt.evaluate_degraded", lambda hr, d, **kw: adapt.evaluate_degraded(aopt, None, None, None, None, None, hr, d, **kw))]


def test_checks_come_before_the_gpu():
    hr = torch.zeros(7, 122, 179, 3, dtype=torch.uint8)
    per_frame = degradation(21, 4)
    per_frame.set_kernel_directly(np.stack([per_frame.kernel] * 5))       # 5 kernels for 7 frames
    for name, f in _calls():
        with pytest.raises(ValueError, match="per-frame kernels"):
            f(hr, per_frame)
        with pytest.raises(ValueError, match="reflection pad"):            # pad 13 of a 12 x 176 crop
            f(hr[:, :13], degradation(21, 4))
        with pytest.raises(ValueError):
            f([], degradation(21, 4))
        with pytest.raises(ValueError):
            f(torch.zeros(7, 3, 122, 179, dtype=torch.uint8), degradation(21, 4))
        if name == "degrade_frames":
            with pytest.raises(ValueError, match="out must be"):
                f(hr, degradation(21, 4), out=torch.zeros(7, 3, 30, 45))
            continue
        with pytest.raises(ValueError, match="scale"):                     # the network is x4
            f(hr, degradation(21, 2))
        with pytest.raises(ValueError, match="even shifted kernel"):       # K = 28: LR frames of 31 x 45
            f(hr, degradation(20, 4))
        for kw in (dict(gt=hr), dict(gt_layout="hwc_rgb"), dict(layout="chw"),
                   dict(out="uint8"), dict(crop_border=-1), dict(score="luma"), dict(cuts=[9]), dict(padding="mirror"),
                   dict(scores=torch.zeros(7, 2, dtype=torch.float64)),     # not on the GPU
                   dict(hr_layout="nv12")):
            with pytest.raises(ValueError):
                f(hr, degradation(21, 4), **kw)
        # arguments that pass reach the device, which this machine does not have -- or the GPU call succeeds
        if not torch.cuda.is_available():
            with pytest.raises((RuntimeError, AssertionError)):
                f(hr, degradation(21, 4), cuts="auto")
    with pytest.raises(ValueError, match="baseline"):
        _calls()[2][1](hr, degradation(21, 4), baseline=False)


@pytest.mark.parametrize("h,w,scale,ks", ORACLE_CASES)
def test_tie_band_leaves_out_little(h, w, scale, ks):
    """The quantised GPU test compares 8-bit levels where the oracle is more than TIE_BAND away from a rounding tie; for its
    inputs that must leave out no more than 2 % of the outputs (0.4 % expected), or the test would check little."""
    d = degradation(ks, scale)
    y = oracle_lr(hr_u8(h + w, h, w), d)
    assert y.shape == (3,) + frames.degraded_size(h, w, d.shifted_edge(), scale)[2:]
    left_out = 1.0 - float(outside_tie_band(y).mean())
    print("left out: %.3f %% of %d" % (100 * left_out, y.size))
    assert left_out <= 0.02
    assert float(y.min()) < 0.2 and float(y.max()) > 0.8                     # the data spans the levels
