"""GPU: dvsr_frame_degrade -- a ground-truth frame degraded from the form it arrives in -- and what stands on it:
frames.degrade, video.degrade_frames, video.evaluate_degraded, adapt.evaluate_degraded.

The entry's contract is bit identity with the composition it replaces, Degradation.apply on the crop of frames.ingest's output,
with the quantiser on and off; against the CPU oracle it holds the bar of tests/test_gpu_degradation.py (2e-6 on [0,1] data) and,
quantised, the oracle's 8-bit level wherever the oracle is not within TIE_BAND of a rounding tie (tests/test_frame_degrade_host.py
holds that this leaves out no more than 2 % of these inputs).  End to end: EDVR-M x4 + MFDN with synthetic weights, T = 7."""
import numpy as np
import pytest
import torch

from dynavsr_amd import frames as fio
from dynavsr_amd import video
from test_frame_degrade_host import ORACLE_CASES, degradation, hr_u8, oracle_lr, outside_tie_band

pytestmark = pytest.mark.gpu
QUANTISE = [False, True]


def composition(x, d, quantise, layout=None):
    """What dvsr_frame_degrade must reproduce bit for bit."""
    K, s = fio.degradation_edge(d)
    _, h, w = fio.resolve_layout(x, layout)
    Hc, Wc = fio.degraded_size(h, w, K, s)[:2]
    return d.apply(fio.ingest(x, layout, multiple=1)[:, :Hc, :Wc].contiguous()[None], quantise)[0]


def u8(seed, h, w, c=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (h, w, c), dtype=torch.uint8, generator=g)


@pytest.mark.parametrize("quantise", QUANTISE)
@pytest.mark.parametrize("h,w,scale,ks,lr_size", [
    (50, 71, 4, 21, (12, 17)),       # ragged against the 32 x 16 tile, h % s and w % s != 0
    (16, 16, 4, 21, (4, 4)),         # the smallest frame a pad of 13 allows: reflection on every side of every tap row
    (47, 100, 3, 21, (15, 33)),      # 33 wide: crosses a tile edge
    (37, 41, 4, 13, (9, 10)),        # K = 19: the generic kernel
    (144, 272, 4, 21, (36, 68)),     # 3 x 3 tiles
])
def test_rgb_bytes_are_the_composition(h, w, scale, ks, lr_size, quantise):
    d = degradation(ks, scale)
    x = u8(h * w, h, w).cuda()
    y = fio.degrade(x, d, quantise=quantise)
    assert y.dtype == torch.float32 and tuple(y.shape) == (3,) + lr_size and y.is_contiguous()
    assert torch.equal(y, composition(x, d, quantise))
    assert torch.equal(fio.degrade(x.cpu(), d, quantise=quantise), y)         # a CPU frame: the same bytes, copied first


@pytest.mark.parametrize("quantise", QUANTISE)
def test_generic_kernel_by_switch(monkeypatch, quantise):
    """DVSR_DEGRADE_GENERIC is read on every call and selects the generic kernel here as in dvsr_degrade_apply: the identity holds
    under it, for a shape that takes the phase-plane kernel otherwise."""
    d = degradation(21, 4)
    x = u8(7, 50, 71).cuda()
    tiled = fio.degrade(x, d, quantise=quantise)
    monkeypatch.setenv("DVSR_DEGRADE_GENERIC", "1")
    y = fio.degrade(x, d, quantise=quantise)
    assert torch.equal(y, composition(x, d, quantise))
    monkeypatch.delenv("DVSR_DEGRADE_GENERIC")
    # the two kernels walk the taps in different orders: each is within 2e-6 of the exact sum (the bar of
    # tests/test_gpu_degradation.py), so they are within 4e-6 of each other, and one level apart at most where quantised
    assert float((y - tiled).abs().max()) <= (1.0 / 255 + 1e-7 if quantise else 4e-6)


@pytest.mark.parametrize("quantise", QUANTISE)
def test_bgr_pixel_stride_4_offset_pitched_view(quantise):
    d = degradation(21, 2)                                                    # K = 25, J = 13
    buf = u8(11, 52, 80, 4).cuda()
    x = buf[3:48, 5:75, :3]                                                   # a 70 x 45 frame: [45,70,3], strides (320, 4, 1)
    assert x.stride() == (320, 4, 1) and x.data_ptr() % 4 == 0
    y = fio.degrade(x, d, 'hwc_bgr', quantise=quantise)
    assert tuple(y.shape) == (3, 22, 35)
    assert torch.equal(y, composition(x, d, quantise, 'hwc_bgr'))
    assert torch.equal(y, composition(x.contiguous(), d, quantise, 'hwc_bgr'))
    assert torch.equal(y.flip(0), fio.degrade(x, d, 'hwc_rgb', quantise=quantise))           # BGR is RGB with the planes swapped
    odd = buf[3:48, 5:75, 1:4]                                                # the same view one byte on: no address is aligned
    assert torch.equal(fio.degrade(odd, d, quantise=quantise), composition(odd.contiguous(), d, quantise))


@pytest.mark.parametrize("quantise", QUANTISE)
def test_float_view_and_strided_destination(quantise):
    d = degradation(21, 4)
    base = torch.rand(3, 64, 96, generator=torch.Generator().manual_seed(5)).cuda()
    x = base[:, 2:62, 4:92]                                                   # [3,60,88], row stride 96
    y = fio.degrade(x, d, quantise=quantise)
    assert tuple(y.shape) == (3, 15, 22)
    assert torch.equal(y, composition(x, d, quantise))
    # a destination that is a view: rows of 24 floats for 17 columns, planes of 14 rows for 12
    xb = u8(3, 50, 71).cuda()
    want = composition(xb, d, quantise)
    big = torch.full((3, 14, 24), -7.0, device="cuda")
    out = big[:, 1:13, 3:20]
    assert fio.degrade(xb, d, quantise=quantise, out=out) is out
    assert torch.equal(out, want)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:, 1:13, 3:20] = False
    assert bool((big[mask] == -7.0).all())                                    # nothing between the rows or planes is touched
    with pytest.raises(ValueError, match="out must"):
        fio.degrade(xb, d, out=torch.empty(3, 12, 34, device="cuda")[:, :, ::2])


@pytest.mark.parametrize("quantise", QUANTISE)
def test_nv12_goes_through_ingest(quantise):
    d = degradation(21, 4)
    g = torch.Generator().manual_seed(9)
    x = torch.randint(16, 236, (72, 64), dtype=torch.uint8, generator=g)      # 48 x 64: 48 rows Y, 24 rows CbCr
    y = fio.degrade(x, d, 'nv12', quantise=quantise)
    assert tuple(y.shape) == (3, 12, 16)
    assert torch.equal(y, composition(x.cuda(), d, quantise, 'nv12'))
    y709 = fio.degrade(x, d, 'nv12', quantise=quantise, matrix='bt709', yuv_range='full')
    full = fio.ingest(x, 'nv12', multiple=1, matrix='bt709', yuv_range='full')
    assert torch.equal(y709, d.apply(full[:, :48, :64].contiguous()[None], quantise)[0])


def test_per_frame_kernels():
    from dynavsr_amd.data.random_kernel_generator import Degradation
    d = degradation(21, 4)
    d.set_kernel_directly(np.stack([Degradation(21, 4, theta=0.3 * j, sigma=[1.0 + 0.4 * j, 2.4 - 0.3 * j]).kernel for j in range(5)]))
    hr = torch.stack([u8(20 + j, 50, 71) for j in range(5)])
    lr = video.degrade_frames(hr, d)
    assert tuple(lr.shape) == (5, 3, 12, 17)
    for j in range(5):
        assert torch.equal(lr[j], fio.degrade(hr[j], d, kernel_index=j))
    assert not torch.equal(lr[1], fio.degrade(hr[1], d, kernel_index=2))
    # ... which is Degradation.apply with one kernel per frame on the ingested crops
    clip = torch.stack([fio.ingest(f, multiple=1)[:, :48, :68] for f in hr]).contiguous()
    assert torch.equal(lr, d.apply(clip, quantise=True))
    out = torch.empty(5, 3, 12, 17, device="cuda")
    assert video.degrade_frames(list(hr.cuda()), d, quantise=False, out=out) is out
    assert torch.equal(out, d.apply(clip))


@pytest.mark.parametrize("h,w,scale,ks", ORACLE_CASES)
def test_against_the_cpu_oracle(h, w, scale, ks):
    d = degradation(ks, scale)
    x = hr_u8(h + w, h, w)
    want = oracle_lr(x, d)
    y = fio.degrade(x, d, quantise=False).cpu().numpy()
    err = float(np.abs(y - want).max())
    print("unquantised: max abs %.3e" % err)
    assert y.shape == want.shape and err < 2e-6
    q = fio.degrade(x, d, quantise=True).cpu().numpy().astype(np.float64) * 255
    assert float(np.abs(q - np.rint(q)).max()) < 1e-4                         # on the 8-bit grid ...
    assert q.min() >= -1e-4 and q.max() <= 255 + 1e-4
    compared = outside_tie_band(want)
    levels = np.rint(np.clip(255.0 * want.astype(np.float64), 0, 255))
    print("quantised: %d of %d compared, %d differ" % (compared.sum(), compared.size, (np.rint(q) != levels)[compared].sum()))
    assert 1.0 - float(compared.mean()) <= 0.02
    assert np.array_equal(np.rint(q)[compared], levels[compared])             # ... and on the oracle's level off the ties
    assert float(np.abs(np.rint(q) - levels).max()) <= 1                      # a tie goes to a neighbouring level, no further


# ---- end to end: EDVR-M x4 with synthetic weights ------------------------------------------------------------------------

T = 7


@pytest.fixture(scope="module")
def nets():
    from test_gpu_adapt_frames import _nets, _opt
    opt = _opt()
    return opt, _nets(opt)


@pytest.fixture(scope="module")
def hr_video():
    """uint8 [7,122,179,3] on the CPU: LR frames of 30 x 44, ground truth 120 x 176."""
    return torch.stack([hr_u8(40 + t, 122, 179) for t in range(T)])


def test_cpu_frames_equal_gpu_frames(hr_video):
    d = degradation(21, 4)
    lr = video.degrade_frames(hr_video, d)
    assert tuple(lr.shape) == (T, 3, 30, 44) and lr.is_cuda
    assert torch.equal(lr, video.degrade_frames(hr_video.cuda(), d))
    assert torch.equal(lr, video.degrade_frames([f for f in hr_video], d))
    assert torch.equal(lr[3], composition(hr_video[3].cuda(), d, True))
    assert torch.equal(video.degrade_frames(hr_video, d, quantise=False)[3], composition(hr_video[3].cuda(), d, False))


@pytest.mark.parametrize("kw", [{}, {"out": "hwc_rgb"}, {"cuts": [4]}], ids=["plain", "hwc_rgb", "cuts"])
def test_evaluate_degraded_is_evaluate_frames_on_the_degraded_video(nets, hr_video, kw):
    opt, (model, *_) = nets
    net = model.netG
    d = degradation(21, 4)
    lr = video.degrade_frames(hr_video, d)
    gt = [f[:120, :176] for f in hr_video]                                     # cut by hand
    want_summary, want_scores = video.evaluate_frames(opt, net, lr, gt, gt_layout="hwc_rgb", **kw)
    summary, scores = video.evaluate_degraded(opt, net, hr_video, d, **kw)
    assert tuple(scores.shape) == (T, 2) and scores.dtype == torch.float64 and scores.is_cuda
    assert torch.equal(scores, want_scores)
    assert bool((scores[:, 0] > 0).all()) and bool(torch.isfinite(scores).all())
    np.testing.assert_equal(summary, want_summary)                             # (NaN == NaN: a scene without centre frames)
    assert len(summary["scenes"]) == (2 if "cuts" in kw else 1)


def test_adapt_evaluate_degraded(nets, hr_video, monkeypatch):
    """The LR video and ground truth that reach adapt_frames are degrade_frames' and the hand-cut views; the returned rows are
    frames.score of the frames adapt_frames yielded; the summaries and gain_db are score_summary's.  Against a second run of
    adapt_frames on that LR video: the baseline rows bit for bit (forward only), the adapted rows at the two-run bar of
    tests/test_gpu_adapt_frames.py -- frames 1e-5 apart move at most 2 * 255 * 1e-5 = 0.5 % of the 8-bit values to a
    neighbouring level, each by at most 2 * 255 + 1 in its squared error: 2.6 in the MSE."""
    from dynavsr_amd import adapt
    opt, five = nets
    d = degradation(21, 4)
    seen = {}
    real = adapt.adapt_frames

    def recording(opt_, *args, **kw):
        seen["lr"], seen["kw"], seen["pairs"] = args[5], kw, []
        for b, a in real(opt_, *args, **kw):
            seen["pairs"].append((b.clone(), a.clone()))
            yield b, a
    monkeypatch.setattr(adapt, "adapt_frames", recording)
    r = adapt.evaluate_degraded(opt, *five, hr_video, d)
    monkeypatch.setattr(adapt, "adapt_frames", real)
    lr = video.degrade_frames(hr_video, d)
    assert torch.equal(seen["lr"], lr)
    gt = [f[:120, :176] for f in hr_video]
    assert len(seen["kw"]["gt"]) == T and all(torch.equal(a, b) for a, b in zip(seen["kw"]["gt"], gt))
    assert seen["kw"]["scores"] is r["scores"] and seen["kw"]["baseline_scores"] is r["baseline_scores"]
    assert len(seen["pairs"]) == T
    for i, (b, a) in enumerate(seen["pairs"]):
        assert tuple(a.shape) == (1, 3, 120, 176)
        assert torch.equal(r["baseline_scores"][i], fio.score(b[0], gt[i], "chw", "hwc_rgb"))
        assert torch.equal(r["scores"][i], fio.score(a[0], gt[i], "chw", "hwc_rgb"))
    n = int(opt["network_G"]["nframes"])
    np.testing.assert_equal(r["baseline"], video.score_summary(r["baseline_scores"], n))
    np.testing.assert_equal(r["adapted"], video.score_summary(r["scores"], n))
    assert r["gain_db"] == r["adapted"]["mean"]["psnr"] - r["baseline"]["mean"]["psnr"]
    assert np.isfinite(r["gain_db"])
    scores = torch.zeros(T, 2, dtype=torch.float64, device="cuda")
    bscores = torch.zeros(T, 2, dtype=torch.float64, device="cuda")
    for _ in adapt.adapt_frames(opt, *five, lr, gt=gt, gt_layout="hwc_rgb", scores=scores, baseline_scores=bscores):
        pass
    print("gain %.4f dB; adapted mse, two runs: %s" % (r["gain_db"], (scores[:, 0] - r["scores"][:, 0]).abs().tolist()))
    assert torch.equal(bscores, r["baseline_scores"])
    assert float((scores[:, 0] - r["scores"][:, 0]).abs().max()) <= 2.6
