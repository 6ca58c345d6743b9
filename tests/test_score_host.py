"""CPU: the host side of frame scoring -- the Y8 integer rule over all 2^24 triples, the numpy restatement (score_ref.py) and the
new colour functions of data/util.py against what the reference recorded (tests/golden/score_reference.npz,
ycbcr_reference.npz), the separable float64 SSIM against the oracle's 2-D window, adapt.score_summary against hand-written
cases, and every argument error of frames.score, of the gt= arguments of adapt.super_resolve_frames and of dvsr_frame_score
without a device call."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import score_ref as ref
from dynavsr_amd import adapt, frames
from dynavsr_amd.data import util as dutil
from oracle import metrics as om

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_y8_over_all_triples():
    """Off the exact ties the integer rule is the rounded float64 formula; on them it is within one level; there are 194."""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    ties = 0
    for r in range(256):
        got = ref.y8(r, g, b)
        want = np.rint((65.481 * r + 128.553 * g + 24.966 * b) / 255.0 + 16.0).astype(np.int64)
        tie = ref.is_tie(r, g, b)
        ties += int(tie.sum())
        assert np.array_equal(got[~tie], want[~tie]), r
        assert np.abs(got[tie] - want[tie]).max(initial=0) <= 1, r
        assert (got[tie] % 2 == 0).all(), r                       # half to even
        assert got.min() >= 16 and got.max() <= 235
    assert ties == 194
    t = ref.tie_triples()
    assert t.shape == (194, 3) and ref.is_tie(t[:, 0], t[:, 1], t[:, 2]).all()


def test_colour_functions_reproduce_the_recorded_reference():
    g = np.load(os.path.join(GOLDEN, "ycbcr_reference.npz"))
    fns = {"rgb2ycbcr": lambda x: dutil.rgb2ycbcr(x, only_y=False), "bgr2ycbcr": lambda x: dutil.bgr2ycbcr(x, only_y=False),
           "ycbcr2rgb": dutil.ycbcr2rgb}
    for name, fn in fns.items():
        for kind in ("f64", "u8"):
            x = g["%s_%s_in" % (name, kind)]
            keep = x.copy()
            got = fn(x)
            assert np.array_equal(x, keep), (name, kind)           # the caller's array is not scaled in place
            want = g["%s_%s_out" % (name, kind)]
            assert got.dtype == want.dtype and got.shape == want.shape, (name, kind)
            if kind == "u8":
                assert np.array_equal(got, want), name
            else:
                assert np.abs(got - want).max() <= 1e-15, (name, float(np.abs(got - want).max()))
    s = np.load(os.path.join(GOLDEN, "score_reference.npz"))
    for order, fn in (("rgb", dutil.rgb2ycbcr), ("bgr", dutil.bgr2ycbcr)):
        u, want = s["y_%s_u8_in" % order], s["y_%s_u8_out" % order]
        got = fn(u)                                                # only_y=True is the default, as in the reference
        assert got.dtype == np.uint8 and np.array_equal(got, want), order
        rgb = u if order == "rgb" else u[:, :, ::-1]
        assert np.array_equal(ref.y8(rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2]), want), order
        assert np.array_equal(ref.samples(u, "hwc_" + order, "y")[:, :, 0], want), order
        f, want = s["y_%s_f32_in" % order], s["y_%s_f32_out" % order]
        keep = f.copy()
        got = fn(f)
        assert np.array_equal(f, keep) and got.dtype == np.float32 and np.array_equal(got, want), order
        # the evaluation scripts' chain on a float image: (Y * 255).round() is Y8 of the bytes
        u = np.rint(f.astype(np.float64) * 255).astype(np.uint8)
        rgb = u if order == "rgb" else u[:, :, ::-1]
        assert np.array_equal(ref.y8(rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2]), np.rint(want.astype(np.float64) * 255)), order


def test_crop_and_psnr_reproduce_the_recorded_reference():
    s = np.load(os.path.join(GOLDEN, "score_reference.npz"))
    a, b = s["psnr_a"], s["psnr_b"]
    assert math.isinf(float(s["psnr_same"])) and math.isinf(frames.psnr(0.0)) and math.isinf(ref.psnr(0))
    for k in s["psnr_crops"].tolist():
        assert np.array_equal(ref.crop(a, k), s["crop_k%d_a" % k])
        for channel in ("rgb", "y"):
            sse, n, mse, _ = ref.score(ref.samples(a, "hwc_rgb", channel), ref.samples(b, "hwc_rgb", channel), k)
            assert n == (a.shape[0] - 2 * k) * (a.shape[1] - 2 * k) * (3 if channel == "rgb" else 1)
            want = float(s["psnr_%s_k%d" % (channel, k)])
            for got in (ref.psnr(mse), frames.psnr(mse), frames.psnr(torch.tensor(mse, dtype=torch.float64))):
                assert abs(got - want) <= 1e-12 * want, (k, channel, got, want)
    assert abs(frames.psnr(4.0, peak=1023) - 20 * math.log10(1023 / 2.0)) < 1e-12


@pytest.mark.parametrize("h,w", [(11, 11), (26, 42), (27, 43), (37, 53)])
def test_separable_ssim_is_the_oracles(h, w):
    r = np.random.RandomState(h * 100 + w)
    a = r.randint(0, 256, (h, w, 3)).astype(np.uint8)
    b = np.clip(a.astype(np.int32) + r.randint(-20, 21, a.shape), 0, 255).astype(np.uint8)
    for sep in (True, False):
        assert abs(ref.ssim(a, b, 255, sep) - om.calculate_ssim(a, b)) < 1e-10
    ya, yb = ref.samples(a, "hwc_rgb", "y"), ref.samples(b, "hwc_rgb", "y")
    assert abs(ref.ssim(ya, yb) - om.calculate_ssim(ya[:, :, 0].astype(np.uint8), yb[:, :, 0].astype(np.uint8))) < 1e-10
    assert abs(ref.ssim(a, a) - 1.0) < 1e-12
    assert math.isnan(ref.ssim(a[:10], b[:10])) and math.isnan(ref.ssim(a[:, :10], b[:, :10]))


def close(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 * max(1.0, abs(b))


def test_score_summary_hand_written():
    mse = {0: 65025.0, 20: 650.25, 40: 6.5025}                     # PSNR in dB -> mse at peak 255
    db = [20, 20, 40, 40, 40, 40, 40, 0, 0]
    rows = torch.tensor([[mse[p], i / 10.0] for i, p in enumerate(db)], dtype=torch.float64)
    s = adapt.score_summary(rows, 5)                               # border_frame 2: frames 0, 1, 7, 8 are border frames
    assert len(s['scenes']) == 1
    sc = s['scenes'][0]
    assert (sc['first'], sc['frames'], sc['center_frames'], sc['border_frames']) == (0, 9, 5, 4)
    want = {'psnr': 240 / 9, 'psnr_center': 40.0, 'psnr_border': 10.0, 'ssim': 0.4, 'ssim_center': 0.4, 'ssim_border': 0.4}
    for k, v in want.items():
        assert close(sc[k], v) and close(s['mean'][k], v), (k, sc[k], v)
    # two scenes; the second (3 frames) is shorter than 2 * border_frame: no centre frame
    s = adapt.score_summary(rows, 5, cuts=[6])
    a, b = s['scenes']
    assert (a['first'], a['frames'], a['center_frames'], a['border_frames']) == (0, 6, 2, 4)
    assert (b['first'], b['frames'], b['center_frames'], b['border_frames']) == (6, 3, 0, 3)
    want_a = {'psnr': 200 / 6, 'psnr_center': 40.0, 'psnr_border': 30.0, 'ssim': 0.25, 'ssim_center': 0.25, 'ssim_border': 0.25}
    want_b = {'psnr': 40 / 3, 'psnr_center': float('nan'), 'psnr_border': 40 / 3, 'ssim': 0.7, 'ssim_center': float('nan'),
              'ssim_border': 0.7}
    for k in want_a:
        assert close(a[k], want_a[k]) and close(b[k], want_b[k]), k
        assert close(s['mean'][k], (want_a[k] + want_b[k]) / 2), k
    # no border frame at all: the border means are 0, like the reference's
    s = adapt.score_summary(rows.numpy(), 1)
    assert s['scenes'][0]['border_frames'] == 0 and s['scenes'][0]['psnr_border'] == 0 and s['scenes'][0]['ssim_border'] == 0
    assert close(s['scenes'][0]['psnr_center'], 240 / 9)
    # identical frames: inf, as calculate_psnr gives
    assert math.isinf(adapt.score_summary(torch.tensor([[0.0, 1.0]] * 3, dtype=torch.float64), 3)['mean']['psnr'])
    # another peak, and the numpy restatement
    for cuts in (None, [6], [2, 3]):
        got, want = adapt.score_summary(rows, 5, cuts=cuts, peak=1023), ref.summary(rows.tolist(), 5, cuts, 1023)
        assert len(got['scenes']) == len(want['scenes'])
        for x, y in zip(got['scenes'] + [got['mean']], want['scenes'] + [want['mean']]):
            assert x.keys() == y.keys() and all(close(x[k], y[k]) for k in x), (cuts, x, y)
    for bad in (dict(scores=torch.zeros(3)), dict(scores=torch.zeros(0, 2)), dict(scores=rows, nframes=0),
                dict(scores=rows, cuts=[9]), dict(scores=rows, cuts=[3, 3])):
        with pytest.raises(ValueError):
            adapt.score_summary(bad['scores'], bad.get('nframes', 5), bad.get('cuts'))


@pytest.fixture
def no_device(monkeypatch):
    """Any call into the library or of a stream fails the test."""
    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(frames.L, "lib", boom)
    monkeypatch.setattr(frames.L, "stream", boom)
    monkeypatch.setattr(torch.cuda, "current_stream", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)


def test_score_argument_errors(no_device):
    u8 = torch.zeros(24, 40, 3, dtype=torch.uint8)
    f32 = torch.zeros(3, 24, 40)
    nv12 = torch.zeros(36, 40, dtype=torch.uint8)
    p010 = torch.zeros(36, 40, dtype=torch.uint16)
    cases = [
        ((u8, u8), dict(channel='luma'), "channel"),
        ((u8, u8), dict(channel=None), "channel"),
        ((u8, u8), dict(crop_border=-1), "crop_border"),
        ((u8, u8), dict(crop_border=1.0), "crop_border"),
        ((u8, u8), dict(crop_border=True), "crop_border"),
        ((u8, u8), dict(crop_border=12), "leaves nothing"),
        ((u8, u8[:23]), dict(), "frame a is"),
        ((u8, f32[:, :, :39]), dict(), "frame a is"),
        ((f32, u8), dict(min_max=(1, 1)), "min_max"),
        ((f32, u8), dict(min_max=(1, 0)), "min_max"),
        ((f32, u8), dict(min_max=3), "min_max"),
        ((u8, nv12, None, 'nv12'), dict(), "channel='rgb'"),
        ((nv12, u8, 'i420', None), dict(channel='rgb'), "channel='rgb'"),
        ((u8, p010, None, 'p010'), dict(channel='y'), "mixed bit depths"),
        ((p010, p010, 'p010', 'i420p12'), dict(channel='y'), "mixed bit depths"),
        ((nv12, p010, 'nv12', 'p012'), dict(channel='y'), "mixed bit depths"),
        ((u8, u8, 'chw'), dict(), "interleaved"),
        ((u8, f32, None, 'hwc_rgb'), dict(), "planar"),
        ((u8, nv12), dict(), "must be"),                           # a 4:2:0 layout is never inferred
        ((u8, None), dict(), "tensor"),
        ((u8, u8), dict(out=torch.zeros(2)), "out must be"),
        ((u8, u8), dict(out=torch.zeros(3, dtype=torch.float64)), "out must be"),
        ((u8, u8), dict(out=torch.zeros(2, dtype=torch.float64)), "on the GPU"),
        ((u8, u8), dict(out=[0.0, 0.0]), "out must be"),
    ]
    for args, kw, match in cases:
        with pytest.raises(ValueError, match=match):
            frames.score(*args, **kw)
    big = torch.zeros(1, 1, 3, dtype=torch.uint8).expand(40000, 16, 3)
    with pytest.raises(ValueError, match="at most"):
        frames.score(big, big)


class Mean(torch.nn.Module):
    nframes = 3

    def forward(self, x):
        return x.mean(1)


def test_super_resolve_frames_gt_argument_errors(no_device):
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    T, h, w = 7, 16, 24
    cpu_scores = torch.zeros(T, 2, dtype=torch.float64)
    for net, s, opt in ((Mean(), 1, {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}),
                        (EDVR(), 4, {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}})):
        u8 = torch.zeros(T, h, w, 3, dtype=torch.uint8)
        f32 = torch.zeros(T, 3, h, w)
        gt8 = torch.zeros(T, s * h, s * w, 3, dtype=torch.uint8)
        gtf = torch.zeros(T, 3, s * h, s * w)
        gtnv = torch.zeros(T, s * h * 3 // 2, s * w, dtype=torch.uint8)
        gtp10 = torch.zeros(T, s * h * 3 // 2, s * w, dtype=torch.uint16)
        cases = [
            (u8, dict(scores=cpu_scores), "scores without gt"),
            (u8, dict(gt=gt8[:6]), "gt has 6 frames"),
            (u8, dict(gt=gt8[:, :-1]), "frame a is"),                              # not the output's size
            (f32, dict(gt=gtf[:, :, :, :-4]), "frame a is"),                       # the float path that needs no conversion
            (u8, dict(gt=gt8, out_size=(s * h - 2, s * w)), "frame a is"),         # the GT has the size of out_size
            (u8, dict(gt=gt8, score='luma'), "channel"),
            (u8, dict(gt=gt8, crop_border=-2), "crop_border"),
            (u8, dict(gt=gt8, crop_border=s * h), "leaves nothing"),
            (u8, dict(gt=gt8, out='nv12'), "channel='rgb'"),                       # rgb on a 4:2:0 output
            (u8, dict(gt=gtnv, gt_layout='nv12'), "channel='rgb'"),
            (u8, dict(gt=gtnv), "must be"),                                        # the GT's 4:2:0 layout is never inferred
            (u8, dict(gt=gt8, gt_layout='chw'), "interleaved"),
            (u8, dict(gt=gt8, out='nv12', score='y', matrix='bt709'), "matrix='bt601'"),
            (u8, dict(gt=gt8, out='i420', score='y', yuv_range='full'), "matrix='bt601'"),
            (u8, dict(gt=gt8, out='p010', score='y'), "mixed bit depths"),
            (u8, dict(gt=gtp10, gt_layout='p010', score='y'), "mixed bit depths"),
            (u8, dict(gt=gtp10, gt_layout='i420p12', out='p010', score='y'), "mixed bit depths"),
            (u8, dict(gt=gt8), "gt needs scores"),
            (u8, dict(gt=gt8, scores=cpu_scores), "gt needs scores"),              # not on the GPU
            (u8, dict(gt=gt8, scores=cpu_scores.float()), "gt needs scores"),
            (u8, dict(gt=gt8, scores=torch.zeros(T - 1, 2, dtype=torch.float64)), "gt needs scores"),
            (u8, dict(gt=gt8, out='nv12', score='y', scores=cpu_scores), "gt needs scores"),   # (everything else is in order)
            (u8, dict(gt=gtnv, gt_layout='i420', out='nv12', score='y', matrix='bt709', scores=cpu_scores), "gt needs scores"),
        ]
        for video, kw, match in cases:
            with pytest.raises(ValueError, match=match):
                next(adapt.super_resolve_frames(opt, net, video, padding='replicate', **kw))


def test_c_abi_argument_errors_return_before_any_launch():
    """Every bad argument of dvsr_frame_score is refused on the host (no device here, and the pointers are never followed)."""
    from dynavsr_amd import _lib as L
    lib = L.lib()
    INVALID, WORKSPACE = -1, -3
    P = 0x10000                                                   # a well-aligned address that is never dereferenced
    h, w = 24, 40
    need = lib.dvsr_frame_score_workspace_bytes(3, h, w)
    assert need > 0 and lib.dvsr_frame_score_workspace_bytes(1, h, w) > 0
    assert lib.dvsr_frame_score_workspace_bytes(0, h, w) == 0 and lib.dvsr_frame_score_workspace_bytes(3, 0, w) == 0
    assert lib.dvsr_frame_score_workspace_bytes(3, h - 14, w - 14) <= need          # the uncropped figure serves every crop

    def call(a=P, da=None, b=P, db=None, args=None, out=P, ws=P, nbytes=need):
        da = da if da is not None else L.FrameDesc(L.FRAME_U8_HWC_RGB, h, w, 3 * w, 0, 3)
        db = db if db is not None else L.FrameDesc(L.FRAME_U8_HWC_BGR, h, w, 4 * w, 0, 4)
        args = args if args is not None else L.ScoreArgs(L.SCORE_RGB, 0, 8, 0.0, 1.0)
        ref_ = lambda s: ctypes.byref(s) if s != 'null' else None
        return lib.dvsr_frame_score(a, ref_(da), b, ref_(db), ref_(args), out, ws, nbytes, None)

    rgb = lambda **k: L.FrameDesc(*[k.get(f, v) for f, v in (('format', L.FRAME_U8_HWC_RGB), ('h', h), ('w', w),
                                                             ('row_stride', 3 * w), ('plane_stride', 0), ('pixel_stride', 3))])
    f32 = lambda **k: L.FrameDesc(*[k.get(f, v) for f, v in (('format', L.FRAME_F32_CHW), ('h', h), ('w', w),
                                                             ('row_stride', w), ('plane_stride', h * w), ('pixel_stride', 1))])
    y8 = lambda **k: L.FrameDesc(*[k.get(f, v) for f, v in (('format', L.FRAME_U8_Y), ('h', h), ('w', w), ('row_stride', w),
                                                            ('plane_stride', 0), ('pixel_stride', 1))])
    y16 = lambda fmt, **k: L.FrameDesc(*[k.get(f, v) for f, v in (('format', fmt), ('h', h), ('w', w), ('row_stride', 2 * w),
                                                                  ('plane_stride', 0), ('pixel_stride', 2))])
    Y = lambda depth=8, k=0: L.ScoreArgs(L.SCORE_Y, k, depth, 0.0, 1.0)
    bad = [
        dict(a=None), dict(b=None), dict(da='null'), dict(db='null'), dict(args='null'), dict(out=None), dict(ws=None),
        dict(db=rgb(h=h - 1)), dict(db=rgb(w=w + 1)), dict(da=rgb(h=0), db=rgb(h=0)),            # sizes
        dict(da=rgb(format=7)), dict(db=rgb(format=-1)),                                          # unknown format
        dict(args=L.ScoreArgs(2, 0, 8, 0.0, 1.0)), dict(args=L.ScoreArgs(L.SCORE_RGB, 0, 9, 0.0, 1.0)),
        dict(args=L.ScoreArgs(L.SCORE_RGB, 0, 16, 0.0, 1.0)),
        dict(args=L.ScoreArgs(L.SCORE_RGB, 0, 10, 0.0, 1.0)),                                     # 8-bit frames at depth 10
        dict(da=y8(), db=y16(L.FRAME_U16_Y_MSB), args=Y(8)), dict(da=y8(), db=y16(L.FRAME_U16_Y_MSB), args=Y(10)),
        dict(da=y16(L.FRAME_U16_Y_10), db=y16(L.FRAME_U16_Y_12), args=Y(10)),
        dict(da=y16(L.FRAME_U16_Y_10), db=y16(L.FRAME_U16_Y_MSB), args=Y(12)),
        dict(da=y8()), dict(db=y16(L.FRAME_U16_Y_MSB), args=L.ScoreArgs(L.SCORE_RGB, 0, 10, 0.0, 1.0)),   # rgb on a Y plane
        dict(args=L.ScoreArgs(L.SCORE_RGB, 12, 8, 0.0, 1.0)), dict(args=L.ScoreArgs(L.SCORE_RGB, -1, 8, 0.0, 1.0)),
        dict(da=rgb(row_stride=3 * w - 1)), dict(db=rgb(pixel_stride=4, row_stride=4 * w - 1)), dict(da=rgb(pixel_stride=2)),
        dict(da=f32(row_stride=w - 1)), dict(da=f32(plane_stride=h * w - 1)), dict(a=P + 2, da=f32()),
        dict(da=f32(), args=L.ScoreArgs(L.SCORE_RGB, 0, 8, 1.0, 1.0)),
        dict(da=y8(pixel_stride=2), db=y8(), args=Y()), dict(da=y8(row_stride=w - 1), db=y8(), args=Y()),
        dict(a=P + 1, da=y16(L.FRAME_U16_Y_MSB), db=y16(L.FRAME_U16_Y_10), args=Y(10)),           # an odd address ...
        dict(da=y16(L.FRAME_U16_Y_MSB), db=y16(L.FRAME_U16_Y_10, row_stride=2 * w + 1), args=Y(10)),   # ... or stride
        dict(da=y16(L.FRAME_U16_Y_12, row_stride=2 * w - 2), db=y16(L.FRAME_U16_Y_12), args=Y(12)),
        dict(out=P + 4), dict(ws=P + 4),
    ]
    for kw in bad:
        assert call(**kw) == INVALID, kw
        assert lib.dvsr_last_error().startswith(b"frame_score:"), kw
    assert call(nbytes=need - 1) == WORKSPACE and call(nbytes=0) == WORKSPACE
    assert b"workspace" in lib.dvsr_last_error()
