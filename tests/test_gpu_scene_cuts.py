"""GPU: scene cuts in the video path -- dvsr_frame_luma_sad (csrc/frame_cut.hip) through frames.luma_sad / detect_cuts, and
adapt.super_resolve_frames(cuts=...), whose windows stay inside a scene.

The sums are integers: frames.luma_sad equals the numpy restatement in tests/cut_ref.py exactly, no tolerance.  Scenes are
independent bit for bit: super_resolve_frames(cuts=[k]) is torch.equal to separate calls on the scenes (the slot count of
the frame cache does not change bits: test_gpu_stream.py::test_stream_results_do_not_depend_on_in_flight)."""
import ctypes

import numpy as np
import pytest
import torch

import cut_ref
from conftest import relerr
from dynavsr_amd import _lib as L
from dynavsr_amd import adapt, engine, synth
from dynavsr_amd import frames as fio

pytestmark = pytest.mark.gpu

MODES = ('replicate', 'reflection', 'new_info', 'circle')
SIZES = [(4, 4), (5, 7), (33, 70), (64, 260)]          # 64 x 260: wider than the 256 pixels of one workgroup's row
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}


def sad(frames, layout=None):
    out = fio.luma_sad(frames, layout)
    assert out.dtype == torch.int64 and not out.is_cuda and tuple(out.shape) == (len(frames) - 1,)
    return out.numpy()


def same(got, want):
    want = np.asarray(want, dtype=np.int64)
    assert got.shape == want.shape and (got == want).all(), (got, want)


@pytest.mark.parametrize("hw", SIZES)
def test_sad_hwc_is_exact(hw):
    h, w = hw
    r = np.random.RandomState(h * 1000 + w)
    v = r.randint(0, 256, (4, h, w, 3)).astype(np.uint8)
    want_rgb, want_bgr = cut_ref.luma_sad(v, 'hwc_rgb'), cut_ref.luma_sad(v, 'hwc_bgr')
    assert (want_rgb != want_bgr).any()
    dev = torch.from_numpy(v).cuda()
    same(sad(dev, 'hwc_rgb'), want_rgb)                                      # one launch over the [4, ...] tensor
    same(sad(dev), want_rgb)                                                 # (uint8 defaults to 'hwc_rgb')
    same(sad(dev, 'hwc_bgr'), want_bgr)
    same(sad(dev.flip(-1).contiguous(), 'hwc_bgr'), want_rgb)                # the two orders differ by the channel swap alone
    same(sad([dev[t] for t in range(4)], 'hwc_rgb'), want_rgb)               # the same frames as a list: a launch per pair
    same(sad(torch.from_numpy(v), 'hwc_bgr'), want_bgr)                      # CPU frames, through the staging buffers
    same(sad([torch.from_numpy(v[t]) for t in range(4)], 'hwc_rgb'), want_rgb)
    # 4 bytes per pixel: the fourth is ignored
    v4 = np.concatenate([v, r.randint(0, 256, (4, h, w, 1)).astype(np.uint8)], -1)
    d4 = torch.from_numpy(v4).cuda()
    same(sad(d4, 'hwc_rgb'), want_rgb)
    same(sad([d4[t] for t in range(4)], 'hwc_bgr'), want_bgr)
    # a pitched view at an odd byte offset, passed by stride
    pitch = w * 3 + 5
    buf = torch.from_numpy(r.randint(0, 256, (1 + 4 * h * pitch,)).astype(np.uint8)).cuda()
    view = buf.as_strided((4, h, w, 3), (h * pitch, pitch, 3, 1), 1)
    assert view.data_ptr() % 2 == 1
    view.copy_(dev)
    assert fio.describe(view[1], 'hwc_rgb')[0].data_ptr() == view[1].data_ptr()      # (no copy is made)
    same(sad(view, 'hwc_rgb'), want_rgb)
    same(sad([view[t] for t in range(4)], 'hwc_bgr'), want_bgr)
    same(sad([view[0], dev[1], view[2], dev[3]], 'hwc_rgb'), want_rgb)       # views of different pitch in one list


@pytest.mark.parametrize("hw", SIZES)
def test_sad_chw_floats_is_exact(hw):
    h, w = hw
    r = np.random.RandomState(h * 1000 + w + 1)
    # values exactly at the .5 / 255 steps (where round-half-to-even decides), below 0, above 1, and ordinary ones
    k = r.randint(-3, 259, (4, 3, h, w))
    v = ((k + 0.5) / 255.0).astype(np.float32)
    plain = r.uniform(-0.2, 1.2, v.shape).astype(np.float32)
    pick = r.randint(0, 2, v.shape).astype(bool)
    v = np.where(pick, v, plain)
    v[0, :, 0, 0] = (-1.0, 2.0, 0.5 / 255.0)
    assert (v < 0).any() and (v > 1).any()
    want = cut_ref.luma_sad(v, 'chw')
    assert want.min() > 0
    dev = torch.from_numpy(v).cuda()
    same(sad(dev, 'chw'), want)
    same(sad(dev), want)
    same(sad([dev[t] for t in range(4)]), want)
    same(sad(torch.from_numpy(v)), want)
    # rows that are not 16-byte aligned: a view one float into a wider buffer
    wide = torch.zeros((4, 3, h, w + 3), device='cuda')
    wide[..., 1:w + 1] = dev
    same(sad(wide[..., 1:w + 1], 'chw'), want)
    same(sad(dev.double(), 'chw'), want)                                      # (other float types are brought to fp32 first)


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("layout", ['nv12', 'i420'])
def test_sad_yuv_is_the_y_plane(hw, layout):
    h, w = hw
    r = np.random.RandomState(h * 1000 + w + 2)
    hc, wc = (h + 1) // 2, (w + 1) // 2
    y = r.randint(0, 256, (4, h, w)).astype(np.uint8)
    want = cut_ref.luma_sad(y, layout)

    def chroma(t):
        c = torch.from_numpy(r.randint(0, 256, (hc, wc, 2)).astype(np.uint8)).cuda()
        return (c,) if layout == 'nv12' else (c[..., 0].contiguous(), c[..., 1].contiguous())

    # planes, every size (odd ones included); the Y plane of frame 1 is a pitched view at an odd offset
    planes = [(torch.from_numpy(y[t]).cuda(),) + chroma(t) for t in range(4)]
    buf = torch.zeros((1 + h * (w + 3),), dtype=torch.uint8, device='cuda')
    yv = buf.as_strided((h, w), (w + 3, 1), 1)
    yv.copy_(planes[1][0])
    planes[1] = (yv,) + planes[1][1:]
    same(sad(planes, layout), want)
    same(sad([tuple(p.cpu() for p in f) for f in planes], layout), want)
    if h % 2 == 0 and w % 2 == 0:
        packed = np.concatenate([y, r.randint(0, 256, (4, h // 2, w)).astype(np.uint8)], axis=1)
        dev = torch.from_numpy(packed).cuda()
        same(sad(dev, layout), want)                                          # [4, h*3/2, w]: one launch
        same(sad([dev[t] for t in range(4)], layout), want)
        same(sad(torch.from_numpy(packed), layout), want)


def test_sad_full_scale_and_beyond_32_bits():
    h, w = 64, 260
    lo, hi = torch.zeros((h, w, 3), dtype=torch.uint8, device='cuda'), torch.full((h, w, 3), 255, dtype=torch.uint8, device='cuda')
    same(sad([lo, hi, lo, lo], 'hwc_rgb'), [255 * h * w, 255 * h * w, 0])
    same(sad((torch.stack([lo, hi]).float() / 255).permute(0, 3, 1, 2)), [255 * h * w])     # (a view that is copied first)
    # two Y planes made on the device: the sum does not fit 32 bits
    n = 4112
    uv = torch.zeros((n // 2, n // 2, 2), dtype=torch.uint8, device='cuda')
    a = (torch.zeros((n, n), dtype=torch.uint8, device='cuda'), uv)
    b = (torch.full((n, n), 255, dtype=torch.uint8, device='cuda'), uv)
    assert 255 * n * n == 4311678720 > 2 ** 32
    same(sad([a, b], 'nv12'), [4311678720])


def test_sad_single_frame_and_bad_arguments():
    one = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device='cuda')
    assert tuple(fio.luma_sad(one).shape) == (0,) and fio.detect_cuts(one) == []
    with pytest.raises(ValueError):
        fio.luma_sad([one[0], torch.zeros((8, 9, 3), dtype=torch.uint8, device='cuda')])
    with pytest.raises(ValueError):
        fio.detect_cuts(one, threshold=0)
    lib, st = L.lib(), L.stream()
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device='cuda')
    out = torch.full((1,), 7, dtype=torch.int64, device='cuda')

    def call(fields, a=x.data_ptr(), b=x[1].data_ptr(), pairs=1, res=out.data_ptr()):
        return lib.dvsr_frame_luma_sad(a, b, ctypes.byref(L.FrameDesc(*fields)), 192, pairs, res, st)

    good = (L.FRAME_U8_HWC_RGB, 8, 8, 24, 0, 3)
    assert call(good, a=None) == -1 and call(good, b=None) == -1 and call(good, res=None) == -1
    assert call(good, pairs=0) == -1 and b"pairs" in lib.dvsr_last_error()
    assert call((7, 8, 8, 24, 0, 3)) == -1 and b"format" in lib.dvsr_last_error()
    assert call((L.FRAME_U8_HWC_RGB, 8, 8, 24, 0, 1)) == -1 and call((L.FRAME_U8_Y, 8, 8, 24, 0, 3)) == -1
    assert call((L.FRAME_U8_HWC_RGB, 8, 8, 23, 0, 3)) == -1 and call((L.FRAME_U8_HWC_RGB, 0, 8, 24, 0, 3)) == -1
    assert call((L.FRAME_F32_CHW, 2, 4, 4, 7, 0)) == -1 and call((L.FRAME_F32_CHW, 2, 4, 4, 8, 0), a=x.data_ptr() + 1) == -1
    assert call(good, res=out.data_ptr() + 4) == -1
    torch.cuda.synchronize()
    assert int(out[0]) == 7                                                   # nothing was launched, nothing zeroed
    assert call(good) == 0
    torch.cuda.synchronize()
    assert int(out[0]) == 0
    # ingest keeps rejecting the single-plane format
    d = L.FrameDesc(L.FRAME_U8_Y, 8, 8, 8, 0, 1)
    dst = torch.zeros((3, 8, 8), device='cuda')
    assert lib.dvsr_frame_ingest(x.data_ptr(), ctypes.byref(d), dst.data_ptr(), 8, 8, L.FRAME_PAD_REPLICATE, st) == -1


def test_cuts_are_found():
    threshold = 10.0
    v = cut_ref.scene_video()                                                 # 14 frames 24 x 40, scenes of 5, 4, 5
    assert v.shape == (14, 24, 40, 3)
    nv12 = cut_ref.rgb_to_nv12(v)
    chw = np.ascontiguousarray(v.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)
    for frames, layout in ((v, 'hwc_rgb'), (nv12[:, :24], 'nv12'), (chw, 'chw')):
        s = cut_ref.scene_scores(cut_ref.luma_sad(frames, layout), 24, 40)
        for t in range(14):
            if t in (5, 9):
                assert s[t] > 4 * threshold, (layout, t, s[t])
            else:
                assert s[t] < threshold / 4, (layout, t, s[t])
    assert fio.detect_cuts(torch.from_numpy(v).cuda(), 'hwc_rgb', threshold) == [5, 9]
    assert fio.detect_cuts(torch.from_numpy(v), None) == [5, 9]               # CPU frames, the default threshold
    assert fio.detect_cuts(torch.from_numpy(nv12).cuda(), 'nv12', threshold) == [5, 9]
    assert fio.detect_cuts(torch.from_numpy(chw).cuda(), 'chw', threshold) == [5, 9]
    assert fio.detect_cuts(torch.from_numpy(chw).cuda(), threshold=90.0) == []


# ---- super_resolve_frames(cuts=...)

_nets, _refs = {}, {}


def make_net():
    if 'edvr' not in _nets:
        from dynavsr_amd.models.archs.EDVR_arch import EDVR
        net = EDVR()
        net.load_state_dict(synth.edvr_state_dict(0), strict=True)
        _nets['edvr'] = net.cuda()
    return _nets['edvr']


def two_scene_video():
    if 'video' not in _refs:
        _refs['video'] = torch.cat([synth.clip(91, 1, 5, 24, 40)[0], synth.clip(92, 1, 7, 24, 40)[0]]).cuda()
    return _refs['video']


def run(frames, mode='new_info', in_flight=2, **kw):
    return [sr.clone() for sr in adapt.super_resolve_frames(OPT, make_net(), frames, padding=mode, in_flight=in_flight, **kw)]


def separate_scenes(mode):
    """The two scenes of the video through two separate calls, once per mode (results do not depend on in_flight)."""
    if mode not in _refs:
        video = two_scene_video()
        _refs[mode] = run(video[:5], mode, 1) + run(video[5:], mode, 1)
    return _refs[mode]


@pytest.mark.parametrize("in_flight", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES)
def test_scenes_are_independent_bit_for_bit(mode, in_flight):
    video = two_scene_video()
    want = separate_scenes(mode)
    plan = engine.get_stream_plan(make_net()._cfg(), 24, 40, adapt.stream_slots(5, in_flight, 2), video.device)
    before = plan.stats['extracted']
    got = run(video, mode, in_flight, cuts=[5])
    assert plan.stats['extracted'] - before == 12
    assert len(got) == 12
    for t in range(12):
        assert torch.equal(got[t], want[t]), (mode, in_flight, t, float((got[t] - want[t]).abs().max()))


def test_short_scenes_take_replicate():
    video = two_scene_video()
    got = run(video, 'new_info', 2, cuts=[3, 4])                              # scenes of 3, 1 and 8 frames
    want = run(video[:3], 'replicate', 2) + run(video[3:4], 'replicate', 2) + run(video[4:], 'new_info', 2)
    assert len(got) == 12
    for t in range(12):
        assert torch.equal(got[t], want[t]), t


def test_the_argument_does_something():
    video = two_scene_video()
    whole = run(video, 'new_info', 2)                                         # cuts=None: frame 5's window reads frames 3 and 4
    cut = separate_scenes('new_info')
    e, d = relerr(whole[5], cut[5]), float((whole[5] - cut[5]).abs().max())
    print("frame 5, one scene vs cut at 5: rel-L2 %.3e max-abs %.3e" % (e, d))
    assert e > 2e-4 and d > 1e-3                                              # beyond the parity bar of test_gpu_stream.py
    assert torch.equal(whole[8], cut[8]) or relerr(whole[8], cut[8]) < 2e-4   # a frame whose window never saw the cut


def test_auto_cuts_on_bytes():
    v = torch.from_numpy(cut_ref.scene_video()).cuda()
    auto = run(v, 'new_info', 2, cuts='auto')
    want = run(v, 'new_info', 2, cuts=[5, 9])
    assert len(auto) == 14 and auto[0].dtype == torch.uint8 and tuple(auto[0].shape) == (96, 160, 3)
    assert all(torch.equal(a, b) for a, b in zip(auto, want))
    none = run(v, 'new_info', 2)
    assert not torch.equal(none[5], want[5])
    with pytest.raises(ValueError):
        next(adapt.super_resolve_frames(OPT, make_net(), v, cuts='scenes'))
    # a threshold nothing reaches: one scene, cuts=[]
    assert all(torch.equal(a, b) for a, b in zip(run(v, 'new_info', 2, cuts='auto', cut_threshold=99.0), run(v, 'new_info', 2, cuts=[])))


def test_another_backbone_respects_cuts():
    from dynavsr_amd.models.archs import DUF_arch
    net = DUF_arch.DUF_16L(scale=2, adapt_official=True)
    net.load_state_dict(synth.duf_state_dict(4, 16, 2), strict=True)
    net = net.cuda().eval()
    opt = {'scale': 2, 'network_G': {'which_model_G': 'DUF', 'nframes': 7}}
    video = torch.cat([synth.clip(93, 1, 5, 8, 12)[0], synth.clip(94, 1, 7, 8, 12)[0]]).cuda()

    def go(frames, **kw):
        return [sr.clone() for sr in adapt.super_resolve_frames(opt, net, frames, padding='reflection', **kw)]

    got = go(video, cuts=[5])
    want = go(video[:5]) + go(video[5:])
    assert len(got) == 12 and tuple(got[0].shape) == (1, 3, 16, 24)
    for t in range(12):
        assert torch.equal(got[t], want[t]), t
    whole = go(video)
    assert not torch.equal(whole[5], got[5])
