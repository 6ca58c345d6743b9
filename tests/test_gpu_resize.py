"""GPU: SR frames at a target output size (csrc/frame_resize.hip, frames.resize / frames.emit(size=),
adapt.super_resolve_frames(out_size=)).

The yardstick is tests/resize_ref.py, the fp64 restatement of the resampler (torch's bicubic antialias op to 1e-12:
test_resize_host.py).  Bars:
  resize   max-abs <= 3 (n + 1) 2^-24, n the larger tap count of the case: two passes, each with weights rounded to fp32 and a
           sum of n products, the second on values of up to sum |w| ~ 1.25 times the input (1.6e-6 at 8 taps, 3.4e-6 at 18)
  bytes    a byte / word equals rint of the fp64 level wherever that level is farther than TIE from a tie and is within 1
           elsewhere; TIE = the conversion's own + the resize bar x (levels - 1).  The conversion's own is 1e-3 of the 8-bit
           YCbCr tests and 4e-3 at 10 bits (test_gpu_yuv.py, test_gpu_yuv16.py); for 8-bit RGB, which those files compare with
           an fp32 recipe bit for bit, it is the fp32 rounding of t x 255 against fp64: 255 x 2^-24 < 2e-5 levels
  video    bit-identical to emit(size=) of the float frame that the same call yields without out_size; the float frames at the
           forward bars against the CPU oracle's SR frame resized by resize_ref: rel-L2 < 2e-4, max-abs < 1.6e-3 (the 1e-3 bar
           times sum |w|^2 <= 1.56 of the two passes)"""
import numpy as np
import pytest
import torch

import resize_ref as ref
import yuv16_ref
from conftest import relerr
from dynavsr_amd import adapt, frames, synth
from dynavsr_amd.data.util import index_generation

pytestmark = pytest.mark.gpu

OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
SENTINEL = 0xA5
LAYOUTS = ['chw', 'hwc_rgb', 'hwc_bgr', 'nv12', 'i420', 'p010', 'i420p12']
TIE_OWN = {'hwc_rgb': 2e-5, 'p010': 4e-3}
TIE_SHARE = 0.05
_INPUT = {}


def case_input(case):
    """(host fp32 [3,Hs,Ws] of uniform [0,1), the fp64 reference of its crop at the target size, the bar, taps): computed once."""
    if case not in _INPUT:
        (h, w), (Hs, Ws), size = case
        host = np.random.RandomState(Hs * 1000 + Ws + size[0]).uniform(0, 1, (3, Hs, Ws)).astype(np.float32)
        bar, n = ref.bound([(h, size[0]), (w, size[1])])
        _INPUT[case] = (torch.from_numpy(host), ref.resize(host[:, :h, :w], size), bar, n)
    return _INPUT[case]


def whole_buffer(view):
    """The [3,oh,Wb] buffer of which resize() returned the [3,oh,ow] view."""
    assert view.stride(2) == 1 and view.stride(1) % 4 == 0 and view.stride(0) == view.shape[1] * view.stride(1)
    assert view.data_ptr() % 16 == 0 and 0 <= view.stride(1) - view.shape[2] < 4
    return view.as_strided((3, view.shape[1], view.stride(1)), view.stride(), view.storage_offset())


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[2]))
def test_resize_against_fp64(case):
    (h, w), (Hs, Ws), (oh, ow) = case
    host, want, bar, n = case_input(case)
    sr = host.cuda()
    got = frames.resize(sr, h, w, (oh, ow))
    assert got.dtype == torch.float32 and got.shape == (3, oh, ow) and got.is_cuda
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print("%dx%d of %dx%d -> %dx%d: %d taps, max-abs %.2e (bar %.2e), values in [%.3f, %.3f]" % (
        h, w, Hs, Ws, oh, ow, n, err, bar, want.min(), want.max()))
    assert err <= bar
    buf = whole_buffer(got)
    assert bool((buf[:, :, ow:] == 0).all())                                    # what emit's 16-byte loads read past ow
    if (h, w) == (oh, ow):
        assert torch.equal(got.cpu(), host[:, :h, :w])                          # weights 0, 1, 0, 0: a copy
    if (h, w) == (12, 20):
        assert want.min() < 0 or want.max() > 1                                 # up-scaling leaves [0,1]
    # into a buffer of the caller's: the same bits, and nothing behind it
    Wb = -(-ow // 4) * 4
    big = torch.full((3 * oh * Wb + 256,), float('nan'), device='cuda')
    out = big[:3 * oh * Wb].view(3, oh, Wb)
    again = frames.resize(sr[None], h, w, (oh, ow), out=out)
    assert again.data_ptr() == out.data_ptr() and torch.equal(again, got)
    assert bool(torch.isnan(big[3 * oh * Wb:]).all()) and bool((out[:, :, ow:] == 0).all())


def test_resize_rejects_bad_arguments():
    sr = torch.zeros(3, 16, 16, device='cuda')
    for size in ((3, 16), (16, 33), (0, 8), (8,), '1080p', (8.0, 8)):
        with pytest.raises(ValueError):
            frames.resize(sr, 16, 16, size)
    with pytest.raises(ValueError):
        frames.resize(sr, 17, 16, (16, 16))
    with pytest.raises(ValueError):
        frames.resize(sr, 16, 16, (8, 10), out=torch.zeros(3, 8, 10, device='cuda'))
    with pytest.raises(ValueError):
        frames.emit(sr, 16, 16, 'nv12', size=(9, 10))                           # packed 4:2:0 needs an even size


def test_padding_never_bleeds():
    case = ref.CASES[0]
    (h, w), (Hs, Ws), size = case
    host, want, bar, _ = case_input(case)
    got = []
    for fill in (float('nan'), 0.0):
        x = torch.full((3, Hs, Ws), fill)
        x[:, :h, :w] = host[:, :h, :w]
        got.append(frames.resize(x.cuda(), h, w, size).cpu())
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32))
    assert float(np.abs(got[0].numpy().astype(np.float64) - want).max()) <= bar


def as_numpy(x):
    if not torch.is_tensor(x):
        return [as_numpy(p) for p in x]
    return (x.view(torch.int16) if x.dtype == torch.uint16 else x).cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(as_numpy(a), as_numpy(b))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_emit_with_a_size_is_resize_then_emit(layout):
    h, w, Hs, Ws, oh, ow = 37, 53, 40, 56, 22, 30
    host = torch.from_numpy(np.random.RandomState(7).uniform(-0.2, 1.2, (3, Hs, Ws)).astype(np.float32))
    sr = host.cuda()
    kw = dict(matrix='bt709', yuv_range='full') if layout in ('i420', 'p010') else {}
    one = frames.emit(sr, h, w, layout, size=(oh, ow), **kw)
    mid = frames.resize(sr, h, w, (oh, ow))
    two = frames.emit(mid, oh, ow, layout, **kw)
    assert same_bits(one, two)
    assert tuple(one.shape) == {'chw': (3, oh, ow), 'hwc_rgb': (oh, ow, 3), 'hwc_bgr': (oh, ow, 3)}.get(layout, (oh * 3 // 2, ow))
    if layout == 'chw':
        assert torch.equal(one, mid)
    ranged = frames.emit(sr[None], h, w, layout, (-0.2, 1.2), size=(oh, ow), **kw)       # min_max passes through
    assert same_bits(ranged, frames.emit(mid, oh, ow, layout, (-0.2, 1.2), **kw))
    if layout not in ('chw',):
        assert not same_bits(ranged, one)


def test_emit_with_a_size_into_a_pitched_offset_out():
    h, w, Hs, Ws, oh, ow = 37, 53, 40, 56, 21, 30
    sr = torch.from_numpy(np.random.RandomState(8).uniform(-0.2, 1.2, (3, Hs, Ws)).astype(np.float32)).cuda()
    pitch = 3 * ow + 7
    buf = torch.full((3 + oh * pitch + 16,), SENTINEL, dtype=torch.uint8, device='cuda')
    dst = buf.as_strided((oh, ow, 3), (pitch, 3, 1), 3)
    assert dst.data_ptr() % 2 == 1
    got = frames.emit(sr, h, w, 'hwc_bgr', out=dst, size=(oh, ow))
    assert got.data_ptr() == dst.data_ptr()
    assert torch.equal(dst, frames.emit(frames.resize(sr, h, w, (oh, ow)), oh, ow, 'hwc_bgr'))
    rest = buf.clone()
    rest.as_strided(dst.shape, dst.stride(), dst.storage_offset()).fill_(SENTINEL)
    assert bool((rest == SENTINEL).all())                                      # not a byte outside the oh x ow image
    # planes of an odd-sized 4:2:0 frame
    y = torch.full((oh, ow), SENTINEL, dtype=torch.uint8, device='cuda')
    uv = torch.full(((oh + 1) // 2, (ow + 1) // 2, 2), SENTINEL, dtype=torch.uint8, device='cuda')
    frames.emit(sr, h, w, 'nv12', out=(y, uv), size=(oh, ow))
    y2, uv2 = torch.empty_like(y), torch.empty_like(uv)
    frames.emit(frames.resize(sr, h, w, (oh, ow)), oh, ow, 'nv12', out=(y2, uv2))
    assert torch.equal(y, y2) and torch.equal(uv, uv2)


@pytest.mark.parametrize("layout", ['hwc_rgb', 'p010'])
def test_bytes_against_fp64(layout):
    """One end-to-end anchor: resize_ref, then the conversion's fp64 restatement, against the bytes / words of emit(size=)."""
    h, w, Hs, Ws, oh, ow = 37, 53, 40, 56, 22, 30
    host = np.random.RandomState(21).uniform(0, 1, (3, Hs, Ws)).astype(np.float32)
    bar, n = ref.bound([(h, oh), (w, ow)])
    resized = ref.resize(host[:, :h, :w], (oh, ow))
    got = frames.emit(torch.from_numpy(host).cuda(), h, w, layout, size=(oh, ow))
    if layout == 'hwc_rgb':
        top, levels = 255, [np.transpose(ref.levels_u8(resized), (1, 2, 0))]
        have = [got.cpu().numpy().astype(np.int64)]
    else:
        top, levels = 1023, yuv16_ref.emit(resized, oh, ow, 10)
        words = yuv16_ref.unpack(got.view(torch.int16).cpu().numpy().view(np.uint16), layout)
        parts = [yuv16_ref.from_words(p, 'msb', 10) for p in words]
        assert all(int(rest.max()) == 0 for _, rest in parts)
        have = [lev.astype(np.int64) for lev, _ in parts]
    tie = TIE_OWN[layout] + bar * top
    near = total = 0
    for g, v in zip(have, levels):
        assert g.shape == v.shape
        want = np.clip(np.rint(v), 0, top).astype(np.int64)
        far = ref.tie_distance(v, top) > tie
        assert np.array_equal(g[far], want[far]), (layout, int((g[far] != want[far]).sum()))
        assert int(np.abs(g - want).max()) <= 1
        near += int((~far).sum())
        total += v.size
    print("%s %dx%d -> %dx%d: %d taps, TIE %.2e levels, %.2f %% of the values within it" % (
        layout, h, w, oh, ow, n, tie, 100.0 * near / total))
    assert near / total <= TIE_SHARE


# ---- end to end ----------------------------------------------------------------------------------
T = 7
SIZE = (40, 50)
_E2E = {}


def make_net(sd):
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    net = EDVR()
    net.load_state_dict(sd, strict=True)
    return net.cuda()


def run(net, video, **kw):
    return [sr.clone() for sr in adapt.super_resolve_frames(OPT, net, video, padding='new_info', **kw)]


def e2e_case(h, w):
    """Per size, computed once and never modified: the 8-bit video, the float SR frames of today's call on it, and the CPU
    oracle's SR frames 0 and 3 of the reflect-padded video, cropped and resized by resize_ref."""
    key = (h, w)
    if key not in _E2E:
        import torch.nn.functional as F
        from oracle import edvr as oedvr
        sd = synth.damp_residual_branch(synth.edvr_state_dict(0), 0.02)
        Hp, Wp = frames.padded_size(h, w, 4)
        u8 = (synth.clip(90 + h, 1, T, h, w)[0] * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # [T,h,w,3]
        flt = torch.from_numpy(np.ascontiguousarray(np.transpose(u8.numpy().astype(np.float32) / 255., (0, 3, 1, 2))))
        padded = F.pad(flt, (0, Wp - w, 0, Hp - h), mode='reflect')
        net = make_net(sd)
        today = run(net, u8.cuda(), out='float')
        oracle = {}
        for i in (0, 3):
            with torch.no_grad():
                yo = oedvr.edvr_forward(sd, padded[index_generation(i, T, 5, 'new_info')][None])[0, :, :4 * h, :4 * w]
            oracle[i] = ref.resize(yo.numpy(), SIZE)
        _E2E[key] = dict(net=net, u8=u8, today=today, oracle=oracle)
    return _E2E[key]


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("hw", [(18, 22), (13, 15)])
def test_video_at_a_target_size(hw, in_flight):
    h, w = hw
    case = e2e_case(h, w)
    net, u8, today = case['net'], case['u8'].cuda(), case['today']
    oh, ow = SIZE
    shapes = {None: (oh, ow, 3), 'float': (1, 3, oh, ow), 'nv12': (oh * 3 // 2, ow)}
    for out, layout in ((None, 'hwc_rgb'), ('float', 'chw'), ('nv12', 'nv12')):
        got = run(net, u8, in_flight=in_flight, out=out, out_size=SIZE)
        assert len(got) == T
        for i in range(T):
            assert tuple(got[i].shape) == shapes[out] and got[i].is_cuda, (out, i)
            want = frames.emit(today[i], 4 * h, 4 * w, layout, size=SIZE)
            assert same_bits(got[i], want[None] if out == 'float' else want), (out, i)
        if out == 'float':
            for i, yo in case['oracle'].items():
                y = got[i][0].cpu().numpy().astype(np.float64)
                e, d = relerr(torch.from_numpy(y), torch.from_numpy(yo)), float(np.abs(y - yo).max())
                print("%dx%d -> %dx%d in_flight %d frame %d: rel-L2 %.3e max-abs %.3e" % (4 * h, 4 * w, oh, ow, in_flight, i, e, d))
                assert e < 2e-4 and d < 1.6e-3, (i, e, d)
    # the SR frame's own size is no resize at all: today's frames, bit for bit
    for out in (None, 'float'):
        plain = run(net, u8, in_flight=in_flight, out=out)
        same = run(net, u8, in_flight=in_flight, out=out, out_size=(4 * h, 4 * w))
        assert all(same_bits(a, b) for a, b in zip(plain, same)), out
    assert all(same_bits(a, b) for a, b in zip(run(net, u8, in_flight=in_flight, out='float'), today))
    # CPU-resident frames as a list, and float frames in, take the same path
    listed = run(net, [case['u8'][i] for i in range(T)], in_flight=in_flight, out_size=SIZE)
    assert all(same_bits(a, frames.emit(b, 4 * h, 4 * w, 'hwc_rgb', size=SIZE)) for a, b in zip(listed, today))


def test_float_video_that_needs_no_padding_at_a_target_size():
    """Float planar frames of a size the network takes as it is: without out_size the fuse tape's own tensor is yielded."""
    net = e2e_case(18, 22)['net']
    video = synth.clip(5, 1, T, 16, 20)[0].cuda()
    today = run(net, video)
    got = run(net, video, out_size=(36, 50))
    assert all(g.shape == (1, 3, 36, 50) and torch.equal(g[0], frames.resize(t, 64, 80, (36, 50))) for g, t in zip(got, today))
    assert all(torch.equal(a, b) for a, b in zip(run(net, video, out_size=(64, 80)), today))


def test_non_edvr_network_at_a_target_size():
    """The `Mean` module of test_gpu_frame_io.py: the branch that builds the windows here and runs them through
    super_resolve_video."""
    class Mean(torch.nn.Module):
        nframes = 3

        def forward(self, x):
            return x.mean(1)

    u8 = torch.from_numpy(np.random.RandomState(11).randint(0, 256, (5, 7, 9, 3)).astype(np.uint8))
    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}

    def go(**kw):
        return [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), u8, padding='replicate', multiple=4, **kw)]
    flt = go(out='float')
    assert all(f.shape == (1, 3, 7, 9) for f in flt)
    for out, layout, shape in ((None, 'hwc_rgb', (10, 12, 3)), ('float', 'chw', (1, 3, 10, 12)), ('i420', 'i420', (15, 12))):
        got = go(out=out, out_size=(10, 12))
        assert len(got) == 5
        for g, f in zip(got, flt):
            want = frames.emit(f, 7, 9, layout, size=(10, 12))
            assert tuple(g.shape) == shape and same_bits(g, want[None] if out == 'float' else want), out
    assert all(same_bits(a, b) for a, b in zip(go(out_size=(7, 9)), go()))
