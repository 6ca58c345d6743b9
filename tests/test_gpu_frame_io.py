"""GPU: frames in and out of the video path (csrc/frame_io.hip, dynavsr_amd/frames.py, StreamPlan.extract_frame and the
uint8 / any-size arguments of adapt.super_resolve_frames).

Expected values come from torch and numpy on the CPU, the reference's own recipe: `x.astype(np.float32) / 255.` (data/util.py:82),
BGR -> RGB (:109), torch.nn.functional.pad(.., (0, pw, 0, ph), mode) and util.tensor2img.  Conversions are compared bit for
bit; the network's output against the CPU oracle at the project's forward bars (rel-L2 < 2e-4, max-abs < 1e-3); 1e-3 is 0.255
of an 8-bit level, so a quantised frame may differ from the quantised oracle by one level at most."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import relerr
from dynavsr_amd import adapt, engine, frames, synth
from dynavsr_amd.data.util import index_generation
from dynavsr_amd.utils import util

pytestmark = pytest.mark.gpu

SIZES = [((5, 7), (8, 8)), ((16, 16), (16, 16)), ((18, 22), (20, 24)), ((13, 15), (16, 16)), ((9, 6), (12, 8))]
KINDS = [('chw', 1), ('hwc_rgb', 3), ('hwc_bgr', 3), ('hwc_rgb', 4)]            # (layout, pixel stride)
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
SENTINEL = 0xA5


def cpu_ingest(img, layout, ph, pw, mode):
    """The reference's recipe for a uint8 [h,w,3|4] numpy image (or a float [3,h,w] tensor): fp32 [3,h+ph,w+pw]."""
    if layout == 'chw':
        x = img.clone()
    else:
        a = img[:, :, :3].astype(np.float32) / 255.
        if layout == 'hwc_bgr':
            a = a[:, :, [2, 1, 0]]
        x = torch.from_numpy(np.ascontiguousarray(np.transpose(a, (2, 0, 1))))
    return F.pad(x[None], (0, pw, 0, ph), mode=mode)[0]


def pitched_u8(img, extra=5, offset=3):
    """A GPU view holding `img` [h,w,ps] inside a larger buffer: odd base address, rows `extra` bytes apart."""
    h, w, ps = img.shape
    pitch = w * ps + extra
    buf = torch.full((offset + h * pitch + 16,), SENTINEL, dtype=torch.uint8, device='cuda')
    view = buf.as_strided((h, w, ps), (pitch, ps, 1), offset)
    view.copy_(torch.from_numpy(img))
    assert view.data_ptr() % 2 == 1
    return buf, view


@pytest.mark.parametrize("mode", ['reflect', 'replicate'])
@pytest.mark.parametrize("kind", KINDS, ids=lambda k: "%s-%d" % k)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s[0])
def test_ingest_bit_exact(size, kind, mode):
    (h, w), (Hp, Wp) = size
    layout, ps = kind
    assert frames.padded_size(h, w, 4) == (Hp, Wp)
    r = np.random.RandomState(h * 100 + w)
    if layout == 'chw':
        img = torch.from_numpy(r.uniform(-0.5, 1.5, (3, h, w)).astype(np.float32))
        pitch, plane = w + 3, h * (w + 3) + 5
        buf = torch.full((1 + 3 * plane,), float('nan'), device='cuda')
        src = buf.as_strided((3, h, w), (plane, pitch, 1), 1)                  # 4 bytes off a 16-byte boundary
        src.copy_(img)
        assert src.data_ptr() % 16 == 4
    else:
        vals = np.arange(h * w * ps) % 256                                     # every 8-bit value as often as it fits
        img = r.permutation(vals).astype(np.uint8).reshape(h, w, ps)
        if (h, w) == (16, 16):
            assert len(np.unique(img[:, :, :3])) == 256
        buf, src = pitched_u8(img)
    assert frames.describe(src, layout)[0].data_ptr() == src.data_ptr()         # passed by stride, not copied
    n = 3 * Hp * Wp
    big = torch.full((n + 256,), -7.0, device='cuda')
    out = big[:n].view(3, Hp, Wp)
    got = frames.ingest(src, layout, 4, mode, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = cpu_ingest(img, layout, Hp - h, Wp - w, mode)
    assert torch.equal(got.cpu(), want)
    assert bool((big[n:] == -7.0).all())                                       # nothing behind the destination
    fresh = frames.ingest(src, layout, 4, mode)                                # ... and the same into its own tensor
    assert fresh.shape == (3, Hp, Wp) and torch.equal(fresh.cpu(), want)


def test_ingest_from_the_host_and_other_multiples():
    r = np.random.RandomState(5)
    img = r.randint(0, 256, (9, 14, 3)).astype(np.uint8)
    host = torch.from_numpy(img)
    for m, mode in ((1, 'reflect'), (2, 'replicate'), (16, 'replicate'), (4, 'reflect')):
        Hp, Wp = frames.padded_size(9, 14, m)
        got = frames.ingest(host, 'hwc_bgr', m, mode)
        assert got.is_cuda and got.shape == (3, Hp, Wp)
        assert torch.equal(got.cpu(), cpu_ingest(img, 'hwc_bgr', Hp - 9, Wp - 14, mode)), (m, mode)


def emit_source(Hs, Ws, both_ranges):
    r = np.random.RandomState(Hs)
    x = r.uniform(-0.2, 1.2, 3 * Hs * Ws).astype(np.float32)
    ties = ((np.arange(255, dtype=np.float64) + 0.5) / 255).astype(np.float32)          # every tie of [0,1] ...
    x[:255] = ties
    if both_ranges:
        x[255:510] = (2 * (np.arange(255, dtype=np.float64) + 0.5) / 255 - 1).astype(np.float32)   # ... and of [-1,1]
    return torch.from_numpy(r.permutation(x).reshape(3, Hs, Ws))


@pytest.mark.parametrize("lohi", [(0.0, 1.0), (-1.0, 1.0)])
@pytest.mark.parametrize("layout", ['chw', 'hwc_rgb', 'hwc_bgr'])
@pytest.mark.parametrize("shape", [((8, 16), (7, 13)), ((8, 16), (8, 16)), ((80, 96), (72, 88))],
                         ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_emit_bit_exact(shape, layout, lohi):
    (Hs, Ws), (h, w) = shape
    host = emit_source(Hs, Ws, Hs > 8)
    sr = host.cuda()
    crop = host[:, :h, :w]
    if layout == 'chw':
        pitch, plane = w + 3, h * (w + 3) + 7
        buf = torch.full((1 + 3 * plane + 8,), 123.0, device='cuda')
        dst = buf.as_strided((3, h, w), (plane, pitch, 1), 1)
        want = crop
    else:
        pitch = 3 * w + 7
        buf = torch.full((3 + h * pitch + 16,), SENTINEL, dtype=torch.uint8, device='cuda')
        dst = buf.as_strided((h, w, 3), (pitch, 3, 1), 3)
        assert dst.data_ptr() % 2 == 1
        want = torch.from_numpy(util.tensor2img(crop.clone(), min_max=lohi, mode='rgb' if layout == 'hwc_rgb' else 'bgr'))
    got = frames.emit(sr, h, w, layout, lohi, out=dst)
    assert got.data_ptr() == dst.data_ptr()
    assert torch.equal(dst.cpu(), want)
    rest = buf.clone()
    rest.as_strided(dst.shape, dst.stride(), dst.storage_offset()).fill_(123.0 if layout == 'chw' else SENTINEL)
    assert bool((rest == (123.0 if layout == 'chw' else SENTINEL)).all())      # not a byte outside the crop
    own = frames.emit(sr[None], h, w, layout, lohi)                            # into a tensor of its own (aligned rows)
    assert own.is_contiguous() and torch.equal(own.cpu(), want)


def test_emit_is_the_image_of_frame_metrics():
    host = emit_source(8, 16, False)
    sr, gt = host.cuda(), torch.rand(3, 8, 16, device='cuda')
    img = util.frame_metrics(sr, gt, need_img=True)[2]
    assert np.array_equal(frames.emit(sr, 8, 16, 'hwc_rgb').cpu().numpy(), img)


def make_net(sd):
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    net = EDVR()
    net.load_state_dict(sd, strict=True)
    return net.cuda()


def test_extract_frame_is_ingest_then_extract():
    h, w, Hp, Wp = 18, 22, 20, 24
    net = make_net(synth.edvr_state_dict(0))
    leaves = net.ordered_parameters()
    plan = engine.StreamPlan(net._cfg(), Hp, Wp, 6)
    img = np.random.RandomState(3).randint(0, 256, (h, w, 3)).astype(np.uint8)
    _, src = pitched_u8(img)
    caches = []
    for fused in (True, False):
        cache = plan.new_cache(src.device)
        cache.view(torch.float32).fill_(float('nan'))
        if fused:
            plan.extract_frame(leaves, src, 2, cache, 'hwc_bgr', 'reflect')
        else:
            plan.extract(leaves, frames.ingest(src, 'hwc_bgr', 4, 'reflect'), 2, cache)
        torch.cuda.synchronize()
        caches.append(cache.view(torch.float32).view(6, -1).cpu())
    a, b = caches
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))          # the whole slot, gaps (NaN) included
    n_fea = 64 * (Hp * Wp + Hp * Wp // 4 + Hp * Wp // 16)                       # L1 | L2 | L3 | frame, NaN gaps between
    assert int(torch.isfinite(a[2]).sum()) == n_fea + 3 * Hp * Wp
    for s in (0, 1, 3, 4, 5):
        assert bool(torch.isnan(a[s]).all()) and bool(torch.isnan(b[s]).all()), s
    want = cpu_ingest(img, 'hwc_bgr', Hp - h, Wp - w, 'reflect').reshape(-1)
    assert torch.equal(a[2][torch.isfinite(a[2])][-want.numel():], want)        # the slot's last section is the padded frame


# ---- end to end ----------------------------------------------------------------------------------
T = 7
_E2E = {}


def e2e_case(h, w, mode):
    """Per (size, pad mode), computed once and never modified: the 8-bit video, the CPU-padded float video, today's float path
    on it (cropped) and the oracle's frames 0, 3 and 6 (cropped)."""
    key = (h, w, mode)
    if key not in _E2E:
        from oracle import edvr as oedvr
        sd = synth.damp_residual_branch(synth.edvr_state_dict(0), 0.02)
        Hp, Wp = frames.padded_size(h, w, 4)
        u8 = (synth.clip(90 + h, 1, T, h, w)[0] * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # [T,h,w,3]
        flt = torch.from_numpy(np.ascontiguousarray(np.transpose(u8.numpy().astype(np.float32) / 255., (0, 3, 1, 2))))
        padded = F.pad(flt, (0, Wp - w, 0, Hp - h), mode=mode)
        net = make_net(sd)
        today = [sr.clone()[:, :, :4 * h, :4 * w].contiguous()
                 for sr in adapt.super_resolve_frames(OPT, net, padded.cuda(), padding='new_info', in_flight=2)]
        oracle = {}
        for i in (0, 3, 6):
            with torch.no_grad():
                oracle[i] = oedvr.edvr_forward(sd, padded[index_generation(i, T, 5, 'new_info')][None])[:, :, :4 * h, :4 * w]
        _E2E[key] = dict(net=net, u8=u8, flt=flt, today=today, oracle=oracle)
    return _E2E[key]


def run(net, video, **kw):
    return [sr.clone() for sr in adapt.super_resolve_frames(OPT, net, video, padding='new_info', **kw)]


def check_against_oracle(case, flt_out, u8_out, what):
    for i, yo in case['oracle'].items():
        y = flt_out[i].cpu()
        e, d = relerr(y, yo), float((y - yo).abs().max())
        print("%s frame %d: rel-L2 %.3e max-abs %.3e" % (what, i, e, d))
        assert e < 2e-4 and d < 1e-3, (what, i, e, d)
        q = util.tensor2img(yo.clone(), mode='rgb')
        sat = float(((q == 0) | (q == 255)).mean())
        print("%s frame %d: %.4f of the oracle's bytes saturated, %d levels" % (what, i, sat, len(np.unique(q))))
        assert sat <= 0.01, (what, i, sat)                                      # quantisation is really exercised
        lv = np.abs(u8_out[i].cpu().numpy().astype(np.int32) - q.astype(np.int32)).max()
        assert lv <= 1, (what, i, lv)


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("hw", [(18, 22), (13, 15)])
def test_video_end_to_end(hw, in_flight):
    h, w = hw
    case = e2e_case(h, w, 'reflect')
    net, u8 = case['net'], case['u8']
    # (a) the float output of the 8-bit video: same kernels, same inputs as today's path on the CPU-padded video
    flt_out = run(net, u8.cuda(), in_flight=in_flight, out='float')
    assert len(flt_out) == T and all(o.shape == (1, 3, 4 * h, 4 * w) for o in flt_out)
    assert all(torch.equal(a, b) for a, b in zip(flt_out, case['today']))
    # (b) uint8 out, in the input's channel order; CPU-resident frames as a list
    rgb = run(net, [u8[i] for i in range(T)], in_flight=in_flight)
    bgr = run(net, u8.flip(-1).cuda(), in_flight=in_flight, layout='hwc_bgr')
    for i in range(T):
        assert rgb[i].dtype == torch.uint8 and rgb[i].shape == (4 * h, 4 * w, 3) and rgb[i].is_cuda
        assert np.array_equal(rgb[i].cpu().numpy(), util.tensor2img(flt_out[i].cpu(), mode='rgb')), i
        assert np.array_equal(bgr[i].cpu().numpy(), util.tensor2img(flt_out[i].cpu(), mode='bgr')), i
    forced = run(net, u8.cuda(), in_flight=in_flight, out='hwc_bgr')           # RGB in, BGR out
    assert all(torch.equal(a, b) for a, b in zip(forced, bgr))
    # (c) against the CPU oracle on the padded window
    check_against_oracle(case, flt_out, rgb, "%dx%d in_flight %d" % (h, w, in_flight))
    # (e) float frames of a size that is no multiple of 4 (refused before) take the same path
    odd = run(net, case['flt'].cuda(), in_flight=in_flight)
    assert all(torch.equal(a, b) for a, b in zip(odd, flt_out))
    # a fourth byte per pixel and a pitched view change nothing
    wide = torch.full((T, h + 2, w + 3, 4), SENTINEL, dtype=torch.uint8, device='cuda')
    wide[:, 1:h + 1, 2:w + 2, :3] = u8.cuda()
    view = wide[:, 1:h + 1, 2:w + 2]
    assert all(torch.equal(a, b) for a, b in zip(run(net, view, in_flight=in_flight), rgb))


@pytest.mark.parametrize("hw", [(18, 22), (13, 15)])
def test_video_replicate_padding(hw):
    h, w = hw
    case, other = e2e_case(h, w, 'replicate'), e2e_case(h, w, 'reflect')
    net, u8 = case['net'], case['u8']
    flt_out = run(net, u8.cuda(), out='float', pad_mode='replicate')
    assert all(torch.equal(a, b) for a, b in zip(flt_out, case['today']))
    assert not all(torch.equal(a, b) for a, b in zip(flt_out, other['today']))   # (d) a different result ...
    rgb = run(net, u8.cuda(), pad_mode='replicate')
    for i in range(T):
        assert np.array_equal(rgb[i].cpu().numpy(), util.tensor2img(flt_out[i].cpu(), mode='rgb')), i
    check_against_oracle(case, flt_out, rgb, "%dx%d replicate" % (h, w))          # ... equally checked


def test_non_edvr_network_takes_uint8_frames():
    """The `Mean` module of tests/test_gpu_stream.py's last test: frames.ingest per frame, the windows through
    super_resolve_video, frames.emit per result."""
    calls = []

    class Mean(torch.nn.Module):
        nframes = 3

        def forward(self, x):
            calls.append(tuple(x.shape))
            return x.mean(1)

    u8 = torch.from_numpy(np.random.RandomState(11).randint(0, 256, (5, 7, 9, 3)).astype(np.uint8))
    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    out = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), u8, padding='replicate', multiple=4)]
    assert len(out) == 5 and calls == [(1, 3, 3, 8, 12)] * 5
    padded = torch.stack([cpu_ingest(u8[i].numpy(), 'hwc_rgb', 1, 3, 'reflect') for i in range(5)])
    for i in range(5):
        want = padded[index_generation(i, 5, 3, 'replicate')][None].mean(1)[0, :, :7, :9]
        assert out[i].dtype == torch.uint8 and out[i].shape == (7, 9, 3)
        assert np.array_equal(out[i].cpu().numpy(), util.tensor2img(want.clone(), mode='rgb')), i
    flt = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), u8.cuda(), padding='replicate', out='float')]
    plain = [padded[i][:, :7, :9].contiguous().cuda() for i in range(5)]
    for i in range(5):                                                          # multiple = 1: no padding, odd width
        want = torch.stack([plain[j] for j in index_generation(i, 5, 3, 'replicate')])[None].mean(1)
        assert flt[i].shape == (1, 3, 7, 9) and torch.equal(flt[i], want), i
