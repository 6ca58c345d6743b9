"""GPU: 16-bit RGB and planar integer RGB / GBR frames in and out of the video path (csrc/frame_rgb.hip through dvsr_frame_ingest /
dvsr_frame_emit, the new fetches of csrc/frame_cut.hip and csrc/frame_score.hip, frames.py, StreamPlan.extract_frame and
super_resolve_frames).

Every result is defined exactly (tests/rgb_ref.py: two fp32 formulas and np.pad), so every comparison is torch.equal /
np.array_equal; SSIM alone has a bar, the one of test_gpu_score.py.  The shapes are the smallest that reach each path of the
kernels: (5, 7) every lane ragged, (6, 261) two workgroups each way (64 lanes x 4 pixels, 4 rows) with a one-pixel tail,
(8, 256) whole lanes alone; a row pitch of one sample more than a row, so that consecutive rows change alignment class; every
base offset of a class; plane strides that are no multiple of 8 bytes; both pad modes to a multiple of 4."""
import math

import numpy as np
import pytest
import torch

import rgb_ref
import score_ref
from dynavsr_amd import adapt, engine, frames, synth

pytestmark = pytest.mark.gpu

SIZES = [(5, 7), (6, 261), (8, 256)]
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
CANARY = {np.dtype(np.uint8): 0xA5, np.dtype(np.uint16): 0xA5C3}


def tdtype(a):
    return torch.uint8 if a.dtype == np.uint8 else torch.uint16


def random_frame(layout, h, w, seed, ps=3, junk=True):
    """A numpy frame of random levels; the bits above a 10- / 12-bit level hold garbage."""
    r = np.random.RandomState(seed)
    planar, d, _ = rgb_ref.LAYOUTS[layout]
    lev = r.randint(0, 1 << d, (3, h, w))
    lev[:, 0, 0], lev[:, -1, -1] = 0, (1 << d) - 1
    return rgb_ref.from_levels(lev, layout, junk=r.randint(0, 65536, (3, h, w)) if junk and planar and 8 < d < 16 else None, ps=ps)


def strided(shape, layout, offset, device='cuda'):
    """(flat, view): a canary-filled flat tensor and a view of `shape` into it -- `offset` samples in, rows one sample longer than
    a row, planes (planar layouts) an odd number of samples apart, so no multiple of 8 bytes."""
    dt = np.dtype(rgb_ref.dtype(layout))
    if rgb_ref.LAYOUTS[layout][0]:
        _, h, w = shape
        row = w + 1
        plane = h * row + 3
        plane += 1 - plane % 2
        strides, n = (plane, row, 1), offset + 2 * plane + h * row + 5
    else:
        h, w, ps = shape
        row = w * ps + 1
        strides, n = (row, ps, 1), offset + h * row + 5
    flat = torch.full((n,), CANARY[dt], dtype=torch.uint8 if dt == np.uint8 else torch.uint16, device=device)
    return flat, flat.as_strided(shape, strides, offset)


def put(frame, layout, offset, device='cuda'):
    flat, view = strided(frame.shape, layout, offset, device)
    view.copy_(torch.from_numpy(frame).to(device))
    return view


@pytest.mark.parametrize("mode", ['reflect', 'replicate'])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", rgb_ref.NAMES)
def test_ingest_is_the_restatement(layout, size, mode):
    h, w = size
    Hp, Wp = frames.padded_size(h, w, 4)
    planar = rgb_ref.LAYOUTS[layout][0]
    for ps in ((3,) if planar else (3, 4)):
        frame = random_frame(layout, h, w, 7 * h + w, ps)
        want = torch.from_numpy(rgb_ref.ingest(frame, layout, Hp, Wp, mode))
        for offset in range(4):                                         # bytes 0 .. 3 / 0, 2, 4, 6
            src = put(frame, layout, offset)
            assert frames.describe(src, layout)[0].data_ptr() == src.data_ptr()      # by stride, not copied
            got = frames.ingest(src, layout, 4, mode)
            assert got.shape == (3, Hp, Wp) and torch.equal(got.cpu(), want), (ps, offset)
        if ps == 4:                                                     # a three-word view of four-word pixels
            assert torch.equal(frames.ingest(put(frame, layout, 1)[:, :, :3], layout, 4, mode).cpu(), want)
    # a CPU source goes to the device as it is and gives the same bits in `out`; int16 is the same bits
    out = torch.full((3, Hp, Wp), float('nan'), device='cuda')
    host = torch.from_numpy(frame)
    if host.dtype == torch.uint16:
        host = host.view(torch.int16)
    assert frames.ingest(host, layout, 4, mode, out=out) is out and torch.equal(out.cpu(), want)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_planar_bytes_ingest_as_interleaved_bytes_do(size):
    h, w = size
    frame = random_frame('chw_rgb8', h, w, 3)
    hwc = torch.from_numpy(np.ascontiguousarray(frame.transpose(1, 2, 0))).cuda()
    want = frames.ingest(hwc, 'hwc_rgb', 4, 'reflect')
    assert torch.equal(frames.ingest(torch.from_numpy(frame).cuda(), 'chw_rgb8', 4, 'reflect'), want)
    assert torch.equal(frames.ingest(put(frame[[1, 2, 0]], 'chw_gbr8', 3), 'chw_gbr8', 4, 'reflect'), want)


def emit_input(h, w, Hs, Ws, top, lo, hi, seed):
    """fp32 [3,Hs,Ws]: values beyond both ends of the range, exact ties (k + 0.5) / top mapped into it, and random ones."""
    r = np.random.RandomState(seed)
    x = (r.rand(3, Hs, Ws) * 1.5 - 0.25) * (hi - lo) + lo
    k = r.randint(0, top, (3, Hs, Ws))
    tie = (k + 0.5) / top * (hi - lo) + lo
    pick = r.rand(3, Hs, Ws) < 0.4
    x[pick] = tie[pick]
    x[:, 0, :4] = [lo - 1.0, hi + 1.0, lo, hi]
    return x.astype(np.float32)


@pytest.mark.parametrize("lohi", [(0.0, 1.0), (-1.0, 1.0)])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", rgb_ref.NAMES)
def test_emit_is_the_restatement_and_touches_nothing_else(layout, size, lohi):
    h, w = size
    Hs, Ws = frames.padded_size(h + 1, w + 2, 4)                        # the crop lies inside a larger frame
    lo, hi = lohi
    x = emit_input(h, w, Hs, Ws, rgb_ref.top(layout), lo, hi, 11 * h + w)
    want = torch.from_numpy(rgb_ref.emit(x, h, w, layout, lo, hi))
    sr = torch.from_numpy(x).cuda()
    got = frames.emit(sr, h, w, layout, min_max=lohi)
    assert got.dtype == tdtype(rgb_ref.emit(x, h, w, layout)) and got.shape == want.shape and torch.equal(got.cpu(), want)
    for offset in range(4):
        flat, view = strided(tuple(want.shape), layout, offset)
        before = flat.clone()
        assert frames.emit(sr, h, w, layout, min_max=lohi, out=view) is view
        assert torch.equal(view.cpu(), want), offset
        # the canaries in the pitch gaps, between the planes, in front of the frame and behind its last row
        view.zero_()
        before.as_strided(view.shape, view.stride(), offset).zero_()
        assert torch.equal(flat, before), offset
    if want.dtype == torch.uint16:                                      # int16 is the same bits
        out16 = torch.zeros(tuple(want.shape), dtype=torch.int16, device='cuda')
        frames.emit(sr, h, w, layout, min_max=lohi, out=out16)
        assert torch.equal(out16.view(torch.uint16).cpu(), want)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_depth_8_emits_the_bytes_of_hwc_rgb(size):
    h, w = size
    Hs, Ws = frames.padded_size(h, w, 4)
    sr = torch.from_numpy(emit_input(h, w, Hs, Ws, 255, 0.0, 1.0, 5)).cuda()
    hwc = frames.emit(sr, h, w, 'hwc_rgb')
    assert torch.equal(frames.emit(sr, h, w, 'chw_rgb8'), hwc.permute(2, 0, 1))
    assert torch.equal(frames.emit(sr, h, w, 'chw_gbr8'), hwc.permute(2, 0, 1)[[1, 2, 0]])


@pytest.mark.parametrize("layout", rgb_ref.NAMES)
def test_round_trip_of_every_level(layout):
    d = rgb_ref.LAYOUTS[layout][1]
    k = np.arange(65536, dtype=np.int64).reshape(256, 256)
    lev = np.stack([k, 65535 - k, (k * 40503) % 65536]) % (1 << d)    # every level in every channel
    assert all(len(np.unique(p)) == 1 << d for p in lev)
    frame = torch.from_numpy(rgb_ref.from_levels(lev, layout)).cuda()
    x = frames.ingest(frame, layout, 4, 'reflect')
    assert torch.equal(x.cpu(), torch.from_numpy(rgb_ref.ingest(frame.cpu().numpy(), layout, 256, 256)))
    assert torch.equal(frames.emit(x, 256, 256, layout), frame)


def make_net(sd):
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    net = EDVR()
    net.load_state_dict(sd, strict=True)
    return net.cuda()


_NET = {}


def net_case():
    """Computed once and never modified: EDVR-M with synthetic weights, 5 frames of 20 x 28 as hwc_rgb16 words, the float frames
    the restatement makes of them and the float path's outputs on those."""
    if not _NET:
        h, w, T = 20, 28, 5
        net = make_net(synth.damp_residual_branch(synth.edvr_state_dict(0), 0.02))
        rgb = synth.clip(31, 1, T, h, w)[0].numpy()                                                     # [T,3,h,w] in [0,1]
        words = np.stack([rgb_ref.emit(rgb[i], h, w, 'hwc_rgb16') for i in range(T)])                   # [T,h,w,3] uint16
        flt = torch.from_numpy(np.stack([rgb_ref.ingest(words[i], 'hwc_rgb16', h, w) for i in range(T)])).cuda()
        today = run(net, flt)
        _NET.update(net=net, h=h, w=w, T=T, words=torch.from_numpy(words), flt=flt, today=today,
                    u8=torch.from_numpy((rgb * 255).round().astype(np.uint8).transpose(0, 2, 3, 1).copy()))
    return _NET


def run(net, video, **kw):
    return [sr.clone() for sr in adapt.super_resolve_frames(OPT, net, video, padding='new_info', **kw)]


def test_frame_cache_takes_the_new_layouts():
    h, w, Hp, Wp = 18, 22, 20, 24
    net = net_case()['net']
    leaves = net.ordered_parameters()
    plan = engine.StreamPlan(net._cfg(), Hp, Wp, 6)
    for layout in ('chw_gbr10', 'hwc_rgb16'):
        frame = random_frame(layout, h, w, 9)
        src = put(frame, layout, 1)
        caches = []
        for fused in (True, False):
            cache = plan.new_cache(src.device)
            cache.view(torch.float32).fill_(float('nan'))
            if fused:
                plan.extract_frame(leaves, src, 2, cache, layout, 'reflect')
            else:
                plan.extract(leaves, frames.ingest(src, layout, 4, 'reflect'), 2, cache)
            torch.cuda.synchronize()
            caches.append(cache.view(torch.float32).view(6, -1).cpu())
        a, b = caches
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))      # the whole slot, gaps (NaN) included
        want = rgb_ref.ingest(frame, layout, Hp, Wp, 'reflect').reshape(-1)
        raw = a[2][torch.isfinite(a[2])][-want.size:].numpy()                   # the slot's last section is the padded frame
        assert np.array_equal(raw, want)
        for s in (0, 1, 3, 4, 5):
            assert bool(torch.isnan(a[s]).all()), s


def test_network_takes_and_yields_the_new_layouts():
    c = net_case()
    net, h, w, T = c['net'], c['h'], c['w'], c['T']
    flt_out = run(net, c['words'].cuda(), layout='hwc_rgb16', out='float')
    assert len(flt_out) == T and all(torch.equal(a, b) for a, b in zip(flt_out, c['today']))
    same = run(net, c['words'], layout='hwc_rgb16')                              # pinned or not, CPU words travel as words
    for i in range(T):
        assert same[i].dtype == torch.uint16 and same[i].shape == (4 * h, 4 * w, 3) and same[i].is_cuda
        assert torch.equal(same[i], frames.emit(flt_out[i], 4 * h, 4 * w, 'hwc_rgb16')), i
    u8 = c['u8'].cuda()                                                          # an 8-bit source leaves as gbrp10le
    from_u8, from_u8_flt = run(net, u8, out='chw_gbr10'), run(net, u8, out='float')
    for i in range(T):
        assert from_u8[i].dtype == torch.uint16 and from_u8[i].shape == (3, 4 * h, 4 * w)
        assert torch.equal(from_u8[i], frames.emit(from_u8_flt[i], 4 * h, 4 * w, 'chw_gbr10')), i
        assert int(from_u8[i].cpu().numpy().max()) <= 1023


def test_tiles_and_out_size_behind_the_new_layouts():
    c = net_case()
    net, h, w, T = c['net'], c['h'], c['w'], c['T']
    planes = torch.from_numpy(np.stack([rgb_ref.from_levels(rgb_ref.levels(f, 'hwc_rgb16') >> 4, 'chw_rgb12')
                                        for f in c['words'].numpy()])).cuda()       # the same video as 12-bit planes
    tiled = run(net, planes, layout='chw_rgb12', tile=(16, 16), tile_overlap=4)
    tiled_f = run(net, planes, layout='chw_rgb12', out='float', tile=(16, 16), tile_overlap=4)
    for i in range(T):
        assert tiled[i].shape == (3, 4 * h, 4 * w) and torch.equal(tiled[i], frames.emit(tiled_f[i], 4 * h, 4 * w, 'chw_rgb12')), i
    size = (3 * h, 3 * w + 1)
    words = c['words'].cuda()
    sized = run(net, words, layout='hwc_rgb16', out_size=size)
    flt = run(net, words, layout='hwc_rgb16', out='float')
    for i in range(T):
        assert sized[i].shape == size + (3,)
        assert torch.equal(sized[i], frames.emit(frames.resize(flt[i], 4 * h, 4 * w, size), size[0], size[1], 'hwc_rgb16')), i


def test_non_edvr_network_takes_the_new_layouts():
    calls = []

    class Mean(torch.nn.Module):
        nframes = 3

        def forward(self, x):
            calls.append(tuple(x.shape))
            return x.mean(1)

    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    video = [random_frame('hwc_rgb16', 7, 10, 40 + i) for i in range(5)]
    host = torch.from_numpy(np.stack(video))
    kw = dict(padding='replicate', multiple=4, layout='hwc_rgb16')
    out = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), host, **kw)]
    flt = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), host.cuda(), out='float', **kw)]
    assert len(out) == 5 and calls == [(1, 3, 3, 8, 12)] * 10
    padded = torch.stack([frames.ingest(host[i], 'hwc_rgb16', 4, 'reflect') for i in range(5)])
    assert torch.equal(padded.cpu(), torch.from_numpy(np.stack([rgb_ref.ingest(f, 'hwc_rgb16', 8, 12) for f in video])))
    for i in range(5):
        assert out[i].dtype == torch.uint16 and out[i].shape == (7, 10, 3)
        assert torch.equal(out[i], frames.emit(flt[i], 7, 10, 'hwc_rgb16')), i


def test_luma_sad_takes_the_top_eight_bits():
    h, w = 37, 261                                                      # two workgroups in y (32 rows each) and in x
    video = np.stack([random_frame('chw_rgb16', h, w, 60 + i) for i in range(3)])
    want = rgb_ref.luma_sad(video, 'chw_rgb16')
    dev = torch.from_numpy(video).cuda()
    assert frames.luma_sad(dev, 'chw_rgb16').tolist() == want                        # one launch over both pairs
    assert frames.luma_sad([torch.from_numpy(f) for f in video], 'chw_rgb16').tolist() == want    # CPU frames, a launch per pair
    top8 = torch.from_numpy(np.ascontiguousarray((video >> 8).astype(np.uint8).transpose(0, 2, 3, 1))).cuda()
    assert frames.luma_sad(top8, 'hwc_rgb').tolist() == want
    for layout in ('hwc_bgr16', 'chw_gbr10', 'chw_gbr8'):                            # the other fetches, pitched and offset
        vid = [random_frame(layout, h, w, 70 + i, ps=4) for i in range(2)]       # (four words a pixel where interleaved)
        got = frames.luma_sad([put(f, layout, 1) for f in vid], layout).tolist()
        assert got == rgb_ref.luma_sad(vid, layout), layout
    assert frames.detect_cuts(dev, 'chw_rgb16', threshold=1.0) == frames.detect_cuts(top8, 'hwc_rgb', threshold=1.0)


def check_score(got, sa, sb, depth, what):
    """got [mse, ssim] against score_ref on the sample arrays: mse exactly, SSIM at test_gpu_score.py's bar."""
    sse, n, mse, ssim = score_ref.score(sa, sb, 0, depth)
    bar = 1e-10
    host = abs(ssim - score_ref.score(sa, sb, 0, depth, separable=False)[3])       # separable vs 2-D window, both on the CPU
    print("%s: separable vs window form on the host %.3e" % (what, host))
    if host > 1e-11:
        bar = 10 * host
    m, s = float(got[0]), float(got[1])
    print("%s: sse %d over %d samples, ssim %.15f (reference %.15f, bar %.1e)" % (what, sse, n, s, ssim, bar))
    assert m == sse / n, (what, m, sse / n)
    assert abs(s - ssim) <= bar, (what, s, ssim, bar)


def test_score_on_the_levels():
    h, w = 29, 45                                                       # two tiles each way, owned tails
    r = np.random.RandomState(5)
    a = random_frame('hwc_rgb16', h, w, 80, ps=4)
    noise = r.randint(-900, 901, (3, h, w))
    b = rgb_ref.from_levels(np.clip(rgb_ref.levels(a, 'hwc_rgb16') + noise, 0, 65535), 'chw_rgb16')
    b[:, 3, 5] = 65535 - rgb_ref.levels(a, 'hwc_rgb16')[:, 3, 5]       # one difference near full scale
    sa, sb = (rgb_ref.levels(f, lay).transpose(1, 2, 0) for f, lay in ((a, 'hwc_rgb16'), (b, 'chw_rgb16')))
    got = frames.score(put(a, 'hwc_rgb16', 3), put(b, 'chw_rgb16', 1), 'hwc_rgb16', 'chw_rgb16').cpu()
    check_score(got, sa, sb, 16, "hwc_rgb16 against chw_rgb16")
    # full-scale differences everywhere: 3 * 65535^2 per pixel is beyond 32 bits
    zero, full = np.zeros((h, w, 3), dtype=np.uint16), np.full((3, h, w), 65535, dtype=np.uint16)
    m = frames.score(torch.from_numpy(zero).cuda(), torch.from_numpy(full), 'hwc_bgr16', 'chw_gbr16').tolist()[0]
    assert m == 65535.0 ** 2
    # depth 10 against an fp32 frame, which is quantised at depth 10
    g = random_frame('chw_gbr10', h, w, 81)
    x = emit_input(h, w, h, w, 1023, 0.0, 1.0, 82)
    x = (0.9 * rgb_ref.ingest(g, 'chw_gbr10', h, w) + 0.1 * x).astype(np.float32)
    sg, sx = rgb_ref.levels(g, 'chw_gbr10').transpose(1, 2, 0), rgb_ref.quant(x, 1023).transpose(1, 2, 0)
    got = frames.score(put(g, 'chw_gbr10', 2), torch.from_numpy(x).cuda(), 'chw_gbr10', 'chw').cpu()
    check_score(got, sg, sx, 10, "chw_gbr10 against fp32")
    # a planar 8-bit side pairs with any other 8-bit side, in either channel
    p8 = random_frame('chw_gbr8', h, w, 83)
    u8 = np.ascontiguousarray(np.clip(rgb_ref.levels(p8, 'chw_gbr8') + r.randint(-9, 10, (3, h, w)), 0, 255).astype(np.uint8).transpose(1, 2, 0))
    got = frames.score(torch.from_numpy(p8).cuda(), torch.from_numpy(u8).cuda(), 'chw_gbr8', 'hwc_rgb').cpu()
    check_score(got, rgb_ref.levels(p8, 'chw_gbr8').transpose(1, 2, 0), u8.astype(np.int64), 8, "chw_gbr8 against hwc_rgb")
    want_y = frames.score(torch.from_numpy(np.ascontiguousarray(rgb_ref.levels(p8, 'chw_gbr8').astype(np.uint8).transpose(1, 2, 0))).cuda(),
                          torch.from_numpy(u8).cuda(), channel='y')
    assert torch.equal(frames.score(torch.from_numpy(p8).cuda(), torch.from_numpy(u8).cuda(), 'chw_gbr8', 'hwc_rgb', channel='y'), want_y)
    with pytest.raises(ValueError, match="channel='y'"):
        frames.score(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 'hwc_rgb16', 'chw_rgb16', channel='y')
    with pytest.raises(ValueError, match="mixed bit depths"):
        frames.score(torch.from_numpy(a).cuda(), torch.from_numpy(g).cuda(), 'hwc_rgb16', 'chw_gbr10')


def test_scores_of_a_video_against_16_bit_ground_truth():
    c = net_case()
    net, h, w, T = c['net'], c['h'], c['w'], c['T']
    r = np.random.RandomState(6)
    gt = torch.from_numpy(r.randint(0, 65536, (T, 3, 4 * h, 4 * w)).astype(np.uint16))
    scores = torch.zeros((T, 2), dtype=torch.float64, device='cuda')
    out = [o.clone() for o in adapt.super_resolve_frames(OPT, net, c['words'], padding='new_info', layout='hwc_rgb16', gt=gt,
                                                         gt_layout='chw_rgb16', scores=scores)]
    for i in range(T):
        want = frames.score(out[i], gt[i], 'hwc_rgb16', 'chw_rgb16')
        assert torch.equal(scores[i], want), i
        sa = rgb_ref.levels(out[i].cpu().numpy(), 'hwc_rgb16').transpose(1, 2, 0)
        assert float(scores[i][0]) == score_ref.sse(sa, gt[i].numpy().astype(np.int64).transpose(1, 2, 0)) / sa.size
    summary, _ = adapt.evaluate_frames(OPT, net, c['words'], gt, layout='hwc_rgb16', gt_layout='chw_rgb16')
    assert math.isclose(summary['mean']['psnr'], sum(frames.psnr(float(m), 65535) for m in scores[:, 0].tolist()) / T, rel_tol=1e-12)


def test_degrade_and_imresize_go_through_ingest():
    frame = random_frame('chw_gbr12', 24, 30, 90)
    x = frames.ingest(torch.from_numpy(frame).cuda(), 'chw_gbr12', 1, 'replicate')
    assert torch.equal(frames.imresize(torch.from_numpy(frame), 0.5, 'chw_gbr12'), frames.imresize(x, 0.5, 'chw'))
    assert torch.equal(frames.degrade(torch.from_numpy(frame), frames.Imresize(2), 'chw_gbr12'), frames.degrade(x, frames.Imresize(2), 'chw'))
