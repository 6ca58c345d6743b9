"""GPU: YCbCr 4:2:0 frames in and out of the video path (csrc/frame_yuv.hip, the 'nv12' / 'i420' layouts of
dynavsr_amd/frames.py, StreamPlan.extract_frame and adapt.super_resolve_frames).

The yardstick is tests/yuv_ref.py, the arithmetic restated in fp64 numpy (test_yuv_host.py ties it to the reference's colour
functions).  Bars:
  ingest  max-abs <= 1e-6 against fp64.  A numpy-fp32 evaluation of the same formulas differs from fp64 by <= 1.7e-7 over 200 k
          random triples per matrix; at most 8 roundings of magnitudes <= 2.3 bound it under 1e-6.
  emit    a byte equals rint of the fp64 value wherever that value is farther than 1e-3 levels from a tie (an fp32 evaluation
          differs from fp64 by <= 3.2e-5 levels before rounding: a factor of 30) and is within 1 level elsewhere; at most 2 % of
          the bytes may sit inside that window, asserted on the fp64 values alone (0.2 - 0.6 % for uniform inputs).
  network the project's forward bars against the CPU oracle (rel-L2 < 2e-4, max-abs < 1e-3)."""
import itertools

import numpy as np
import pytest
import torch

import yuv_ref
from conftest import relerr
from dynavsr_amd import adapt, engine, frames, synth
from dynavsr_amd.data.util import index_generation
from dynavsr_amd.utils import util

pytestmark = pytest.mark.gpu

LAYOUTS = ['nv12', 'i420']
PAIRS = list(itertools.product(('bt601', 'bt709'), ('limited', 'full')))
# frame -> padded size: even and ragged in x | odd both ways (the last chroma row and column serve one luma row and column) |
# across the 256-pixel workgroup edge in x and the 8-row edge in y | no padding
SIZES = [((6, 10), (8, 12)), ((7, 9), (8, 12)), ((18, 262), (20, 264)), ((16, 16), (16, 16))]
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
SENTINEL = 0xA5
TIE, TIE_SHARE = 1e-3, 0.02


def random_planes(h, w, seed):
    """uint8 planes y [h,w], cb, cr [Hc,Wc] of seeded random bytes holding every value as often as it fits: out-of-gamut
    triples and the clamp are exercised."""
    hc, wc = (h + 1) // 2, (w + 1) // 2
    n = h * w + 2 * hc * wc
    v = np.random.RandomState(seed).permutation(np.arange(n) % 256).astype(np.uint8)
    if n >= 256:
        assert len(np.unique(v)) == 256
    return v[:h * w].reshape(h, w), v[h * w:h * w + hc * wc].reshape(hc, wc), v[h * w + hc * wc:].reshape(hc, wc)


def pitched(rows, row_bytes, offset, extra=5):
    """(buffer, [rows, row_bytes] view): rows `extra` bytes apart at an odd address inside a sentinel-filled GPU buffer."""
    pitch = row_bytes + extra
    buf = torch.full((offset + rows * pitch + 16,), SENTINEL, dtype=torch.uint8, device='cuda')
    view = buf.as_strided((rows, row_bytes), (pitch, 1), offset)
    assert view.data_ptr() % 2 == 1
    return buf, view


def pitched_planes(h, w, layout):
    """(buffers, planes) of an h x w frame: every plane a pitched view at an odd base address."""
    hc, wc = (h + 1) // 2, (w + 1) // 2
    by, y = pitched(h, w, 3)
    if layout == 'nv12':
        bc, c = pitched(hc, 2 * wc, 1, extra=3)
        return [by, bc], (y, c.as_strided((hc, wc, 2), (c.stride(0), 2, 1), c.storage_offset()))
    bu, u = pitched(hc, wc, 5, extra=4)
    bv, v = pitched(hc, wc, 7, extra=2)
    return [by, bu, bv], (y, u, v)


def gpu_planes(y, cb, cr, layout):
    bufs, planes = pitched_planes(y.shape[0], y.shape[1], layout)
    planes[0].copy_(torch.from_numpy(y))
    if layout == 'nv12':
        planes[1].copy_(torch.from_numpy(np.stack([cb, cr], -1)))
    else:
        planes[1].copy_(torch.from_numpy(cb))
        planes[2].copy_(torch.from_numpy(cr))
    return planes


def host_planes(y, cb, cr, layout):
    t = [torch.from_numpy(np.ascontiguousarray(a)) for a in (y, cb, cr)]
    return (t[0], torch.stack(t[1:], -1)) if layout == 'nv12' else tuple(t)


def check_ingest(size, layout, mode, matrix, yuv_range):
    (h, w), (Hp, Wp) = size
    assert frames.padded_size(h, w, 4) == (Hp, Wp)
    y, cb, cr = random_planes(h, w, 100 * h + w)
    planes = gpu_planes(y, cb, cr, layout)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(frames.describe_yuv(planes, layout, h, w)[0], planes))
    n = 3 * Hp * Wp
    big = torch.full((n + 256,), -7.0, device='cuda')
    out = big[:n].view(3, Hp, Wp)
    got = frames.ingest(planes, layout, 4, mode, out=out, matrix=matrix, yuv_range=yuv_range)
    assert got.data_ptr() == out.data_ptr()
    want = yuv_ref.ingest(y, cb, cr, Hp, Wp, mode, matrix, yuv_range)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print("ingest %s %dx%d %s %s/%s: max-abs %.2e" % (layout, h, w, mode, matrix, yuv_range, err))
    assert err <= 1e-6
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert bool((big[n:] == -7.0).all())                                       # nothing behind the destination
    fresh = frames.ingest(planes, layout, 4, mode, matrix=matrix, yuv_range=yuv_range)   # ... the same into its own tensor
    assert fresh.shape == (3, Hp, Wp) and torch.equal(fresh, got)
    if h % 2 == 0 and w % 2 == 0:                                              # ... and from the packed form
        packed = torch.from_numpy(yuv_ref.pack(y, cb, cr, layout)).cuda()
        assert torch.equal(frames.ingest(packed, layout, 4, mode, matrix=matrix, yuv_range=yuv_range), got)


@pytest.mark.parametrize("mode", ['reflect', 'replicate'])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s[0])
def test_ingest_against_fp64(size, layout, mode):
    check_ingest(size, layout, mode, 'bt601', 'limited')


@pytest.mark.parametrize("matrix,yuv_range", PAIRS[1:])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", [SIZES[1], SIZES[2]], ids=lambda s: "%dx%d" % s[0])
def test_ingest_matrices_and_ranges(size, layout, matrix, yuv_range):
    check_ingest(size, layout, 'reflect', matrix, yuv_range)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ingest_from_the_host_and_other_multiples(layout):
    y, cb, cr = random_planes(9, 14, 5)
    host, dev = host_planes(y, cb, cr, layout), gpu_planes(y, cb, cr, layout)
    for m in (1, 2, 16):
        Hp, Wp = frames.padded_size(9, 14, m)
        got = frames.ingest(host, layout, m, 'replicate')
        assert got.is_cuda and got.shape == (3, Hp, Wp)
        assert torch.equal(got, frames.ingest(dev, layout, m, 'replicate')), m           # the same bits as from the device
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - yuv_ref.ingest(y, cb, cr, Hp, Wp, 'replicate')).max())
        assert err <= 1e-6, (m, err)
    y, cb, cr = random_planes(8, 14, 6)                                                  # a packed frame in host memory
    packed = torch.from_numpy(yuv_ref.pack(y, cb, cr, layout))
    assert torch.equal(frames.ingest(packed, layout, 4, 'reflect'), frames.ingest(gpu_planes(y, cb, cr, layout), layout, 4, 'reflect'))


# ---- emit
EMIT_SHAPES = [((8, 16), (7, 13)), ((8, 16), (8, 16)), ((80, 96), (72, 88)), ((20, 264), (18, 262))]


def check_bytes(got, levels, what):
    """got: uint8 arrays; levels: their fp64 values before rounding.  Returns the share of bytes within TIE of a tie."""
    near_n = total = 0
    for g, v in zip(got, levels):
        assert g.shape == v.shape, (what, g.shape, v.shape)
        want, far = yuv_ref.to_bytes(v), yuv_ref.tie_distance(v) > TIE
        assert np.array_equal(g[far], want[far]), (what, int((g[far] != want[far]).sum()))
        assert int(np.abs(g.astype(np.int32) - want.astype(np.int32)).max()) <= 1, what
        near_n += int((~far).sum())
        total += v.size
    return near_n / total


def planes_to_numpy(planes, layout):
    p = [t.cpu().numpy() for t in planes]
    return (p[0], p[1][:, :, 0], p[1][:, :, 1]) if layout == 'nv12' else tuple(p)


def check_emit(shape, layout, lohi, matrix, yuv_range):
    (Hs, Ws), (h, w) = shape
    host = torch.from_numpy(np.random.RandomState(Hs + h).uniform(-0.2, 1.2, (3, Hs, Ws)).astype(np.float32))
    sr = host.cuda()
    levels = yuv_ref.emit(host.numpy(), h, w, lohi[0], lohi[1], matrix, yuv_range)
    share = sum(int((yuv_ref.tie_distance(v) <= TIE).sum()) for v in levels) / sum(v.size for v in levels)
    print("emit %s %dx%d of %dx%d [%g,%g] %s/%s: %.2f %% of the bytes within %g of a tie" % (
        layout, h, w, Hs, Ws, lohi[0], lohi[1], matrix, yuv_range, 100 * share, TIE))
    assert share <= TIE_SHARE                                                  # (on the fp64 values alone)
    bufs, planes = pitched_planes(h, w, layout)
    got = frames.emit(sr, h, w, layout, lohi, out=planes, matrix=matrix, yuv_range=yuv_range)
    assert got is planes
    assert check_bytes(planes_to_numpy(planes, layout), levels, (shape, layout, lohi)) == share
    for buf, p in zip(bufs, planes):                                            # not a byte outside the planes' rows
        rest = buf.clone()
        rest.as_strided(p.shape, p.stride(), p.storage_offset()).fill_(SENTINEL)
        assert bool((rest == SENTINEL).all())
    if h % 2 == 0 and w % 2 == 0:                                              # the packed result is the planes result
        packed = frames.emit(sr[None], h, w, layout, lohi, matrix=matrix, yuv_range=yuv_range)
        assert packed.dtype == torch.uint8 and packed.shape == (h * 3 // 2, w) and packed.is_contiguous()
        for a, b in zip(yuv_ref.unpack(packed.cpu().numpy(), layout), planes_to_numpy(planes, layout)):
            assert np.array_equal(a, b)
        into = torch.full((h * 3 // 2, w), SENTINEL, dtype=torch.uint8, device='cuda')
        assert frames.emit(sr, h, w, layout, lohi, out=into, matrix=matrix, yuv_range=yuv_range) is into
        assert torch.equal(into, packed)


@pytest.mark.parametrize("lohi", [(0.0, 1.0), (-1.0, 1.0)])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", EMIT_SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_emit_against_fp64(shape, layout, lohi):
    check_emit(shape, layout, lohi, 'bt601', 'limited')


@pytest.mark.parametrize("matrix,yuv_range", PAIRS[1:])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_emit_matrices_and_ranges(layout, matrix, yuv_range):
    check_emit(EMIT_SHAPES[0], layout, (0.0, 1.0), matrix, yuv_range)
    check_emit(EMIT_SHAPES[2], layout, (0.0, 1.0), matrix, yuv_range)


# ---- the stream plan
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
    y, cb, cr = random_planes(h, w, 3)
    for layout in LAYOUTS:
        src = gpu_planes(y, cb, cr, layout)
        caches = []
        for fused in (True, False):
            cache = plan.new_cache(src[0].device)
            cache.view(torch.float32).fill_(float('nan'))
            if fused:
                plan.extract_frame(leaves, src, 2, cache, layout, 'reflect')
            else:
                plan.extract(leaves, frames.ingest(src, layout, 4, 'reflect'), 2, cache)
            torch.cuda.synchronize()
            caches.append(cache.view(torch.float32).view(6, -1).cpu())
        a, b = caches
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))      # the whole slot, gaps (NaN) included
        n_fea = 64 * (Hp * Wp + Hp * Wp // 4 + Hp * Wp // 16)                   # L1 | L2 | L3 | frame, NaN gaps between
        assert int(torch.isfinite(a[2]).sum()) == n_fea + 3 * Hp * Wp
        for s in (0, 1, 3, 4, 5):
            assert bool(torch.isnan(a[s]).all()) and bool(torch.isnan(b[s]).all()), s
        want = yuv_ref.ingest(y, cb, cr, Hp, Wp, 'reflect').reshape(-1)
        raw = a[2][torch.isfinite(a[2])][-want.size:].numpy().astype(np.float64)  # the slot's last section is the padded frame
        assert float(np.abs(raw - want).max()) <= 1e-6


# ---- end to end
T = 7
_E2E = {}


def e2e_case(h, w, layout):
    """Per (size, layout), computed once and never modified: synth.clip content turned into 4:2:0 bytes by the restatement, the
    float path of today on the per-frame frames.ingest results (cropped) and the oracle's frames 0, 3 and 6 (cropped)."""
    key = (h, w, layout)
    if key not in _E2E:
        from oracle import edvr as oedvr
        sd = synth.damp_residual_branch(synth.edvr_state_dict(0), 0.02)
        Hp, Wp = frames.padded_size(h, w, 4)
        rgb = synth.clip(90 + h, 1, T, h, w)[0]                                                        # [T,3,h,w] in [0,1]
        planes = [tuple(yuv_ref.to_bytes(v) for v in yuv_ref.emit(rgb[i].numpy(), h, w)) for i in range(T)]
        if h % 2 == 0 and w % 2 == 0:
            video = torch.from_numpy(np.stack([yuv_ref.pack(*p, layout) for p in planes]))             # [T, h*3/2, w]
        else:
            video = [host_planes(*p, layout) for p in planes]
        net = make_net(sd)
        ingested = torch.stack([frames.ingest(video[i], layout, 4, 'reflect') for i in range(T)])
        today = [sr.clone()[:, :, :4 * h, :4 * w].contiguous()
                 for sr in adapt.super_resolve_frames(OPT, net, ingested, padding='new_info', in_flight=2)]
        padded = torch.from_numpy(np.stack([yuv_ref.ingest(*p, Hp, Wp, 'reflect') for p in planes]))
        assert float((ingested.cpu().double() - padded).abs().max()) <= 1e-6
        padded = padded.float()
        oracle = {}
        for i in (0, 3, 6):
            with torch.no_grad():
                oracle[i] = oedvr.edvr_forward(sd, padded[index_generation(i, T, 5, 'new_info')][None])[:, :, :4 * h, :4 * w]
        u8 = (rgb * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()                      # the same content as RGB
        _E2E[key] = dict(net=net, video=video, today=today, oracle=oracle, u8=u8)
    return _E2E[key]


def run(net, video, **kw):
    return [sr.clone() for sr in adapt.super_resolve_frames(OPT, net, video, padding='new_info', **kw)]


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("case", [(18, 22, 'nv12'), (13, 15, 'i420')], ids=lambda c: "%dx%d-%s" % c)
def test_video_end_to_end(case, in_flight):
    h, w, layout = case
    c = e2e_case(h, w, layout)
    net, video = c['net'], c['video']
    on_gpu = video.cuda() if torch.is_tensor(video) else video                  # (the planes of 13 x 15 stay on the host)
    # (a) the float output: same kernels, same inputs as today's float path on the per-frame frames.ingest results
    flt_out = run(net, on_gpu, in_flight=in_flight, layout=layout, out='float')
    assert len(flt_out) == T and all(o.shape == (1, 3, 4 * h, 4 * w) for o in flt_out)
    assert all(torch.equal(a, b) for a, b in zip(flt_out, c['today']))           # (whatever in_flight is)
    # (b) 4:2:0 out, in the input's layout: frames.emit of (a)
    yuv_out = run(net, video, in_flight=in_flight, layout=layout)
    for i in range(T):
        assert yuv_out[i].dtype == torch.uint8 and yuv_out[i].shape == (6 * h, 4 * w) and yuv_out[i].is_cuda
        assert torch.equal(yuv_out[i], frames.emit(flt_out[i], 4 * h, 4 * w, layout)), i
    other = 'i420' if layout == 'nv12' else 'nv12'
    forced = run(net, on_gpu, in_flight=in_flight, layout=layout, out=other, matrix='bt601', yuv_range='limited')
    for i in range(T):
        assert torch.equal(forced[i], frames.emit(flt_out[i], 4 * h, 4 * w, other)), i
    rgb = run(net, on_gpu, in_flight=in_flight, layout=layout, out='hwc_rgb')    # 4:2:0 in, RGB out
    for i in range(T):
        assert np.array_equal(rgb[i].cpu().numpy(), util.tensor2img(flt_out[i].cpu(), mode='rgb')), i
    u8 = c['u8'].cuda()                                                          # RGB in, 4:2:0 out
    from_rgb, from_rgb_flt = run(net, u8, in_flight=in_flight, out=layout), run(net, u8, in_flight=in_flight, out='float')
    for i in range(T):
        assert torch.equal(from_rgb[i], frames.emit(from_rgb_flt[i], 4 * h, 4 * w, layout)), i
    # (c) against the CPU oracle on the restated padded windows
    for i, yo in c['oracle'].items():
        y = flt_out[i].cpu()
        e, d = relerr(y, yo), float((y - yo).abs().max())
        print("%dx%d %s in_flight %d frame %d: rel-L2 %.3e max-abs %.3e" % (h, w, layout, in_flight, i, e, d))
        assert e < 2e-4 and d < 1e-3, (i, e, d)
        q = util.tensor2img(yo.clone(), mode='rgb')
        sat = float(((q == 0) | (q == 255)).mean())
        print("frame %d: %.4f of the oracle's bytes saturated" % (i, sat))
        assert sat <= 0.01, (i, sat)
        luma = yuv_ref.to_bytes(yuv_ref.emit(yo[0].numpy(), 4 * h, 4 * w)[0]).astype(np.int32)
        got = yuv_out[i][:4 * h].cpu().numpy().astype(np.int32)
        assert int(np.abs(got - luma).max()) <= 1, i


def test_non_edvr_network_takes_nv12_frames():
    """The `Mean` stand-in of test_gpu_frame_io.py: frames.ingest per frame, the windows through super_resolve_video,
    frames.emit per result."""
    calls = []

    class Mean(torch.nn.Module):
        nframes = 3

        def forward(self, x):
            calls.append(tuple(x.shape))
            return x.mean(1)

    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    planes = [random_planes(8, 10, 20 + i) for i in range(5)]
    video = torch.from_numpy(np.stack([yuv_ref.pack(*p, 'nv12') for p in planes]))                     # [5,12,10] on the host
    kw = dict(padding='replicate', multiple=4, layout='nv12', matrix='bt709', yuv_range='full')
    out = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), video, **kw)]
    flt = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), video.cuda(), out='float', **kw)]
    assert len(out) == 5 and calls == [(1, 3, 3, 8, 12)] * 10
    padded = np.stack([yuv_ref.ingest(*p, 8, 12, 'reflect', 'bt709', 'full') for p in planes])
    for i in range(5):
        want = padded[index_generation(i, 5, 3, 'replicate')].mean(0)[:, :8, :10]
        # three ingested values, each within 1e-6, and the three fp32 roundings of their mean (<= 6e-8 each)
        assert flt[i].shape == (1, 3, 8, 10) and float(np.abs(flt[i][0].cpu().numpy() - want).max()) <= 1.2e-6, i
        assert out[i].dtype == torch.uint8 and out[i].shape == (12, 10)
        assert torch.equal(out[i], frames.emit(flt[i], 8, 10, 'nv12', matrix='bt709', yuv_range='full')), i
        check_bytes(yuv_ref.unpack(out[i].cpu().numpy(), 'nv12'),
                    yuv_ref.emit(flt[i][0].cpu().numpy(), 8, 10, 0.0, 1.0, 'bt709', 'full'), i)
    odd = [host_planes(*random_planes(7, 9, 30 + i), 'nv12') for i in range(5)]                        # planes, odd both ways
    rgb = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), odd, padding='replicate', layout='nv12', out='hwc_rgb')]
    assert len(rgb) == 5 and all(o.shape == (7, 9, 3) and o.dtype == torch.uint8 for o in rgb)
