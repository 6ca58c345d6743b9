"""GPU: 10- and 12-bit YCbCr 4:2:0 frames in and out of the video path (csrc/frame_yuv.hip, the 'p010' / 'p012' / 'i420p10' /
'i420p12' layouts of dynavsr_amd/frames.py, StreamPlan.extract_frame, adapt.super_resolve_frames) and the 16-bit Y planes of
dvsr_frame_luma_sad (csrc/frame_cut.hip).

The yardstick is tests/yuv16_ref.py, the arithmetic restated in fp64 numpy (test_yuv16_host.py ties it to the 8-bit restatement
and to H.273's anchor points).  Bars:
  ingest  max-abs <= 1e-6 against fp64, the 8-bit bar.  A numpy-fp32 evaluation of the kernel's formulas (reciprocals formed in
          double, rounded once) differs from fp64 by <= 2.6e-7 over 200 k triples per depth, matrix and range.
  emit    a word equals rint of the fp64 value wherever that value is farther than TIE from a tie and is within 1 level
          elsewhere; TIE = 4e-3 levels at 10 bits, 8e-3 at 12 (the same numpy-fp32 evaluation differs from fp64 by <= 1.5e-4 and
          <= 6.0e-4 levels before rounding: factors of 27 and 13); at most 2 % / 2.5 % of the samples may sit inside that window,
          asserted on the fp64 values alone.
  luma    sums of integers: exact."""
import itertools

import numpy as np
import pytest
import torch

import cut_ref
import yuv16_ref as ref
from dynavsr_amd import adapt, engine, frames, synth
from dynavsr_amd.data.util import index_generation
from dynavsr_amd.utils import util

pytestmark = pytest.mark.gpu

LAYOUTS = ['p010', 'p012', 'i420p10', 'i420p12']
PAIRS = list(itertools.product(('bt601', 'bt709'), ('limited', 'full')))
# frame -> padded size: even and ragged in x | odd both ways (the last chroma row and column serve one luma row and column) |
# across the 256-pixel workgroup edge in x and the 8-row edge in y | no padding
SIZES = [((6, 10), (8, 12)), ((7, 9), (8, 12)), ((18, 262), (20, 264)), ((16, 16), (16, 16))]
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
SENTINEL = 0x5A5A
TIE = {10: 4e-3, 12: 8e-3}
TIE_SHARE = {10: 0.02, 12: 0.025}


def same(a, b):
    """Bit equality of two tensors of 16-bit words (uint16 or int16) or of anything else."""
    if a.dtype in (torch.uint16, torch.int16):
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.shape == b.shape and torch.equal(a, b)


def semi(layout):
    return ref.LAYOUTS[layout][0] == 'msb'


def random_levels(h, w, depth, seed):
    """Level planes y [h,w], cb, cr [Hc,Wc] of seeded uniform random levels: 0, 2^d - 1 and out-of-gamut triples occur (the
    clamp is exercised)."""
    hc, wc = (h + 1) // 2, (w + 1) // 2
    r = np.random.RandomState(seed)
    planes = [r.randint(0, 2 ** depth, s) for s in ((h, w), (hc, wc), (hc, wc))]
    for p in planes:
        flat = p.reshape(-1)
        flat[r.permutation(flat.size)[:4]] = [0, 2 ** depth - 1, 0, 2 ** depth - 1]
    return planes


def words_of(levels, layout, garbage_seed=None):
    storage, depth = ref.LAYOUTS[layout]
    out = []
    for i, p in enumerate(levels):
        g = None if garbage_seed is None else np.random.RandomState(garbage_seed + i).randint(0, 65536, p.shape)
        out.append(ref.to_words(p, storage, depth, g))
    return out


def pitched(rows, row_words, offset, extra=3):
    """(buffer, [rows, row_words] view): rows `extra` words apart, at an address that is 2- but not 4-byte aligned, inside a
    sentinel-filled int16 GPU buffer."""
    assert offset % 2 == 1
    pitch = row_words + extra
    buf = torch.full((offset + rows * pitch + 16,), SENTINEL, dtype=torch.int16, device='cuda')
    view = buf.as_strided((rows, row_words), (pitch, 1), offset)
    assert view.data_ptr() % 4 == 2
    return buf, view


def pitched_planes(h, w, layout, dtype=torch.uint16):
    """(buffers, planes) of an h x w frame: every plane a pitched view at a 2- but not 4-byte aligned base address."""
    hc, wc = (h + 1) // 2, (w + 1) // 2
    by, y = pitched(h, w, 3)
    if semi(layout):
        bc, c = pitched(hc, 2 * wc, 1, extra=5)
        planes = (y, c.as_strided((hc, wc, 2), (c.stride(0), 2, 1), c.storage_offset()))
        return [by, bc], tuple(p.view(dtype) for p in planes)
    bu, u = pitched(hc, wc, 5, extra=4)
    bv, v = pitched(hc, wc, 7, extra=1)
    return [by, bu, bv], tuple(p.view(dtype) for p in (y, u, v))


def fill(planes, words, layout):
    """Copies numpy uint16 word planes (y, cb, cr) into GPU planes."""
    src = [words[0], np.stack(words[1:], -1)] if semi(layout) else list(words)
    for p, s in zip(planes, src):
        p.view(torch.int16).copy_(torch.from_numpy(np.ascontiguousarray(s).view(np.int16)))
    return planes


def gpu_planes(words, layout, dtype=torch.uint16):
    return fill(pitched_planes(words[0].shape[0], words[0].shape[1], layout, dtype)[1], words, layout)


def host_planes(words, layout):
    t = [torch.from_numpy(np.ascontiguousarray(a)) for a in words]
    return (t[0], torch.from_numpy(np.ascontiguousarray(np.stack(words[1:], -1)))) if semi(layout) else tuple(t)


def check_ingest(size, layout, mode, matrix, yuv_range):
    (h, w), (Hp, Wp) = size
    depth = ref.LAYOUTS[layout][1]
    assert frames.padded_size(h, w, 4) == (Hp, Wp)
    levels = random_levels(h, w, depth, 100 * h + w + depth)
    words = words_of(levels, layout)
    planes = gpu_planes(words, layout)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(frames.describe_yuv(planes, layout, h, w)[0], planes))
    n = 3 * Hp * Wp
    big = torch.full((n + 256,), -7.0, device='cuda')
    out = big[:n].view(3, Hp, Wp)
    got = frames.ingest(planes, layout, 4, mode, out=out, matrix=matrix, yuv_range=yuv_range)
    assert got.data_ptr() == out.data_ptr()
    want = ref.ingest(*levels, Hp, Wp, depth, mode, matrix, yuv_range)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print("ingest %s %dx%d %s %s/%s: max-abs %.2e" % (layout, h, w, mode, matrix, yuv_range, err))
    assert err <= 1e-6
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert bool((big[n:] == -7.0).all())                                       # nothing behind the destination
    fresh = frames.ingest(planes, layout, 4, mode, matrix=matrix, yuv_range=yuv_range)   # ... the same into its own tensor
    assert fresh.shape == (3, Hp, Wp) and torch.equal(fresh, got)
    kw = dict(matrix=matrix, yuv_range=yuv_range)
    assert torch.equal(frames.ingest(host_planes(words, layout), layout, 4, mode, **kw), got)        # planes in host memory
    assert torch.equal(frames.ingest(tuple(p.view(torch.int16) for p in planes), layout, 4, mode, **kw), got)   # int16: same bits
    if h % 2 == 0 and w % 2 == 0:                                              # ... and from the packed form, host and device
        packed = torch.from_numpy(ref.pack(*words, layout))
        assert packed.dtype == torch.uint16
        assert torch.equal(frames.ingest(packed, layout, 4, mode, **kw), got)
        assert torch.equal(frames.ingest(packed.cuda(), layout, 4, mode, **kw), got)
    return got, levels


@pytest.mark.parametrize("mode", ['reflect', 'replicate'])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s[0])
def test_ingest_against_fp64(size, layout, mode):
    check_ingest(size, layout, mode, 'bt601', 'limited')


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", [SIZES[1], SIZES[2]], ids=lambda s: "%dx%d" % s[0])
def test_ingest_bt709_full(size, layout):
    check_ingest(size, layout, 'reflect', 'bt709', 'full')


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ingest_ignores_the_bits_that_carry_no_level(layout):
    (h, w), (Hp, Wp) = SIZES[2]
    depth = ref.LAYOUTS[layout][1]
    levels = random_levels(h, w, depth, 7)
    clean, dirty = words_of(levels, layout), words_of(levels, layout, garbage_seed=11)
    assert all(not np.array_equal(a, b) for a, b in zip(clean, dirty))
    a = frames.ingest(gpu_planes(clean, layout), layout, 4, 'reflect')
    b = frames.ingest(gpu_planes(dirty, layout), layout, 4, 'reflect')
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(np.abs(b.cpu().numpy().astype(np.float64) - ref.ingest(*levels, Hp, Wp, depth, 'reflect')).max()) <= 1e-6


@pytest.mark.parametrize("layout", ['p010', 'i420p12'])
def test_ingest_other_multiples(layout):
    depth = ref.LAYOUTS[layout][1]
    levels = random_levels(9, 14, depth, 5)
    words = words_of(levels, layout)
    host, dev = host_planes(words, layout), gpu_planes(words, layout)
    for m in (1, 2, 16):
        Hp, Wp = frames.padded_size(9, 14, m)
        got = frames.ingest(host, layout, m, 'replicate')
        assert got.is_cuda and got.shape == (3, Hp, Wp)
        assert torch.equal(got, frames.ingest(dev, layout, m, 'replicate')), m
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref.ingest(*levels, Hp, Wp, depth, 'replicate')).max())
        assert err <= 1e-6, (m, err)


# ---- emit
EMIT_SHAPES = [((8, 16), (7, 13)), ((8, 16), (8, 16)), ((80, 96), (72, 88)), ((20, 264), (18, 262))]


def check_words(got, levels, layout, what):
    """got: uint16 word arrays; levels: their fp64 values before rounding.  Returns the share of samples within TIE of a tie."""
    storage, depth = ref.LAYOUTS[layout]
    near_n = total = 0
    for g, v in zip(got, levels):
        assert g.shape == v.shape, (what, g.shape, v.shape)
        lev, rest = ref.from_words(g, storage, depth)
        assert int(rest.max()) == 0, (what, "the bits that carry no level must be written as 0")
        want, far = ref.to_levels(v, depth), ref.tie_distance(v, depth) > TIE[depth]
        assert np.array_equal(lev[far], want[far]), (what, int((lev[far] != want[far]).sum()))
        assert int(np.abs(lev.astype(np.int32) - want.astype(np.int32)).max()) <= 1, what
        near_n += int((~far).sum())
        total += v.size
    return near_n / total


def planes_to_numpy(planes, layout):
    p = [t.view(torch.int16).cpu().numpy().view(np.uint16) for t in planes]
    return (p[0], p[1][:, :, 0], p[1][:, :, 1]) if semi(layout) else tuple(p)


def emit_input(shape, layout, lohi, matrix, yuv_range):
    """(host fp32 [3,Hs,Ws], its fp64 levels, the share of them inside the tie window): the first seed whose fp64 levels keep
    the share under the cap -- a property of the input alone, decided before the device is asked anything."""
    (Hs, Ws), (h, w) = shape
    depth = ref.LAYOUTS[layout][1]
    for seed in range(Hs + h, Hs + h + 50):
        host = np.random.RandomState(seed).uniform(-0.2, 1.2, (3, Hs, Ws)).astype(np.float32)
        levels = ref.emit(host, h, w, depth, lohi[0], lohi[1], matrix, yuv_range)
        share = sum(int((ref.tie_distance(v, depth) <= TIE[depth]).sum()) for v in levels) / sum(v.size for v in levels)
        if share <= TIE_SHARE[depth]:
            return torch.from_numpy(host), levels, share
    raise AssertionError("no input under the cap")


def check_emit(shape, layout, lohi, matrix, yuv_range):
    (Hs, Ws), (h, w) = shape
    depth = ref.LAYOUTS[layout][1]
    host, levels, share = emit_input(shape, layout, lohi, matrix, yuv_range)
    print("emit %s %dx%d of %dx%d [%g,%g] %s/%s: %.2f %% of the samples within %g of a tie" % (
        layout, h, w, Hs, Ws, lohi[0], lohi[1], matrix, yuv_range, 100 * share, TIE[depth]))
    assert share <= TIE_SHARE[depth]                                            # (on the fp64 values alone)
    sr = host.cuda()
    bufs, planes = pitched_planes(h, w, layout)
    got = frames.emit(sr, h, w, layout, lohi, out=planes, matrix=matrix, yuv_range=yuv_range)
    assert got is planes
    assert check_words(planes_to_numpy(planes, layout), levels, layout, (shape, layout, lohi)) == share
    for buf, p in zip(bufs, planes):                                            # not a byte outside the planes' rows
        rest = buf.clone()
        rest.as_strided(p.shape, p.stride(), p.storage_offset() - buf.storage_offset()).fill_(SENTINEL)
        assert bool((rest == SENTINEL).all())
    if h % 2 == 0 and w % 2 == 0:                                              # the packed result is the planes result
        packed = frames.emit(sr[None], h, w, layout, lohi, matrix=matrix, yuv_range=yuv_range)
        assert packed.dtype == torch.uint16 and packed.shape == (h * 3 // 2, w) and packed.is_contiguous()
        for a, b in zip(ref.unpack(packed.view(torch.int16).cpu().numpy().view(np.uint16), layout), planes_to_numpy(planes, layout)):
            assert np.array_equal(a, b)
        into = torch.full((h * 3 // 2, w), SENTINEL, dtype=torch.int16, device='cuda')
        assert frames.emit(sr, h, w, layout, lohi, out=into, matrix=matrix, yuv_range=yuv_range) is into
        assert same(into, packed)


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


@pytest.mark.parametrize("layout", ['p010', 'i420p10'])
def test_ten_bits_survive_the_round_trip(layout):
    """An achromatic limited-range frame holding every 10-bit luma level 64 .. 940: emit(ingest(x)) returns the same words.
    Anything that passes through 8 bits on the way keeps a quarter of them."""
    h = w = 30
    y = (64 + np.arange(h * w) % 877).reshape(h, w)
    assert set(y.reshape(-1).tolist()) == set(range(64, 941))
    c = np.full((15, 15), 512)
    words = words_of((y, c, c), layout)
    packed = torch.from_numpy(ref.pack(*words, layout)).cuda()
    x = frames.ingest(packed, layout, 4, 'reflect')
    assert x.shape == (3, 32, 32)
    back = frames.emit(x, h, w, layout)
    assert back.dtype == torch.uint16 and same(back, packed)
    eight = frames.ingest(frames.emit(x, h, w, 'nv12' if semi(layout) else 'i420'), 'nv12' if semi(layout) else 'i420', 4, 'reflect')
    assert not same(frames.emit(eight, h, w, layout), packed)                   # (the comparison can tell)


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
    for layout in ('p010', 'i420p12'):
        depth = ref.LAYOUTS[layout][1]
        levels = random_levels(h, w, depth, 3)
        src = gpu_planes(words_of(levels, layout), layout)
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
        want = ref.ingest(*levels, Hp, Wp, depth, 'reflect').reshape(-1)
        raw = a[2][torch.isfinite(a[2])][-want.size:].numpy().astype(np.float64)  # the slot's last section is the padded frame
        assert float(np.abs(raw - want).max()) <= 1e-6


# ---- end to end
T = 7
_E2E = {}


def e2e_case(h, w, layout):
    """Per (size, layout), computed once and never modified: synth.clip content turned into 10-bit words by the restatement and
    the float path of today on the per-frame frames.ingest results (cropped)."""
    key = (h, w, layout)
    if key not in _E2E:
        depth = ref.LAYOUTS[layout][1]
        sd = synth.damp_residual_branch(synth.edvr_state_dict(0), 0.02)
        rgb = synth.clip(90 + h, 1, T, h, w)[0]                                                        # [T,3,h,w] in [0,1]
        words = [words_of([ref.to_levels(v, depth) for v in ref.emit(rgb[i].numpy(), h, w, depth)], layout) for i in range(T)]
        if h % 2 == 0 and w % 2 == 0:
            video = torch.from_numpy(np.stack([ref.pack(*p, layout) for p in words]))                  # [T, h*3/2, w] uint16
        else:
            video = [host_planes(p, layout) for p in words]
        net = make_net(sd)
        ingested = torch.stack([frames.ingest(video[i], layout, 4, 'reflect') for i in range(T)])
        today = [sr.clone()[:, :, :4 * h, :4 * w].contiguous()
                 for sr in adapt.super_resolve_frames(OPT, net, ingested, padding='new_info', in_flight=2)]
        u8 = (rgb * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()                      # the same content as RGB
        _E2E[key] = dict(net=net, video=video, today=today, u8=u8)
    return _E2E[key]


def run(net, video, **kw):
    return [sr.clone() for sr in adapt.super_resolve_frames(OPT, net, video, padding='new_info', **kw)]


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("case", [(18, 22, 'p010'), (13, 15, 'i420p10')], ids=lambda c: "%dx%d-%s" % c)
def test_video_end_to_end(case, in_flight):
    h, w, layout = case
    c = e2e_case(h, w, layout)
    net, video = c['net'], c['video']
    on_gpu = video.cuda() if torch.is_tensor(video) else video                  # (the planes of 13 x 15 stay on the host)
    flt_out = run(net, on_gpu, in_flight=in_flight, layout=layout, out='float')
    assert len(flt_out) == T and all(o.shape == (1, 3, 4 * h, 4 * w) for o in flt_out)
    assert all(torch.equal(a, b) for a, b in zip(flt_out, c['today']))           # (whatever in_flight is)
    out = run(net, video, in_flight=in_flight, layout=layout)                    # 16-bit words out, in the input's layout
    for i in range(T):
        assert out[i].dtype == torch.uint16 and out[i].shape == (6 * h, 4 * w) and out[i].is_cuda
        assert same(out[i], frames.emit(c['today'][i], 4 * h, 4 * w, layout)), i
    other = 'i420p12' if layout == 'p010' else 'p012'
    forced = run(net, on_gpu, in_flight=in_flight, layout=layout, out=other)
    eight = run(net, on_gpu, in_flight=in_flight, layout=layout, out='nv12')     # 10 bits in, 8 out
    for i in range(T):
        assert same(forced[i], frames.emit(flt_out[i], 4 * h, 4 * w, other)), i
        assert eight[i].dtype == torch.uint8 and torch.equal(eight[i], frames.emit(flt_out[i], 4 * h, 4 * w, 'nv12')), i
    if in_flight == 2:
        u8 = c['u8'].cuda()                                                      # 8-bit RGB in, 10 bits out
        from_rgb, from_rgb_flt = run(net, u8, in_flight=2, out='p010'), run(net, u8, in_flight=2, out='float')
        for i in range(T):
            assert from_rgb[i].dtype == torch.uint16 and from_rgb[i].shape == (6 * h, 4 * w)
            assert same(from_rgb[i], frames.emit(from_rgb_flt[i], 4 * h, 4 * w, 'p010')), i
        lev = ref.from_words(from_rgb[3].view(torch.int16).cpu().numpy().view(np.uint16), 'msb', 10)[0][:4 * h]
        assert int((lev % 4 != 0).sum()) > lev.size // 2                         # (levels between the 8-bit ones are in use)


def test_non_edvr_network_takes_p012_frames():
    """The `Mean` stand-in of test_gpu_frame_io.py: frames.ingest per frame, the windows through super_resolve_video,
    frames.emit per result."""
    calls = []

    class Mean(torch.nn.Module):
        nframes = 3

        def forward(self, x):
            calls.append(tuple(x.shape))
            return x.mean(1)

    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    levels = [random_levels(8, 10, 12, 20 + i) for i in range(5)]
    video = torch.from_numpy(np.stack([ref.pack(*words_of(p, 'p012'), 'p012') for p in levels]))       # [5,12,10] on the host
    kw = dict(padding='replicate', multiple=4, layout='p012', matrix='bt709', yuv_range='full')
    out = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), video, **kw)]
    flt = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), video.cuda(), out='float', **kw)]
    assert len(out) == 5 and calls == [(1, 3, 3, 8, 12)] * 10
    padded = np.stack([ref.ingest(*p, 8, 12, 12, 'reflect', 'bt709', 'full') for p in levels])
    for i in range(5):
        want = padded[index_generation(i, 5, 3, 'replicate')].mean(0)[:, :8, :10]
        # three ingested values, each within 1e-6, and the three fp32 roundings of their mean (<= 6e-8 each)
        assert flt[i].shape == (1, 3, 8, 10) and float(np.abs(flt[i][0].cpu().numpy() - want).max()) <= 1.2e-6, i
        assert out[i].dtype == torch.uint16 and out[i].shape == (12, 10)
        assert same(out[i], frames.emit(flt[i], 8, 10, 'p012', matrix='bt709', yuv_range='full')), i
    odd = [host_planes(words_of(random_levels(7, 9, 12, 30 + i), 'p012'), 'p012') for i in range(5)]  # planes, odd both ways
    rgb = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), odd, padding='replicate', layout='p012', out='hwc_rgb')]
    assert len(rgb) == 5 and all(o.shape == (7, 9, 3) and o.dtype == torch.uint8 for o in rgb)


# ---- scene cuts
def luma_video(y8, layout, seed):
    """Packed 16-bit video [T, h*3/2, w] whose Y words hold y8 (uint8 [T,h,w]) in the top 8 bits of the level and random bits
    everywhere else; the chroma is mid-grey."""
    storage, depth = ref.LAYOUTS[layout]
    T, h, w = y8.shape
    g = np.random.RandomState(seed).randint(0, 65536, y8.shape).astype(np.uint32)
    y = y8.astype(np.uint32)
    if storage == 'msb':
        yw = (y << 8) | (g & 0xff)
    else:
        yw = (y << (depth - 8)) | (g & (2 ** (depth - 8) - 1)) | ((g >> 8) << depth)
    c = ref.to_words(np.full((T, h // 2, w), 2 ** (depth - 1)), storage, depth)
    return np.ascontiguousarray(np.concatenate([(yw & 0xffff).astype(np.uint16), c], axis=1))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_luma_sad_of_16_bit_words_is_that_of_their_top_8_bits(layout):
    rgb = cut_ref.scene_video()                                                 # [14,24,40,3], cuts at 5 and 9
    T, h, w, _ = rgb.shape
    nv12 = cut_ref.rgb_to_nv12(rgb)
    y8 = nv12[:, :h]
    want = cut_ref.luma_sad(y8, 'nv12')
    video = torch.from_numpy(luma_video(y8, layout, 1))
    assert video.dtype == torch.uint16 and video.shape == (T, h * 3 // 2, w)
    dev = video.cuda()
    assert frames.luma_sad(dev, layout).tolist() == want.tolist()               # a device-resident video: one launch
    assert frames.luma_sad(dev.view(torch.int16), layout).tolist() == want.tolist()
    assert frames.luma_sad(video, layout).tolist() == want.tolist()             # host frames: the Y plane through staging buffers
    assert frames.luma_sad([dev[t] for t in range(T)], layout).tolist() == want.tolist()
    # planes of an odd width at a 2- but not 4-byte aligned address (the ragged end, the shifted row)
    ww = 37
    odd = []
    for t in range(T):
        _, yp = pitched(h, ww, 3)
        yp.copy_(dev[t, :h, :ww].view(torch.int16))
        chroma = torch.zeros((h // 2, (ww + 1) // 2) + ((2,) if semi(layout) else ()), dtype=torch.int16, device='cuda')
        odd.append((yp, chroma) if semi(layout) else (yp, chroma, chroma))
    assert frames.luma_sad(odd, layout).tolist() == cut_ref.luma_sad(y8[:, :, :ww], 'nv12').tolist()
    cuts = cut_ref.detect_cuts(want, h, w, 10.0)
    assert cuts == [5, 9]
    assert frames.detect_cuts(video, layout) == cuts and frames.detect_cuts(dev, layout) == cuts
    assert frames.detect_cuts(torch.from_numpy(nv12), 'nv12') == cuts           # ... what the 8-bit video gives


def test_auto_cuts_on_a_p010_video():
    class Mean(torch.nn.Module):
        nframes = 3

        def forward(self, x):
            return x.mean(1)

    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    rgb = cut_ref.scene_video()
    video = torch.from_numpy(luma_video(cut_ref.rgb_to_nv12(rgb)[:, :24], 'p010', 2)).cuda()

    def go(**kw):
        return [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), video, padding='replicate', layout='p010', **kw)]

    auto, want, none = go(cuts='auto'), go(cuts=[5, 9]), go()
    assert len(auto) == 14 and auto[0].dtype == torch.uint16 and tuple(auto[0].shape) == (36, 40)
    assert all(same(a, b) for a, b in zip(auto, want))
    assert not same(none[5], want[5])                                           # (a window across the cut gives other words)
