"""GPU: YCbCr 4:2:2 and 4:4:4 frames of 8, 10 and 12 bits in and out of the video path (the chroma axis of the kernel pair of
csrc/frame_yuv.hip; the nine layouts 'i422' / 'nv16' / 'i422p10' / 'i422p12' / 'p210' / 'p212' / 'i444' / 'i444p10' /
'i444p12' of dynavsr_amd/frames.py, StreamPlan.extract_frame, luma_sad, score, adapt.super_resolve_frames).

The yardstick is tests/yuv_chroma_ref.py, the arithmetic restated in fp64 numpy (test_yuv_chroma_host.py ties it to the 4:2:0
restatements).  The bars are those of test_gpu_yuv.py / test_gpu_yuv16.py for the same sample kind -- the matrix step, the
quotients and the rounding are the same lines of the kernels, and the resampling that differs has fewer operations than 4:2:0's
(4:2:2: (a + b) / 2 of two levels, exact in fp32; 4:4:4: none):
  ingest  max-abs <= 1e-6 against fp64, output within [0,1].
  emit    a sample equals rint of the fp64 value wherever that value is farther than TIE from a tie and is within 1 level
          elsewhere; TIE = 1e-3 levels at 8 bits, 4e-3 at 10, 8e-3 at 12; at most 2 % (2.5 % at 12 bits) of the samples may sit
          inside that window, asserted on the fp64 values alone (the seed is the first for which the helper says so).
  luma    sums of integers: exact.  mse: exact; ssim: 1e-10 (test_gpu_score.py).
  forward rel-L2 < 2e-4, max-abs < 1e-3 against the CPU oracle (test_gpu_yuv.py).
Planes sit at every sample offset 0 .. 3 of a 16-byte line, rows an odd number of samples apart."""
import numpy as np
import pytest
import torch

import cut_ref
import score_ref
import yuv_chroma_ref as ref
from conftest import relerr
from dynavsr_amd import adapt, engine, frames, synth
from dynavsr_amd.data.util import index_generation

pytestmark = pytest.mark.gpu

LAYOUTS = ['i422', 'nv16', 'i422p10', 'i422p12', 'p210', 'p212', 'i444', 'i444p10', 'i444p12']
# frame -> padded size: even and ragged in x | odd both ways (the last 4:2:2 chroma column serves one luma column) | across the
# 256-pixel workgroup edge in x and the 8-row edge in y | no padding
SIZES = [((6, 10), (8, 12)), ((7, 9), (8, 12)), ((18, 262), (20, 264)), ((16, 16), (16, 16))]
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
TIE = {8: 1e-3, 10: 4e-3, 12: 8e-3}
TIE_SHARE = {8: 0.02, 10: 0.02, 12: 0.025}
GUARD = 16                    # sentinel bytes ahead of the first row: a 16-byte line, so the offset stays the view's alignment


def info(layout):
    chroma, semi, depth, _ = ref.LAYOUTS[layout]
    return chroma, semi, depth, (torch.uint8 if depth == 8 else torch.uint16)


def same(a, b):
    """Bit equality of two tensors of 16-bit words (uint16 or int16) or of anything else."""
    if a.dtype in (torch.uint16, torch.int16):
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.shape == b.shape and torch.equal(a, b)


def plane_shapes(h, w, layout):
    hc, wc = ref.chroma_size(layout, h, w)
    return [(h, w), (hc, wc, 2)] if info(layout)[1] else [(h, w), (hc, wc), (hc, wc)]


def random_levels(h, w, layout, seed):
    """Level planes y [h,w], cb, cr [Hc,Wc] of seeded uniform random levels with 0 and 2^d - 1 planted: out-of-gamut triples
    occur, the clamp is exercised."""
    depth = info(layout)[2]
    hc, wc = ref.chroma_size(layout, h, w)
    r = np.random.RandomState(seed)
    planes = [r.randint(0, 2 ** depth, s) for s in ((h, w), (hc, wc), (hc, wc))]
    for p in planes:
        flat = p.reshape(-1)
        flat[r.permutation(flat.size)[:4]] = [0, 2 ** depth - 1, 0, 2 ** depth - 1]
    return planes


def offset_view(shape, dtype, o):
    """(buffer, view): a plane of `shape` whose first sample sits `o` samples into a 16-byte line of a sentinel-filled uint8
    buffer, its rows an odd number of samples apart."""
    es = torch.empty((), dtype=dtype).element_size()
    row = shape[1] * (shape[2] if len(shape) == 3 else 1)
    pitch = row + 1 + row % 2
    n = GUARD + o * es + shape[0] * pitch * es + GUARD
    buf = torch.full((n + n % 2,), 0x5A, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0 and pitch % 2 == 1
    view = buf.view(dtype).as_strided(shape, (pitch,) + ((2, 1) if len(shape) == 3 else (1,)), GUARD // es + o)
    assert view.data_ptr() % 16 == o * es
    return buf, view


def offset_planes(h, w, layout, o):
    pairs = [offset_view(s, info(layout)[3], o) for s in plane_shapes(h, w, layout)]
    return [b for b, _ in pairs], tuple(v for _, v in pairs)


def untouched_outside(bufs, planes):
    """Every sentinel between rows, before the first row and after the last row is still there."""
    for buf, p in zip(bufs, planes):
        rest, es = buf.clone(), p.element_size()
        inside = rest.view(p.dtype).as_strided(p.shape, p.stride(), (p.data_ptr() - buf.data_ptr()) // es)
        inside.view(torch.int16 if es == 2 else torch.uint8).fill_(0x5A5A if es == 2 else 0x5A)
        if not bool((rest == 0x5A).all()):
            return False
    return True


def fill(planes, samples, layout):
    """Copies numpy sample planes (y, cb, cr) into GPU planes."""
    src = [samples[0], np.stack(samples[1:], -1)] if info(layout)[1] else list(samples)
    for p, s in zip(planes, src):
        s = np.ascontiguousarray(s)
        if s.dtype == np.uint16:
            p.view(torch.int16).copy_(torch.from_numpy(s.view(np.int16)))
        else:
            p.copy_(torch.from_numpy(s))
    return planes


def gpu_planes(samples, layout, o=1):
    h, w = samples[0].shape
    return fill(offset_planes(h, w, layout, o)[1], samples, layout)


def host_planes(samples, layout):
    t = [torch.from_numpy(np.ascontiguousarray(a)) for a in samples]
    return (t[0], torch.from_numpy(np.ascontiguousarray(np.stack(samples[1:], -1)))) if info(layout)[1] else tuple(t)


def planes_to_numpy(planes, layout):
    p = [(t.view(torch.int16).cpu().numpy().view(np.uint16) if t.element_size() == 2 else t.cpu().numpy()) for t in planes]
    return (p[0], p[1][:, :, 0], p[1][:, :, 1]) if info(layout)[1] else tuple(p)


def packed_numpy(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.element_size() == 2 else t.cpu().numpy()


# ---- ingest
def check_ingest(size, layout, mode, matrix, yuv_range):
    (h, w), (Hp, Wp) = size
    chroma, semi, depth, dt = info(layout)
    assert frames.padded_size(h, w, 4) == (Hp, Wp)
    levels = random_levels(h, w, layout, 100 * h + w + depth)
    samples = [ref.samples_of(p, layout) for p in levels]
    want = ref.ingest(*levels, Hp, Wp, layout, mode, matrix, yuv_range)
    kw = dict(matrix=matrix, yuv_range=yuv_range)
    first = None
    for o in range(4):
        bufs, planes = offset_planes(h, w, layout, o)
        fill(planes, samples, layout)
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(frames.describe_yuv(planes, layout, h, w)[0], planes))
        n = 3 * Hp * Wp
        big = torch.full((n + 256,), -7.0, device='cuda')
        out = big[:n].view(3, Hp, Wp)
        got = frames.ingest(planes, layout, 4, mode, out=out, **kw)
        assert got.data_ptr() == out.data_ptr()
        assert bool((big[n:] == -7.0).all())                                   # nothing behind the destination
        assert untouched_outside(bufs, planes), o
        if first is None:
            first = got
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
            print("ingest %s %dx%d %s %s/%s: max-abs %.2e" % (layout, h, w, mode, matrix, yuv_range, err))
            assert err <= 1e-6
            assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
        else:
            assert torch.equal(got, first), o                                   # whatever the alignment of the planes
    fresh = frames.ingest(host_planes(samples, layout), layout, 4, mode, **kw)  # planes in host memory, into a tensor of its own
    assert fresh.shape == (3, Hp, Wp) and torch.equal(fresh, first)
    if depth > 8:                                                              # int16: the same bits
        assert torch.equal(frames.ingest(tuple(p.view(torch.int16) for p in planes), layout, 4, mode, **kw), first)
    if chroma == '444' or w % 2 == 0:                                          # ... and from the packed form, host and device
        packed = torch.from_numpy(ref.pack(*samples, layout))
        assert packed.dtype == dt
        assert torch.equal(frames.ingest(packed, layout, 4, mode, **kw), first)
        assert torch.equal(frames.ingest(packed.cuda(), layout, 4, mode, **kw), first)
    return first


@pytest.mark.parametrize("mode", ['reflect', 'replicate'])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s[0])
def test_ingest_against_fp64(size, layout, mode):
    check_ingest(size, layout, mode, 'bt601', 'limited')


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ingest_bt709_full(layout):
    check_ingest(SIZES[2], layout, 'reflect', 'bt709', 'full')


@pytest.mark.parametrize("pair", [('i422', 'nv16'), ('i422p10', 'p210'), ('i422p12', 'p212')], ids="-".join)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s[0])
def test_planar_and_semi_planar_frames_of_the_same_levels_ingest_alike(size, pair):
    (h, w), _ = size
    planar, semi = pair
    levels = random_levels(h, w, planar, 7 + h)
    a = frames.ingest(gpu_planes([ref.samples_of(p, planar) for p in levels], planar), planar, 4, 'reflect')
    b = frames.ingest(gpu_planes([ref.samples_of(p, semi) for p in levels], semi), semi, 4, 'reflect')
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("layout", ['p210', 'i422p12', 'i444p10'])
def test_ingest_ignores_the_bits_that_carry_no_level(layout):
    (h, w), (Hp, Wp) = SIZES[2]
    levels = random_levels(h, w, layout, 7)
    clean = [ref.samples_of(p, layout) for p in levels]
    dirty = [ref.samples_of(p, layout, np.random.RandomState(11 + i).randint(0, 65536, p.shape)) for i, p in enumerate(levels)]
    assert all(not np.array_equal(a, b) for a, b in zip(clean, dirty))
    a = frames.ingest(gpu_planes(clean, layout), layout, 4, 'reflect')
    b = frames.ingest(gpu_planes(dirty, layout), layout, 4, 'reflect')
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- emit
EMIT_SHAPES = [((8, 12), (6, 10)), ((8, 12), (7, 9)), ((20, 264), (18, 262)), ((16, 16), (16, 16))]   # source, crop


def check_samples(got, levels, layout, what):
    """got: sample arrays; levels: their fp64 values before rounding.  Returns the share of samples within TIE of a tie."""
    depth = info(layout)[2]
    near_n = total = 0
    for g, v in zip(got, levels):
        assert g.shape == v.shape, (what, g.shape, v.shape)
        lev, rest = ref.levels_of(g, layout)
        assert int(rest.max()) == 0, (what, "the bits that carry no level must be written as 0")
        want, far = ref.round_levels(v, layout), ref.tie_distance(v, layout) > TIE[depth]
        assert np.array_equal(lev[far], want[far]), (what, int((lev[far] != want[far]).sum()))
        assert int(np.abs(lev.astype(np.int32) - want.astype(np.int32)).max()) <= 1, what
        near_n += int((~far).sum())
        total += v.size
    return near_n / total


def emit_input(shape, layout, lohi, matrix, yuv_range):
    """(host fp32 [3,Hs,Ws], its fp64 levels, the share of them inside the tie window): the first seed whose fp64 levels keep
    the share under the cap -- a property of the input alone, decided before the device is asked anything."""
    (Hs, Ws), (h, w) = shape
    depth = info(layout)[2]
    for seed in range(Hs + h, Hs + h + 50):
        host = np.random.RandomState(seed).uniform(-0.2, 1.2, (3, Hs, Ws)).astype(np.float32)
        levels = ref.emit(host, h, w, layout, lohi[0], lohi[1], matrix, yuv_range)
        share = sum(int((ref.tie_distance(v, layout) <= TIE[depth]).sum()) for v in levels) / sum(v.size for v in levels)
        if share <= TIE_SHARE[depth]:
            return torch.from_numpy(host), levels, share
    raise AssertionError("no input under the cap")


def check_emit(shape, layout, lohi, matrix, yuv_range):
    (Hs, Ws), (h, w) = shape
    chroma, semi, depth, dt = info(layout)
    host, levels, share = emit_input(shape, layout, lohi, matrix, yuv_range)
    print("emit %s %dx%d of %dx%d [%g,%g] %s/%s: %.2f %% of the samples within %g of a tie" % (
        layout, h, w, Hs, Ws, lohi[0], lohi[1], matrix, yuv_range, 100 * share, TIE[depth]))
    assert share <= TIE_SHARE[depth]                                            # (on the fp64 values alone)
    sr = host.cuda()
    kw = dict(matrix=matrix, yuv_range=yuv_range)
    first = None
    for o in range(4):
        bufs, planes = offset_planes(h, w, layout, o)
        assert untouched_outside(bufs, planes)                                 # (the test's own views are what they claim)
        got = frames.emit(sr, h, w, layout, lohi, out=planes, **kw)
        assert got is planes
        assert untouched_outside(bufs, planes), (o, "a byte outside the planes' rows was written")
        if first is None:
            first = planes_to_numpy(planes, layout)
            assert check_samples(first, levels, layout, (shape, layout, lohi)) == share
        else:
            assert all(np.array_equal(a, b) for a, b in zip(planes_to_numpy(planes, layout), first)), o
    if frames.packed_needs(layout, h, w) is None:                              # the packed result is the planes result
        rows = (2 if chroma == '422' else 3) * h
        packed = frames.emit(sr[None], h, w, layout, lohi, **kw)
        assert packed.dtype == dt and packed.shape == (rows, w) and packed.is_contiguous()
        assert all(np.array_equal(a, b) for a, b in zip(ref.unpack(packed_numpy(packed), layout), first))
        into = torch.full((rows, w), 0x5A5A if depth > 8 else 0x5A, dtype=torch.int16 if depth > 8 else torch.uint8, device='cuda')
        assert frames.emit(sr, h, w, layout, lohi, out=into, **kw) is into
        assert same(into, packed)
    else:
        assert chroma == '422' and w % 2 == 1
        with pytest.raises(ValueError, match="even width"):
            frames.emit(sr, h, w, layout, lohi, **kw)


@pytest.mark.parametrize("lohi", [(0.0, 1.0), (-1.0, 1.0)])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", EMIT_SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_emit_against_fp64(shape, layout, lohi):
    check_emit(shape, layout, lohi, 'bt601', 'limited')


@pytest.mark.parametrize("layout", LAYOUTS)
def test_emit_bt709_full(layout):
    check_emit(EMIT_SHAPES[1], layout, (0.0, 1.0), 'bt709', 'full')
    check_emit(EMIT_SHAPES[2], layout, (0.0, 1.0), 'bt709', 'full')


@pytest.mark.parametrize("pair", [('i422', 'i420'), ('i444', 'i420'), ('nv16', 'nv12'), ('i422p10', 'i420p10'), ('i444p12', 'i420p12'),
                                  ('p210', 'p010')], ids="-".join)
@pytest.mark.parametrize("shape", EMIT_SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_emitted_luma_does_not_depend_on_the_chroma_axis(shape, pair):
    (Hs, Ws), (h, w) = shape
    layout, like = pair
    sr = torch.from_numpy(np.random.RandomState(h + w).uniform(-0.2, 1.2, (3, Hs, Ws)).astype(np.float32)).cuda()
    dt = info(layout)[3]
    for lohi in ((0.0, 1.0), (-1.0, 1.0)):
        planes = tuple(torch.zeros(s, dtype=dt, device='cuda') for s in plane_shapes(h, w, layout))
        hc, wc = (h + 1) // 2, (w + 1) // 2
        shapes420 = [(h, w), (hc, wc, 2)] if info(layout)[1] else [(h, w), (hc, wc), (hc, wc)]
        planes420 = tuple(torch.zeros(s, dtype=dt, device='cuda') for s in shapes420)
        frames.emit(sr, h, w, layout, lohi, out=planes)
        frames.emit(sr, h, w, like, lohi, out=planes420)
        assert same(planes[0], planes420[0])
        assert int(planes[0].view(torch.int16 if dt == torch.uint16 else torch.uint8).max()) > 0


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
    for layout in ('nv16', 'i444p10'):
        levels = random_levels(h, w, layout, 3)
        src = gpu_planes([ref.samples_of(p, layout) for p in levels], layout)
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
        want = ref.ingest(*levels, Hp, Wp, layout, 'reflect').reshape(-1)
        raw = a[2][torch.isfinite(a[2])][-want.size:].numpy().astype(np.float64)  # the slot's last section is the padded frame
        assert float(np.abs(raw - want).max()) <= 1e-6


# ---- scene cuts
@pytest.mark.parametrize("layout", ['i422p10', 'i444'])
def test_luma_sad_of_a_three_frame_video(layout):
    chroma, semi, depth, dt = info(layout)
    h, w, T = 12, 20, 3
    levels = [random_levels(h, w, layout, 40 + t) for t in range(T)]
    garbage = np.random.RandomState(5).randint(0, 65536, (h, w))
    frames_np = [ref.pack(*[ref.samples_of(p, layout, garbage if i == 0 else None) for i, p in enumerate(lv)], layout) for lv in levels]
    y8 = np.stack([lv[0] >> (depth - 8) for lv in levels])                      # the top 8 bits of the level
    want = cut_ref.luma_sad(y8, 'nv12')
    assert len(want) == 2 and int(want.min()) > 0
    video = torch.from_numpy(np.stack(frames_np))
    assert video.dtype == dt and video.shape == (T, (2 if chroma == '422' else 3) * h, w)
    dev = video.cuda()
    assert frames.luma_sad(dev, layout).tolist() == want.tolist()               # a device-resident video: one launch
    assert frames.luma_sad(video, layout).tolist() == want.tolist()             # host frames: the Y plane through staging buffers
    assert frames.luma_sad([dev[t] for t in range(T)], layout).tolist() == want.tolist()
    planes = [gpu_planes([ref.samples_of(p, layout) for p in lv], layout, o=3) for lv in levels]       # planes, shifted and pitched
    assert frames.luma_sad(planes, layout).tolist() == want.tolist()
    assert frames.detect_cuts(dev, layout, threshold=1e-3) == cut_ref.detect_cuts(want, h, w, 1e-3)


# ---- score
def test_score_of_an_emitted_nv16_frame_against_an_rgb_gt():
    h, w = 27, 44
    r = np.random.RandomState(2)
    gt = r.randint(0, 256, (h, w, 3)).astype(np.uint8)
    sr = torch.from_numpy((gt.transpose(2, 0, 1) / 255.0 + r.normal(0, 0.02, (3, h, w))).astype(np.float32))
    sr = torch.nn.functional.pad(sr, (0, 0, 0, 1)).cuda()                       # [3,28,44]
    out = frames.emit(sr, h, w, 'nv16')
    assert out.shape == (2 * h, w)
    a = score_ref.samples(out[:h].cpu().numpy(), 'y', 'y')
    b = score_ref.samples(gt, 'hwc_rgb', 'y')
    for k in (0, 4):
        sse, n, mse, ssim = score_ref.score(a, b, k)
        for g in (torch.from_numpy(gt), torch.from_numpy(gt).cuda()):
            got = frames.score(out, g, 'nv16', 'hwc_rgb', channel='y', crop_border=k).cpu().tolist()
            assert got[0] == mse and round(got[0] * n) == sse and sse > 0, (k, got, mse)
            assert abs(got[1] - ssim) < 1e-10, (k, got, ssim)
    with pytest.raises(ValueError, match="channel='y'"):
        frames.score(out, torch.from_numpy(gt), 'nv16', 'hwc_rgb')


# ---- end to end
T = 7
_E2E = {}


def e2e_case(h, w, layout):
    """Per (size, layout), computed once and never modified: synth.clip content turned into the layout's samples by the
    restatement, and the CPU oracle's frames 0, 3 and 6 on the restated padded windows (cropped)."""
    key = (h, w, layout)
    if key not in _E2E:
        from oracle import edvr as oedvr
        sd = synth.damp_residual_branch(synth.edvr_state_dict(0), 0.02)
        Hp, Wp = frames.padded_size(h, w, 4)
        rgb = synth.clip(90 + h, 1, T, h, w)[0]                                                        # [T,3,h,w] in [0,1]
        levels = [[ref.round_levels(v, layout) for v in ref.emit(rgb[i].numpy(), h, w, layout)] for i in range(T)]
        samples = [[ref.samples_of(p, layout) for p in lv] for lv in levels]
        if frames.packed_needs(layout, h, w) is None and h % 2 == 0:
            video = torch.from_numpy(np.stack([ref.pack(*p, layout) for p in samples]))                # packed, on the host
        else:
            video = [host_planes(p, layout) for p in samples]
        padded = torch.from_numpy(np.stack([ref.ingest(*lv, Hp, Wp, layout, 'reflect') for lv in levels])).float()
        oracle = {}
        for i in (0, 3, 6):
            with torch.no_grad():
                oracle[i] = oedvr.edvr_forward(sd, padded[index_generation(i, T, 5, 'new_info')][None])[:, :, :4 * h, :4 * w]
        u8 = (rgb * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()                      # the same content as RGB
        _E2E[key] = dict(net=make_net(sd), video=video, oracle=oracle, u8=u8)
    return _E2E[key]


def run(net, video, opt=OPT, **kw):
    kw.setdefault('padding', 'new_info')
    return [sr.clone() for sr in adapt.super_resolve_frames(opt, net, video, **kw)]


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("case", [(18, 22, 'nv16'), (13, 15, 'i444p10')], ids=lambda c: "%dx%d-%s" % c)
def test_video_end_to_end(case, in_flight):
    h, w, layout = case
    chroma, semi, depth, dt = info(layout)
    c = e2e_case(h, w, layout)
    net, video = c['net'], c['video']
    assert torch.is_tensor(video) == (layout == 'nv16')                          # 18 x 22 packed, 13 x 15 as planes
    on_gpu = video.cuda() if torch.is_tensor(video) else video                  # (the planes stay on the host)
    flt_out = run(net, on_gpu, in_flight=in_flight, layout=layout, out='float')
    assert len(flt_out) == T and all(o.shape == (1, 3, 4 * h, 4 * w) for o in flt_out)
    out = run(net, video, in_flight=in_flight, layout=layout)                    # samples out, in the input's layout
    rows = (2 if chroma == '422' else 3) * 4 * h
    for i in range(T):
        assert out[i].dtype == dt and out[i].shape == (rows, 4 * w) and out[i].is_cuda
        assert same(out[i], frames.emit(flt_out[i], 4 * h, 4 * w, layout)), i
    for i, yo in c['oracle'].items():                                           # against the CPU oracle on the restated input
        y = flt_out[i].cpu()
        e, d = relerr(y, yo), float((y - yo).abs().max())
        print("%dx%d %s in_flight %d frame %d: rel-L2 %.3e max-abs %.3e" % (h, w, layout, in_flight, i, e, d))
        assert e < 2e-4 and d < 1e-3, (i, e, d)


def test_flip_test_on_an_nv16_video():
    c = e2e_case(18, 22, 'nv16')
    video = c['video'].cuda()
    flt = run(c['net'], video, in_flight=2, layout='nv16', out='float', flip_test=True)
    out = run(c['net'], video, in_flight=2, layout='nv16', flip_test=True)
    plain = run(c['net'], video, in_flight=2, layout='nv16', out='float')
    assert len(out) == T
    for i in range(T):
        assert out[i].shape == (144, 88) and torch.equal(out[i], frames.emit(flt[i], 72, 88, 'nv16')), i
    assert not torch.equal(flt[3], plain[3])                                    # (the ensemble ran)


def test_cuts_on_an_nv16_video():
    c = e2e_case(18, 22, 'nv16')
    video = c['video'].cuda()
    cut = run(c['net'], video, in_flight=2, layout='nv16', cuts=[3])
    # (cuts=[]: one scene under the rule of scene mode, where a scene too short for 'new_info' takes 'replicate')
    alone = run(c['net'], video[:3], in_flight=2, layout='nv16', cuts=[]) + run(c['net'], video[3:], in_flight=2, layout='nv16', cuts=[])
    whole = run(c['net'], video, in_flight=2, layout='nv16')
    assert len(cut) == T and all(torch.equal(a, b) for a, b in zip(cut, alone))  # every scene as if it had been passed alone
    assert not torch.equal(cut[3], whole[3])                                    # (a window across the cut gives other bytes)


def test_out_size_with_an_i422_output():
    c = e2e_case(18, 22, 'nv16')
    video = c['video'].cuda()
    flt = run(c['net'], video, in_flight=2, layout='nv16', out='float')
    out = run(c['net'], video, in_flight=2, layout='nv16', out='i422', out_size=(54, 66))
    flt_sized = run(c['net'], video, in_flight=2, layout='nv16', out='float', out_size=(54, 66))
    for i in range(T):
        assert out[i].dtype == torch.uint8 and out[i].shape == (108, 66)
        assert flt_sized[i].shape == (1, 3, 54, 66)
        assert torch.equal(out[i], frames.emit(flt[i], 72, 88, 'i422', size=(54, 66))), i
        assert torch.equal(out[i], frames.emit(flt_sized[i], 54, 66, 'i422')), i
    odd = run(c['net'], video[:5], in_flight=2, layout='nv16', out='i422', out_size=(53, 66))          # an odd height packs
    assert odd[0].shape == (106, 66)


def test_p210_out_of_a_uint8_hwc_input():
    c = e2e_case(18, 22, 'nv16')
    u8 = c['u8'].cuda()
    out, flt = run(c['net'], u8, in_flight=2, out='p210'), run(c['net'], u8, in_flight=2, out='float')
    for i in range(T):
        assert out[i].dtype == torch.uint16 and out[i].shape == (144, 88)
        assert same(out[i], frames.emit(flt[i], 72, 88, 'p210')), i
    lev = ref.levels_of(packed_numpy(out[3]), 'p210')[0][:72]
    assert int((lev % 4 != 0).sum()) > lev.size // 2                             # (levels between the 8-bit ones are in use)


def test_non_edvr_network_takes_i422_frames():
    """The `Mean` stand-in of test_gpu_frame_io.py: frames.ingest per frame, the windows through super_resolve_video,
    frames.emit per result."""
    calls = []

    class Mean(torch.nn.Module):
        nframes = 3

        def forward(self, x):
            calls.append(tuple(x.shape))
            return x.mean(1)

    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    levels = [random_levels(7, 10, 'i422', 20 + i) for i in range(5)]
    video = torch.from_numpy(np.stack([ref.pack(*[ref.samples_of(p, 'i422') for p in lv], 'i422') for lv in levels]))   # [5,14,10]
    kw = dict(padding='replicate', multiple=4, layout='i422', matrix='bt709', yuv_range='full')
    out = run(Mean(), video, opt, **kw)
    flt = run(Mean(), video.cuda(), opt, out='float', **kw)
    assert len(out) == 5 and calls == [(1, 3, 3, 8, 12)] * 10
    padded = np.stack([ref.ingest(*lv, 8, 12, 'i422', 'reflect', 'bt709', 'full') for lv in levels])
    for i in range(5):
        want = padded[index_generation(i, 5, 3, 'replicate')].mean(0)[:, :7, :10]
        # three ingested values, each within 1e-6, and the three fp32 roundings of their mean (<= 6e-8 each)
        assert flt[i].shape == (1, 3, 7, 10) and float(np.abs(flt[i][0].cpu().numpy() - want).max()) <= 1.2e-6, i
        assert out[i].dtype == torch.uint8 and out[i].shape == (14, 10)
        assert torch.equal(out[i], frames.emit(flt[i], 7, 10, 'i422', matrix='bt709', yuv_range='full')), i
