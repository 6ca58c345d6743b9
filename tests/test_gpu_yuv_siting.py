"""GPU: chroma siting ('center' | 'topleft') and the BT.2020 NCL matrix in the kernel pair of csrc/frame_yuv.hip (the SITE axis,
DESIGN 3.2x) through dynavsr_amd/frames.py, StreamPlan.extract_frame and video.super_resolve_frames.

The yardstick is tests/yuv_siting_ref.py, the arithmetic restated in fp64 numpy (test_yuv_siting_host.py ties it to the older
restatements, to plain linear interpolation at the sited positions and to torch's bilinear interpolation).  The bars and the
machinery are those of test_gpu_yuv_chroma.py -- the matrix step, the quotients and the rounding are the same lines of the
kernels, and the resampling that differs is exact in fp32 on the way in (multiples of 1/16 of a level below 2^12) and has no more
operations than 4:2:0 "left" on the way out (center: fewer taps; topleft: the [1,2,1]/4 taps of the columns, on the rows too):
  ingest  max-abs <= 1e-6 against fp64, output within [0,1].
  emit    a sample equals rint of the fp64 value wherever that value is farther than TIE from a tie and is within 1 level
          elsewhere; TIE = 1e-3 levels at 8 bits, 4e-3 at 10, 8e-3 at 12; at most 2 % (2.5 % at 12 bits) of the samples may sit
          inside that window, asserted on the fp64 values alone (the seed is the first for which the helper says so).
  forward rel-L2 < 2e-4, max-abs < 1e-3 against the CPU oracle (test_gpu_yuv.py).
Planes sit at every sample offset 0 .. 3 of a 16-byte line, rows an odd number of samples apart."""
import numpy as np
import pytest
import torch

import yuv_siting_ref as ref
from conftest import relerr
from dynavsr_amd import engine, frames, synth, video
from dynavsr_amd.data.util import index_generation
from test_gpu_yuv_chroma import offset_view, same, untouched_outside

pytestmark = pytest.mark.gpu

# (layout, siting): 4:2:0 x {center, topleft}, 4:2:2 x {center}; bytes and words, semi-planar and planar
CASES = [(lay, s) for lay in ('nv12', 'i420', 'p010', 'i420p12') for s in ('center', 'topleft')] + \
        [(lay, 'center') for lay in ('nv16', 'i422', 'p210', 'i422p10')]
# frame -> padded size: even and ragged in x | odd both ways | Hc = 2, Wc = 3: both clamps meet | across the 256-pixel workgroup
# edge in x and the 8-row edge in y | no padding
SIZES = [((6, 10), (8, 12)), ((7, 9), (8, 12)), ((3, 5), (4, 8)), ((18, 262), (20, 264)), ((16, 16), (16, 16))]
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
TIE = {8: 1e-3, 10: 4e-3, 12: 8e-3}
TIE_SHARE = {8: 0.02, 10: 0.02, 12: 0.025}
case_id = "-".join
size_id = lambda s: "%dx%d" % s[0]


def info(layout):
    sub, semi, depth, _ = ref.LAYOUTS[layout]
    return sub, semi, depth, (torch.uint8 if depth == 8 else torch.uint16)


def plane_shapes(h, w, layout):
    hc, wc = ref.chroma_size(layout, h, w)
    return [(h, w), (hc, wc, 2)] if info(layout)[1] else [(h, w), (hc, wc), (hc, wc)]


def random_levels(h, w, layout, seed):
    """Level planes y [h,w], cb, cr [Hc,Wc] of seeded uniform random levels with 0 and 2^d - 1 planted where there is room:
    out-of-gamut triples occur, the clamp is exercised."""
    depth = info(layout)[2]
    hc, wc = ref.chroma_size(layout, h, w)
    r = np.random.RandomState(seed)
    planes = [r.randint(0, 2 ** depth, s) for s in ((h, w), (hc, wc), (hc, wc))]
    for p in planes:
        flat = p.reshape(-1)
        flat[r.permutation(flat.size)[:4]] = [0, 2 ** depth - 1, 0, 2 ** depth - 1][:min(4, flat.size)]
    return planes


def offset_planes(h, w, layout, o):
    pairs = [offset_view(s, info(layout)[3], o) for s in plane_shapes(h, w, layout)]
    return [b for b, _ in pairs], tuple(v for _, v in pairs)


def fill(planes, samples, layout):
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
def check_ingest(size, layout, siting, mode, matrix='bt601', yuv_range='limited'):
    (h, w), (Hp, Wp) = size
    sub, semi, depth, dt = info(layout)
    assert frames.padded_size(h, w, 4) == (Hp, Wp)
    levels = random_levels(h, w, layout, 100 * h + w + depth)
    samples = [ref.samples_of(p, layout) for p in levels]
    want = ref.ingest(*levels, Hp, Wp, layout, mode, matrix, yuv_range, siting)
    kw = dict(matrix=matrix, yuv_range=yuv_range, siting=siting)
    first = None
    for o in range(4):
        bufs, planes = offset_planes(h, w, layout, o)
        fill(planes, samples, layout)
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
            print("ingest %s %s %dx%d %s %s/%s: max-abs %.2e" % (layout, siting, h, w, mode, matrix, yuv_range, err))
            assert err <= 1e-6
            assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
        else:
            assert torch.equal(got, first), o                                   # whatever the alignment of the planes
    fresh = frames.ingest(host_planes(samples, layout), layout, 4, mode, **kw)  # planes in host memory, into a tensor of its own
    assert fresh.shape == (3, Hp, Wp) and torch.equal(fresh, first)
    if depth > 8:                                                              # int16: the same bits
        assert torch.equal(frames.ingest(tuple(p.view(torch.int16) for p in planes), layout, 4, mode, **kw), first)
    if frames.packed_needs(layout, h, w) is None:                              # ... and from the packed form
        packed = torch.from_numpy(ref.pack(*samples, layout))
        assert packed.dtype == dt
        assert torch.equal(frames.ingest(packed.cuda(), layout, 4, mode, **kw), first)
    return first


@pytest.mark.parametrize("mode", ['reflect', 'replicate'])
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_ingest_against_fp64(size, case, mode):
    check_ingest(size, case[0], case[1], mode)


def test_the_sitings_ingest_differently():
    """(the axis is wired: three sitings of one frame give three tensors)"""
    (h, w), _ = SIZES[0]
    levels = random_levels(h, w, 'nv12', 1)
    src = gpu_planes([ref.samples_of(p, 'nv12') for p in levels], 'nv12')
    a, b, c = (frames.ingest(src, 'nv12', 4, 'reflect', siting=s) for s in ref.SITINGS)
    assert not torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(b, c)


PAIRS = [('i420', 'nv12', 'center'), ('i420', 'nv12', 'topleft'), ('i420p10', 'p010', 'center'), ('i420p10', 'p010', 'topleft'),
         ('i420p12', 'p012', 'topleft'), ('i422', 'nv16', 'center'), ('i422p10', 'p210', 'center')]


@pytest.mark.parametrize("pair", PAIRS, ids=case_id)
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_planar_and_semi_planar_frames_of_the_same_levels_ingest_alike(size, pair):
    (h, w), _ = size
    planar, semi, siting = pair
    levels = random_levels(h, w, planar, 7 + h)
    for matrix, rng in (('bt601', 'limited'), ('bt2020nc', 'full')):
        kw = dict(siting=siting, matrix=matrix, yuv_range=rng)
        a = frames.ingest(gpu_planes([ref.samples_of(p, planar) for p in levels], planar), planar, 4, 'reflect', **kw)
        b = frames.ingest(gpu_planes([ref.samples_of(p, semi) for p in levels], semi), semi, 4, 'reflect', **kw)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("case", [('p010', 'center'), ('p010', 'topleft'), ('i420p12', 'center'), ('i420p12', 'topleft'),
                                  ('p210', 'center'), ('i422p10', 'center')], ids=case_id)
def test_ingest_ignores_the_bits_that_carry_no_level(case):
    layout, siting = case
    for (h, w), _ in (SIZES[1], SIZES[3]):
        levels = random_levels(h, w, layout, 7)
        clean = [ref.samples_of(p, layout) for p in levels]
        dirty = [ref.samples_of(p, layout, np.random.RandomState(11 + i).randint(0, 65536, p.shape)) for i, p in enumerate(levels)]
        assert all(not np.array_equal(a, b) for a, b in zip(clean, dirty))
        a = frames.ingest(gpu_planes(clean, layout), layout, 4, 'reflect', siting=siting)
        b = frames.ingest(gpu_planes(dirty, layout), layout, 4, 'reflect', siting=siting)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- emit
EMIT_SHAPES = [((8, 12), (6, 10)), ((8, 12), (7, 9)), ((4, 8), (3, 5)), ((20, 264), (18, 262)), ((16, 16), (16, 16))]   # source, crop
shape_id = lambda s: "%dx%d-%dx%d" % (s[0] + s[1])


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


def emit_input(shape, layout, siting, lohi, matrix, yuv_range):
    """(host fp32 [3,Hs,Ws], its fp64 levels, the share of them inside the tie window): the first seed whose fp64 levels keep
    the share under the cap -- a property of the input alone, decided before the device is asked anything."""
    (Hs, Ws), (h, w) = shape
    depth = info(layout)[2]
    for seed in range(Hs + h, Hs + h + 50):
        host = np.random.RandomState(seed).uniform(-0.2, 1.2, (3, Hs, Ws)).astype(np.float32)
        levels = ref.emit(host, h, w, layout, lohi[0], lohi[1], matrix, yuv_range, siting)
        share = sum(int((ref.tie_distance(v, layout) <= TIE[depth]).sum()) for v in levels) / sum(v.size for v in levels)
        if share <= TIE_SHARE[depth]:
            return torch.from_numpy(host), levels, share
    raise AssertionError("no input under the cap")


def check_emit(shape, layout, siting, lohi, matrix='bt601', yuv_range='limited'):
    (Hs, Ws), (h, w) = shape
    sub, semi, depth, dt = info(layout)
    host, levels, share = emit_input(shape, layout, siting, lohi, matrix, yuv_range)
    print("emit %s %s %dx%d of %dx%d [%g,%g] %s/%s: %.2f %% of the samples within %g of a tie" % (
        layout, siting, h, w, Hs, Ws, lohi[0], lohi[1], matrix, yuv_range, 100 * share, TIE[depth]))
    assert share <= TIE_SHARE[depth]                                            # (on the fp64 values alone)
    sr = host.cuda()
    kw = dict(matrix=matrix, yuv_range=yuv_range, siting=siting)
    first = None
    for o in range(4):
        bufs, planes = offset_planes(h, w, layout, o)
        assert untouched_outside(bufs, planes)                                 # (the test's own views are what they claim)
        got = frames.emit(sr, h, w, layout, lohi, out=planes, **kw)
        assert got is planes
        assert untouched_outside(bufs, planes), (o, "a byte outside the planes' rows was written")
        if first is None:
            first = planes_to_numpy(planes, layout)
            assert check_samples(first, levels, layout, (shape, layout, siting, lohi)) == share
        else:
            assert all(np.array_equal(a, b) for a, b in zip(planes_to_numpy(planes, layout), first)), o
    if frames.packed_needs(layout, h, w) is None:                              # the packed result is the planes result
        packed = frames.emit(sr[None], h, w, layout, lohi, **kw)
        assert packed.dtype == dt and packed.shape == (frames.packed_rows(layout, h), w) and packed.is_contiguous()
        assert all(np.array_equal(a, b) for a, b in zip(ref.unpack(packed_numpy(packed), layout), first))
    return sr, first


@pytest.mark.parametrize("lohi", [(0.0, 1.0), (-1.0, 1.0)])
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("shape", EMIT_SHAPES, ids=shape_id)
def test_emit_against_fp64(shape, case, lohi):
    check_emit(shape, case[0], case[1], lohi)


@pytest.mark.parametrize("pair", PAIRS, ids=case_id)
@pytest.mark.parametrize("shape", EMIT_SHAPES, ids=shape_id)
def test_the_same_rgb_emits_to_the_same_samples_for_both_forms(shape, pair):
    (Hs, Ws), (h, w) = shape
    planar, semi, siting = pair
    sr = torch.from_numpy(np.random.RandomState(h + w).uniform(-0.2, 1.2, (3, Hs, Ws)).astype(np.float32)).cuda()
    for matrix, rng in (('bt601', 'limited'), ('bt2020nc', 'full')):
        kw = dict(siting=siting, matrix=matrix, yuv_range=rng)
        out = []
        for layout in (planar, semi):
            planes = offset_planes(h, w, layout, 1)[1]
            frames.emit(sr, h, w, layout, out=planes, **kw)
            out.append([ref.levels_of(p, layout)[0] for p in planes_to_numpy(planes, layout)])
        assert all(np.array_equal(a, b) for a, b in zip(*out)), (matrix, rng)


@pytest.mark.parametrize("layout", ['nv12', 'i420', 'p010', 'i420p12', 'nv16', 'i422p10'])
@pytest.mark.parametrize("shape", EMIT_SHAPES, ids=shape_id)
def test_emitted_luma_is_identical_for_the_three_sitings(shape, layout):
    (Hs, Ws), (h, w) = shape
    sr = torch.from_numpy(np.random.RandomState(h + w).uniform(-0.2, 1.2, (3, Hs, Ws)).astype(np.float32)).cuda()
    for lohi in ((0.0, 1.0), (-1.0, 1.0)):
        out = []
        for siting in ref.SITINGS:
            planes = offset_planes(h, w, layout, 2)[1]
            frames.emit(sr, h, w, layout, lohi, out=planes, siting=siting)
            out.append(planes_to_numpy(planes, layout))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][0], out[2][0])
        assert int(out[0][0].max()) > 0
        if h > 1 and w > 2:
            assert not np.array_equal(out[0][1], out[1][1])                       # (center is not left)
        if info(layout)[0] == '422':
            assert all(np.array_equal(a, b) for a, b in zip(out[0], out[2]))     # 4:2:2: 'topleft' is 'left'


# ---- BT.2020 NCL: one size per layout kind
@pytest.mark.parametrize("yuv_range", ['limited', 'full'])
@pytest.mark.parametrize("case", [('i420', 'center'), ('p010', 'topleft'), ('nv16', 'center'), ('i444p10', 'left'), ('i444', 'left'),
                                  ('nv12', 'left')], ids=case_id)
def test_bt2020nc(case, yuv_range):
    layout, siting = case
    check_ingest(SIZES[3], layout, siting, 'reflect', 'bt2020nc', yuv_range)
    check_emit(EMIT_SHAPES[3], layout, siting, (0.0, 1.0), 'bt2020nc', yuv_range)
    check_emit(EMIT_SHAPES[1], layout, siting, (-1.0, 1.0), 'bt2020nc', yuv_range)


def test_444_takes_a_siting_and_ignores_it():
    (h, w), _ = SIZES[1]
    levels = random_levels(h, w, 'i444', 2)
    src = gpu_planes([ref.samples_of(p, 'i444') for p in levels], 'i444')
    a = frames.ingest(src, 'i444', 4, 'reflect')
    for siting in ('center', 'topleft'):
        assert torch.equal(frames.ingest(src, 'i444', 4, 'reflect', siting=siting), a)
    u8 = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (h, w, 3)).astype(np.uint8)).cuda()
    assert torch.equal(frames.ingest(u8, siting='topleft'), frames.ingest(u8))


# ---- 'left' is what it always was
@pytest.mark.parametrize("layout", ['nv12', 'p010'])
def test_left_gives_the_bytes_of_a_call_without_siting(layout):
    for (h, w), (Hp, Wp) in SIZES:
        levels = random_levels(h, w, layout, 9)
        src = gpu_planes([ref.samples_of(p, layout) for p in levels], layout)
        a, b = frames.ingest(src, layout, 4, 'reflect'), frames.ingest(src, layout, 4, 'reflect', siting='left')
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        sr = torch.from_numpy(np.random.RandomState(h).uniform(-0.2, 1.2, (3, Hp, Wp)).astype(np.float32)).cuda()
        pa, pb = offset_planes(h, w, layout, 3)[1], offset_planes(h, w, layout, 3)[1]
        frames.emit(sr, h, w, layout, out=pa)
        frames.emit(sr, h, w, layout, out=pb, siting='left')
        assert all(same(x, y) for x, y in zip(pa, pb))


# ---- the stream plan
def make_net(sd):
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    net = EDVR()
    net.load_state_dict(sd, strict=True)
    return net.cuda()


def test_extract_frame_of_a_center_sited_frame_is_ingest_then_extract():
    h, w, Hp, Wp = 18, 22, 20, 24
    net = make_net(synth.edvr_state_dict(0))
    leaves = net.ordered_parameters()
    plan = engine.StreamPlan(net._cfg(), Hp, Wp, 6)
    layout = 'i420'
    levels = random_levels(h, w, layout, 3)
    src = gpu_planes([ref.samples_of(p, layout) for p in levels], layout)
    caches = []
    for fused in (True, False):
        cache = plan.new_cache(src[0].device)
        cache.view(torch.float32).fill_(float('nan'))
        if fused:
            plan.extract_frame(leaves, src, 2, cache, layout, 'reflect', siting='center')
        else:
            plan.extract(leaves, frames.ingest(src, layout, 4, 'reflect', siting='center'), 2, cache)
        torch.cuda.synchronize()
        caches.append(cache.view(torch.float32).view(6, -1).cpu())
    a, b = caches
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))          # the whole slot, gaps (NaN) included
    want = ref.ingest(*levels, Hp, Wp, layout, 'reflect', siting='center').reshape(-1)
    raw = a[2][torch.isfinite(a[2])][-want.size:].numpy().astype(np.float64)    # the slot's last section is the padded frame
    assert float(np.abs(raw - want).max()) <= 1e-6
    left = ref.ingest(*levels, Hp, Wp, layout, 'reflect').reshape(-1)
    assert float(np.abs(raw - left).max()) > 1e-3                               # (and not the left-sited frame)


# ---- end to end: a 7-frame p010 topleft bt2020nc video
T = 7
KW = dict(layout='p010', siting='topleft', matrix='bt2020nc')
_E2E = {}


def e2e_case():
    """Computed once and never modified: synth.clip content turned into p010 samples by the restatement, and the CPU oracle's
    frames 0, 3 and 6 on the restated (fp64-converted) padded windows, cropped."""
    if not _E2E:
        from oracle import edvr as oedvr
        h, w, layout = 18, 22, 'p010'
        sd = synth.damp_residual_branch(synth.edvr_state_dict(0), 0.02)
        Hp, Wp = frames.padded_size(h, w, 4)
        rgb = synth.clip(90 + h, 1, T, h, w)[0]                                                        # [T,3,h,w] in [0,1]
        conv = dict(matrix='bt2020nc', yuv_range='limited', siting='topleft')
        levels = [[ref.round_levels(v, layout) for v in ref.emit(rgb[i].numpy(), h, w, layout, **conv)] for i in range(T)]
        samples = [[ref.samples_of(p, layout) for p in lv] for lv in levels]
        video_ = torch.from_numpy(np.stack([ref.pack(*p, layout) for p in samples]))                   # packed, on the host
        padded = torch.from_numpy(np.stack([ref.ingest(*lv, Hp, Wp, layout, 'reflect', **conv) for lv in levels])).float()
        oracle = {}
        for i in (0, 3, 6):
            with torch.no_grad():
                oracle[i] = oedvr.edvr_forward(sd, padded[index_generation(i, T, 5, 'new_info')][None])[:, :, :4 * h, :4 * w]
        _E2E.update(net=make_net(sd), video=video_, oracle=oracle, h=h, w=w)
    return _E2E


def run(net, frames_, opt=OPT, **kw):
    kw.setdefault('padding', 'new_info')
    return [sr.clone() for sr in video.super_resolve_frames(opt, net, frames_, **kw)]


def emitted_by_the_rule(out, flt, h, w, layout, **conv):
    """A device frame `out` (packed) holds the samples of the fp32 frame `flt` by the emit rule."""
    levels = ref.emit(flt[0].cpu().numpy(), h, w, layout, **conv)
    check_samples(ref.unpack(packed_numpy(out), layout), levels, layout, 'video')


def test_video_end_to_end():
    c = e2e_case()
    h, w, net = c['h'], c['w'], c['net']
    flt = run(net, c['video'].cuda(), in_flight=2, out='float', **KW)
    assert len(flt) == T and all(o.shape == (1, 3, 4 * h, 4 * w) for o in flt)
    for i, yo in c['oracle'].items():                                           # against the CPU oracle on the restated input
        y = flt[i].cpu()
        e, d = relerr(y, yo), float((y - yo).abs().max())
        print("p010 topleft bt2020nc frame %d: rel-L2 %.3e max-abs %.3e" % (i, e, d))
        assert e < 2e-4 and d < 1e-3, (i, e, d)
    out = run(net, c['video'], in_flight=2, **KW)                               # samples out, in the input's layout
    conv = dict(matrix='bt2020nc', yuv_range='limited', siting='topleft')
    for i in range(T):
        assert out[i].dtype == torch.uint16 and out[i].shape == (6 * h, 4 * w) and out[i].is_cuda
        assert same(out[i], frames.emit(flt[i], 4 * h, 4 * w, 'p010', **conv)), i
        emitted_by_the_rule(out[i], flt[i], 4 * h, 4 * w, 'p010', **conv)
    left = run(net, c['video'].cuda(), in_flight=2, out='float', layout='p010', matrix='bt2020nc')
    assert not torch.equal(left[3], flt[3])                                     # (the siting reached the frame cache)


def test_video_with_out_size_and_flip_test():
    c = e2e_case()
    h, w, net = c['h'], c['w'], c['net']
    conv = dict(matrix='bt2020nc', yuv_range='limited', siting='topleft')
    flt = run(net, c['video'].cuda(), in_flight=2, out='float', **KW)
    sized = run(net, c['video'].cuda(), in_flight=2, out_size=(54, 66), **KW)
    flt_sized = run(net, c['video'].cuda(), in_flight=2, out='float', out_size=(54, 66), **KW)
    for i in range(T):
        assert sized[i].dtype == torch.uint16 and sized[i].shape == (81, 66)
        assert same(sized[i], frames.emit(flt[i], 4 * h, 4 * w, 'p010', size=(54, 66), **conv)), i
        assert same(sized[i], frames.emit(flt_sized[i], 54, 66, 'p010', **conv)), i
        emitted_by_the_rule(sized[i], flt_sized[i], 54, 66, 'p010', **conv)
    flip_flt = run(net, c['video'].cuda(), in_flight=2, out='float', flip_test=True, **KW)
    flip = run(net, c['video'].cuda(), in_flight=2, flip_test=True, **KW)
    for i in range(T):
        assert same(flip[i], frames.emit(flip_flt[i], 4 * h, 4 * w, 'p010', **conv)), i
    assert not torch.equal(flip_flt[3], flt[3])                                 # (the ensemble ran)


def test_non_edvr_network_takes_center_sited_i420_frames():
    """The `Mean` stand-in of test_gpu_frame_io.py: frames.ingest per frame, the windows through super_resolve_video,
    frames.emit per result."""
    calls = []

    class Mean(torch.nn.Module):
        nframes = 3

        def forward(self, x):
            calls.append(tuple(x.shape))
            return x.mean(1)

    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    levels = [random_levels(8, 10, 'i420', 20 + i) for i in range(5)]
    frames_ = torch.from_numpy(np.stack([ref.pack(*[ref.samples_of(p, 'i420') for p in lv], 'i420') for lv in levels]))   # [5,12,10]
    conv = dict(matrix='bt709', yuv_range='full', siting='center')
    kw = dict(padding='replicate', multiple=4, layout='i420', **conv)
    out = run(Mean(), frames_, opt, **kw)
    flt = run(Mean(), frames_.cuda(), opt, out='float', **kw)
    assert len(out) == 5 and calls == [(1, 3, 3, 8, 12)] * 10
    padded = np.stack([ref.ingest(*lv, 8, 12, 'i420', 'reflect', **conv) for lv in levels])
    for i in range(5):
        want = padded[index_generation(i, 5, 3, 'replicate')].mean(0)[:, :8, :10]
        # three ingested values, each within 1e-6, and the three fp32 roundings of their mean (<= 6e-8 each)
        assert flt[i].shape == (1, 3, 8, 10) and float(np.abs(flt[i][0].cpu().numpy() - want).max()) <= 1.2e-6, i
        assert out[i].dtype == torch.uint8 and out[i].shape == (12, 10)
        assert torch.equal(out[i], frames.emit(flt[i], 8, 10, 'i420', **conv)), i
        emitted_by_the_rule(out[i], flt[i], 8, 10, 'i420', **conv)
