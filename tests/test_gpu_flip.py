"""GPU: the flip-test x4 self-ensemble (csrc/frame_flip.hip, frames.flip / frames.flip_mean,
adapt.super_resolve_frames(flip_test=True), adapt.super_resolve_video(flip_test=True)).

Bars:
  kernels  the bits of torch: flip moves values, and flip_mean's three additions and its exact * 0.25 are the statements of
           the torch composition in the same order.  A NaN compares unequal to itself, so the outputs are compared as
           integers where the reference is not NaN, and the NaNs must sit where the reference has them (a NaN's payload
           is not part of the definition).
  video    flip_test=True is bit-identical to the composition of today's calls: super_resolve_frames(out='float') on the
           ingested (padded) video and on its three torch.flips, un-flipped and summed with torch in the reference's order,
           then frames.emit -- every launch is deterministic and the composition issues the same ones on the same data.
  oracle   rel-L2 < 2e-4 and max-abs < 1e-3 against the CPU oracle on the four flips of the padded window, combined the same
           way: the forward parity bar (test_gpu_stream.py); the mean of four outputs that each meet it meets it (measured: rel-L2
           5.3e-8, max-abs 1.8e-7)."""
import numpy as np
import pytest
import torch

import flip_ref as ref
from conftest import relerr
from dynavsr_amd import _lib as L
from dynavsr_amd import adapt, engine, frames, synth
from dynavsr_amd.data.util import index_generation

pytestmark = pytest.mark.gpu

OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
DIMS = {1: (-1,), 2: (-2,), 3: (-2, -1)}
SENTINEL = -123.5
GUARD = 512                      # floats in front of and behind a tensor


def tflip(x, flags):
    return x if flags == 0 else torch.flip(x, DIMS[flags])


def combine(y0, yw, yh, yhw):
    """flipx4_forward's statements (utils/util.py:232-254), with torch."""
    return (((y0 + yw.flip(-1)) + yh.flip(-2)) + yhw.flip((-2, -1))) * 0.25


def ints(x):
    return x.contiguous().view(torch.int32)


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.uint16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return torch.equal(ints(a), ints(b)) if a.dtype == torch.float32 else torch.equal(a, b)


def same_bits_nan_aware(got, want):
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(ints(got)[~nan], ints(want)[~nan])


def guarded(host, fill=SENTINEL):
    """(the whole buffer, a 16-byte aligned view of host's shape in its middle holding host) on the GPU."""
    n = host.numel()
    buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device='cuda')
    view = buf[GUARD:GUARD + n].view(host.shape)
    view.copy_(host)
    assert view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


# ---- 1, 2: the kernels against torch, inside guard bands -------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_flip_is_torch_flip(shape):
    host = torch.from_numpy(ref.data(shape, sum(shape)))
    sbuf, src = guarded(host)
    before = sbuf.clone()
    for flags in range(4):
        dbuf, dst = guarded(torch.zeros(shape))
        got = frames.flip(src, flags, out=dst)
        assert got.data_ptr() == dst.data_ptr()
        want = tflip(src, flags)
        assert torch.equal(ints(got), ints(want)), flags                # values only move: NaN and inf bits included
        assert np.array_equal(got.cpu().numpy().view(np.int32), ref.flip(host.numpy(), flags).view(np.int32))
        nan_at, inf_at = ref.special_places(shape, flags)
        flat = got.reshape(-1)
        assert bool(torch.isnan(flat[nan_at])) and float(flat[inf_at]) == float('inf')
        assert int(torch.isnan(flat).sum()) == 1 and int(torch.isinf(flat).sum()) == 1
        assert guards_intact(dbuf, host.numel()), flags                 # nothing in front of or behind dst
        fresh = frames.flip(src, flags)                                 # a tensor of the wrapper's own
        assert fresh.shape == src.shape and torch.equal(ints(fresh), ints(want))
    assert torch.equal(ints(sbuf), ints(before))                        # the source and its surroundings are only read


@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_flip_mean_is_the_torch_composition(shape):
    hosts = [torch.from_numpy(ref.data(shape, 7 * sum(shape) + i)) for i in range(4)]
    pairs = [guarded(h) for h in hosts]
    srcs = [v for _, v in pairs]
    before = [b.clone() for b, _ in pairs]
    want = combine(*srcs)
    dbuf, dst = guarded(torch.zeros(shape))
    got = frames.flip_mean(*srcs, out=dst)
    assert got.data_ptr() == dst.data_ptr()
    assert same_bits_nan_aware(got, want)
    assert int(torch.isnan(want).sum()) >= 1 and bool(torch.isinf(want).any() or shape == (1, 1, 4))
    host_want = ref.flip_mean(*[h.numpy() for h in hosts])
    assert same_bits_nan_aware(got.cpu(), torch.from_numpy(host_want))
    assert guards_intact(dbuf, hosts[0].numel())
    assert all(torch.equal(ints(b), ints(c)) for (b, _), c in zip(pairs, before))
    assert same_bits_nan_aware(frames.flip_mean(*srcs), want)


def test_five_dimensional_clip():
    """A clip [B,N,3,H,W] is planes = B N 3 planes of H x W."""
    clip = torch.from_numpy(np.random.RandomState(3).standard_normal((1, 5, 3, 7, 20)).astype(np.float32)).cuda()
    for flags in range(4):
        assert torch.equal(frames.flip(clip, flags), tflip(clip, flags))
    ys = [clip + i for i in range(4)]
    assert torch.equal(frames.flip_mean(*ys), combine(*ys))


# ---- 3: rejections at the C ABI, nothing launched --------------------------------------------------
def test_rejections_at_the_c_abi():
    l = L.lib()
    t = [torch.full((3, 4, 8), float(i), device='cuda') for i in range(5)]
    torch.cuda.synchronize()
    p = [x.data_ptr() for x in t]
    st = L.stream()
    inv = -1                                                            # DVSR_ERR_INVALID
    assert l.dvsr_frame_flip(None, p[1], 3, 4, 8, 1, st) == inv
    assert l.dvsr_frame_flip(p[0], None, 3, 4, 8, 1, st) == inv
    for planes, H, W in ((0, 4, 8), (3, 0, 8), (3, 4, 0), (-3, 4, 8), (3, 4, 6), (3, 4, 2)):
        assert l.dvsr_frame_flip(p[0], p[1], planes, H, W, 1, st) == inv, (planes, H, W)
        assert l.dvsr_frame_flip_mean(p[0], p[1], p[2], p[3], p[4], planes, H, W, st) == inv, (planes, H, W)
    for flags in (-1, 4, 8):
        assert l.dvsr_frame_flip(p[0], p[1], 3, 4, 8, flags, st) == inv, flags
    assert l.dvsr_frame_flip(p[0] + 4, p[1], 3, 4, 4, 1, st) == inv      # misaligned source / destination
    assert l.dvsr_frame_flip(p[0], p[1] + 4, 3, 4, 4, 1, st) == inv
    assert l.dvsr_frame_flip(p[0], p[0], 3, 4, 8, 1, st) == inv          # in place
    for i in range(5):
        q = list(p)
        q[i] = None
        assert l.dvsr_frame_flip_mean(*q, 3, 4, 8, st) == inv, i
        q[i] = p[i] + 4
        assert l.dvsr_frame_flip_mean(*q, 3, 4, 4, st) == inv, i
    for i in range(4):
        q = list(p)
        q[4] = p[i]
        assert l.dvsr_frame_flip_mean(*q, 3, 4, 8, st) == inv, i
    torch.cuda.synchronize()
    for i, x in enumerate(t):                                           # nothing was launched: nothing was written
        assert bool((x == float(i)).all())
    assert l.dvsr_frame_flip(p[0], p[1], 3, 4, 8, 3, st) == 0            # and the good call still works
    assert torch.equal(t[1], t[0])


# ---- 4 - 6, 8: the video path, EDVR ----------------------------------------------------------------
T = 7
_CASE = {}


def make_net(sd):
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    net = EDVR()
    net.load_state_dict(sd, strict=True)
    return net.cuda()


def run(net, video, **kw):
    kw.setdefault('padding', 'new_info')
    return [sr.clone() for sr in adapt.super_resolve_frames(OPT, net, video, **kw)]


def case(h, w):
    """Per size, computed once and never modified: the tiny EDVR of test_gpu_resize.py, the 8-bit video, today's float SR
    frames of it, and the COMPOSITION -- today's call on the ingested video and on its three torch.flips, combined by torch."""
    key = (h, w)
    if key not in _CASE:
        sd = synth.damp_residual_branch(synth.edvr_state_dict(0), 0.02)
        net = make_net(sd)
        u8 = (synth.clip(90 + h, 1, T, h, w)[0] * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # [T,h,w,3]
        dev = u8.cuda()
        padded = torch.stack([frames.ingest(dev[i], 'hwc_rgb', 4, 'reflect') for i in range(T)])                  # [T,3,Hp,Wp]
        ys = [run(net, tflip(padded, v).contiguous(), out='float') for v in range(4)]
        composed = [combine(ys[0][i], ys[1][i], ys[2][i], ys[3][i]) for i in range(T)]                            # [1,3,4Hp,4Wp]
        today = run(net, dev, out='float')
        _CASE[key] = dict(sd=sd, net=net, u8=u8, dev=dev, composed=composed, today=today)
    return _CASE[key]


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("hw", [(18, 22), (13, 15)])
def test_video_equals_the_composition_of_todays_calls(hw, in_flight):
    h, w = hw
    c = case(h, w)
    net, u8, composed, today = c['net'], c['dev'], c['composed'], c['today']
    sizes = [None, (50, 62)] if hw == (18, 22) else [None]
    for size in sizes:
        oh, ow = size if size is not None else (4 * h, 4 * w)
        shapes = {None: (oh, ow, 3), 'float': (1, 3, oh, ow), 'nv12': (oh * 3 // 2, ow)}
        for out, layout in ((None, 'hwc_rgb'), ('float', 'chw'), ('nv12', 'nv12')):
            got = run(net, u8, in_flight=in_flight, out=out, out_size=size, flip_test=True)
            assert len(got) == T
            for i in range(T):
                want = frames.emit(composed[i], 4 * h, 4 * w, layout, size=size)
                want = want[None] if out == 'float' else want
                assert tuple(got[i].shape) == shapes[out] and got[i].is_cuda, (size, out, i)
                if not same_bits(got[i], want):
                    d = (got[i].double() - want.double()).abs()
                    print("size %s out %s frame %d: %d values differ, max-abs %.3e" % (size, out, i, int((d > 0).sum()), float(d.max())))
                assert same_bits(got[i], want), (size, out, i)
    # the flag does something: the synthetic frames are not symmetric ...
    flipped = run(net, u8, in_flight=in_flight, out='float', flip_test=True)
    assert any(not torch.equal(a, b) for a, b in zip(flipped, today))
    # ... and False is today's call, bit for bit
    plain = run(net, u8, in_flight=in_flight, out='float', flip_test=False)
    assert all(same_bits(a, b) for a, b in zip(plain, today))


def test_parity_with_the_cpu_oracle():
    import torch.nn.functional as F
    from oracle import edvr as oedvr
    h, w = 18, 22
    c = case(h, w)
    Hp, Wp = frames.padded_size(h, w, 4)
    flt = torch.from_numpy(np.ascontiguousarray(np.transpose(c['u8'].numpy().astype(np.float32) / 255., (0, 3, 1, 2))))
    padded = F.pad(flt, (0, Wp - w, 0, Hp - h), mode='reflect')
    got = run(c['net'], c['dev'], out='float', flip_test=True)
    for i in (0, 3):
        win = padded[index_generation(i, T, 5, 'new_info')][None]
        with torch.no_grad():
            ys = [oedvr.edvr_forward(c['sd'], tflip(win, v).contiguous()) for v in range(4)]
        want = combine(*ys)[:, :, :4 * h, :4 * w]
        y = got[i].cpu()
        e, d = relerr(y, want), float((y - want).abs().max())
        print("flip_test frame %d: rel-L2 %.3e max-abs %.3e" % (i, e, d))
        assert e < 2e-4 and d < 1e-3, (i, e, d)


def test_scenes_stay_independent():
    c = case(18, 22)
    net, u8 = c['net'], c['dev']
    got = run(net, u8, padding='replicate', cuts=[3], flip_test=True)
    want = run(net, u8[:3], padding='replicate', flip_test=True) + run(net, u8[3:], padding='replicate', flip_test=True)
    assert len(got) == T == len(want)
    for i in range(T):
        assert got[i].dtype == torch.uint8 and torch.equal(got[i], want[i]), i
    flt = run(net, u8, padding='replicate', cuts=[3], out='float', flip_test=True)
    alone = run(net, u8[:3], padding='replicate', out='float', flip_test=True) + \
        run(net, u8[3:], padding='replicate', out='float', flip_test=True)
    assert all(same_bits(a, b) for a, b in zip(flt, alone))


@pytest.mark.parametrize("in_flight", [1, 2])
def test_call_counts(in_flight):
    """A frame size that is this test's alone (12 x 16 bytes), so that the plans it finds are those its own calls made."""
    c = case(18, 22)
    net, u8 = c['net'], c['dev'][:, :12, :16]
    slots = adapt.stream_slots(5, in_flight, 1)

    def plans(n):
        return [p for p in engine._splans.values() if (p.h, p.w, p.slots) == (12, 16, n)]
    had_wide = bool(plans(4 * slots))                                   # (only when the test runs twice in one process)
    run(net, u8, in_flight=in_flight)                                   # (creates the plan of `slots` slots if need be)
    narrow, = plans(slots)
    before = dict(narrow.stats)
    run(net, u8, in_flight=in_flight, flip_test=False)
    assert narrow.stats['extracted'] - before['extracted'] == T and narrow.stats['fused'] - before['fused'] == T
    assert bool(plans(4 * slots)) == had_wide                           # False builds no plan of 4 x slots slots
    run(net, u8, in_flight=in_flight, flip_test=True)
    wide, = plans(4 * slots)
    before, narrow_before = dict(wide.stats), dict(narrow.stats)
    run(net, u8, in_flight=in_flight, flip_test=True)
    assert wide.stats['extracted'] - before['extracted'] == 4 * T
    assert wide.stats['fused'] - before['fused'] == 4 * T
    assert narrow.stats == narrow_before


# ---- 7: other networks ------------------------------------------------------------------------------
class Mean(torch.nn.Module):
    """test_gpu_resize.py::test_non_edvr_network_at_a_target_size's: flip-equivariant."""
    nframes = 3

    def forward(self, x):
        return x.mean(1)


class Ramp(torch.nn.Module):
    """NOT flip-equivariant: adds a fixed ramp along x (and a smaller one along y)."""
    nframes = 3

    def forward(self, x):
        rx = torch.arange(x.shape[-1], dtype=torch.float32, device=x.device) * 0.03125
        ry = torch.arange(x.shape[-2], dtype=torch.float32, device=x.device)[:, None] * 0.0078125
        return x.mean(1) * 0.5 + rx + ry


@pytest.mark.parametrize("net", [Mean(), Ramp()], ids=["mean", "ramp"])
def test_other_networks(net):
    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    rs = np.random.RandomState(12)
    clips = [torch.from_numpy(rs.uniform(0, 1, (1, 3, 3, 6, 12)).astype(np.float32)).cuda() for _ in range(4)]

    def composed(clip):
        return combine(*[net(tflip(clip, v)) for v in range(4)])
    for in_flight in (1, 2):
        got = [o.clone() for o in adapt.super_resolve_video(opt, net, clips, in_flight, flip_test=True)]
        assert len(got) == 4
        for g, clip in zip(got, clips):
            assert g.shape == (1, 3, 6, 12) and torch.equal(g, composed(clip))
        plain = [o.clone() for o in adapt.super_resolve_video(opt, net, clips, in_flight)]
        assert all(torch.equal(p, net(clip)) for p, clip in zip(plain, clips))
    if isinstance(net, Ramp):
        assert not torch.equal(got[0], net(clips[0]))                   # the ensemble of a network that is not equivariant differs
    # through super_resolve_frames: float frames of a size taken as it is, and bytes that are padded (7 x 9 -> 8 x 12)
    video = torch.from_numpy(rs.uniform(0, 1, (5, 3, 6, 12)).astype(np.float32)).cuda()
    got = [o.clone() for o in adapt.super_resolve_frames(opt, net, video, padding='replicate', flip_test=True)]
    for i, g in enumerate(got):
        win = video[index_generation(i, 5, 3, 'replicate')][None]
        assert torch.equal(g, composed(win)), i
    u8 = torch.from_numpy(rs.randint(0, 256, (5, 7, 9, 3)).astype(np.uint8)).cuda()
    padded = torch.stack([frames.ingest(u8[i], 'hwc_rgb', 4, 'reflect') for i in range(5)])
    for out, layout in ((None, 'hwc_rgb'), ('float', 'chw')):
        got = [o.clone() for o in adapt.super_resolve_frames(opt, net, u8, padding='replicate', multiple=4, out=out, flip_test=True)]
        for i, g in enumerate(got):
            want = frames.emit(composed(padded[index_generation(i, 5, 3, 'replicate')][None]), 7, 9, layout)
            assert same_bits(g, want[None] if out == 'float' else want), (out, i)
