"""GPU: the streaming EDVR video forward (adapt.super_resolve_frames over engine.StreamPlan / dvsr_edvr_stream_*): every
frame's features extracted once into a frame cache, one gather + the tape from PCD alignment on per window.

Bars are the project's own forward parity bars (tests/test_gpu_edvr.py): rel-L2 < 2e-4 and max-abs < 1e-3, against the
per-clip forward `net(clip)` and against the CPU oracle.  (Extraction runs at batch 1 instead of the clip's batch 5 and may
take other kernel kinds, so streaming vs per-clip is parity, not bit-identity.)"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import relerr
from dynavsr_amd import adapt, engine, synth
from dynavsr_amd import _lib as L
from dynavsr_amd.data.util import index_generation

pytestmark = pytest.mark.gpu

MODES = ('replicate', 'reflection', 'new_info', 'circle')
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}


def make_net(seed=0):
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    net = EDVR()
    net.load_state_dict(synth.edvr_state_dict(seed), strict=True)
    return net.cuda()


def run_stream(net, frames, mode='new_info', in_flight=2):
    """All SR frames of a video, cloned as they are yielded (a yielded frame is only valid for in_flight advances)."""
    return [sr.clone() for sr in adapt.super_resolve_frames(OPT, net, frames, padding=mode, in_flight=in_flight)]


def per_clip(net, video, i, mode):
    with torch.no_grad():
        return net(video[index_generation(i, video.shape[0], 5, mode)][None])


def assert_bar(y, ref, what):
    e, d = relerr(y, ref), float((y.detach().cpu() - torch.as_tensor(ref).detach().cpu()).abs().max())
    print("%s: rel-L2 %.3e max-abs %.3e" % (what, e, d))
    assert e < 2e-4 and d < 1e-3, (what, e, d)


@pytest.mark.parametrize("hw", [(32, 48), (24, 40)])
@pytest.mark.parametrize("mode", MODES)
def test_stream_matches_per_clip_and_oracle(hw, mode):
    from oracle import edvr as oedvr
    T = 9
    host = synth.clip(70 + hw[0], 1, T, *hw)[0]
    video = host.cuda()
    net = make_net(0)
    out = run_stream(net, video, mode)
    assert len(out) == T and all(o.shape == (1, 3, 4 * hw[0], 4 * hw[1]) for o in out)
    for i in range(T):
        assert_bar(out[i], per_clip(net, video, i, mode), "stream vs per-clip %s %s frame %d" % (hw, mode, i))
    P = synth.edvr_state_dict(0)
    for i in (0, T // 2, T - 1):
        with torch.no_grad():
            yo = oedvr.edvr_forward(P, host[index_generation(i, T, 5, mode)][None])
        assert_bar(out[i], yo, "stream vs oracle %s %s frame %d" % (hw, mode, i))


def test_stream_results_do_not_depend_on_in_flight():
    video = synth.clip(81, 1, 9, 32, 48)[0].cuda()
    net = make_net(0)
    ref = run_stream(net, video, 'new_info', 1)
    for k in (2, 3):
        got = run_stream(net, video, 'new_info', k)
        assert all(torch.equal(a, b) for a, b in zip(ref, got)), k


def test_stream_counters_and_repacking():
    T = 9
    video, video2 = synth.clip(82, 1, T, 32, 48)[0].cuda(), synth.clip(83, 1, T, 32, 48)[0].cuda()
    net = make_net(0)
    plan = engine.get_stream_plan(net._cfg(), 32, 48, 5 + 2 - 1, video.device)
    plan.release()
    before = dict(plan.stats)
    run_stream(net, video)
    assert plan.stats['extracted'] - before['extracted'] == T
    assert plan.stats['fused'] - before['fused'] == T and plan.stats['gathers'] - before['gathers'] == T
    packs = plan.stats['packs']
    assert packs > before['packs']
    run_stream(net, video2)                                   # a second video through the same frozen net: nothing to pack
    assert plan.stats['packs'] == packs and plan.stats['extracted'] - before['extracted'] == 2 * T
    net.load_state_dict(synth.edvr_state_dict(3), strict=True)
    got = run_stream(net, video)
    assert plan.stats['packs'] > packs
    fresh = make_net(3)
    plan.release()
    want = run_stream(fresh, video)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def _raw_stream(net, h, w, slots):
    plan = engine.StreamPlan(net._cfg(), h, w, slots)
    leaves = net.ordered_parameters()
    return plan, leaves


def test_gather_indexing_at_the_c_abi():
    h, w = 32, 48
    net = make_net(0)
    frames = synth.clip(84, 1, 5, h, w)[0].cuda()
    plan, leaves = _raw_stream(net, h, w, 6)
    outs = []
    for order in ([3, 0, 4, 1, 2], [0, 1, 2, 3, 4]):
        cache = plan.new_cache(frames.device)
        cache.view(torch.float32).fill_(float('nan'))         # the unused slot and every gap stay NaN
        for f, slot in enumerate(order):
            plan.extract(leaves, frames[f].contiguous(), slot, cache)
        out = torch.full((1, 3, 4 * h, 4 * w), float('nan'), device=frames.device)
        plan.fuse(leaves, order, cache, out)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    with torch.no_grad():
        assert_bar(outs[0], net(frames[None]), "C ABI stream vs per-clip")


def test_error_paths_return_invalid_without_launching():
    h, w = 16, 16
    net = make_net(0)
    plan, leaves = _raw_stream(net, h, w, 6)
    dev = leaves[0].device
    params = [p.detach().contiguous() for p in leaves]
    arr = (ctypes.c_void_p * len(params))(*[p.data_ptr() for p in params])
    cache = plan.new_cache(dev)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
    frame = torch.zeros(3, h, w, device=dev)
    out = torch.full((1, 3, 4 * h, 4 * w), 7.0, device=dev)
    cache.zero_()
    lib, st = L.lib(), L.stream()
    INVALID = -1

    def extract(slot, cache_bytes=plan.cache_bytes, ws_bytes=plan.workspace_bytes, frame_ptr=frame.data_ptr()):
        return lib.dvsr_edvr_stream_extract(plan._h, arr, frame_ptr, slot, cache.data_ptr(), cache_bytes, ws.data_ptr(),
                                            ws_bytes, 0, st)

    def fuse(slots, cache_bytes=plan.cache_bytes, ws_bytes=plan.workspace_bytes):
        sl = (ctypes.c_int * 5)(*slots)
        return lib.dvsr_edvr_stream_fuse(plan._h, arr, sl, cache.data_ptr(), cache_bytes, out.data_ptr(), ws.data_ptr(),
                                         ws_bytes, 0, st)

    assert extract(6) == INVALID and b"slot" in lib.dvsr_last_error()
    assert extract(-1) == INVALID
    assert extract(0, ws_bytes=plan.workspace_bytes - 4) == INVALID and b"workspace" in lib.dvsr_last_error()
    assert extract(0, cache_bytes=plan.cache_bytes - 4) == INVALID and b"cache" in lib.dvsr_last_error()
    assert extract(0, frame_ptr=None) == INVALID
    assert fuse([0, 1, 2, 3, 6]) == INVALID and b"slots[4]" in lib.dvsr_last_error()
    assert fuse([0, 1, 2, 3, 4], ws_bytes=plan.workspace_bytes - 4) == INVALID
    assert fuse([0, 1, 2, 3, 4], cache_bytes=plan.cache_bytes - 4) == INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((cache == 0).all())        # nothing was launched
    h_ = ctypes.c_void_p()
    assert lib.dvsr_edvr_stream_create(L.EdvrConfig(*net._cfg()), h, w, 4, ctypes.byref(h_)) == INVALID   # slots < nframes
    assert lib.dvsr_edvr_stream_create(L.EdvrConfig(*net._cfg()), 18, w, 6, ctypes.byref(h_)) == INVALID


def test_stream_full_size():
    from oracle import edvr as oedvr
    T, mode = 8, 'new_info'
    host = synth.clip(1, 1, T, 180, 320, smooth=False)[0]
    video = host.cuda()
    net = make_net(0)
    out = run_stream(net, video, mode, 2)
    for i in range(T):
        assert_bar(out[i], per_clip(net, video, i, mode), "full size, stream vs per-clip, frame %d" % i)
    i = 3
    with torch.no_grad():
        yo = oedvr.edvr_forward(synth.edvr_state_dict(0), host[index_generation(i, T, 5, mode)][None])
    y = out[i].cpu()
    d = (y - yo).abs()
    assert y.shape == (1, 3, 720, 1280)
    assert float(d.max()) <= 1e-3, float(d.max())
    assert relerr(y, yo) < 2e-4
    assert 10 * np.log10(1.0 / float(((y - yo) ** 2).mean())) >= 60.0
    engine.release_stream_plans()


def test_stream_mixed_use():
    net = make_net(0)
    a = synth.clip(85, 1, 7, 32, 48)[0]                       # CPU-resident frames, as a list
    b = synth.clip(86, 1, 6, 24, 40)[0].cuda()
    wide = synth.clip(87, 1, 7, 32, 96)[0].cuda()
    view = wide[..., ::2]                                     # a non-contiguous [T,3,32,48] view
    assert not view[0].is_contiguous()
    ga, gb = a.cuda(), b
    out_a = run_stream(net, [a[i] for i in range(7)], 'reflection')
    out_b = run_stream(net, b, 'replicate', 3)
    out_v = run_stream(net, view, 'new_info')
    for i in range(7):
        assert_bar(out_a[i], per_clip(net, ga, i, 'reflection'), "CPU frames, frame %d" % i)
        assert_bar(out_v[i], per_clip(net, view.contiguous(), i, 'new_info'), "strided view, frame %d" % i)
    for i in range(6):
        assert_bar(out_b[i], per_clip(net, gb, i, 'replicate'), "second size, frame %d" % i)
    # early close, then an ordinary forward: it must come behind whatever the generator left running
    want0 = run_stream(net, ga, 'new_info', 2)[0]
    net.train()
    gen = adapt.super_resolve_frames(OPT, net, ga, in_flight=2)
    first = next(gen).clone()
    next(gen)
    gen.close()
    assert net.training
    assert torch.equal(first, want0)
    clip = ga[index_generation(3, 7, 5, 'new_info')][None]
    with torch.no_grad():
        y = net(clip)
    fresh = make_net(0)
    with torch.no_grad():
        assert torch.equal(y, fresh(clip))


def test_non_edvr_network_delegates_to_per_clip_windows():
    """A backbone without the split tape takes index_generation's windows through super_resolve_video: same interface."""
    calls = []

    class Mean(torch.nn.Module):
        nframes = 3

        def forward(self, x):
            calls.append(tuple(x.shape))
            return x.mean(1)

    video = synth.clip(88, 1, 5, 8, 8)[0].cuda()
    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    out = [o.clone() for o in adapt.super_resolve_frames(opt, Mean(), video, padding='replicate')]
    assert len(out) == 5 and calls == [(1, 3, 3, 8, 8)] * 5
    for i in range(5):
        assert torch.equal(out[i], video[index_generation(i, 5, 3, 'replicate')][None].mean(1))
