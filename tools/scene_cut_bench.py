#!/usr/bin/env python3
"""Scene cuts (csrc/frame_cut.hip, frames.luma_sad / detect_cuts, super_resolve_frames(cuts=...)) measured, in one process:

1. dvsr_frame_luma_sad on a device-resident video of `--pairs` + 1 frames, 'hwc_rgb' and 'nv12', at 180x320 and 1080x1920:
   `--calls` back-to-back calls through the C ABI (each one: the memset of the sums + one launch over all pairs) captured into
   one graph whose replay is timed by hipEvents, `--repeats` repetitions; bytes read per second from the algorithmic bytes
   (every pair reads both of its frames once: 2 x pairs x the bytes of a frame -- the Y plane alone for NV12).
   Beside it, alternated, the torch-op composition of the same integer arithmetic on the same frames (widen, luma, subtract,
   abs, sum), captured and timed the same way and checked to give the same sums.  The composition is the BASELINE, not the
   kernel under test.
2. frames/s of a uint8 video without cuts in PINNED host memory -> uint8 SR frames on the host (EDVR-M x4), through
   cuts=None (the path of before) and through cuts='auto' (luma_sad over the whole video first), alternated, `--video-repeats`
   timed passes each after a warm-up pass.  The overhead of 'auto' is accepted if it lies inside the max - min spread of the
   cuts=None runs; otherwise the figure stands as measured.

usage (GPU box): python tools/scene_cut_bench.py [--pairs 8 --calls 50 --repeats 10 --frames 100 --video-repeats 5]
                 > profiles/r11_scene_cuts.txt"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dynavsr_amd  # noqa: E402
dynavsr_amd.configure_runtime()
from dynavsr_amd import _lib as L  # noqa: E402
from dynavsr_amd import adapt, frames, synth  # noqa: E402
from dynavsr_amd.models.archs.EDVR_arch import EDVR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--h", type=int, default=180)
ap.add_argument("--w", type=int, default=320)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--video-repeats", type=int, default=5)
ap.add_argument("--in-flight", type=int, default=2)
args = ap.parse_args()
print("# scene cuts; %s; %d pairs per call, %d calls per replay, %d repetitions alternated" % (
    torch.cuda.get_device_name(0), args.pairs, args.calls, args.repeats))
lib = L.lib()
r = np.random.RandomState(0)


def graph_us(launch, n):
    """Device time per call: `n` back-to-back calls captured into one graph; returns a function that replays and times it."""
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            launch()
    g.replay()
    torch.cuda.synchronize()

    def timed_replay():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n
    return timed_replay


def torch_sad_rgb(v, out):
    x = v.to(torch.int32)
    y = (77 * x[..., 0] + 150 * x[..., 1] + 29 * x[..., 2] + 128) >> 8
    out.copy_((y[1:] - y[:-1]).abs().sum((1, 2)))


def torch_sad_y(v, h, out):
    y = v[:, :h].to(torch.int32)
    out.copy_((y[1:] - y[:-1]).abs().sum((1, 2)))


T = args.pairs + 1
for (h, w) in ((180, 320), (1080, 1920)):
    rgb = torch.from_numpy(r.randint(0, 256, (T, h, w, 3)).astype(np.uint8)).cuda()
    nv12 = torch.from_numpy(r.randint(0, 256, (T, h * 3 // 2, w)).astype(np.uint8)).cuda()
    for name, video, fields, stride, nbytes, base in (
            ("hwc_rgb", rgb, (L.FRAME_U8_HWC_RGB, h, w, 3 * w, 0, 3), 3 * h * w, 2 * args.pairs * 3 * h * w,
             lambda out: torch_sad_rgb(rgb, out)),
            ("nv12", nv12, (L.FRAME_U8_Y, h, w, w, 0, 1), h * 3 // 2 * w, 2 * args.pairs * h * w,
             lambda out: torch_sad_y(nv12, h, out))):
        desc = L.FrameDesc(*fields)
        sad = torch.zeros((args.pairs,), dtype=torch.int64, device='cuda')
        ref = torch.zeros((args.pairs,), dtype=torch.int64, device='cuda')

        def kernel():
            L.check(lib.dvsr_frame_luma_sad(video.data_ptr(), video[1].data_ptr(), ctypes.byref(desc), stride, args.pairs,
                                            sad.data_ptr(), L.stream()), "dvsr_frame_luma_sad")

        tk, tb = graph_us(kernel, args.calls), graph_us(lambda: base(ref), args.calls)
        assert torch.equal(sad, ref) and torch.equal(sad.cpu(), frames.luma_sad(video, name)), "the sums differ"
        uk, ub = [], []
        for _ in range(args.repeats):
            uk.append(tk())
            ub.append(tb())
        mk, mb = statistics.median(uk), statistics.median(ub)
        print("luma_sad %-7s %4dx%-4d %d pairs: %8.2f us per call (spread %6.2f), %7.2f MB read -> %6.3f TB/s   |  torch-op "
              "composition (baseline) %9.2f us per call (spread %7.2f) -> %6.3f TB/s of the same bytes; same sums" % (
                  name, h, w, args.pairs, mk, max(uk) - min(uk), nbytes / 1e6, nbytes / mk / 1e6, mb, max(ub) - min(ub),
                  nbytes / mb / 1e6))
    del rgb, nv12

# ---- 2. cuts=None against cuts='auto' on a video without cuts
H, W, N = args.h, args.w, args.frames
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
net = EDVR()
net.load_state_dict(synth.edvr_state_dict(0))
net = net.cuda()
yy, xx = np.mgrid[0:H, 0:W + N].astype(np.float64)
field = np.stack([128 + 40 * (np.sin(2 * np.pi * xx / 61.0 + c) + np.sin(2 * np.pi * yy / 47.0 + 2 * c)) for c in range(3)], -1)
field = np.clip(np.rint(field), 0, 255).astype(np.uint8)
video = torch.from_numpy(np.ascontiguousarray(np.stack([field[:, t:t + W] for t in range(N)]))).pin_memory()   # one scene, panning
host_out = torch.empty((N, 4 * H, 4 * W, 3), dtype=torch.uint8).pin_memory()
found = frames.detect_cuts(video)
print("video %d frames uint8 %dx%d pinned host -> uint8 %dx%d host, in_flight %d; detect_cuts finds %s" % (
    N, H, W, 4 * H, 4 * W, args.in_flight, found))
assert found == [], "the video of this measurement must be one scene"


def run(cuts):
    for i, sr in enumerate(adapt.super_resolve_frames(OPT, net, video, in_flight=args.in_flight, cuts=cuts)):
        host_out[i].copy_(sr, non_blocking=True)
    torch.cuda.synchronize()


def timed(cuts):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(cuts)
    return N / (time.perf_counter() - t0)


run(None)
a = host_out.clone()
run('auto')
assert torch.equal(a, host_out), "cuts='auto' on one scene must give cuts=None's frames"
del a
fn, fa = [], []
for _ in range(args.video_repeats):
    fn.append(timed(None))
    fa.append(timed('auto'))
mn, ma, sn = statistics.median(fn), statistics.median(fa), max(fn) - min(fn)
print("  cuts=None   median %7.1f frames/s  spread %5.1f  (%s)" % (mn, sn, " ".join("%.1f" % v for v in fn)))
print("  cuts='auto' median %7.1f frames/s  spread %5.1f  (%s)" % (ma, max(fa) - min(fa), " ".join("%.1f" % v for v in fa)))
print("  auto - None = %+.1f frames/s (%+.2f %%); spread of the cuts=None runs %.1f -> %s" % (
    ma - mn, 100 * (ma - mn) / mn, sn,
    "ACCEPTED (inside the spread of the cuts=None runs)" if ma >= mn - sn else "OUTSIDE the spread: the overhead stands as measured"))
