#!/usr/bin/env python3
"""The flip-test x4 self-ensemble (csrc/frame_flip.hip, frames.flip / frames.flip_mean, super_resolve_frames(flip_test=True))
measured, in one process:

1. the kernels: dvsr_frame_flip (flags W | H) and dvsr_frame_flip_mean through the C ABI on 3 x 720 x 1280 fp32 -- the SR frame
   of a 180 x 320 video through a x4 network -- against the torch-op composition on the same device and the same values:
   torch.flip(x, (-2, -1)), and (((a + b.flip(-1)) + c.flip(-2)) + d.flip((-2, -1))) * 0.25 (three flips, three adds and a
   multiply: seven passes).  dvsr_frame_flip also at 3 x 180 x 320, the frame that is flipped in front of an extraction.  Each as
   `--calls` back-to-back launches captured into one graph whose replay is timed by hipEvents (device time per launch, without
   the host's call rate), `--repeats` repetitions alternated; consecutive launches read different source buffers.  GB/s against
   the algorithmic bytes (every source read once, the result written once) is recorded.  No bar is set.
2. end to end: a pinned 8-bit RGB video of 180 x 320 through EDVR-M x4 to 8-bit frames on the host, with and without flip_test,
   in frames/s: `--video-repeats` timed passes each after one warm-up pass, alternated.  Expectation: a frame with flip_test
   costs at most 4 x the per-frame time of the SAME build's flip_test=False run, plus one flip_mean at 720 x 1280 and three
   flips at 180 x 320 as measured in part 1; the margin is the max - min spread of the baseline's per-frame times.

usage (GPU box): python tools/flip_bench.py [--calls 40 --repeats 10 --frames 100 --video-repeats 5] > profiles/r14_flip_test.txt"""
import argparse
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
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--video-repeats", type=int, default=5)
ap.add_argument("--in-flight", type=int, default=2)
ap.add_argument("--skip-video", action="store_true")
args = ap.parse_args()
print("# flip-test path; %s; %d launches per replay, %d repetitions per kernel figure, %d per video figure" % (
    torch.cuda.get_device_name(0), args.calls, args.repeats, args.video_repeats))
lib = L.lib()
NBUF = 8


def graph_us(launch, n):
    """Device time per launch: `n` back-to-back launches (launch(i)) captured into one graph; returns a function that replays
    and times it."""
    for i in range(3):
        launch(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(n):
            launch(i)
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


def report(title, timers, nbytes):
    us = {name: [] for name, _ in timers}
    for _ in range(args.repeats):
        for name, t in timers:
            us[name].append(t())
    print(title)
    med = {}
    for name, _ in timers:
        m, sp = statistics.median(us[name]), max(us[name]) - min(us[name])
        med[name] = m
        print("  %-28s median %8.2f us per launch  spread %6.2f  -> %7.1f GB/s of algorithmic bytes" % (name, m, sp, nbytes / m / 1e3))
    return med


def flip_case(H, W):
    srcs = [torch.randn((3, H, W), device='cuda') for _ in range(NBUF)]
    dst = torch.empty((3, H, W), device='cuda')
    assert torch.equal(frames.flip(srcs[0], 3, out=dst), torch.flip(srcs[0], (-2, -1)))

    def ours(i):
        L.check(lib.dvsr_frame_flip(srcs[i % NBUF].data_ptr(), dst.data_ptr(), 3, H, W, 3, L.stream()), "dvsr_frame_flip")

    def theirs(i):
        torch.flip(srcs[i % NBUF], (-2, -1))
    nbytes = 2 * 12 * H * W
    return report("flip W | H of 3 x %d x %d fp32, %.2f MB algorithmic; bit-identical to torch.flip" % (H, W, nbytes / 1e6),
                  [("torch.flip", graph_us(theirs, args.calls)), ("dvsr_frame_flip", graph_us(ours, args.calls))], nbytes)


def mean_case(H, W):
    srcs = [torch.randn((3, H, W), device='cuda') for _ in range(NBUF)]
    dst = torch.empty((3, H, W), device='cuda')

    def compose(a, b, c, d):
        return (((a + b.flip(-1)) + c.flip(-2)) + d.flip((-2, -1))) * 0.25
    assert torch.equal(frames.flip_mean(*srcs[:4], out=dst), compose(*srcs[:4]))

    def ours(i):
        p = [srcs[(i + j) % NBUF].data_ptr() for j in range(4)]
        L.check(lib.dvsr_frame_flip_mean(p[0], p[1], p[2], p[3], dst.data_ptr(), 3, H, W, L.stream()), "dvsr_frame_flip_mean")

    def theirs(i):
        compose(*[srcs[(i + j) % NBUF] for j in range(4)])
    nbytes = 5 * 12 * H * W
    return report("flip_mean of four 3 x %d x %d fp32, %.2f MB algorithmic; bit-identical to the torch composition" % (
        H, W, nbytes / 1e6), [("torch: 3 flips, 3 adds, 1 mul", graph_us(theirs, args.calls)),
                              ("dvsr_frame_flip_mean", graph_us(ours, args.calls))], nbytes)


flip_big = flip_case(720, 1280)
flip_small = flip_case(180, 320)
mean_big = mean_case(720, 1280)
torch.cuda.empty_cache()
if args.skip_video:
    sys.exit(0)

# ---- 2. end to end
H, W, T = 180, 320, args.frames
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
net = EDVR()
net.load_state_dict(synth.edvr_state_dict(0))
net = net.cuda()
video = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (T, H, W, 3)).astype(np.uint8)).pin_memory()
out = torch.empty((T, 4 * H, 4 * W, 3), dtype=torch.uint8).pin_memory()


def go(flip_test):
    for i, y in enumerate(adapt.super_resolve_frames(OPT, net, video, in_flight=args.in_flight, flip_test=flip_test)):
        out[i].copy_(y, non_blocking=True)
    torch.cuda.synchronize()


def timed(flip_test):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    go(flip_test)
    return T / (time.perf_counter() - t0)


go(False)
go(True)
fp, ff = [], []
for _ in range(args.video_repeats):
    fp.append(timed(False))
    ff.append(timed(True))
mp, mf = statistics.median(fp), statistics.median(ff)
ms_plain = [1e3 / v for v in fp]
spread_ms = max(ms_plain) - min(ms_plain)
kernels_ms = (mean_big["dvsr_frame_flip_mean"] + 3 * flip_small["dvsr_frame_flip"]) / 1e3
bound_ms = 4 * 1e3 / mp + kernels_ms
print("video %d frames uint8 RGB %dx%d pinned host -> uint8 %dx%d on the host, EDVR-M x4, in_flight %d, %d repetitions alternated" % (
    T, H, W, 4 * H, 4 * W, args.in_flight, args.video_repeats))
print("  flip_test=False   median %7.2f frames/s  spread %5.2f  = %6.3f ms per frame, spread %.3f ms  (%s)" % (
    mp, max(fp) - min(fp), 1e3 / mp, spread_ms, " ".join("%.2f" % v for v in fp)))
print("  flip_test=True    median %7.2f frames/s  spread %5.2f  = %6.3f ms per frame  (%s)" % (
    mf, max(ff) - min(ff), 1e3 / mf, " ".join("%.2f" % v for v in ff)))
print("  expectation: 4 x %.3f + %.3f ms of flip kernels = %.3f ms per frame, margin %.3f ms (the baseline's spread); measured "
      "%.3f ms = %.2f x the baseline -> %s" % (1e3 / mp, kernels_ms, bound_ms, spread_ms, 1e3 / mf, mp / mf,
                                              "MET" if 1e3 / mf <= bound_ms + spread_ms else "MISSED"))
