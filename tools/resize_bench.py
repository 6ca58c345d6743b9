#!/usr/bin/env python3
"""SR frames at a target output size (csrc/frame_resize.hip, frames.resize, super_resolve_frames(out_size=)) measured, in one
process:

1. the kernel: dvsr_frame_resize through the C ABI at 1920x3416 (a crop of 1920x3424) -> 1080x1920 and at 720x1280 ->
   1080x1920, against torch.nn.functional.interpolate(x, size, mode='bicubic', antialias=True) on the same device and the same
   values (torch gets a contiguous tensor of the crop's size: its best case).  Each as `--calls` back-to-back launches captured
   into one graph whose replay is timed by hipEvents (device time per launch, without the host's call rate), `--repeats`
   repetitions alternated.  Consecutive launches read different source buffers (four of them: 315 MB at the larger size, more
   than the 256 MiB Infinity Cache), so the figure is not that of a cache-resident frame.  Bar: the kernel's median is not above
   torch's median by more than torch's own max - min spread.  GB/s against the algorithmic bytes (crop read once + result
   written once) is recorded; no bar is set for it.
2. end to end: a pinned NV12 video of 480x854 through EDVR-M x4 to NV12 frames of 1080x1920 on the host
   (super_resolve_frames(..., layout='nv12', out_size=(1080, 1920))) against the same call without out_size -- 1920x3416 frames
   to the host, what the parent commit can do -- in frames/s, `--video-repeats` timed passes each after one warm-up pass,
   alternated.  Bar: not below that baseline's median by more than the baseline's own max - min spread.

usage (GPU box): python tools/resize_bench.py [--calls 40 --repeats 10 --frames 30 --video-repeats 5] > profiles/r13_resize.txt"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dynavsr_amd  # noqa: E402
dynavsr_amd.configure_runtime()
from dynavsr_amd import _lib as L  # noqa: E402
from dynavsr_amd import adapt, frames, synth  # noqa: E402
from dynavsr_amd.models.archs.EDVR_arch import EDVR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--frames", type=int, default=30)
ap.add_argument("--video-repeats", type=int, default=5)
ap.add_argument("--in-flight", type=int, default=2)
ap.add_argument("--skip-video", action="store_true")
args = ap.parse_args()
print("# resize path; %s; %d launches per replay, %d repetitions per kernel figure, %d per video figure" % (
    torch.cuda.get_device_name(0), args.calls, args.repeats, args.video_repeats))
lib = L.lib()
NBUF = 4


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


def kernel_case(h, w, Hs, Ws, oh, ow):
    srcs = [torch.rand((3, Hs, Ws), device='cuda') for _ in range(NBUF)]
    crops = [s[:, :h, :w].contiguous()[None] for s in srcs]
    dst = frames.resize_buffer((oh, ow), 'cuda')
    Wb = int(dst.shape[2])
    got = frames.resize(srcs[0], h, w, (oh, ow), out=dst).clone()              # (also builds the tables)
    want = F.interpolate(crops[0], size=(oh, ow), mode='bicubic', antialias=True, align_corners=False)[0]
    rows, cols = frames._resize_axis(h, oh, dst.device), frames._resize_axis(w, ow, dst.device)

    def ours(i):
        L.check(lib.dvsr_frame_resize(srcs[i % NBUF].data_ptr(), Hs, Ws, h, w, dst.data_ptr(), oh, Wb, oh, ow, ctypes.byref(rows),
                                      ctypes.byref(cols), L.stream()), "dvsr_frame_resize")

    def theirs(i):
        F.interpolate(crops[i % NBUF], size=(oh, ow), mode='bicubic', antialias=True, align_corners=False)
    timers = [("torch interpolate antialias", graph_us(theirs, args.calls)), ("dvsr_frame_resize", graph_us(ours, args.calls))]
    us = {name: [] for name, _ in timers}
    for _ in range(args.repeats):
        for name, t in timers:
            us[name].append(t())
    nbytes = 12 * (h * w + oh * ow)
    print("resize %dx%d (of %dx%d) -> %dx%d, taps %d x %d, %.1f MB algorithmic; max |ours - torch| = %.2e" % (
        h, w, Hs, Ws, oh, ow, rows.taps, cols.taps, nbytes / 1e6, float((got - want).abs().max())))
    mb, sb = statistics.median(us[timers[0][0]]), max(us[timers[0][0]]) - min(us[timers[0][0]])
    for name, _ in timers:
        m, sp = statistics.median(us[name]), max(us[name]) - min(us[name])
        verdict = "yardstick" if name == timers[0][0] else "not slower than torch by more than its spread %.2f us: %s" % (
            sb, "MET" if m <= mb + sb else "MISSED")
        print("  %-28s median %8.2f us per launch  spread %6.2f  -> %7.1f GB/s of algorithmic bytes  (%s)" % (
            name, m, sp, nbytes / m / 1e3, verdict))


kernel_case(1920, 3416, 1920, 3424, 1080, 1920)
kernel_case(720, 1280, 720, 1280, 1080, 1920)
torch.cuda.empty_cache()
if args.skip_video:
    sys.exit(0)

# ---- 2. end to end
H, W, T = 480, 854, args.frames
OH, OW = 1080, 1920
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
net = EDVR()
net.load_state_dict(synth.edvr_state_dict(0))
net = net.cuda()
r = np.random.RandomState(0)
video = torch.from_numpy(r.randint(16, 236, (T, H * 3 // 2, W)).astype(np.uint8)).pin_memory()          # [T,H*3/2,W] uint8, pinned
out_sized = torch.empty((T, OH * 3 // 2, OW), dtype=torch.uint8).pin_memory()
out_full = torch.empty((T, 6 * H, 4 * W), dtype=torch.uint8).pin_memory()


def sized():
    for i, y in enumerate(adapt.super_resolve_frames(OPT, net, video, in_flight=args.in_flight, layout='nv12', out_size=(OH, OW))):
        out_sized[i].copy_(y, non_blocking=True)
    torch.cuda.synchronize()


def full():
    for i, y in enumerate(adapt.super_resolve_frames(OPT, net, video, in_flight=args.in_flight, layout='nv12')):
        out_full[i].copy_(y, non_blocking=True)
    torch.cuda.synchronize()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return T / (time.perf_counter() - t0)


sized()
full()
fs, ff = [], []
for _ in range(args.video_repeats):
    fs.append(timed(sized))
    ff.append(timed(full))
ms, mf = statistics.median(fs), statistics.median(ff)
sf = max(ff) - min(ff)
print("video %d frames NV12 %dx%d pinned host -> NV12 on the host, EDVR-M x4, in_flight %d, %d repetitions alternated" % (
    T, H, W, args.in_flight, args.video_repeats))
print("  out_size=(%d, %d)  (%.2f MB back per frame)   median %7.2f frames/s  spread %5.2f  (%s)" % (
    OH, OW, 1.5 * OH * OW / 1e6, ms, max(fs) - min(fs), " ".join("%.2f" % v for v in fs)))
print("  no out_size: %dx%d (%.2f MB back per frame)  median %7.2f frames/s  spread %5.2f  (%s)" % (
    4 * H, 4 * W, 24.0 * H * W / 1e6, mf, sf, " ".join("%.2f" % v for v in ff)))
print("  sized - full = %+.2f frames/s (%+.1f %%); baseline spread %.2f -> %s" % (
    ms - mf, 100 * (ms - mf) / mf, sf, "MET (not below the baseline by more than its spread)" if ms >= mf - sf else "MISSED"))
