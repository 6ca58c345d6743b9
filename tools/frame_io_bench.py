#!/usr/bin/env python3
"""The frame path (csrc/frame_io.hip, dynavsr_amd/frames.py) measured, in one process:

1. frame_ingest (uint8 HWC -> fp32 planar, 180x320 and 480x854 -> 480x856) and frame_emit (fp32 planar 720x1280 -> uint8
   HWC) by hipEvents around `--calls` back-to-back calls each, with the algorithmic bytes (bytes read + bytes written once)
   over that time.  At <= 14 MB a frame these kernels are launch-sized: the figure is a time, not a share of the HBM peak.
2. frames/s of a uint8 video in PINNED host memory -> uint8 SR frames on the host, EDVR-M x4, two ways alternated in one call,
   `--repeats` timed passes each after one warm-up pass:
     new       adapt.super_resolve_frames(uint8 frames): bytes to the device, extract_frame, fuse, emit, bytes back
     baseline  the float path wrapped in torch ops: .float() / 255 + permute on the device in front,
               clamp * 255 round to(uint8) permute behind
   Accepted if the new path's median is not below the baseline's median by more than the baseline's own max - min spread.

usage (GPU box): python tools/frame_io_bench.py [--h 180 --w 320 --frames 100 --repeats 5 --calls 200] > profiles/r08_frame_io.txt"""
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
from dynavsr_amd import adapt, frames, synth  # noqa: E402
from dynavsr_amd.models.archs.EDVR_arch import EDVR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--h", type=int, default=180)
ap.add_argument("--w", type=int, default=320)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--in-flight", type=int, default=2)
args = ap.parse_args()
H, W, T = args.h, args.w, args.frames
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
print("# frame path; %s; %d calls per kernel figure, %d repeats per video figure" % (torch.cuda.get_device_name(0), args.calls,
                                                                                     args.repeats))


def event_us(fn, n):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


r = np.random.RandomState(0)
for (h, w) in ((180, 320), (480, 854)):
    Hp, Wp = frames.padded_size(h, w, 4)
    src = torch.from_numpy(r.randint(0, 256, (h, w, 3)).astype(np.uint8)).cuda()
    dst = torch.empty((3, Hp, Wp), device='cuda')
    us = event_us(lambda: frames.ingest(src, 'hwc_bgr', 4, 'reflect', out=dst), args.calls)
    nbytes = h * w * 3 + 3 * Hp * Wp * 4
    print("frame_ingest uint8 BGR %dx%d -> fp32 [3,%d,%d]: %.2f us per call (host call + launch included), %.2f MB algorithmic "
          "-> %.1f GB/s; launch-sized, not a share of the HBM peak" % (h, w, Hp, Wp, us, nbytes / 1e6, nbytes / us / 1e3))
sr = torch.rand((3, 720, 1280), device='cuda')
img = torch.empty((720, 1280, 3), dtype=torch.uint8, device='cuda')
us = event_us(lambda: frames.emit(sr, 720, 1280, 'hwc_rgb', out=img), args.calls)
nbytes = 3 * 720 * 1280 * 5
print("frame_emit fp32 [3,720,1280] -> uint8 RGB 720x1280: %.2f us per call (host call + launch included), %.2f MB algorithmic "
      "-> %.1f GB/s; launch-sized, not a share of the HBM peak" % (us, nbytes / 1e6, nbytes / us / 1e3))
del sr, img

net = EDVR()
net.load_state_dict(synth.edvr_state_dict(0))
net = net.cuda()
base = (synth.clip(1, 1, 10, H, W, smooth=False)[0] * 255).round().to(torch.uint8).permute(0, 2, 3, 1)
video = torch.cat([base] * ((T + 9) // 10))[:T].contiguous().pin_memory()            # [T,H,W,3] uint8, pinned
host_out = torch.empty((T, 4 * H, 4 * W, 3), dtype=torch.uint8).pin_memory()


def new_path():
    for i, sr in enumerate(adapt.super_resolve_frames(OPT, net, video, in_flight=args.in_flight)):
        host_out[i].copy_(sr, non_blocking=True)
    torch.cuda.synchronize()


def float_frames():
    for i in range(T):
        yield (video[i].cuda(non_blocking=True).float() / 255).permute(2, 0, 1).contiguous()


def baseline():
    fl = list(float_frames())           # (super_resolve_frames indexes its frames: the conversions are enqueued up front)
    for i, sr in enumerate(adapt.super_resolve_frames(OPT, net, fl, in_flight=args.in_flight)):
        host_out[i].copy_((sr[0].clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0), non_blocking=True)
    torch.cuda.synchronize()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return T / (time.perf_counter() - t0)


new_path()
a = host_out.clone()
baseline()
print("uint8 results of the two paths differ in %d of %d bytes (max %d levels)" % (
    int((a != host_out).sum()), a.numel(), int((a.int() - host_out.int()).abs().max())))
del a
fn, fb = [], []
for _ in range(args.repeats):
    fn.append(timed(new_path))
    fb.append(timed(baseline))
mn, mb = statistics.median(fn), statistics.median(fb)
sn, sb = max(fn) - min(fn), max(fb) - min(fb)
print("video %d frames uint8 %dx%d pinned host -> uint8 %dx%d host, in_flight %d" % (T, H, W, 4 * H, 4 * W, args.in_flight))
print("  new      (uint8 in, extract_frame, emit, uint8 out)  median %7.1f frames/s  spread %5.1f  (%s)" % (
    mn, sn, " ".join("%.1f" % v for v in fn)))
print("  baseline (torch ops around the float path)           median %7.1f frames/s  spread %5.1f  (%s)" % (
    mb, sb, " ".join("%.1f" % v for v in fb)))
print("  new - baseline = %+.1f frames/s (%+.1f %%); baseline spread %.1f -> %s" % (
    mn - mb, 100 * (mn - mb) / mb, sb, "ACCEPTED (not below the baseline by more than its spread)" if mn >= mb - sb else "REJECTED"))
