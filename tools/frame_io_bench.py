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
3. the YCbCr 4:2:0 pair (csrc/frame_yuv.hip) next to the unchanged 8-bit HWC kernels, on the same frames in this process:
   frame_ingest_yuv (NV12, I420; 180x320) and frame_emit_yuv (720x1280) against frame_ingest / frame_emit, each as `--calls`
   back-to-back launches through the C ABI captured into one graph, whose replay is timed by hipEvents (device time per launch,
   without the host's call rate), `--yuv-repeats` repetitions alternated; effective bytes/s from the algorithmic bytes (ingest
   1.5 B read + 12 B written per padded pixel, emit 12 B read + 1.5 B written; HWC: 3 B).  Then frames/s of a pinned NV12
   video -> NV12 frames on the host against the same video through the HWC path of 2.  The HWC path of the same build is the
   yardstick, not code under test: a YUV figure is expected not to be slower than its HWC counterpart by more than that
   counterpart's own max - min spread.

4. the 10- / 12-bit pair (csrc/frame_yuv.hip too) next to the 8-bit 4:2:0 kernels of 3, by the method of 3: frame_ingest_yuv16
   (P010, yuv420p10le; 180x320) and frame_emit_yuv16 (720x1280) against frame_ingest_yuv / frame_emit_yuv NV12.  A 16-bit
   frame is twice the bytes on its side (ingest 3 B read + 12 B written per pixel, emit 12 B read + 3 B written, against
   13.5), so the comparison is PER BYTE MOVED: a 16-bit kernel's us per MB is expected not to exceed the 8-bit yardstick's by
   more than that yardstick's own max - min spread.  Then frames/s of a pinned P010 video -> P010 frames on the host against
   the same video through the HWC uint8 path of 2, which moves the same 3 bytes per output pixel back to the host.

usage (GPU box): python tools/frame_io_bench.py [--h 180 --w 320 --frames 100 --repeats 5 --calls 200 --yuv-repeats 10]
                 > profiles/r12_yuv16_io.txt   (profiles/r10_yuv_io.txt: parts 1 to 3; profiles/r08_frame_io.txt: 1 and 2)"""
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
from dynavsr_amd import adapt, frames, synth  # noqa: E402
from dynavsr_amd.models.archs.EDVR_arch import EDVR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--h", type=int, default=180)
ap.add_argument("--w", type=int, default=320)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--in-flight", type=int, default=2)
ap.add_argument("--yuv-repeats", type=int, default=10)
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


# ---- 3. the YCbCr 4:2:0 pair next to the HWC kernels
from dynavsr_amd import _lib as L  # noqa: E402

lib = L.lib()


def graph_us(launch, n):
    """Device time per launch: `n` back-to-back launches captured into one graph; returns a function that replays and times it."""
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


def c_launch(fn, *a):
    def go():
        L.check(fn(*a, L.stream()), fn.__name__)
    return go


def compare(title, entries, reps, per_byte=False):
    """entries: [(name, launch, algorithmic bytes)], the first one the yardstick; alternated `reps` times.  per_byte: the
    verdict is on us per MB moved, not on us per launch."""
    timers = [(name, graph_us(launch, args.calls), nbytes) for name, launch, nbytes in entries]
    us = {name: [] for name, _, _ in timers}
    for _ in range(reps):
        for name, t, _ in timers:
            us[name].append(t())
    print(title)
    base = timers[0][0]
    mb, sb = statistics.median(us[base]), max(us[base]) - min(us[base])
    nb = timers[0][2]
    for name, _, nbytes in timers:
        m, sp = statistics.median(us[name]), max(us[name]) - min(us[name])
        if name == base:
            verdict = "yardstick"
        elif per_byte:
            verdict = "%.3f us/MB against %.3f + spread %.3f of %s: %s" % (
                1e6 * m / nbytes, 1e6 * mb / nb, 1e6 * sb / nb, base, "MET" if m / nbytes <= (mb + sb) / nb else "MISSED")
        else:
            verdict = "not slower than %s by more than its spread %.2f us: %s" % (base, sb, "MET" if m <= mb + sb else "MISSED")
        print("  %-22s median %7.2f us per launch  spread %5.2f  %6.2f MB algorithmic -> %6.3f TB/s effective  (%s)" % (
            name, m, sp, nbytes / 1e6, nbytes / m / 1e6, verdict))


h, w = 180, 320
rgb = torch.from_numpy(r.randint(0, 256, (h, w, 3)).astype(np.uint8)).cuda()
packed = torch.from_numpy(r.randint(0, 256, (h * 3 // 2, w)).astype(np.uint8)).cuda()
dst = torch.empty((3, h, w), device='cuda')
_, d_rgb = frames.describe(rgb, 'hwc_rgb')
entries = [("frame_ingest HWC RGB", c_launch(lib.dvsr_frame_ingest, rgb.data_ptr(), ctypes.byref(d_rgb), dst.data_ptr(), h, w,
                                               L.FRAME_PAD_REFLECT), 15 * h * w)]
keep = []
for lay in ('nv12', 'i420'):
    planes, d = frames.describe_yuv(frames.yuv_planes(packed, lay)[0], lay, h, w)
    keep.append((planes, d))
    entries.append(("frame_ingest_yuv " + lay.upper(), c_launch(lib.dvsr_frame_ingest_yuv, ctypes.byref(d), dst.data_ptr(), h, w,
                                                                  L.FRAME_PAD_REFLECT), int(13.5 * h * w)))
compare("ingest %dx%d -> fp32 [3,%d,%d], %d launches per replay, %d repetitions alternated" % (h, w, h, w, args.calls,
                                                                                               args.yuv_repeats), entries, args.yuv_repeats)
h, w = 720, 1280
sr = torch.rand((3, h, w), device='cuda')
img = torch.empty((h, w, 3), dtype=torch.uint8, device='cuda')
out = torch.empty((h * 3 // 2, w), dtype=torch.uint8, device='cuda')
_, d_img = frames.describe(img, 'hwc_rgb')
entries = [("frame_emit HWC RGB", c_launch(lib.dvsr_frame_emit, sr.data_ptr(), h, w, img.data_ptr(), ctypes.byref(d_img),
                                             ctypes.c_float(0.0), ctypes.c_float(1.0)), 15 * h * w)]
for lay in ('nv12', 'i420'):
    planes, d = frames.describe_yuv(frames.yuv_planes(out, lay)[0], lay, h, w, copy=False)
    keep.append((planes, d))
    entries.append(("frame_emit_yuv " + lay.upper(), c_launch(lib.dvsr_frame_emit_yuv, sr.data_ptr(), h, w, ctypes.byref(d),
                                                                ctypes.c_float(0.0), ctypes.c_float(1.0)), int(13.5 * h * w)))
compare("emit fp32 [3,%d,%d] -> %dx%d, %d launches per replay, %d repetitions alternated" % (h, w, h, w, args.calls,
                                                                                             args.yuv_repeats), entries, args.yuv_repeats)
del sr, img, out, keep

if H % 2 or W % 2:
    sys.exit("the NV12 video needs an even --h and --w")
yuv_video = torch.from_numpy(r.randint(16, 236, (T, H * 3 // 2, W)).astype(np.uint8)).pin_memory()     # [T,H*3/2,W] uint8, pinned
yuv_out = torch.empty((T, 6 * H, 4 * W), dtype=torch.uint8).pin_memory()


def yuv_path():
    for i, y in enumerate(adapt.super_resolve_frames(OPT, net, yuv_video, in_flight=args.in_flight, layout='nv12')):
        yuv_out[i].copy_(y, non_blocking=True)
    torch.cuda.synchronize()


yuv_path()
new_path()
fy, fh = [], []
for _ in range(args.yuv_repeats):
    fy.append(timed(yuv_path))
    fh.append(timed(new_path))
my, mh = statistics.median(fy), statistics.median(fh)
sh = max(fh) - min(fh)
print("video %d frames %dx%d pinned host -> %dx%d host, in_flight %d, %d repetitions alternated" % (T, H, W, 4 * H, 4 * W,
                                                                                                   args.in_flight, args.yuv_repeats))
print("  NV12 in, NV12 out (%.2f MB back per frame)   median %7.1f frames/s  spread %5.1f  (%s)" % (
    6 * H * 4 * W / 1e6, my, max(fy) - min(fy), " ".join("%.1f" % v for v in fy)))
print("  HWC RGB in, HWC RGB out (%.2f MB back)        median %7.1f frames/s  spread %5.1f  (%s)" % (
    12 * H * 4 * W / 1e6, mh, sh, " ".join("%.1f" % v for v in fh)))
print("  NV12 - HWC = %+.1f frames/s (%+.1f %%); HWC spread %.1f -> expectation %s" % (
    my - mh, 100 * (my - mh) / mh, sh, "MET (not below the HWC path by more than its spread)" if my >= mh - sh else "MISSED"))


# ---- 4. the 10- / 12-bit pair next to the 8-bit 4:2:0 kernels
h, w = 180, 320
packed = torch.from_numpy(r.randint(0, 256, (h * 3 // 2, w)).astype(np.uint8)).cuda()
packed16 = torch.from_numpy((r.randint(0, 1024, (h * 3 // 2, w)) << 6).astype(np.uint16)).cuda()
planar16 = torch.from_numpy(r.randint(0, 1024, (h * 3 // 2, w)).astype(np.uint16)).cuda()
dst = torch.empty((3, h, w), device='cuda')
keep = []
planes, d = frames.describe_yuv(frames.yuv_planes(packed, 'nv12')[0], 'nv12', h, w)
keep.append((planes, d))
entries = [("frame_ingest_yuv NV12", c_launch(lib.dvsr_frame_ingest_yuv, ctypes.byref(d), dst.data_ptr(), h, w,
                                                L.FRAME_PAD_REFLECT), int(13.5 * h * w))]
for lay, src in (('p010', packed16), ('i420p10', planar16)):
    planes, d = frames.describe_yuv(frames.yuv_planes(src, lay)[0], lay, h, w)
    keep.append((planes, d))
    entries.append(("frame_ingest_yuv16 " + lay, c_launch(lib.dvsr_frame_ingest_yuv16, ctypes.byref(d), dst.data_ptr(), h, w,
                                                            L.FRAME_PAD_REFLECT), 15 * h * w))
compare("16-bit ingest %dx%d -> fp32 [3,%d,%d], %d launches per replay, %d repetitions alternated" % (
    h, w, h, w, args.calls, args.yuv_repeats), entries, args.yuv_repeats, per_byte=True)
h, w = 720, 1280
sr = torch.rand((3, h, w), device='cuda')
out = torch.empty((h * 3 // 2, w), dtype=torch.uint8, device='cuda')
out16 = torch.empty((h * 3 // 2, w), dtype=torch.uint16, device='cuda')
planes, d = frames.describe_yuv(frames.yuv_planes(out, 'nv12')[0], 'nv12', h, w, copy=False)
keep.append((planes, d))
entries = [("frame_emit_yuv NV12", c_launch(lib.dvsr_frame_emit_yuv, sr.data_ptr(), h, w, ctypes.byref(d), ctypes.c_float(0.0),
                                              ctypes.c_float(1.0)), int(13.5 * h * w))]
for lay in ('p010', 'i420p10'):
    planes, d = frames.describe_yuv(frames.yuv_planes(out16, lay)[0], lay, h, w, copy=False)
    keep.append((planes, d))
    entries.append(("frame_emit_yuv16 " + lay, c_launch(lib.dvsr_frame_emit_yuv16, sr.data_ptr(), h, w, ctypes.byref(d),
                                                          ctypes.c_float(0.0), ctypes.c_float(1.0)), 15 * h * w))
compare("16-bit emit fp32 [3,%d,%d] -> %dx%d, %d launches per replay, %d repetitions alternated" % (
    h, w, h, w, args.calls, args.yuv_repeats), entries, args.yuv_repeats, per_byte=True)
del sr, out, out16, keep

p010_video = torch.from_numpy((r.randint(64, 941, (T, H * 3 // 2, W)) << 6).astype(np.uint16)).pin_memory()   # [T,H*3/2,W] pinned
p010_out = torch.empty((T, 6 * H, 4 * W), dtype=torch.uint16).pin_memory()


def p010_path():
    for i, y in enumerate(adapt.super_resolve_frames(OPT, net, p010_video, in_flight=args.in_flight, layout='p010')):
        p010_out[i].copy_(y, non_blocking=True)
    torch.cuda.synchronize()


p010_path()
new_path()
fp, fh = [], []
for _ in range(args.yuv_repeats):
    fp.append(timed(p010_path))
    fh.append(timed(new_path))
mp, mh = statistics.median(fp), statistics.median(fh)
sh = max(fh) - min(fh)
print("video %d frames %dx%d pinned host -> %dx%d host, in_flight %d, %d repetitions alternated" % (T, H, W, 4 * H, 4 * W,
                                                                                                   args.in_flight, args.yuv_repeats))
print("  P010 in, P010 out (%.2f MB back per frame)   median %7.1f frames/s  spread %5.1f  (%s)" % (
    12 * H * 4 * W / 1e6, mp, max(fp) - min(fp), " ".join("%.1f" % v for v in fp)))
print("  HWC RGB in, HWC RGB out (%.2f MB back)        median %7.1f frames/s  spread %5.1f  (%s)" % (
    12 * H * 4 * W / 1e6, mh, sh, " ".join("%.1f" % v for v in fh)))
print("  P010 - HWC = %+.1f frames/s (%+.1f %%); HWC spread %.1f -> expectation %s" % (
    mp - mh, 100 * (mp - mh) / mh, sh, "MET (not below the HWC path by more than its spread)" if mp >= mh - sh else "MISSED"))
