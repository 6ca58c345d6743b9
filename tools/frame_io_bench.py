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

5. the chroma axis of that kernel pair (4:2:2 and 4:4:4), by the method of 3:
   a. with `--parent-lib PATH` (a libdynavsr_hip.so built from the commit before the axis): the four 4:2:0 kernels of part 3 / 4
      -- ingest 180x320 and emit 720x1280, NV12 and P010 -- of this build and of that library, alternated in this process.
      Expected: the difference of the medians inside the parent's own max - min spread.
   b. every new layout's ingest and emit against the 4:2:0 kernel of the same sample kind in this build (NV12 for bytes, P010
      for words), PER BYTE MOVED: per pixel, ingest reads 1.5 / 2 / 3 samples (4:2:0 / 4:2:2 / 4:4:4) and writes 12 B, emit the
      reverse.  Expectation, not a gate: us per MB not above the yardstick's by more than its spread.
   c. frames/s of a pinned p210 video -> p210 frames on the host against the same levels as a p010 video -> p010 frames.  A p210
      frame is 4 bytes per pixel against 3 both ways; what comes back dominates (16 x the pixels), so the expected cost is the
      copy time of a third more bytes, where the copy is not hidden behind the network.

6. 16-bit RGB and planar integer RGB / GBR (csrc/frame_rgb.hip), by the method of 3 with `--rgb-repeats` repetitions;
   the expectations are printed ahead of the figures:
   a. with `--parent-lib PATH`: dvsr_frame_ingest (uint8 HWC 180x320) and dvsr_frame_emit (uint8 HWC 720x1280), and the NV12 / P010
      ingest and emit kernels, of this build and of that library, alternated in this process.
   b. every new kernel against the uint8 HWC kernel of its direction in this build, PER BYTE MOVED (fp32 bytes + sample bytes).
   c. frames/s of a pinned hwc_rgb16 video of `--rgb-frames` frames -> hwc_rgb16 frames on the host against the same video as
      hwc_rgb; recorded as measured.

7. chroma siting and BT.2020 NCL (the SITE axis of csrc/frame_yuv.hip), by the method of 3 with `--rgb-repeats`
   repetitions; the expectations are printed ahead of the figures:
   a. with `--parent-lib PATH`: the left-sited ingest (180x320) and emit (720x1280) kernels of nv12, i420, p010, nv16 and i444 of
      this build and of that library, alternated in this process.
   b. every new ingest instantiation against the left kernel of the same layout in this build.
   c. every new emit instantiation against the left kernel of the same layout; topleft reads 1.5 x the fp32 rows: recorded.
   d. frames/s of a pinned p010 video of `--rgb-frames` frames -> p010 frames on the host with siting='topleft',
      matrix='bt2020nc' against the same call with the defaults.

usage (GPU box): python tools/frame_io_bench.py [--h 180 --w 320 --frames 100 --repeats 5 --calls 200 --yuv-repeats 10]
                 [--parent-lib PATH] > profiles/r16_chroma_io.txt   (profiles/r12_yuv16_io.txt: parts 1 to 4;
                 profiles/r10_yuv_io.txt: 1 to 3; profiles/r08_frame_io.txt: 1 and 2)
                 python tools/frame_io_bench.py --parts rgb --parent-lib PATH > profiles/r22_rgb_io.txt   (part 6 alone)
                 python tools/frame_io_bench.py --parts siting --parent-lib PATH > profiles/r23_yuv_siting.txt   (part 7 alone)"""
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
ap.add_argument("--parent-lib", default=None, help="parts 5a and 6a: a libdynavsr_hip.so built from the parent commit")
ap.add_argument("--parts", choices=("all", "rgb", "siting"), default="all", help="rgb: part 6 alone; siting: part 7 alone")
ap.add_argument("--rgb-repeats", type=int, default=11)
ap.add_argument("--rgb-frames", type=int, default=60)
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


def compare(title, entries, reps, per_byte=False, recorded=()):
    """entries: [(name, launch, algorithmic bytes)], the first one the yardstick; alternated `reps` times.  per_byte: the
    verdict is on us per MB moved, not on us per launch.  recorded: names whose ratio to the yardstick is printed, not judged."""
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
        elif name in recorded:
            verdict = "%.3f x %s, recorded" % (m / mb, base)
        elif per_byte:
            verdict = "%.3f us/MB against %.3f + spread %.3f of %s: %s" % (
                1e6 * m / nbytes, 1e6 * mb / nb, 1e6 * sb / nb, base, "MET" if m / nbytes <= (mb + sb) / nb else "MISSED")
        else:
            verdict = "not slower than %s by more than its spread %.2f us: %s" % (base, sb, "MET" if m <= mb + sb else "MISSED")
        print("  %-22s median %7.2f us per launch  spread %5.2f  %6.2f MB algorithmic -> %6.3f TB/s effective  (%s)" % (
            name, m, sp, nbytes / 1e6, nbytes / m / 1e6, verdict))


# ---- 6. 16-bit RGB and planar integer RGB / GBR (csrc/frame_rgb.hip; --parts rgb runs this part alone)
def part_rgb():
    reps, calls = args.rgb_repeats, args.calls
    print("6. 16-bit RGB and planar integer RGB / GBR frames (csrc/frame_rgb.hip, DESIGN 3.2w); %d launches per replay, %d repetitions "
          "alternated" % (calls, reps))
    print("Expectations, written before the run:")
    print("  1. existing kernels unchanged: dvsr_frame_ingest (uint8 HWC 180x320) and dvsr_frame_emit (uint8 HWC 720x1280) of this build "
          "against the parent commit's library in this process, and the NV12 / P010 ingest and emit kernels (frame_yuv.hip now takes "
          "its sample groups from frame_sample.h): each median inside the parent's own max - min spread of the parent's median.")
    print("  2. new kernels per byte moved (fp32 bytes + sample bytes) against the uint8 HWC kernel of the same direction in this build: "
          "no new kernel's us per MB above the yardstick's by more than the yardstick's spread -- they move wider, better-aligned "
          "groups and have no reason to be slower.")
    print("  3. end to end, a pinned hwc_rgb16 180x320 video of %d frames -> hwc_rgb16 720x1280 frames on the host against the same "
          "video as hwc_rgb: twice the bytes come back, so a deficit is expected; recorded as measured, no figure fixed." % args.rgb_frames)
    rs = np.random.RandomState(6)
    keep = []
    fin, fout = torch.empty((3, 180, 320), device='cuda'), torch.rand((3, 720, 1280), device='cuda')

    def frame_of(lay, h, w):
        if lay in ('hwc_rgb', 'hwc_bgr'):
            return torch.from_numpy(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).cuda()
        depth = frames.layout_depth(lay.rstrip('x'))
        shape = (3, h, w) if lay.startswith('chw') else (h, w, 4 if lay.endswith('x') else 3)
        return torch.from_numpy(rs.randint(0, 2 ** depth, shape).astype(np.uint8 if depth == 8 else np.uint16)).cuda()

    def rgb_launch(lb, lay, h, w, ingest):
        """(one launch of `lay`'s ingest or emit through library `lb`, its algorithmic bytes); 'hwc_rgb16x': four words a pixel."""
        name = lay.rstrip('x')
        buf = frame_of(lay, h, w)
        t, d = frames.describe(buf, name)
        keep.append((buf, t, d))
        nbytes = buf.numel() * buf.element_size() + 12 * h * w
        if ingest:
            return c_launch(lb.dvsr_frame_ingest, t.data_ptr(), ctypes.byref(d), fin.data_ptr(), h, w, L.FRAME_PAD_REFLECT), nbytes
        return c_launch(lb.dvsr_frame_emit, fout.data_ptr(), h, w, t.data_ptr(), ctypes.byref(d), ctypes.c_float(0.0),
                        ctypes.c_float(1.0)), nbytes

    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        for name in ("dvsr_frame_ingest", "dvsr_frame_emit", "dvsr_frame_ingest_yuv", "dvsr_frame_emit_yuv", "dvsr_frame_ingest_yuv16",
                     "dvsr_frame_emit_yuv16"):
            getattr(parent, name).argtypes, getattr(parent, name).restype = getattr(lib, name).argtypes, getattr(lib, name).restype
        print("6a. the existing kernels of this build against those of %s" % os.path.basename(args.parent_lib))
        for ingest, (h, w) in ((True, (180, 320)), (False, (720, 1280))):
            what = "%s hwc_rgb %dx%d" % ("ingest" if ingest else "emit", h, w)
            entries = [("%s %s" % (who, what),) + rgb_launch(lb, 'hwc_rgb', h, w, ingest) for who, lb in (("parent", parent), ("this build", lib))]
            compare(what, entries, reps)
        for lay in ('nv12', 'p010'):
            for ingest, (h, w), plane in ((True, (180, 320), fin), (False, (720, 1280), fout)):
                depth = frames.layout_depth(lay)
                buf = torch.from_numpy((rs.randint(0, 2 ** depth, (h * 3 // 2, w)) << (16 - depth if depth > 8 else 0)).astype(
                    np.uint8 if depth == 8 else np.uint16)).cuda()
                planes, d = frames.describe_yuv(frames.yuv_planes(buf, lay)[0], lay, h, w, copy=ingest)
                keep.append((buf, planes, d))
                suffix = "yuv16" if depth > 8 else "yuv"
                entries = []
                for who, lb in (("parent", parent), ("this build", lib)):
                    if ingest:
                        go = c_launch(getattr(lb, "dvsr_frame_ingest_" + suffix), ctypes.byref(d), plane.data_ptr(), h, w, L.FRAME_PAD_REFLECT)
                    else:
                        go = c_launch(getattr(lb, "dvsr_frame_emit_" + suffix), plane.data_ptr(), h, w, ctypes.byref(d), ctypes.c_float(0.0),
                                      ctypes.c_float(1.0))
                    entries.append(("%s %s %s" % (who, "ingest" if ingest else "emit", lay), go,
                                    buf.numel() * buf.element_size() + 12 * h * w))
                compare("%s %s %dx%d" % ("ingest" if ingest else "emit", lay, h, w), entries, reps)
    else:
        print("6a. NOT measured: no --parent-lib")
    print("6b. every new kernel against the uint8 HWC kernel of its direction in this build, per byte moved")
    for ingest, (h, w), lays in ((True, (180, 320), ('hwc_rgb', 'hwc_rgb16', 'hwc_rgb16x', 'chw_rgb8', 'chw_gbr10', 'chw_rgb16')),
                                 (False, (720, 1280), ('hwc_rgb', 'hwc_rgb16', 'chw_rgb8', 'chw_gbr10', 'chw_rgb16'))):
        entries = [("%s %s" % ("ingest" if ingest else "emit", lay),) + rgb_launch(lib, lay, h, w, ingest) for lay in lays]
        compare("%s %dx%d" % ("ingest" if ingest else "emit", h, w), entries, reps, per_byte=True)
    del keep[:]
    # 6c. end to end
    n, hh, ww = args.rgb_frames, 180, 320
    edvr = EDVR()
    edvr.load_state_dict(synth.edvr_state_dict(0))
    edvr = edvr.cuda()
    clip = synth.clip(1, 1, 10, hh, ww, smooth=False)[0].permute(0, 2, 3, 1)                          # [10,H,W,3] in [0,1]
    v8 = torch.cat([(clip * 255).round().to(torch.uint8)] * ((n + 9) // 10))[:n].contiguous().pin_memory()
    v16 = torch.from_numpy(np.concatenate([(clip.numpy() * 65535).round().astype(np.uint16)] * ((n + 9) // 10))[:n].copy()).pin_memory()
    o8 = torch.empty((n, 4 * hh, 4 * ww, 3), dtype=torch.uint8).pin_memory()
    o16 = torch.empty((n, 4 * hh, 4 * ww, 3), dtype=torch.uint16).pin_memory()

    def path(video, out, layout):
        def go():
            for i, sr in enumerate(adapt.super_resolve_frames(OPT, edvr, video, in_flight=args.in_flight, layout=layout)):
                out[i].copy_(sr, non_blocking=True)
            torch.cuda.synchronize()
        return go

    def fps(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return n / (time.perf_counter() - t0)
    p16, p8 = path(v16, o16, 'hwc_rgb16'), path(v8, o8, 'hwc_rgb')
    p16()
    p8()
    f16, f8 = [], []
    for _ in range(reps):
        f16.append(fps(p16))
        f8.append(fps(p8))
    m16, m8 = statistics.median(f16), statistics.median(f8)
    print("6c. video %d frames %dx%d pinned host -> %dx%d host, in_flight %d, %d repetitions alternated" % (
        n, hh, ww, 4 * hh, 4 * ww, args.in_flight, reps))
    print("  hwc_rgb16 in, hwc_rgb16 out (%.2f MB in, %.2f MB back per frame)  median %7.1f frames/s  spread %5.1f  (%s)" % (
        6 * hh * ww / 1e6, 96 * hh * ww / 1e6, m16, max(f16) - min(f16), " ".join("%.1f" % v for v in f16)))
    print("  hwc_rgb in, hwc_rgb out     (%.2f MB in, %.2f MB back per frame)  median %7.1f frames/s  spread %5.1f  (%s)" % (
        3 * hh * ww / 1e6, 48 * hh * ww / 1e6, m8, max(f8) - min(f8), " ".join("%.1f" % v for v in f8)))
    print("  hwc_rgb16 - hwc_rgb = %+.1f frames/s (%+.1f %%), as measured; twice the bytes travel both ways" % (
        m16 - m8, 100 * (m16 - m8) / m8))


# ---- 7. chroma siting and BT.2020 NCL (the SITE axis of csrc/frame_yuv.hip; --parts siting runs this part alone)
def part_siting():
    reps, calls = args.rgb_repeats, args.calls
    print("7. chroma siting and BT.2020 NCL (the SITE axis of csrc/frame_yuv.hip, DESIGN 3.2x); %d launches per replay, %d repetitions "
          "alternated" % (calls, reps))
    print("Expectations, written before the run:")
    print("  1. the existing left kernels are not slower than the parent's beyond the parent's own spread: ingest 180x320 and emit "
          "720x1280 for nv12, i420, p010, nv16 and i444.  A miss means the new axis leaked into the old instantiations, by "
          "registers or occupancy.")
    print("  2. each new ingest instantiation is not slower than the left kernel of the same layout and build beyond that kernel's "
          "spread: center reads one more chroma sample per row, topleft one chroma row fewer.")
    print("  3. center emit is not slower than left emit (no left-neighbour loads); topleft emit reads 1.5 x the fp32 rows, and its "
          "ratio to left is recorded, not bounded.")
    print("  Also recorded: frames/s of a pinned p010 180x320 video -> p010 720x1280 frames on the host with siting='topleft', "
          "matrix='bt2020nc' against the same call with the defaults.")
    rs = np.random.RandomState(7)
    keep = []
    fin, fout = torch.empty((3, 180, 320), device='cuda'), torch.rand((3, 720, 1280), device='cuda')

    def yuv_launch(lb, lay, siting, ingest):
        """(one launch of `lay`'s ingest 180x320 or emit 720x1280 with `siting` through library `lb`, its algorithmic bytes)"""
        h, w = (180, 320) if ingest else (720, 1280)
        depth = frames.layout_depth(lay)
        msb = 16 - depth if lay.startswith('p') else 0
        buf = torch.from_numpy((rs.randint(0, 2 ** depth, (frames.packed_rows(lay, h), w)) << msb).astype(
            np.uint8 if depth == 8 else np.uint16)).cuda()
        planes, d = frames.describe_yuv(frames.yuv_planes(buf, lay)[0], lay, h, w, copy=ingest, siting=siting)
        keep.append((buf, planes, d))
        suffix = "yuv16" if depth > 8 else "yuv"
        nbytes = buf.numel() * buf.element_size() + 12 * h * w
        if ingest:
            return c_launch(getattr(lb, "dvsr_frame_ingest_" + suffix), ctypes.byref(d), fin.data_ptr(), h, w, L.FRAME_PAD_REFLECT), nbytes
        return c_launch(getattr(lb, "dvsr_frame_emit_" + suffix), fout.data_ptr(), h, w, ctypes.byref(d), ctypes.c_float(0.0),
                        ctypes.c_float(1.0)), nbytes

    def title(ingest, lay):
        return "%s %s %s" % ("ingest" if ingest else "emit", lay, "180x320" if ingest else "720x1280")

    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        for name in ("dvsr_frame_ingest_yuv", "dvsr_frame_emit_yuv", "dvsr_frame_ingest_yuv16", "dvsr_frame_emit_yuv16"):
            getattr(parent, name).argtypes, getattr(parent, name).restype = getattr(lib, name).argtypes, getattr(lib, name).restype
        print("7a. the left kernels of this build against those of %s" % os.path.basename(args.parent_lib))
        for lay in ('nv12', 'i420', 'p010', 'nv16', 'i444'):
            for ingest in (True, False):
                compare(title(ingest, lay), [("%s %s" % (who, title(ingest, lay)),) + yuv_launch(lb, lay, 'left', ingest)
                                             for who, lb in (("parent", parent), ("this build", lib))], reps)
    else:
        print("7a. NOT measured: no --parent-lib")
    sited = [(lay, ('left', 'center', 'topleft')) for lay in ('nv12', 'i420', 'p010', 'i420p10')] + \
            [(lay, ('left', 'center')) for lay in ('nv16', 'i422', 'p210', 'i422p10')]
    for ingest, part in ((True, "7b. every new ingest instantiation against the left kernel of its layout in this build"),
                         (False, "7c. every new emit instantiation against the left kernel of its layout in this build")):
        print(part)
        for lay, sitings in sited:
            compare(title(ingest, lay), [("%s %s" % (title(ingest, lay), s),) + yuv_launch(lib, lay, s, ingest) for s in sitings], reps,
                    recorded=() if ingest else ("%s topleft" % title(ingest, lay),))
    del keep[:]
    # 7d. end to end
    n, hh, ww = args.rgb_frames, 180, 320
    edvr = EDVR()
    edvr.load_state_dict(synth.edvr_state_dict(0))
    edvr = edvr.cuda()
    video = torch.from_numpy((rs.randint(0, 1024, (n, hh * 3 // 2, ww)) << 6).astype(np.uint16)).pin_memory()
    out = torch.empty((n, 4 * hh * 3 // 2, 4 * ww), dtype=torch.uint16).pin_memory()

    def path(**kw):
        def go():
            for i, sr in enumerate(adapt.super_resolve_frames(OPT, edvr, video, in_flight=args.in_flight, layout='p010', **kw)):
                out[i].copy_(sr, non_blocking=True)
            torch.cuda.synchronize()
        return go

    def fps(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return n / (time.perf_counter() - t0)
    new, old = path(siting='topleft', matrix='bt2020nc'), path()
    new()
    old()
    fn, fo = [], []
    for _ in range(reps):
        fn.append(fps(new))
        fo.append(fps(old))
    mn, mo = statistics.median(fn), statistics.median(fo)
    print("7d. p010 video %d frames %dx%d pinned host -> p010 %dx%d host, in_flight %d, %d repetitions alternated" % (
        n, hh, ww, 4 * hh, 4 * ww, args.in_flight, reps))
    print("  siting='topleft', matrix='bt2020nc'  median %7.1f frames/s  spread %5.1f  (%s)" % (
        mn, max(fn) - min(fn), " ".join("%.1f" % v for v in fn)))
    print("  the defaults (left, bt601)           median %7.1f frames/s  spread %5.1f  (%s)" % (
        mo, max(fo) - min(fo), " ".join("%.1f" % v for v in fo)))
    print("  topleft bt2020nc - defaults = %+.1f frames/s (%+.1f %%), as measured" % (mn - mo, 100 * (mn - mo) / mo))


if args.parts == 'rgb':
    part_rgb()
    sys.exit(0)
if args.parts == 'siting':
    part_siting()
    sys.exit(0)

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


# ---- 5. the chroma axis: 4:2:2 and 4:4:4 next to 4:2:0
def yuv_launches(lb, lay, h, w, buf, plane, ingest):
    """One launch of `lay`'s ingest (packed frame `buf` -> `plane`) or emit (`plane` -> `buf`) through library `lb`."""
    planes, d = frames.describe_yuv(frames.yuv_planes(buf, lay)[0], lay, h, w, copy=ingest)
    keep.append((planes, d))
    suffix = "yuv16" if frames.layout_depth(lay) > 8 else "yuv"
    if ingest:
        return c_launch(getattr(lb, "dvsr_frame_ingest_" + suffix), ctypes.byref(d), plane.data_ptr(), h, w, L.FRAME_PAD_REFLECT)
    return c_launch(getattr(lb, "dvsr_frame_emit_" + suffix), plane.data_ptr(), h, w, ctypes.byref(d), ctypes.c_float(0.0),
                    ctypes.c_float(1.0))


def packed_frame(lay, h, w):
    """A packed frame of random levels in `lay` on the device."""
    depth, rows = frames.layout_depth(lay), frames.packed_rows(lay, h)
    if depth == 8:
        return torch.from_numpy(r.randint(0, 256, (rows, w)).astype(np.uint8)).cuda()
    shift = 16 - depth if lay.startswith('p') else 0
    return torch.from_numpy((r.randint(0, 2 ** depth, (rows, w)) << shift).astype(np.uint16)).cuda()


def frame_bytes(lay, h, w):
    """The algorithmic bytes of one ingest or emit: the packed frame once and the fp32 planes once."""
    return frames.packed_rows(lay, h) * w * (1 if frames.layout_depth(lay) == 8 else 2) + 12 * h * w


keep = []
planes_in, planes_out = torch.empty((3, 180, 320), device='cuda'), torch.rand((3, 720, 1280), device='cuda')
if args.parent_lib:
    parent = ctypes.CDLL(args.parent_lib)
    for name in ("dvsr_frame_ingest_yuv", "dvsr_frame_emit_yuv", "dvsr_frame_ingest_yuv16", "dvsr_frame_emit_yuv16"):
        getattr(parent, name).argtypes, getattr(parent, name).restype = getattr(lib, name).argtypes, getattr(lib, name).restype
    print("5a. the 4:2:0 kernels of this build against those of %s (the yardstick of every pair)" % os.path.basename(args.parent_lib))
    for lay in ('nv12', 'p010'):
        for ingest, (h, w), plane in ((True, (180, 320), planes_in), (False, (720, 1280), planes_out)):
            buf = packed_frame(lay, h, w)
            what = "%s %s %dx%d" % ("ingest" if ingest else "emit", lay, h, w)
            compare("%s, %d launches per replay, %d repetitions alternated" % (what, args.calls, args.yuv_repeats),
                    [("parent " + what, yuv_launches(parent, lay, h, w, buf, plane, ingest), frame_bytes(lay, h, w)),
                     ("this build " + what, yuv_launches(lib, lay, h, w, buf, plane, ingest), frame_bytes(lay, h, w))],
                    args.yuv_repeats)
else:
    print("5a. NOT measured: no --parent-lib")
print("5b. every new layout against the 4:2:0 kernel of its sample kind, per byte moved")
for group in (('nv12', 'nv16', 'i422', 'i444'), ('p010', 'p210', 'i422p10', 'i444p10')):
    for ingest, (h, w), plane in ((True, (180, 320), planes_in), (False, (720, 1280), planes_out)):
        entries = [("%s %s" % ("ingest" if ingest else "emit", lay),
                    yuv_launches(lib, lay, h, w, packed_frame(lay, h, w), plane, ingest), frame_bytes(lay, h, w)) for lay in group]
        compare("%s %dx%d, %d launches per replay, %d repetitions alternated" % ("ingest" if ingest else "emit", h, w, args.calls,
                                                                                args.yuv_repeats), entries, args.yuv_repeats, per_byte=True)
del keep, planes_in, planes_out

levels = r.randint(64, 941, (T, 2 * H, W))                                   # Y | CbCr rows of a 4:2:2 frame; 4:2:0 takes 3/4 of them
p210_video = torch.from_numpy((levels << 6).astype(np.uint16)).pin_memory()                          # [T,2H,W] pinned
p010_video = torch.from_numpy((levels[:, :H * 3 // 2] << 6).astype(np.uint16)).pin_memory()          # [T,H*3/2,W] pinned
p210_out = torch.empty((T, 8 * H, 4 * W), dtype=torch.uint16).pin_memory()


def p2x0_path(video, layout, out):
    def go():
        for i, y in enumerate(adapt.super_resolve_frames(OPT, net, video, in_flight=args.in_flight, layout=layout)):
            out[i].copy_(y, non_blocking=True)
        torch.cuda.synchronize()
    return go


p210_path, p010_path = p2x0_path(p210_video, 'p210', p210_out), p2x0_path(p010_video, 'p010', p010_out)
p210_path()
p010_path()
f2, f0 = [], []
for _ in range(args.yuv_repeats):
    f2.append(timed(p210_path))
    f0.append(timed(p010_path))
m2, m0 = statistics.median(f2), statistics.median(f0)
s0 = max(f0) - min(f0)
print("5c. video %d frames %dx%d pinned host -> %dx%d host, in_flight %d, %d repetitions alternated" % (
    T, H, W, 4 * H, 4 * W, args.in_flight, args.yuv_repeats))
print("  p210 in, p210 out (%.2f MB in, %.2f MB back per frame)   median %7.1f frames/s  spread %5.1f  (%s)" % (
    4 * H * W / 1e6, 16 * H * 4 * W / 1e6, m2, max(f2) - min(f2), " ".join("%.1f" % v for v in f2)))
print("  p010 in, p010 out (%.2f MB in, %.2f MB back per frame)   median %7.1f frames/s  spread %5.1f  (%s)" % (
    3 * H * W / 1e6, 12 * H * 4 * W / 1e6, m0, s0, " ".join("%.1f" % v for v in f0)))
print("  p210 - p010 = %+.1f frames/s (%+.1f %%); p010 spread %.1f; 4 bytes per pixel against 3 travel both ways -> %s" % (
    m2 - m0, 100 * (m2 - m0) / m0, s0, "inside the p010 spread" if m2 >= m0 - s0 else "below the p010 path by more than its spread"))

part_rgb()
