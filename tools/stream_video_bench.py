#!/usr/bin/env python3
"""A video through EDVR-M x4 two ways, in one process: per-clip windows through adapt.super_resolve_video (every window
runs the whole tape) and adapt.super_resolve_frames (every frame's features extracted once, one gather + the tape from PCD
alignment on per window).  Same windows (index_generation, padding new_info), same network.

usage (GPU box): python tools/stream_video_bench.py [--h 180 --w 320 --frames 100 --repeats 5] > profiles/r07_stream_video.txt
                 rocprofv3 --kernel-trace --stats -d DIR -o r -- python tools/stream_video_bench.py --trace stream|clip
The two are alternated, `repeats` timed passes each after one warm-up pass, host clock around a device synchronise; reported:
median frames/s and the spread (max - min) of each, per in_flight.  --trace: a few untimed passes of one path for a kernel
trace (tools/rocprof_summary.py turns the database into the per-kernel table)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dynavsr_amd  # noqa: E402
dynavsr_amd.configure_runtime()
from dynavsr_amd import adapt, engine, synth  # noqa: E402
from dynavsr_amd.data.util import index_generation  # noqa: E402
from dynavsr_amd.models.archs.EDVR_arch import EDVR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--h", type=int, default=180)
ap.add_argument("--w", type=int, default=320)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--trace", choices=("stream", "clip"), default=None)
args = ap.parse_args()
H, W, T, MODE = args.h, args.w, args.frames, 'new_info'
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}

net = EDVR()
net.load_state_dict(synth.edvr_state_dict(0))
net = net.cuda()
# (a short clip repeated: the timing does not depend on the pixels, and 100 distinct synthetic frames take minutes to draw)
base = synth.clip(1, 1, 10, H, W, smooth=False)[0]
video = torch.cat([base] * ((T + 9) // 10))[:T].cuda().contiguous()


def clips():
    for i in range(T):
        yield video[index_generation(i, T, 5, MODE)][None]


def per_clip(in_flight, keep=()):
    out = {}
    for i, sr in enumerate(adapt.super_resolve_video(OPT, net, clips(), in_flight=in_flight)):
        if i in keep:
            out[i] = sr.clone()
    torch.cuda.synchronize()
    return out


def streaming(in_flight, keep=()):
    out = {}
    for i, sr in enumerate(adapt.super_resolve_frames(OPT, net, video, padding=MODE, in_flight=in_flight)):
        if i in keep:
            out[i] = sr.clone()
    torch.cuda.synchronize()
    return out


def timed(fn, in_flight):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(in_flight)
    return T / (time.perf_counter() - t0)


if args.trace:
    T = min(T, 20)
    video = video[:T].contiguous()
    for _ in range(3):
        (streaming if args.trace == "stream" else per_clip)(1)
    sys.exit(0)

print("# EDVR-M x4, %d frames %dx%d, padding %s, windows of 5; %s" % (T, H, W, MODE, torch.cuda.get_device_name(0)))
keep = (0, T // 2, T - 1)
a, b = per_clip(2, keep), streaming(2, keep)
for i in keep:
    d = (a[i] - b[i]).double()
    print("frame %3d: streaming vs per-clip rel-L2 %.3e, max-abs %.3e" % (i, float(d.norm() / a[i].double().norm()), float(d.abs().max())))
del a, b

for in_flight in (1, 2):
    per_clip(in_flight); streaming(in_flight)                  # warm-up: plans, workspaces, packs, allocator pools
    fa, fb = [], []
    for _ in range(args.repeats):
        fa.append(timed(per_clip, in_flight))
        fb.append(timed(streaming, in_flight))
    ma, mb = statistics.median(fa), statistics.median(fb)
    sa, sb = max(fa) - min(fa), max(fb) - min(fb)
    print("in_flight %d: per-clip  super_resolve_video   median %7.1f frames/s  spread %5.1f  (%s)" % (in_flight, ma, sa, " ".join("%.1f" % v for v in fa)))
    print("in_flight %d: streaming super_resolve_frames  median %7.1f frames/s  spread %5.1f  (%s)" % (in_flight, mb, sb, " ".join("%.1f" % v for v in fb)))
    print("in_flight %d: streaming - per-clip = %+.1f frames/s (%+.1f %%), larger spread %.1f -> %s" % (
        in_flight, mb - ma, 100 * (mb - ma) / ma, max(sa, sb), "ABOVE the spread" if mb - ma > max(sa, sb) else "NOT above the spread"))

# what one extraction and one fuse cost on an otherwise idle device (hipEvents around back-to-back calls on one stream)
plan = engine.get_stream_plan(net._cfg(), H, W, 5, video.device)
leaves = net.ordered_parameters()
cache = plan.new_cache(video.device)
out = torch.empty((1, 3, 4 * H, 4 * W), device=video.device)
for f in range(5):
    plan.extract(leaves, video[f], f, cache)
plan.fuse(leaves, [0, 1, 2, 3, 4], cache, out)


def event_ms(fn, n=50):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


x5 = video[:5][None].contiguous()
with torch.no_grad(), engine.FrozenWeights():
    net(x5)
    t_whole = event_ms(lambda: net(x5))
t_ext = event_ms(lambda: plan.extract(leaves, video[0], 0, cache))
t_fuse = event_ms(lambda: plan.fuse(leaves, [0, 1, 2, 3, 4], cache, out))
print("one stream, back to back: whole per-clip forward %.3f ms; extract (one frame, %d launches + frame copy) %.3f ms; "
      "fuse (gather + %d launches) %.3f ms; extract + fuse %.3f ms" % (t_whole, plan.n_launches[0], t_ext, plan.n_launches[1] - 1,
                                                                        t_fuse, t_ext + t_fuse))
