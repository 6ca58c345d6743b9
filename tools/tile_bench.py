#!/usr/bin/env python3
"""Frames in overlapping tiles (csrc/frame_stitch.hip, frames.stitch, super_resolve_frames(tile=...)) measured, in
one process:

1. the kernel: dvsr_frame_stitch through the C ABI into an SR frame of 3 x 2160 x 3840 fp32 from 2 x 2 and from 3 x 3 tiles with
   an overlap of 16 LR pixels at scale 4, against the torch composition on the same device (per tile one weighted
   accumulation into the frame: a multiply by the outer product of the two weight vectors and an add on the tile's region),
   and against dvsr_frame_flip_mean of the same build on the same output size, PER BYTE MOVED: algorithmic bytes are every tile
   read once and the frame written once (stitch), four sources read once and the frame written once (flip_mean).  Each figure
   is `--calls` back-to-back launches between two hipEvents, `--repeats` repetitions alternated, median and max - min spread.
   Target: stitch not slower per byte than flip_mean beyond that kernel's spread; the figure stands as measured.
2. a video both ways: a pinned uint8 RGB video of 360 x 640 through EDVR-M x4 to uint8 frames on the host with tile=None and
   with tile=(192, 336), in frames/s, beside the ratio of tile area to frame area.  A record, no bar.
3. a video that cannot run whole: a pinned NV12 video of 1080 x 1920 to NV12 2160 x 3840 (out_size), tile='auto', in_flight 2:
   the chosen tile, frames/s, and torch.cuda.max_memory_allocated beside adapt.tile_footprint.
4. the seam cost: PSNR (8-bit RGB, frames.score) of the tiled against the untiled frames at 360 x 640 for tile_overlap 0 / 8 /
   16 / 32.  Synthetic weights say little about trained ones: the default overlap of 16 stays a policy value.

usage (GPU box): python tools/tile_bench.py [--calls 20 --repeats 10 --frames 40 --video-repeats 3] > profiles/r17_tiles.txt"""
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
from dynavsr_amd import adapt, engine, frames, synth  # noqa: E402
from dynavsr_amd.models.archs.EDVR_arch import EDVR  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--frames", type=int, default=40)
ap.add_argument("--big-frames", type=int, default=12)
ap.add_argument("--video-repeats", type=int, default=3)
ap.add_argument("--in-flight", type=int, default=2)
ap.add_argument("--skip-video", action="store_true")
ap.add_argument("--skip-big", action="store_true")
args = ap.parse_args()
print("# tiles; %s; %d launches per figure, %d repetitions per kernel figure, %d per video figure" % (
    torch.cuda.get_device_name(0), args.calls, args.repeats, args.video_repeats))
lib = L.lib()


def timer(launch, n):
    """Device time per launch in us: n back-to-back launches (launch(i)) between two hipEvents."""
    for i in range(3):
        launch(i)
    torch.cuda.synchronize()

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            launch(i)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n
    return timed


def report(title, timers):
    us = {name: [] for name, _, _ in timers}
    for _ in range(args.repeats):
        for name, t, _ in timers:
            us[name].append(t())
    print(title)
    out = {}
    for name, _, nbytes in timers:
        m, sp = statistics.median(us[name]), max(us[name]) - min(us[name])
        out[name] = (m, sp, nbytes)
        print("  %-34s median %8.2f us per launch  spread %6.2f  %7.2f MB -> %7.1f GB/s, %6.3f ns per KB" % (
            name, m, sp, nbytes / 1e6, nbytes / m / 1e3, 1e6 * m / nbytes))
    return out


# ---- 1. the kernel
S, HP, WP, OV = 4, 540, 960, 16
H, W = S * HP, S * WP
flip_srcs = [torch.randn((3, H, W), device='cuda') for _ in range(5)]
dst = torch.empty((3, H, W), device='cuda')


def flip_mean_launch(i):
    p = [flip_srcs[(i + j) % 5].data_ptr() for j in range(4)]
    L.check(lib.dvsr_frame_flip_mean(p[0], p[1], p[2], p[3], dst.data_ptr(), 3, H, W, L.stream()), "dvsr_frame_flip_mean")


def stitch_case(ky, kx):
    # the smallest tile that gives ky x kx tiles, as adapt.choose_tile takes it
    th = -(-(HP + (ky - 1) * OV) // (4 * ky)) * 4
    tw = -(-(WP + (kx - 1) * OV) // (4 * kx)) * 4
    rows, cols = frames.stitch_table(HP, th, OV, S), frames.stitch_table(WP, tw, OV, S)
    assert (len(rows[0]), len(cols[0])) == (ky, kx)
    tiles = [torch.randn((ky * kx, 3, S * th, S * tw), device='cuda') for _ in range(2)]
    ar, ac = frames._stitch_axis(rows, dst.device), frames._stitch_axis(cols, dst.device)
    # the torch composition: dense per-tile weights on the device, one multiply-accumulate per tile on its region
    oy, ox = rows[0].tolist(), cols[0].tolist()

    def dense(table, k, length):
        o, first, w = table
        d = torch.zeros(length)
        for r in range(length):
            a = k - int(first[o[k] + r])
            d[r] = w[o[k] + r, a] if 0 <= a < w.shape[1] else 0.0
        return d.cuda()
    wy = [dense(rows, k, S * th) for k in range(ky)]
    wx = [dense(cols, k, S * tw) for k in range(kx)]
    w2 = [[wy[iy][:, None] * wx[ix][None, :] for ix in range(kx)] for iy in range(ky)]
    acc = torch.empty((3, H, W), device='cuda')

    def torch_launch(i):
        t = tiles[i % 2]
        acc.zero_()
        for iy in range(ky):
            for ix in range(kx):
                acc[:, oy[iy]:oy[iy] + S * th, ox[ix]:ox[ix] + S * tw] += w2[iy][ix] * t[iy * kx + ix]

    def ours(i):
        frames._stitch_run(tiles[i % 2], ky, kx, ar, ac, dst)
    ours(0)
    torch_launch(0)
    err = float((dst - acc).abs().max())
    nbytes = tiles[0].numel() * 4 + 12 * H * W
    res = report("stitch of %d x %d tiles of 3 x %d x %d into 3 x %d x %d fp32 (overlap %d LR pixels, scale %d); max-abs against the "
                 "torch composition %.2e (another summation order)" % (ky, kx, S * th, S * tw, H, W, OV, S, err),
                 [("torch: zero + %d x (mul, add)" % (ky * kx), timer(torch_launch, args.calls), nbytes),
                  ("dvsr_frame_flip_mean (same size)", timer(flip_mean_launch, args.calls), 5 * 12 * H * W),
                  ("dvsr_frame_stitch", timer(ours, args.calls), nbytes)])
    (ms, ss, bs), (mf, sf, bf) = res["dvsr_frame_stitch"], res["dvsr_frame_flip_mean (same size)"]
    per_s, per_f, margin = ms / bs, mf / bf, sf / bf
    print("  per byte: stitch %.4f, flip_mean %.4f us per MB, margin (flip_mean's spread) %.4f -> %s" % (
        1e6 * per_s, 1e6 * per_f, 1e6 * margin, "MET" if per_s <= per_f + margin else "MISSED"))
    del tiles


stitch_case(2, 2)
stitch_case(3, 3)
del flip_srcs, dst
torch.cuda.empty_cache()
if args.skip_video:
    sys.exit(0)

# ---- 2. a video both ways, 4. the seam cost
OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
net = EDVR()
net.load_state_dict(synth.damp_residual_branch(synth.edvr_state_dict(0), 0.02))
net = net.cuda()
h, w, T = 360, 640, args.frames
TILE = (192, 336)
clip = synth.clip(7, 1, 8, h, w)[0]
video = (torch.stack([clip[i % 8].roll(i // 8, -1) for i in range(T)]) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().pin_memory()
out = torch.empty((T, 4 * h, 4 * w, 3), dtype=torch.uint8).pin_memory()


def go(**kw):
    for i, y in enumerate(adapt.super_resolve_frames(OPT, net, video, in_flight=args.in_flight, **kw)):
        out[i].copy_(y, non_blocking=True)
    torch.cuda.synchronize()


def fps(frames_, fn, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(**kw)
    return frames_ / (time.perf_counter() - t0)


go()
go(tile=TILE)
whole, tiled = [], []
for _ in range(args.video_repeats):
    whole.append(fps(T, go))
    tiled.append(fps(T, go, tile=TILE))
ys, xs = adapt.tile_origins(h, TILE[0], 16), adapt.tile_origins(w, TILE[1], 16)
area = len(ys) * len(xs) * TILE[0] * TILE[1] / (h * w)
print("video %d frames uint8 RGB %dx%d pinned host -> uint8 %dx%d on the host, EDVR-M x4, in_flight %d, %d repetitions alternated" % (
    T, h, w, 4 * h, 4 * w, args.in_flight, args.video_repeats))
print("  tile=None          median %7.2f frames/s  spread %5.2f  (%s)" % (
    statistics.median(whole), max(whole) - min(whole), " ".join("%.2f" % v for v in whole)))
print("  tile=(%d, %d)    median %7.2f frames/s  spread %5.2f  (%s)" % (
    TILE + (statistics.median(tiled), max(tiled) - min(tiled), " ".join("%.2f" % v for v in tiled))))
print("  %d x %d tiles: tile area / frame area = %.3f; frame time tiled / whole = %.3f" % (
    len(ys), len(xs), area, statistics.median(whole) / statistics.median(tiled)))

n_psnr = min(T, 8)
ref_frames = [y.clone() for y in adapt.super_resolve_frames(OPT, net, video[:n_psnr])]
print("seam cost: PSNR (8-bit RGB) of tile=(%d, %d) against tile=None at %dx%d, mean over %d frames; synthetic weights" % (
    TILE + (h, w, n_psnr)))
for ov in (0, 8, 16, 32):
    got = [y.clone() for y in adapt.super_resolve_frames(OPT, net, video[:n_psnr], tile=TILE, tile_overlap=ov)]
    mse = [float(frames.score(a, b)[0]) for a, b in zip(got, ref_frames)]
    print("  tile_overlap %2d: PSNR %6.2f dB (min %6.2f), %d of %d frames identical" % (
        ov, statistics.mean(frames.psnr(m) for m in mse), min(frames.psnr(m) for m in mse), sum(m == 0 for m in mse), n_psnr))
del ref_frames, got
engine.release_stream_plans()
torch.cuda.empty_cache()
if args.skip_big:
    sys.exit(0)

# ---- 3. 1080p NV12 -> 2160p NV12, tile='auto'
h, w, T = 1080, 1920, args.big_frames
rs = np.random.RandomState(0)
base = torch.from_numpy(rs.randint(16, 236, (h * 3 // 2, w)).astype(np.uint8))
video = torch.stack([base.roll(4 * i, -1) for i in range(T)]).pin_memory()
out = torch.empty((T, 2160 * 3 // 2, 3840), dtype=torch.uint8).pin_memory()
try:
    next(adapt.super_resolve_frames(OPT, net, video, layout='nv12', out_size=(2160, 3840)))
    print("1080p whole: ran (unexpected)")
except ValueError as e:
    print("1080p with tile=None: ValueError: %s" % e)
free = torch.cuda.mem_get_info()[0]
chosen = adapt.choose_tile(net, h, w, 0.8 * free, 16, args.in_flight)
foot = adapt.tile_footprint(net, h, w, chosen, 16, args.in_flight)
torch.cuda.reset_peak_memory_stats()
base_alloc = torch.cuda.memory_allocated()


def go_big():
    for i, y in enumerate(adapt.super_resolve_frames(OPT, net, video, in_flight=args.in_flight, layout='nv12', out_size=(2160, 3840),
                                                     tile='auto')):
        out[i].copy_(y, non_blocking=True)
    torch.cuda.synchronize()


go_big()
big = [fps(T, go_big) for _ in range(args.video_repeats)]
peak = torch.cuda.max_memory_allocated()
print("video %d frames NV12 %dx%d pinned host -> NV12 2160x3840 on the host (out_size), EDVR-M x4, tile='auto', in_flight %d" % (
    T, h, w, args.in_flight))
print("  free device memory %.1f GB, budget 0.8 x that; chosen tile %s: %d x %d tiles" % (
    free / 1e9, chosen, len(adapt.tile_origins(h, chosen[0], 16)), len(adapt.tile_origins(w, chosen[1], 16))))
print("  median %6.2f frames/s  spread %5.2f  (%s)" % (statistics.median(big), max(big) - min(big), " ".join("%.2f" % v for v in big)))
print("  torch.cuda.max_memory_allocated %.2f GB (%.2f GB before the call: the network and nothing else); tile_footprint %.2f GB" % (
    peak / 1e9, base_alloc / 1e9, foot / 1e9))
