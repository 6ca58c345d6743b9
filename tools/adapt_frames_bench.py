#!/usr/bin/env python3
"""adapt.adapt_frames and the region losses behind it (csrc/misc.hip, dvsr_*_region_*) measured on the GPU box.

Without --step this is a driver that never touches the GPU: it runs each step below as a fresh child process under its own
`timeout`, stops at the first step that fails (a non-zero status, a time limit included) and writes what the steps printed
to --out (profiles/r18_adapt_frames.txt).  The protocol is tools/score_bench.py's.

  kernel  the four region entry points through the C ABI at [16,3,192,320] region 180x320 (the pixel loss of 16 frames) and
          [16,15,48,80] region 45x80 (their SLR term) -- one element per thread: a group has its own row of the grid --, and at
          [4,3,272,480] region 270x480 and [1,3,1088,1920] region 1080x1920, where a thread of the forwards takes 2 and 24
          elements (more than 1024 x 256 per group) and, at the last, a thread of the backwards 2 quads (more than 4096 x 256):
          the sizes at which the carried position is advanced.  Each against the existing grouped entry point on contiguous
          tensors of the region's element count: `--calls` back-to-back calls on one stream between two hipEvents, `--repeats`
          repetitions, the two alternated; median and max - min spread of the time per call.  The expectation to confirm or
          refute: a region kernel is not slower than the existing kernel beyond that kernel's own spread.
  video   a uint8 180x320 video of `--frames` frames in PINNED host memory through adapt_frames(frames_per_batch=4) to uint8
          frames on the host (EDVR-M x4 + MFDN, Adam, one step per frame), against adapt_video(frames_per_batch=4) over pre-cut
          float GPU clips of 192x320 whose results stay on the device -- the difference is what the front and the back end cost
          -- and against adapt_frames(baseline=False); alternated, `--video-repeats` timed passes each after a warm-up pass.

usage (GPU box): python tools/adapt_frames_bench.py [--out profiles/r18_adapt_frames.txt]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("kernel", 180), ("video", 420))                       # (step, its time limit in seconds)

ap = argparse.ArgumentParser()
ap.add_argument("--step", choices=[s for s, _ in STEPS])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_adapt_frames.txt"))
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=11)
ap.add_argument("--frames", type=int, default=60)
ap.add_argument("--video-repeats", type=int, default=5)
args = ap.parse_args()


def driver():
    text = []
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
               "--calls", str(args.calls), "--repeats", str(args.repeats), "--frames", str(args.frames),
               "--video-repeats", str(args.video_repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)       # (stderr goes to the terminal, not into the file)
        print(r.stdout, end="")
        text.append(r.stdout)
        if r.returncode:
            text.append("# step %s FAILED with status %d: stopped here\n" % (step, r.returncode))
            print(text[-1], end="")
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("".join(text))
    return r.returncode


if args.step is None:
    sys.exit(driver())

import statistics  # noqa: E402
import time        # noqa: E402

import numpy as np  # noqa: E402
import torch       # noqa: E402

sys.path.insert(0, ROOT)
import dynavsr_amd  # noqa: E402
dynavsr_amd.configure_runtime()
from dynavsr_amd import _lib as L  # noqa: E402
from dynavsr_amd import adapt, frames, synth  # noqa: E402

lib = L.lib()


def per_call_us(launch, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def step_kernel():
    print("# region losses, kernels; %s; %d calls between two events, %d repetitions alternated; `crop`: the existing grouped "
          "entry point on contiguous tensors of the region's element count" % (torch.cuda.get_device_name(0), args.calls,
                                                                              args.repeats))
    g = torch.Generator().manual_seed(0)
    for (k, planes, H, W), (h, w) in (((16, 3, 192, 320), (180, 320)), ((16, 15, 48, 80), (45, 80)),
                                      ((4, 3, 272, 480), (270, 480)), ((1, 3, 1088, 1920), (1080, 1920))):
        x, y = torch.rand((k, planes, H, W), generator=g).cuda(), torch.rand((k, planes, H, W), generator=g).cuda()
        xc, yc = x[..., :h, :w].contiguous(), y[..., :h, :w].contiguous()
        n = planes * h * w
        base, gl = torch.rand(k, generator=g).cuda(), torch.rand(k, generator=g).cuda()
        ws = torch.empty(k * int(lib.dvsr_charbonnier_workspace_bytes()), dtype=torch.uint8, device='cuda')
        lo = {v: torch.zeros(k, device='cuda') for v in ("r", "c")}
        gx, gxc = torch.empty_like(x), torch.empty_like(xc)
        st = L.stream()
        pairs = {
            "charbonnier forward": (
                lambda: lib.dvsr_charbonnier_region_forward(x.data_ptr(), y.data_ptr(), lo["r"].data_ptr(), k, planes, H, W, h, w,
                                                            1e-6, ws.data_ptr(), ws.numel(), st),
                lambda: lib.dvsr_charbonnier_forward_grouped(xc.data_ptr(), yc.data_ptr(), lo["c"].data_ptr(), n, k, 1e-6,
                                                             ws.data_ptr(), ws.numel(), st)),
            "charbonnier backward": (
                lambda: lib.dvsr_charbonnier_region_backward(x.data_ptr(), y.data_ptr(), gl.data_ptr(), gx.data_ptr(), k, planes,
                                                             H, W, h, w, 1e-6, st),
                lambda: lib.dvsr_charbonnier_backward_grouped(xc.data_ptr(), yc.data_ptr(), gl.data_ptr(), gxc.data_ptr(), n, k,
                                                              1e-6, st)),
            "l1 tail forward": (
                lambda: lib.dvsr_l1_tail_region_forward(x.data_ptr(), y.data_ptr(), base.data_ptr(), 10.0, lo["r"].data_ptr(), k,
                                                        planes, H, W, h, w, ws.data_ptr(), ws.numel(), st),
                lambda: lib.dvsr_l1_tail_forward_grouped(xc.data_ptr(), yc.data_ptr(), base.data_ptr(), 10.0, lo["c"].data_ptr(),
                                                         n, k, ws.data_ptr(), ws.numel(), st)),
            "l1 tail backward": (
                lambda: lib.dvsr_l1_tail_region_backward(x.data_ptr(), y.data_ptr(), gl.data_ptr(), 10.0, gx.data_ptr(), k, planes,
                                                         H, W, h, w, st),
                lambda: lib.dvsr_l1_tail_backward_grouped(xc.data_ptr(), yc.data_ptr(), gl.data_ptr(), 10.0, gxc.data_ptr(), n, k,
                                                          st)),
        }
        print("[%d,%d,%d,%d] region %dx%d (%.1f MB read per operand pair inside the region; the backward writes the whole "
              "%.1f MB of gx, the crop's %.1f MB)" % (k, planes, H, W, h, w, 2 * 4e-6 * k * n, 4e-6 * x.numel(), 4e-6 * xc.numel()))
        for name, (region, crop) in pairs.items():
            for fn in (region, crop):
                for _ in range(5):
                    L.check(fn(), name)
            torch.cuda.synchronize()
            if "forward" in name:
                assert torch.equal(lo["r"], lo["c"]), name + ": the region value is the crop's, bit for bit"
            else:
                assert torch.equal(gx[..., :h, :w], gxc), name + ": the in-region gradient is the crop's, bit for bit"
            us = {"region": [], "crop": []}
            for _ in range(args.repeats):
                us["region"].append(per_call_us(region, args.calls))
                us["crop"].append(per_call_us(crop, args.calls))
            med = {v: statistics.median(t) for v, t in us.items()}
            spread = {v: max(t) - min(t) for v, t in us.items()}
            d = med["region"] - med["crop"]
            print("  %-21s region %7.2f us (spread %5.2f)  crop %7.2f us (spread %5.2f)  region - crop = %+.2f us (%+.1f %%) -> %s" % (
                name, med["region"], spread["region"], med["crop"], spread["crop"], d, 100 * d / med["crop"],
                "not slower beyond the spread: CONFIRMED" if d <= spread["crop"] else "slower beyond the spread: MISSED"))


def step_video():
    from dynavsr_amd.models import create_model
    from dynavsr_amd.options import options as option
    opt = option.dict_to_nonedict(option.parse(os.path.join(ROOT, "dynavsr_amd", "options", "test", "EDVR", "EDVR_M_S4.yml"),
                                               is_train=False))
    opt["dist"] = False
    for k in ("pretrain_model_G", "pretrain_model_E"):
        opt["path"][k] = None
    model, est = create_model(opt)
    modelcp, estcp = create_model(opt)
    _, est_fixed = create_model(opt)
    model.netG.load_state_dict(synth.edvr_state_dict(0)); est.netE.load_state_dict(synth.mfdn_state_dict(0))
    est_fixed.netE.load_state_dict(synth.mfdn_state_dict(1))
    nets = (model, est, modelcp, estcp, est_fixed)
    H, W, N, K = 180, 320, args.frames, 4
    yy, xx = np.mgrid[0:H, 0:W + N].astype(np.float64)
    field = np.stack([128 + 40 * (np.sin(2 * np.pi * xx / 61.0 + c) + np.sin(2 * np.pi * yy / 47.0 + 2 * c)) for c in range(3)], -1)
    field = np.clip(np.rint(field), 0, 255).astype(np.uint8)
    video = torch.from_numpy(np.ascontiguousarray(np.stack([field[:, t:t + W] for t in range(N)]))).pin_memory()
    host_out = torch.empty((N, 4 * H, 4 * W, 3), dtype=torch.uint8).pin_memory()
    windows, _ = adapt.video_windows(N, 5, 'new_info')
    padded = [frames.ingest(video[i], 'hwc_rgb', 16, 'reflect') for i in range(N)]
    clips = [{'LQs': torch.stack([padded[j] for j in win])[None]} for win in windows]          # float GPU clips of 192x320
    print("# adapt_frames, video; %s; %d frames uint8 %dx%d pinned host -> uint8 %dx%d host, frames_per_batch %d, Adam, "
          "adapt_iter %d; `clips`: adapt_video over pre-cut float GPU clips of %dx%d, results left on the device" % (
              torch.cuda.get_device_name(0), N, H, W, 4 * H, 4 * W, K, opt['train']['maml']['adapt_iter'], *padded[0].shape[-2:]))

    def run_frames(baseline):
        for i, (_, sr) in enumerate(adapt.adapt_frames(opt, *nets, video, frames_per_batch=K, baseline=baseline)):
            host_out[i].copy_(sr, non_blocking=True)
        torch.cuda.synchronize()

    def run_clips():
        for _ in adapt.adapt_video(opt, *nets, clips, frames_per_batch=K):
            pass
        torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return N / (time.perf_counter() - t0)
    runs = {"clips": run_clips, "frames": lambda: run_frames(True), "no baseline": lambda: run_frames(False)}
    for fn in runs.values():
        fn()
    fps = {k: [] for k in runs}
    for _ in range(args.video_repeats):
        for k, fn in runs.items():
            fps[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in fps.items()}
    names = {"clips": "adapt_video, pre-cut float clips", "frames": "adapt_frames, uint8 host -> uint8 host",
             "no baseline": "adapt_frames(baseline=False)"}
    for k in runs:
        print("  %-40s median %6.2f frames/s = %6.2f ms per frame  spread %5.2f  (%s)" % (
            names[k], med[k], 1e3 / med[k], max(fps[k]) - min(fps[k]), " ".join("%.2f" % v for v in fps[k])))
    print("  front + back end: %+.2f ms per frame (adapt_frames - adapt_video)" % (1e3 / med["frames"] - 1e3 / med["clips"]))
    print("  baseline forward: %+.2f ms per frame (baseline=True - baseline=False), %.1f %% of a frame" % (
        1e3 / med["frames"] - 1e3 / med["no baseline"], 100 * (1 - med["frames"] / med["no baseline"])))


{"kernel": step_kernel, "video": step_video}[args.step]()
