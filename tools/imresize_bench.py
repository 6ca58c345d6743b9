#!/usr/bin/env python3
"""MATLAB's imresize of a frame from the form it arrives in (csrc/frame_imresize.hip: dvsr_frame_imresize, frames.imresize,
video.evaluate_degraded with frames.Imresize) measured on the GPU box.

Without --step this is a driver that never touches the GPU: it runs each step below as a fresh child process under its own
`timeout`, stops at the first step that fails (a non-zero status, a time limit included) and writes what the steps printed
to --out (profiles/r20_imresize.txt).

  kernel  dvsr_frame_imresize through the C ABI, scale 1/4, antialiased (16-tap windows), quantiser on, against the composition
          that gives a frame of the same size from existing entries which this change does not touch: dvsr_frame_ingest into a
          contiguous fp32 [3,h,w] buffer + dvsr_frame_resize to h/4 x w/4 (torch's antialiased bicubic: 17-tap windows, no
          quantiser); a uint8 RGB 720x1280 frame and a uint8 RGB 2160x3840 frame.  `--calls` back-to-back calls on one stream
          between two hipEvents, `--repeats` repetitions, the two alternated; median and max - min spread of the time per call.
          Buffers and tables are made once, outside the timing.  The two follow different definitions and are not compared.
          THE EXPECTATION, written down before the run: on both sizes dvsr_frame_imresize is not slower than the composition
          beyond the composition's own spread -- it reads the bytes once where the composition also writes and re-reads an
          fp32 HR frame.
          Also recorded, no expectation: an fp32 planar 180x320 frame up-scaled x4 to 720x1280 (4-tap windows, no quantiser).
  video   frames/s of a uint8 720x1280 ground-truth video in PINNED host memory (`--frames` frames) through
          video.evaluate_degraded(.., frames.Imresize(4)) (EDVR-M x4, uint8 SR frames scored against the HR frames, channel
          rgb) against video.evaluate_frames on the LR tensor made beforehand, alternated, `--video-repeats` timed passes each
          after a warm-up pass.  The scores of the two must agree bit for bit.

usage (GPU box): python tools/imresize_bench.py [--out profiles/r20_imresize.txt]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("kernel", 240), ("video", 420))                       # (step, its time limit in seconds)

ap = argparse.ArgumentParser()
ap.add_argument("--step", choices=[s for s, _ in STEPS])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_imresize.txt"))
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=11)
ap.add_argument("--frames", type=int, default=60)
ap.add_argument("--video-repeats", type=int, default=5)
ap.add_argument("--in-flight", type=int, default=2)
args = ap.parse_args()


def driver():
    text = []
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
               "--calls", str(args.calls), "--repeats", str(args.repeats), "--frames", str(args.frames),
               "--video-repeats", str(args.video_repeats), "--in-flight", str(args.in_flight)]
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

import ctypes      # noqa: E402
import statistics  # noqa: E402
import time        # noqa: E402

import numpy as np  # noqa: E402
import torch       # noqa: E402

sys.path.insert(0, ROOT)
import dynavsr_amd  # noqa: E402
dynavsr_amd.configure_runtime()
from dynavsr_amd import _lib as L  # noqa: E402
from dynavsr_amd import frames, synth, video  # noqa: E402

lib = L.lib()
r = np.random.RandomState(0)
SCALE = 4


def per_call_us(launch, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def smooth_u8(h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 60 * (np.sin(2 * np.pi * xx / 61.0 + c) + np.sin(2 * np.pi * yy / 47.0 + 2 * c)) for c in range(3)], -1)
    return np.clip(np.rint(img + r.randint(-8, 9, img.shape)), 0, 255).astype(np.uint8)


def measure(runs):
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, fn in runs.items():
            us[k].append(per_call_us(fn, args.calls))
    for k in runs:
        print("  %-42s %8.2f us per call, spread %6.2f  (%s)" % (k, statistics.median(us[k]), max(us[k]) - min(us[k]),
                                                                " ".join("%.1f" % v for v in us[k])))
    return {k: statistics.median(v) for k, v in us.items()}, {k: max(v) - min(v) for k, v in us.items()}


def step_kernel():
    dev = torch.device('cuda', torch.cuda.current_device())
    print("# imresize, kernel; %s; %d calls between two events, %d repetitions alternated" % (
        torch.cuda.get_device_name(0), args.calls, args.repeats))
    for h, w in ((720, 1280), (2160, 3840)):
        oh, ow = frames.imresize_size(h, w, (1, SCALE))
        x = torch.from_numpy(smooth_u8(h, w)).cuda()
        desc = L.FrameDesc(L.FRAME_U8_HWC_RGB, h, w, 3 * w, 0, 3)
        rows, cols = frames._imresize_axis(h, (1, SCALE), True, dev), frames._imresize_axis(w, (1, SCALE), True, dev)
        trows, tcols = frames._resize_axis(h, oh, dev), frames._resize_axis(w, ow, dev)
        mid = torch.empty((3, h, w), dtype=torch.float32, device='cuda')
        out = {k: torch.empty((3, oh, ow), dtype=torch.float32, device='cuda') for k in ("fused", "composition")}

        def fused():
            L.check(lib.dvsr_frame_imresize(x.data_ptr(), ctypes.byref(desc), h, w, 1, SCALE, 1, out["fused"].data_ptr(), ow,
                                            oh * ow, oh, ow, ctypes.byref(rows), ctypes.byref(cols), 1, L.stream()),
                    "dvsr_frame_imresize")

        def composition():
            L.check(lib.dvsr_frame_ingest(x.data_ptr(), ctypes.byref(desc), mid.data_ptr(), h, w, L.FRAME_PAD_REFLECT,
                                          L.stream()), "dvsr_frame_ingest")
            L.check(lib.dvsr_frame_resize(mid.data_ptr(), h, w, h, w, out["composition"].data_ptr(), oh, ow, oh, ow,
                                          ctypes.byref(trows), ctypes.byref(tcols), L.stream()), "dvsr_frame_resize")
        print("uint8 RGB %dx%d -> fp32 [3,%d,%d] (source %.1f MB, fp32 HR frame %.1f MB); windows of %d taps against %d" % (
            h, w, oh, ow, x.numel() / 1e6, 3 * h * w * 4 / 1e6, rows.taps, trows.taps))
        med, spread = measure({"dvsr_frame_imresize": fused, "dvsr_frame_ingest + dvsr_frame_resize": composition})
        dlt = med["dvsr_frame_imresize"] - med["dvsr_frame_ingest + dvsr_frame_resize"]
        sp = spread["dvsr_frame_ingest + dvsr_frame_resize"]
        print("  imresize - composition = %+.2f us (%+.1f %%); spread of the composition %.2f -> %s" % (
            dlt, 100 * dlt / med["dvsr_frame_ingest + dvsr_frame_resize"], sp,
            "not slower beyond the spread: CONFIRMED" if dlt <= sp else "slower beyond the spread: REFUTED"))
    h, w = 180, 320
    oh, ow = frames.imresize_size(h, w, (SCALE, 1))
    xf = (torch.from_numpy(smooth_u8(h, w)).cuda().permute(2, 0, 1).float() / 255).contiguous()
    fdesc = L.FrameDesc(L.FRAME_F32_CHW, h, w, w, h * w, 1)
    rows, cols = frames._imresize_axis(h, (SCALE, 1), True, dev), frames._imresize_axis(w, (SCALE, 1), True, dev)
    up = torch.empty((3, oh, ow), dtype=torch.float32, device='cuda')

    def upscale():
        L.check(lib.dvsr_frame_imresize(xf.data_ptr(), ctypes.byref(fdesc), h, w, SCALE, 1, 1, up.data_ptr(), ow, oh * ow, oh, ow,
                                        ctypes.byref(rows), ctypes.byref(cols), 0, L.stream()), "dvsr_frame_imresize")
    print("fp32 planar %dx%d -> fp32 [3,%d,%d] at x%d (windows of %d taps, result %.1f MB)" % (h, w, oh, ow, SCALE, rows.taps,
                                                                                             3 * oh * ow * 4 / 1e6))
    measure({"dvsr_frame_imresize": upscale})


def step_video():
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    H, W, N = 720, 1280, args.frames
    opt = {'scale': SCALE, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
    net = EDVR()
    net.load_state_dict(synth.edvr_state_dict(0))
    net = net.cuda()
    d = frames.Imresize(SCALE)
    field = smooth_u8(H, W + N)
    hr = torch.from_numpy(np.ascontiguousarray(np.stack([field[:, t:t + W] for t in range(N)]))).pin_memory()
    lr = video.degrade_frames(hr, d)
    gt = [f for f in hr]
    kw = dict(out='hwc_rgb', in_flight=args.in_flight)
    print("# imresize, video; %s; %d frames uint8 %dx%d pinned host, EDVR-M x%d on fp32 %dx%d, uint8 SR frames scored against "
          "the HR frames (channel rgb), in_flight %d" % (torch.cuda.get_device_name(0), N, H, W, SCALE, lr.shape[-2], lr.shape[-1],
                                                         args.in_flight))

    def degraded():
        return video.evaluate_degraded(opt, net, hr, d, **kw)

    def pre_degraded():
        return video.evaluate_frames(opt, net, lr, gt, gt_layout='hwc_rgb', **kw)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return N / (time.perf_counter() - t0)

    (s0, a), (s1, b) = degraded(), pre_degraded()
    assert torch.equal(a, b), "evaluate_degraded must give evaluate_frames' scores on the degraded video"
    print("  mean PSNR %.4f dB, SSIM %.6f: the two agree bit for bit" % (s0['mean']['psnr'], s0['mean']['ssim']))
    f0, f1 = [], []
    for _ in range(args.video_repeats):
        f0.append(timed(pre_degraded))
        f1.append(timed(degraded))
    m0, m1, sp = statistics.median(f0), statistics.median(f1), max(f0) - min(f0)
    print("  evaluate_frames on the LR tensor              median %7.1f frames/s  spread %5.1f  (%s)" % (
        m0, sp, " ".join("%.1f" % v for v in f0)))
    print("  evaluate_degraded(Imresize(4)) on the HR video median %7.1f frames/s  spread %5.1f  (%s)" % (
        m1, max(f1) - min(f1), " ".join("%.1f" % v for v in f1)))
    print("  degraded - pre-degraded = %+.1f frames/s (%+.2f %%): what BI of %d HR frames costs (%.2f ms per frame)" % (
        m1 - m0, 100 * (m1 - m0) / m0, N, 1e3 * (1 / m1 - 1 / m0)))


{"kernel": step_kernel, "video": step_video}[args.step]()
