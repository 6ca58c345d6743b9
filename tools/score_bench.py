#!/usr/bin/env python3
"""Frame scoring (csrc/frame_score.hip, frames.score, super_resolve_frames(gt=...)) measured on the GPU box.

Without --step this is a driver that never touches the GPU: it runs each step below as a fresh child process under its own
`timeout`, stops at the first step that fails (a non-zero status, a time limit included) and writes what the steps printed
to --out (profiles/r15_frame_score.txt).

  kernel  dvsr_frame_score through the C ABI at 720x1280, channel rgb, for a uint8 RGB pair and for an fp32 planar pair,
          against dvsr_frame_metrics (util.frame_metrics' three launches) on the same fp32 frames: `--calls` back-to-back calls
          on one stream between two hipEvents, `--repeats` repetitions, the three alternated; median and max - min spread of the
          time per call (launch gaps included: the calls are 2 and 3 launches long).  Buffers are allocated once, outside the
          timing.  The fp32 pair must give frame_metrics' mse exactly and its SSIM within 1e-10.
          Compulsory traffic: the uint8 pair reads 2 x 3 x 720 x 1280 B = 5.5 MB; frame_metrics reads 22 MB of fp32, writes
          5.5 MB of quantised planes and reads them again.  The expectation to confirm or refute: dvsr_frame_score is not slower
          than dvsr_frame_metrics beyond the spread.
  video   frames/s of a uint8 180x320 video in PINNED host memory -> uint8 SR frames on the host (EDVR-M x4), without gt and
          with gt= (a pinned uint8 720x1280 ground-truth video that travels as bytes, channel rgb), alternated, `--video-repeats`
          timed passes each after a warm-up pass, with the spread of the gt=None runs.

usage (GPU box): python tools/score_bench.py [--out profiles/r15_frame_score.txt]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("kernel", 180), ("video", 420))                       # (step, its time limit in seconds)

ap = argparse.ArgumentParser()
ap.add_argument("--step", choices=[s for s, _ in STEPS])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_frame_score.txt"))
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
from dynavsr_amd import adapt, frames, synth  # noqa: E402

lib = L.lib()
r = np.random.RandomState(0)


def per_call_us(launch, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def step_kernel():
    h, w = 720, 1280
    print("# frame score, kernel; %s; %dx%d, channel rgb, %d calls between two events, %d repetitions alternated" % (
        torch.cuda.get_device_name(0), h, w, args.calls, args.repeats))
    a8 = r.randint(0, 256, (h, w, 3)).astype(np.uint8)
    b8 = np.clip(a8.astype(np.int32) + r.randint(-12, 13, a8.shape), 0, 255).astype(np.uint8)
    ua, ub = torch.from_numpy(a8).cuda(), torch.from_numpy(b8).cuda()
    fa = torch.from_numpy(np.ascontiguousarray(np.transpose(a8.astype(np.float32) / 255., (2, 0, 1)))).cuda()
    fb = torch.from_numpy(np.ascontiguousarray(np.transpose(b8.astype(np.float32) / 255., (2, 0, 1)))).cuda()
    du = L.FrameDesc(L.FRAME_U8_HWC_RGB, h, w, 3 * w, 0, 3)
    df = L.FrameDesc(L.FRAME_F32_CHW, h, w, w, h * w, 1)
    sargs = L.ScoreArgs(L.SCORE_RGB, 0, 8, 0.0, 1.0)
    n_s, n_m = lib.dvsr_frame_score_workspace_bytes(3, h, w), lib.dvsr_frame_metrics_workspace_bytes(3, h, w)
    ws_s, ws_m = torch.empty(n_s, dtype=torch.uint8, device='cuda'), torch.empty(n_m, dtype=torch.uint8, device='cuda')
    out = {k: torch.zeros(2, dtype=torch.float64, device='cuda') for k in ("u8", "f32", "metrics")}

    def score(x, y, d, o):
        L.check(lib.dvsr_frame_score(x.data_ptr(), ctypes.byref(d), y.data_ptr(), ctypes.byref(d), ctypes.byref(sargs),
                                     o.data_ptr(), ws_s.data_ptr(), n_s, L.stream()), "dvsr_frame_score")

    def metrics():
        L.check(lib.dvsr_frame_metrics(fa.data_ptr(), fb.data_ptr(), 3, h, w, 0.0, 1.0, None, out["metrics"].data_ptr(),
                                       ws_m.data_ptr(), n_m, L.stream()), "dvsr_frame_metrics")
    runs = {"u8": lambda: score(ua, ub, du, out["u8"]), "f32": lambda: score(fa, fb, df, out["f32"]), "metrics": metrics}
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    res = {k: v.tolist() for k, v in out.items()}
    assert res["u8"][0] == res["f32"][0] == res["metrics"][0], res
    assert abs(res["f32"][1] - res["metrics"][1]) < 1e-10 and res["u8"][1] == res["f32"][1], res
    us = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, fn in runs.items():
            us[k].append(per_call_us(fn, args.calls))
    med = {k: statistics.median(v) for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}
    names = {"u8": "dvsr_frame_score   uint8 RGB pair (5.5 MB read)",
             "f32": "dvsr_frame_score   fp32 planar pair (22 MB read)",
             "metrics": "dvsr_frame_metrics fp32 planar pair (22 MB read, 5.5 MB written and re-read)"}
    print("mse %.6f (PSNR %.4f dB), SSIM %.12f: the three agree (mse exactly, SSIM within 1e-10)" % (
        res["u8"][0], frames.psnr(res["u8"][0]), res["u8"][1]))
    for k in runs:
        print("  %-78s %8.2f us per call, spread %6.2f  (%s)" % (names[k], med[k], spread[k], " ".join("%.1f" % v for v in us[k])))
    for k in ("u8", "f32"):
        d = med[k] - med["metrics"]
        print("  %s - frame_metrics = %+.2f us (%+.1f %%); spread of frame_metrics %.2f -> %s" % (
            k, d, 100 * d / med["metrics"], spread["metrics"],
            "not slower beyond the spread: CONFIRMED" if d <= spread["metrics"] else "slower beyond the spread: REFUTED"))


def step_video():
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    H, W, N = 180, 320, args.frames
    opt = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
    net = EDVR()
    net.load_state_dict(synth.edvr_state_dict(0))
    net = net.cuda()
    yy, xx = np.mgrid[0:H, 0:W + N].astype(np.float64)
    field = np.stack([128 + 40 * (np.sin(2 * np.pi * xx / 61.0 + c) + np.sin(2 * np.pi * yy / 47.0 + 2 * c)) for c in range(3)], -1)
    field = np.clip(np.rint(field), 0, 255).astype(np.uint8)
    video = torch.from_numpy(np.ascontiguousarray(np.stack([field[:, t:t + W] for t in range(N)]))).pin_memory()
    gt = torch.from_numpy(r.randint(0, 256, (N, 4 * H, 4 * W, 3)).astype(np.uint8)).pin_memory()
    host_out = torch.empty((N, 4 * H, 4 * W, 3), dtype=torch.uint8).pin_memory()
    scores = torch.zeros((N, 2), dtype=torch.float64, device='cuda')
    print("# frame score, video; %s; %d frames uint8 %dx%d pinned host -> uint8 %dx%d host, in_flight %d; gt: uint8 %dx%d "
          "pinned host, channel rgb" % (torch.cuda.get_device_name(0), N, H, W, 4 * H, 4 * W, args.in_flight, 4 * H, 4 * W))

    def run(with_gt):
        kw = dict(gt=gt, scores=scores) if with_gt else {}
        for i, sr in enumerate(adapt.super_resolve_frames(opt, net, video, in_flight=args.in_flight, **kw)):
            host_out[i].copy_(sr, non_blocking=True)
        torch.cuda.synchronize()

    def timed(with_gt):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(with_gt)
        return N / (time.perf_counter() - t0)

    run(False)
    keep = host_out.clone()
    run(True)
    assert torch.equal(keep, host_out), "gt= must not change the frames"
    want = frames.score(host_out[N // 2], gt[N // 2])
    assert torch.equal(scores[N // 2].view(torch.int64), want.view(torch.int64)), "a row of scores is frames.score of its frame"
    del keep
    f0, f1 = [], []
    for _ in range(args.video_repeats):
        f0.append(timed(False))
        f1.append(timed(True))
    m0, m1, s0 = statistics.median(f0), statistics.median(f1), max(f0) - min(f0)
    print("  gt=None  median %7.1f frames/s  spread %5.1f  (%s)" % (m0, s0, " ".join("%.1f" % v for v in f0)))
    print("  gt=      median %7.1f frames/s  spread %5.1f  (%s)" % (m1, max(f1) - min(f1), " ".join("%.1f" % v for v in f1)))
    print("  gt - None = %+.1f frames/s (%+.2f %%); spread of the gt=None runs %.1f -> %s" % (
        m1 - m0, 100 * (m1 - m0) / m0, s0,
        "inside the spread of the gt=None runs" if m1 >= m0 - s0 else "OUTSIDE the spread: the cost stands as measured"))


{"kernel": step_kernel, "video": step_video}[args.step]()
