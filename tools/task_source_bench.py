#!/usr/bin/env python3
"""Meta-training tasks made on the device (csrc/task.hip, csrc/degrade.hip: dvsr_task_degrade / dvsr_task_gather;
dynavsr_amd/data/tasks.py) measured on the GPU box.

Without --step this is a driver that never touches the GPU: it writes the expectations below into --out
(profiles/r21_task_source.txt) BEFORE anything runs, then runs each step as a fresh child process under its own `timeout`,
stops at the first step that fails (a non-zero status, a time limit included) and appends what the steps printed.

Each expectation is a comparison against code that exists without this change, not against the code under test:

  batch    the four launches of make_batch (B = 16 tasks, N = 5, 256x256 crops of uint8 720x1280 frames, scale 4, K = 27) against
           the composition they replace -- 80 dvsr_frame_degrade + 16 dvsr_degrade_apply + 80 dvsr_frame_ingest + the
           dvsr_frame_flip of every clip that a task flips -- through the C ABI, tables and buffers made once outside the timing.
           `--calls` back-to-back batches on one stream between two hipEvents, `--repeats` repetitions, the two alternated;
           median and max - min spread.  The two must agree bit for bit.  EXPECTED: device time not slower than the composition
           beyond the composition's own spread.  Reported beside it: the host wall time of one make_batch call (kernels shifted
           with scipy, tables filled, one upload, four launches) and the B = 1 figures.
  kernels  dvsr_frame_degrade (uint8 720x1280) and dvsr_degrade_apply (5x3x256x256) of this build against the parent commit's
           library (--parent-lib, loaded into the same process), alternated, same protocol.  EXPECTED: each inside the parent's
           spread -- the kernels gained a template parameter, no work.  Without --parent-lib the step says so and measures this
           build alone.
  step     adapt.meta_train_step at tools/meta_bench.py's shapes (B = 4 and 16; LR 5x3x64x64, EDVR-M x4 + MFDN, adapt_iter 1) fed
           a fresh TaskSource batch every iteration against the same step on one resident batch, alternated, wall clock over
           `--iters` iterations, `--step-repeats` repetitions.  EXPECTED: tasks/s not below the resident run by more than that
           run's spread.  TaskSource alone is reported in tasks/s.

usage (GPU box): python tools/task_source_bench.py [--parent-lib PATH] [--out profiles/r21_task_source.txt]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("batch", 300), ("kernels", 180), ("step", 420))      # (step, its time limit in seconds)
HEADER = """# Meta-training tasks made on the device: tools/task_source_bench.py on an MI355X.
# Expectations, written before the run; each compares against code that exists without this change:
#  1. batch: the four launches (B = 16, N = 5, 256x256 crops of uint8 720x1280, scale 4, K = 27) are not slower in device time than
#     the 80 dvsr_frame_degrade + 16 dvsr_degrade_apply + 80 dvsr_frame_ingest + flips they replace, beyond that composition's spread.
#  2. kernels: dvsr_frame_degrade at 720x1280 and dvsr_degrade_apply at 5x3x256x256 are each inside the parent library's spread.
#  3. step: meta_train_step fed a fresh TaskSource batch per iteration is not below the resident-batch run by more than its spread.
"""

ap = argparse.ArgumentParser()
ap.add_argument("--step", choices=[s for s, _ in STEPS])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_task_source.txt"))
ap.add_argument("--parent-lib", default="")
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=11)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--step-repeats", type=int, default=5)
args = ap.parse_args()


def driver():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(HEADER)
    print(HEADER, end="")
    rc = 0
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--calls", str(args.calls),
               "--repeats", str(args.repeats), "--iters", str(args.iters), "--step-repeats", str(args.step_repeats),
               "--parent-lib", args.parent_lib]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)       # (stderr goes to the terminal, not into the file)
        text = r.stdout
        if r.returncode:
            text += "# step %s FAILED with status %d: stopped here\n" % (step, r.returncode)
        print(text, end="")
        with open(args.out, "a") as f:
            f.write(text)
        rc = r.returncode
        if rc:
            break
    return rc


if args.step is None:
    sys.exit(driver())

import ctypes      # noqa: E402
import random      # noqa: E402
import statistics  # noqa: E402
import time        # noqa: E402

import numpy as np  # noqa: E402
import torch       # noqa: E402

sys.path.insert(0, ROOT)
import dynavsr_amd  # noqa: E402
dynavsr_amd.configure_runtime()
from dynavsr_amd import _lib as L  # noqa: E402
from dynavsr_amd.data import tasks as T  # noqa: E402
from dynavsr_amd.data.random_kernel_generator import Degradation  # noqa: E402

lib = L.lib()
SCALE, KS, N, H, W = 4, 21, 5, 720, 1280


def per_call_us(launch, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def smooth_u8(r, t, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for i in range(t):
        img = np.stack([128 + 60 * (np.sin(2 * np.pi * (xx + 3 * i) / 61.0 + c) + np.sin(2 * np.pi * yy / 47.0 + 2 * c)) for c in range(3)], -1)
        out.append(np.clip(np.rint(img + r.randint(-8, 9, img.shape)), 0, 255).astype(np.uint8))
    return np.stack(out)


def pool_of(sequences=4, frames=8):
    r = np.random.RandomState(0)
    return T.FramePool({"%03d" % s: smooth_u8(r, frames, H, W) for s in range(sequences)})


def alternated(runs, names, calls, repeats, unit="us per call"):
    us = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            us[k].append(per_call_us(fn, calls))
    med = {k: statistics.median(v) for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}
    for k in runs:
        print("  %-58s %9.2f %s, spread %6.2f  (%s)" % (names[k], med[k], unit, spread[k], " ".join("%.1f" % v for v in us[k])))
    return med, spread


def batch_case(pool, B, crop=256):
    """Tables, kernels and buffers of one batch, made once; returns (fused, composition, outputs of both)."""
    py_rng, np_rng = random.Random(1), np.random.RandomState(1)
    keys = sorted(pool.lengths)
    picks = [(keys[b % len(keys)], [(b + f) % pool.lengths[keys[0]] for f in range(N)]) for b in range(B)]
    draws = [T.draw_task(py_rng, np_rng, H, W, crop) for _ in range(B)]
    kernels = T.shifted_kernels(draws, KS, SCALE)
    K = int(kernels.shape[-1])
    hl, hs = T.check_geometry(crop, K, SCALE)
    n = B * N
    dev = pool.device
    new = {"GT": torch.empty((B, N, 3, crop, crop), device=dev), "LQs": torch.empty((B, N, 3, hl, hl), device=dev),
           "SuperLQs": torch.empty((B, N, 3, hs, hs), device=dev)}
    old = {k: torch.empty_like(v) for k, v in new.items()}
    lr0 = torch.empty((n, 3, hl, hl), device=dev)
    tb = n * T.ITEM.itemsize
    host = np.empty(3 * tb + kernels.nbytes, dtype=np.uint8)
    t_hr0, t_hr, t_lr = (host[i * tb:(i + 1) * tb].view(T.ITEM) for i in range(3))
    i = 0
    for b, ((key, fr), d) in enumerate(zip(picks, draws)):
        for f in fr:
            src, row, plane = pool.crop_item(key, f, d["py"], d["px"])
            t_hr0[i], t_hr[i] = (src, row, plane, b, 0), (src, row, plane, b, T.draw_flags(d))
            t_lr[i] = (lr0.data_ptr() + 4 * i * 3 * hl * hl, hl, hl * hl, b, T.draw_flags(d))
            i += 1
    host[3 * tb:].view(np.float32)[:] = kernels.reshape(-1)
    devb = torch.from_numpy(host).to(dev)

    def fused():
        T.four_launches(pool, host.ctypes.data, devb.data_ptr(), B, N, crop, K, SCALE, lr0, new["SuperLQs"], new["GT"], new["LQs"])

    kt = torch.from_numpy(kernels).to(dev)
    lr0_c = torch.empty_like(lr0)
    tmp = {k: torch.empty_like(v[0]) for k, v in new.items()}
    descs = [[L.FrameDesc(pool.format, crop, crop, W * 3, 0, 3) for _ in range(N)] for _ in range(B)]
    srcs = [[pool.crop_item(key, f, d["py"], d["px"])[0] for f in fr] for (key, fr), d in zip(picks, draws)]

    tos = [dict(tmp, LQs=lr0_c[b * N:(b + 1) * N]) if T.draw_flags(d) else {k: v[b] for k, v in old.items()} for b, d in enumerate(draws)]

    def composition():
        st = L.stream()
        for b, d in enumerate(draws):
            fl = T.draw_flags(d)
            # a task that flips nothing writes where the result belongs; the others into temporaries that dvsr_frame_flip reads
            to = tos[b]
            for f in range(N):
                L.check(lib.dvsr_frame_degrade(srcs[b][f], ctypes.byref(descs[b][f]), kt[b].data_ptr(), K, SCALE,
                                               to["LQs"][f].data_ptr(), hl, hl * hl, 1, st), "dvsr_frame_degrade")
                L.check(lib.dvsr_frame_ingest(srcs[b][f], ctypes.byref(descs[b][f]), to["GT"][f].data_ptr(), crop, crop,
                                              L.FRAME_PAD_REFLECT, st), "dvsr_frame_ingest")
            L.check(lib.dvsr_degrade_apply(to["LQs"].data_ptr(), kt[b].data_ptr(), to["SuperLQs"].data_ptr(), N, 3, hl, hl, K, SCALE, 1,
                                           0, 0, st), "dvsr_degrade_apply")
            if fl:
                for k, src in to.items():
                    L.check(lib.dvsr_frame_flip(src.data_ptr(), old[k][b].data_ptr(), 3 * N, src.shape[-2], src.shape[-1], fl, st),
                            "dvsr_frame_flip")
    return fused, composition, new, old, (picks, draws)


def step_batch():
    pool = pool_of()
    print("# task source, batch; %s; pool %d sequences x %d frames uint8 %dx%d (%.0f MB); scale %d, 21-tap kernels shifted; %d calls "
          "between two events, %d repetitions alternated" % (torch.cuda.get_device_name(0), len(pool.lengths), 8, H, W,
                                                             pool.nbytes / 1e6, SCALE, args.calls, args.repeats))
    for B in (16, 1):
        fused, composition, new, old, (picks, draws) = batch_case(pool, B)
        for fn in (fused, composition):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for k in new:
            assert torch.equal(new[k], old[k]), "the four launches must give the composition's bits (%s)" % k
        flips = sum(1 for d in draws if T.draw_flags(d))
        print("B = %d tasks x %d frames, 256x256 crops -> LR 64x64, SLR 16x16; %d of the tasks flip; the two agree bit for bit" % (B, N, flips))
        names = {"fused": "4 launches (dvsr_task_degrade x2, dvsr_task_gather x2)",
                 "composition": "%d frame_degrade + %d degrade_apply + %d frame_ingest + %d flips" % (B * N, B, B * N, 3 * flips)}
        med, spread = alternated({"fused": fused, "composition": composition}, names, args.calls if B > 1 else 4 * args.calls, args.repeats,
                                 "us per batch")
        dlt = med["fused"] - med["composition"]
        print("  fused - composition = %+.2f us (%+.1f %%); spread of the composition %.2f -> %s" % (
            dlt, 100 * dlt / med["composition"], spread["composition"],
            "not slower beyond the spread: CONFIRMED" if dlt <= spread["composition"] else "slower beyond the spread: REFUTED"))
        staging = [T.Staging(T.table_bytes(B * N, B), pool.device) for _ in range(2)]
        wall = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(20):
                staging[i & 1].wait()
                T.make_batch(pool, picks, draws, KS, SCALE, out=new, staging=staging[i & 1])
            host_s = (time.perf_counter() - t0) / 20
            torch.cuda.synchronize()
            wall.append(1e6 * host_s)
        print("  make_batch host wall time (kernels shifted, tables, upload, launches; no wait for the device)  median %8.1f us per "
              "batch, spread %.1f" % (statistics.median(wall), max(wall) - min(wall)))


def step_kernels():
    print("# task source, kernels; %s; this build against the parent commit's library%s; %d calls between two events, %d repetitions "
          "alternated" % (torch.cuda.get_device_name(0), "" if args.parent_lib else " -- NOT GIVEN (--parent-lib): this build alone",
                          args.calls, args.repeats))
    libs = {"this build": lib}
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("dvsr_frame_degrade", "dvsr_degrade_apply"):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = lib._signatures[name]
        libs = {"parent": parent, "this build": lib}
    d = Degradation(KS, SCALE, theta=0.4, sigma=[2.0, 0.8])
    kt = d._shifted_on(torch.device("cuda"))[0]
    K = int(kt.shape[-1])
    r = np.random.RandomState(0)
    x8 = torch.from_numpy(smooth_u8(r, 1, H, W)[0]).cuda()
    desc = L.FrameDesc(L.FRAME_U8_HWC_RGB, H, W, 3 * W, 0, 3)
    clip = torch.rand(5, 3, 256, 256, device="cuda")
    outs = {k: (torch.empty(3, 180, 320, device="cuda"), torch.empty(5, 3, 64, 64, device="cuda")) for k in libs}
    cases = (("dvsr_frame_degrade uint8 720x1280", lambda l, o: L.check(l.dvsr_frame_degrade(
                 x8.data_ptr(), ctypes.byref(desc), kt.data_ptr(), K, SCALE, o[0].data_ptr(), 320, 180 * 320, 1, L.stream()))),
             ("dvsr_degrade_apply 5x3x256x256", lambda l, o: L.check(l.dvsr_degrade_apply(
                 clip.data_ptr(), kt.data_ptr(), o[1].data_ptr(), 5, 3, 256, 256, K, SCALE, 1, 0, 1, L.stream()))))
    for i, (what, call) in enumerate(cases):
        runs = {k: (lambda l=l, k=k: call(l, outs[k])) for k, l in libs.items()}
        for fn in runs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        if args.parent_lib:
            assert torch.equal(outs["parent"][i], outs["this build"][i]), "the bits of %s changed" % what
        print("%s%s" % (what, "; the two agree bit for bit" if args.parent_lib else ""))
        med, spread = alternated(runs, {k: k for k in runs}, args.calls, args.repeats)
        if args.parent_lib:
            dlt = med["this build"] - med["parent"]
            print("  this build - parent = %+.2f us (%+.1f %%); spread of the parent %.2f -> %s" % (
                dlt, 100 * dlt / med["parent"], spread["parent"],
                "inside the parent's spread: CONFIRMED" if abs(dlt) <= spread["parent"] else
                ("faster beyond the spread" if dlt < 0 else "slower beyond the spread: REFUTED")))


def step_step():
    from dynavsr_amd import synth
    from dynavsr_amd.adapt import meta_train_step
    from dynavsr_amd.models import create_model
    from dynavsr_amd.options import options as option
    opt = option.dict_to_nonedict(option.parse(os.path.join(ROOT, "dynavsr_amd/options/test/EDVR/EDVR_M_S4.yml"), is_train=False))
    opt["dist"] = False
    for k in ("pretrain_model_G", "pretrain_model_E"):
        opt["path"][k] = None
    opt["train"]["maml"]["adapt_iter"] = 1
    model, est = create_model(opt)
    modelcp, estcp = create_model(opt)
    model.netG.load_state_dict(synth.edvr_state_dict(0)); est.netE.load_state_dict(synth.mfdn_state_dict(0))
    params = [p for p in model.netG.parameters()] + [p for p in est.netE.parameters()]
    optimizer = torch.optim.Adam(params, lr=1e-5, betas=(0.9, 0.99))
    pool = pool_of()
    print("# task source, step; %s; meta_train_step (EDVR-M x4 + MFDN, adapt_iter 1, inner 'reference') at LR 5x3x64x64; pool %d x %d "
          "frames uint8 %dx%d; wall clock over %d iterations, %d repetitions alternated" % (
              torch.cuda.get_device_name(0), len(pool.lengths), 8, H, W, args.iters, args.step_repeats))
    for B in (4, 16):
        sopt = {"scale": SCALE, "datasets": {"train": {"N_frames": N, "interval_list": [1], "patch_size": 128, "kernel_size": KS,
                                                       "batch_size": B}}}
        source = T.TaskSource(sopt, pool, seed=0)
        feed = iter(())

        def fresh():
            nonlocal feed
            b = next(feed, None)
            if b is None:
                feed = iter(source)
                b = next(feed)
            return b
        resident = fresh()

        def timed(get):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                r = meta_train_step(opt, model, est, modelcp, estcp, get(), optimizer)
            torch.cuda.synchronize()
            assert np.isfinite(r["loss_q"])
            return B * args.iters / (time.perf_counter() - t0)
        for get in (lambda: resident, fresh):
            timed(get)
        t = {"resident": [], "fed": []}
        for _ in range(args.step_repeats):
            t["resident"].append(timed(lambda: resident))
            t["fed"].append(timed(fresh))
        alone = []
        for _ in range(args.step_repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(4 * args.iters):
                fresh()
            torch.cuda.synchronize()
            alone.append(B * 4 * args.iters / (time.perf_counter() - t0))
        m = {k: statistics.median(v) for k, v in t.items()}
        sp = max(t["resident"]) - min(t["resident"])
        print("B = %d tasks" % B)
        for k, name in (("resident", "one resident batch"), ("fed", "a fresh TaskSource batch per iteration")):
            print("  %-42s median %7.1f tasks/s  spread %5.1f  (%s)" % (name, m[k], max(t[k]) - min(t[k]), " ".join("%.1f" % v for v in t[k])))
        dlt = m["fed"] - m["resident"]
        print("  fed - resident = %+.1f tasks/s (%+.2f %%); spread of the resident run %.1f -> %s" % (
            dlt, 100 * dlt / m["resident"], sp, "not starved: CONFIRMED" if -dlt <= sp else "below the resident run beyond its spread: REFUTED"))
        print("  TaskSource alone                           median %7.1f tasks/s  spread %5.1f" % (statistics.median(alone), max(alone) - min(alone)))


{"batch": step_batch, "kernels": step_kernels, "step": step_step}[args.step]()
