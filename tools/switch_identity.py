#!/usr/bin/env python
"""What the native library chooses and computes under its DVSR_* switches, to compare two builds of it (this tree's and a
parent commit's, built into a scratch directory).

    python tools/switch_identity.py --parent PARENT.so [--new NEW.so] --work DIR --part host|plans|bits [--report FILE]

One library per fresh process (DVSR_HIP_LIB) and one process per switch value, one process with the GPU open at a time, every
step under its own time limit; the first fault, abort or time-out ends the run.  This tree's Python drives both libraries through
the C ABI (engine.Plan / EstimatorPlan, never the plan caches, which ask the library for its switch table).

  host   no device: dvsr_conv2d_wgrad_geometry and dvsr_conv2d_wgrad_workspace_bytes over the rows of
         tests/golden/wgrad_choice_parent.json under the DVSR_WGRAD_* switches; equal line for line.
  plans  needs the device for its CU count, launches nothing: per plan num_params, launch counts, workspace sizes, every op_info,
         op_launch_count in both modes, op_output of both outputs, plan_work and plan_work_nograd, under the defaults and the BUILD
         switches (and DVSR_SPLIT_TH8_FROM); equal line for line, a plan one library refuses must be refused by the other.
  bits   forward with the no-grad and the need-grad workspace (sha256 of the output and of the whole workspace), backward
         (gradients saved as fp32), under the defaults and one non-default value of every PROCESS switch: the parent three times,
         the new library once.  Forward digests must be equal.  A gradient the parent reproduces bit for bit must be bit-equal;
         for the others the relative L2 of parent~parent (largest of three pairs) and new~parent (largest of three), per tensor
         and as one vector per plan; the whole-plan vector is judged against the parent's own figure times --margin.
"""
import argparse
import ctypes
import hashlib
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

HOST = ["", "DVSR_WGRAD_WIDE=0", "DVSR_WGRAD_S3V=0", "DVSR_WGRAD_S3W=0", "DVSR_WGRAD_SPLIT3=0", "DVSR_WGRAD_S3_KYS_BELOW=0",
        "DVSR_WGRAD_S3_KYS_BELOW=100000", "DVSR_WGRAD_S3_WGS=64"]
PLANS = ["", "DVSR_CONV_WINO=0", "DVSR_CONV_WINO=2", "DVSR_CONV_WINO3=0", "DVSR_CONV_WINO5=0", "DVSR_CONV_WINO5=2", "DVSR_CONV_WINO5=3",
         "DVSR_CONV_V1=1", "DVSR_EST_SPLIT=0", "DVSR_EST_SPLIT2=0", "DVSR_EST_SPLIT2=2", "DVSR_FUSE_ACT_BWD=0", "DVSR_BWD_STREAMS=0",
         "DVSR_PCD_HOIST=0", "DVSR_SPLIT_TH8_FROM=1"]
BITS = ["", "DVSR_DCN_FWD=dma", "DVSR_DCN_FWD=reg", "DVSR_DCN_FWD=lds", "DVSR_DCN_BWD=unfused", "DVSR_DCN_BWD=fp32", "DVSR_UP2=4",
        "DVSR_TSA_V=1", "DVSR_TSA_V=4", "DVSR_TSA_DUAL=0", "DVSR_CONV_LAST_MFMA=1", "DVSR_EST_FUSE_PAD=0", "DVSR_FUSE_RES_BWD=0",
        "DVSR_BWD_FORK_EVERY=1", "DVSR_BWD_PROBE=0", "DVSR_WGRAD_SPLIT3=0", "DVSR_DEGRADE_GENERIC=1", "DVSR_DEGRADE_GENERIC=0"]
EDVR_M = (64, 5, 8, 5, 10, 4, 2)


# ---- the children: one library, one setting ---------------------------------------------------------------------------
def load_library():
    """This tree's bindings over the library DVSR_HIP_LIB names.  A parent from before the dvsr_switch_* queries lacks exactly
    those, which _declare lists last."""
    from dynavsr_amd import _lib as L
    L._lib = ctypes.CDLL(os.environ["DVSR_HIP_LIB"])
    try:
        L._lib._signatures = L._declare(L._lib)
    except AttributeError as e:
        assert "dvsr_switch_" in str(e), e
    return L


def child_host():
    L = load_library()
    with open(os.path.join(ROOT, "tests", "golden", "wgrad_choice_parent.json")) as f:
        doc = json.load(f)
    for row in doc["rows"]:
        r = dict(zip(doc["columns"], row))
        dense = r["Cin"] * r["H"] * r["W"]
        d = L.Conv2dDesc(0x10000000 + r["x_off"], None, None, None, None, 0x20000000 + r["gy_off"], r["N"], r["Cin"], 0, r["H"], r["W"],
                         r["Cout"], r["ks"], r["stride"], r["pad"], 0, 2 * r["gy_ps"], 1, dense + r["x_bs_extra"] if r["x_bs_extra"] else 0,
                         0, None, 0)
        geo = (ctypes.c_int * 8)()
        rc = L.lib().dvsr_conv2d_wgrad_geometry(d, r["mode"], r["groups"], ctypes.byref(geo))
        print(row, "rc", rc, "geo", list(geo), "ws", L.lib().dvsr_conv2d_wgrad_workspace_bytes(d, r["groups"]))


def plan_lines(name, make):
    """Everything the queries say about one plan; a refused plan is one line with the library's message."""
    from dynavsr_amd import _lib as L
    try:
        p = make()
    except RuntimeError as e:
        print("%s | refused | %s" % (name, " ".join(str(e).split())))
        return
    est = not hasattr(p, "op_info")
    print("%s | params %d launches %d backward %d ws %d %d" % (name, p.n_params, p.n_launches, p.n_backward_launches,
                                                            p.workspace_bytes(False), p.workspace_bytes(True)))
    kind, opname = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    fl, by = ctypes.c_double(), ctypes.c_double()
    ia, off, n = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong()
    for i in range(p.n_launches):      # (an estimator's handle starts with its tape: the per-op queries read it too)
        L.check(L.lib().dvsr_edvr_op_info(p._h, i, kind, 32, opname, 64, ctypes.byref(fl), ctypes.byref(by)), "dvsr_edvr_op_info")
        outs = []
        for which in (0, 1):
            rc = L.lib().dvsr_edvr_op_output(p._h, i, which, ctypes.byref(ia), ctypes.byref(off), ctypes.byref(n))
            outs.append("%d:%d:%d" % (ia.value, off.value, n.value) if rc == 0 else "none(%d)" % rc)   # (most launches have one output)
        print("%s | op %d | %s %s %s %s | launches %d %d | out %s" % (
            name, i, kind.value.decode(), opname.value.decode(), fl.value.hex(), by.value.hex(),
            L.lib().dvsr_edvr_op_launch_count(p._h, i, 0), L.lib().dvsr_edvr_op_launch_count(p._h, i, 1), " ".join(outs)))
    works = [p.work()] if est else [p.work(), p.work(nograd=True)]
    for w in works:
        print("%s | work | %s" % (name, " ".join(float(v).hex() for v in w.values())))


def child_plans():
    load_library()
    import torch
    from dynavsr_amd import engine
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")
    for bf in (0, 2):
        for b, h, w in ((1, 180, 320), (1, 140, 320), (1, 44, 288), (2, 32, 48)):
            plan_lines("edvr_m bf%d %dx%dx%d" % (bf, b, h, w), lambda: engine.Plan(EDVR_M + (bf,), b, h, w))
        plan_lines("edvr_m bf%d 16x44x80 groups=sets=16" % bf, lambda: engine.Plan(EDVR_M + (bf,), 16, 44, 80, 16, 16))
    plan_lines("mfdn_x4 1x5x3x32x32", lambda: engine.EstimatorPlan((engine.MFDN, 64, 3, 4, 5), 1, 32, 32))
    plan_lines("sfdn 2x3x20x28", lambda: engine.EstimatorPlan((engine.SFDN, 32, 3, 2, 1), 2, 20, 28))
    print("done")


def child_bits(dump):
    L = load_library()
    import torch
    from dynavsr_amd import engine, synth
    from dynavsr_amd.models.archs.LRimg_estimator import DirectKernelEstimatorVideo, DirectKernelEstimator_CMS
    dev = torch.device("cuda")
    grads = {}

    def digest(t):
        return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:24]

    def noise(seed, shape):
        return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)

    networks = "DVSR_DEGRADE_GENERIC" not in os.environ      # (that switch: the degradation op alone)
    params = [v.to(dev) for v in synth.edvr_state_dict(0).values()]
    for b, h, w in ((2, 32, 48), (1, 44, 288)) if networks else ():
        name = "edvr_%dx%dx%d" % (b, h, w)
        plan = engine.Plan(EDVR_M + (0,), b, h, w)
        x = synth.clip(3, b, 5, h, w).to(dev)
        for mode, need_grad in (("nograd", False), ("needgrad", True)):
            ws = torch.zeros(plan.workspace_bytes(need_grad), dtype=torch.uint8, device=dev)
            out = torch.zeros((b, 3, 4 * h, 4 * w), device=dev)
            plan.forward(params, x, out, ws)
            torch.cuda.synchronize()
            print("%s/%s/forward/out %s" % (name, mode, digest(out)))
            print("%s/%s/forward/ws %s" % (name, mode, digest(ws)))
        gparams, gx = [torch.zeros_like(p) for p in params], torch.zeros_like(x)
        plan.backward(params, x, noise(5, out.shape), gparams, gx, ws)
        torch.cuda.synchronize()
        for i, g in enumerate(gparams):
            grads["%s/gparam%03d" % (name, i)] = g.cpu()
        grads["%s/gx" % name] = gx.cpu()
    for name, net, sd, cfg, xshape, oshape, hw in (
            ("mfdn_x4_1x5x3x32x32", DirectKernelEstimatorVideo(64, 3, 4), synth.mfdn_state_dict(0), (engine.MFDN, 64, 3, 4, 5),
             (1, 3, 5, 32, 32), (1, 3, 5, 8, 8), (32, 32)),
            ("sfdn_2x3x20x28", None, synth.sfdn_state_dict(0), None, (2, 3, 20, 28), (2, 3, 10, 14), (20, 28))) if networks else ():
        if net is None:
            nf = sd["conv0.weight"].shape[0]
            net, cfg = DirectKernelEstimator_CMS(nf), (engine.SFDN, nf, 3, 2, 1)
        net.load_state_dict(sd, strict=True)
        eparams = [p.detach().to(dev) for p in net.ordered_parameters()]
        plan = engine.EstimatorPlan(cfg, xshape[0], hw[0], hw[1])
        x = torch.rand(xshape, generator=torch.Generator().manual_seed(7)).to(dev)
        for mode, need_grad in (("nograd", False), ("needgrad", True)):
            ws = torch.zeros(plan.workspace_bytes(need_grad), dtype=torch.uint8, device=dev)
            out = torch.zeros(oshape, device=dev)
            plan.forward(eparams, x, out, ws)
            torch.cuda.synchronize()
            print("%s/%s/forward/out %s" % (name, mode, digest(out)))
            print("%s/%s/forward/ws %s" % (name, mode, digest(ws)))
        gparams = [torch.zeros_like(p) for p in eparams]
        plan.backward(eparams, x, noise(9, oshape), gparams, ws)
        torch.cuda.synchronize()
        for i, g in enumerate(gparams):
            grads["%s/gparam%02d" % (name, i)] = g.cpu()
    # the degradation op (DVSR_DEGRADE_GENERIC): 27 x 27 kernels, scale 4, one kernel per frame
    img, ker = torch.rand((5, 3, 64, 64), generator=torch.Generator().manual_seed(11)).to(dev), noise(12, (5, 27, 27)).abs()
    lr = torch.zeros((5, 3, 16, 16), device=dev)
    L.check(L.lib().dvsr_degrade_apply(L.ptr(img), L.ptr(ker), L.ptr(lr), 5, 3, 64, 64, 27, 4, 5, 0, 1, L.stream()), "dvsr_degrade_apply")
    torch.cuda.synchronize()
    print("degrade_5x3x64x64_k27_s4/out %s" % digest(lr))
    torch.save(grads, dump)
    print("done")


# ---- the parent process: runs the children, compares ---------------------------------------------------------------------
class Stop(Exception):
    pass


def run_child(part, lib, setting, limit, dump=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DVSR_")}
    env["DVSR_HIP_LIB"] = lib
    if setting:
        k, v = setting.split("=")
        env[k] = v
    cmd = [sys.executable, os.path.abspath(__file__), "--child", part] + (["--dump", dump] if dump else [])
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise Stop("%s under %r with %s: no end after %d s -- stopping" % (part, setting, lib, limit))
    if r.returncode != 0:
        raise Stop("%s under %r with %s: exit status %d -- stopping\n%s" % (part, setting, lib, r.returncode, r.stderr[-2000:]))
    return r.stdout.splitlines()


def sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def compare_lines(part, settings, args, say, limit):
    ok = True
    for s in settings:
        a, b = run_child(part, args.parent, s, limit), run_child(part, args.new, s, limit)
        same = a == b
        ok = ok and same
        refused = sum(" | refused | " in line for line in a)
        say("   %-32s %5d lines, sha256 %s, refused plans %d: %s" % (s or "default", len(a), sha(a), refused, "EQUAL" if same else "DIFFERENT"))
        if not same:
            for x, y in itertools.zip_longest(a, b):
                if x != y:
                    say("      parent: %s\n      new:    %s" % (x, y))
                    break
    return ok


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm()) if float(b.norm()) else float((a - b).norm())


def compare_bits(args, say):
    import torch
    ok = True
    for s in BITS:
        tag = (s or "default").replace("=", "_")
        runs = []
        for who, lib in (("parent1", args.parent), ("parent2", args.parent), ("parent3", args.parent), ("new", args.new)):
            dump = os.path.join(args.work, "%s_%s.pt" % (tag, who))
            runs.append((run_child("bits", lib, s, 240, dump), torch.load(dump)))
        (l1, g1), (l2, g2), (l3, g3), (ln, gn) = runs
        stable_fwd, equal_fwd = l1 == l2 == l3, ln == l1
        say("   %s" % (s or "default"))
        say("      forward outputs and workspaces, %d digests (sha256 of all: %s): parent reproduces itself: %s, new == parent: %s"
            % (len(l1) - 1, sha(l1), "yes" if stable_fwd else "NO", "yes" if equal_fwd else "NO"))
        ok = ok and stable_fwd and equal_fwd
        if not equal_fwd:
            for x, y in zip(l1, ln):
                if x != y:
                    say("         parent: %s\n         new:    %s" % (x, y))
        parents, outliers, stable_bad, nstable = (g1, g2, g3), [], [], 0
        for plan in sorted({k.split("/")[0] for k in g1}):
            names = sorted(k for k in g1 if k.startswith(plan + "/gparam"))
            vec = lambda g: torch.cat([g[k].flatten() for k in names])   # noqa: E731
            pp = max(rel(vec(a), vec(b)) for a, b in itertools.combinations(parents, 2))
            npar = max(rel(vec(gn), vec(p)) for p in parents)
            good = npar <= args.margin * pp
            ok = ok and good
            say("      %-22s all %3d parameter gradients as one vector: parent~parent %.3e, new~parent %.3e (x%.2f) %s"
                % (plan, len(names), pp, npar, npar / pp if pp else float("inf"), "ok" if good else "OUTSIDE x%.2f" % args.margin))
            for k in sorted(k for k in g1 if k.startswith(plan + "/")):
                if all(torch.equal(parents[0][k], p[k]) for p in parents[1:]):
                    nstable += 1
                    if not torch.equal(gn[k], parents[0][k]):
                        stable_bad.append(k)
                    continue
                tp = max(rel(a[k], b[k]) for a, b in itertools.combinations(parents, 2))
                tn = max(rel(gn[k], p[k]) for p in parents)
                if tn > tp:
                    outliers.append((tn / tp, k, tp, tn))
        ok = ok and not stable_bad
        say("      tensors the parent reproduces bit for bit: %d, of which the new library differs in: %d %s" % (nstable, len(stable_bad), stable_bad or ""))
        outliers.sort(reverse=True)
        say("      tensors above the parent's largest of three pairs (not judged): %d%s" % (
            len(outliers), "".join("\n         %-40s parent~parent %.3e new~parent %.3e (x%.2f)" % (k, tp, tn, r) for r, k, tp, tn in outliers[:5])))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--parent")
    ap.add_argument("--new", default=os.path.join(ROOT, "dynavsr_amd", "libdynavsr_hip.so"))
    ap.add_argument("--work", default=".")
    ap.add_argument("--part", choices=("host", "plans", "bits"), default="host")
    ap.add_argument("--report", default=None)
    ap.add_argument("--margin", type=float, default=1.1,
                    help="whole-plan gradient vector: new~parent may be this many times parent~parent")
    args = ap.parse_args()
    if args.child:
        return {"host": child_host, "plans": child_plans, "bits": lambda: child_bits(args.dump)}[args.child]()
    out = open(args.report, "a") if args.report else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    args.parent, args.new = os.path.abspath(args.parent), os.path.abspath(args.new)
    os.makedirs(args.work, exist_ok=True)
    try:
        if args.part == "host":
            say("host: wgrad geometry and workspace over the golden rows, parent against new, one process per value")
            ok = compare_lines("host", HOST, args, say, 120)
        elif args.part == "plans":
            say("plans: every query of every plan, parent against new, one process per library and value")
            ok = compare_lines("plans", PLANS, args, say, 180)
        else:
            say("bits: parent three times, new once, one process per run (whole-plan margin x%.2f)" % args.margin)
            ok = compare_bits(args, say)
    except Stop as e:
        say(str(e))
        return 2
    say("%s: %s" % (args.part, "IDENTICAL" if ok else "DIFFERENCES"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
