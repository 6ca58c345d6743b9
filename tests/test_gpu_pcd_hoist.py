"""The PCD offset convs' reference half, convolved once per clip (engine.hip: Op::hoist; conv2d_wino5_kernel's PRE instantiation).

L1_offset_conv1, L2_offset_conv1 and cas_offset_conv1 convolve cat([frame_i, ref]) for the frames of a clip.  A convolution is
linear in its input channels,

    lrelu(conv_W(cat(f_i, ref)) + b)  =  lrelu(conv_W[:, :c0](f_i) + [conv_W[:, c0:](ref) + b]),

and the bracket does not depend on i: the no-grad forward computes it once per clip (the reference part: one launch of the
F(4x4) kernel, no activation) and hands it to the main part's epilogue as a pre-activation addend (`pre`, `pre_bdiv` of
dvsr_conv2d_desc).  Three layers of tests: the addend at op level against fp64, the plan's decision through
dvsr_edvr_op_launch_count, and the network against its own grad-mode forward, the CPU oracle and its batched / in-flight forms."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, relerr
from dynavsr_amd import synth

pytestmark = pytest.mark.gpu

CFG = (64, 5, 8, 5, 10, 4, 2, 0)          # EDVR-M x4: nf, nframes, groups, front_RBs, back_RBs, scale, center, bf16_mfma
HOISTED = ("L1_offset_conv1", "L2_offset_conv1", "cas_offset_conv1")
UNSUPPORTED = -2                          # DVSR_ERR_UNSUPPORTED


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in ("DVSR_CONV_WINO", "DVSR_CONV_WINO3", "DVSR_CONV_WINO5", "DVSR_PCD_HOIST"):
        monkeypatch.delenv(k, raising=False)


def rnd(*shape, seed, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def lrelu64(t, act):
    return F.leaky_relu(t, 0.1) if act == 1 else t


# ---- 1. the addend at op level ------------------------------------------------------------------------------------------
N, BDIV, C0, C1 = 6, 3, 24, 16            # two clips of three frames; two inputs of different widths (3 and 2 chunks)


@pytest.fixture(scope="module")
def op_inputs():
    """Inputs and fp64 references of every op-level case, computed once on the CPU and left unchanged: per (cout, h, w) the
    un-activated, un-biased fp64 sums of the unsplit form and of the split form (which agree below 1e-12)."""
    out = {}
    for cout in (64, 72, 128):
        for h, w in ((12, 64), (10, 64)):
            x0, x1 = rnd(N, C0, h, w, seed=1), rnd(N // BDIV, C1, h, w, seed=6)
            wt = rnd(cout, C0 + C1, 3, 3, seed=2, scale=1 / np.sqrt((C0 + C1) * 9))
            b = rnd(cout, seed=3, scale=0.1)
            x1b = x1.repeat_interleave(BDIV, 0)                   # batch item n reads x1[n // BDIV]
            whole = F.conv2d(torch.cat([x0, x1b], 1).double(), wt.double(), None, 1, 1)
            split = F.conv2d(x0.double(), wt[:, :C0].double(), None, 1, 1) + \
                F.conv2d(x1.double(), wt[:, C0:].double(), None, 1, 1).repeat_interleave(BDIV, 0)
            assert relerr(split, whole) < 1e-12
            out[cout, h, w] = dict(x0=x0, x1=x1, wt=wt, b=b, whole=whole)
    return out


def _desc(L, x0, x1, w, b, res, y, n, c0, c1, h, wd, cout, act, ps=0, bdiv=1, pre=None, pre_bdiv=0, ks=3):
    return L.Conv2dDesc(L.ptr(x0), L.ptr(x1), L.ptr(w), L.ptr(b), L.ptr(res), L.ptr(y), n, c0, c1, h, wd, cout, ks, 1, ks // 2, act, ps,
                        bdiv, 0, 0, pre, pre_bdiv)


def _run(L, d, what="dvsr_conv2d_forward_packed"):
    ws = torch.empty(max(int(L.lib().dvsr_conv2d_packed_workspace_bytes(d)), 16), dtype=torch.uint8, device="cuda")
    L.check(L.lib().dvsr_conv2d_forward_packed(d, ws.data_ptr(), ws.numel(), L.stream()), what)
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["2", "3"])                      # DVSR_CONV_WINO5: 8 x 64-pixel workgroup tiles / 16 x 32
@pytest.mark.parametrize("h,w", [(12, 64), (10, 64)])             # 10: H % 4 == 2, the last tile row is cut
@pytest.mark.parametrize("cout", [64, 72, 128])                   # 72: a partial cout block; 128: the second block's channel offset
def test_addend_against_fp64_and_the_unsplit_launch(cout, h, w, mode, op_inputs, monkeypatch):
    """y = act(conv_Wa(x0) + b? + pre[n / 3]) with pre = conv_Wb(x1) (+ b) from the library's own reference-part launch, against
    fp64 lrelu(conv(cat(x0, x1 broadcast)) + b) on the CPU (4e-6 relative L2: test_conv3x3_winograd_f4x4's bar) and against the
    unsplit launch cat(x0, x1 / x1_bdiv = 3) on the same kernel (5e-6).  Activation lrelu and none, with and without bias.  The
    addend lives inside a NaN-filled buffer and the outputs start as NaN: a read outside the addend's rows (past a cut tile
    row, a cout block's idle channels, another clip's image) or a missed store shows up as a non-finite output."""
    from dynavsr_amd import _lib as L
    monkeypatch.setenv("DVSR_CONV_WINO5", mode)
    c = op_inputs[cout, h, w]
    x0, x1, wt, b = (c[k].cuda() for k in ("x0", "x1", "wt", "b"))
    wa, wb = wt[:, :C0].contiguous(), wt[:, C0:].contiguous()      # the split of the weights is the caller's
    guard, numel = 256, (N // BDIV) * cout * h * w
    for act in (1, 0):
        for bias in (b, None):
            buf = torch.full((guard + numel + guard,), float("nan"), device="cuda")
            pre = buf[guard:guard + numel]
            d_ref = _desc(L, x1, None, wb, bias, None, pre, N // BDIV, C1, 0, h, w, cout, 0)
            geo = (ctypes.c_int * 4)()
            _run(L, d_ref)
            assert bool(torch.isfinite(pre).all()) and bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + numel:]).all())
            y = torch.full((N, cout, h, w), float("nan"), device="cuda")
            d = _desc(L, x0, None, wa, None, None, y, N, C0, 0, h, w, cout, act, pre=pre.data_ptr(), pre_bdiv=BDIV)
            L.check(L.lib().dvsr_conv2d_packed_geometry(d, ctypes.byref(geo)), "dvsr_conv2d_packed_geometry")
            assert list(geo)[3] == 5 and list(geo)[1] == (8 if mode == "2" else 16), list(geo)
            _run(L, d)
            assert bool(torch.isfinite(y).all())
            yu = torch.full((N, cout, h, w), float("nan"), device="cuda")
            _run(L, _desc(L, x0, x1, wt, bias, None, yu, N, C0, C1, h, w, cout, act, bdiv=BDIV))
            ref = c["whole"] if bias is None else c["whole"] + c["b"].double().view(1, -1, 1, 1)
            ref = lrelu64(ref, act)
            e64, eu = relerr(y, ref), relerr(y, yu)
            print("cout %d %dx%d mode %s act %d bias %d: vs fp64 %.2e, vs unsplit %.2e" % (cout, h, w, mode, act, bias is not None, e64, eu))
            assert e64 < 4e-6 and eu < 5e-6, (e64, eu)


def test_addend_is_refused_where_no_kernel_implements_it():
    """`pre` with `res`, with PixelShuffle, on launches the F(4x4) kernel does not take (W % 4 != 0, channels not in whole
    chunks, 1x1) and on dvsr_conv2d_forward (no pack): DVSR_ERR_UNSUPPORTED, and the output is not written."""
    from dynavsr_amd import _lib as L
    n, c0, h, w, cout = 2, 16, 8, 64, 64

    def rc_of(c0=c0, w=w, cout=cout, res=False, ps=0, ks=3, packed=True):
        x = torch.zeros(n, c0, h, w, device="cuda")
        wt = torch.zeros(cout, c0, ks, ks, device="cuda")
        pre = torch.zeros(n, cout, h, w, device="cuda")
        r = torch.zeros(n, cout, h, w, device="cuda") if res else None
        y = torch.full((n, cout, h, w), float("nan"), device="cuda")
        d = _desc(L, x, None, wt, None, r, y, n, c0, 0, h, w, cout, 1, ps=ps, pre=pre.data_ptr(), pre_bdiv=1, ks=ks)
        if packed:
            ws = torch.empty(max(int(L.lib().dvsr_conv2d_packed_workspace_bytes(d)), 1 << 20), dtype=torch.uint8, device="cuda")
            rc = L.lib().dvsr_conv2d_forward_packed(d, ws.data_ptr(), ws.numel(), L.stream())
        else:
            rc = L.lib().dvsr_conv2d_forward(d, L.stream())
        torch.cuda.synchronize()
        assert rc == 0 or bool(torch.isnan(y).all())
        return rc

    assert rc_of() == 0                                           # (the eligible form of the same descriptor runs)
    assert rc_of(res=True) == UNSUPPORTED
    assert b"addend" in L.lib().dvsr_last_error()
    assert rc_of(ps=2) == UNSUPPORTED
    assert rc_of(w=66) == UNSUPPORTED
    assert rc_of(c0=20) == UNSUPPORTED
    assert rc_of(cout=16) == UNSUPPORTED
    assert rc_of(ks=1) == UNSUPPORTED
    assert rc_of(packed=False) == UNSUPPORTED


# ---- 2. the plan --------------------------------------------------------------------------------------------------------
def launch_counts(plan, nograd):
    from dynavsr_amd import _lib as L
    names = [nm.split("[")[0] for (_k, nm, _f, _b) in plan.op_info()]
    return names, [L.lib().dvsr_edvr_op_launch_count(plan._h, i, int(nograd)) for i in range(plan.n_launches)]


def split_ops(b, h, w):
    from dynavsr_amd import engine
    torch.cuda.current_device()
    names, cnt = launch_counts(engine.Plan(CFG, b, h, w), True)
    assert set(cnt) <= {1, 2}
    return [n for n, c in zip(names, cnt) if c == 2]


def test_headline_plan_splits_the_three_offset_convs(monkeypatch):
    """1x5x3x180x320: exactly L1_offset_conv1, L2_offset_conv1 and cas_offset_conv1 report two launches in the no-grad slot
    (L3_offset_conv1, 45x80, is on the K-split kernel), every op one in the grad slot; names, tags and the algorithmic figures
    are those of the plan without the hoist, the arena grows by the three addend tensors alone and the issued work drops by
    the four fifths of the reference halves that are no longer multiplied."""
    from dynavsr_amd import engine, _lib as L
    torch.cuda.current_device()
    plan = engine.Plan(CFG, 1, 180, 320)
    names, cnt = launch_counts(plan, True)
    assert len(names) == plan.n_launches
    assert sorted(n for n, c in zip(names, cnt) if c != 1) == sorted(HOISTED) and all(c in (1, 2) for c in cnt)
    assert all(c == 1 for c in launch_counts(plan, False)[1])
    assert L.lib().dvsr_edvr_op_launch_count(plan._h, plan.n_launches, 1) == -1 and L.lib().dvsr_edvr_op_launch_count(plan._h, -1, 1) == -1
    monkeypatch.setenv("DVSR_PCD_HOIST", "0")
    off = engine.Plan(CFG, 1, 180, 320)
    assert all(c == 1 for c in launch_counts(off, True)[1])
    assert plan.op_info() == off.op_info()
    scratch = 4 * 64 * (2 * 180 * 320 + 90 * 160)                 # one image of 64 channels per split op, fp32
    assert plan.workspace_bytes(False) - off.workspace_bytes(False) == scratch
    won, woff = plan.work(nograd=True), off.work(nograd=True)
    assert won["fwd_algorithmic"] == woff["fwd_algorithmic"] and plan.work() == off.work()
    saved = 0.25 * 2.0 * 64 * 64 * 9 * (2 * 180 * 320 + 90 * 160) * 4     # F(4x4): a quarter of the multiplies; 4 of 5 frames
    assert abs((woff["fwd_executed"] - won["fwd_executed"]) - saved) < 1e-6 * saved


@pytest.mark.parametrize("b,h,w", [(1, 64, 96), (2, 32, 48)])
def test_small_plans_split_nothing(b, h, w):
    assert split_ops(b, h, w) == []


_CHILD = r"""
import json, sys, torch
from dynavsr_amd import engine, synth, _lib as L
from dynavsr_amd.models.archs.EDVR_arch import EDVR
net = EDVR(); net.load_state_dict(synth.edvr_state_dict(0), strict=True); net = net.cuda()
x = synth.clip(77, 1, 5, 180, 320).cuda()
net._debug_ws = []
with torch.no_grad():
    y = net(x)
plan, ws = net._debug_ws[-1]
out = torch.full_like(y, float("nan"))
ws2 = torch.empty(plan.workspace_bytes(False), dtype=torch.uint8, device="cuda")
plan.forward_timed([p.detach() for p in net.ordered_parameters()], x, out, ws2)
cnt = [L.lib().dvsr_edvr_op_launch_count(plan._h, i, 1) for i in range(plan.n_launches)]
print(json.dumps(dict(equal=bool(torch.equal(out, y)), finite=bool(torch.isfinite(y).all()), counts=cnt,
                      tags=[nm for (_k, nm, _f, _b) in plan.op_info()])))
"""


def test_switch_off_keeps_one_launch_per_op_in_a_fresh_process():
    """DVSR_PCD_HOIST=0 in a child process: the 180x320 no-grad forward runs one launch per op and gives the bits of
    dvsr_edvr_forward_timed in the same child; its tags are this process's (the switch moves no tag)."""
    from dynavsr_amd import engine
    env = dict(os.environ, DVSR_PCD_HOIST="0")
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["equal"] and got["finite"] and set(got["counts"]) == {1}
    torch.cuda.current_device()
    tags = [nm for (_k, nm, _f, _b) in engine.Plan(CFG, 1, 180, 320).op_info()]
    assert got["tags"] == tags and len(got["counts"]) == len(tags)


# ---- 3. the network -----------------------------------------------------------------------------------------------------
H, W = 44, 288


def make_net(seed=0):
    from dynavsr_amd.models.archs.EDVR_arch import EDVR
    net = EDVR()
    net.load_state_dict(synth.edvr_state_dict(seed), strict=True)
    return net.cuda()


@pytest.fixture(scope="module")
def hoisted():
    """One clip at H x W through the no-grad forward (split offset convs), the grad-mode forward (one launch each, training
    geometries) of the same network and the CPU oracle; computed once."""
    from oracle import edvr as oedvr
    net = make_net(0)
    x = synth.clip(1, 1, 5, H, W, smooth=False)
    xg = x.cuda()
    names = {"L1_offset_conv1": (5, 64, H, W), "cas_offset_conv1": (5, 64, H, W)}
    net._debug_ws = []
    with torch.no_grad():
        y_ng = net(xg)
    plan, ws = net._debug_ws[-1]
    assert ws.numel() == plan.workspace_bytes(False) < plan.workspace_bytes(True)
    t_ng = {k: plan.tensor(ws, k, s).clone() for k, s in names.items()}
    y_rec = net(xg)
    plan_r, ws_r = net._debug_ws[-1]
    assert y_rec.requires_grad and ws_r.numel() == plan.workspace_bytes(True)
    t_rec = {k: plan_r.tensor(ws_r, k, s).clone() for k, s in names.items()}
    with torch.no_grad():
        yo = oedvr.edvr_forward(synth.edvr_state_dict(0), x)
    return dict(net=net, x=xg, plan=plan, y_ng=y_ng.detach(), y_rec=y_rec.detach(), t_ng=t_ng, t_rec=t_rec, yo=yo)


def test_smallest_hoisting_clip(hoisted):
    """1x5x3x44x288 is the smallest clip (fewest pixels) at which the default plan applies the hoist, found with
    dvsr_edvr_op_launch_count over H = 16 .. 180 in steps of 4 and W = 64 .. 320 in steps of 32 (the narrower F(4x4) workgroup
    tile): the smallest H with a split is 44 at W = 288 and 320, 52 at 256, 60 at 224, 72 at 192, 84 at 160, 104 at 128, 140
    at 96, none at 64 -- below that the five-frame layers are on the K-split kernel (fewer than 700 workgroups of the 4x32x32
    geometry), and the split needs its op on the F(4x4) kernel.  There L1_offset_conv1 and cas_offset_conv1 split
    (L2_offset_conv1, 22x144, is on the K-split kernel; at 180x320 it splits too); H % 8 == 4, so the last F(4x4) tile row is
    cut.  Four rows less, or the next narrower width at fewer pixels, and nothing splits."""
    names, cnt = launch_counts(hoisted["plan"], True)
    assert [n for n, c in zip(names, cnt) if c == 2] == ["L1_offset_conv1", "cas_offset_conv1"]
    assert split_ops(1, H - 4, W) == [] and split_ops(1, 48, 256) == []


def test_split_layers_match_the_grad_mode_forward(hoisted):
    """No-grad forward (offset convs as reference + main part) against the grad-mode forward of the same network (one launch,
    training geometries): the two split tensors and the output to the 5e-6 relative L2 of test_flipped_layers_match_..."""
    errs = {k: relerr(hoisted["t_ng"][k], hoisted["t_rec"][k]) for k in hoisted["t_ng"]}
    errs["out"] = relerr(hoisted["y_ng"], hoisted["y_rec"])
    print("no-grad vs grad-mode forward, rel L2:", errs)
    assert all(e < 5e-6 for e in errs.values()), errs


def test_hoisted_forward_against_the_oracle(hoisted):
    """The bounds of test_flipped_forward_against_the_oracle."""
    y, yo = hoisted["y_ng"].cpu(), hoisted["yo"]
    assert y.shape == (1, 3, 4 * H, 4 * W)
    d = (y - yo).abs()
    print("vs oracle: max-abs %.3e rel L2 %.3e" % (float(d.max()), relerr(y, yo)))
    assert float(d.max()) <= 1e-3, float(d.max())
    assert relerr(y, yo) < 2e-4
    assert 10 * np.log10(1.0 / float(((y - yo) ** 2).mean())) >= 60.0


def test_two_batched_clips_give_the_bits_of_single_ones(hoisted):
    """B = 2: the decision is read off one clip's grids, so both clips of a batch run what a single clip runs."""
    net, x = hoisted["net"], hoisted["x"]
    x2 = synth.clip(2, 1, 5, H, W, smooth=False).cuda()
    assert sorted(split_ops(2, H, W)) == ["L1_offset_conv1", "cas_offset_conv1"]
    with torch.no_grad():
        yb = net(torch.cat([x, x2], 0))
        y2 = net(x2)
    assert torch.equal(yb[0:1], hoisted["y_ng"]) and torch.equal(yb[1:2], y2)


def test_two_clips_in_flight_give_the_bits_of_one(hoisted):
    """adapt.super_resolve_video(in_flight=2): every stream's plan makes the same choice and owns its addend tensors."""
    from dynavsr_amd.adapt import super_resolve_video
    net, x = hoisted["net"], hoisted["x"]
    out = [y_.clone() for y_ in super_resolve_video({"network_G": {"which_model_G": "EDVR"}}, net, [x] * 4, in_flight=2)]
    assert len(out) == 4 and all(torch.equal(o, hoisted["y_ng"]) for o in out)
