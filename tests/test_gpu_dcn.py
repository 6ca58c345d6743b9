"""Modulated deformable convolution at the C ABI: every shipped kernel variant against the fp64 CPU oracle.

tests/test_gpu_ops.py holds the DCN at EDVR's configuration with random offsets.  This file covers what stays reachable
beside it: the three-kernel backward at other strides / paddings / dilations / channel counts, the (-1,H) x (-1,W)
sampling gate on the kernels EDVR runs (LDS-window forward kernels, fused backward), the NULL / accumulating arguments
the header allows, partial and odd tile counts, the kernels behind DVSR_DCN_FWD / DVSR_DCN_BWD, and the drop-in modules
with stride / dilation.

Every call goes through dynavsr_amd._lib directly: outputs the header calls "overwritten" and the workspace are filled
with NaN first and must come back finite, so a kernel that skips a tile (or reads scratch it never wrote) cannot pass on
what an earlier call left in the allocator's buffer.

Reference: oracle.dcn (C, fp64) on the fp32-rounded inputs; inside each case the independent gather formulation under
autograd must agree with it to 1e-11 (what oracle/gen_golden.py asks before it writes a golden).  Bar: the TOL = 2e-5
relative L2 of tests/test_gpu_ops.py (exact fp32 products, fp32 round-off only; the plain fp32 C oracle lies 8e-8 to 8e-7
from the fp64 one on these cases).  Each test prints the errors it saw.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import relerr

pytestmark = pytest.mark.gpu

TOL = 2e-5
GRADS = ("gx", "goffset", "gmask", "gw", "gb")

# n, c, dg, cout, h, w, stride, pad, dil
GENERAL = [
    (2, 16, 4, 12, 11, 13, 2, 1, 1),    # C/dg = 4, stride 2 -> 6x7
    (1, 16, 2, 8, 10, 10, 1, 2, 2),     # C/dg = 8, but dilation 2
    (1, 32, 8, 40, 9, 14, 2, 0, 1),     # pad 0 -> 4x6
    (2, 64, 8, 64, 9, 12, 2, 2, 2),     # EDVR's channels, stride 2 and dilation 2 -> 5x6
    (1, 64, 16, 24, 7, 10, 1, 0, 1),    # C*9 = 576 over 32-channel chunks; Cout < 32
    (1, 64, 8, 80, 9, 33, 1, 1, 1),     # EDVR geometry kept off the fused kernel by Cout
    (1, 32, 2, 16, 8, 12, 1, 1, 1),     # C/dg = 16
]
# n, c, dg, cout, h, w (stride = pad = dil = 1)
FUSED = [
    (1, 64, 8, 64, 3, 5),               # one partial tile: seven of the eight interleaved workgroup slots idle
    (1, 64, 8, 64, 1, 4),
    (3, 64, 8, 64, 8, 32),              # three full tiles: not a multiple of 8
    (1, 64, 8, 128, 12, 36),            # C/dg = 8 with Cout = 128
    (1, 128, 8, 64, 12, 36),            # C/dg = 16, Cout = 64, W % 4 == 0: two chunks per group on the bf16 3-way split
    (1, 128, 8, 64, 9, 33),             # the same on the fp32 MFMAs
]
FUSED_VARIANTS = (1, 64, 8, 64, 12, 36)
GATE = [(1, 64, 8, 64, 10, 36), (1, 64, 8, 64, 10, 35)]


def _id(case):
    return "-".join(str(v) for v in case)


def _out_hw(h, w, stride, pad, dil):
    return (h + 2 * pad - (2 * dil + 1)) // stride + 1, (w + 2 * pad - (2 * dil + 1)) // stride + 1


def dev(t):
    return t.float().contiguous().cuda()


def nan_like_shape(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def nan_bytes(nbytes):
    # 0xFF bytes read as NaN both as fp32 and as bf16
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device="cuda")


@functools.lru_cache(maxsize=None)
def make_case(n, c, dg, cout, h, w, stride, pad, dil, gate=False):
    """Inputs (fp64 tensors holding fp32-representable values) and the fp64 reference of one case: computed once, shared
    by the tests that need it, never modified."""
    from oracle import dcn as odcn
    ho, wo = _out_hw(h, w, stride, pad, dil)
    r = np.random.RandomState(1000 * h + 10 * w + c + cout + stride + 3 * dil)
    x = torch.from_numpy(r.standard_normal((n, c, h, w)))
    off = torch.from_numpy(r.standard_normal((n, dg * 18, ho, wo)) * 2.0)
    off[:, :, 0, :] = torch.round(off[:, :, 0, :])       # the first output row samples exactly integer positions
    if gate:                                             # oracle/gen_golden.py, case "b", plus two more exact boundaries
        assert (stride, pad, dil) == (1, 1, 1) and dg == 8
        o = off.view(n, dg, 9, 2, h, w)
        o[0, 0, :, :, 0, :] = 0.0                        # integer sampling positions
        o[0, 1, :, 0, 1, :] = -1.0 + 1e-3                # just inside the top gate at row 1 / tap 0
        o[0, 1, 0, 0, 0, :] = -1e-3                      # h_im = -1 - 1e-3 -> outside
        o[0, 2, :, 0, h - 1, :] = 1.0 - 1e-3             # h_im = H - 1e-3 at the bottom row, tap 1
        o[0, 3, :, :, 3, :] = 50.0                       # far outside
        o[0, 4, :, :, 4, :] = -50.0
        o[0, 5, 4, 0, 0, :] = -1.0                       # centre tap on row 0 -> h_im == -1 exactly
        o[0, 5, 4, 1, :, w - 1] = 1.0                    # w_im == W exactly
        o[0, 6, 4, 1, :, 0] = -1.0                       # w_im == -1 exactly
        o[0, 7, 4, 0, h - 1, :] = 1.0                    # h_im == H exactly
    m = torch.from_numpy(r.random_sample((n, dg * 9, ho, wo)))
    wt = torch.from_numpy(r.standard_normal((cout, c, 3, 3)) / np.sqrt(9.0 * c))
    b = torch.from_numpy(r.standard_normal(cout) * 0.1)
    go = torch.from_numpy(r.standard_normal((n, cout, ho, wo)))
    x, off, m, wt, b, go = (t.float().double() for t in (x, off, m, wt, b, go))
    cfg = (stride, pad, dil, 1, dg)
    out = odcn.forward(x, off, m, wt, b, *cfg)
    grads = odcn.backward(x, off, m, wt, True, go, *cfg)
    # the two CPU formulations (C loops / index gathers under autograd: no shared code) must agree first
    leaves = [t.clone().requires_grad_(True) for t in (x, off, m, wt, b)]
    out2 = odcn.gather_reference(*leaves, *cfg)
    grads2 = torch.autograd.grad(out2, leaves, go)
    agree = [relerr(out, out2)] + [relerr(a, b_) for a, b_ in zip(grads, grads2)]
    assert max(agree) < 1e-11, ("the CPU oracles disagree", agree)
    # the pack form reads mask logits: the reference is the oracle on the sigmoid of the logits as rounded to fp32
    lg = torch.logit(m).float().double()
    assert bool(torch.isfinite(lg).all())
    out_pack = odcn.forward(x, off, torch.sigmoid(lg), wt, b, *cfg)
    return dict(shape=(n, c, dg, cout, h, w, stride, pad, dil), ho=ho, wo=wo, x=x, off=off, m=m, wt=wt, b=b, go=go,
                lg=lg, out=out, out_pack=out_pack, grads=dict(zip(GRADS, grads)))


def _finite(name, t):
    assert bool(torch.isfinite(t).all()), "%s: %d non-finite values (an element the kernel never wrote, or scratch it read " \
        "before writing)" % (name, int((~torch.isfinite(t)).sum()))


def gpu_forward(cs, kind, finite=True):
    """kind: 'plain' = dvsr_mdcn_forward, 'pack' = dvsr_mdcn_pack_forward on cat(offset, logit(mask)) (both: the generic
    gather kernel, fp32 MFMAs, any geometry), 'fast' = dvsr_mdcn_forward_fast, 'packfast' = dvsr_mdcn_pack_forward_fast on
    the same cat(offset, logit(mask)) (stride = pad = dil = 1 only: the LDS-window kernels the engine runs -- the split kernel
    on aligned W % 4 == 0, reading masks / mask logits).  The output starts as NaN and must come back finite
    (finite=False: the caller feeds non-finite inputs and checks where the output is finite itself)."""
    from dynavsr_amd import _lib as L
    n, c, dg, cout, h, w, stride, pad, dil = cs["shape"]
    x, wt, b = dev(cs["x"]), dev(cs["wt"]), dev(cs["b"])
    out = nan_like_shape(n, cout, cs["ho"], cs["wo"])
    if kind == "plain":
        off, m = dev(cs["off"]), dev(cs["m"])
        L.check(L.lib().dvsr_mdcn_forward(L.ptr(x), L.ptr(off), L.ptr(m), L.ptr(wt), L.ptr(b), L.ptr(out), n, c, h, w,
                                          cout, 3, 3, stride, pad, dil, 1, dg, L.ACT_NONE, L.stream()),
                "dvsr_mdcn_forward")
    elif kind == "pack":
        om = dev(torch.cat([cs["off"], cs["lg"]], 1))
        L.check(L.lib().dvsr_mdcn_pack_forward(L.ptr(x), L.ptr(om), L.ptr(wt), L.ptr(b), L.ptr(out), n, c, h, w, cout,
                                               3, 3, stride, pad, dil, 1, dg, L.ACT_NONE, L.stream()),
                "dvsr_mdcn_pack_forward")
    elif kind == "packfast":
        assert (stride, pad, dil) == (1, 1, 1)
        om = dev(torch.cat([cs["off"], cs["lg"]], 1))
        nbytes = int(L.lib().dvsr_mdcn_forward_fast_workspace_bytes(c, cout, dg))
        ws = nan_bytes(nbytes)
        L.check(L.lib().dvsr_mdcn_pack_forward_fast(L.ptr(x), L.ptr(om), L.ptr(wt), L.ptr(b), L.ptr(out), n, c, h, w,
                                                    cout, dg, L.ACT_NONE, ws.data_ptr(), nbytes, L.stream()),
                "dvsr_mdcn_pack_forward_fast")
    else:
        assert kind == "fast" and (stride, pad, dil) == (1, 1, 1)
        off, m = dev(cs["off"]), dev(cs["m"])
        nbytes = int(L.lib().dvsr_mdcn_forward_fast_workspace_bytes(c, cout, dg))
        ws = nan_bytes(nbytes)
        L.check(L.lib().dvsr_mdcn_forward_fast(L.ptr(x), L.ptr(off), L.ptr(m), L.ptr(wt), L.ptr(b), L.ptr(out), n, c,
                                               h, w, cout, dg, L.ACT_NONE, ws.data_ptr(), nbytes, L.stream()),
                "dvsr_mdcn_forward_fast")
    torch.cuda.synchronize()
    if finite:
        _finite("out (%s)" % kind, out)
    return out


def gpu_backward(cs, want_gx=True, want_gw=True, want_gb=True, gx_init=None, finite=True):
    """dvsr_mdcn_backward with NaN in goffset / gmask / gw / gb and in the workspace; gx starts as zeros (or gx_init: the
    op accumulates into it).  Returns a dict of the outputs that were asked for; all of them must be finite (finite=False:
    the caller feeds non-finite inputs and checks where the outputs are finite itself)."""
    from dynavsr_amd import _lib as L
    n, c, dg, cout, h, w, stride, pad, dil = cs["shape"]
    x, off, m, wt, go = (dev(cs[k]) for k in ("x", "off", "m", "wt", "go"))
    nbytes = int(L.lib().dvsr_mdcn_backward_workspace_bytes(n, c, h, w, cout, 3, 3, stride, pad, dil))
    ws = nan_bytes(nbytes)
    gx = None
    if want_gx:
        gx = torch.zeros_like(x) if gx_init is None else gx_init.clone()
    goff, gm = nan_like_shape(*off.shape), nan_like_shape(*m.shape)
    gw = nan_like_shape(*wt.shape) if want_gw else None
    gb = nan_like_shape(cout) if want_gb else None
    L.check(L.lib().dvsr_mdcn_backward(L.ptr(x), L.ptr(off), L.ptr(m), L.ptr(wt), L.ptr(go), L.ptr(gx), L.ptr(goff),
                                       L.ptr(gm), L.ptr(gw), L.ptr(gb), n, c, h, w, cout, 3, 3, stride, pad, dil, 1, dg,
                                       ws.data_ptr(), nbytes, L.stream()), "dvsr_mdcn_backward")
    torch.cuda.synchronize()
    got = {k: v for k, v in zip(GRADS, (gx, goff, gm, gw, gb)) if v is not None}
    if finite:
        for k, v in got.items():
            _finite(k, v)
    return got


def check(tag, got, ref):
    """Every tensor of `got` against the entry of the same name in `ref`: prints all errors, then asserts the bar."""
    errs = {k: relerr(v, ref[k]) for k, v in got.items()}
    print("[dcn] %s: %s" % (tag, "  ".join("%s %.2e" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e < TOL, (tag, k, e)
    return errs


def check_forwards(tag, cs, kinds):
    ref = {"plain": cs["out"], "fast": cs["out"], "pack": cs["out_pack"], "packfast": cs["out_pack"]}
    check(tag, {k: gpu_forward(cs, k) for k in kinds}, ref)


def check_argument_variants(tag, cs):
    """The arguments the header allows beside the all-pointers call: gx = NULL, gw = gb = NULL, gb = NULL alone, and a gx
    that already holds values (the op accumulates).  Whatever is still asked for must meet the bar."""
    ref = cs["grads"]
    got = gpu_backward(cs, want_gx=False)
    assert set(got) == {"goffset", "gmask", "gw", "gb"}
    check(tag + " gx=NULL", got, ref)
    got = gpu_backward(cs, want_gw=False, want_gb=False)
    assert set(got) == {"gx", "goffset", "gmask"}
    check(tag + " gw=gb=NULL", got, ref)
    got = gpu_backward(cs, want_gb=False)
    assert set(got) == {"gx", "goffset", "gmask", "gw"}
    check(tag + " gb=NULL", got, ref)
    r = torch.from_numpy(np.random.RandomState(77).standard_normal(tuple(cs["x"].shape))).float().cuda()
    got = gpu_backward(cs, gx_init=r)
    got["gx"] = got["gx"].double() - r.double()
    check(tag + " gx+=", got, ref)


# ---- 1. the three-kernel backward (and the generic forward) away from stride = pad = dilation = 1 ---------------------
@pytest.mark.parametrize("case", GENERAL, ids=_id)
def test_general_backward(case):
    cs = make_case(*case)
    tag = "general " + _id(case)
    check(tag + " bwd", gpu_backward(cs), cs["grads"])
    check_forwards(tag + " fwd", cs, ("plain", "pack"))


def test_general_backward_argument_variants():
    check_argument_variants("general " + _id(GENERAL[1]), make_case(*GENERAL[1]))


# ---- 2. the fused backward: partial tiles, odd tile counts, two chunks per group, Cout = 128 --------------------------
@pytest.mark.parametrize("case", FUSED, ids=_id)
def test_fused_backward(case):
    cs = make_case(*case, 1, 1, 1)
    check("fused " + _id(case) + " bwd", gpu_backward(cs), cs["grads"])


def test_fused_backward_argument_variants():
    check_argument_variants("fused " + _id(FUSED_VARIANTS), make_case(*FUSED_VARIANTS, 1, 1, 1))


# ---- 3. the (-1,H) x (-1,W) gate on the kernels EDVR runs --------------------------------------------------------------
def _boundary_groups(t_off, t_msk, cs):
    """goffset / gmask at the four hand-placed exact boundaries (centre tap of groups 5, 5, 6, 7), as flat tensors."""
    n, c, dg, cout, h, w = cs["shape"][:6]
    o, k = t_off.reshape(n, dg, 9, 2, h, w), t_msk.reshape(n, dg, 9, h, w)
    return {"h_im == -1": (o[0, 5, 4, :, 0, :], k[0, 5, 4, 0, :]),
            "w_im == W": (o[0, 5, 4, :, :, w - 1], k[0, 5, 4, :, w - 1]),
            "w_im == -1": (o[0, 6, 4, :, :, 0], k[0, 6, 4, :, 0]),
            "h_im == H": (o[0, 7, 4, :, h - 1, :], k[0, 7, 4, h - 1, :])}


@pytest.mark.parametrize("case", GATE, ids=_id)
def test_gate_backward(case):
    """Samples exactly on -1 and on H / W are outside: the reference returns 0 for their offset and mask gradients.  The
    zero padding of an LDS window gives the sample VALUE of the gate for free, but not the coordinate gradient at exactly
    -1 (the padded image's slope towards row / column 0 is not zero), so the kernels need an explicit test there."""
    cs = make_case(*case, 1, 1, 1, gate=True)
    ref = cs["grads"]
    for where, (ro, rm) in _boundary_groups(ref["goffset"], ref["gmask"], cs).items():
        assert float(ro.abs().max()) == 0.0 and float(rm.abs().max()) == 0.0, "oracle not 0 at " + where
    x = cs["x"]
    # an ungated kernel would differ: the rows / columns next to the boundary hold values
    assert float(x[0, 40:64, 0, :].abs().min()) > 0 and float(x[0, 40:64, :, 0].abs().min()) > 0
    got = gpu_backward(cs)
    check("gate " + _id(case) + " bwd", got, ref)
    for where, (go_, gm_) in _boundary_groups(got["goffset"], got["gmask"], cs).items():
        assert float(go_.abs().max()) == 0.0, ("goffset must be exactly 0 where " + where, float(go_.abs().max()))
        assert float(gm_.abs().max()) == 0.0, ("gmask must be exactly 0 where " + where, float(gm_.abs().max()))


@pytest.mark.parametrize("case", GATE, ids=_id)
def test_gate_forward(case):
    """The same inputs through the four forward entries; dvsr_mdcn_forward_fast and dvsr_mdcn_pack_forward_fast take the split
    kernel at W = 36 and the register-staged one at W = 35 (DVSR_DCN_FWD=dma / reg move W = 36 to the other two kernels, see
    below)."""
    cs = make_case(*case, 1, 1, 1, gate=True)
    check_forwards("gate " + _id(case) + " fwd", cs, ("plain", "fast", "pack", "packfast"))


# ---- 4. kernels behind process-wide switches (read once per process: each in a fresh child) ---------------------------
def _child(env, kexpr):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-k", kexpr],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    sys.stdout.write("".join("%s (child %s)\n" % (l[l.index("[dcn]"):], ",".join(env.values()))
                             for l in r.stdout.splitlines() if "[dcn]" in l))
    assert r.returncode == 0, "child %s exited with %d\n%s%s" % (env, r.returncode, r.stdout[-3000:], r.stderr[-1500:])
    assert " passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-1000:]


def test_switch_forward_dma():
    """mdcn_fwd_dma_kernel (fp32 MFMAs, DMA-staged window) takes the aligned shape of the gate cases."""
    _child({"DVSR_DCN_FWD": "dma"}, "test_gate_forward")


def test_switch_forward_reg():
    """mdcn_fwd_reg_kernel on aligned input as well as on W % 4 != 0."""
    _child({"DVSR_DCN_FWD": "reg"}, "test_gate_forward")


def test_switch_backward_unfused():
    """The three-kernel backward at EDVR's shapes, argument variants and gate included."""
    _child({"DVSR_DCN_BWD": "unfused"}, "test_fused_backward or test_gate_")


# ---- 5. the drop-in autograd surface with stride / dilation ------------------------------------------------------------
def _rs(seed, *shape, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape) * scale).float()


def _check_module(tag, y, yr, pairs):
    errs = {"out": relerr(y, yr)}
    errs.update({k: relerr(a, b) for k, (a, b) in pairs.items()})
    print("[dcn] %s: %s" % (tag, "  ".join("%s %.2e" % kv for kv in errs.items())))
    assert errs.pop("out") < 2e-5
    for k, e in errs.items():
        assert e < 1e-4, (tag, k, e)


def test_dropin_pack_stride2():
    from dynavsr_amd.models.archs.dcn import ModulatedDeformConvPack
    from oracle import dcn as odcn
    mod = ModulatedDeformConvPack(64, 64, 3, stride=2, padding=1, deformable_groups=8)
    with torch.no_grad():
        mod.weight.copy_(_rs(1, 64, 64, 3, 3, scale=1 / 24.0))
        mod.bias.copy_(_rs(2, 64, scale=0.1))
        mod.conv_offset_mask.weight.copy_(_rs(3, 216, 64, 3, 3, scale=0.05))
        mod.conv_offset_mask.bias.copy_(_rs(4, 216, scale=0.05))
    mod = mod.cuda()
    x0 = _rs(5, 2, 64, 11, 14)
    x = x0.cuda().requires_grad_()
    y = mod(x)
    assert tuple(y.shape) == (2, 64, 6, 7)
    go = _rs(6, *y.shape)
    y.backward(go.cuda())
    P = {k: v.detach().cpu().double().requires_grad_() for k, v in mod.named_parameters()}
    xc = x0.double().requires_grad_()
    om = F.conv2d(xc, P["conv_offset_mask.weight"], P["conv_offset_mask.bias"], 2, 1)
    yr = odcn.modulated_deform_conv(xc, om[:, :144].contiguous(), torch.sigmoid(om[:, 144:]).contiguous(), P["weight"],
                                    P["bias"], 2, 1, 1, 1, 8)
    yr.backward(go.double())
    pairs = {"x": (x.grad, xc.grad)}
    pairs.update({k: (v.grad, P[k].grad) for k, v in mod.named_parameters()})
    _check_module("dropin pack 64-64 s2 p1", y, yr, pairs)


def test_dropin_module_dilation2():
    from dynavsr_amd.models.archs.dcn import ModulatedDeformConv
    from oracle import dcn as odcn
    mod = ModulatedDeformConv(16, 8, 3, stride=1, padding=2, dilation=2, deformable_groups=2)
    with torch.no_grad():
        mod.weight.copy_(_rs(1, 8, 16, 3, 3, scale=1 / 12.0))
        mod.bias.copy_(_rs(2, 8, scale=0.1))
    mod = mod.cuda()
    h, w = 9, 11
    x0, off0 = _rs(3, 2, 16, h, w), _rs(4, 2, 36, h, w, scale=2.0)
    m0 = torch.from_numpy(np.random.RandomState(5).random_sample((2, 18, h, w))).float()
    leaves = [t.cuda().requires_grad_() for t in (x0, off0, m0)]
    y = mod(*leaves)
    assert tuple(y.shape) == (2, 8, h, w)
    go = _rs(6, *y.shape)
    y.backward(go.cuda())
    P = {k: v.detach().cpu().double().requires_grad_() for k, v in mod.named_parameters()}
    cl = [t.double().requires_grad_() for t in (x0, off0, m0)]
    yr = odcn.modulated_deform_conv(*cl, P["weight"], P["bias"], 1, 2, 2, 1, 2)
    yr.backward(go.double())
    pairs = {k: (a.grad, b.grad) for k, a, b in zip(("x", "offset", "mask"), leaves, cl)}
    pairs.update({k: (v.grad, P[k].grad) for k, v in mod.named_parameters()})
    _check_module("dropin 16-8 p2 d2", y, yr, pairs)
