"""The two DCN kernels on the bf16 pipe -- mdcn_fwd_split_kernel (the default forward) and the SPLIT instantiation of
mdcn_bwd_fused_kernel -- on the domain DESIGN 3.3 states for every kernel under the exact 3-way split: per-channel scales over
ten decades, operand magnitudes 2^+-100 inside the domain and 2^-116 .. 2^-124 below it, one inf / NaN element, and mask logits
over a wide range.  The other DCN files draw everything from N(0,1) and judge one rel-L2 per tensor; here errors are taken per
channel, after undoing the scale (compared at O(1): conftest.relerr guards its denominator with 1e-30), and the non-finite
tests compare SETS of elements.

Shapes (n, c, dg, cout, h, w; stride = pad = dilation = 1), the smallest that reach the kernels in question:
  S  = (1, 64, 8, 64, 12, 36)   forward_fast / pack_forward_fast -> split forward kernel (reading masks / mask logits),
                                backward -> fused SPLIT kernel; two tile rows and a partial tile column
  S2 = (1, 128, 8, 64, 12, 36)  two 8-channel chunks per deformable group: atomic goffset / gmask, forward sub = 2
  F  = S with w = 35            the same entries on the fp32 MFMAs (register-staged forward): the in-process control
Forward kinds (test_gpu_dcn.gpu_forward): 'fast' and 'packfast' are the kernels under test; 'plain' (dvsr_mdcn_forward) and
'pack' (dvsr_mdcn_pack_forward) run the generic fp32 gather kernel on every shape -- measured here: 'pack' tracks 'plain' to
the digit below the domain and returns +-inf where the split returns NaN -- and are the fp32 controls of the forward on S.

Inputs (one cached builder): x, gout ~ N(0,1), w ~ N(0, 1/(9c)), b ~ 0.1 N(0,1), masks 0.25 + 0.75 U[0,1) (a tiny mask would push
blended values out of the domain on its own), offsets round(2 N(0,1) * 64) / 64 + 1/128: every sampling coordinate is exact in
fp32 and at least 2^-7 from an integer (asserted), so no gate or floor decision differs between fp32 and fp64 and no corner has
weight 0.  Output row 3 has +50 on all offsets: one row through the global fix-up path of both kernels.  Offsets and masks stay
finite throughout: every address is one the other DCN tests already produce.

Reference: oracle.dcn (C, fp64) on the fp32-rounded inputs.  Bar: TOL = 2e-5 of the DCN files, except
  * the fixed-point bound of test 1c (derived from the inputs, see there), and
  * the magnitudes below the domain (SUB_BARS: measured, then the next "nice" value >= 3x above, the margin of round 5).
Every test prints the errors it measured ("[dcn] ...").
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_dcn import GRADS, TOL, dev, gpu_backward, gpu_forward, nan_bytes, nan_like_shape, relerr  # noqa: F401

pytestmark = pytest.mark.gpu

S = (1, 64, 8, 64, 12, 36)
S2 = (1, 128, 8, 64, 12, 36)
F = (1, 64, 8, 64, 12, 35)
NAMES = {S: "S", S2: "S2", F: "F"}
CFG = (1, 1, 1, 1)  # stride, pad, dil, groups
KINDS = ("fast", "packfast", "pack", "plain")
PACKED = ("pack", "packfast")   # read mask logits: the reference is the oracle on sigmoid(fp32 logits)


# ---- inputs and references ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base(shape):
    """The shared inputs of one shape: fp64 tensors holding fp32-representable values; never modified (the tests copy)."""
    from oracle import dcn as odcn
    n, c, dg, cout, h, w = shape
    r = np.random.RandomState(7 * c + w)
    x = torch.from_numpy(r.standard_normal((n, c, h, w)))
    off = torch.from_numpy(np.round(r.standard_normal((n, dg * 18, h, w)) * 2.0 * 64.0) / 64.0 + 1.0 / 128.0)
    off[:, :, 3, :] += 50.0
    m = torch.from_numpy(0.25 + 0.75 * r.random_sample((n, dg * 9, h, w)))
    wt = torch.from_numpy(r.standard_normal((cout, c, 3, 3)) / np.sqrt(9.0 * c))
    b = torch.from_numpy(r.standard_normal(cout) * 0.1)
    go = torch.from_numpy(r.standard_normal((n, cout, h, w)))
    assert torch.equal(off.float().double(), off)
    x, m, wt, b, go = (t.float().double() for t in (x, m, wt, b, go))
    # the sampling coordinates: exact in fp32, never an integer, 2^-7 or more away from one
    py, px = _coords(off, n, dg, h, w)
    for t in (py, px):
        assert torch.equal(t.float().double(), t)
        assert float((t - torch.round(t)).abs().min()) >= 2.0 ** -7
    lg = torch.logit(m).float().double()
    cs = dict(shape=shape + (1, 1, 1), ho=h, wo=w, x=x, off=off, m=m, wt=wt, b=b, go=go, lg=lg)
    # the two CPU formulations (C loops / index gathers under autograd: no shared code) agree on these inputs
    leaves = [t.clone().requires_grad_(True) for t in (x, off, m, wt, b)]
    out2 = odcn.gather_reference(*leaves, *CFG, dg)
    grads2 = torch.autograd.grad(out2, leaves, go)
    agree = [relerr(ref_forward(cs), out2)] + [relerr(a, b_) for a, b_ in zip(ref_backward(cs).values(), grads2)]
    assert max(agree) < 1e-11, ("the CPU oracles disagree", agree)
    return cs


def _coords(off, n, dg, h, w):
    o = off.view(n, dg, 9, 2, h, w)
    ki = (torch.arange(9) // 3).view(1, 1, 9, 1, 1).double()
    kj = (torch.arange(9) % 3).view(1, 1, 9, 1, 1).double()
    ys = torch.arange(h).view(1, 1, 1, h, 1).double()
    xs = torch.arange(w).view(1, 1, 1, 1, w).double()
    return ys - 1.0 + ki + o[:, :, :, 0], xs - 1.0 + kj + o[:, :, :, 1]


def case(shape, **over):
    cs = dict(base(shape))
    cs.update(over)
    return cs


def r32(t):
    """Round to fp32, keep as fp64: what the kernels are given."""
    return t.float().double()


def ref_forward(cs, pack=False):
    from oracle import dcn as odcn
    m = torch.sigmoid(cs["lg"]) if pack else cs["m"]
    return odcn.forward(cs["x"], cs["off"], m, cs["wt"], cs["b"], *CFG, cs["shape"][2])


def ref_backward(cs):
    from oracle import dcn as odcn
    return dict(zip(GRADS, odcn.backward(cs["x"], cs["off"], cs["m"], cs["wt"], True, cs["go"], *CFG, cs["shape"][2])))


def chan_err(got, ref, dim, scale=None):
    """rel-L2 per index of `dim`, after multiplying that index's slice by scale[index] (both sides: at O(1))."""
    g = torch.as_tensor(got).detach().double().cpu().movedim(dim, 0)
    r = ref.movedim(dim, 0)
    g, r = g.reshape(g.shape[0], -1), r.reshape(r.shape[0], -1)
    if scale is not None:
        g, r = g * scale.view(-1, 1), r * scale.view(-1, 1)
    return (g - r).norm(dim=1) / (r.norm(dim=1) + 1e-30)


def all_finite(tag, got):
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (tag, k, "%d non-finite values" % int((~torch.isfinite(v)).sum()))


def report(tag, errs, bars=None):
    """Prints every error, then asserts each against TOL (or its entry in bars)."""
    print("[dcn] %s: %s" % (tag, "  ".join("%s %.2e" % kv for kv in errs.items())))
    for k, e in errs.items():
        bar = TOL if bars is None or k not in bars else bars[k]
        assert e < bar, (tag, k, e, bar)


def worst(v):
    return float(v.max())


# ---- 1. per-channel scales over ten decades ----------------------------------------------------------------------------
def test_input_channel_scales():
    """x * s_c with w / s_c, s = logspace(-6, 4, C): the output is O(1); every input channel of gx (x s_c) and gw (/ s_c)
    on its own meets TOL, goffset / gmask / gb as tensors."""
    c = S[1]
    s = torch.logspace(-6, 4, c, dtype=torch.float64)
    b0 = base(S)
    cs = case(S, x=r32(b0["x"] * s.view(1, c, 1, 1)), wt=r32(b0["wt"] / s.view(1, c, 1, 1)))
    errs = {k: relerr(gpu_forward(cs, k), ref_forward(cs, pack=(k in PACKED))) for k in KINDS}
    report("domain 1a in-channel scales S fwd", errs)
    got, ref = gpu_backward(cs), ref_backward(cs)
    pc = {"gx": chan_err(got["gx"], ref["gx"], 1, s), "gw": chan_err(got["gw"], ref["gw"], 1, 1.0 / s)}
    errs = {"gx/ch": worst(pc["gx"]), "gw/ch": worst(pc["gw"])}
    errs.update({k: relerr(got[k], ref[k]) for k in ("goffset", "gmask", "gb")})
    report("domain 1a in-channel scales S bwd (worst channel: gx %d, gw %d)" % (int(pc["gx"].argmax()), int(pc["gw"].argmax())),
           errs)


def test_output_channel_scales():
    """w[o] * t_o with gout[o] / t_o: the forward per output channel, gw and gb per output channel after undoing the scale,
    gx / goffset / gmask (O(1)) as tensors."""
    co = S[3]
    t = torch.logspace(-6, 4, co, dtype=torch.float64)
    b0 = base(S)
    cs = case(S, wt=r32(b0["wt"] * t.view(co, 1, 1, 1)), go=r32(b0["go"] / t.view(1, co, 1, 1)))
    errs = {}
    for k in KINDS:
        errs[k + "/ch"] = worst(chan_err(gpu_forward(cs, k), ref_forward(cs, pack=(k in PACKED)), 1))
    report("domain 1b out-channel scales S fwd", errs)
    got, ref = gpu_backward(cs), ref_backward(cs)
    errs = {"gw/ch": worst(chan_err(got["gw"], ref["gw"], 0, t)), "gb/ch": worst(chan_err(got["gb"], ref["gb"], 0, t))}
    errs.update({k: relerr(got[k], ref[k]) for k in ("gx", "goffset", "gmask")})
    report("domain 1b out-channel scales S bwd", errs)


def gx_scatter(cs):
    """The input gradient as the oracle scatters it (kernel.cu:634-692: gate (-1,H) x (-1,W), per-corner validity), in fp64
    from dcol = W^T gout: per element the number of (pixel, tap, corner) contributions, their signed sum and the sum of
    their magnitudes |w_corner * dcol * mask|; and per channel the frexp exponent E of max |dcol| x max |mask| over the
    channel's 8-channel chunk (its group's masks) and the whole image."""
    n, c, dg, cout, h, w = cs["shape"][:6]
    assert n == 1
    cpg = c // dg
    dcol = torch.einsum("ockl,op->cklp", cs["wt"], cs["go"].view(cout, h * w)).reshape(dg, cpg, 9, h, w)
    m = cs["m"].view(dg, 9, h, w)
    py, px = (t[0] for t in _coords(cs["off"], n, dg, h, w))
    inside = (py > -1) & (px > -1) & (py < h) & (px < w)
    y0, x0 = torch.floor(py), torch.floor(px)
    ly, lx = py - y0, px - x0
    top = dcol * m.view(dg, 1, 9, h, w)
    cnt = torch.zeros(dg, h * w, dtype=torch.float64)
    ssum, sabs = torch.zeros(c, h * w, dtype=torch.float64), torch.zeros(c, h * w, dtype=torch.float64)
    for dy, dx, wc in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
        yy, xx = y0 + dy, x0 + dx
        ok = (inside & (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1)).double()
        idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).long()
        cnt.scatter_add_(1, idx.view(dg, -1), ok.view(dg, -1))
        contrib = (top * (wc * ok).view(dg, 1, 9, h, w)).reshape(c, -1)
        idxc = idx.view(dg, 1, -1).expand(-1, cpg, -1).reshape(c, -1)
        ssum.scatter_add_(1, idxc, contrib)
        sabs.scatter_add_(1, idxc, contrib.abs())
    dmax = dcol.reshape(c // 8, -1).abs().max(dim=1).values                          # per 8-channel chunk
    mmax = m.reshape(dg, -1).abs().max(dim=1).values[torch.arange(c // 8) * 8 // cpg]   # its group's masks
    expo = torch.frexp(dmax * mmax).exponent.double()
    return dict(cnt=cnt.view(dg, 1, h, w).expand(-1, cpg, -1, -1).reshape(1, c, h, w), sum=ssum.view(1, c, h, w),
                abs=sabs.view(1, c, h, w), E=expo.repeat_interleave(8).view(1, c, 1, 1))


@pytest.mark.parametrize("shape", [S, S2], ids=["S", "S2"])
def test_interleaved_input_channel_scales_and_fixed_point_window(shape):
    """s'_c = s[(c % 8) * (C / 8) + c // 8]: every 8-channel chunk spans the ten decades.  Forward, gw (per input channel),
    goffset and gmask meet TOL as in test_input_channel_scales.  gx is the one place where channels share precision: the fused
    backward accumulates it in a fixed-point window whose scale is set by the largest |dcol| x |mask| of the WORKGROUP
    (8 channels, one tile), so it is held to the design's own arithmetic, per element and derived from the inputs:

        |gx - ref| <= cnt * 2^(E - 41) + TOL * S_abs

    A contribution w_corner * dcol * mask is scaled by 2^(40 - aexp) (aexp = the frexp exponent of the workgroup's max |dcol| x
    max |mask|, so the maximum lands in [2^39, 2^40)) and rounded to an integer: at most half a unit = 2^(aexp - 41) each, cnt
    of them per element, and aexp <= E = the same exponent over the channel's chunk and the WHOLE image.  Everything else
    (fp32 dcol and blend weights, the fp32 flush and atomics) is fp32 round-off of the terms, held to TOL of their magnitudes
    S_abs.  A scale of 2^30 instead of 2^40, or a window that drops low bits, fails this; the design as written passes.
    Channels whose scale lies within 2^-16 of their chunk's largest keep >= 24 significant bits and meet plain TOL."""
    c = shape[1]
    s = torch.logspace(-6, 4, c, dtype=torch.float64)
    ch = torch.arange(c)
    sp = s[(ch % 8) * (c // 8) + ch // 8]
    assert sorted(sp.tolist()) == sorted(s.tolist())
    b0 = base(shape)
    cs = case(shape, x=r32(b0["x"] * sp.view(1, c, 1, 1)), wt=r32(b0["wt"] / sp.view(1, c, 1, 1)))
    name = NAMES[shape]
    errs = {k: relerr(gpu_forward(cs, k), ref_forward(cs, pack=(k in PACKED))) for k in KINDS}
    report("domain 1c interleaved scales %s fwd" % name, errs)
    got, ref = gpu_backward(cs), ref_backward(cs)
    st = gx_scatter(cs)
    assert relerr(st["sum"], ref["gx"]) < 1e-11, "the scatter of this test is not the oracle's"
    gxe = chan_err(got["gx"], ref["gx"], 1, sp)
    errs = {"gw/ch": worst(chan_err(got["gw"], ref["gw"], 1, 1.0 / sp))}
    errs.update({k: relerr(got[k], ref[k]) for k in ("goffset", "gmask", "gb")})
    # channels within 2^-16 of their chunk's largest dcol scale (1 / s'_c)
    inv = (1.0 / sp).view(c // 8, 8)
    near = (inv / inv.max(dim=1, keepdim=True).values >= 2.0 ** -16).view(c)
    assert int(near.sum()) >= c // 8 and int((~near).sum()) >= c // 8
    errs["gx/ch (within 2^-16)"] = worst(gxe[near])
    err = (got["gx"].double().cpu() - ref["gx"]).abs()
    quant = st["cnt"] * 2.0 ** (st["E"] - 41.0)
    bound = quant + TOL * st["abs"]
    ratio = err / bound.clamp_min(1e-300)
    print("[dcn] domain 1c interleaved scales %s gx: worst |err| / bound %.3f (channel %d); worst |err| / fixed-point term alone "
          "%.3f; per-channel rel-L2 far channels up to %.2e"
          % (name, float(ratio.max()), int(ratio.flatten(2).max(dim=2).values.argmax()),
             float((err / quant.clamp_min(1e-300))[:, ~near].max()), worst(gxe[~near])))
    report("domain 1c interleaved scales %s bwd" % name, errs)
    assert bool((err[bound == 0] == 0).all())
    assert float(ratio.max()) <= 1.0, ("gx outside the fixed-point bound", float(ratio.max()))


# ---- 2. magnitude range ------------------------------------------------------------------------------------------------
# which outputs carry the factor 2^e when one operand does (the bias is zero in these tests: the output then scales cleanly)
CARRIES = {"x": ("out", "goffset", "gmask", "gw"), "wt": ("out", "gx", "goffset", "gmask"),
           "go": ("gx", "goffset", "gmask", "gw", "gb")}


def _scaled_case(shape, operand, e):
    b0 = base(shape)
    return case(shape, b=torch.zeros_like(b0["b"]), **{operand: b0[operand] * 2.0 ** e})


def _fwd_errs(cs, up, kinds=KINDS):
    errs = {}
    for k in kinds:
        errs[k] = relerr(gpu_forward(cs, k).double().cpu() * up, ref_forward(cs, pack=(k in PACKED)) * up)
    return errs


def _bwd_errs(cs, operand, e, keys=GRADS):
    got, ref = gpu_backward(cs, finite=False), ref_backward(cs)
    up = {k: 2.0 ** (-e if k in CARRIES[operand] else 0) for k in keys}
    return {k: relerr(got[k].double().cpu() * up[k], ref[k] * up[k]) for k in keys}, {k: got[k] for k in keys}


@pytest.mark.parametrize("e", [100, -100])
@pytest.mark.parametrize("operand,shape", [("x", S), ("wt", S), ("go", S), ("go", F)], ids=["x-S", "w-S", "gout-S", "gout-F"])
def test_magnitude_in_domain(operand, shape, e):
    """One operand times 2^+-100 (inside 2^-110 <= |v| < 2^127): every output at TOL once its factor is undone, and finite.
    gout * 2^-100 puts the workgroup maximum of the gradient window at 2^-101: its scale 2^(40 - aexp) is clamped to 2^126
    (DESIGN 3.3), the maximum lands at 2^25 instead of 2^39 and gx keeps TOL; unclamped, the scale is +inf and gx garbage, on
    both instantiations (F: fp32 MFMAs, same window)."""
    cs = _scaled_case(shape, operand, e)
    tag = "domain 2 %s * 2^%d %s" % ({"x": "x", "wt": "w", "go": "gout"}[operand], e, NAMES[shape])
    if operand != "go":
        report(tag + " fwd", _fwd_errs(cs, 2.0 ** -e))
    errs, got = _bwd_errs(cs, operand, e)
    report(tag + " bwd", errs)
    all_finite(tag, got)


# rel-L2 of the SPLIT kernels against the fp64 oracle with x * 2^e below the domain (the small pieces of the split are bf16
# subnormals: the growth has no sharp edge).  Measured on the MI355X (profiles/r07_dcn_domain.txt), asserted at
# the next value of the 1-2-5 series at least 3x above.  The fp32 controls ('pack' and 'plain' on S, everything on F) are held to
# TOL: measured 4.0e-07 .. 5.6e-07 forward, 1.7e-07 gw, at all three magnitudes.
SUB_BARS = {
    -116: {"fast": 2e-5, "packfast": 2e-5, "gw": 2e-5},     # measured 5.19e-06 / 5.20e-06 / 5.13e-06
    -120: {"fast": 5e-4, "packfast": 5e-4, "gw": 5e-4},     # measured 8.26e-05 / 8.27e-05 / 8.25e-05
    -124: {"fast": 5e-3, "packfast": 5e-3, "gw": 5e-3},     # measured 1.33e-03 / 1.33e-03 / 1.31e-03
}


@pytest.mark.parametrize("e", [-116, -120, -124])
def test_magnitude_below_domain(e):
    """x * 2^e: the split forward ('fast', 'packfast' on S) and gw of the fused SPLIT backward stay finite and within the
    measured bars; the fp32 controls -- 'pack' and 'plain' on S, everything on F -- stay at TOL."""
    tag = "domain 2 x * 2^%d" % e
    cs, cf = _scaled_case(S, "x", e), _scaled_case(F, "x", e)
    errs = _fwd_errs(cs, 2.0 ** -e)
    gw_s, got_s = _bwd_errs(cs, "x", e, keys=("gw",))
    errs["gw"] = gw_s["gw"]
    ctl = {"F " + k: v for k, v in _fwd_errs(cf, 2.0 ** -e).items()}
    gw_f, got_f = _bwd_errs(cf, "x", e, keys=("gw",))
    ctl["F gw"] = gw_f["gw"]
    report(tag + " S", errs, bars=SUB_BARS[e])
    report(tag + " F", ctl)
    all_finite(tag, got_s)
    all_finite(tag, got_f)


# ---- 3. one non-finite element -----------------------------------------------------------------------------------------
def _masked_err(got, ref, bad):
    z = torch.zeros_like(ref)
    return relerr(torch.where(bad, z, got.double().cpu()), torch.where(bad, z, ref))


@pytest.mark.parametrize("val", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("shape", [S, F], ids=["S", "F"])
def test_non_finite_x(shape, val):
    """x[0, 19, 5, 17] = inf / NaN.  Forward (all four kinds): non-finite on exactly the oracle's pixels (every output
    channel), everything else at TOL; on the split kernel ('fast', 'packfast' on S) the values are all NaN -- inf - inf in the
    split, as for the other split kernels -- where the fp32 kernels return +-inf.  Backward: gx and gb do not read x: finite, TOL; goffset / gmask
    non-finite wherever the oracle's are and only in deformable group 2; gw wherever the oracle's is and only in input channel
    19; elements finite on both sides at TOL."""
    n, c, dg, cout, h, w = shape
    x = base(shape)["x"].clone()
    x[0, 19, 5, 17] = val
    cs = case(shape, x=x)
    tag = "domain 3 x[0,19,5,17] = %s %s" % (val, NAMES[shape])
    errs = {}
    for k in KINDS:
        ref = ref_forward(cs, pack=(k in PACKED))
        bad_ref = ~torch.isfinite(ref)
        npix = int(bad_ref[0, 0].sum())
        assert 0 < npix < h * w and torch.equal(bad_ref, bad_ref[:, :1].expand_as(bad_ref))
        got = gpu_forward(cs, k, finite=False).cpu()
        bad = ~torch.isfinite(got)
        assert torch.equal(bad, bad_ref), (tag, k, "non-finite on %d elements, the oracle on %d" % (int(bad.sum()), int(bad_ref.sum())))
        if shape == S and k in ("fast", "packfast"):
            assert bool(torch.isnan(got[bad]).all()), (tag, k, "the split kernel returns NaN, not inf")
        errs[k] = _masked_err(got, ref, bad)
    report(tag + " fwd (%d of %d pixels non-finite)" % (npix, h * w), errs)
    got, ref = gpu_backward(cs, finite=False), ref_backward(cs)
    got = {k: v.cpu() for k, v in got.items()}
    bad, bad_ref = ({k: ~torch.isfinite(v) for k, v in d.items()} for d in (got, ref))
    errs = {k: _masked_err(got[k], ref[k], bad[k] | bad_ref[k]) for k in GRADS}
    print("[dcn] %s bwd non-finite (kernel / oracle): %s" % (tag, "  ".join("%s %d/%d" % (k, int(bad[k].sum()), int(bad_ref[k].sum()))
                                                                          for k in GRADS)))
    report(tag + " bwd", errs)
    assert not bad["gx"].any() and not bad["gb"].any() and not bad_ref["gx"].any() and not bad_ref["gb"].any()
    for k, per in (("goffset", 18), ("gmask", 9)):
        assert bad_ref[k].any() and bool((bad[k] | ~bad_ref[k]).all()), (tag, k, "finite where the oracle is not")
        allowed = torch.zeros_like(bad[k])
        allowed[:, 2 * per:3 * per] = True
        assert bool((allowed | ~bad[k]).all()), (tag, k, "non-finite outside deformable group 2")
    assert bad_ref["gw"].any() and bool((bad["gw"] | ~bad_ref["gw"]).all()), (tag, "gw finite where the oracle is not")
    allowed = torch.zeros_like(bad["gw"])
    allowed[:, 19] = True
    assert bool((allowed | ~bad["gw"]).all()), (tag, "gw non-finite outside input channel 19")


def test_non_finite_x_under_a_clamped_window_cell():
    """S2, x[0, 19, 11, 35] = inf.  The samples of output row 3 (+50 on both offsets) leave the staged window down and to the
    right; the fused backward's straight-line path reads them at the window's clamped last cell -- image rows 11 / 12 and
    columns 35 / 36 for tile (0, 0), so through this element -- and must contribute exact zeros there.  With two chunks per group the offset / mask gradients
    are ADDED (atomics), so what that path stores cannot be overwritten by the exact loop: goffset / gmask are non-finite
    on exactly the oracle's entries (row 3 of the oracle is 0: those samples are outside the image).  A product with a zero
    mask instead of a select leaves NaN in row 3."""
    n, c, dg, cout, h, w = S2
    x = base(S2)["x"].clone()
    x[0, 19, 11, 35] = float("inf")
    cs = case(S2, x=x)
    tag = "domain 3 x[0,19,11,35] = inf S2"
    got, ref = gpu_backward(cs, finite=False), ref_backward(cs)
    got = {k: v.cpu() for k, v in got.items()}
    bad, bad_ref = ({k: ~torch.isfinite(v) for k, v in d.items()} for d in (got, ref))
    errs = {k: _masked_err(got[k], ref[k], bad[k] | bad_ref[k]) for k in GRADS}
    print("[dcn] %s bwd non-finite (kernel / oracle): %s; in output row 3: goffset %d/%d  gmask %d/%d"
          % (tag, "  ".join("%s %d/%d" % (k, int(bad[k].sum()), int(bad_ref[k].sum())) for k in GRADS),
             int(bad["goffset"][:, :, 3].sum()), int(bad_ref["goffset"][:, :, 3].sum()),
             int(bad["gmask"][:, :, 3].sum()), int(bad_ref["gmask"][:, :, 3].sum())))
    report(tag + " bwd", errs)
    assert not bad["gx"].any() and not bad["gb"].any()
    for k in ("goffset", "gmask"):
        assert bad_ref[k].any() and not bad_ref[k][:, :, 3].any()
        assert torch.equal(bad[k], bad_ref[k]), (tag, k, "non-finite on %d entries, the oracle on %d" % (int(bad[k].sum()), int(bad_ref[k].sum())))
    assert bad_ref["gw"].any() and bool((bad["gw"] | ~bad_ref["gw"]).all())
    allowed = torch.zeros_like(bad["gw"])
    allowed[:, 19] = True
    assert bool((allowed | ~bad["gw"]).all()), (tag, "gw non-finite outside input channel 19")


def _window_mask(shape, py, px):
    """The elements of gx that the fused backward's workgroups of the tile holding output pixel (py, px) flush: their
    gradient window -- the 8 x 32 tile with a border of 1 + HALO = 5 -- inside the image, all channels."""
    n, c, dg, cout, h, w = shape
    oy0, ox0 = py // 8 * 8, px // 32 * 32
    mk = torch.zeros(n, c, h, w, dtype=torch.bool)
    mk[:, :, max(oy0 - 5, 0):min(oy0 + 8 + 5, h), max(ox0 - 5, 0):min(ox0 + 32 + 5, w)] = True
    return mk


@pytest.mark.parametrize("val", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("pos", [(5, 17), (9, 33)], ids=["p5-17", "p9-33"])
@pytest.mark.parametrize("shape", [S, F], ids=["S", "F"])
def test_non_finite_gout(shape, pos, val):
    """gout[0, 23, py, px] = inf / NaN.  Every element that is non-finite in the oracle is non-finite in the kernel (no silent
    finite garbage); gb and gw are non-finite nowhere outside output channel 23, goffset / gmask nowhere outside that pixel;
    every element finite on both sides is at TOL.  (Inside the pixel the kernel's gmask is non-finite on all 72 entries, the
    oracle's on those whose sample passes the gate: the kernel tests only the lower bounds of the gate -- beyond H / W the
    zero padding gives the sample value 0 -- and NaN x 0 is NaN where the oracle skips the sample.)

    gx is a structural superset, pinned here: the fused backward accumulates the input gradient of a workgroup (8 channels,
    one 8 x 32 tile) in a fixed-point LDS window, which cannot hold inf or NaN; when the workgroup's largest |dcol| is not finite
    the flush writes NaN to the WHOLE window (the tile and a border of 5, inside the image) -- DESIGN 3.3.  So gx is non-finite
    on exactly the oracle's elements plus that window, in all channels (dcol = W^T gout spreads the element over every input
    channel), and finite at TOL outside.  At (5, 17) the window of tile (0, 0) covers the whole 12 x 36 image; (9, 33) lies
    in tile (1, 1), whose window leaves rows 0-2 and columns 0-26 finite."""
    n, c, dg, cout, h, w = shape
    py, px = pos
    go = base(shape)["go"].clone()
    go[0, 23, py, px] = val
    cs = case(shape, go=go)
    tag = "domain 3 gout[0,23,%d,%d] = %s %s" % (py, px, val, NAMES[shape])
    got, ref = gpu_backward(cs, finite=False), ref_backward(cs)
    got = {k: v.cpu() for k, v in got.items()}
    bad, bad_ref = ({k: ~torch.isfinite(v) for k, v in d.items()} for d in (got, ref))
    errs = {k: _masked_err(got[k], ref[k], bad[k] | bad_ref[k]) for k in GRADS}
    print("[dcn] %s non-finite (kernel / oracle): %s" % (tag, "  ".join("%s %d/%d" % (k, int(bad[k].sum()), int(bad_ref[k].sum()))
                                                                      for k in GRADS)))
    report(tag, errs)
    for k in GRADS:
        assert bad_ref[k].any()
        missing = bad_ref[k] & ~bad[k]
        assert not missing.any(), (tag, k, "%d elements finite where the oracle is not" % int(missing.sum()))
    for k in ("gw", "gb"):
        allowed = torch.zeros_like(bad[k])
        allowed[23] = True
        assert bool((allowed | ~bad[k]).all()), (tag, k, "non-finite outside output channel 23")
    for k in ("goffset", "gmask"):
        allowed = torch.zeros_like(bad[k])
        allowed[:, :, py, px] = True
        assert bool((allowed | ~bad[k]).all()), (tag, k, "non-finite outside the pixel")
    want = bad_ref["gx"] | _window_mask(shape, py, px)
    assert torch.equal(bad["gx"], want), (tag, "gx non-finite on %d elements, oracle + window %d" % (int(bad["gx"].sum()), int(want.sum())))
    if pos == (9, 33):
        assert int((~want).sum()) > c * h * w // 2


# ---- 4. mask logits over a wide range ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [S, F], ids=["S", "F"])
def test_pack_mask_logits_wide_range(shape):
    """Logits ~ N(0, 8^2) with a few exactly +-100 and +-inf: the kernels' sigmoid is rcp(1 + __expf(-m)) (exp overflows to
    inf -> 0, underflows to 0 -> 1).  Reference: the oracle on torch.sigmoid of the fp32 logits in fp64."""
    n, c, dg, cout, h, w = shape
    r = np.random.RandomState(99)
    lg = r32(torch.from_numpy(r.standard_normal((n, dg * 9, h, w)) * 8.0))
    flat = lg.view(-1)
    pos = torch.from_numpy(r.choice(flat.numel(), 16, replace=False))
    flat[pos] = torch.tensor([100.0, -100.0, float("inf"), float("-inf")], dtype=torch.float64).repeat(4)
    cs = case(shape, lg=lg)
    ref = ref_forward(cs, pack=True)
    assert bool(torch.isfinite(ref).all())
    report("domain 4 mask logits N(0,64), +-100, +-inf %s" % NAMES[shape], {k: relerr(gpu_forward(cs, k), ref) for k in PACKED})
