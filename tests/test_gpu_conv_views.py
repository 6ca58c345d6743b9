"""Dense convolution on operands that are VIEWS: x0_bstride, x1_bstride and x1_bdiv of dvsr_conv2d_desc, and stride 2 at odd sizes.

The engine convolves channel slices of wider tensors (the centre frame of [B][Nf][C][H][W], the hoisted reference part) and shares
one reference frame among the frames of a clip (x1 batch index = n / x1_bdiv); every kernel family has its own copy of that
indexing.  Here each family runs it at op level: every strided operand is a channel slice of a larger device buffer whose other
elements hold a large finite sentinel, so a read across the slice boundary, a dropped stride or a wrong n / x1_bdiv shows in the
result.  Nothing points outside an allocation.

Two checks per case:
  1. against fp64 torch on the CPU over the materialised operands, at the bar the suite already holds that kernel family to (the
     direct fp32 kernels 2e-5, F(2x2) 2e-6, F(4x4) 4e-6 and 5e-5 max-abs, the split weight gradient 2e-6, plain bf16 2e-5 against
     the gradient of the bf16-rounded operands) -- on the whole output and on the LAST batch item alone;
  2. against the same entry point on dense copies (x0.contiguous(), x1 materialised with x1_bdiv = 1): torch.equal wherever the
     geometry query returns the same tuple for both descriptors -- stride and sharing change addresses, not the order of a sum --
     and the bar of check 1 where the tuples differ (the weight gradient's staging width follows the stride: said in the ids).

Bit equality of the weight gradient needs a flush whose order cannot matter: the kernels add their partial sums atomically into
min(nsplit, 8) slots, so with at most 16 workgroups per launch and one addend per workgroup and element a slot gets at most two
addends (0 + a + b == 0 + b + a).  Every backward shape here has at most 16 two-row tiles.  One addend per workgroup holds for the
bf16, split and stride-2 kernels everywhere, and for the pipelined fp32 kernel on the 64 x 64 (cout, cin) blocks that hold more
than 32 channels on both sides: where a half of a block is empty, the waves that would own it share the other half's pixel
reduction and flush to the same elements (conv2d_wgrad_pipe_item: kinc > 1), four addends per slot in an order that two runs of
the SAME launch need not repeat.  Outside `flushed_once` the dense launch is compared at the bar of check 1; cin = 40 / cout = 104
have no such block and are compared bit for bit throughout.  The bias gradient does not read x at all and its flush adds several
lanes of a workgroup to one element: it is held to the fp64 bar only.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import relerr

pytestmark = pytest.mark.gpu

SENTINEL = 1.0e4
TOL = 2e-5        # the direct fp32 kernels (test_gpu_ops.TOL)
TOL_F2 = 2e-6     # Winograd F(2x2) on either pipe (test_conv3x3_winograd)
TOL_F4 = 4e-6     # Winograd F(4x4): rel-L2, and ...
MAXABS_F4 = 5e-5  # ... max-abs on O(1) outputs (test_conv3x3_winograd_f4x4)
TOL_SPLIT = 2e-6  # the split weight gradient (test_conv3x3_wgrad_split3)

ACT = {0: lambda v: v, 1: lambda v: F.leaky_relu(v, 0.1), 2: F.relu}
REG, DMA_HALO, ROW_SPLIT, WINO_F2, WINO_F2_BF16, WINO_F4 = range(6)   # geo[3] of dvsr_conv2d_packed_geometry


def rnd(*shape, seed, scale=1.0):
    """fp32-representable values (the fp64 reference and the kernels see the same numbers)."""
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape) * scale).float()


def slice_of(t, extra, tail=0):
    """t [N][C][H][W] -> the same values on the device as channels [extra / 2, extra / 2 + C) of a [N][C + extra][H][W] buffer with
    `tail` more floats per batch item (batch strides off the multiples of 4); everything else in the buffer is SENTINEL."""
    n, c, h, w = t.shape
    hw = h * w
    bs, lead = (c + extra) * hw + tail, (extra // 2) * hw
    buf = torch.full((n * bs,), SENTINEL, device="cuda")
    v = buf.as_strided((n, c, h, w), (bs, hw, w, 1), lead)
    v.copy_(t)
    assert lead + (n - 1) * bs + c * hw <= buf.numel() and int((buf == SENTINEL).sum()) == buf.numel() - t.numel()
    return v


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bs(t):
    return 0 if t is None or t.is_contiguous() else t.stride(0)


def _desc(x0, x1, wt, b, res, y, n, cout, ks, stride, act=0, ps=0, bdiv=1):
    from dynavsr_amd import _lib as L
    _, c0, h, w = x0.shape
    c1 = 0 if x1 is None else x1.shape[1]
    return L.Conv2dDesc(_ptr(x0), _ptr(x1), _ptr(wt), _ptr(b), _ptr(res), _ptr(y), n, c0, c1, h, w, cout, ks, stride, ks // 2, act, ps,
                        bdiv, _bs(x0), _bs(x1))


def _packed_geo(d):
    from dynavsr_amd import _lib as L
    geo = (ctypes.c_int * 4)()
    L.check(L.lib().dvsr_conv2d_packed_geometry(d, ctypes.byref(geo)), "dvsr_conv2d_packed_geometry")
    return list(geo)


def conv_forward(entry, x0, x1, wt, b, res, cout, ks, stride, act, ps, bdiv):
    """One launch through dvsr_conv2d_forward ("plain") or dvsr_conv2d_forward_packed ("packed"); returns (y on the CPU, geometry).
    y starts as NaN: an output the kernel does not write fails both checks."""
    from dynavsr_amd import _lib as L
    n, _, h, w = x0.shape
    ho, wo = (h + 2 * (ks // 2) - ks) // stride + 1, (w + 2 * (ks // 2) - ks) // stride + 1
    y = torch.full((n, cout // 4, 2 * ho, 2 * wo) if ps else (n, cout, ho, wo), float("nan"), device="cuda")
    d = _desc(x0, x1, wt, b, res, y, n, cout, ks, stride, act, ps, bdiv)
    if entry == "plain":
        L.check(L.lib().dvsr_conv2d_forward(d, L.stream()), "dvsr_conv2d_forward")
        return y.cpu(), None
    geo = _packed_geo(d)
    ws = torch.empty(max(int(L.lib().dvsr_conv2d_packed_workspace_bytes(d)), 16), dtype=torch.uint8, device="cuda")
    L.check(L.lib().dvsr_conv2d_forward_packed(d, ws.data_ptr(), ws.numel(), L.stream()), "dvsr_conv2d_forward_packed")
    return y.cpu(), geo


_FWD = {}


def _forward_operands(n, bdiv, c0, c1, cout, h, w, ks, stride, act, res, ps):
    """Operands and the fp64 reference of a forward case, computed once per shape (the pipes / modes / entries share them)."""
    key = (n, bdiv, c0, c1, cout, h, w, ks, stride, act, res, ps)
    if key not in _FWD:
        nx1 = -(-n // bdiv)                                          # the header's ceil(N / x1_bdiv)
        x0 = rnd(n, c0, h, w, seed=1)
        x1 = rnd(nx1, c1, h, w, seed=6) if c1 else None
        wt = rnd(cout, c0 + c1, ks, ks, seed=2, scale=1 / np.sqrt((c0 + c1) * ks * ks))
        b = rnd(cout, seed=3, scale=0.1)
        x = torch.cat([x0, x1.repeat_interleave(bdiv, 0)[:n]], 1) if c1 else x0
        ref = ACT[act](F.conv2d(x.double(), wt.double(), b.double(), stride, ks // 2))
        r = rnd(*ref.shape, seed=4) if res else None
        if res:
            ref = ref + r.double()
        if ps:
            ref = F.pixel_shuffle(ref, 2)
        _FWD[key] = (x0, x1, wt, b, r, ref)
    return _FWD[key]


def _check(got, ref, bar, maxabs=None, what="y"):
    """The whole tensor and its last batch item alone, where a wrong n / x1_bdiv or a dropped stride shows first."""
    e, e_last = relerr(got, ref), relerr(got[-1], ref[-1])
    print("%s: rel-L2 %.3g, last item %.3g (bar %.1g)" % (what, e, e_last, bar))
    assert e < bar and e_last < bar, (what, e, e_last)
    if maxabs is not None:
        m = float((got.double() - ref).abs().max())
        print("%s: max-abs %.3g (bar %.1g)" % (what, m, maxabs))
        assert m < maxabs, (what, m)


def _forward_case(entry, n, bdiv, c0, c1, cout, h, w, bar, ks=3, stride=1, act=1, res=False, ps=0, tail0=0, tail1=0, expect=None,
                  maxabs=None):
    x0, x1, wt, b, r, ref = _forward_operands(n, bdiv, c0, c1, cout, h, w, ks, stride, act, res, ps)
    dw, db, dr = wt.cuda(), b.cuda(), (r.cuda() if res else None)
    s0, s1 = slice_of(x0, 16, tail0), (slice_of(x1, 8, tail1) if c1 else None)
    y, geo = conv_forward(entry, s0, s1, dw, db, dr, cout, ks, stride, act, ps, bdiv)
    if expect is not None:
        assert expect(geo), "not the kernel this case is for: geometry %s" % geo
    _check(y, ref, bar, maxabs)
    # the same entry point on dense copies: the same kernel and launch, every sum in the same order
    d0, d1 = x0.cuda(), (x1.repeat_interleave(bdiv, 0)[:n].contiguous().cuda() if c1 else None)
    yd, geod = conv_forward(entry, d0, d1, dw, db, dr, cout, ks, stride, act, ps, 1)
    assert geod == geo, (geo, geod)
    assert torch.equal(y, yd), "strided / shared operands change the result: %d elements differ" % int((y != yd).sum())
    return geo


def _env(monkeypatch, wino=None, wino3=None, wino5=None):
    for k, v in (("DVSR_CONV_WINO", wino), ("DVSR_CONV_WINO3", wino3), ("DVSR_CONV_WINO5", wino5)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


# ---- the un-packed kernel (conv2d.hip): 3x3 and 1x1, N = 7 with x1_bdiv = 3 (x1 holds ceil(7 / 3) = 3 items) ------------------------
@pytest.mark.parametrize("ks,w,tail0,tail1", [(3, 36, 0, 0), (1, 36, 0, 0), (3, 36, 2, 0), (3, 35, 0, 0), (1, 35, 1, 1)],
                         ids=["3x3", "1x1", "3x3-x0_bstride%4==2", "3x3-W35", "1x1-W35-odd-strides"])
def test_conv2d_unpacked_views(ks, w, tail0, tail1):
    _forward_case("plain", 7, 3, 24, 8, 40, 10, w, TOL, ks=ks, act=1, res=True, tail0=tail0, tail1=tail1)


# ---- the pipelined register-staged kernel (conv2d_v2.hip: conv2d_pipe_kernel) ---------------------------------------------------
def test_conv3x3_packed_reg_views(monkeypatch):
    """W = 35 is not "aligned" (no DMA-halo, no Winograd), c0 % 32 != 0 keeps the K-split kernel away, c0 % 8 == 0 as two inputs need."""
    _env(monkeypatch)
    _forward_case("packed", 7, 3, 24, 8, 40, 10, 35, TOL, res=True, expect=lambda g: g[3] == REG and g[0] == 8)


def test_conv1x1_packed_reg_views(monkeypatch):
    _env(monkeypatch)
    _forward_case("packed", 7, 3, 32, 32, 40, 10, 36, TOL, ks=1, res=True, expect=lambda g: g[3] == REG and g[0] == 32)


# ---- the K-split small-grid kernel (small_grid.h) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,tail0,geo", [(40, 0, [32, 2, 1, REG]), (64, 2, [32, 1, 2, REG])],
                         ids=["2rows-x-32couts", "1row-x-64couts-x0_bstride%4==2"])
def test_conv3x3_ksplit_views(cout, tail0, geo, monkeypatch):
    _env(monkeypatch)
    _forward_case("packed", 6, 3, 32, 32, cout, 10, 36, TOL, res=True, tail0=tail0, expect=lambda g: g == geo)


# ---- the DMA-halo kernel (conv2d_dma_kernel) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
def test_conv3x3_dma_halo_views(res, monkeypatch):
    """c0 = 24, c1 = 8: not "plain", so the K-split kernel is skipped; every stride a multiple of 4, 16-byte aligned slices."""
    _env(monkeypatch, wino="0")
    _forward_case("packed", 6, 3, 24, 8, 40, 10, 36, TOL, res=res, expect=lambda g: g[3] == DMA_HALO and g[:2] == [8, 4])


# ---- Winograd F(2x2) on the fp32 pipe (conv2d_wino.hip) and on the bf16 pipe under the 3-way split (conv2d_wino3 / wino4.hip) -----------
F2_SHAPES = {   # n, bdiv, c0, c1, cout, h, w, res, ps, tile rows
    "4x64-residual": (6, 3, 24, 8, 40, 10, 36, True, 0, 4),      # one round of workgroups: the cost model ties and takes 4x64; Cout % 32 != 0
    "4x64-pixelshuffle": (6, 3, 24, 8, 64, 10, 36, False, 2, 4),  # ... with the PixelShuffle(2) store
    "8x32-200-images": (200, 5, 8, 8, 64, 8, 32, False, 0, 8),    # many tiny images, 40 shared references: 400 workgroups of 4x64 against 200 of 8x32
    "16x16-200-images": (200, 5, 8, 8, 64, 16, 16, False, 0, 16),  # 800 / 400 / 200 workgroups: the 16x16 tile, which the bf16 pipe alone has
}


@pytest.mark.parametrize("pipe,shape", [("fp32", "4x64-residual"), ("fp32", "4x64-pixelshuffle"), ("fp32", "8x32-200-images"),
                                        ("bf16x3", "4x64-residual"), ("bf16x3", "4x64-pixelshuffle"), ("bf16x3", "8x32-200-images"),
                                        ("bf16x3", "16x16-200-images")])
def test_conv3x3_winograd_f2x2_views(pipe, shape, monkeypatch):
    n, bdiv, c0, c1, cout, h, w, res, ps, th = F2_SHAPES[shape]
    _env(monkeypatch, wino="2", wino3="1" if pipe == "bf16x3" else "0", wino5="0")
    kernel = WINO_F2_BF16 if pipe == "bf16x3" else WINO_F2
    _forward_case("packed", n, bdiv, c0, c1, cout, h, w, TOL_F2, res=res, ps=ps, expect=lambda g: g == [8, th, 2, kernel])


# ---- Winograd F(4x4) (conv2d_wino5.hip), both workgroup tiles -------------------------------------------------------------------------
@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("mode", ["2", "3"])
def test_conv3x3_winograd_f4x4_views(res, mode, monkeypatch):
    """H % 4 == 2 cuts the last tile row."""
    _env(monkeypatch, wino="2", wino3="1", wino5=mode)
    _forward_case("packed", 6, 3, 24, 8, 40, 10, 36, TOL_F4, res=res, maxabs=MAXABS_F4,
                  expect=lambda g: g == [8, 8 if mode == "2" else 16, 2, WINO_F4])


@pytest.mark.parametrize("mode", ["2", "3"])
def test_conv3x3_winograd_f4x4_reference_part_view(mode, monkeypatch):
    """The descriptor the engine builds for the hoisted reference part of a two-input conv: ONE strided input -- the second
    input's slice of a wider buffer, its batch stride as x0_bstride --, N = 2 clips, the bias, no activation."""
    _env(monkeypatch, wino="2", wino3="1", wino5=mode)
    _forward_case("packed", 2, 1, 24, 0, 40, 10, 36, TOL_F4, act=0, maxabs=MAXABS_F4,
                  expect=lambda g: g == [8, 8 if mode == "2" else 16, 2, WINO_F4])


# ---- the row-split 7x7 kernel (conv2d_dmarow_kernel) -----------------------------------------------------------------------------------
def test_conv7x7_row_split_views(monkeypatch):
    """SpyNet's two-input 7x7 with a partial last chunk (c1 = 5), the second input shared by pairs of items."""
    _env(monkeypatch)
    _forward_case("packed", 4, 2, 8, 5, 32, 9, 36, TOL, ks=7, act=2, res=True, expect=lambda g: g[3] == ROW_SPLIT and g[:2] == [8, 4])


# ---- weight gradient: batch strides = 0, 2 (mod 4) and odd --------------------------------------------------------------------------
def _wgrad_geo(x, gy, cout, ks, stride, mode):
    from dynavsr_amd import _lib as L
    d = _desc(x, None, None, None, None, gy, x.shape[0], cout, ks, stride)   # (y stands for the gradient: its alignment is read)
    geo = (ctypes.c_int * 8)()
    L.check(L.lib().dvsr_conv2d_wgrad_geometry(d, mode, 1, ctypes.byref(geo)), "dvsr_conv2d_wgrad_geometry")
    return list(geo)


def conv_backward(x0, x1, wt, gy, ks, stride):
    """dvsr_conv2d_backward (its weight gradient: mode 0); returns (gx0, gx1, gw, gb) on the CPU, NaN where nothing was written."""
    from dynavsr_amd import _lib as L
    n, cout = x0.shape[0], wt.shape[0]
    d = _desc(x0, x1, wt, None, None, None, n, cout, ks, stride)
    ws = torch.empty(max(int(L.lib().dvsr_conv2d_backward_workspace_bytes(d)), 16), dtype=torch.uint8, device="cuda")
    nan = float("nan")
    gx0 = torch.full(tuple(x0.shape), nan, device="cuda")
    gx1 = torch.full(tuple(x1.shape), nan, device="cuda") if x1 is not None else None
    gw, gb = torch.full(tuple(wt.shape), nan, device="cuda"), torch.full((cout,), nan, device="cuda")
    L.check(L.lib().dvsr_conv2d_backward(d, gy.data_ptr(), gx0.data_ptr(), _ptr(gx1), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(),
                                         ws.numel(), L.stream()), "dvsr_conv2d_backward")
    return gx0.cpu(), (gx1.cpu() if x1 is not None else None), gw.cpu(), gb.cpu()


def conv_wgrad(mode, x, gy, cout):
    """dvsr_conv2d_wgrad_bf16 (mode 1) / dvsr_conv2d_wgrad_split3 (mode 2) of a 3x3 stride-1 conv; (gw, gb) on the CPU."""
    from dynavsr_amd import _lib as L
    n, cin = x.shape[:2]
    d = _desc(x, None, None, None, None, None, n, cout, 3, 1)
    ws = torch.empty(max(int(L.lib().dvsr_conv2d_backward_workspace_bytes(d)), 16), dtype=torch.uint8, device="cuda")
    gw, gb = torch.full((cout, cin, 3, 3), float("nan"), device="cuda"), torch.full((cout,), float("nan"), device="cuda")
    fn = L.lib().dvsr_conv2d_wgrad_bf16 if mode == 1 else L.lib().dvsr_conv2d_wgrad_split3
    L.check(fn(d, gy.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), ws.numel(), L.stream()), "dvsr_conv2d_wgrad (mode %d)" % mode)
    return gw.cpu(), gb.cpu()


_BWD = {}


def _backward_operands(n, cin, cout, h, w, ks, stride):
    """x, w, gy and the fp64 gradients (gx, gw, gb; gw of the bf16-rounded operands too for 3x3 stride 1), once per shape."""
    key = (n, cin, cout, h, w, ks, stride)
    if key not in _BWD:
        x, wt = rnd(n, cin, h, w, seed=1), rnd(cout, cin, ks, ks, seed=2, scale=1 / np.sqrt(cin * ks * ks))
        xd, wd = x.double().requires_grad_(), wt.double().requires_grad_()
        y = F.conv2d(xd, wd, None, stride, ks // 2)
        gy = rnd(*y.shape, seed=4)
        gx, gw = torch.autograd.grad(y, [xd, wd], gy.double())
        gw_bf = None
        if ks == 3 and stride == 1:
            (gw_bf,) = torch.autograd.grad(F.conv2d(x.bfloat16().double(), wd, None, 1, 1), wd, gy.bfloat16().double())
        _BWD[key] = (x, wt, gy, y.detach(), gx, gw, gy.double().sum(dim=(0, 2, 3)), gw_bf)
    return _BWD[key]


# tail floats per batch item -> (x0_bstride mod 4, the staging width the fp32 and the split kernels take: float4, float2, scalar = 0)
STRIDES = [(0, 4), (2, 2), (1, 0)]


def _wgrad_stride_case(mode, cin, tail, cout=72):
    n, h, w = 3, 7, 20                                  # 12 two-row tiles: at most two workgroups per flush slot
    x, _, gy, _, _, gw_ref, gb_ref, gw_bf = _backward_operands(n, cin, cout, h, w, 3, 1)
    sx, dx, dgy = slice_of(x, 16, tail), x.cuda(), gy.cuda()
    assert sx.stride(0) % 4 == {0: 0, 2: 2, 1: 1}[tail] and sx.stride(0) % 2 == tail % 2
    geo, geod = _wgrad_geo(sx, dgy, cout, 3, 1, mode), _wgrad_geo(dx, dgy, cout, 3, 1, mode)
    print("mode %d: geometry %s, dense %s" % (mode, geo, geod))
    return sx, dx, dgy, geo, geod, gw_ref, gb_ref, gw_bf, x, gy


def flushed_once(cout, cin):
    """[cout][cin] mask of the weight-gradient elements the pipelined fp32 kernel flushes with one addend per workgroup: those of
    the 64 x 64 blocks with more than 32 channels on both sides (see the module docstring)."""
    o, c = torch.arange(cout), torch.arange(cin)
    return ((cout - o // 64 * 64 > 32)[:, None] & (cin - c // 64 * 64 > 32)[None, :])


def _same_or_close(got, dense, geo, geod, bar, what, mask=None):
    if geo == geod:
        if mask is None:
            mask = torch.ones(got.shape[:2], dtype=torch.bool)
        print("%s: %d of %d (cout, cin) pairs compared bit for bit" % (what, int(mask.sum()), mask.numel()))
        assert torch.equal(got[mask], dense[mask]), "%s: the batch stride changes the result: %d elements differ" % (
            what, int((got[mask] != dense[mask]).sum()))
        if not bool(mask.all()):
            e = relerr(got[~mask], dense[~mask])
            print("%s against the dense launch where several waves flush one element: rel-L2 %.3g" % (what, e))
            assert e < bar, (what, e)
    else:
        e = relerr(got, dense)
        print("%s against the dense launch (another geometry): rel-L2 %.3g" % (what, e))
        assert e < bar, (what, e)


@pytest.mark.parametrize("cin,cout", [(24, 72), (40, 72), (40, 104)],
                         ids=["24-72-shared-halves-bar", "40-72-wide-staging-last-8-couts-bar", "40-104-wide-staging"])
@pytest.mark.parametrize("tail,vx", STRIDES, ids=["vx4-bit-equal", "vx2-dense-differs-bar", "scalar-dense-differs-bar"])
def test_conv2d_backward_batch_strides(tail, vx, cin, cout):
    """dvsr_conv2d_backward on a strided x0: the pipelined fp32 weight gradient (one kernel row per workgroup on this grid), and
    the data gradient.  cin = 24 keeps the kernel's general staging whatever vx says (its wide forms need more than 32 channels
    in the block); cin = 40 stages float4 / float2 / scalar as the geometry reports.  With cin = 24 every element, with cout = 72
    the last eight output channels are flushed by several waves in a free order: bit equality is asserted on the rest (flushed_once)."""
    sx, dx, dgy, geo, geod, gw_ref, gb_ref, _, x, gy = _wgrad_stride_case(0, cin, tail, cout)
    assert geo[0] == 1 and geo[2] == vx and geod[2] == 4, (geo, geod)
    _, wt, _, _, gx_ref, _, _, _ = _backward_operands(3, cin, cout, 7, 20, 3, 1)
    dw = wt.cuda()
    gx, _, gw, gb = conv_backward(sx, None, dw, dgy, 3, 1)
    _check(gx, gx_ref, TOL, what="gx")
    for name, got, ref in (("gw", gw, gw_ref), ("gb", gb, gb_ref)):
        e = relerr(got, ref)
        print("%s: rel-L2 %.3g" % (name, e))
        assert e < TOL, (name, e)
    gxd, _, gwd, _ = conv_backward(dx, None, dw, dgy, 3, 1)
    assert torch.equal(gx, gxd)                                   # (the data gradient reads gy and w only)
    _same_or_close(gw, gwd, geo, geod, TOL, "gw", flushed_once(cout, cin))


@pytest.mark.parametrize("tail", [0, 2, 1], ids=["stride%4==0-bit-equal", "stride%4==2-bit-equal", "odd-stride-bit-equal"])
def test_conv3x3_wgrad_bf16_batch_strides(tail):
    """The plain bf16 kernel has one staging form (vx = 0 for every stride): the dense launch has the same geometry throughout."""
    sx, dx, dgy, geo, geod, _, _, gw_bf, x, gy = _wgrad_stride_case(1, 24, tail)
    assert geo[0] == 2 and geo[2] == 0 and geod == geo, (geo, geod)
    gw, gb = conv_wgrad(1, sx, dgy, 72)
    e, eb = relerr(gw, gw_bf), relerr(gb, gy.bfloat16().double().sum(dim=(0, 2, 3)))
    print("gw against the gradient of the bf16-rounded operands: rel-L2 %.3g; gb %.3g" % (e, eb))
    assert e < TOL and eb < 1e-5, (e, eb)                         # (gb: the bar of test_conv3x3_wgrad_bf16)
    gwd, _ = conv_wgrad(1, dx, dgy, 72)
    _same_or_close(gw, gwd, geo, geod, TOL, "gw")


@pytest.mark.parametrize("cin", [24, 40], ids=["cin24", "cin40"])
@pytest.mark.parametrize("tail,vx", STRIDES, ids=["vx4-bit-equal", "vx2-dense-differs-bar", "scalar-dense-differs-bar"])
def test_conv3x3_wgrad_split3_batch_strides(tail, vx, cin):
    """The exact 3-way split: vector staging (float4 / float2) or the scalar-staging kernel by the stride (DVSR_WGRAD_S3V=0: the
    scalar-staging kernel for every stride)."""
    sx, dx, dgy, geo, geod, gw_ref, gb_ref, _, x, gy = _wgrad_stride_case(2, cin, tail)
    assert geo[2] == vx and geod[2] == 4, (geo, geod)
    assert geo[0] in (3, 4, 5) and (geo[0] == 3) == (vx == 0 or os.environ.get("DVSR_WGRAD_S3V", "1")[0] == "0"), geo
    gw, gb = conv_wgrad(2, sx, dgy, 72)
    e, eb = relerr(gw, gw_ref), relerr(gb, gb_ref)
    print("gw: rel-L2 %.3g; gb %.3g" % (e, eb))
    assert e < TOL_SPLIT and eb < TOL_SPLIT, (e, eb)
    gwd, _ = conv_wgrad(2, dx, dgy, 72)
    _same_or_close(gw, gwd, geo, geod, TOL_SPLIT, "gw")


@pytest.mark.parametrize("env", [{"DVSR_WGRAD_S3_KYS_BELOW": "0"}, {"DVSR_WGRAD_S3_KYS_BELOW": "0", "DVSR_WGRAD_S3W": "0"},
                                 {"DVSR_WGRAD_S3V": "0"}, {"DVSR_WGRAD_S3_WGS": "96"}],
                         ids=["eight_waves", "four_waves", "round4_schedule", "row_split_96_workgroups"])
def test_conv3x3_wgrad_split3_batch_strides_other_schedules(env):
    """By default these small shapes run the row-split form of the vector-staging kernel.  The same cases on the forms
    test_gpu_ops.test_conv3x3_wgrad_split3_other_schedules names (that test collects its own file only).  The switches are read
    once per process: each runs in a child."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "test_conv3x3_wgrad_split3_batch_strides and not other_schedules"],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    assert " passed" in r.stdout


# ---- backward of a two-input conv, both inputs strided slices -----------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 1], ids=["strides%4==0-bit-equal", "odd-strides-dense-differs-bar"])
def test_conv2d_backward_two_input_views(tail):
    """gx0, gx1, gw over both channel ranges (the second input's at c_off = c0) and gb; 6x36: two tile columns, 12 tiles; every
    (cout, cin) block populated on both sides (flushed_once everywhere)."""
    n, c0, c1, cout, h, w = 2, 48, 40, 104, 6, 36
    assert bool(flushed_once(cout, c0).all()) and bool(flushed_once(cout, c1).all())
    x, wt, gy, _, gx_ref, gw_ref, gb_ref, _ = _backward_operands(n, c0 + c1, cout, h, w, 3, 1)
    x0, x1 = x[:, :c0].contiguous(), x[:, c0:].contiguous()
    s0, s1, dw, dgy = slice_of(x0, 16, tail), slice_of(x1, 8, tail), wt.cuda(), gy.cuda()
    geos = [(_wgrad_geo(s, dgy, cout, 3, 1, 0), _wgrad_geo(dn, dgy, cout, 3, 1, 0)) for s, dn in ((s0, x0.cuda()), (s1, x1.cuda()))]
    print("geometries (strided, dense) per input: %s" % geos)
    assert all(g[0] == 1 and g[2] == (0 if tail else 4) and gd[2] == 4 for g, gd in geos), geos
    gx0, gx1, gw, gb = conv_backward(s0, s1, dw, dgy, 3, 1)
    _check(gx0, gx_ref[:, :c0], TOL, what="gx0")
    _check(gx1, gx_ref[:, c0:], TOL, what="gx1")
    for name, got, ref in (("gw[:, :c0]", gw[:, :c0], gw_ref[:, :c0]), ("gw[:, c0:]", gw[:, c0:], gw_ref[:, c0:]), ("gb", gb, gb_ref)):
        e = relerr(got, ref)
        print("%s: rel-L2 %.3g" % (name, e))
        assert e < TOL, (name, e)
    d0, d1, gwd, _ = conv_backward(x0.cuda(), x1.cuda(), dw, dgy, 3, 1)
    assert torch.equal(gx0, d0) and torch.equal(gx1, d1)
    _same_or_close(gw[:, :c0], gwd[:, :c0], geos[0][0], geos[0][1], TOL, "gw[:, :c0]")
    _same_or_close(gw[:, c0:], gwd[:, c0:], geos[1][0], geos[1][1], TOL, "gw[:, c0:]")


# ---- stride 2 at odd sizes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,h,w,strided", [(16, 24, 11, 13, False), (16, 24, 12, 13, False), (16, 24, 11, 14, False),
                                                  (64, 64, 11, 13, False), (16, 24, 11, 13, True)],
                         ids=["11x13", "12x13", "11x14", "11x13-64-64", "11x13-strided-x0"])
def test_conv3x3_stride2_odd_sizes(cin, cout, h, w, strided):
    """With odd H or W the zero-dilated view of the data gradient ends exactly at the image edge and the last window of the simple
    weight-gradient kernel sits on the border.  Forward, data, weight and bias gradient against F.conv2d(..., 2, 1) in fp64."""
    n = 2
    x, wt, gy, y_ref, gx_ref, gw_ref, gb_ref, _ = _backward_operands(n, cin, cout, h, w, 3, 2)
    assert tuple(y_ref.shape[2:]) == ((h + 1) // 2, (w + 1) // 2)
    dw, dgy = wt.cuda(), gy.cuda()
    sx = slice_of(x, 16) if strided else x.cuda()
    y, _ = conv_forward("plain", sx, None, dw, None, None, cout, 3, 2, 0, 0, 1)
    _check(y, y_ref, TOL)
    geo = _wgrad_geo(sx, dgy, cout, 3, 2, 0)
    assert geo[0] == 0, geo                                        # the simple fp32 kernel
    gx, _, gw, gb = conv_backward(sx, None, dw, dgy, 3, 2)
    _check(gx, gx_ref, TOL, what="gx")
    for name, got, ref in (("gw", gw, gw_ref), ("gb", gb, gb_ref)):
        e = relerr(got, ref)
        print("%s: rel-L2 %.3g" % (name, e))
        assert e < TOL, (name, e)
    if strided:
        dx = x.cuda()
        geod = _wgrad_geo(dx, dgy, cout, 3, 2, 0)
        assert geod == geo, (geo, geod)
        yd, _ = conv_forward("plain", dx, None, dw, None, None, cout, 3, 2, 0, 0, 1)
        gxd, _, gwd, _ = conv_backward(dx, None, dw, dgy, 3, 2)
        assert torch.equal(y, yd) and torch.equal(gx, gxd) and torch.equal(gw, gwd)
