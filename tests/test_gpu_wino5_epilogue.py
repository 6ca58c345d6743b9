"""conv2d_wino5_kernel's epilogue exchange (dynavsr_amd/csrc/wino5_exchange.h): which LDS record a consumer wave writes, which
reader wave picks it up and which cout it becomes.

Every round of the exchange carries register quads of BOTH cout halves, a record holds the four j of one cout, and the reader
of (cout half, register quad, register) is chosen by its wave number -- so a wrong map shows as couts swapped inside a 64-cout
block, as a padded cout stored past Cout, or as a row stored past a cut last tile row.  The cases are the smallest at which
each of those can happen, through the C entry points test_conv3x3_winograd_f4x4 uses, against fp64 torch at its bars
(rel-L2 < 4e-6, max-abs < 5e-5 on O(1) outputs), with both workgroup tile shapes:

  sizes    N in {1, 2}; two chunks as one input (c0 = 16) and as two (c0 = 8, c1 = 8); one tile row block (8 x 64 resp.
           16 x 32 pixels) and H % 4 == 2 (10 x 64, 18 x 32: the last tile row is cut).
  Cout     40 (half 1 live in register quad 0 only), 64, and second cout blocks that hold 8 (72: only unit (0, 0) live),
           24 (88: half 1 all padding -- the offset / mask convs' last block, 216 = 3 x 64 + 24) and 40 (104).
  variants plain with LeakyReLU (eight pair readers), residual and addend (sixteen readers), PixelShuffle(2) (pairs; 64, 72).

conv2_choose gives the kernel no launch with Cout < 32 or fewer than 16 input channels (test_not_eligible_below holds that),
so one chunk and a Cout of 8 or 24 ALONE cannot reach it through these entry points: the 8 and the 24 are run as the live part
of a second 64-cout block, which is the same code path (cbi = 1, co0 < Cout).

Overwrites: the output (and the addend the library computes) lies between NaN guard bands wider than a 64-cout block of planes,
and starts as NaN: a store past the last cout or past the last row of the last plane lands in a band, one past a cut tile row of
any other plane in the next plane's first rows, where it fails the comparison."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import relerr

pytestmark = pytest.mark.gpu

TOL_F4, MAXABS_F4 = 4e-6, 5e-5            # tests/test_gpu_ops.py: test_conv3x3_winograd_f4x4
WINO_F4 = 5                               # geo[3] of dvsr_conv2d_packed_geometry
COUTS = (40, 64, 72, 88, 104)
COUT_MAX = max(COUTS)
CIN = 16                                  # two 8-channel chunks
SIZES = {"2": ((8, 64), (10, 64)), "3": ((16, 32), (18, 32))}   # DVSR_CONV_WINO5 -> (H, W): 8 x 64 resp. 16 x 32-pixel tiles


def rnd(*shape, seed, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    monkeypatch.setenv("DVSR_CONV_WINO", "2")
    monkeypatch.setenv("DVSR_CONV_WINO3", "1")
    monkeypatch.delenv("DVSR_PCD_HOIST", raising=False)


@pytest.fixture(scope="module")
def cases():
    """Operands and un-activated fp64 sums of every size, computed once on the CPU and left unchanged: x (N = 2, 16 channels),
    the addend's input xr (one image of 16 channels, shared by both batch items), weights for COUT_MAX couts (a smaller Cout
    takes the first rows), bias, residual."""
    out = {}
    for sizes in SIZES.values():
        for h, w in sizes:
            x, xr = rnd(2, CIN, h, w, seed=1), rnd(1, CIN, h, w, seed=6)
            wt = rnd(COUT_MAX, CIN, 3, 3, seed=2, scale=1 / np.sqrt(CIN * 9))
            wr = rnd(COUT_MAX, CIN, 3, 3, seed=7, scale=1 / np.sqrt(CIN * 9))
            b = rnd(COUT_MAX, seed=3, scale=0.1)
            r = rnd(2, COUT_MAX, h, w, seed=4)
            out[h, w] = dict(x=x, xr=xr, wt=wt, wr=wr, b=b, r=r,
                             conv=F.conv2d(x.double(), wt.double(), b.double(), 1, 1),
                             conv_r=F.conv2d(xr.double(), wr.double(), None, 1, 1))
    return out


def guarded(shape, band):
    """A NaN buffer [band | tensor of `shape` | band]; returns (buffer, the tensor's view)."""
    numel = int(np.prod(shape))
    buf = torch.full((band + numel + band,), float("nan"), device="cuda")
    return buf, buf[band:band + numel].view(shape)


def bands_untouched(buf, band):
    return bool(torch.isnan(buf[:band]).all()) and bool(torch.isnan(buf[-band:]).all())


def launch(L, x0, x1, wt, b, res, y, cout, act, ps, mode, pre=None, pre_bdiv=0):
    n, c0, h, w = x0.shape
    c1 = 0 if x1 is None else x1.shape[1]
    d = L.Conv2dDesc(L.ptr(x0), L.ptr(x1), L.ptr(wt), L.ptr(b), L.ptr(res), L.ptr(y), n, c0, c1, h, w, cout, 3, 1, 1, act, ps, 1, 0, 0,
                     pre, pre_bdiv)
    geo = (ctypes.c_int * 4)()
    L.check(L.lib().dvsr_conv2d_packed_geometry(d, ctypes.byref(geo)), "dvsr_conv2d_packed_geometry")
    assert list(geo)[3] == WINO_F4 and list(geo)[1] == (8 if mode == "2" else 16), list(geo)
    ws = torch.empty(max(int(L.lib().dvsr_conv2d_packed_workspace_bytes(d)), 16), dtype=torch.uint8, device="cuda")
    L.check(L.lib().dvsr_conv2d_forward_packed(d, ws.data_ptr(), ws.numel(), L.stream()), "dvsr_conv2d_forward_packed")
    torch.cuda.synchronize()


@pytest.mark.parametrize("variant", ["plain", "residual", "pixelshuffle", "addend"])
@pytest.mark.parametrize("mode", ["2", "3"])
def test_exchange_remap(mode, variant, cases, monkeypatch):
    from dynavsr_amd import _lib as L
    monkeypatch.setenv("DVSR_CONV_WINO5", mode)
    ps = 2 if variant == "pixelshuffle" else 0
    worst = (0.0, 0.0)
    for h, w in SIZES[mode]:
        c = cases[h, w]
        band = 64 * h * w + 256                                   # more than a whole 64-cout block of planes
        for n in (1, 2):
            for split in (False, True):                           # c0 = 16 | c0 = 8 + c1 = 8
                x = c["x"][:n].cuda()
                x0, x1 = (x[:, :8].contiguous(), x[:, 8:].contiguous()) if split else (x, None)
                for cout in ((64, 72) if ps else COUTS):
                    wt, b = c["wt"][:cout].cuda(), c["b"][:cout].cuda()
                    ref = c["conv"][:n, :cout]
                    res = pre = None
                    if variant == "addend":
                        # the library's own reference-part launch (no bias, no activation) into a guarded buffer; both batch
                        # items share it (pre_bdiv = n)
                        pbuf, pre_t = guarded((1, cout, h, w), band)
                        launch(L, c["xr"].cuda(), None, c["wr"][:cout].cuda(), None, None, pre_t, cout, 0, 0, mode)
                        assert bool(torch.isfinite(pre_t).all()) and bands_untouched(pbuf, band)
                        pre = pre_t.data_ptr()
                        ref = ref + c["conv_r"][:, :cout]
                    ref = F.leaky_relu(ref, 0.1)
                    if variant == "residual":
                        res = c["r"][:n, :cout].contiguous().cuda()
                        ref = ref + c["r"][:n, :cout].double()
                    if ps:
                        ref = F.pixel_shuffle(ref, 2)
                    ybuf, y = guarded(tuple(ref.shape), band)
                    launch(L, x0, x1, wt, b, res, y, cout, 1, ps, mode, pre=pre, pre_bdiv=n if pre else 0)
                    what = "%s mode %s %dx%d n %d split %d cout %d" % (variant, mode, h, w, n, split, cout)
                    assert bands_untouched(ybuf, band), what + ": a store outside the output"
                    assert bool(torch.isfinite(y).all()), what + ": an output was not stored"
                    if variant == "addend":
                        assert bands_untouched(pbuf, band), what
                    e, m = relerr(y, ref), float((y.cpu().double() - ref).abs().max())
                    worst = (max(worst[0], e), max(worst[1], m))
                    assert e < TOL_F4 and m < MAXABS_F4, (what, e, m)
    print("%s mode %s: worst rel-L2 %.2e, max-abs %.2e" % (variant, mode, worst[0], worst[1]))


def test_not_eligible_below(monkeypatch):
    """Why no case above has one chunk, or a Cout of 8 or 24 alone: with DVSR_CONV_WINO5=2 ("wherever it is eligible") those
    launches are still not given to the F(4x4) kernel."""
    from dynavsr_amd import _lib as L
    monkeypatch.setenv("DVSR_CONV_WINO5", "2")

    def kernel_of(c0, cout):
        x = torch.zeros(1, c0, 8, 64, device="cuda")
        wt = torch.zeros(cout, c0, 3, 3, device="cuda")
        y = torch.zeros(1, cout, 8, 64, device="cuda")
        d = L.Conv2dDesc(L.ptr(x), None, L.ptr(wt), None, None, L.ptr(y), 1, c0, 0, 8, 64, cout, 3, 1, 1, 1, 0, 1, 0, 0)
        geo = (ctypes.c_int * 4)()
        L.check(L.lib().dvsr_conv2d_packed_geometry(d, ctypes.byref(geo)), "dvsr_conv2d_packed_geometry")
        return list(geo)[3]

    assert kernel_of(16, 40) == WINO_F4
    assert kernel_of(8, 64) != WINO_F4 and kernel_of(16, 8) != WINO_F4 and kernel_of(16, 24) != WINO_F4
