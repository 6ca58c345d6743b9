"""GPU: the region forms of the Charbonnier loss and of the L1 tail of the inner step (csrc/misc.hip,
dvsr_charbonnier_region_* / dvsr_l1_tail_region_*): the loss over the top-left h x w of every [H, W] plane.  They walk the
region in the row-major order of the cropped tensor with the grid, stride and reduction of the existing kernels, so every
comparison with those kernels on a contiguous copy of the crop is bit for bit."""
import pytest
import torch

from conftest import relerr

pytestmark = pytest.mark.gpu

# [groups, planes, H, W], (h, w)
CASES = [((2, 3, 32, 48), (30, 44)),
         ((2, 15, 8, 12), (8, 11)),
         ((1, 3, 5, 7), (3, 5)),          # W not a multiple of 4
         ((1, 3, 5, 7), (1, 1)),
         ((1, 3, 5, 7), (5, 7)),          # the whole plane
         ((3, 3, 17, 19), (17, 1)),
         # Sizes at which a thread takes MORE than one element, so that the carried (plane, row, column) position is advanced
         # by the grid's stride and its row and plane carries run.  The forwards launch at most 1024 blocks of 256 per group:
         # n > 262144.  The backwards launch at most 4096 blocks: the one-column kernel (W % 4 != 0) wraps for
         # planes H W > 2^20, the four-column kernel (W % 4 == 0) for planes H W / 4 > 2^20; w % 4 != 0 there puts a quad
         # across the region's right edge.
         ((2, 3, 300, 484), (270, 479)),          # forward: n = 387990, 2 elements per thread (a 270 x 480-class frame)
         ((1, 3, 600, 601), (555, 598)),          # one-column backward: 1081800 > 2^20; forward: 4 elements per thread
         ((1, 5, 900, 1000), (801, 997))]         # four-column backward: 1125000 quads > 2^20; forward: 16 per thread
IDS = ["%s-%dx%d" % ("x".join(map(str, s)), r[0], r[1]) for s, r in CASES]
EPS, WEIGHT = 1e-6, 10.0


def _operands(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    x, y = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    base, gl = torch.rand(shape[0], generator=g), torch.rand(shape[0], generator=g) + 0.5
    return x.cuda(), y.cuda(), base.cuda(), gl.cuda()


def _ws(L, k):
    return torch.empty(k * int(L.lib().dvsr_charbonnier_workspace_bytes()), dtype=torch.uint8, device="cuda")


def _region_forward(L, kind, x, y, base, region):
    k, planes, H, W = x.shape
    h, w = region
    ws, loss = _ws(L, k), torch.full((k,), float("nan"), device="cuda")
    if kind == "charbonnier":
        L.check(L.lib().dvsr_charbonnier_region_forward(L.ptr(x), L.ptr(y), loss.data_ptr(), k, planes, H, W, h, w, EPS,
                                                        ws.data_ptr(), ws.numel(), L.stream()), kind)
    else:
        L.check(L.lib().dvsr_l1_tail_region_forward(L.ptr(x), L.ptr(y), base.data_ptr(), WEIGHT, loss.data_ptr(), k, planes, H, W,
                                                    h, w, ws.data_ptr(), ws.numel(), L.stream()), kind)
    return loss


def _region_backward(L, kind, x, y, gl, region):
    """Through the C ABI into a gx that is NaN everywhere: the functions must write every element."""
    k, planes, H, W = x.shape
    h, w = region
    gx = torch.full_like(x, float("nan"))
    if kind == "charbonnier":
        L.check(L.lib().dvsr_charbonnier_region_backward(L.ptr(x), L.ptr(y), gl.data_ptr(), L.ptr(gx), k, planes, H, W, h, w, EPS,
                                                         L.stream()), kind)
    else:
        L.check(L.lib().dvsr_l1_tail_region_backward(L.ptr(x), L.ptr(y), gl.data_ptr(), WEIGHT, L.ptr(gx), k, planes, H, W, h, w,
                                                     L.stream()), kind)
    return gx


def _crop_backward(L, kind, xc, yc, gl):
    k = xc.shape[0]
    gx = torch.full_like(xc, float("nan"))
    if kind == "charbonnier":
        L.check(L.lib().dvsr_charbonnier_backward_grouped(L.ptr(xc), L.ptr(yc), gl.data_ptr(), L.ptr(gx), xc.numel() // k, k, EPS,
                                                          L.stream()), kind)
    else:
        L.check(L.lib().dvsr_l1_tail_backward_grouped(L.ptr(xc), L.ptr(yc), gl.data_ptr(), WEIGHT, L.ptr(gx), xc.numel() // k, k,
                                                      L.stream()), kind)
    return gx


@pytest.mark.parametrize("shape,region", CASES, ids=IDS)
def test_region_forward_is_the_existing_loss_of_the_crop(shape, region):
    """(a) bit-equal to the existing per-sample functions on x[..., :h, :w].contiguous(), through the C ABI and through
    hipops; within 1e-5 (the project's loss bar) of the float64 composition."""
    from dynavsr_amd import _lib as L, hipops
    x, y, base, _ = _operands(shape)
    h, w = region
    xc, yc = x[..., :h, :w].contiguous(), y[..., :h, :w].contiguous()
    d = xc.double() - yc.double()
    want = {"charbonnier": (hipops.charbonnier_per_sample(xc, yc, EPS), torch.sqrt(d * d + EPS).mean(dim=(1, 2, 3))),
            "l1_tail": (hipops.inner_loss_per_sample(base, xc, yc, WEIGHT), base.double() + WEIGHT * d.abs().mean(dim=(1, 2, 3)))}
    got = {"charbonnier": hipops.charbonnier_region(x, y, region, EPS, per_sample=True),
           "l1_tail": hipops.inner_loss_region(base, x, y, region, WEIGHT, per_sample=True)}
    for kind in ("charbonnier", "l1_tail"):
        raw = _region_forward(L, kind, x, y, base, region)
        print(kind, shape, region, raw.tolist(), want[kind][0].tolist(), want[kind][1].tolist())
        assert torch.equal(raw, want[kind][0]), kind
        assert torch.equal(got[kind], want[kind][0]), kind
        assert float(((raw.double() - want[kind][1]).abs() / want[kind][1].abs()).max()) < 1e-5, kind
    if shape[0] == 1:            # the scalar forms: groups = 1
        assert torch.equal(hipops.charbonnier_region(x, y, region, EPS), hipops.charbonnier(xc, yc, EPS))
        assert torch.equal(hipops.inner_loss_region(base[0], x, y, region, WEIGHT), hipops.inner_loss(base[0], xc, yc, WEIGHT))


@pytest.mark.parametrize("shape,region", CASES, ids=IDS)
def test_region_backward_writes_every_element(shape, region):
    """(b) gx pre-filled with NaN: inside the region bit-equal to the existing backward on the contiguous crop, outside exactly
    0, no NaN left.  (c) elements with x == y give an L1 gradient of 0."""
    from dynavsr_amd import _lib as L
    x, y, _, gl = _operands(shape, seed=1)
    h, w = region
    y[..., 0, 0] = x[..., 0, 0]                  # d = 0 inside every region
    y[..., ::2, ::3] = x[..., ::2, ::3]
    xc, yc = x[..., :h, :w].contiguous(), y[..., :h, :w].contiguous()
    inside = torch.zeros(shape, dtype=torch.bool, device="cuda")
    inside[..., :h, :w] = True
    for kind in ("charbonnier", "l1_tail"):
        gx = _region_backward(L, kind, x, y, gl, region)
        assert not torch.isnan(gx).any(), kind
        assert torch.equal(gx[..., :h, :w], _crop_backward(L, kind, xc, yc, gl)), kind
        assert torch.equal(gx[~inside], torch.zeros_like(gx[~inside])), kind
        assert int((gx[~inside] != 0).sum()) == 0
    gx = _region_backward(L, "l1_tail", x, y, gl, region)
    assert torch.equal(gx[x == y], torch.zeros_like(gx[x == y]))
    n = shape[1] * h * w
    nz = gx[inside & (x != y)].reshape(-1)
    if nz.numel():                               # everywhere else the magnitude is grad_loss * weight / n of the element's group
        per_group = (gl * (WEIGHT / n)).reshape(-1, 1, 1, 1).expand(shape)[inside & (x != y)]
        assert relerr(nz.abs(), per_group) < 1e-6


def test_region_backward_of_operands_that_are_not_16_byte_aligned():
    """W a multiple of 4 takes four columns per thread with 16-byte accesses -- when the operands are aligned.  Operands one
    float off a 16-byte boundary take the one-column kernel: same bits."""
    from dynavsr_amd import _lib as L
    shape, region = (2, 3, 8, 12), (7, 10)
    x, y, _, gl = _operands(shape, seed=4)
    n = x.numel()

    def off(t):
        buf = torch.empty(n + 4, device="cuda")
        v = buf[1:n + 1].view(shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    for kind in ("charbonnier", "l1_tail"):
        want = _region_backward(L, kind, x, y, gl, region)
        assert want.data_ptr() % 16 == 0
        xo, yo = off(x), off(y)
        k, planes, H, W = shape
        gx = off(torch.full_like(x, float("nan")))
        if kind == "charbonnier":
            L.check(L.lib().dvsr_charbonnier_region_backward(L.ptr(xo), L.ptr(yo), gl.data_ptr(), L.ptr(gx), k, planes, H, W,
                                                             region[0], region[1], EPS, L.stream()), kind)
        else:
            L.check(L.lib().dvsr_l1_tail_region_backward(L.ptr(xo), L.ptr(yo), gl.data_ptr(), WEIGHT, L.ptr(gx), k, planes, H, W,
                                                         region[0], region[1], L.stream()), kind)
        assert torch.equal(gx, want), kind


def test_region_autograd_matches_the_c_abi():
    """hipops.charbonnier_region / inner_loss_region as autograd functions: the gradients are the C ABI's, that of the target
    is the negative, the base's passes through."""
    from dynavsr_amd import _lib as L, hipops
    shape, region = (2, 3, 32, 48), (30, 44)
    x, y, base, gl = _operands(shape, seed=2)
    xr, yr, br = x.clone().requires_grad_(), y.clone().requires_grad_(), base.clone().requires_grad_()
    loss = hipops.charbonnier_region(xr, yr, region, EPS, per_sample=True)
    loss.backward(gl)
    want = _region_backward(L, "charbonnier", x, y, gl, region)
    assert torch.equal(xr.grad, want) and torch.equal(yr.grad, -want)
    xr.grad = yr.grad = None
    loss = hipops.inner_loss_region(br, xr, yr, region, WEIGHT, per_sample=True)
    loss.backward(gl)
    want = _region_backward(L, "l1_tail", x, y, gl, region)
    assert torch.equal(xr.grad, want) and torch.equal(yr.grad, -want) and torch.equal(br.grad, gl)


def test_whole_region_takes_the_existing_entry_points():
    """(d) region == (H, W): the existing functions are called -- their autograd nodes, their bits -- and no region launch."""
    from dynavsr_amd import hipops
    x, y, base, _ = _operands((2, 3, 8, 12), seed=3)
    x.requires_grad_()
    for per_sample in (False, True):
        b = base if per_sample else base[0]
        c = hipops.charbonnier_region(x, y, (8, 12), EPS, per_sample=per_sample)
        t = hipops.inner_loss_region(b, x, y, (8, 12), WEIGHT, per_sample=per_sample)
        assert "Region" not in type(c.grad_fn).__name__ and "Region" not in type(t.grad_fn).__name__
        assert torch.equal(c, (hipops.charbonnier_per_sample if per_sample else hipops.charbonnier)(x, y, EPS))
        assert torch.equal(t, (hipops.inner_loss_per_sample if per_sample else hipops.inner_loss)(b, x, y, WEIGHT))
    part = hipops.charbonnier_region(x, y, (8, 11), EPS)
    assert "Region" in type(part.grad_fn).__name__
    for bad in ((0, 4), (9, 12), (8, 13), (8,), "8x12", (8.0, 12)):
        with pytest.raises(ValueError):
            hipops.charbonnier_region(x, y, bad)
