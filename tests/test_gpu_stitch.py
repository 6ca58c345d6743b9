"""GPU: frames in overlapping tiles (csrc/frame_stitch.hip, frames.stitch, adapt.super_resolve_frames(tile=...)).

Bars:
  kernel   the bits of the same loop in torch (stitch_ref.stitch_torch) on the library's own table: the products and sums are the
           same fp32 operations in the same order, never contracted.  Compared as integers where the reference is not NaN.
  video    tile=... is bit-identical to the composition of today's calls: per tile super_resolve_frames(out='float') on the video
           of that tile's view, the tiles stitched with torch, then frames.emit -- every launch is deterministic and the
           composition issues the same ones on the same data.
  oracle   rel-L2 < 2e-4 and max-abs < 1e-3 (the forward parity bar, test_gpu_stream.py) against the CPU oracle on every tile's
           padded crop, stitched in float64 with the restated weights: a convex combination of outputs that each meet the bar."""
import ctypes

import numpy as np
import pytest
import torch

import stitch_ref as ref
from conftest import relerr
from dynavsr_amd import _lib as L
from dynavsr_amd import adapt, engine, frames, synth
from dynavsr_amd.data.util import index_generation

pytestmark = pytest.mark.gpu

OPT = {'scale': 4, 'network_G': {'which_model_G': 'EDVR', 'nframes': 5}}
SENTINEL = -123.5
GUARD = 512                      # floats in front of and behind a tensor


def ints(x):
    return x.contiguous().view(torch.int32)


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.uint16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return torch.equal(ints(a), ints(b)) if a.dtype == torch.float32 else torch.equal(a, b)


def same_bits_nan_aware(got, want):
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(ints(got)[~nan], ints(want)[~nan])


def guarded(host, fill=SENTINEL):
    n = host.numel()
    buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device='cuda')
    view = buf[GUARD:GUARD + n].view(host.shape)
    view.copy_(host)
    assert view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


# ---- 1: the kernel against the torch loop, inside guard bands ----------------------------------------
# (n_y, n_x, tile_y, tile_x, overlap, scale, planes): 4 x 3 tiles with a 3-way cover on the rows and a large anchored overlap on
# the columns; the same at scale 2 and 1; one tile; no overlap; a row longer than one workgroup's 256 chunks; 3 x 3-way covers
KERNEL_CASES = [(36, 40, 16, 20, 8, 4, 3), (36, 40, 16, 20, 8, 2, 3), (36, 40, 16, 20, 8, 1, 3), (16, 20, 16, 20, 8, 4, 3),
                (32, 40, 16, 20, 0, 4, 2), (32, 300, 32, 160, 16, 4, 1), (36, 36, 16, 16, 8, 2, 5)]


def covering(origins, length, r):
    return [k for k, o in enumerate(origins) if o <= r < o + length]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=str)
def test_kernel_is_the_torch_loop(case):
    n_y, n_x, t_y, t_x, overlap, s, planes = case
    rows, cols = frames.stitch_table(n_y, t_y, overlap, s), frames.stitch_table(n_x, t_x, overlap, s)
    ny, nx = len(rows[0]), len(cols[0])
    Ht, Wt, H, W = s * min(t_y, n_y), s * min(t_x, n_x), s * n_y, s * n_x
    host = torch.from_numpy(ref.data((ny * nx, planes, Ht, Wt), sum(case)))
    # finite data first, every bit compared; whole tiles are poisoned with NaN / inf one at a time further down
    tbuf, tiles = guarded(host)
    before = tbuf.clone()
    dbuf, dst = guarded(torch.zeros((planes, H, W)))
    got = frames.stitch(tiles, ny, nx, rows, cols, out=dst)
    assert got.data_ptr() == dst.data_ptr()
    want = ref.stitch_torch(tiles, ny, nx, rows, cols)
    assert torch.equal(ints(got), ints(want))
    assert guards_intact(dbuf, planes * H * W)                          # nothing in front of or behind dst
    assert torch.equal(ints(tbuf), ints(before))                        # the tiles and their surroundings are only read
    fresh = frames.stitch(tiles, ny, nx, rows, cols)
    assert fresh.shape == (planes, H, W) and torch.equal(ints(fresh), ints(want))
    # where one tile covers, the bits are the tile's
    oy, ox = rows[0].tolist(), cols[0].tolist()
    single = 0
    for r in range(H):
        ky = covering(oy, Ht, r)
        for c in range(0, W, 4):
            kx = covering(ox, Wt, c)
            if len(ky) == 1 and len(kx) == 1:
                t = tiles[ky[0] * nx + kx[0]][:, r - oy[ky[0]], c - ox[kx[0]]:c - ox[kx[0]] + 4]
                assert torch.equal(ints(got[:, r, c:c + 4]), ints(t)), (r, c)
                single += 1
    assert single > 0
    # a tile full of NaN / inf reaches the pixels it covers and no other
    for bad in sorted({0, (ny * nx) // 2, ny * nx - 1}):
        for poison in (float('nan'), float('inf')):
            spoiled = tiles.clone()
            spoiled[bad] = poison
            out = frames.stitch(spoiled, ny, nx, rows, cols)
            iy, ix = divmod(bad, nx)
            inside = torch.zeros((H, W), dtype=torch.bool, device='cuda')
            inside[oy[iy]:oy[iy] + Ht, ox[ix]:ox[ix] + Wt] = True
            assert torch.equal(ints(out[:, ~inside]), ints(want[:, ~inside])), (bad, poison)
            assert not bool(torch.isfinite(out[:, inside]).any()), (bad, poison)
            assert same_bits_nan_aware(out, ref.stitch_torch(spoiled, ny, nx, rows, cols))


def test_five_dimensional_tiles_and_a_foreign_table():
    """tiles [n, 1, 3, Ht, Wt] are planes = 3; a table that is not the library's (weights that do not sum to 1, a first tile that
    does not cover) gives the picture the formula gives, clamped -- and no access outside the tensors."""
    rows, cols = frames.stitch_table(36, 16, 8, 2), frames.stitch_table(40, 20, 8, 2)
    ny, nx = 4, 3
    tiles = torch.from_numpy(ref.data((ny * nx, 1, 3, 32, 40), 5)).cuda()
    want = ref.stitch_torch(tiles.view(ny * nx, 3, 32, 40), ny, nx, rows, cols)
    assert torch.equal(frames.stitch(tiles, ny, nx, rows, cols), want[None])
    rs = np.random.RandomState(9)
    odd_rows = (rows[0], torch.from_numpy(rs.randint(0, ny, rows[1].shape).astype(np.int32)),
                torch.from_numpy((rs.uniform(0, 1, rows[2].shape) * (rs.uniform(0, 1, rows[2].shape) > 0.3)).astype(np.float32)))
    odd_cols = (cols[0], torch.from_numpy(rs.randint(0, nx, cols[1].shape).astype(np.int32)),
                torch.from_numpy((rs.uniform(0, 1, cols[2].shape) * (rs.uniform(0, 1, cols[2].shape) > 0.3)).astype(np.float32)))
    dbuf, dst = guarded(torch.zeros((3, 72, 80)))
    got = frames.stitch(tiles.view(ny * nx, 3, 32, 40), ny, nx, odd_rows, odd_cols, out=dst)
    assert torch.equal(ints(got), ints(ref.stitch_torch(tiles.view(ny * nx, 3, 32, 40), ny, nx, odd_rows, odd_cols)))
    assert guards_intact(dbuf, 3 * 72 * 80)


# ---- 2: rejections, nothing launched -----------------------------------------------------------------
def test_rejections_at_the_c_abi():
    l = L.lib()
    rows, cols = frames.stitch_table(36, 16, 8, 1), frames.stitch_table(40, 20, 8, 1)
    ny, nx, Ht, Wt, H, W = 4, 3, 16, 20, 36, 40
    tiles = torch.full((ny * nx, 3, Ht, Wt), 1.0, device='cuda')
    dst = torch.full((3, H, W), 7.0, device='cuda')
    (_, ar, oy), (_, ac, ox) = frames._stitch_axis(rows, tiles.device), frames._stitch_axis(cols, tiles.device)
    torch.cuda.synchronize()
    st, inv = L.stream(), -1

    def call(t=tiles.data_ptr(), d=dst.data_ptr(), ny=ny, nx=nx, planes=3, Ht=Ht, Wt=Wt, H=H, W=W, r=ar, c=ac, oy=oy, ox=ox):
        return l.dvsr_frame_stitch(t, ny, nx, planes, Ht, Wt, d, H, W, ctypes.byref(r) if r is not None else None,
                                   ctypes.byref(c) if c is not None else None, oy, ox, st)

    def axis(like, **kw):
        a = L.StitchAxis(like.first, like.weights, like.origins, like.cover)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    Ints = ctypes.c_int
    assert call(t=None) == inv and call(d=None) == inv and call(r=None) == inv and call(c=None) == inv
    assert call(oy=None) == inv and call(ox=None) == inv
    assert call(t=tiles.data_ptr() + 4) == inv and call(d=dst.data_ptr() + 4) == inv            # misaligned
    for kw in (dict(ny=0), dict(nx=0), dict(planes=0), dict(ny=-4), dict(planes=70000), dict(Ht=0), dict(Wt=0), dict(Ht=18),
               dict(Wt=18), dict(H=38), dict(W=42), dict(H=0), dict(W=0)):
        assert call(**kw) == inv, kw
    for k in (0, 4, -1):
        assert call(r=axis(ar, cover=k)) == inv and call(c=axis(ac, cover=k)) == inv, k
    for field in ('first', 'weights', 'origins'):
        assert call(r=axis(ar, **{field: None})) == inv and call(c=axis(ac, **{field: None})) == inv, field
    assert call(c=axis(ac, weights=ac.weights + 4)) == inv and call(r=axis(ar, first=ar.first + 2)) == inv
    # origins inconsistent with H, W, Ht, Wt: a count, a first or a last that does not fit, a gap, an odd origin, an order
    assert call(ny=3) == inv and call(nx=2) == inv and call(H=40) == inv and call(W=44) == inv and call(Ht=20) == inv
    for bad in ([4, 8, 16, 20], [0, 8, 16, 16], [0, 2, 16, 20], [0, 16, 8, 20], [0, 8, 8, 20]):
        assert call(oy=(Ints * 4)(*bad)) == inv, bad
    assert call(ox=(Ints * 3)(0, 0, 20)) == inv
    assert call(ny=2, oy=(Ints * 2)(0, 20)) == inv                                              # a gap: 16 < 20
    assert call(Ht=40) == inv                                                                   # a tile larger than the frame
    both = torch.zeros(ny * nx * 3 * Ht * Wt + 3 * H * W, device='cuda')                        # dst inside / overlapping tiles
    torch.cuda.synchronize()
    assert call(t=both.data_ptr(), d=both.data_ptr()) == inv
    assert call(t=both.data_ptr(), d=both.data_ptr() + 4 * (ny * nx * 3 * Ht * Wt) - 16) == inv
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()) and bool((tiles == 1.0).all()) and not bool(both.any())     # nothing was launched
    assert call(t=both.data_ptr(), d=both.data_ptr() + 4 * (ny * nx * 3 * Ht * Wt)) == 0        # adjacent is fine
    assert call() == 0                                                                          # and the good call works
    assert torch.equal(ints(dst), ints(ref.stitch_torch(tiles, ny, nx, rows, cols)))
    # the wrapper raises before the GPU call
    for args in ((tiles, 3, 3, rows, cols), (tiles, ny, nx, cols, rows), (tiles[:, :, :, :16], ny, nx, rows, cols),
                 (tiles.double(), ny, nx, rows, cols), (tiles, ny, nx, rows[:2], cols)):
        with pytest.raises(ValueError):
            frames.stitch(*args)
    with pytest.raises(ValueError):
        frames.stitch(tiles, ny, nx, rows, cols, out=torch.zeros((3, H, W + 4), device='cuda'))
    with pytest.raises(ValueError):
        frames.stitch(both[:ny * nx * 3 * Ht * Wt].view(ny * nx, 3, Ht, Wt), ny, nx, rows, cols,
                      out=both[4:4 + 3 * H * W].view(3, H, W))
    with pytest.raises(RuntimeError, match="no CPU path"):
        frames.stitch(tiles.cpu(), ny, nx, rows, cols)


# ---- 3 - 9: the video path, EDVR -----------------------------------------------------------------------
T, H0, W0 = 7, 34, 38                                                  # padded to 36 x 40
TILE, OVERLAP = (16, 20), 8                                            # 4 x 3 tiles
_CASE = {}
_COMPOSED = {}


def run(net, video, **kw):
    kw.setdefault('padding', 'new_info')
    return [sr.clone() if torch.is_tensor(sr) else tuple(p.clone() for p in sr)
            for sr in adapt.super_resolve_frames(OPT, net, video, **kw)]


def case():
    """Computed once and never modified: the tiny EDVR of test_gpu_flip.py and the 8-bit video."""
    if not _CASE:
        from dynavsr_amd.models.archs.EDVR_arch import EDVR
        sd = synth.damp_residual_branch(synth.edvr_state_dict(0), 0.02)
        net = EDVR()
        net.load_state_dict(sd, strict=True)
        u8 = (synth.clip(90 + H0, 1, T, H0, W0)[0] * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # [T,h,w,3]
        _CASE.update(sd=sd, net=net.cuda(), u8=u8, dev=u8.cuda())
    return _CASE


def grid(h, w, tile=TILE, overlap=OVERLAP, multiple=4):
    Hp, Wp = frames.padded_size(h, w, multiple)
    return Hp, Wp, adapt.tile_origins(Hp, tile[0], overlap), adapt.tile_origins(Wp, tile[1], overlap)


def compose(net, video, layout, h, w, key=None, tile=TILE, overlap=OVERLAP, scale=4, opt_run=run, multiple=4, **kw):
    """The composition of today's calls: per tile run(out='float') on the video of the tile's view, stitched by the torch loop
    with the library's own table -> a list of T [3, s Hp, s Wp] tensors (what lies beyond s h x s w is never looked at)."""
    if key is not None and key in _COMPOSED:
        return _COMPOSED[key]
    Hp, Wp, ys, xs = grid(h, w, tile, overlap, multiple)
    th, tw = tile
    n = len(video)
    bufs = [torch.zeros((len(ys) * len(xs), 3, scale * th, scale * tw), device='cuda') for _ in range(n)]
    for iy, y in enumerate(ys):
        for ix, x in enumerate(xs):
            views = [frames.tile_view(video[i], layout, y, x, th, tw) for i in range(n)]
            outs = opt_run(net, views, layout=layout, out='float', **kw)
            for i, o in enumerate(outs):
                vh, vw = min(y + th, h) - y, min(x + tw, w) - x
                assert tuple(o.shape) == (1, 3, scale * vh, scale * vw)
                bufs[i][iy * nx_(xs) + ix, :, :scale * vh, :scale * vw] = o[0]
    rows, cols = frames.stitch_table(Hp, th, overlap, scale), frames.stitch_table(Wp, tw, overlap, scale)
    out = [ref.stitch_torch(b, len(ys), len(xs), rows, cols) for b in bufs]
    if key is not None:
        _COMPOSED[key] = out
    return out


def nx_(xs):
    return len(xs)


def check_frames(got, composed, h, w, out, layout, size=None, what=""):
    assert len(got) == len(composed)
    for i, (g, c) in enumerate(zip(got, composed)):
        want = frames.emit(c, 4 * h, 4 * w, layout, size=size)
        want = want[None] if out == 'float' else want
        if not same_bits(g, want):
            d = (g.double() - want.double()).abs()
            print("%s out %s size %s frame %d: %d values differ, max-abs %.3e" % (what, out, size, i, int((d > 0).sum()), float(d.max())))
        assert same_bits(g, want), (what, out, size, i)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_video_equals_the_composition_of_todays_calls(in_flight):
    c = case()
    net, u8 = c['net'], c['dev']
    composed = compose(net, u8, 'hwc_rgb', H0, W0, key='rgb')
    for size in (None, (100, 118)):
        for out, layout in ((None, 'hwc_rgb'), ('float', 'chw'), ('nv12', 'nv12')):
            got = run(net, u8, in_flight=in_flight, out=out, out_size=size, tile=TILE, tile_overlap=OVERLAP)
            check_frames(got, composed, H0, W0, out, layout, size, "in_flight %d" % in_flight)
    # frames on the CPU cross the bus once and give the same bits
    got = run(net, c['u8'], in_flight=in_flight, out='float', tile=TILE, tile_overlap=OVERLAP)
    check_frames(got, composed, H0, W0, 'float', 'chw', None, "cpu frames")


def test_tile_none_and_a_tile_as_large_as_the_frame_are_todays_bits_and_tiles_differ():
    c = case()
    net, u8 = c['net'], c['dev']
    today = run(net, u8, out='float')
    for kw in (dict(tile=None), dict(tile=(36, 40)), dict(tile=64), dict(tile=(48, 40), tile_overlap=0)):
        got = run(net, u8, out='float', **kw)
        assert all(same_bits(a, b) for a, b in zip(got, today)), kw
    flt = torch.stack([frames.ingest(u8[i], 'hwc_rgb', 4, 'reflect') for i in range(T)])          # float frames, no padding
    today_f = run(net, flt)
    assert all(same_bits(a, b) for a, b in zip(run(net, flt, tile=64), today_f))
    tiled = run(net, u8, out='float', tile=TILE, tile_overlap=OVERLAP)
    assert all(a.shape == b.shape for a, b in zip(tiled, today))
    assert any(not torch.equal(a, b) for a, b in zip(tiled, today))      # the argument does something
    # float frames that need no padding, tiled: [1,3,4H,4W] like today's
    tiled_f = run(net, flt, tile=TILE, tile_overlap=OVERLAP)
    composed = compose(net, flt, 'chw', 36, 40, key='flt')
    check_frames(tiled_f, composed, 36, 40, 'float', 'chw', None, "float frames")


def test_yuv_inputs_through_tile_view():
    c = case()
    net = c['net']
    rs = np.random.RandomState(4)
    nv12 = torch.from_numpy(rs.randint(16, 236, (T, H0 * 3 // 2, W0)).astype(np.uint8)).cuda()
    composed = compose(net, nv12, 'nv12', H0, W0, matrix='bt709')
    for out, layout in ((None, 'nv12'), ('float', 'chw')):
        got = run(net, nv12, layout='nv12', out=out, matrix='bt709', tile=TILE, tile_overlap=OVERLAP)
        assert len(got) == T
        for i in range(T):
            want = frames.emit(composed[i], 4 * H0, 4 * W0, layout, matrix='bt709')
            assert same_bits(got[i], want[None] if out == 'float' else want), (out, i)
    # 16-bit 4:2:2, planar, as a list of plane tuples
    packed = torch.from_numpy(rs.randint(64, 940, (T, 2 * H0, W0)).astype(np.uint16)).cuda()
    planes = [tuple(p.clone() for p in frames.yuv_planes(packed[i], 'i422p10')[0]) for i in range(T)]
    composed = compose(net, planes, 'i422p10', H0, W0)
    for video in (packed, planes):
        got = run(net, video, layout='i422p10', tile=TILE, tile_overlap=OVERLAP, in_flight=1)
        for i in range(T):
            want = frames.emit(composed[i], 4 * H0, 4 * W0, 'i422p10')
            assert got[i].dtype == torch.uint16 and same_bits(got[i], want), i


def test_flip_test_and_scenes():
    c = case()
    net, u8 = c['net'], c['dev']
    composed = compose(net, u8, 'hwc_rgb', H0, W0, flip_test=True)
    for in_flight in (1, 2):
        got = run(net, u8, in_flight=in_flight, out='float', flip_test=True, tile=TILE, tile_overlap=OVERLAP)
        check_frames(got, composed, H0, W0, 'float', 'chw', None, "flip_test in_flight %d" % in_flight)
    plain = compose(net, u8, 'hwc_rgb', H0, W0, key='rgb')
    assert any(not torch.equal(a, b) for a, b in zip(composed, plain))
    # every scene comes out as if it had been passed alone
    kw = dict(padding='replicate', tile=TILE, tile_overlap=OVERLAP)
    for extra in (dict(), dict(out='float', flip_test=True)):
        got = run(net, u8, cuts=[3], **kw, **extra)
        want = run(net, u8[:3], **kw, **extra) + run(net, u8[3:], **kw, **extra)
        assert len(got) == T == len(want) and all(same_bits(a, b) for a, b in zip(got, want)), extra
    composed_cut = compose(net, u8, 'hwc_rgb', H0, W0, padding='replicate', cuts=[3])
    check_frames(run(net, u8, cuts=[3], **kw), composed_cut, H0, W0, None, 'hwc_rgb', None, "cuts")


def test_scores_are_of_the_yielded_frames():
    c = case()
    net, u8 = c['net'], c['dev']
    rs = np.random.RandomState(2)
    for out, size, channel in ((None, None, 'rgb'), ('float', (100, 118), 'y'), ('nv12', None, 'y')):
        oh, ow = size if size is not None else (4 * H0, 4 * W0)
        gt = torch.from_numpy(rs.randint(0, 256, (T, oh, ow, 3)).astype(np.uint8)).cuda()
        scores = torch.zeros((T, 2), dtype=torch.float64, device='cuda')
        got = run(net, u8, out=out, out_size=size, gt=gt, scores=scores, score=channel, crop_border=2, tile=TILE, tile_overlap=OVERLAP)
        same = run(net, u8, out=out, out_size=size, tile=TILE, tile_overlap=OVERLAP)
        olay = {None: 'hwc_rgb', 'float': 'chw', 'nv12': 'nv12'}[out]
        for i in range(T):
            assert same_bits(got[i], same[i])                           # the frames are what they are without gt
            want = frames.score(got[i][0] if out == 'float' else got[i], gt[i], olay, 'hwc_rgb', channel=channel, crop_border=2)
            assert torch.equal(scores[i], want), (out, i)


def test_parity_with_the_cpu_oracle():
    import torch.nn.functional as F
    from oracle import edvr as oedvr
    c = case()
    Hp, Wp, ys, xs = grid(H0, W0)
    th, tw = TILE
    flt = torch.from_numpy(np.ascontiguousarray(np.transpose(c['u8'].numpy().astype(np.float32) / 255., (0, 3, 1, 2))))
    got = run(c['net'], c['dev'], out='float', tile=TILE, tile_overlap=OVERLAP)
    wy, wx = ref.dense_weights(Hp, th, OVERLAP, 4), ref.dense_weights(Wp, tw, OVERLAP, 4)       # float64 [4 Hp, ny], [4 Wp, nx]
    for i in (0, 3):
        win = flt[index_generation(i, T, 5, 'new_info')]
        want = torch.zeros((3, 4 * Hp, 4 * Wp), dtype=torch.float64)
        for iy, y in enumerate(ys):
            for ix, x in enumerate(xs):
                crop = win[:, :, y:min(y + th, H0), x:min(x + tw, W0)]
                crop = F.pad(crop, (0, tw - crop.shape[-1], 0, th - crop.shape[-2]), mode='reflect')[None]
                with torch.no_grad():
                    sr = oedvr.edvr_forward(c['sd'], crop.contiguous())[0].double()
                w2 = torch.from_numpy(wy[4 * y:4 * (y + th), iy])[:, None] * torch.from_numpy(wx[4 * x:4 * (x + tw), ix])[None, :]
                want[:, 4 * y:4 * (y + th), 4 * x:4 * (x + tw)] += w2 * sr
        want = want[None, :, :4 * H0, :4 * W0].float()
        y_ = got[i].cpu()
        e, d = relerr(y_, want), float((y_ - want).abs().max())
        print("tiled frame %d: rel-L2 %.3e max-abs %.3e" % (i, e, d))
        assert e < 2e-4 and d < 1e-3, (i, e, d)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_call_counts(in_flight):
    """A frame size that is this test's alone (30 x 34 bytes, padded to 32 x 36: 3 x 3 tiles), so that the plans it finds are
    those its own calls made."""
    c = case()
    net, u8 = c['net'], c['dev'][:, :30, :34]
    assert grid(30, 34)[2:] == ([0, 8, 16], [0, 12, 16])
    n_t, slots = 9, adapt.stream_slots(5, in_flight, 1)

    def plans(h, w):
        return [p for p in engine._splans.values() if (p.h, p.w) == (h, w)]
    run(net, u8, in_flight=in_flight, tile=TILE, tile_overlap=OVERLAP)
    mine = [p for p in plans(16, 20) if p.slots == n_t * slots]
    assert len(mine) == 1                                               # one plan of the tile's size for all tiles ...
    assert not plans(32, 36)                                            # ... and none of the whole frame's
    before = dict(mine[0].stats)
    others = {id(p): dict(p.stats) for p in engine._splans.values() if p is not mine[0]}
    run(net, u8, in_flight=in_flight, tile=TILE, tile_overlap=OVERLAP)
    assert mine[0].stats['extracted'] - before['extracted'] == n_t * T
    assert mine[0].stats['fused'] - before['fused'] == n_t * T
    assert mine[0].stats['packs'] == before['packs']                    # the second video packs nothing
    assert all(dict(p.stats) == others[id(p)] for p in engine._splans.values() if p is not mine[0])
    assert not plans(32, 36)
    run(net, u8, in_flight=in_flight, flip_test=True, tile=TILE, tile_overlap=OVERLAP)
    wide, = [p for p in plans(16, 20) if p.slots == 4 * n_t * slots]
    assert wide.stats['extracted'] >= 4 * n_t * T and wide.stats['fused'] >= 4 * n_t * T


# ---- 10: other networks ----------------------------------------------------------------------------------
class Mean(torch.nn.Module):
    nframes = 3

    def forward(self, x):
        return x.mean(1)


class Ramp(torch.nn.Module):
    """Not shift-equivariant: adds a ramp along x and y, so a tile's output depends on where the tile starts."""
    nframes = 3

    def forward(self, x):
        rx = torch.arange(x.shape[-1], dtype=torch.float32, device=x.device) * 0.03125
        ry = torch.arange(x.shape[-2], dtype=torch.float32, device=x.device)[:, None] * 0.0078125
        return x.mean(1) * 0.5 + rx + ry


@pytest.mark.parametrize("net", [Mean(), Ramp()], ids=["mean", "ramp"])
def test_other_networks(net):
    opt = {'scale': 1, 'network_G': {'which_model_G': 'DUF', 'nframes': 3}}
    rs = np.random.RandomState(12)
    u8 = torch.from_numpy(rs.randint(0, 256, (5, 30, 34, 3)).astype(np.uint8)).cuda()

    def run1(net_, video, **kw):
        kw.setdefault('multiple', 4)                                    # (what `tile` raises it to)
        return [o.clone() for o in adapt.super_resolve_frames(opt, net_, video, padding='replicate', **kw)]
    composed = compose(net, u8, 'hwc_rgb', 30, 34, scale=1, opt_run=run1, multiple=4)
    for in_flight in (1, 2):
        for out, layout in ((None, 'hwc_rgb'), ('float', 'chw')):
            got = run1(net, u8, in_flight=in_flight, out=out, tile=TILE, tile_overlap=OVERLAP)
            assert len(got) == 5
            for i in range(5):
                want = frames.emit(composed[i], 30, 34, layout)
                assert same_bits(got[i], want[None] if out == 'float' else want), (in_flight, out, i)
    today = run1(net, u8, out='float')
    tiled = run1(net, u8, out='float', tile=TILE, tile_overlap=OVERLAP)
    if isinstance(net, Ramp):
        assert any(not torch.equal(a, b) for a, b in zip(tiled, today))
    assert all(same_bits(a, b) for a, b in zip(run1(net, u8, out='float', tile=64), today))     # one tile: today's bits
